"""The band scanner on the GPU (include/ext/mercury_scanner.h, mercury_amd.BandScanner): every line and every report against the normative
host twin, byte for byte, at the smallest N, the largest (the LDS ceiling) and one between, with one and with three blocks per line;
every format from host and device memory; chunk invariance and seeks; a large position; the decision edges; three links end to end
through BandScanner.plan; memory.

The block kernel runs N / 4 groups on min(N / 4, 256) threads: N = 256 has one group per thread on a single wavefront, N = 1024 one on
four, N = 4096 four; N = 512 runs the odd-length form (stage 1 alone, then pairs of stages)."""
import numpy as np
import pytest

import scanner_ref as ref
from band_links import iq as make_iq, rx as _rx, torch as _torch
from mercury_amd import SCAN_REPORT_DTYPE, BandScanner, MgpuError, host_scan_process, scan_reports

pytestmark = pytest.mark.gpu
SMALL = dict(edge_bins=5, dc_bins=1, gap=2, min_bins=1, max_runs=32, threshold=3.0)
HAND = dict(log2n=8, blocks_per_line=1, threshold=50.0, edge_bins=8, dc_bins=2, gap=3, min_bins=1, max_runs=32)


def _same(got, want):
    return (got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes() and got[1].shape == want[1].shape
            and got[1].tobytes() == want[1].tobytes())


def _signal(seed, log2n, n, fmt="cf64"):
    """noise with three two-bin tones in it: every line has runs"""
    N = 1 << log2n
    x = make_iq(np.random.default_rng(seed), n, fmt)
    tones = ref.two_bin_tones(log2n, n, [N // 4, N // 4 + 3, 3 * N // 4], 6.0)
    if fmt == "cs16":
        return (x // 8 + np.stack([tones.real, tones.imag], 1) * 4096).astype(np.int16)
    return (x + tones).astype(x.dtype)


def _in_calls(sc, x, blocks):
    """x fed in calls of the given block counts -> (lines, reports) of all calls"""
    lines, reports, at = [], [], 0
    for m in blocks:
        want_n = sc.lines(m * sc.H)
        got_l, got_r = sc.process_raw(x[at * sc.H: (at + m) * sc.H])
        assert len(got_l) == len(got_r) == want_n
        lines.append(got_l)
        reports.append(got_r)
        at += m
    assert at * sc.H == len(x)
    return np.concatenate(lines), np.concatenate(reports)


@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("log2n", [8, 10, 12])
def test_lines_and_reports_equal_the_twin(log2n, A):
    """a first call of 1, 2, A and A + 1 blocks (a lone block, a call that ends inside a line, exactly one line, a line and a block), then
    2 A blocks more, which finish what the first call left: each call's output is the twin's for the stream so far"""
    H = (1 << log2n) // 2
    config = dict(SMALL, log2n=log2n, blocks_per_line=A)
    sc = BandScanner(_rx(), 4, **config)
    for first in sorted({1, 2, A, A + 1}):
        x = _signal(1000 * log2n + 10 * A + first, log2n, (first + 2 * A) * H)
        sc.seek(0)
        got_first = sc.process_raw(x[: first * H])
        assert _same(got_first, host_scan_process(x[: first * H], 4, **config)), (first, "the first call")
        got = _in_calls(sc, x[first * H:], [2 * A])
        want = host_scan_process(x, 4, **config)
        n1 = len(got_first[0])
        assert len(want[0]) == (first + 2 * A) // A and want[1]["n_runs"].min() >= 1
        assert _same((np.concatenate([got_first[0], got[0]]), np.concatenate([got_first[1], got[1]])), want), (first, n1)
        assert sc.status().position == len(x) and sc.status().blocks == first + 2 * A and sc.status().lines == (first + 2 * A) // A
    sc.close()


def test_the_odd_length_form_equals_the_twin():
    """N = 512 and 2048: stage 1 runs alone before the pairs of stages"""
    for log2n in (9, 11):
        config = dict(SMALL, log2n=log2n, blocks_per_line=2)
        x = _signal(log2n, log2n, 5 * (1 << log2n) // 2)
        sc = BandScanner(_rx(), 4, **config)
        assert _same(sc.process_raw(x), host_scan_process(x, 4, **config)), log2n
        sc.close()


@pytest.mark.parametrize("fmt", ["cs16", "cf32", "cf64"])
def test_every_format_from_host_and_device_memory(fmt):
    """CS16 (with both full-scale values in it), CF32 and CF64 through process() from host memory and from a device tensor, and through
    mgpu_scan_process_dev (device in and out) on a stream of the caller's and on the context's"""
    torch = _torch()
    log2n, A = 9, 2
    H = (1 << log2n) // 2
    config = dict(SMALL, log2n=log2n, blocks_per_line=A)
    x = _signal(40 + len(fmt) + ord(fmt[2]), log2n, 5 * H, fmt)
    if fmt == "cs16":
        x[3], x[H + 1], x[4 * H + 7] = (-32768, 32767), (32767, -32768), (-32768, -32768)
    want = host_scan_process(x, 4, **config)
    assert len(want[0]) == 2
    sc = BandScanner(_rx(), 4, **config)
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()                                            # the library works on its own stream
    assert _same(sc.process_raw(x), want)
    sc.seek(0)
    assert _same(sc.process_raw(d_x), want)
    for stream in (torch.cuda.Stream(), None):
        sc.seek(0)
        d_lines = torch.zeros((2, 1 << log2n), dtype=torch.float64, device="cuda")
        d_reports = torch.full((2, SCAN_REPORT_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device="cuda")     # every byte is written
        torch.cuda.synchronize()
        n = sc.process_raw(d_x, d_lines, d_reports, stream=stream.cuda_stream if stream else None)
        if stream:
            stream.synchronize()
        else:
            sc.rx.lib.mgpu_synchronize(sc.rx.h, None)
        assert n == 2
        assert _same((d_lines.cpu().numpy(), d_reports.cpu().numpy().view(SCAN_REPORT_DTYPE).reshape(-1)), want)
    with pytest.raises(MgpuError):
        sc.process_raw(d_x, torch.zeros((1, 1 << log2n), dtype=torch.float64, device="cuda"), d_reports)       # room for one line of two
    sc.close()


def test_chunking_and_seeking_do_not_change_a_line():
    """7 A H samples at A = 3 fed whole, block by block and in an uneven cut give the same bytes; a bad n_in is refused and changes
    nothing; a seek in mid-stream gives a fresh scanner's lines"""
    log2n, A = 10, 3
    H = (1 << log2n) // 2
    config = dict(SMALL, log2n=log2n, blocks_per_line=A)
    x = _signal(77, log2n, 7 * A * H)
    want = host_scan_process(x, 4, **config)
    assert len(want[0]) == 7
    sc = BandScanner(_rx(), 4, **config)
    assert sc.max_in == 256 * H
    assert _same(sc.process_raw(x), want)
    small = BandScanner(_rx(), 4, max_in=7 * H, **config)
    for cut in ([1] * 21, [2, 5, 1, 7, 3, 3], [4, 4, 4, 4, 4, 1]):
        small.seek(0)
        assert _same(_in_calls(small, x, cut), want), cut
    small.seek(0)
    first = small.process_raw(x[: 4 * H])
    for bad in (x[:0], x[: H - 1], x[: H + 1], x[: 8 * H]):            # none, no multiple of H, more than max_in
        assert small.lines(len(bad)) < 0
        with pytest.raises(MgpuError) as e:
            small.process_raw(bad)
        assert e.value.code == 1
    assert small.status().position == 4 * H
    rest = _in_calls(small, x[4 * H:], [7, 7, 3])
    assert _same((np.concatenate([first[0], rest[0]]), np.concatenate([first[1], rest[1]])), want)
    # a seek in the middle of a line forgets the history and the partial line
    for bad in (H, A * H + 1, 2 ** 62 + A * H):
        with pytest.raises(MgpuError):
            small.seek(bad)
    small.seek(5 * A * H)
    assert _same(_in_calls(small, x[: 6 * H], [2, 4]), host_scan_process(x[: 6 * H], 4, position=5 * A * H, **config))
    sc.close(), small.close()


def test_a_large_position():
    log2n, A = 8, 3
    H = (1 << log2n) // 2
    config = dict(SMALL, log2n=log2n, blocks_per_line=A)
    position = 2 ** 40 * H * A
    x = _signal(5, log2n, 7 * H)
    sc = BandScanner(_rx(), 4, **config)
    sc.process_raw(x[: 2 * H])                                          # a history and a partial line to forget
    sc.seek(position)
    got = _in_calls(sc, x, [2, 5])
    want = host_scan_process(x, 4, position=position, **config)
    assert list(want[1]["first_block"]) == [2 ** 40 * A, 2 ** 40 * A + A]
    assert _same(got, want) and sc.status().position == position + 7 * H
    sc.close()


# ---- the decision edges, on lines built as tests/test_scanner_host.py builds them --------------------------------------------------------
def _hand(firsts, x=None, **config):
    config = dict(HAND, **config)
    if x is None:
        x = ref.two_bin_tones(8, 512, firsts) + ref.floor_noise(3, 512)
    sc = BandScanner(_rx(), 4, **config)
    got = sc.process_raw(x)
    sc.close()
    assert _same(got, host_scan_process(x, 4, **config))
    return scan_reports(got[1]), got[0]


def _spans(report):
    return [(r["first"], r["count"]) for r in report["runs"]]


def test_a_nan_line_is_reported_nonfinite():
    """the reports are the twin's byte for byte; so are the lines except that a NaN is a NaN: which one (its sign and payload) is the
    processor's choice, x86's is not gfx950's, and the rule leaves it open"""
    x = ref.two_bin_tones(8, 512, [40]) + ref.floor_noise(3, 512)
    x[300] = complex(np.nan, 0.0)                               # in blocks 2 and 3: lines 2 and 3
    sc = BandScanner(_rx(), 4, **HAND)
    lines, reports = sc.process_raw(x)
    sc.close()
    want_lines, want_reports = host_scan_process(x, 4, **HAND)
    assert reports.tobytes() == want_reports.tobytes()
    assert list(reports["nonfinite"]) == [0, 0, 1, 1] and list(reports["n_runs"][2:]) == [0, 0] and reports["level"][3].tobytes() == bytes(8)
    assert lines[:2].tobytes() == want_lines[:2].tobytes()
    assert np.isnan(lines[2:]).all() and np.isnan(want_lines[2:]).all()


def test_more_runs_than_max_runs():
    reports, _ = _hand([20 + 6 * i for i in range(12)] + [140 + 6 * i for i in range(12)], max_runs=32, gap=0)
    assert reports[-1]["n_runs"] == 24 and reports[-1]["reported"] == 24
    reports, _ = _hand([20 + 6 * i for i in range(12)] + [140 + 6 * i for i in range(12)], max_runs=5, gap=0)
    assert reports[-1]["n_runs"] == 24 and reports[-1]["reported"] == 5 and _spans(reports[-1])[-1] == (44, 2)
    # more runs than a report has room for at all: 40 runs at max_runs = 32
    reports, _ = _hand([10 + 5 * i for i in range(22)] + [135 + 5 * i for i in range(18)], gap=0)
    assert reports[-1]["n_runs"] == 40 and reports[-1]["reported"] == 32


def test_the_exclusions_and_the_gaps():
    assert _spans(_hand([7, 247])[0][-1]) == [(8, 1), (247, 1)]
    assert _spans(_hand([124, 131], gap=8)[0][-1]) == [(124, 2), (131, 2)]
    assert _spans(_hand([124, 131], gap=8, dc_bins=0)[0][-1]) == [(124, 9)]
    assert _spans(_hand([40, 45, 60, 66])[0][-1]) == [(40, 7), (60, 2), (66, 2)]
    assert _spans(_hand([40, 60, 62], min_bins=3)[0][-1]) == [(60, 4)]
    # a gap across a word of the mask (bins 63 | 64) and runs that end and begin on one
    assert _spans(_hand([60, 65, 190, 192], gap=3)[0][-1]) == [(60, 7), (190, 4)]
    assert _spans(_hand([62, 64], gap=0)[0][-1]) == [(62, 4)]


def test_a_bin_exactly_at_threshold_times_level():
    """the threshold is chosen from the twin's own line so that threshold * level is, to the bit, the smaller of a tone's two bins: that
    bin is not occupied (<=), and one unit in the last place less of threshold makes it so. The device decides both as the twin does."""
    x = ref.two_bin_tones(8, 512, [40]) + ref.floor_noise(3, 512)
    lines, reports = host_scan_process(x, 4, **HAND)
    line, level = lines[-1], reports["level"][-1]
    f = 40 if line[40] < line[41] else 41
    t = line[f] / level
    for _ in range(64):                                                 # a threshold whose product with the level is the bin's value
        if t * level == line[f]:
            break
        t = np.nextafter(t, np.inf if t * level < line[f] else 0.0)
    while np.nextafter(t, 0.0) * level == line[f]:                      # the smallest such threshold
        t = np.nextafter(t, 0.0)
    assert t * level == line[f] and np.nextafter(t, 0.0) * level < line[f]
    at, _ = _hand([40], x, threshold=float(t))
    below, _ = _hand([40], x, threshold=float(np.nextafter(t, 0.0)))
    assert _spans(at[-1]) == [(81 - f, 1)] and _spans(below[-1]) == [(40, 2)]


def test_three_links_end_to_end_through_the_plan():
    """tests/test_scanner_host.py's three links at its SNR of 15 dB, on the device: the lines are the twin's, and BandScanner.plan gives
    three channels, each within a bin of its link's offset for the link's own sideband"""
    x = ref.three_links(15.0)
    sc = BandScanner(_rx(), ref.LINK_D)
    got = sc.process_raw(x)
    assert _same(got, host_scan_process(x, ref.LINK_D))
    lines, reports = sc.process(x[: 16 * 2048])                         # the stream goes on: line 2 is not line 0
    assert lines.shape == (1, 4096) and reports[0]["first_block"] == 32
    report = scan_reports(got[1])[-1]
    usb, lsb = sc.plan(report, sideband=0), sc.plan(report, sideband=1)
    assert len(usb) == len(lsb) == 3
    for i, (offset, sideband, _) in enumerate(sorted(ref.LINK_PLAN)):
        found = (lsb if sideband else usb)[i]
        assert found[1] == sideband and found[2] == 1.0 and abs(found[0] - offset) <= 47, (found, offset)
    assert sc.plan(report, min_hz=3000) == []                           # no run is that wide
    sc.close()


def test_create_use_destroy_gives_the_memory_back():
    """50 create / process / destroy cycles (tables, history, workspace, staging, the output buffers) leave the device's free memory
    where it was"""
    import gc
    torch = _torch()

    def free_hbm():
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info()[0]

    rx = _rx()
    x = _signal(6, 12, 17 * 2048)

    def cycle():
        sc = BandScanner(rx, 64)
        sc.process_raw(x)
        return sc

    cycle().close()
    first = free_hbm()
    sc = cycle()
    in_use = first - free_hbm()
    sc.close()
    assert in_use >= 256 * 4096 * 8, in_use                             # the workspace of 256 blocks' powers
    for _ in range(50):
        cycle().close()
    after = free_hbm()
    assert abs(after - first) < 64 << 20, (first, after)

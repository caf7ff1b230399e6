"""The wideband impulse blanker on the GPU (include/ext/mercury_wideband_blanker.h, mercury_amd.WidebandBlanker): output and reports
against the normative host twin, byte for byte, from one flag word per block (B = 64) to the register ceiling (B = 4096: sixteen powers
per lane), with a block that fills no whole workgroup pass (B = 320); every format from host and device memory; the narrowest and the
widest guard; chunk invariance, seeks and refusals; a caller's stream; three links end to end with and without clicks; two contexts;
memory.

The analyse kernel keeps K = 1, 4 or 16 powers per lane: B <= 256, <= 1024, above. B = 64 leaves three of its four wavefronts without a
sample; B = 320 gives the second pass one wavefront."""
import numpy as np
import pytest

import wblank_ref as ref
from band_links import ThreeLinks, last_error, other_rx, rx as _rx, torch as _torch
from block_stage_cases import device_reports, in_calls as _in_calls, join as _join, memory_comes_back, same as _same
from mercury_amd import (WBLANK_REPORT_DTYPE, Channelizer, MgpuError, RxCapture, Synthesizer, WidebandBlanker, host_wblank_process,
                         wblank_reports)
from oraclelib import CARRIER

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("guard", [0, 64])
@pytest.mark.parametrize("B", [64, 256, 320, 4096])
@pytest.mark.parametrize("fmt", ["cs16", "cf32", "cf64"])
def test_output_and_reports_equal_the_twin(fmt, B, guard):
    """wblank_ref.planted, the inputs of tests/test_wideband_blanker_host.py, in one call from host memory and in one from device memory"""
    torch = _torch()
    x = ref.planted(100 + B + guard, B, fmt, B // 8)
    config = dict(block=B, guard=guard)
    want = host_wblank_process(x, 4, **config)
    assert want[1]["capped"].sum() == (1 if fmt == "cs16" else 2) and want[1]["blanked"].sum() > B // 8
    wb = WidebandBlanker(_rx(), 4, fmt, **config)
    assert (wb.B, wb.cap, wb.delay, wb.max_in) == (B, B // 8, B, 1024 * B)
    assert _same(wb.process_raw(x), want)
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()                                            # the library works on its own stream
    wb.seek(0)
    assert _same(wb.process_raw(d_x), want)
    assert wb.status().position == len(x) and wb.status().blocks == ref.PLANTED_BLOCKS
    wb.close()


@pytest.mark.parametrize("fmt,B", [("cf32", 256), ("cs16", 64), ("cf64", 4096)])
def test_chunking_and_seeking_do_not_change_a_byte(fmt, B):
    """two planted streams on end, 24 blocks, at max_in = 8 B: calls of 1, 2, 1, 8 (exactly max_in), 8 and 4 blocks, and block by block,
    give the twin's bytes for the stream fed whole: every planted border case lies on a call's border in one of the cuts. A refused
    n_in changes nothing; a seek in mid-stream gives a fresh stage's output."""
    x = np.concatenate([ref.planted(31, B, fmt, B // 8), ref.planted(32, B, fmt, B // 8)])
    config = dict(block=B, guard=64)
    want = host_wblank_process(x, 4, **config)
    wb = WidebandBlanker(_rx(), 4, fmt, max_in=8 * B, **config)
    assert wb.max_in == 8 * B
    for cut in ([1, 2, 1, 8, 8, 4], [1] * 24, [8, 8, 7, 1]):
        wb.seek(0)
        assert _same(_in_calls(wb, x, cut), want), cut
    wb.seek(0)
    first = wb.process_raw(x[: 4 * B])
    for bad in (x[:0], x[: B - 1], x[: B + 1], x[: 9 * B]):             # none, no multiple of B, more than max_in
        with pytest.raises(MgpuError) as e:
            wb.process_raw(bad)
        assert e.value.code == 1
    assert "n_in must be a positive multiple of B" in last_error(_rx())
    assert wb.status().position == 4 * B
    rest = _in_calls(wb, x[4 * B:], [8, 8, 4])
    assert _same(_join([first, rest]), want)
    for bad in (B // 2, B + 1, 2 ** 62 + B):
        with pytest.raises(MgpuError):
            wb.seek(bad)
    position = (2 ** 62 // B - 6) * B                                   # the call ends on 2^62
    wb.seek(position)
    assert _same(_in_calls(wb, x[: 6 * B], [2, 4]), host_wblank_process(x[: 6 * B], 4, position=position, **config))
    with pytest.raises(MgpuError):
        wb.process_raw(x[:B])                                           # past 2^62
    wb.close()


def test_process_dev_on_a_callers_stream_and_on_the_contexts():
    """device in, device out: the same bytes on a stream of the caller's and on the context's, with and without reports; every byte of
    the output and of the reports is written; an output that overlaps the input is refused"""
    torch = _torch()
    B, fmt = 320, "cf32"
    x = ref.planted(41, B, fmt, B // 8)
    n, m = len(x), ref.PLANTED_BLOCKS
    want = host_wblank_process(x, 4, block=B)
    wb = WidebandBlanker(_rx(), 4, fmt, block=B)
    d_x = torch.from_numpy(x).cuda()
    for stream in (torch.cuda.Stream(), None):
        for with_reports in (True, False):
            wb.seek(0)
            d_out = torch.full((n,), complex(7.0, 7.0), dtype=torch.complex64, device="cuda")
            d_reports = torch.full((m, WBLANK_REPORT_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            half = (m // 2) * B                                             # two calls in a row on the stream, no wait between them
            got = wb.process_raw(d_x[:half], d_out[:half], d_reports[: m // 2] if with_reports else None,
                                 stream=stream.cuda_stream if stream else None)
            got += wb.process_raw(d_x[half:], d_out[half:], d_reports[m // 2:] if with_reports else None,
                                  stream=stream.cuda_stream if stream else None)
            if stream:
                stream.synchronize()
            else:
                wb.rx.lib.mgpu_synchronize(wb.rx.h, None)
            assert got == m
            assert d_out.cpu().numpy().tobytes() == want[0].tobytes()
            if with_reports:
                assert device_reports(d_reports, m, WBLANK_REPORT_DTYPE).tobytes() == want[1].tobytes()
            else:
                assert (d_reports.cpu().numpy() == 0xA5).all()
    with pytest.raises(MgpuError):
        wb.process_raw(d_x[: 2 * B], d_x[B: 3 * B])
    assert "d_out must not overlap d_iq" in last_error(_rx())
    with pytest.raises(MgpuError):
        wb.process_raw(x.astype(np.complex128))                         # not the handle's format
    wb.close()


REFUSALS = [(dict(D=65), "D must be 1..64"), (dict(fmt=5), "unknown IQ format"), (dict(block=96), "block must be a multiple of 64, 64..4096, or 0"),
            (dict(threshold=float("nan")), "threshold must be finite and at least 2"), (dict(guard=65), "guard must be 0..64"),
            (dict(max_share=0.75), "max_share must be in (0, 0.5]"), (dict(max_in=300), "max_in must be a multiple of B, 2^26 at most")]


def test_a_refused_configuration_leaves_its_reason_with_the_context():
    for bad, why in REFUSALS:
        config = dict(D=4, fmt="cf64")
        config.update(bad)
        with pytest.raises(MgpuError) as e:
            WidebandBlanker(_rx(), config.pop("D"), config.pop("fmt"), **config)
        assert e.value.code == 1 and last_error(_rx()) == "mgpu_wblank_create: " + why, bad


def test_two_handles_on_two_contexts_stay_independent():
    """one stream through a blanker of each context, their calls interleaved and cut differently: each gives the twin's bytes"""
    B = 256
    xa, xb = ref.planted(51, B, "cf64", B // 8), ref.planted(52, B, "cs16", B // 8)
    a, b = WidebandBlanker(_rx(), 4, "cf64", guard=7), WidebandBlanker(other_rx(), 1, "cs16", guard=0, threshold=30.0)
    got_a, got_b = [], []
    for i in range(4):
        got_a.append(a.process_raw(xa[i * 3 * B: (i + 1) * 3 * B]))
        got_b += [b.process_raw(xb[(3 * i + j) * B: (3 * i + j + 1) * B]) for j in range(3)]
    assert _same(_join(got_a), host_wblank_process(xa, 4, guard=7))
    assert _same(_join(got_b), host_wblank_process(xb, 1, guard=0, threshold=30.0))
    a.close(), b.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
TP, D, B = 320, 4, 256          # synthesiser -> channeliser delays a frame by tp audio samples; the blanker by B / D = 64 more
HOPS_PER_CALL = 16              # 16 hops of 1088 audio samples are 272 blocks of 256 IQ samples
LINKS = ThreeLinks(seed=2026, tail=TP + B // D, hops_per_call=HOPS_PER_CALL)
PLAN = ((-30000, 0, 1.0), (-27000, 0, 1.0), (12000, 1, 1.0))           # multiples of R / B = 750 Hz: the blanker's delay turns no carrier
CLICK_DB = 60.0                 # tests/test_wideband_blanker_host.py MEASURED_DB: the unblanked audio error is 8.8 dB above the station


def test_three_links_end_to_end_with_clicks():
    """Mode 8, D = 4: three frames in silence through Synthesizer -> (clicks) -> (WidebandBlanker) -> Channelizer ->
    RxCapture.run_wideband in calls of 16 hops. One-sample clicks at 100 Hz, 60 dB above a link's rms. The blanked run delivers exactly
    the links the click-free run delivers; the clicked run without the blanker delivers a strict subset of them. The frames start where
    the existing loop delivers the transmitted audio itself delayed by tp and by tp + B / D samples
    (band_links.ThreeLinks.starts_the_loop_delivers): chosen on a pure delay, never by the new stage's output."""
    torch = _torch()
    rx = _rx()
    starts = LINKS.starts_the_loop_delivers((TP, TP + B // D))
    _, frames = LINKS.frames()
    fsz = frames.shape[1]
    audio = LINKS.audio(starts)
    sy = Synthesizer(rx, D, PLAN)
    step = HOPS_PER_CALL * rx.Nofdm * 4
    iq = np.concatenate([sy.process(np.ascontiguousarray(audio[:, c: c + step]), fmt="cf32") for c in range(0, audio.shape[1], step)])
    sy.close()
    lo, hi = (max(starts) + TP) * D, (min(starts) + fsz) * D
    assert hi - lo > 48000                                              # a stretch where all three links are on
    link_rms = np.sqrt(np.mean(np.abs(iq[lo:hi]) ** 2) / 3.0)
    clicked = (iq + ref.clicks(iq.size, 100.0, 48000.0 * D, link_rms * 10 ** (CLICK_DB / 20.0))).astype(np.complex64)

    def delivered(x, blank):
        ch = Channelizer(rx, D, PLAN)
        cap = RxCapture(rx, 3, CARRIER, max_hops=HOPS_PER_CALL)
        wb = WidebandBlanker(rx, D, "cf32") if blank else None
        d_x = torch.from_numpy(x).cuda()
        d_out = torch.zeros(step * D, dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()
        events, zeroed = [], 0
        for c in range(0, x.size, step * D):
            part = d_x[c: c + step * D]
            if wb:
                d_reports = torch.zeros((step * D // B, WBLANK_REPORT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
                wb.process_raw(part, d_out, d_reports)                  # the context's stream, as run_wideband's
                part = d_out
            events += [(e[0], e[1], None, e[3].tobytes()) for e in cap.run_wideband(ch, part)]
            if wb:
                zeroed += int(device_reports(d_reports, step * D // B, WBLANK_REPORT_DTYPE)["blanked"].sum())
        for h in (ch, cap, wb):
            if h:
                h.close()
        return LINKS.delivered(events), zeroed

    clean, _ = delivered(iq, False)
    plain, _ = delivered(clicked, False)
    blanked, zeroed = delivered(clicked, True)
    print("delivered links: click-free", sorted(clean), "clicked", sorted(plain), "clicked and blanked", sorted(blanked), "; samples zeroed",
          zeroed, "of", iq.size)
    assert clean == {0, 1, 2}
    assert blanked == clean
    assert plain < clean


def test_create_use_destroy_gives_the_memory_back():
    """50 create / process / destroy cycles (the held block, the flag words, staging, the output buffers) leave the device's free memory
    where it was"""
    memory_comes_back(lambda: WidebandBlanker(_rx(), 64), ref.noise(6, 64 * 4096, "cf64"))

"""Host-only parts of the band scanner (include/ext/mercury_scanner.h): the normative twin against the NumPy statement of the rule
(tests/scanner_ref.py) byte for byte, hand-built lines that pin every decision of the rule, the refusals, three links found in noise,
the plan made from them, and the twin under the sanitizers. No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scanner_ref as ref
from band_links import create_without_a_context, iq as make_iq, refused
from mercury_amd import (SCAN_REPORT_DTYPE, SCANNER_SYMBOLS, host_scan_plan, host_scan_process, load_library, scan_config,
                         scan_reports)
from mercury_amd.physical_layer import ChanChannel, ScanConfig, ScanState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(edge_bins=5, dc_bins=1, gap=2, min_bins=1, max_runs=32, threshold=3.0)


def same(got, want):
    """lines and reports, byte for byte"""
    return (got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes() and got[1].shape == want[1].shape
            and got[1].tobytes() == want[1].tobytes())


def test_symbols_are_exported_and_the_struct_layouts_are_the_headers():
    lib = load_library()
    assert len(SCANNER_SYMBOLS) == 9
    for name in SCANNER_SYMBOLS:
        assert hasattr(lib, name), name
    assert C.sizeof(ScanConfig) == 48           # four ints, a double, six ints
    assert C.sizeof(ScanState) == 40            # three uint64, four ints
    assert SCAN_REPORT_DTYPE.itemsize == 800    # 32 bytes and 32 runs of 24


@pytest.mark.parametrize("position_lines", [0, 2 ** 40])
@pytest.mark.parametrize("fmt", ["cs16", "cf32", "cf64"])
@pytest.mark.parametrize("A", [1, 2, 3])
@pytest.mark.parametrize("log2n", [8, 9])
def test_twin_equals_the_numpy_statement(log2n, A, fmt, position_lines):
    """noise with two tones in it, so that every line has runs; 2 A + 1 blocks: two lines and a block that completes none"""
    N, H = 1 << log2n, (1 << log2n) // 2
    n_in = (2 * A + 1) * H
    x = make_iq(np.random.default_rng(100 * log2n + A), n_in, fmt)
    tones = ref.two_bin_tones(log2n, n_in, [N // 4, N // 4 + 3, 3 * N // 4], 6.0)
    if fmt == "cs16":
        x = (x // 8 + np.stack([tones.real, tones.imag], 1) * 4096).astype(np.int16)
    else:
        x = (x + tones).astype(x.dtype)
    position = position_lines * H * A
    config = dict(SMALL, log2n=log2n, blocks_per_line=A)
    got = host_scan_process(x, 4, position=position, **config)
    want = ref.process(x, position=position, **config)
    assert got[0].shape == ((2 * A + 1) // A, N) and got[1]["n_runs"].min() >= 1
    assert int(got[1]["first_block"][0]) == position // H
    assert same(got, want)


# ---- hand-built lines ----------------------------------------------------------------------------------------------------------------------
# N = 256, A = 1. A tone half-way between two bins falls into exactly those two (scanner_ref.two_bin_tones); a noise floor 60 dB below
# gives the level. Bins of the floor are exponentially distributed: one reaches 50 times the median (35 times the mean) with
# probability e^-35. The line judged is the last of four: every block of it is full.
HAND = dict(log2n=8, blocks_per_line=1, threshold=50.0, edge_bins=8, dc_bins=2, gap=3, min_bins=1, max_runs=32)


def hand_line(firsts, **config):
    config = dict(HAND, **config)
    n = 4 * 128
    x = ref.two_bin_tones(8, n, firsts) + ref.floor_noise(3, n)
    got = host_scan_process(x, 4, **config)
    assert same(got, ref.process(x, **config))
    return scan_reports(got[1])[-1], got[0][-1]


def spans(report):
    return [(r["first"], r["count"]) for r in report["runs"]]


def test_a_gap_of_gap_bins_closes_and_one_more_does_not():
    report, line = hand_line([40, 45, 60, 66])                 # 42..44 unoccupied: 3 bins; 62..65: 4
    assert spans(report) == [(40, 7), (60, 2), (66, 2)] and report["n_runs"] == 3
    run = report["runs"][0]
    assert run["power"] == float(np.add.accumulate(line[40:47])[-1]) and run["peak"] == 40 + int(np.argmax(line[40:47]))
    assert spans(hand_line([40, 45, 60, 66], gap=4)[0]) == [(40, 7), (60, 8)]
    assert spans(hand_line([40, 45, 60, 66], gap=0)[0]) == [(40, 2), (45, 2), (60, 2), (66, 2)]


def test_a_run_of_min_bins_less_one_is_dropped():
    assert spans(hand_line([40, 60, 62], min_bins=3)[0]) == [(60, 4)]
    assert spans(hand_line([40, 60, 62], min_bins=2)[0]) == [(40, 2), (60, 4)]


def test_a_run_touching_the_edges_stops_there():
    """edge_bins = 8: bins 7 and 248 are excluded, 8 and 247 usable"""
    assert spans(hand_line([7, 247])[0]) == [(8, 1), (247, 1)]
    assert spans(hand_line([7, 247], edge_bins=0)[0]) == [(7, 2), (247, 2)]


def test_runs_on_either_side_of_dc_never_join():
    """dc_bins = 2 excludes 126..130; the tones at 124 and 131 leave exactly those five bins between their runs, and gap = 8 would close
    five usable ones; the tone at 125 has one bin on either side of the exclusion's edge"""
    assert spans(hand_line([124, 131], gap=8)[0]) == [(124, 2), (131, 2)]
    assert spans(hand_line([124, 131], gap=8, dc_bins=0)[0]) == [(124, 9)]
    assert spans(hand_line([125])[0]) == [(125, 1)]


def test_more_runs_than_max_runs_are_counted_not_reported():
    report, _ = hand_line([40, 60, 80], max_runs=2)
    assert report["n_runs"] == 3 and report["reported"] == 2 and spans(report) == [(40, 2), (60, 2)]


def test_a_nan_sample_makes_the_line_nonfinite():
    config = dict(HAND)
    x = ref.two_bin_tones(8, 512, [40]) + ref.floor_noise(3, 512)
    x[300] = complex(np.nan, 0.0)                               # in blocks 2 and 3: lines 2 and 3
    lines, reports = host_scan_process(x, 4, **config)
    assert same((lines, reports), ref.process(x, **config))
    assert list(reports["nonfinite"]) == [0, 0, 1, 1] and list(reports["n_runs"][2:]) == [0, 0]
    assert reports["level"][3].tobytes() == np.float64(0.0).tobytes() and np.isnan(lines[3]).all()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
BAD_CONFIGS = [dict(D=0), dict(D=65), dict(log2n=7), dict(log2n=13), dict(blocks_per_line=0), dict(blocks_per_line=4097),
               dict(threshold=1.5), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(edge_bins=-1), dict(edge_bins=65),
               dict(dc_bins=-1), dict(dc_bins=17), dict(gap=-1), dict(gap=65), dict(min_bins=0), dict(min_bins=257), dict(max_runs=0),
               dict(max_runs=33), dict(max_in=-128), dict(max_in=100)]


@pytest.mark.parametrize("bad", BAD_CONFIGS, ids=[repr(b) for b in BAD_CONFIGS])
def test_every_bad_configuration_is_refused(bad):
    """by the twin, and by mgpu_scan_create before any device work: without a context it says MGPU_ERR_ARG, not MGPU_ERR_DEVICE"""
    config = dict(log2n=8, blocks_per_line=1)
    D = 4
    if "D" in bad:
        D = bad["D"]
    else:
        config.update(bad)
    x = np.zeros(256, np.complex128)
    refused(lambda: host_scan_process(x, D, **config))
    assert create_without_a_context(load_library().mgpu_scan_create, C.byref(scan_config(D, **config))) == 1


def test_a_good_configuration_without_a_context_is_a_device_error_and_struct_size_is_checked():
    lib = load_library()
    assert create_without_a_context(lib.mgpu_scan_create, C.byref(scan_config(4, log2n=8))) == 2
    k = scan_config(4, log2n=8)
    k.struct_size -= 4
    assert create_without_a_context(lib.mgpu_scan_create, C.byref(k)) == 1
    refused(lambda: host_scan_process(np.zeros(256, np.complex128), 4, log2n=8, struct_size=52))
    assert lib.mgpu_scan_lines(None, 128) < 0 and lib.mgpu_scan_seek(None, 0) == 1 and lib.mgpu_scan_destroy(None) == 1


@pytest.mark.parametrize("n_in", [0, 127, 129, 64])
def test_every_bad_n_in_is_refused(n_in):
    refused(lambda: host_scan_process(np.zeros(max(n_in, 1), np.complex128)[:n_in], 4, log2n=8, blocks_per_line=1))


@pytest.mark.parametrize("position", [128, 255, 3 * 128 + 1, 2 ** 62 + 256])
def test_every_bad_position_is_refused(position):
    """A = 2: a position is a multiple of H A = 256, 2^62 at most"""
    refused(lambda: host_scan_process(np.zeros(256, np.complex128), 4, position=position, log2n=8, blocks_per_line=2))


def test_an_unknown_format_is_refused():
    refused(lambda: host_scan_process(np.zeros(256, np.complex128), 4, fmt=7, log2n=8))


# ---- three links ---------------------------------------------------------------------------------------------------------------------------
LINK_SNR_DB = 15.0


def found_links(reports):
    """the runs of the last line as (centre in Hz, width in Hz)"""
    bin_hz = 48000.0 * ref.LINK_D / 4096
    return [((r["first"] + (r["count"] - 1) / 2.0 - 2048) * bin_hz, r["count"] * bin_hz) for r in reports[-1]["runs"]]


def test_three_links_are_found_within_a_bin_of_their_centres():
    """Three links, two USB and one LSB, in a 192 kHz span (D = 4) with the default scanner (N = 4096, A = 16, threshold 5): exactly three
    runs, each centred within one bin, 46.875 Hz, of its link's offset + sigma a_c. The in-band SNR (a link's power over the noise inside
    its own 2343.75 Hz) is 15 dB. Measured on the CPU with the twin alone, over five noise seeds: it meets this at 10, 15, 20 and 30 dB
    with every seed; at 8 dB with one seed of five (a link's run breaks in two or loses an edge: signal plus noise is then 7.3 times the
    noise, and a bin summed over 16 overlapped blocks falls under 5 times the median now and then); from 6 dB down with none. 15 dB
    stands 5 dB clear of where it holds. Every link is asserted."""
    lines, reports = host_scan_process(ref.three_links(LINK_SNR_DB), ref.LINK_D)
    assert lines.shape == (2, 4096)
    found = found_links(scan_reports(reports))
    print("found", found, "true centres", ref.link_centres())
    assert len(found) == 3 and reports["n_runs"][-1] == 3
    for (centre, width), true in zip(found, sorted(ref.link_centres())):
        assert abs(centre - true) <= 46.875, (centre, true)
        assert 1800.0 <= width <= 3200.0


def test_the_plan_round_trips_the_three_links():
    """mgpu_host_scan_plan on each found run, with the link's own sideband, gives its offset back to a bin; a band that leaves the span is
    refused"""
    _, reports = host_scan_process(ref.three_links(LINK_SNR_DB), ref.LINK_D)
    runs = scan_reports(reports)[-1]["runs"]
    truth = sorted(ref.LINK_PLAN)
    for run, (offset, sideband, _) in zip(runs, truth):
        got = host_scan_plan(run, ref.LINK_D, sideband=sideband)
        centre = (run["first"] + (run["count"] - 1) / 2.0 - 2048) * 46.875
        assert got == (int(np.round(centre - (-1 if sideband else 1) * 1472)), sideband, 1.0)
        assert abs(got[0] - offset) <= 47
    refused(lambda: host_scan_plan({"first": 4090, "count": 6}, ref.LINK_D))                     # USB: the band would end above R / 2
    refused(lambda: host_scan_plan({"first": 0, "count": 6}, ref.LINK_D, sideband=1))            # LSB: below -R / 2
    refused(lambda: host_scan_plan({"first": 4090, "count": 7}, ref.LINK_D))                     # no such run
    assert C.sizeof(ChanChannel) == 16


# ---- sanitizers ----------------------------------------------------------------------------------------------------------------------------
def test_the_twin_is_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/scanner_sanitize.cpp with mercury_amd/csrc/scan_rule.hpp and scan_fft.h built as one stand-alone program and run on the
    CPU: the twin over the formats, cuts and refusals, and the block kernel's schedule against the rule's loop nest at every N"""
    exe = str(tmp_path / "scanner_sanitize")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "mercury_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "scanner_sanitize.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "scanner: clean" in out.stdout

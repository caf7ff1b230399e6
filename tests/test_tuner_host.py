"""Host-only parts of the carrier tuner (include/ext/mercury_tuner.h): the normative twin against the NumPy statement of the rule
(tests/tuner_ref.py) bit for bit, the pinned decisions, the refusals, the accuracy on generated Mercury-geometry frames over the whole
stated range of displacements, noise alone, and the twin under the sanitizers. No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tuner_ref as ref
from band_links import create_without_a_context, refused, taps
from mercury_amd import (TUNE_DEFAULT_MIN_METRIC, TUNE_REPORT_DTYPE, TUNER_SYMBOLS, chan_channels, host_tune_plan, host_tune_process,
                         load_library, tune_config, tune_reports, tune_samples)
from mercury_amd.physical_layer import TuneConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEARCH_LIMIT_HZ = 1125                  # what profiles/tuner.md states as the limit of `search`: 24 carriers, measured with the default taps


def test_symbols_are_exported_and_the_struct_layouts_are_the_headers():
    lib = load_library()
    assert len(TUNER_SYMBOLS) == 8
    for name in TUNER_SYMBOLS:
        assert hasattr(lib, name), name
    assert C.sizeof(TuneConfig) == 56           # six ints, a pointer, two doubles, two ints
    assert TUNE_REPORT_DTYPE.itemsize == 56     # four doubles, six ints
    assert TUNE_DEFAULT_MIN_METRIC == 0.44 and tune_samples(3, 4) == 4 * 3 * 272 * 5


# ---- the twin against the restatement -------------------------------------------------------------------------------------------------------
def small_plan(D):
    """three stations, both sidebands, and the plan that looks for them: off by less and by more than a carrier spacing"""
    true = [(-9000 * D + 123, 0, 1.0), (5217 * D, 1, 0.7), (37, 0, 1.3)]
    plan = [(true[0][0] + 31, 0, 1.0), (true[1][0] - 58, 1, 0.7), (true[2][0] + 3, 0, 1.3)]
    return true, plan


@pytest.mark.parametrize("fmt", ["cs16", "cf32", "cf64"])
@pytest.mark.parametrize("D", [1, 3])
def test_twin_equals_the_numpy_statement(D, fmt):
    """tp = 8, J = 4, S = 3: the smallest shape at which every index formula is exercised: the stride of 4 D between outputs, the
    floor-mod phasors of a negative centre, the fold's and the comb's last samples at m = 272 J + 270 and 272 J + 262 of 272 (J + 1)"""
    true, plan = small_plan(D)
    config = dict(symbols=4, search=8, taps=taps(D, 8))
    x = ref.block(5 + D, D, true, symbols=4, n_symbols=3, noise_db=-30, fmt=fmt, taps=taps(D, 8))
    got = host_tune_process(x, D, plan, want_arrays=True, **config)
    want = ref.process(x, D, plan, **config)
    assert got[0]["nonfinite"].max() == 0 and got[0]["metric"].min() > 0.0
    assert ref.same(got, want)


def test_twin_equals_the_numpy_statement_at_the_edges_of_the_configuration():
    """search 0 (one score, no second: contrast +0.0) and 24, another carrier and audio centre, a threshold nothing reaches"""
    D = 1
    true, plan = small_plan(D)
    x = ref.block(9, D, true, symbols=5, n_symbols=4, noise_db=-20, taps=taps(D, 8))
    for config in (dict(search=0), dict(search=24), dict(search=3, carrier_hz=1500.0, audio_centre_hz=1400), dict(search=8, min_metric=1.0)):
        config = dict(config, symbols=5, taps=taps(D, 8))
        got = host_tune_process(x, D, plan, want_arrays=True, **config)
        assert ref.same(got, ref.process(x, D, plan, **config)), config
        if config["search"] == 0:
            assert list(got[0]["shift"]) == [0, 0, 0] and got[0]["contrast"].tobytes() == bytes(24)
        if config.get("min_metric") == 1.0:
            assert list(got[0]["valid"]) == [0, 0, 0] and [int(o) for o in got[0]["offset_hz"]] == [p[0] for p in plan]


# ---- pinned decisions -----------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_first_index_and_silence_is_not_valid():
    """a block of zeros: every |G|^2 is equal (phi* = 0, the first), every score is equal (shift = -K, the first), E = 0 gives the
    metric +0.0, and the report is not valid whatever min_metric is; nothing is nonfinite"""
    D, plan = 1, [(1000, 0, 1.0), (-3000, 1, 2.0)]
    x = np.zeros(tune_samples(D, 4), np.complex128)
    reports, G, E, Q = host_tune_process(x, D, plan, want_arrays=True, symbols=4, search=5, taps=taps(D, 8), min_metric=1e-300)
    assert not G.any() and not E.any() and not Q.any()
    for r, ch in zip(tune_reports(reports), plan):
        assert r["phase"] == 0 and r["shift"] == -5 and r["metric"] == 0.0 and r["contrast"] == 0.0
        assert r["valid"] == 0 and r["nonfinite"] == 0 and r["offset_hz"] == ch[0]
    assert reports["metric"].tobytes() == bytes(16)                             # +0.0, not -0.0
    assert ref.same((reports, G, E, Q), ref.process(x, D, plan, symbols=4, search=5, taps=taps(D, 8), min_metric=1e-300))


def test_a_tie_of_the_score_between_two_positions_goes_to_the_first():
    """one symbol's worth of a single tone, turned so that it falls on bin 26 exactly: the combs at d = 1 (bins 2..26) .. d = 24 hold it on
    their upper side, each with the same sum to the bit where the other bins are exact zeros; here they are rounding noise, so the
    restatement is the judge: the twin decides as it does"""
    D = 1
    x = np.exp(2j * np.pi * (26 * 46.875) * np.arange(tune_samples(D, 4)) / 48000.0)
    plan = [(-1472, 0, 1.0)]                                                    # F = 0
    got = host_tune_process(x, D, plan, want_arrays=True, symbols=4, search=24, taps=taps(D, 8))
    assert got[0]["shift"][0] >= 1
    assert ref.same(got, ref.process(x, D, plan, symbols=4, search=24, taps=taps(D, 8)))


def test_a_nan_sample_makes_every_channel_nonfinite():
    D = 3
    true, plan = small_plan(D)
    x = ref.block(11, D, true, symbols=4, n_symbols=3, taps=taps(D, 8)).copy()
    x[len(x) // 2] = complex(np.nan, 0.0)
    reports = host_tune_process(x, D, plan, symbols=4, taps=taps(D, 8))
    for r, ch in zip(tune_reports(reports), plan):
        assert r == dict(metric=0.0, phase=0, frac_hz=0.0, shift=0, delta_hz=0.0, contrast=0.0, offset_hz=ch[0], valid=0, nonfinite=1)
    assert host_tune_plan(reports, plan) == plan
    assert reports.tobytes() == ref.process(x, D, plan, symbols=4, taps=taps(D, 8))[0].tobytes()


def test_the_plan_keeps_sideband_and_gain_and_an_offset_that_is_not_valid():
    reports = np.zeros(2, TUNE_REPORT_DTYPE)
    reports["offset_hz"], reports["valid"] = [1234, 777], [1, 0]
    assert host_tune_plan(reports, [(1200, 1, 0.25), (-5000, 0, 3.0)]) == [(1234, 1, 0.25), (-5000, 0, 3.0)]
    assert host_tune_plan(tune_reports(reports), [(1200, 1, 0.25), (-5000, 0, 3.0)]) == [(1234, 1, 0.25), (-5000, 0, 3.0)]
    lib = load_library()
    assert lib.mgpu_host_tune_plan(None, None, None) == 1


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
BAD_CONFIGS = [dict(D=0), dict(D=65), dict(symbols=3), dict(symbols=257), dict(search=-1), dict(search=25), dict(audio_centre_hz=0),
               dict(audio_centre_hz=24000), dict(carrier_hz=0.0), dict(carrier_hz=24000.0), dict(carrier_hz=float("nan")),
               dict(min_metric=0.0), dict(min_metric=1.5), dict(min_metric=float("nan")), dict(taps=np.ones(8)), dict(taps=np.ones(1027)),
               dict(taps=np.array([1.0] * 8 + [np.inf])), dict(channels=[]), dict(channels=[(0, 2, 1.0)]), dict(channels=[(24000 - 2944, 0, 1.0)]),
               dict(channels=[(-24000 + 2944, 1, 1.0)]), dict(channels=[(0, 0, float("inf"))])]


@pytest.mark.parametrize("bad", BAD_CONFIGS, ids=[repr(b)[:40] for b in BAD_CONFIGS])
def test_every_bad_configuration_is_refused(bad):
    """by the twin, and by mgpu_tune_create before any device work: without a context it says MGPU_ERR_ARG, not MGPU_ERR_DEVICE"""
    config = dict(symbols=4, search=2, taps=taps(1, 8))
    config.update({k: v for k, v in bad.items() if k not in ("D", "channels")})
    D, channels = bad.get("D", 1), bad.get("channels", [(0, 0, 1.0)])
    x = np.zeros(tune_samples(max(D, 1), max(config["symbols"], 0)), np.complex128)
    refused(lambda: host_tune_process(x, D, channels, **config))
    k, _keep = tune_config(D, len(channels), **config)
    assert create_without_a_context(load_library().mgpu_tune_create, C.byref(k), chan_channels(channels)) == 1


def test_a_good_configuration_without_a_context_is_a_device_error_and_struct_size_is_checked():
    lib = load_library()
    k, _keep = tune_config(4, 1)
    chs = chan_channels([(0, 0, 1.0)])
    assert create_without_a_context(lib.mgpu_tune_create, C.byref(k), chs) == 2
    assert create_without_a_context(lib.mgpu_tune_create, C.byref(k), None) == 1
    k.struct_size -= 4
    assert create_without_a_context(lib.mgpu_tune_create, C.byref(k), chs) == 1
    refused(lambda: host_tune_process(np.zeros(tune_samples(1, 4), np.complex128), 1, [(0, 0, 1.0)], symbols=4, struct_size=60))
    assert lib.mgpu_tune_samples(None) < 0 and lib.mgpu_tune_destroy(None) == 1 and lib.mgpu_tune_retune(None, 0, chs) == 1
    assert lib.mgpu_tune_process(None, None, 2, 0, None) == 1 and lib.mgpu_tune_arrays(None, None, None, None) == 1


@pytest.mark.parametrize("change", [-1, 1, -272 * 4, 272 * 4])
def test_every_wrong_n_in_is_refused(change):
    n = tune_samples(1, 4)
    refused(lambda: host_tune_process(np.zeros(n + change, np.complex128), 1, [(0, 0, 1.0)], symbols=4, taps=taps(1, 8)))


def test_an_unknown_format_is_refused():
    refused(lambda: host_tune_process(np.zeros(tune_samples(1, 4), np.complex128), 1, [(0, 0, 1.0)], symbols=4, taps=taps(1, 8), fmt=7))


# ---- accuracy -------------------------------------------------------------------------------------------------------------------------------
# The displacement of the plan from the station, in Hz, over the whole stated range. The station's distance from the planned centre is
# -d -+ 0.125 Hz (the carrier is 1471.875, the audio centre 1472): 0 and +-1 lie at the fraction 0, +-47 at it one carrier on, +-23 and
# +-24 either side of half a spacing, and +-117 within 0.07 Hz of the fraction's wrap at +-23.4375 (117.1875 = 2.5 spacings).
DISPLACEMENTS = [0, 1, -1, 23, -23, 24, -24, 47, -47, 117, -117, 375, -375, 563, -563, 800, -800, 1000, -1000, 1100, -1100,
                 SEARCH_LIMIT_HZ, -SEARCH_LIMIT_HZ, 200]


@pytest.mark.parametrize("case", range(len(DISPLACEMENTS)))
def test_a_displaced_plan_is_tuned_to_within_a_hertz(case):
    """A generated frame of 12..40 symbols in silence at a random start, noise at -30 or -10 dB relative to the signal, D = 1 or 4, USB or
    LSB, the default taps and the largest search: the tuned offset is within 1 Hz of the offset the frame was synthesised at, and valid.
    The 1 Hz is the project's own figure: the link planned within 1 Hz is the one profiles/scanner.md shows arriving."""
    d = DISPLACEMENTS[case]
    D, sideband, noise_db = (1, 4)[case % 2], (case // 2) % 2, (-30, -10)[(case // 4) % 2]
    half, reach = 24000 * D, SEARCH_LIMIT_HZ + 1
    lo, hi = (-half + 1 + reach, half - 2945 - reach) if sideband == 0 else (-half + 2945 + reach, half - 1 - reach)
    true = int(np.random.default_rng(700 + case).integers(lo, hi + 1))
    x = ref.block(7000 + case, D, [(true, sideband, 1.0)], noise_db=noise_db)
    r = tune_reports(host_tune_process(x, D, [(true + d, sideband, 1.0)], search=24))[0]
    print(dict(D=D, sideband=sideband, noise_db=noise_db, displacement=d, true=true), r)
    assert r["valid"] == 1 and r["nonfinite"] == 0
    assert abs(r["offset_hz"] - true) <= 1


@pytest.mark.parametrize("D", [1, 4])
def test_the_default_search_tunes_a_plan_a_scanner_bin_off(D):
    """the defaults throughout (search 8, 375 Hz): a plan one scanner bin (46.875 Hz at D = 4, N = 4096) and eight carriers off"""
    for seed, d in ((1, 47), (2, -46), (3, 375), (4, -375)):
        true = 6000 * D - 5000 + seed
        x = ref.block(7100 + seed, D, [(true, seed % 2, 1.0)], noise_db=-30)
        r = tune_reports(host_tune_process(x, D, [(true + d, seed % 2, 1.0)]))[0]
        assert r["valid"] == 1 and abs(r["offset_hz"] - true) <= 1, (d, r)


def test_noise_alone_is_not_valid():
    """64 seeded blocks of white Gaussian noise at the measured default threshold (the highest metric over 1024 blocks was 0.2926)"""
    top = 0.0
    for seed in range(64):
        r = host_tune_process(ref.noise_block(seed), 1, [(0, 0, 1.0)])[0]
        top = max(top, float(r["metric"]))
        assert r["valid"] == 0 and r["nonfinite"] == 0 and r["offset_hz"] == 0
    print("highest metric", top)


# ---- sanitizers -----------------------------------------------------------------------------------------------------------------------------
def test_the_twin_is_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/tuner_sanitize.cpp with mercury_amd/csrc/tune_rule.hpp and chan_tables.cpp built as one stand-alone program and run on
    the CPU: the twin in exactly sized buffers over the formats, a NaN block, silence and the refusals, and the comb kernel's schedule
    against the rule's loop nest"""
    exe = str(tmp_path / "tuner_sanitize")
    csrc = os.path.join(ROOT, "mercury_amd", "csrc")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", csrc,
                    os.path.join(ROOT, "tests", "cpp", "tuner_sanitize.cpp"), os.path.join(csrc, "chan_tables.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tuner: clean" in out.stdout

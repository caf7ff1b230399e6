"""Host-only parts of the wideband impulse blanker (include/ext/mercury_wideband_blanker.h): the normative twin against the NumPy statement
of the rule (tests/wblank_ref.py) byte for byte on inputs planted where the rule can go wrong, the refusals, white noise at the measured
default threshold, what the stage is for at the signal level, and the twin under the sanitizers. No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import wblank_ref as ref
from band_links import create_without_a_context, refused
from mercury_amd import (WBLANK_DEFAULT_THRESHOLD, WBLANK_REPORT_DTYPE, WBLANK_SYMBOLS, host_chan_process, host_synth_process,
                         host_wblank_process, load_library, wblank_block, wblank_config)
from mercury_amd.physical_layer import WblankConfig, WblankState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(got, want):
    """output and reports, byte for byte"""
    return (got[0].shape == want[0].shape and got[0].dtype == want[0].dtype and got[0].tobytes() == want[0].tobytes()
            and got[1].shape == want[1].shape and got[1].tobytes() == want[1].tobytes())


def test_symbols_are_exported_and_the_struct_layouts_are_the_headers():
    lib = load_library()
    assert len(WBLANK_SYMBOLS) == 7
    for name in WBLANK_SYMBOLS:
        assert hasattr(lib, name), name
    assert C.sizeof(WblankConfig) == 40         # four ints, two doubles, two ints
    assert C.sizeof(WblankState) == 40          # two uint64, six ints
    assert WBLANK_REPORT_DTYPE.itemsize == 32 and WBLANK_REPORT_DTYPE == ref.REPORT_DTYPE
    assert WBLANK_DEFAULT_THRESHOLD == ref.DEFAULT_THRESHOLD
    assert [wblank_block(D) for D in (1, 2, 3, 4, 5, 63, 64)] == [256, 256, 384, 256, 320, 4032, 4096]
    assert [ref.default_block(D) for D in (1, 2, 3, 4, 5, 63, 64)] == [256, 256, 384, 256, 320, 4032, 4096]


@pytest.mark.parametrize("guard", [0, 1, 64])
@pytest.mark.parametrize("B", [64, 256, 320, 4096])
@pytest.mark.parametrize("fmt", ["cs16", "cf32", "cf64"])
def test_twin_equals_the_numpy_statement(fmt, B, guard):
    """wblank_ref.planted at the stream's start, at a seeked multiple of B and where the call ends on 2^62"""
    cap = B // 8
    x = ref.planted(100 + B + guard, B, fmt, cap)
    config = dict(block=B, guard=guard)
    for position in (0, 5 * B, (2 ** 62 // B - ref.PLANTED_BLOCKS) * B):
        got = host_wblank_process(x, 4, position=position, **config)
        want = ref.process(x, 4, position=position, **config)
        assert same(got, want), position
    out, reports = got
    assert int(reports["block"][0]) == position // B - 1 and reports[0].tobytes()[8:] == bytes(24)
    assert not out[:B].any()
    r = {int(q["block"]) - position // B: q for q in reports[1:]}
    assert r[2]["exceeding"] == cap and not r[2]["capped"] and r[2]["blanked"] >= cap
    assert r[3]["exceeding"] == cap + 1 and r[3]["capped"] and (guard > 1 or r[3]["blanked"] == 0)
    assert r[4]["exceeding"] == 0 and r[5]["exceeding"] == 0 and r[5]["level"] == 0.0
    assert r[6]["exceeding"] == 3 and r[6]["level"] == 0.0 and not r[6]["capped"]
    assert r[0]["blanked"] == min(1 + guard, B) and (guard > 1 or r[1]["blanked"] == 1 + guard)   # each reaches into the other's block
    assert r[10]["blanked"] == guard                                                # the last block's click reaches into the emitted one
    if fmt != "cs16":
        assert np.isnan(r[8]["level"]) and r[8]["capped"] and r[8]["exceeding"] == B
        assert r[7]["exceeding"] == 3
        if guard <= 1:                                  # the block of NaN passes byte for byte; the -0.0 samples are unmarked and stay -0.0
            assert r[8]["blanked"] == 0 and out[9 * B: 10 * B].tobytes() == x[8 * B: 9 * B].tobytes()
            assert out[8 * B + 40: 8 * B + 42].tobytes() == x[7 * B + 40: 7 * B + 42].tobytes()
            assert np.signbit(out[8 * B + 40].real) and np.signbit(out[8 * B + 41].imag) and not np.signbit(out[8 * B + 41].real)
            assert out[8 * B + 9] == 0 and not np.signbit(out[8 * B + 9].real) and not np.signbit(out[8 * B + 9].imag)


def test_a_capped_block_and_the_default_block():
    """max_share = 0.25 at B = 64: cap = 16; the default block of D = 5 is 320"""
    x = ref.planted(7, 64, "cf32", 16)
    got = host_wblank_process(x, 4, block=64, max_share=0.25)
    assert same(got, ref.process(x, 4, block=64, max_share=0.25))
    assert got[1]["exceeding"][3] == 16 and not got[1]["capped"][3] and got[1]["exceeding"][4] == 17 and got[1]["capped"][4]
    y = ref.planted(8, 320, "cf64", 40)
    assert same(host_wblank_process(y, 5), ref.process(y, 5))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
BAD_CONFIGS = [dict(D=0), dict(D=65), dict(fmt=3), dict(fmt=-1), dict(block=32), dict(block=96), dict(block=4160), dict(block=-64),
               dict(threshold=1.5), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(guard=-1), dict(guard=65),
               dict(max_share=0.0), dict(max_share=0.51), dict(max_share=float("nan")), dict(max_share=-0.1), dict(max_in=-256),
               dict(max_in=100), dict(max_in=2 ** 26 + 256)]


@pytest.mark.parametrize("bad", BAD_CONFIGS, ids=[repr(b) for b in BAD_CONFIGS])
def test_every_bad_configuration_is_refused(bad):
    """by the twin, and by mgpu_wblank_create before any device work: without a context it says MGPU_ERR_ARG, not MGPU_ERR_DEVICE"""
    config = dict(block=256)
    D = bad.get("D", 4)
    config.update({k: v for k, v in bad.items() if k != "D"})
    x = np.zeros(512, np.complex128)
    refused(lambda: host_wblank_process(x, D, **config))
    config.setdefault("fmt", "cf64")
    assert create_without_a_context(load_library().mgpu_wblank_create, C.byref(wblank_config(D, **config))) == 1


def test_a_good_configuration_without_a_context_is_a_device_error_and_struct_size_is_checked():
    lib = load_library()
    assert create_without_a_context(lib.mgpu_wblank_create, C.byref(wblank_config(4))) == 2
    k = wblank_config(4)
    k.struct_size -= 4
    assert create_without_a_context(lib.mgpu_wblank_create, C.byref(k)) == 1
    refused(lambda: host_wblank_process(np.zeros(256, np.complex128), 4, struct_size=44))
    assert lib.mgpu_wblank_seek(None, 0) == 1 and lib.mgpu_wblank_destroy(None) == 1 and lib.mgpu_wblank_status(None, None) == 1


@pytest.mark.parametrize("n_in", [0, 255, 257, 64, 768])
def test_every_bad_n_in_is_refused(n_in):
    """no positive multiple of B = 256, or more than max_in = 512"""
    refused(lambda: host_wblank_process(np.zeros(max(n_in, 1), np.complex128)[:n_in], 4, max_in=512))


@pytest.mark.parametrize("position", [64, 255, 2 ** 62 + 256, 2 ** 62])
def test_every_bad_position_is_refused(position):
    """a position is a multiple of B = 256, and the call ends at 2^62 at most"""
    refused(lambda: host_wblank_process(np.zeros(256, np.complex128), 4, position=position))


# ---- noise -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 4, 64])
def test_noise_passes_at_the_default_threshold(D):
    """2^22 samples of white Gaussian noise at the default block of D, the profile's seeds: nothing exceeds, nothing is marked, and what
    comes out is the input one block late. The default threshold is 1.5 times the highest p / med_b over these very inputs
    (profiles/wideband_blanker.md), so the test stands a factor of 1.5 inside what it asserts."""
    B = wblank_block(D)
    x = ref.noise(ref.NOISE_SEEDS[D], 1 << 22)
    highest = ref.highest_ratio(x, B)
    print("D", D, "B", B, "highest p / med_b", highest)
    assert highest * 1.5 <= WBLANK_DEFAULT_THRESHOLD
    out, reports = host_wblank_process(x, D)
    assert len(reports) == (1 << 22) // B and not reports["exceeding"].any() and not reports["blanked"].any() and not reports["capped"].any()
    assert out[B:].tobytes() == x[:-B].tobytes() and not out[:B].any()


# ---- what the stage is for -------------------------------------------------------------------------------------------------------------------
# One station at unit rms through the synthesiser at D = 4 (offset 12 kHz: a multiple of R / B = 750 Hz, so that the delay of B samples is a
# pure delay of B / D audio samples behind the channeliser and no turn of the carrier's phase), one-sample clicks of random phase at
# 100 Hz, the channeliser; the error is the power of (audio - click-free audio) over the click-free audio's, in dB, away from the edges.
# Measured with the twin (profiles/wideband_blanker.md), click level above the station's rms in the IQ -> error unblanked, blanked:
MEASURED_DB = {40: (-11.18, -31.83), 50: (-1.18, -31.83), 60: (8.82, -31.83)}
N_AUDIO = 372 * 64


def signal_level_errors(level_db):
    D, B = ref.STATION_D, wblank_block(ref.STATION_D)
    station = ref.STATION
    iq = host_synth_process(D, [station], ref.station(N_AUDIO))
    rms = np.sqrt(np.mean(np.abs(iq) ** 2))
    clicked = iq + ref.clicks(iq.size, 100.0, 48000.0 * D, rms * 10 ** (level_db / 20.0))
    clean = host_chan_process(D, [station], iq)[0]
    plain = host_chan_process(D, [station], clicked)[0]
    out, reports = host_wblank_process(clicked, D)
    blanked = host_chan_process(D, [station], out)[0]
    edge, d = 400, B // D
    power = np.mean(clean[edge:-edge] ** 2)
    db = lambda e: 10 * np.log10(np.mean(e ** 2) / power)
    return (db(plain[edge:-edge] - clean[edge:-edge]), db(blanked[edge + d: -edge] - clean[edge: -edge - d]), int(reports["blanked"].sum()),
            int(reports["exceeding"].sum()))


@pytest.fixture(scope="module")
def errors():
    return {level: signal_level_errors(level) for level in MEASURED_DB}


@pytest.mark.parametrize("level_db", sorted(MEASURED_DB))
def test_blanking_lowers_the_audio_error(errors, level_db):
    """at each click level blanking lowers the error by at least half of the measured improvement in dB"""
    plain, blanked, zeroed, found = errors[level_db]
    print("clicks %d dB above the station: error %.2f dB unblanked, %.2f dB blanked; %d clicks found, %d samples zeroed"
          % (level_db, plain, blanked, found, zeroed))
    measured = MEASURED_DB[level_db]
    assert plain - blanked >= (measured[0] - measured[1]) / 2.0


def test_blanking_costs_the_zeroed_samples_not_the_clicks_height(errors):
    assert abs(errors[60][1] - errors[40][1]) <= 1.0


# ---- sanitizers ----------------------------------------------------------------------------------------------------------------------------
def test_the_twin_is_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/wblank_sanitize.cpp with mercury_amd/csrc/wblank_rule.hpp built as one stand-alone program and run on the CPU in exactly
    sized buffers: three formats, B = 64 and 4096, guard 64, a seeked position, the refusals"""
    exe = str(tmp_path / "wblank_sanitize")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "mercury_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "wblank_sanitize.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "wideband blanker: clean" in out.stdout

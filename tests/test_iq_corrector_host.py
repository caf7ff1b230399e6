"""Host-only parts of the IQ corrector (include/ext/mercury_iq_corrector.h): the normative twin against the NumPy statement of the rule
(tests/iqc_ref.py) byte for byte on inputs planted where the rule can go wrong, the recursion as the stage's only memory, the refusals,
what the stage is for at the signal level, and the twin under the sanitizers. No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import iqc_ref as ref
from band_links import create_without_a_context, refused
from mercury_amd import (IQC_DEFAULT_BLOCK, IQC_DEFAULT_MEMORY, IQC_NO_BALANCE, IQC_REPORT_DTYPE, IQC_SKIPPED, IQC_SYMBOLS, host_iqc_process,
                         iqc_config, iqc_image_db, iqc_reports, load_library)
from mercury_amd.physical_layer import IqcConfig, IqcState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(got, want):
    """output and reports, byte for byte"""
    return (got[0].shape == want[0].shape and got[0].dtype == want[0].dtype and got[0].tobytes() == want[0].tobytes()
            and got[1].shape == want[1].shape and got[1].tobytes() == want[1].tobytes())


def test_symbols_are_exported_and_the_struct_layouts_are_the_headers():
    lib = load_library()
    assert len(IQC_SYMBOLS) == 8
    for name in IQC_SYMBOLS:
        assert hasattr(lib, name), name
    assert C.sizeof(IqcConfig) == 72            # eight ints, four doubles, two ints
    assert C.sizeof(IqcState) == 128            # two uint64, four ints, eleven doubles, two ints
    assert IQC_REPORT_DTYPE.itemsize == 48 and IQC_REPORT_DTYPE == ref.REPORT_DTYPE
    assert (IQC_DEFAULT_BLOCK, IQC_DEFAULT_MEMORY, IQC_SKIPPED, IQC_NO_BALANCE) == (ref.DEFAULT_BLOCK, ref.DEFAULT_MEMORY, ref.SKIPPED, ref.NO_BALANCE)


@pytest.mark.parametrize("memory", [0, 2, 1024])
@pytest.mark.parametrize("B", [256, 768, 4096])
@pytest.mark.parametrize("fmt", ["cs16", "cf32", "cf64"])
def test_twin_equals_the_numpy_statement(fmt, B, memory):
    """iqc_ref.planted at the stream's start, at a seeked multiple of B and where the call ends on 2^62"""
    x = ref.planted(100 + B + memory, B, fmt)
    config = dict(block=B, memory=memory)
    for position in (0, 5 * B, (2 ** 62 // B - ref.PLANTED_BLOCKS) * B):
        got = host_iqc_process(x, 4, position=position, **config)
        want = ref.process(x, 4, position=position, **config)[:2]
        assert same(got, want), position
    out, r = got
    assert int(r["block"][0]) == position // B and int(r["block"][-1]) == position // B + ref.PLANTED_BLOCKS - 1
    # the all-zero start: no balance, and the output is the input less nothing
    assert r["flags"][0] == IQC_NO_BALANCE and (r["dc_re"][0], r["dc_im"][0], r["skew"][0], r["gain"][0]) == (0.0, 0.0, 0.0, 1.0)
    assert (out[:B] == x[:B]).all()
    # pure I: r <= 0
    assert r["flags"][1] == IQC_NO_BALANCE and r["dc_re"][1] != 0.0 and r["dc_im"][1] == 0.0
    assert not r["flags"][2:5].any() and (r["gain"][2:5] != 1.0).all() and (r["skew"][2:5] != 0.0).all()
    if fmt == "cs16":
        assert not (r["flags"] & IQC_SKIPPED).any()
        assert r["clamped"][5] >= 2 and r["clamped"][7] >= 2 and not r["clamped"][[0, 1, 8, 9]].any()
    else:
        assert [int(f) for f in r["flags"][5:8]] == [IQC_SKIPPED, 0, IQC_SKIPPED] and not r["clamped"].any()
        for b in (5, 7):                        # a skipped block is corrected with the standing estimate: the block before's
            assert r[b].tobytes()[8:40] == r[b - 1].tobytes()[8:40]
        assert np.isnan(out.ravel()[5 * B + 9].real) and np.isfinite(out.ravel()[5 * B + 10])
    if memory == 0:                             # lambda = 1: N counts the samples that went in
        T = ref.process(x, 4, **config)[2]
        assert T[5] == B * (ref.PLANTED_BLOCKS - (0 if fmt == "cs16" else 2))


@pytest.mark.parametrize("config", [dict(dc=0), dict(balance=0), dict(dc=0, balance=0),
                                    dict(fixed=1, fixed_dc_re=0.25, fixed_dc_im=-0.125, fixed_skew=0.09, fixed_gain=0.91),
                                    dict(fixed=1, fixed_dc_re=0.25, fixed_dc_im=-0.125, fixed_skew=-0.5, fixed_gain=2.0, dc=0),
                                    dict(fixed=1, fixed_skew=0.5, fixed_gain=0.5, balance=0)], ids=repr)
@pytest.mark.parametrize("fmt", ["cs16", "cf32", "cf64"])
def test_the_switches_and_the_fixed_mode(fmt, config):
    x = ref.planted(7, 256, fmt)
    got = host_iqc_process(x, 4, block=256, memory=2, **config)
    assert same(got, ref.process(x, 4, block=256, memory=2, **config)[:2])
    r = got[1]
    if not config.get("dc", 1):
        assert not r["dc_re"].any() and not r["dc_im"].any()
    if not config.get("balance", 1):
        assert not r["skew"].any() and (r["gain"] == 1.0).all()
    if config.get("fixed"):
        assert not r["flags"].any() and len(set(q.tobytes()[8:40] for q in r)) == 1
    else:
        assert r["flags"][0] == IQC_NO_BALANCE and not r["flags"][3]       # the flag says what was measured, whatever was applied


def test_the_default_block_and_memory():
    x = ref.planted(8, 4096, "cf32")
    got = host_iqc_process(x, 64)
    assert len(got[1]) == ref.PLANTED_BLOCKS and same(got, ref.process(x, 64)[:2])
    assert iqc_reports(got[1])[5]["skipped"] and iqc_reports(got[1])[0]["no_balance"] and not iqc_reports(got[1])[9]["no_balance"]


@pytest.mark.parametrize("memory", [0, 2, 1024])
def test_the_recursion_is_the_only_memory(memory):
    """the stream fed whole, and continued after every cut from the six doubles carried by hand"""
    B = 768
    x = ref.planted(9, B, "cf64")
    config = dict(block=B, memory=memory)
    whole = host_iqc_process(x, 4, position=3 * B, **config)
    for cut in (1, 2, 5, 6, 9):
        state = np.zeros(6)
        first = host_iqc_process(x[: cut * B], 4, position=3 * B, state=state, **config)
        assert state.tolist() == ref.process(x[: cut * B], 4, **config)[2]
        rest = host_iqc_process(x[cut * B:], 4, position=(3 + cut) * B, state=state.copy(), **config)
        assert same((np.concatenate([first[0], rest[0]]), np.concatenate([first[1], rest[1]])), whole), cut
        fresh = host_iqc_process(x[cut * B:], 4, position=(3 + cut) * B, **config)
        assert not same(fresh, rest)


def test_a_gain_outside_its_range_is_no_balance():
    """Q three times as strong as I: gain = 1/3 < 1/2; the other way round: gain = 3; and a skew above 1/2"""
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(4096), rng.standard_normal(4096)
    for x, balanced in ((a + 3j * b, False), (3 * a + 1j * b, False), (a + 1j * (b + 0.6 * a), False), (a + 1.9j * b, True), (1.9 * a + 1j * b, True),
                        (a + 1j * (b + 0.45 * a), True)):
        got = host_iqc_process(x, 4, block=4096)
        assert same(got, ref.process(x, 4, block=4096)[:2])
        r = got[1][0]
        assert bool(r["flags"] & IQC_NO_BALANCE) != balanced
        assert balanced or (r["skew"] == 0.0 and r["gain"] == 1.0 and r["dc_re"] != 0.0)


def test_cs16_that_clamps_is_counted():
    """full-scale samples of both signs under a fixed DC of (-0.5, 0.5) and a gain of 2: every component of every sample clamps or not
    as the rule says, and the count is the report's"""
    B = 256
    x = np.zeros((B, 2), np.int16)
    x[:, 0] = np.linspace(-32768, 32767, B).astype(np.int16)
    x[:, 1] = x[::-1, 0]
    config = dict(block=B, fixed=1, fixed_dc_re=-0.5, fixed_dc_im=0.5, fixed_skew=0.0, fixed_gain=2.0)
    got = host_iqc_process(x, 4, **config)
    assert same(got, ref.process(x, 4, **config)[:2])
    I, Q = x[:, 0] / 32768.0 + 0.5, 2.0 * (x[:, 1] / 32768.0 - 0.5)
    want = int((np.rint(I * 32768) > 32767).sum() + (np.rint(Q * 32768) < -32768).sum() + (np.rint(Q * 32768) > 32767).sum())
    assert want > B // 2 and got[1]["clamped"][0] == want
    assert got[0].max() == 32767 and got[0].min() == -32768


def test_negative_zeros_in_cf64():
    B = 256
    x = np.zeros(2 * B, np.complex128)
    x[:B] = complex(-0.0, -0.0)
    x[B:] = ref.to_format(ref.impair(ref.white(B, 3)), "cf64")
    x[B + 7] = complex(-0.0, 0.0)
    got = host_iqc_process(x, 4, block=B, memory=0)
    assert same(got, ref.process(x, 4, block=B, memory=0)[:2])
    assert np.signbit(got[0][:B].real).all()                          # -0.0 - 0.0 = -0.0: I passes as it is


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
BAD_CONFIGS = [dict(D=0), dict(D=65), dict(fmt=3), dict(fmt=-1), dict(block=128), dict(block=384), dict(block=4352), dict(block=-256),
               dict(memory=1), dict(memory=-1), dict(memory=2 ** 20 + 1), dict(dc=2), dict(dc=-1), dict(balance=2), dict(fixed=2),
               dict(fixed=1, fixed_dc_re=NAN), dict(fixed=1, fixed_dc_im=INF), dict(fixed=1, fixed_skew=NAN), dict(fixed=1, fixed_skew=0.51),
               dict(fixed=1, fixed_skew=-0.51), dict(fixed=1, fixed_gain=NAN), dict(fixed=1, fixed_gain=0.49), dict(fixed=1, fixed_gain=2.01),
               dict(fixed=1, fixed_gain=INF), dict(fixed=1, fixed_gain=0.0), dict(max_in=-256), dict(max_in=100), dict(max_in=2 ** 26 + 256)]


@pytest.mark.parametrize("bad", BAD_CONFIGS, ids=[repr(b) for b in BAD_CONFIGS])
def test_every_bad_configuration_is_refused(bad):
    """by the twin, and by mgpu_iqc_create before any device work: without a context it says MGPU_ERR_ARG, not MGPU_ERR_DEVICE"""
    config = dict(block=256)
    D = bad.get("D", 4)
    config.update({k: v for k, v in bad.items() if k != "D"})
    x = np.zeros(512, np.complex128)
    refused(lambda: host_iqc_process(x, D, **config))
    config.setdefault("fmt", "cf64")
    assert create_without_a_context(load_library().mgpu_iqc_create, C.byref(iqc_config(D, **config))) == 1


def test_a_good_configuration_without_a_context_is_a_device_error_and_struct_size_is_checked():
    lib = load_library()
    assert create_without_a_context(lib.mgpu_iqc_create, C.byref(iqc_config(4))) == 2
    assert create_without_a_context(lib.mgpu_iqc_create, C.byref(iqc_config(4, fixed=1, fixed_skew=0.5, fixed_gain=2.0))) == 2
    assert create_without_a_context(lib.mgpu_iqc_create, C.byref(iqc_config(4, fixed=0, fixed_gain=NAN))) == 2     # not read
    k = iqc_config(4)
    k.struct_size -= 4
    assert create_without_a_context(lib.mgpu_iqc_create, C.byref(k)) == 1
    refused(lambda: host_iqc_process(np.zeros(256, np.complex128), 4, block=256, struct_size=76))
    assert lib.mgpu_iqc_seek(None, 0) == 1 and lib.mgpu_iqc_destroy(None) == 1 and lib.mgpu_iqc_status(None, None) == 1
    assert lib.mgpu_host_iqc_continue(C.byref(iqc_config(4, "cf64", block=256)), None, None, 256, 0, None, None, None) == 1


@pytest.mark.parametrize("n_in", [0, 255, 257, 128, 768])
def test_every_bad_n_in_is_refused(n_in):
    """no positive multiple of B = 256, or more than max_in = 512"""
    refused(lambda: host_iqc_process(np.zeros(max(n_in, 1), np.complex128)[:n_in], 4, block=256, max_in=512))


@pytest.mark.parametrize("position", [64, 255, 2 ** 62 + 256, 2 ** 62])
def test_every_bad_position_is_refused(position):
    """a position is a multiple of B = 256, and the call ends at 2^62 at most"""
    refused(lambda: host_iqc_process(np.zeros(256, np.complex128), 4, block=256, position=position))


# ---- what the stage is for -------------------------------------------------------------------------------------------------------------------
# A station in one sideband (band-limited complex noise at 30.3 .. 32.7 kHz, R = 192 kHz), white noise as strong as the station, gain 1.1,
# 5 degrees, DC (0.3, -0.2). The image ratio is the station's own: the twin's reported coefficients applied to the impaired station alone.
# Measured with the twin over 8 seeds (profiles/iq_corrector.md): uncorrected 23.8 dB; after 65536 samples under the noise 47.1 dB at the
# least and 56.0 dB in the median; the DC's error 5.0e-3 at the most; iqc_image_db of the coefficients 23.59 .. 24.38 dB.
PLANTED_IMAGE_DB = 23.8
N_SIGNAL = 65536


def test_iqc_image_db_is_the_closed_form():
    phi = np.radians(ref.PHASE_DEG)
    assert abs(iqc_image_db(ref.GAIN * np.sin(phi), 1.0 / (ref.GAIN * np.cos(phi))) - PLANTED_IMAGE_DB) < 0.05
    assert abs(iqc_image_db(ref.GAIN * np.sin(phi), 1.0 / (ref.GAIN * np.cos(phi))) - ref.image_db(ref.impair(ref.station(N_SIGNAL, 1), dc=(0, 0)))) < 0.05
    assert iqc_image_db(0.0, 1.0) == float("inf")
    assert abs(iqc_image_db(0.0, 1.0 / 1.1) - 20 * np.log10(2.1 / 0.1)) < 1e-9


@pytest.mark.parametrize("seed", [1, 2])
def test_the_image_and_the_dc_go_down(seed):
    """at 65536 samples under noise as strong as the station: the image ratio after >= the image ratio before + 20 dB (half the margin a
    float model of the estimator showed; the bar is set against the uncorrected input), the DC residual below a tenth of the planted DC,
    and iqc_image_db of the reported coefficients within 1 dB of the planted 23.8"""
    s = ref.station(N_SIGNAL, seed)
    x = ref.impair(s + ref.white(N_SIGNAL, 1000 + seed))
    _, reports = host_iqc_process(x, 4)
    r = reports[-1]
    assert int(r["block"]) == N_SIGNAL // 4096 - 1 and not r["flags"]
    alone = ref.impair(s)
    before = ref.image_db(alone)
    after = ref.image_db(ref.apply(alone, r["dc_re"], r["dc_im"], r["skew"], r["gain"]))
    dc_error = np.hypot(r["dc_re"] - ref.DC[0], r["dc_im"] - ref.DC[1])
    described = iqc_image_db(r["skew"], r["gain"])
    print("seed %d: image ratio %.2f dB before, %.2f dB after; DC error %.2e; the coefficients describe %.2f dB" % (seed, before, after, dc_error, described))
    assert abs(before - PLANTED_IMAGE_DB) < 0.1
    assert after >= before + 20.0
    assert dc_error < 0.1 * np.hypot(*ref.DC)
    assert abs(described - PLANTED_IMAGE_DB) <= 1.0


# ---- sanitizers ----------------------------------------------------------------------------------------------------------------------------
def test_the_twin_is_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/iqc_sanitize.cpp with mercury_amd/csrc/iqc_rule.hpp built as one stand-alone program and run on the CPU in exactly sized
    buffers: three formats, B = 256 and 4096, a seeked position, a skipped block, the refusals"""
    exe = str(tmp_path / "iqc_sanitize")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "mercury_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "iqc_sanitize.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "iq corrector: clean" in out.stdout

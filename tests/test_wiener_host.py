"""CPU tests of the separable Wiener estimator's host side (include/mercury_estimator.h: MGPU_RUNG_WIENER): the tables and the normative twin
mgpu_host_wiener_estimate against a numpy restatement written from the header's rule (tests/wiener_ref.py), what the estimator is worth on
two-path frames against the 5 x 5 LS window through the same demapper and decoder, the header against the library, the twin's refusals
(the setter's need a context: tests/test_gpu_wiener.py), and the new kernels' LDS carve."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wiener_ref as W
from oraclelib import Oracle, noise_amp_for

# absolute bound on a table entry: ten times the worst error measured over GEOMETRIES x DESIGNS (1.59e-11: mode 0, the 40 dB design)
TABLE_BOUND = 1.6e-10


@pytest.fixture(scope="module")
def frames():
    out = {}
    for cfg, x in W.GEOMETRIES:
        orc = Oracle(cfg, 50, explicit=dict(x or {}))
        bb, _ = orc.gen_frame(5, 0, noise_amp_for(10.0), 1)
        out[(cfg, tuple(sorted((x or {}).items())))] = (orc, orc.rx(bb))
    return out


def _key(cfg, x):
    return (cfg, tuple(sorted((x or {}).items())))


def _library_tables(cfg, d, x):
    from mercury_amd import host_wiener_tables
    tc, fc = host_wiener_tables(cfg, d, explicit=x)
    return dict(time={tuple(m.tolist()): A for m, A in tc}, freq={tuple(m.tolist()): B for m, B in fc})


@pytest.mark.parametrize("cfg,explicit", W.GEOMETRIES)
def test_tables_equal_the_numpy_restatement(cfg, explicit, frames):
    """Measured worst absolute difference of a table entry (the library's elimination against LAPACK's inverse), per design over the five
    geometries: 3.8e-15 at 0 dB, 1.59e-11 at 40 dB, 4.0e-16 at -20 dB, 4.3e-15 for the 5 dB / 2 Hz / -100..1200 us design. The bound is ten
    times the worst, 1.6e-10. It is no looser than cond(R + s2 I) * 2^-52 * 1e3 of the worst design tested (40 dB: cond 2.1e5 in mode 0 -
    4.7e-8 -, 6.4e4 at least in every geometry - 1.4e-8), which the test asserts for that design in every geometry."""
    orc, _ = frames[_key(cfg, explicit)]
    worst_cond = 0.0
    for d in W.DESIGNS:
        want = W.np_tables(orc, d)
        got = _library_tables(cfg, d, explicit)
        assert set(got["time"]) == set(want["time"]) and set(got["freq"]) == set(want["freq"])
        err = max([np.abs(got[k][m] - want[k][m]).max() for k in ("time", "freq") for m in want[k]])
        print(cfg, explicit, d["snr_db"], "table error %.3g" % err, "cond %.3g" % want["cond"])
        assert err <= TABLE_BOUND, (d, err)
        worst_cond = max(worst_cond, want["cond"])
    assert TABLE_BOUND <= worst_cond * 2.0 ** -52 * 1e3
    # the classes: one per residue of the lattice, every member list ascending, unit gain on the model channel
    Dy = (explicit or {}).get("Dy", 3)
    got = _library_tables(cfg, W.DEFAULT, explicit)
    assert len(got["time"]) == Dy and len(got["freq"]) == Dy
    assert all(list(m) == sorted(m) for k in got for m in got[k])


@pytest.mark.parametrize("cfg,explicit", W.GEOMETRIES)
def test_twin_equals_the_numpy_restatement(cfg, explicit, frames):
    """With the library's own tables the twin and the restatement differ by the grouping of at most 17 + 16 sums alone: within
    1e-12 max|Hp| for every design (measured: 3.1e-16 .. 7.3e-16). With the restatement's tables the difference of the tables comes on top,
    to first order |dB| sum|t| + sum|B| |dA| sum|yp|; at 40 dB that term is what is measured (2.1e-11 max|Hp| in mode 0, against
    1e-12 max|Hp| for the 0 dB design: 3.8e-15), so the bound for that comparison is 1e-12 max|Hp| plus that term with the tables' measured
    difference."""
    from mercury_amd import host_wiener_estimate
    orc, ref = frames[_key(cfg, explicit)]
    pilots = np.flatnonzero(orc.frame_types() != 0)
    yp_max = np.abs(ref["grid"][pilots]).max()
    for d in W.DESIGNS:
        got = host_wiener_estimate(cfg, ref["grid"], d, explicit=explicit)
        assert got.shape == (orc.nPilots,)
        lib, own = _library_tables(cfg, d, explicit), W.np_tables(orc, d)
        same_tables = W.np_estimate(orc, ref["grid"], lib)
        scale = np.abs(same_tables).max()
        gap = np.abs(got - same_tables).max()
        assert gap <= 1e-12 * scale, (d, gap / scale)
        dA = max(np.abs(lib["time"][m] - own["time"][m]).max() for m in own["time"])
        dB = max(np.abs(lib["freq"][m] - own["freq"][m]).max() for m in own["freq"])
        n_t, n_f = max(len(m) for m in own["time"]), max(len(m) for m in own["freq"])
        t_max = max(np.abs(A).sum(axis=1).max() for A in own["time"].values()) * yp_max
        b_sum = max(np.abs(B).sum(axis=1).max() for B in own["freq"].values())
        bound = 1e-12 * scale + dB * n_f * t_max + b_sum * dA * n_t * yp_max
        gap2 = np.abs(got - W.np_estimate(orc, ref["grid"], own)).max()
        print(cfg, explicit, d["snr_db"], "gap %.3g (same tables) %.3g (own tables) of max|Hp|" % (gap / scale, gap2 / scale))
        assert gap2 <= bound, (d, gap2, bound)
    # another design is another estimate, and no design is the LS mean
    from mercury_amd import host_ls_estimate
    a, b = host_wiener_estimate(cfg, ref["grid"], W.DESIGNS[0], explicit=explicit), host_wiener_estimate(cfg, ref["grid"], W.DESIGNS[3], explicit=explicit)
    assert not np.array_equal(a, b) and not np.array_equal(a, host_ls_estimate(cfg, ref["grid"], 5, 5, explicit=explicit))
    assert np.array_equal(a, host_wiener_estimate(cfg, ref["grid"], None, explicit=explicit))          # None: the defaults


@pytest.mark.parametrize("cfg,explicit", W.GEOMETRIES)
def test_the_column_interpolation_restated_here_is_the_oracles(cfg, explicit, frames):
    """wiener_ref.interpolate_cols carries an estimate at the pilots to every cell for host_demap_csi: on the oracle's own pilot estimates
    it gives the oracle's estimate at every cell, bit for bit"""
    orc, ref = frames[_key(cfg, explicit)]
    full = ref["H_noamp"] if orc.amp_restore else ref["H"]
    pilots = np.flatnonzero(orc.frame_types() != 0)
    assert np.array_equal(W.interpolate_cols(orc, full[pilots]), full)


# ---- what it is worth ----------------------------------------------------------------------------------------------------------------
def test_value_mode_13_two_paths_2ms():
    """Mode 13 at 15 dB, second path 24 samples (2 ms) late, design SNR 5 dB, 24 frames, both estimates through host_demap_csi and the
    oracle's decoder. Measured with the finished twin: Wiener 24 of 24, the 5 x 5 LS window 10 of 24."""
    ls, wiener, _ = W.value_counts(13, 15.0, 24, 24, 5.0)
    print("mode 13, 15 dB, delay 24: 5x5", ls, "wiener", wiener)
    assert 22 <= wiener <= 24 and 8 <= ls <= 12
    assert wiener >= ls + 8


def test_value_mode_11_two_paths_2ms():
    """Mode 11 at 8 dB, delay 24, design SNR 5 dB, 24 frames. Measured: Wiener 18 of 24, the 5 x 5 LS window 0."""
    ls, wiener, _ = W.value_counts(11, 8.0, 24, 24, 5.0)
    print("mode 11, 8 dB, delay 24: 5x5", ls, "wiener", wiener)
    assert 16 <= wiener <= 20 and 0 <= ls <= 2
    assert wiener >= ls + 8


def test_value_mode_8_awgn_at_threshold():
    """Mode 8 at 0 dB on one path (AWGN), design SNR 0 dB, 32 frames. Measured: Wiener 24 of 32, the 5 x 5 LS window 21 (the 21 x 21
    window decodes 30: the price of a filter that passes 2.7 ms of delay)."""
    ls, wiener, _ = W.value_counts(8, 0.0, 0, 32, 0.0)
    print("mode 8, 0 dB, AWGN: 5x5", ls, "wiener", wiener)
    assert 22 <= wiener <= 26 and 19 <= ls <= 23
    assert wiener >= ls


# ---- header, library, refusals -------------------------------------------------------------------------------------------------------
def test_the_header_the_library_and_the_symbol_list_agree():
    from mercury_amd import ESTIMATOR_SYMBOLS, load_library
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mercury_estimator.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mgpu_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(ESTIMATOR_SYMBOLS)
    for name in ("mgpu_set_estimator_ladder_ex", "mgpu_get_estimator_ladder_ex", "mgpu_host_wiener_estimate", "mgpu_host_wiener_tables"):
        assert name in declared and hasattr(load_library(), name), name
    assert "NOT one of the reference's configurations" in open(os.path.join(root, "include", "mercury_estimator.h")).read()
    from mercury_amd.physical_layer import EstimatorRung, WienerDesign
    assert C.sizeof(WienerDesign) == 32 and C.sizeof(EstimatorRung) == 48          # int, two ints, padding, four doubles


def test_parse_ladder_takes_wiener_rungs():
    from mercury_amd import MgpuError, parse_ladder
    assert parse_ladder("21x21,wiener") == [(21, 21), ("wiener", {})]
    assert parse_ladder("wiener:tau=-333/2333,fd=0.5,snr=5") == [("wiener", dict(tau_min_us=-333.0, tau_max_us=2333.0, doppler_hz=0.5, snr_db=5.0))]
    assert parse_ladder("5x21,wiener:snr=5,5x5") == [(5, 21), ("wiener", dict(snr_db=5.0)), (5, 5)]
    assert parse_ladder("wiener:fd=2,wiener") == [("wiener", dict(doppler_hz=2.0)), ("wiener", {})]
    assert parse_ladder("21x21,5x21") == [(21, 21), (5, 21)] and parse_ladder("") == []
    for bad in ("wiener:bw=3", "wienerx", "wiener:tau=5"):
        with pytest.raises((MgpuError, ValueError)):
            parse_ladder(bad)


def test_the_twins_refusals():
    from mercury_amd import MgpuError, host_wiener_estimate, host_wiener_tables, load_library, physical_layer
    g = np.zeros(48 * 50, np.complex128)
    assert host_wiener_estimate(8, g[: 24 * 50]).shape == (400,)
    for cfg in (15, 16, 100, 101, 102, physical_layer.cfg_explicit(32, 8, 1, 0)):       # zero-forcing and MFSK modes
        with pytest.raises(MgpuError) as e:
            host_wiener_estimate(cfg, g)
        assert e.value.code == 4, cfg                                                  # MGPU_ERR_UNSUPPORTED
    nan, inf = float("nan"), float("inf")
    for bad in (dict(tau_max_us=-333.33), dict(tau_min_us=10.0, tau_max_us=5.0), dict(doppler_hz=-0.1), dict(snr_db=40.5), dict(snr_db=-20.5),
                dict(snr_db=nan), dict(tau_min_us=-inf), dict(tau_max_us=inf), dict(doppler_hz=nan)):
        with pytest.raises(MgpuError) as e:
            host_wiener_estimate(8, g, W.design(**bad))
        assert e.value.code == 1, bad                                                  # MGPU_ERR_ARG
        with pytest.raises(MgpuError) as e:
            host_wiener_tables(8, W.design(**bad))
        assert e.value.code == 1, bad
    with pytest.raises(MgpuError) as e:
        host_wiener_estimate(17, g)                                                    # no such mode
    assert e.value.code == 1
    host_wiener_estimate(8, g, W.design(snr_db=40.0)), host_wiener_estimate(8, g, W.design(snr_db=-20.0), explicit=W.DY5)   # the ends are inside
    lib = load_library()
    fn = lib.mgpu_host_wiener_tables
    n = C.c_int()
    assert fn(8, None, None, 0, 0, C.byref(n), None, None, None) == 0 and n.value == 3
    assert fn(8, None, None, 2, 0, C.byref(n), None, None, None) == 1                  # neither time nor frequency
    assert fn(8, None, None, 0, 3, None, C.byref(n), None, None) == 1 and fn(8, None, None, 1, -1, None, C.byref(n), None, None) == 1
    assert lib.mgpu_host_wiener_estimate(8, None, None, None, g.ctypes.data) == 1 and lib.mgpu_host_wiener_estimate(8, None, None, g.ctypes.data, None) == 1
    # the setters refuse a missing context before anything else
    assert lib.mgpu_set_estimator_ladder_ex(None, None, 0, 48) == 1
    assert lib.mgpu_get_estimator_ladder_ex(None, None, None, 48) == 1


def test_non_finite_input_gives_what_ieee_gives():
    from mercury_amd import host_wiener_estimate
    orc = Oracle(8, 50)
    grid = orc.rx(orc.gen_frame(5, 0, noise_amp_for(10.0), 1)[0])["grid"].copy()
    pilots = np.flatnonzero(orc.frame_types() != 0)
    clean = host_wiener_estimate(8, grid)
    grid[pilots[40]] = complex(np.nan, 1.0)             # symbol 2, one carrier: its carrier's time sums, then every symbol row they feed
    got = host_wiener_estimate(8, grid)
    bad = np.isnan(got.real) | np.isnan(got.imag)
    want = W.np_estimate(orc, grid, W.np_tables(orc, W.DEFAULT))
    assert np.array_equal(bad, np.isnan(want.real) | np.isnan(want.imag)) and 0 < bad.sum() < got.size
    assert np.array_equal(got[~bad], clean[~bad])


# ---- the kernels' LDS carve ------------------------------------------------------------------------------------------------------------
def test_the_wiener_kernels_carve_is_the_rect_and_csi_forms():
    """The two passes live in Hp and in the signed pilots' area: in every mode and on the low-density geometry, at both workgroup sizes,
    the new kernels ask for the bytes of the rectangular form (of the CSI form with that demapper), hold the two pilot-sized arrays they
    use, and leave the workgroups per compute unit what they are."""
    from mercury_amd import load_library
    lib = load_library()
    for cfg, explicit in [(c, None) for c in range(15)] + [(8, W.DY5)]:
        orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
        G = orc.Nsymb * orc.Nc
        for threads in (512, 1024):
            rect, csi = lib.mgpu_frontend_lds_bytes(G, orc.nPilots, orc.nBits, threads), lib.mgpu_frontend_csi_lds_bytes(G, orc.nPilots, orc.nBits, threads)
            w, wcsi = lib.mgpu_frontend_wiener_lds_bytes(G, orc.nPilots, orc.nBits, threads, 0), lib.mgpu_frontend_wiener_lds_bytes(G, orc.nPilots, orc.nBits, threads, 1)
            assert (w, wcsi) == (rect, csi), (cfg, threads)
            assert w >= 16 * G + 16 * orc.nPilots + 16 * orc.nPilots                     # grid, the time pass's output, the signed pilots
            assert lib.mgpu_frontend_lds_workgroups(w) == lib.mgpu_frontend_lds_workgroups(rect)
            assert lib.mgpu_frontend_lds_workgroups(wcsi) == lib.mgpu_frontend_lds_workgroups(csi)

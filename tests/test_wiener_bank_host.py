"""CPU tests of a Wiener rung's bank of designs (include/mercury_wiener_bank.h): the normative twin mgpu_host_wiener_select against a numpy
restatement written from the header's rule (tests/wiener_bank_ref.py), the pair lists against a brute-force count, the default thresholds,
what choosing per frame is worth on the four frame sets the feature was sized on, non-finite input, the header against the library,
parse_ladder's bank rung and the twin's refusals (the setter's need a context: tests/test_gpu_wiener_bank.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wiener_bank_ref as B
import wiener_ref as W
from oraclelib import Oracle, noise_amp_for


def _check_select(cfg, explicit, orc, grid, entries, tag):
    """twin against restatement on one grid: the same choice, corr within 1e-12 |R1| (only the grouping of the sums differs); a frame so
    close to a threshold that the grouping could decide it is not one these tests may use"""
    from mercury_amd import host_wiener_select
    want, got = B.np_select(orc, grid, entries), host_wiener_select(cfg, grid, entries, explicit=explicit)
    assert want["margin"] > 1e-9, (tag, "a frame too close to a threshold: replace it", want["margin"])
    assert got["design"] == want["design"], (tag, got["design"], want["design"])
    assert (got["n1"], got["n2"]) == (want["n1"], want["n2"]), tag
    scale = np.hypot(want["corr"][0], want["corr"][1])
    assert np.abs(got["corr"] - want["corr"]).max() <= 1e-12 * scale, (tag, np.abs(got["corr"] - want["corr"]).max() / scale)
    return got["design"]


# ---- the twin is the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,explicit", W.GEOMETRIES)
def test_twin_equals_the_numpy_restatement_on_every_geometry(cfg, explicit):
    """Frames of different delay spread (none, 12 and 24 samples) on every geometry, mode 0 (800 pilots) and the Dy-5 geometry included,
    where s = 5 waives the centroid test of the 16-sample design. Measured corr difference: at most 5e-16 |R1|."""
    esn0 = {0: 0.0, 8: 3.0, 11: 8.0, 13: 15.0}[cfg]
    t = B.mixed_batch(cfg, esn0, tuple(sorted((explicit or {}).items())))
    seen = set()
    for snr_db in (0.0, 5.0):
        for f, grid in enumerate(t["grid"]):
            seen.add(_check_select(cfg, explicit, t["orc"], grid, B.bank(snr_db), (cfg, explicit, f)))
    print(cfg, explicit, "designs chosen", sorted(seen))
    assert len(seen) >= 2
    # explicit thresholds are honoured: with rho_min 0 the spread test passes everything (the one-path frames get the narrow design), and
    # a threshold nothing reaches sends every frame to the fallback
    for f, grid in enumerate(t["grid"]):
        got = _check_select(cfg, explicit, t["orc"], grid, B.bank(0.0, rho=[0.0, 0.0]), (cfg, "rho 0", f))
        assert got == 0 or f >= 2
        assert _check_select(cfg, explicit, t["orc"], grid, B.bank(0.0, rho=[50.0, 50.0]), (cfg, "rho 50", f)) == 2
    # a bank of one: the fallback
    from mercury_amd import host_wiener_select
    assert host_wiener_select(cfg, t["grid"][0], B.bank()[2:], explicit=explicit)["design"] == 0


@pytest.mark.parametrize("st", B.SETS)
def test_twin_equals_the_numpy_restatement_on_the_frame_sets(st):
    """every frame of the four sets (nearest to a threshold: relative margin 0.0175, rho 0.871 against 0.894 in the 12-sample set)"""
    cfg, esn0, delay, frames, snr_db = st
    t = W.two_path_delay(cfg, esn0, delay, frames)
    for f in range(frames):
        _check_select(cfg, None, t["orc"], t["ref"][f]["grid"], B.bank(snr_db), (st, f))


def test_a_late_channel_fails_the_centroid_test():
    """a pure delay has rho = 1: only the centroid test keeps a frame whose one path sits 20 samples late from the narrow (+-4 samples)
    and from the mid (-4 .. 12) design"""
    from mercury_amd import host_wiener_select, wiener_sounding
    orc = Oracle(8, 50)
    x, _ = orc.gen_frame(5, 0, 0.0, 0)
    for delay, want in ((0, 0), (8, 1), (20, 2)):
        y = np.concatenate([np.zeros(delay, x.dtype), x[: x.size - delay]])
        grid = orc.rx(y)["grid"]
        got = _check_select(8, None, orc, grid, B.bank(), ("late", delay))
        sel = host_wiener_select(8, grid, B.bank())
        rho, delay_us = wiener_sounding(sel["corr"], sel["n1"], sel["n2"], 3)
        print("delay", delay, "design", got, "rho %.3f centroid %.1f us" % (rho, delay_us))
        assert got == want, (delay, got)
        assert abs(rho - 1.0) < 0.05 and abs(delay_us - delay / 0.012) < 60.0


# ---- pair lists --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,explicit", W.GEOMETRIES)
def test_pair_counts_equal_a_brute_force_count(cfg, explicit):
    from mercury_amd import host_wiener_bank_thresholds, host_wiener_select
    orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
    Nc, Ns = orc.Nc, orc.Nsymb
    types = orc.frame_types().reshape(Ns, Nc) != 0
    s = host_wiener_bank_thresholds(cfg, B.bank(), explicit=explicit)[1]
    assert s == (explicit or {}).get("Dy", 3)
    n1 = n2 = straddle = 0
    for i in range(Ns):
        cars = np.flatnonzero(types[i])
        k = W.carrier_bin(cars, Nc)
        for a in range(cars.size):
            for b in range(a + 1, cars.size):
                hit1 = b == a + 1 and k[b] - k[a] == s
                hit2 = b == a + 2 and k[b] - k[a] == 2 * s
                n1 += hit1
                n2 += hit2
                straddle += (hit1 or hit2) and (k[a] < 0) != (k[b] < 0)
    got = host_wiener_select(cfg, np.zeros(Ns * Nc, np.complex128), B.bank(), explicit=explicit)
    print(cfg, explicit, "s", s, "n1", n1, "n2", n2)
    assert (got["n1"], got["n2"]) == (n1, n2) and n1 > 0 and n2 > 0
    assert straddle == 0
    _, one, two = B.np_pairs(orc)
    assert (len(one), len(two)) == (n1, n2)


# ---- thresholds --------------------------------------------------------------------------------------------------------------------------
def test_default_thresholds_and_explicit_ones():
    from mercury_amd import host_wiener_bank_thresholds
    rho, s = host_wiener_bank_thresholds(8, B.bank())
    assert s == 3 and abs(rho[0] - 0.894) <= 1e-3 and abs(rho[1] - 0.607) <= 1e-3
    assert np.allclose(rho, B.np_thresholds(B.bank(), 3), rtol=1e-13, atol=0)
    rho, _ = host_wiener_bank_thresholds(8, B.bank(rho=[0.9, None]))
    assert rho[0] == 0.9 and abs(rho[1] - 0.607) <= 1e-3
    rho, s = host_wiener_bank_thresholds(8, B.bank(), explicit=W.DY5)
    assert s == 5 and np.allclose(rho, B.np_thresholds(B.bank(), 5), rtol=1e-13, atol=0)
    # a design so wide that a uniform profile of its width decorrelates within one spacing: m = 0
    rho, _ = host_wiener_bank_thresholds(8, B.bank(intervals=[(-333.33, 333.33), (0.0, 8000.0)]))
    assert abs(rho[0] - 0.957 / 2) <= 1e-3


# ---- what it is worth ------------------------------------------------------------------------------------------------------------------
# measured with the finished twin, per set: each design alone (narrow, mid, wide), the bank, the histogram of its choices
MEASURED = {B.SETS[0]: ((31, 28, 24), 31, (32, 0, 0)), B.SETS[1]: ((14, 16, 13), 16, (10, 6, 0)),
            B.SETS[2]: ((0, 16, 16), 16, (0, 11, 5)), B.SETS[3]: ((0, 0, 24), 24, (0, 0, 24))}


@pytest.mark.parametrize("st", B.SETS)
def test_value_of_choosing_per_frame(st):
    """The four sets through the twins and the oracle's decoder (tests/wiener_bank_ref.py bank_counts). Measured: AWGN 0 dB rho 0.931 ..
    1.072, alone 31 / 28 / 24, bank 31 (32 / 0 / 0); 6 samples rho 0.860 .. 0.986, alone 14 / 16 / 13, bank 16 (10 / 6 / 0); 12 samples rho
    0.575 .. 0.871, alone 0 / 16 / 16, bank 16 (0 / 11 / 5); mode 13, 24 samples rho 0.253 .. 0.352, alone 0 / 0 / 24, bank 24 (0 / 0 / 24)."""
    cfg, esn0, delay, frames, snr_db = st
    r = B.bank_counts(*st)
    alone = r["ok"].sum(axis=1)
    got = int(r["ok"][r["choice"], np.arange(frames)].sum())
    hist = np.bincount(r["choice"], minlength=3)
    print(st, "rho %.3f .. %.3f" % (r["rho"].min(), r["rho"].max()), "alone", alone.tolist(), "bank", got, "choices", hist.tolist())
    assert got >= alone.max() - 1
    if delay >= 12:
        assert hist[0] == 0
    if delay == 0:
        assert got >= alone[2] + 5
    want_alone, want_bank, _ = MEASURED[st]
    assert abs(got - want_bank) <= 2 and all(abs(int(a) - w) <= 2 for a, w in zip(alone, want_alone))


# ---- non-finite input --------------------------------------------------------------------------------------------------------------------
def test_a_nan_cell_gives_the_fallback_and_what_ieee_gives():
    from mercury_amd import host_wiener_estimate, host_wiener_select
    orc = Oracle(8, 50)
    grid = orc.rx(orc.gen_frame(5, 0, noise_amp_for(10.0), 1)[0])["grid"].copy()
    pilots = np.flatnonzero(orc.frame_types() != 0)
    assert host_wiener_select(8, grid, B.bank())["design"] == 0
    for bad in (complex(np.nan, 1.0), complex(np.inf, 0.0)):
        g = grid.copy()
        g[pilots[40]] = bad
        sel = host_wiener_select(8, g, B.bank())
        assert sel["design"] == 2 and not np.isfinite(sel["corr"]).all()
        if not np.isnan(bad.real):                                      # (the restatement's complex product makes NaNs of an Inf)
            continue
        wide = B.bank()[2][0]
        got = host_wiener_estimate(8, g, wide)
        nan = np.isnan(got.real) | np.isnan(got.imag)
        want = W.np_estimate(orc, g, W.np_tables(orc, wide))
        assert np.array_equal(nan, np.isnan(want.real) | np.isnan(want.imag)) and 0 < nan.sum() < got.size
    g = grid.copy()
    g[np.flatnonzero(orc.frame_types() == 0)[7]] = complex(np.nan, np.nan)      # a data cell is not sounded
    assert host_wiener_select(8, g, B.bank())["design"] == 0


# ---- header, library, parser, refusals -----------------------------------------------------------------------------------------------
def test_the_header_the_library_and_the_symbol_list_agree():
    from mercury_amd import WIENER_BANK_MAX, WIENER_BANK_SYMBOLS, WienerBankEntry, load_library
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = open(os.path.join(root, "include", "mercury_wiener_bank.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mgpu_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(WIENER_BANK_SYMBOLS)
    for name in declared:
        assert hasattr(load_library(), name), name
    assert "NOT one of the reference's configurations" in raw and "mgpu_pool_* does not forward the bank" in raw
    assert C.sizeof(WienerBankEntry) == 40 and WIENER_BANK_MAX == int(re.search(r"#define MGPU_WIENER_BANK_MAX (\d+)", raw).group(1)) == 4


def test_parse_ladder_takes_bank_rungs():
    from mercury_amd import MgpuError, bank_entries, parse_ladder
    spec = dict(tau=[(-333.0, 333.0), (-333.0, 1000.0), (-333.0, 2333.0)], doppler_hz=0.5, snr_db=5.0)
    assert parse_ladder("bank:tau=-333/333|-333/1000|-333/2333,fd=0.5,snr=5") == [("bank", spec)]
    assert parse_ladder("21x21,bank:tau=-333/333|-333/2333,rho=0.9,5x5") == [(21, 21), ("bank", dict(tau=[(-333.0, 333.0), (-333.0, 2333.0)], rho=[0.9])), (5, 5)]
    assert parse_ladder("bank:tau=-333/333|-333/1000|-333/2333,rho=0.9|0.6,wiener:snr=5") == [("bank", dict(tau=spec["tau"], rho=[0.9, 0.6])), ("wiener", dict(snr_db=5.0))]
    entries = bank_entries(spec)
    assert entries == [(dict(doppler_hz=0.5, snr_db=5.0, tau_min_us=lo, tau_max_us=hi), None) for lo, hi in spec["tau"]]
    assert [e[1] for e in bank_entries(dict(spec, rho=[0.9, 0.6]))] == [0.9, 0.6, None]
    for bad in ("bank", "bank:fd=2", "bank:tau=5", "bank:tau=-333/333|5", "bank:tau=-333/333|-333/1000,rho=0.9|0.6", "bank:bw=3", "bankx", "bank:tau=-1/1,rho=0.5"):
        with pytest.raises((MgpuError, ValueError)):
            parse_ladder(bad)
    # what was accepted and refused before the bank rung keeps its outcome
    assert parse_ladder("21x21,wiener") == [(21, 21), ("wiener", {})]
    assert parse_ladder("5x21,wiener:snr=5,5x5") == [(5, 21), ("wiener", dict(snr_db=5.0)), (5, 5)]
    assert parse_ladder("wiener:tau=-333/2333,fd=0.5,snr=5") == [("wiener", dict(tau_min_us=-333.0, tau_max_us=2333.0, doppler_hz=0.5, snr_db=5.0))]
    for bad in ("wiener:bw=3", "wienerx", "wiener:tau=5"):
        with pytest.raises((MgpuError, ValueError)):
            parse_ladder(bad)


def test_the_twins_refusals():
    from mercury_amd import MgpuError, WienerBankEntry, host_wiener_bank_thresholds, host_wiener_select, load_library, physical_layer
    g = np.zeros(48 * 50, np.complex128)
    assert host_wiener_select(8, g[: 24 * 50], B.bank())["design"] == 2            # an all-zero frame: 0 >= 0 passes, zr > 0 does not
    for cfg in (15, 16, 100, 101, 102, physical_layer.cfg_explicit(32, 8, 1, 0)):       # zero-forcing and MFSK modes
        for fn in (lambda: host_wiener_select(cfg, g, B.bank()), lambda: host_wiener_bank_thresholds(cfg, B.bank())):
            with pytest.raises(MgpuError) as e:
                fn()
            assert e.value.code == 4, cfg                                              # MGPU_ERR_UNSUPPORTED
    nan, inf = float("nan"), float("inf")
    wide = B.bank()[2]
    refused = [[], B.bank() + [(W.design(tau_max_us=5000.0), None), (W.design(tau_max_us=6000.0), None)],      # n = 0, n = 5
               B.bank()[::-1], [B.bank()[0], B.bank()[0], wide],                                               # widths descending, equal
               [(W.design(tau_min_us=10.0, tau_max_us=5.0), None), wide], [(W.design(tau_max_us=333.33, snr_db=41.0), None), wide],
               [(W.design(tau_max_us=333.33, doppler_hz=-1.0), None), wide], [(W.design(tau_max_us=333.33, snr_db=nan), None), wide],
               B.bank(rho=[-0.1]), B.bank(rho=[inf]), B.bank(rho=[0.9, -inf])]
    for entries in refused:
        for fn in (lambda: host_wiener_select(8, g, entries), lambda: host_wiener_bank_thresholds(8, entries)):
            with pytest.raises(MgpuError) as e:
                fn()
            assert e.value.code == 1, entries                                          # MGPU_ERR_ARG
    assert host_wiener_select(8, g, B.bank(rho=[0.0, 0.0]))["design"] == 2 and host_wiener_select(8, g, B.bank()[:2] + [(wide[0], -5.0)])["design"] == 2   # the fallback's rho_min is not read
    with pytest.raises(MgpuError) as e:
        host_wiener_select(17, g, B.bank())                                            # no such mode
    assert e.value.code == 1
    lib = load_library()
    arr, n = physical_layer._bank_array(B.bank())
    fn = lib.mgpu_host_wiener_select
    assert fn(8, None, arr, n, 40, g.ctypes.data, None, None, None, None) == 0          # every output may be NULL
    for size in (0, 32, 48):
        assert fn(8, None, arr, n, size, g.ctypes.data, None, None, None, None) == 1
    assert fn(8, None, None, n, 40, g.ctypes.data, None, None, None, None) == 1 and fn(8, None, arr, n, 40, None, None, None, None, None) == 1
    # the context's entry points refuse a missing context before anything else
    assert lib.mgpu_set_wiener_bank(None, 0, arr, n, C.sizeof(WienerBankEntry)) == 1
    assert lib.mgpu_get_wiener_bank(None, 0, arr, None, 40) == 1
    assert lib.mgpu_get_wiener_choice(None, 0, 0, None, None, None, None) == 1

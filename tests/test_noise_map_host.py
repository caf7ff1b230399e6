"""CPU tests of the noise-map demapper's host twin (include/mercury_demapper.h: mgpu_host_demap_nmap): against a numpy restatement of the
rule on the CPU oracle's stage outputs, against the channel-aware twin where no factor leaves the dead band, and on frames with a tone or a
burst inside the channel, which one variance per frame loses and the map decodes."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from noise_map_ref import INF, LS_CASES, decoded_count, disturbed, full_estimate, np_demap_nmap, np_noise_map, same_bits, twin_decode
from oraclelib import Oracle

TONE_DB = 3.0


@functools.lru_cache(maxsize=None)
def _frames(cfg, key, tone):
    """4 frames at 10 dB, with or without the +3 dB tone: (orc, explicit, [(grid, full estimate)])"""
    t = disturbed(cfg, dict(key) or None, 10.0, tone_db=TONE_DB if tone else None, frames=4)
    return t["orc"], t["explicit"], [(r["grid"], full_estimate(t["orc"], r)) for r in t["ref"]]


def _case(cfg, explicit, tone):
    return _frames(cfg, tuple(sorted((explicit or {}).items())), tone)


@pytest.mark.parametrize("tone", [False, True])
@pytest.mark.parametrize("cfg,explicit", LS_CASES)
def test_twin_equals_the_numpy_restatement(cfg, explicit, tone):
    from mercury_amd import host_demap_nmap
    orc, explicit, frames = _case(cfg, explicit, tone)
    worst = 0.0
    moved = 0
    for f, (grid, H) in enumerate(frames):
        got, sigma2, fc, fs = host_demap_nmap(cfg, grid, H, explicit=explicit)
        want, want_sigma2, want_fc, want_fs = np_demap_nmap(orc, grid, H)
        assert got.shape == (orc.nBits,) and fc.shape == (orc.Nc,) and fs.shape == (orc.Nsymb,)
        for a, b in ((sigma2, want_sigma2), (fc, want_fc), (fs, want_fs)):
            worst = max(worst, float(np.max(np.abs(np.asarray(a) - b) / np.abs(b))))
        assert np.array_equal(fc == 1.0, want_fc == 1.0) and np.array_equal(fs == 1.0, want_fs == 1.0), f     # the same side of the band
        assert got.dtype == want.dtype and same_bits(got, want), (cfg, f, np.nanmax(np.abs(got - want)))      # bit for bit, NaN where NaN
        moved += int((fc != 1.0).sum())
    print("mode %d %s tone=%s: worst relative difference of sigma2 / fc / fs %.3g, carrier factors outside the band %d" % (cfg, explicit, tone, worst, moved))
    assert worst <= 1e-12, worst
    if tone:
        assert moved > 0                                             # the tone is seen


@pytest.mark.parametrize("tone", [False, True])
@pytest.mark.parametrize("cfg,explicit", LS_CASES)
def test_an_infinite_band_gives_the_csi_llrs_bit_for_bit(cfg, explicit, tone):
    from mercury_amd import host_demap_csi, host_demap_nmap
    orc, explicit, frames = _case(cfg, explicit, tone)
    for f, (grid, H) in enumerate(frames):
        got, sigma2, fc, fs = host_demap_nmap(cfg, grid, H, dead_band=INF, explicit=explicit)
        want, want_sigma2 = host_demap_csi(cfg, grid, H, explicit=explicit)
        assert sigma2 == want_sigma2 and (fc == 1.0).all() and (fs == 1.0).all(), f
        assert got.tobytes() == want.tobytes(), (cfg, f)


def white_frames_inside_the_band(cfg, explicit, want=4, of=24):
    """(orc, explicit, the first `want` of `of` white-noise frames at 10 dB none of whose factors the restatement sees within 1e-9 of the
    band's edges or beyond them). A factor of white noise can leave the band by the chi-square tail alone - a symbol's mean is over as few as
    10 pilots with Dy 5, and the long BPSK frames have 50 + Nsymb chances each - and that is no fault: such frames are passed over."""
    t = disturbed(cfg, explicit, 10.0, frames=of)
    orc, chosen = t["orc"], []
    for f, r in enumerate(t["ref"]):
        grid, H = r["grid"], full_estimate(orc, r)
        _, _, _, raw_c, raw_s = np_noise_map(orc, grid, H)
        raw = np.concatenate([raw_c, raw_s])
        if ((raw < 2.0 * (1 - 1e-9)) & (raw * 2.0 > 1 + 1e-9)).all():
            chosen.append((f, grid, H))
        if len(chosen) == want:
            break
    return orc, t["explicit"], chosen


@pytest.mark.parametrize("cfg,explicit", LS_CASES)
def test_the_default_band_leaves_white_noise_alone(cfg, explicit):
    """On white-noise frames every factor the twin reports is exactly 1.0 and the LLRs are the CSI twin's bit for bit. The claim is made for
    the 4 frames white_frames_inside_the_band chooses: those for which the restatement says that no factor leaves the band."""
    from mercury_amd import host_demap_csi, host_demap_nmap
    orc, explicit, chosen = white_frames_inside_the_band(cfg, explicit)
    print("mode %d %s: frames" % (cfg, explicit), [f for f, _, _ in chosen])
    assert len(chosen) == 4
    for f, grid, H in chosen:
        got, sigma2, fc, fs = host_demap_nmap(cfg, grid, H, explicit=explicit)
        want, want_sigma2 = host_demap_csi(cfg, grid, H, explicit=explicit)
        assert (fc == 1.0).all() and (fs == 1.0).all() and sigma2 == want_sigma2, (cfg, f)
        assert got.tobytes() == want.tobytes(), (cfg, f)


@pytest.mark.parametrize("cfg,explicit", LS_CASES)
def test_smooth_matters_outside_the_band_and_only_there(cfg, explicit):
    from mercury_amd import host_demap_nmap
    orc, explicit, tone_frames = _case(cfg, explicit, True)
    differs = {0: 0, 2: 0}
    for grid, H in tone_frames:
        base = host_demap_nmap(cfg, grid, H, smooth=1, explicit=explicit)
        for w in (0, 2):
            other = host_demap_nmap(cfg, grid, H, smooth=w, explicit=explicit)
            assert np.array_equal(other[3], base[3])                 # the symbol factors do not depend on it
            differs[w] += int(not np.array_equal(other[2], base[2]) and other[0].tobytes() != base[0].tobytes())
    assert differs[0] == 4 and differs[2] == 4, differs
    _, _, clean_frames = _case(cfg, explicit, False)
    inside = 0
    for grid, H in clean_frames:
        base = host_demap_nmap(cfg, grid, H, smooth=1, explicit=explicit)
        for w in (0, 2):
            other = host_demap_nmap(cfg, grid, H, smooth=w, explicit=explicit)
            if (other[2] == 1.0).all() and (other[3] == 1.0).all() and (base[2] == 1.0).all():
                inside += 1
                assert other[0].tobytes() == base[0].tobytes()
    assert inside > 0


POINTS = [(8, 6.0, 3.0, 15.0, 2, 2, 26), (13, 14.0, 0.0, None, 2, 2, 24)]


@pytest.mark.parametrize("cfg,esn0,tone,burst,plain_most,csi_most,nmap_least", POINTS)
def test_disturbed_frames_one_variance_loses_decode_with_the_map(cfg, esn0, tone, burst, plain_most, csi_most, nmap_least):
    """Measured with the twin, 32 frames: mode 8 at 6 dB, tone +3 dB and burst +15 dB: the oracle alone 0, the CSI twin 0, the noise map 32;
    mode 13 at 14 dB, tone 0 dB: 0, 0 and 30."""
    t = disturbed(cfg, None, esn0, tone, burst)
    plain = int(t["plain_ok"].sum())
    csi = decoded_count(t, twin_decode(cfg, None, esn0, tone, burst, which="csi"))
    nmap = decoded_count(t, twin_decode(cfg, None, esn0, tone, burst, which="nmap"))
    print("mode %d at %.0f dB, tone %s burst %s: the oracle alone decodes %d of 32, the CSI twin %d, the noise map %d" % (cfg, esn0, tone, burst, plain, csi, nmap))
    assert plain <= plain_most and csi <= csi_most and nmap >= nmap_least, (plain, csi, nmap)


def test_white_noise_at_the_waterfall_costs_at_most_three_frames():
    """Measured with the twin, mode 8 at 0 dB, 32 frames: the oracle alone 29, the CSI twin 29, the noise map 28."""
    t = disturbed(8, None, 0.0)
    csi = decoded_count(t, twin_decode(8, None, 0.0, which="csi"))
    nmap = decoded_count(t, twin_decode(8, None, 0.0, which="nmap"))
    print("mode 8 at 0 dB, white noise: the oracle alone decodes %d of 32, the CSI twin %d, the noise map %d" % (int(t["plain_ok"].sum()), csi, nmap))
    assert nmap >= csi - 3, (csi, nmap)


def test_library_exports_what_the_header_declares_for_the_noise_map():
    from mercury_amd import DEMAPPER_SYMBOLS, DEMAPPERS, DemapperParams, NMAP_DEFAULT, load_library
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mercury_demapper.h")).read()
    assert DEMAPPERS["nmap"] == 2 and int(re.search(r"#define MGPU_DEMAP_NMAP (\d+)", text).group(1)) == 2
    for name, value in DEMAPPERS.items():
        assert int(re.search(r"#define MGPU_DEMAP_%s (\d+)" % name.upper(), text).group(1)) == value
    for word in ("dead band", "!(f > band) && !(f * band < 1)", "zero-forcing", "mgpu_pool_", "mercury_stages.h", "captured graph", "rung 0's", "MGPU_ERR_TABLES"):
        assert word in text, word
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mgpu_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(DEMAPPER_SYMBOLS)
    for name in ("mgpu_set_demapper_ex", "mgpu_get_demapper_ex", "mgpu_get_noise_map", "mgpu_host_demap_nmap"):
        assert name in declared
    lib = load_library()
    for name in declared:
        assert hasattr(lib, name), name
    fields = re.search(r"typedef struct mgpu_demapper_params \{(.*?)\}", code, re.S).group(1)
    assert re.findall(r"(double|int)\s+(\w+);", fields) == [("double", "dead_band"), ("int", "smooth")]
    assert [n for n, _ in DemapperParams._fields_] == ["dead_band", "smooth"] and C.sizeof(DemapperParams) == 16
    assert NMAP_DEFAULT == {"dead_band": 2.0, "smooth": 1}


def test_refusals():
    from mercury_amd import DemapperParams, MgpuError, host_demap_nmap, load_library
    g = np.zeros(1200, np.complex128)
    for cfg in (100, 101, 102, 15, 16):                              # MFSK: no channel estimate; zero-forcing: no residuals
        n = Oracle(cfg, 50).Nsymb * 50 if cfg < 100 else 1200
        with pytest.raises(MgpuError) as e:
            host_demap_nmap(cfg, np.zeros(n, np.complex128), np.ones(n, np.complex128))
        assert e.value.code == 4, cfg                                # MGPU_ERR_UNSUPPORTED
    for kw in (dict(dead_band=0.5), dict(dead_band=float("nan")), dict(smooth=5), dict(smooth=-1)):
        with pytest.raises(MgpuError) as e:
            host_demap_nmap(8, g, g + 1, **kw)
        assert e.value.code == 1, kw                                 # MGPU_ERR_ARG
    for kw in (dict(dead_band=1.0), dict(dead_band=INF), dict(smooth=0), dict(smooth=4)):
        host_demap_nmap(8, g, g + 1, **kw)
    lib = load_library()
    prm, llr = DemapperParams(2.0, 1), np.zeros(6000, np.float32)
    h = g + 1
    args = (8, None, g.ctypes.data, h.ctypes.data, C.byref(prm))
    assert lib.mgpu_host_demap_nmap(*args, C.sizeof(prm), llr.ctypes.data, None, None, None) == 0
    assert lib.mgpu_host_demap_nmap(8, None, g.ctypes.data, h.ctypes.data, None, C.sizeof(prm), llr.ctypes.data, None, None, None) == 0      # NULL: the defaults
    for size in (0, 8, C.sizeof(prm) + 8):
        assert lib.mgpu_host_demap_nmap(*args, size, llr.ctypes.data, None, None, None) == 1, size


def test_the_noise_map_carve_fits_and_keeps_the_csi_forms_workgroups():
    from mercury_amd import load_library
    lib = load_library()
    for cfg, explicit in [(c, None) for c in range(15)] + [(8, dict(Dy=5, Nsymb=20))]:         # every LS mode
        orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
        G = orc.Nsymb * orc.Nc
        for threads in (512, 1024):
            csi = lib.mgpu_frontend_csi_lds_bytes(G, orc.nPilots, orc.nBits, threads)
            nmap = lib.mgpu_frontend_nmap_lds_bytes(G, orc.nPilots, orc.nBits, threads)
            need = 16 * G + 16 * orc.nPilots + 16 * (orc.nPilots + 8) + 8 * orc.nPilots + 4 * orc.nData + 12 * (orc.Nc + orc.Nsymb)
            assert csi <= nmap <= 160 * 1024 and nmap >= need, (cfg, threads, csi, nmap, need)
            assert nmap - csi < 4096, (cfg, threads, csi, nmap)
            assert lib.mgpu_frontend_lds_workgroups(nmap) == lib.mgpu_frontend_lds_workgroups(csi), (cfg, threads, csi, nmap)

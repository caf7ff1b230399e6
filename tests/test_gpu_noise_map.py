"""GPU tests of the noise-map demapper (include/mercury_demapper.h MGPU_DEMAP_NMAP): the channel-aware demapper's LLRs divided by a noise
factor per carrier and per symbol, measured at the pilots.

Yardsticks: the demapped LLRs and the factors against the host twin (which tests/test_noise_map_host.py holds against a numpy restatement
on the CPU oracle) bit for bit, fed the device's own grid and H taps, in all eight kernels; the decode against twin -> the oracle's decoder
-> the oracle's tail, frame by frame, on frames with a tone and a burst that one variance per frame loses; under a ladder against the host
chain rung by rung; under diversity against the sum of its parts; with an infinite band against the channel-aware demapper byte for byte;
and with the mode off again every byte as before."""
import ctypes as C

import numpy as np
import pytest

import wiener_ref as W
from noise_map_ref import INF, LS_CASES, decoded_count, disturbed, llr_src, tail, twin_decode
from oraclelib import Oracle

pytestmark = pytest.mark.gpu

FE_THREADS = "MERCURY_FE_THREADS"   # read by mgpu_create with getenv: per context (as tests/test_gpu_wiener.py reaches the 1024-thread kernels)


def _rx(cfg, **kw):
    from mercury_amd import RxPhy
    return RxPhy(cfg, **kw)


def _record(out, f):
    return (out["payload"][f].tobytes(), out["stats"][f].tobytes())


def _same_floats(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _check_decode(orc, out, f, llr_ldpc):
    """payload, iteration count, CRC and message_decoded of row f against the oracle's decoder and tail on llr_ldpc"""
    bits, it = orc.ldpc_decode(llr_ldpc)
    payload, crc, all_zeros, decoded = tail(orc, bits)
    st = out["stats"][f]
    assert st["iterations_done"] == it and st["message_decoded"] == decoded and st["crc"] == crc and st["all_zeros"] == all_zeros, (f, st, it, decoded)
    assert np.array_equal(out["payload"][f][: payload.size], payload), f
    return decoded


def _check_against_twin(orc, cfg, explicit, out, maps, grid, H, f, **prm):
    """row f's llr_demod, llr_ldpc, factors and decode against the twin on (grid, H)"""
    from mercury_amd import host_demap_nmap
    want, sigma2, fc, fs = host_demap_nmap(cfg, grid, H, explicit=explicit, **prm)
    assert _same_floats(out["llr_demod"][f], want), (f, sigma2, np.nanmax(np.abs(out["llr_demod"][f] - want)))
    assert _same_floats(out["llr_ldpc"][f][: orc.N], want[llr_src(orc)]), f
    assert maps[0][f].tobytes() == fc.tobytes() and maps[1][f].tobytes() == fs.tobytes(), (f, np.abs(maps[0][f] - fc).max(), np.abs(maps[1][f] - fs).max())
    _check_decode(orc, out, f, want[llr_src(orc)])
    return fc, fs


# ---- 1. the LLRs and the map are the twin's ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("cfg,explicit", LS_CASES)
def test_llrs_and_factors_equal_the_host_twin_bit_for_bit(cfg, explicit, threads, monkeypatch):
    F = 8
    t = disturbed(cfg, explicit, 10.0, 3.0, 15.0, frames=F)
    orc, bb = t["orc"], t["bb"]
    monkeypatch.setenv(FE_THREADS, str(threads))
    rx = _rx(cfg, max_batch=F, explicit=explicit)
    monkeypatch.delenv(FE_THREADS)
    rx.set_demapper("csi")
    csi = rx.receive(bb, taps=True)
    rx.set_demapper("nmap")
    assert rx.demapper == "nmap" and rx.demapper_ex == ("nmap", {"dead_band": 2.0, "smooth": 1})
    out = rx.receive(bb, taps=True)
    maps = rx.noise_map()
    assert maps[0].shape == (F, orc.Nc) and maps[1].shape == (F, orc.Nsymb)
    moved_c = moved_s = 0
    for f in range(F):
        fc, fs = _check_against_twin(orc, cfg, explicit, out, maps, out["grid"][f], out["H"][f], f)
        moved_c += int((fc != 1.0).sum())
        moved_s += int((fs != 1.0).sum())
    print("mode %d %s, %d threads: carrier factors outside the band %d, symbol factors %d" % (cfg, explicit, threads, moved_c, moved_s))
    assert moved_c > 0 and moved_s > 0                                    # the tone and the burst are both seen
    # the taps and what is reported are the channel-aware demapper's (which holds them against the plain front-end's)
    for key in ("grid", "H", "eq", "variance", "agc_gain"):
        assert out[key].tobytes() == csi[key].tobytes(), key
    assert out["stats"]["variance"].tobytes() == csi["stats"]["variance"].tobytes()
    both = (out["stats"]["message_decoded"] != 0) & (csi["stats"]["message_decoded"] != 0)
    assert out["stats"]["snr_db"][both].tobytes() == csi["stats"]["snr_db"][both].tobytes()
    # a window of the rows, and other parameters
    part = rx.noise_map(first=2, count=3)
    assert part[0].tobytes() == maps[0][2:5].tobytes() and part[1].tobytes() == maps[1][2:5].tobytes()
    rx.set_demapper("nmap", dead_band=1.5, smooth=2)
    assert rx.demapper_ex == ("nmap", {"dead_band": 1.5, "smooth": 2})
    out = rx.receive(bb, taps=True)
    maps = rx.noise_map()
    for f in range(F):
        _check_against_twin(orc, cfg, explicit, out, maps, out["grid"][f], out["H"][f], f, dead_band=1.5, smooth=2)
    rx.close()


# ---- 2. the other six kernels: with the carrier-offset stage, with a Wiener rung, with both ---------------------------------------------------
@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("cfo,wiener", [(True, False), (False, True), (True, True)])
def test_kernel_combinations_equal_twins_chained_on_the_host(cfo, wiener, threads, monkeypatch):
    from mercury_amd import host_cfo_pilots, host_ls_estimate, host_wiener_estimate
    F, cfg = 8, 8
    t = disturbed(cfg, None, 10.0, 3.0, 15.0, frames=F)
    orc, bb = t["orc"], t["bb"]
    monkeypatch.setenv(FE_THREADS, str(threads))
    rx = _rx(cfg, max_batch=F)
    monkeypatch.delenv(FE_THREADS)
    plain = rx.receive(bb, taps=True)
    rx.set_demapper("nmap")
    alone = rx.receive(bb, taps=True)
    if wiener:
        rx.set_estimator_ladder([("wiener", {})])
    if cfo:
        rx.set_cfo("pilots")
    out = rx.receive(bb, taps=True)
    maps = rx.noise_map()
    steps = rx.cfo_steps(F) if cfo else None
    for f in range(F):
        grid = plain["grid"][f]
        if cfo:
            grid, step = host_cfo_pilots(cfg, grid)
            assert step == steps[f], f
        Hp = host_wiener_estimate(cfg, grid, None) if wiener else host_ls_estimate(cfg, grid, 21, 21)
        H = W.interpolate_cols(orc, Hp)
        assert np.array_equal(out["grid"][f], grid), f
        assert np.array_equal(out["H"][f], H), (f, np.abs(out["H"][f] - H).max())
        _check_against_twin(orc, cfg, None, out, maps, grid, H, f)
    assert out["llr_ldpc"].tobytes() != alone["llr_ldpc"].tobytes()       # another kernel, another result
    rx.close()


# ---- 3. what it is worth, on the device ------------------------------------------------------------------------------------------------------
def test_decode_count_on_the_device_is_the_host_tests_frame_by_frame():
    """mode 8 at 6 dB, tone +3 dB and burst +15 dB (tests/test_noise_map_host.py: the oracle alone 0, the CSI twin 0, the noise map 32 of 32)"""
    cfg, point = 8, (6.0, 3.0, 15.0)
    t, twin = disturbed(cfg, None, *point), twin_decode(cfg, None, *point)
    orc, F = t["orc"], len(t["bb"])
    rx = _rx(cfg, max_batch=F)
    plain = rx.receive(t["bb"])
    rx.set_demapper("csi")
    csi = rx.receive(t["bb"])
    rx.set_demapper("nmap")
    out = rx.receive(t["bb"], want_llr=True)
    rx.close()
    n = 0
    for f in range(F):
        llr_ldpc, bits, it = twin[f]
        assert _same_floats(out["llr_ldpc"][f][: orc.N], llr_ldpc), f
        n += int(_check_decode(orc, out, f, llr_ldpc) and np.array_equal(bits, t["bits"][f]))
    n_plain, n_csi = int((plain["stats"]["message_decoded"] != 0).sum()), int((csi["stats"]["message_decoded"] != 0).sum())
    print("mode 8 at 6 dB, tone +3 dB, burst +15 dB: plain decodes", n_plain, "of", F, "- csi", n_csi, "- nmap", n)
    assert n == decoded_count(t, twin)
    assert n_plain <= 2 and n_csi <= 2 and n >= 26, (n_plain, n_csi, n)


# ---- 4. with a ladder ------------------------------------------------------------------------------------------------------------------------
def test_ladder_records_are_those_of_the_first_rung_the_host_chain_decodes():
    from mercury_amd import host_demap_nmap, host_ls_estimate
    from test_gpu_demapper_csi import F2, _two_path_mode8
    cfg, windows = 8, [(21, 21), (5, 5)]
    # the two-path frames at 20 dB, of which the 21 x 21 window loses a third; every other frame also gets a tone 6 dB below the frame's
    # power (drawn as noise_map_ref.disturbed draws it), so that rung 0's map and rung 1's differ from all ones and from each other
    bb = _two_path_mode8().copy()
    rng, t = np.random.default_rng(11), np.arange(bb.shape[1])
    for f in range(1, F2, 2):
        fb, phase = rng.uniform(-24, 24), rng.uniform(0, 6.28)
        bb[f] += np.sqrt(np.mean(np.abs(bb[f]) ** 2) * 10.0 ** -0.6) * np.exp(1j * (2 * np.pi * fb * t / 256.0 + phase))
    orc = Oracle(cfg, 50)
    src = llr_src(orc)
    rx = _rx(cfg, max_batch=F2)
    rx.set_demapper("nmap")
    rx.set_estimator_ladder(windows)
    assert rx.demapper == "nmap"
    grids = rx.receive(bb, taps=True)["grid"]                             # (no carrier-offset stage: every rung estimates from this grid)
    whole = rx.receive(bb, want_llr=True)
    rungs = rx.last_rungs(F2)
    maps = rx.noise_map()
    seen = np.zeros(3, int)
    for f in range(F2):
        grid = grids[f]
        chain = []
        for w, h in windows:
            H = W.interpolate_cols(orc, host_ls_estimate(cfg, grid, w, h))
            llr, _, fc, fs = host_demap_nmap(cfg, grid, H)
            bits, it = orc.ldpc_decode(llr[src])
            chain.append((llr[src], fc, fs, tail(orc, bits)[3]))
        want = 0 if chain[0][3] else (1 if chain[1][3] else -1)
        assert rungs[f] == want, (f, rungs[f], want)
        seen[want + 1] += 1
        # a frame no rung decodes keeps rung 0's record
        assert _same_floats(whole["llr_ldpc"][f][: orc.N], chain[max(want, 0)][0]), f
        _check_decode(orc, whole, f, chain[max(want, 0)][0])
        assert maps[0][f].tobytes() == chain[0][1].tobytes() and maps[1][f].tobytes() == chain[0][2].tobytes(), f       # rung 0's map: retries do not write
    print("nmap, two paths, 20 dB: no rung / 21 x 21 / 5 x 5", seen, "- rung-0 factors outside the band", int((maps[0] != 1).sum()), int((maps[1] != 1).sum()))
    assert seen[1] > 0 and seen[2] > 0                                    # both rungs are exercised
    assert (maps[0][1::2] != 1).any()                                     # ... and the map is there where the tone is
    rx.close()


# ---- 5. with diversity -----------------------------------------------------------------------------------------------------------------------
def test_grouped_call_is_the_float_sum_of_the_branches_twin_llrs():
    from mercury_amd import host_demap_nmap
    from test_diversity_host import fixture_branches
    cfg, esn0, D, G = 12, 4.5, 2, 8
    orc, _, bb = fixture_branches(cfg, esn0, D, G)
    F, src = G * D, llr_src(orc)
    rx = _rx(cfg, max_batch=F)
    rx.set_demapper("nmap")
    taps = rx.receive(bb, taps=True)
    rows = np.stack([host_demap_nmap(cfg, taps["grid"][f], taps["H"][f])[0][src] for f in range(F)])
    div = rx.receive_div(bb, D, want_llr=True)
    assert _same_floats(div["llr_ldpc"][:, : orc.N], rows)                # the BRANCH LLRs
    sums = rows[0::2] + rows[1::2]                                        # float32
    for f in range(F):
        _check_decode(orc, div, f, sums[f // D])
    assert div["stats"]["variance"].tobytes() == taps["stats"]["variance"].tobytes()
    rx.close()


# ---- 6. off and on again ---------------------------------------------------------------------------------------------------------------------
def test_mode_off_is_off_again_and_a_one_frame_call_is_its_row():
    F = 8
    t = disturbed(8, None, 10.0, 3.0, 15.0, frames=F)
    bb = t["bb"]
    rx = _rx(8, max_batch=F)
    before = {}
    for name in ("maxlog", "csi"):
        rx.set_demapper(name)
        before[name] = rx.receive(bb, want_llr=True)
    rx.set_demapper("maxlog")
    assert _record(rx.receive(bb[0:1]), 0) == _record(before["maxlog"], 0)        # the one-frame call: captures its graph
    rx.set_demapper("nmap")
    on = rx.receive(bb, want_llr=True)
    assert on["llr_ldpc"].tobytes() not in (before["maxlog"]["llr_ldpc"].tobytes(), before["csi"]["llr_ldpc"].tobytes())
    assert _record(rx.receive(bb[0:1]), 0) == _record(on, 0)              # mgpu_rx_batch with one frame: not the captured graph
    one = rx.receive(bb[0:1], want_llr=True)
    assert one["llr_ldpc"][0].tobytes() == on["llr_ldpc"][0].tobytes()
    for name in ("csi", "maxlog"):
        rx.set_demapper(name)
        assert rx.demapper == name
        again = rx.receive(bb, want_llr=True)
        for key in ("payload", "stats", "llr_ldpc"):
            assert again[key].tobytes() == before[name][key].tobytes(), (name, key)
    assert _record(rx.receive(bb[0:1]), 0) == _record(before["maxlog"], 0)
    rx.close()


# ---- 7. an infinite band is the channel-aware demapper ------------------------------------------------------------------------------------------
def test_an_infinite_band_equals_csi_byte_for_byte():
    F = 8
    t = disturbed(8, None, 10.0, 3.0, 15.0, frames=F)
    rx = _rx(8, max_batch=F)
    rx.set_demapper("csi")
    csi = rx.receive(t["bb"], taps=True)
    rx.set_demapper("nmap", dead_band=INF)
    assert rx.demapper_ex == ("nmap", {"dead_band": INF, "smooth": 1})
    out = rx.receive(t["bb"], taps=True)
    for key in ("payload", "stats", "llr_demod", "llr_ldpc"):
        assert out[key].tobytes() == csi[key].tobytes(), key
    fc, fs = rx.noise_map()
    assert (fc == 1.0).all() and (fs == 1.0).all()
    rx.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    from mercury_amd import DemapperParams, MgpuError
    for cfg in (100, 101, 102, 15, 16):                                   # MFSK: no channel estimate; zero-forcing: no residuals
        rx = _rx(cfg, max_batch=2)
        if cfg < 100:
            rx.set_demapper("csi")
        before = rx.demapper
        with pytest.raises(MgpuError) as e:
            rx.set_demapper("nmap")
        assert e.value.code == 4, (cfg, str(e.value))                     # MGPU_ERR_UNSUPPORTED
        assert rx.demapper == before
        rx.close()
    rx = _rx(8, max_batch=2)
    with pytest.raises(MgpuError):
        rx.noise_map()                                                    # never set: no map
    for before in (("csi", None), ("nmap", dict(dead_band=3.0, smooth=2))):
        rx.set_demapper(before[0], **(before[1] or {}))
        state = rx.demapper_ex
        for kw in (dict(dead_band=0.5), dict(dead_band=float("nan")), dict(smooth=5), dict(smooth=-1)):
            with pytest.raises(MgpuError) as e:
                rx.set_demapper("nmap", **kw)
            assert e.value.code == 1, kw                                  # MGPU_ERR_ARG
            assert rx.demapper_ex == state
        prm = DemapperParams(2.0, 1)
        for size in (0, 8, C.sizeof(prm) + 8):
            assert rx.lib.mgpu_set_demapper_ex(rx.h, 2, C.byref(prm), size) == 1
        assert rx.lib.mgpu_set_demapper_ex(rx.h, 3, C.byref(prm), C.sizeof(prm)) == 1
        assert rx.demapper_ex == state
    assert rx.lib.mgpu_set_demapper_ex(rx.h, 2, None, C.sizeof(DemapperParams)) == 0         # NULL: the defaults
    assert rx.demapper_ex == ("nmap", {"dead_band": 2.0, "smooth": 1})
    rx.close()

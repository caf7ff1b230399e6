"""GPU tests of the separable Wiener estimator as a rung of the estimator ladder (include/mercury_estimator.h: MGPU_RUNG_WIENER).

Yardsticks: the estimate at the pilot cells against the normative host twin (which tests/test_wiener_host.py holds against a numpy
restatement) bit for bit, in all four demapper x carrier-offset forms at both workgroup sizes; with the channel-aware demapper the LLRs against
its twin and the decode against the oracle's decoder and tail; the same records from every entry point; the ladder 21x21,wiener against the
oracle's 21 x 21 estimate and the twin; what the estimator is worth on the device against the CPU count; diversity against the sum of its
parts; an all-LS ladder set through the new call against the old one; the setter's refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import wiener_ref as W
from conftest import SEED
from demapper_csi_ref import llr_src, tail
from oraclelib import Oracle, noise_amp_for

pytestmark = pytest.mark.gpu

FE_THREADS = "MERCURY_FE_THREADS"   # read by mgpu_create with getenv: per context (as tests/test_gpu_frontend_shapes.py reaches the 1024-thread kernels)
WIENER = [("wiener", {})]
W_LADDER = [(21, 21), ("wiener", {})]


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


# ---- the estimate is the twin's --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("cfg,explicit", [(8, None), (13, None), (8, W.DY5), (0, None)])
def test_estimate_equals_the_host_twin_bit_for_bit(cfg, explicit, threads, monkeypatch):
    from mercury_amd import host_demap_csi, host_wiener_estimate
    F = 8
    orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
    bb = np.stack([orc.gen_frame(SEED, f, noise_amp_for(10.0), 1)[0] for f in range(F)])
    pilots = np.flatnonzero(orc.frame_types() != 0)
    G, src = orc.Nsymb * orc.Nc, llr_src(orc)
    monkeypatch.setenv(FE_THREADS, str(threads))
    rx = _rx(cfg, max_batch=F, explicit=explicit)
    monkeypatch.delenv(FE_THREADS)
    ls = rx.receive(bb, taps=True)
    rx.set_estimator_ladder(WIENER)
    assert rx.estimator_ladder == [(0, 0)] and rx.estimator_ladder_ex == [("wiener", W.DEFAULT)]
    seen = set()
    for cfo in ("off", "pilots"):
        for demapper in ("maxlog", "csi"):
            rx.set_cfo(cfo)
            rx.set_demapper(demapper)
            out = rx.receive(bb, taps=True)
            want = np.ones((F, G), np.complex128)
            for f in range(F):
                want[f, pilots] = host_wiener_estimate(cfg, out["grid"][f], None, explicit=explicit)
            if cfo == "off":
                assert np.array_equal(out["grid"], ls["grid"])
            if demapper == "maxlog" and rx.amp_restore:      # the plain H tap is the estimate after restore_channel_amplitude (the device's own atan / sincos)
                rx._ck(rx.lib.mgpu_restore_channel_amplitude(rx.h, want.ctypes.data_as(C.c_void_p), F))
            assert np.array_equal(out["H"][:, pilots], want[:, pilots]), (cfo, demapper, np.abs(out["H"][:, pilots] - want[:, pilots]).max())
            assert not np.array_equal(out["H"][:, pilots], ls["H"][:, pilots])
            if demapper == "csi":
                for f in range(F):
                    llr, _ = host_demap_csi(cfg, out["grid"][f], out["H"][f], explicit=explicit)
                    assert _same_floats(out["llr_demod"][f], llr), (cfo, f)
                    assert _same_floats(out["llr_ldpc"][f][: orc.N], llr[src]), (cfo, f)
                    _check_decode(orc, out, f, out["llr_ldpc"][f][: orc.N])
            seen.add(out["llr_ldpc"].tobytes())
    assert len(seen) == 4                                    # four kernels, four results
    rx.close()


# ---- one record, whatever the entry point ------------------------------------------------------------------------------------------------
def test_records_are_the_same_from_every_entry_point(monkeypatch):
    import torch
    from mercury_amd import STATS_DTYPE
    F = 8
    orc = Oracle(8, 50)
    bb = np.stack([orc.gen_frame(SEED, f, noise_amp_for(3.0 if f < 6 else -15.0), 1)[0] for f in range(F)])
    rx = _rx(8, max_batch=F)
    rx.set_estimator_ladder(WIENER)
    whole = rx.receive(bb, want_llr=True)
    decoded = whole["stats"]["message_decoded"] != 0
    assert decoded[:6].sum() >= 4 and decoded[6:].sum() == 0
    assert np.array_equal(rx.last_rungs(F), np.where(decoded, 0, -1))
    d_bb = torch.from_numpy(bb.view(np.float64).copy()).cuda()
    d_payload = torch.zeros((F, rx.payload_stride), dtype=torch.uint8, device="cuda")
    d_stats = torch.zeros(F * STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    rx.receive_dev(d_bb.data_ptr(), F, d_payload.data_ptr(), d_stats.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)      # mgpu_rx_batch_dev
    torch.cuda.synchronize()
    dev = dict(payload=d_payload.cpu().numpy(), stats=d_stats.cpu().numpy().view(STATS_DTYPE))
    taps = rx.receive(bb, taps=True)                                      # the taps entry point
    monkeypatch.setenv("MERCURY_RX_CHUNK", "3")
    chunked = rx.receive(bb)                                              # the chunked host path
    monkeypatch.delenv("MERCURY_RX_CHUNK")
    for f in range(F):
        single = rx.receive(bb[f:f + 1])                                  # the one-frame call: no captured graph while a ladder is set
        for name, out, k in (("dev", dev, f), ("taps", taps, f), ("chunked", chunked, f), ("one frame", single, 0)):
            assert _record(out, k) == _record(whole, f), (name, f)
    assert taps["llr_ldpc"].tobytes() == whole["llr_ldpc"].tobytes()
    rx.close()


# ---- the ladder ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ladder_reference():
    """the delay-12 mode-8 frames at 20 dB of tests/test_gpu_estimator_ladder.py under the channel-aware demapper, whose twin takes any estimate:
    per frame the chain of the oracle's 21 x 21 estimate and the chain of the Wiener twin, each through host_demap_csi, the oracle's decoder
    and its tail. Measured on the CPU: the 21 x 21 chain decodes 22 of the 32 frames, the Wiener chain all 32."""
    from mercury_amd import host_wiener_estimate
    from test_gpu_estimator_ladder import F2, _two_path
    t = _two_path()
    orc = Oracle(8, 50)
    chains = []
    for f in range(F2):
        ref = t["ref21"][f]
        rung0 = W.decode_with(orc, ref["grid"], ref["H_noamp"] if orc.amp_restore else ref["H"])
        rung1 = W.decode_with(orc, ref["grid"], W.interpolate_cols(orc, host_wiener_estimate(8, ref["grid"])))
        chains.append((rung0, rung1))
    ok0 = np.array([tail(orc, c[0][2])[3] for c in chains], bool)
    ok1 = np.array([tail(orc, c[1][2])[3] for c in chains], bool)
    assert (~ok0).sum() >= 3 and ok1[~ok0].all(), (ok0.sum(), ok1.sum())
    return dict(bb=t["bb"], orc=orc, chains=chains, ok0=ok0, F=F2)


@functools.lru_cache(maxsize=None)
def _ladder_gpu():
    t = _ladder_reference()
    rx = _rx(8, max_batch=t["F"])
    rx.set_demapper("csi")
    rx.set_estimator_ladder(W_LADDER)
    out = rx.receive(t["bb"], want_llr=True)
    out["rungs"] = rx.last_rungs(t["F"])
    out["counters"] = rx.ladder_counters()
    rx.close()
    return out



def test_ladder_21x21_wiener_against_the_oracle_and_the_twin():
    t, out = _ladder_reference(), _ladder_gpu()
    orc = t["orc"]
    for f in range(t["F"]):
        rung = 0 if t["ok0"][f] else 1
        assert out["rungs"][f] == rung, (f, out["rungs"][f])
        llr_demod, llr_ldpc, bits, it = t["chains"][f][rung]
        assert _same_floats(out["llr_ldpc"][f][: orc.N], llr_ldpc), (f, rung)
        assert _check_decode(orc, out, f, llr_ldpc) == 1, f
    by, frames = out["counters"]
    assert frames == t["F"] and by[0] == t["ok0"].sum() and by[1] == (~t["ok0"]).sum() and by[2:].sum() == 0 and by.sum() == frames


def test_a_frame_of_the_ladder_does_not_depend_on_its_batch():
    t, whole = _ladder_reference(), _ladder_gpu()
    F = t["F"]
    rx = _rx(8, max_batch=F)
    rx.set_demapper("csi")
    rx.set_estimator_ladder(W_LADDER)
    order = list(range(F))[::-1]
    out = rx.receive(t["bb"][order], want_llr=True)
    rungs = rx.last_rungs(F)
    for k, f in enumerate(order):
        assert _record(out, k) == _record(whole, f) and out["llr_ldpc"][k].tobytes() == whole["llr_ldpc"][f].tobytes() and rungs[k] == whole["rungs"][f], (k, f)
    for lo, hi in ((0, 5), (5, F)):
        out = rx.receive(t["bb"][lo:hi], want_llr=True)
        rungs = rx.last_rungs(hi - lo)
        for k, f in enumerate(range(lo, hi)):
            assert _record(out, k) == _record(whole, f) and out["llr_ldpc"][k].tobytes() == whole["llr_ldpc"][f].tobytes() and rungs[k] == whole["rungs"][f], (lo, f)
    out = rx.receive(t["bb"])                                             # no LLRs asked for: the chunked host path
    for f in range(F):
        assert _record(out, f) == _record(whole, f), f
    assert np.array_equal(rx.last_rungs(F), whole["rungs"])
    for f in (int(np.flatnonzero(t["ok0"])[0]), int(np.flatnonzero(~t["ok0"])[0])):       # one-frame calls: a rung-0 and a rung-1 frame
        assert _record(rx.receive(t["bb"][f:f + 1]), 0) == _record(whole, f), f
        assert rx.last_rungs(1)[0] == whole["rungs"][f]
    rx.close()


# ---- what it is worth, on the device -------------------------------------------------------------------------------------------------
def test_value_on_the_device_is_the_cpu_count():
    """mode 13 at 15 dB, second path 24 samples late, design SNR 5 dB (tests/test_wiener_host.py: Wiener 24 of 24, 5 x 5 10 of 24): estimate
    and LLRs are the twins' bit for bit, so the device decodes the frames the CPU chain decodes"""
    frames = 24
    ls, wiener, verdicts = W.value_counts(13, 15.0, 24, frames, 5.0)
    t = W.two_path_delay(13, 15.0, 24, frames)
    orc = t["orc"]
    rx = _rx(13, max_batch=frames)
    rx.set_demapper("csi")
    rx.set_estimator_ladder([("wiener", dict(snr_db=5.0))])
    out = rx.receive(t["bb"])
    rx.set_estimator_ladder([(5, 5)])
    out5 = rx.receive(t["bb"])
    rx.close()

    def right(o, f):
        sent = tail(orc, t["bits"][f])[0]
        return bool(o["stats"]["message_decoded"][f] != 0 and np.array_equal(o["payload"][f][: sent.size], sent))

    got = [right(out, f) for f in range(frames)]
    print("mode 13, 15 dB, delay 24 on the device: wiener", sum(got), "5x5", sum(right(out5, f) for f in range(frames)))
    assert tuple(got) == verdicts and sum(got) == wiener
    assert sum(right(out5, f) for f in range(frames)) == ls


# ---- diversity -------------------------------------------------------------------------------------------------------------------------
def test_diversity_with_a_one_rung_wiener_ladder_is_the_sum_of_its_branches():
    from mercury_amd import host_llr_combine
    from test_diversity_host import fixture_branches
    cfg, esn0, D, G = 12, 4.5, 2, 8
    orc, _, bb = fixture_branches(cfg, esn0, D, G)
    F = G * D
    rx = _rx(cfg, max_batch=F)
    rx.set_estimator_ladder(WIENER)
    rows = np.stack([rx.receive(bb[f:f + 1], want_llr=True)["llr_ldpc"][0] for f in range(F)])      # single calls
    plain = rx.receive(bb, want_llr=True)
    assert plain["llr_ldpc"].tobytes() == rows.tobytes()
    div = rx.receive_div(bb, D, want_llr=True)
    assert div["llr_ldpc"].tobytes() == rows.tobytes()                    # the BRANCH LLRs
    sums = host_llr_combine(rows, D=D)
    for g in range(G):
        for f in range(g * D, g * D + D):
            _check_decode(orc, div, f, sums[g][: orc.N])
    assert div["stats"]["variance"].tobytes() == plain["stats"]["variance"].tobytes()
    rx.set_estimator_ladder([])
    assert rx.receive_div(bb, D, want_llr=True)["llr_ldpc"].tobytes() != rows.tobytes()
    rx.close()


# ---- off means off ---------------------------------------------------------------------------------------------------------------------
def _set_ex(rx, rungs, size=None):
    from mercury_amd.physical_layer import EstimatorRung, LsWindow, WienerDesign
    arr = (EstimatorRung * max(len(rungs), 1))()
    for i, (kind, window, d) in enumerate(rungs):
        arr[i] = EstimatorRung(kind, LsWindow(*window), WienerDesign(*d))
    return rx.lib.mgpu_set_estimator_ladder_ex(rx.h, arr, len(rungs), C.sizeof(EstimatorRung) if size is None else size)


DEFAULT4 = (-333.33, 2333.33, 0.5, 0.0)


def test_an_all_ls_ladder_through_the_new_call_is_the_old_call():
    from test_gpu_estimator_ladder import F2, _two_path
    bb = _two_path()["bb"]
    rx = _rx(8, max_batch=F2)
    never = rx.receive(bb, want_llr=True)
    rx.set_estimator_ladder([(21, 21), (5, 21)])
    old = rx.receive(bb, want_llr=True)
    old_rungs = rx.last_rungs(F2)
    assert (old_rungs == 1).any()
    assert _set_ex(rx, [(0, (20, 20), (0, 0, 0, 0)), (0, (5, 21), (9e9, -1.0, -5.0, 99.0))]) == 0     # an LS rung's design is not looked at
    assert rx.estimator_ladder == [(21, 21), (5, 21)] and rx.estimator_ladder_ex == [(21, 21), (5, 21)]
    new = rx.receive(bb, want_llr=True)
    for key in ("payload", "stats", "llr_ldpc"):
        assert new[key].tobytes() == old[key].tobytes(), key
    assert np.array_equal(rx.last_rungs(F2), old_rungs)
    assert _set_ex(rx, []) == 0 and rx.estimator_ladder == []
    again = rx.receive(bb, want_llr=True)
    for key in ("payload", "stats", "llr_ldpc"):
        assert again[key].tobytes() == never[key].tobytes(), key
    rx.set_estimator_ladder(WIENER)                                      # and a Wiener rung set and cleared leaves nothing behind
    assert rx.receive(bb, want_llr=True)["llr_ldpc"].tobytes() != never["llr_ldpc"].tobytes()
    rx.set_estimator_ladder([])
    assert rx.receive(bb, want_llr=True)["llr_ldpc"].tobytes() == never["llr_ldpc"].tobytes()
    assert _record(rx.receive(bb[3:4]), 0) == _record(never, 3)          # the one-frame graph is back
    rx.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_untouched():
    from mercury_amd import MgpuError, physical_layer
    for cfg in (15, 16, physical_layer.cfg_explicit(32, 8, 1, 0), 100, 102):       # zero-forcing and MFSK modes
        rx = _rx(cfg, max_batch=2)
        with pytest.raises(MgpuError) as e:
            rx.set_estimator_ladder(WIENER)
        assert "mgpu error 4" in str(e.value), (cfg, str(e.value))            # MGPU_ERR_UNSUPPORTED
        assert _set_ex(rx, []) == 0 and rx.estimator_ladder == []
        rx.close()
    rx = _rx(8, max_batch=2)
    set_to = [(21, 21), ("wiener", dict(W.DEFAULT, snr_db=5.0))]
    rx.set_estimator_ladder([(21, 21), ("wiener", dict(snr_db=5.0))])
    assert rx.estimator_ladder_ex == set_to and rx.estimator_ladder == [(21, 21), (0, 0)]
    nan = float("nan")
    bad = [[(1, (0, 0), (10.0, 5.0, 0.5, 0.0))], [(1, (0, 0), (-333.33, 2333.33, -1.0, 0.0))], [(1, (0, 0), (-333.33, 2333.33, 0.5, 41.0))],
           [(1, (0, 0), (-333.33, 2333.33, 0.5, -21.0))], [(1, (0, 0), (nan, 2333.33, 0.5, 0.0))], [(0, (21, 21), DEFAULT4), (1, (0, 0), (0.0, 0.0, 0.5, 0.0))],
           [(2, (21, 21), DEFAULT4)], [(-1, (21, 21), DEFAULT4)], [(0, (23, 21), DEFAULT4)], [(1, (0, 0), DEFAULT4)] * 5]
    for rungs in bad:
        assert _set_ex(rx, rungs) == 1, rungs                                 # MGPU_ERR_ARG
        assert rx.estimator_ladder_ex == set_to
    for size in (0, 8, 40, 56):                                               # not this library's sizeof(mgpu_estimator_rung)
        assert _set_ex(rx, [(1, (0, 0), DEFAULT4)], size=size) == 1, size
        assert rx.estimator_ladder_ex == set_to
    from mercury_amd.physical_layer import EstimatorRung
    arr, n = (EstimatorRung * 4)(), C.c_int()
    assert rx.lib.mgpu_get_estimator_ladder_ex(rx.h, arr, C.byref(n), 40) == 1
    with pytest.raises(MgpuError):
        rx.set_estimator_ladder([("wiener", dict(bandwidth=3.0))])
    rx.close()

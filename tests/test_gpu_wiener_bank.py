"""GPU tests of a Wiener rung's bank of designs (include/mercury_wiener_bank.h).

Yardsticks: the choice, the four sums and the pair counts against the normative host twin (which tests/test_wiener_bank_host.py holds against
a numpy restatement) bit for bit, and the estimate at the pilot cells against host_wiener_estimate of the chosen design, in all twelve Wiener
kernels (three demappers x carrier-offset stage off / on x both workgroup sizes), on batches whose frames choose different designs: the place
the kernel can go wrong is the per-frame table base. A one-entry bank against the plain rung; the same record whatever the batch and the
entry point; the ladder 21x21,bank against the oracle's 21 x 21 estimate and the twins; diversity against the sum of its parts; what the
bank is worth on the device against the CPU verdicts; the setter's refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import wiener_bank_ref as B
import wiener_ref as W
from demapper_csi_ref import tail
from oraclelib import Oracle

pytestmark = pytest.mark.gpu

FE_THREADS = "MERCURY_FE_THREADS"   # read by mgpu_create with getenv: per context (as tests/test_gpu_wiener.py reaches the 1024-thread kernels)
BANK = B.bank(5.0)
BANK_RUNG = ("bank", dict(tau=B.INTERVALS, doppler_hz=0.5, snr_db=5.0))
DESIGNS = [d for d, _ in BANK]


def _rx(cfg, **kw):
    from mercury_amd import RxPhy
    return RxPhy(cfg, **kw)


def _record(out, f):
    return (out["payload"][f].tobytes(), out["stats"][f].tobytes())


def _same_floats(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _check_decode(orc, out, f, llr_ldpc):
    bits, it = orc.ldpc_decode(llr_ldpc)
    payload, crc, all_zeros, decoded = tail(orc, bits)
    st = out["stats"][f]
    assert st["iterations_done"] == it and st["message_decoded"] == decoded and st["crc"] == crc and st["all_zeros"] == all_zeros, (f, st, it, decoded)
    assert np.array_equal(out["payload"][f][: payload.size], payload), f
    return decoded


@functools.lru_cache(maxsize=None)
def _mixed(cfg, explicit=()):
    """F = 6 frames of which two each want the narrow, the mid and the wide design. Mode 8: two frames each of the AWGN set and of the
    12-sample set of wiener_ref.two_path_delay, and two made the same way with the second path 24 samples late; the other geometries:
    wiener_bank_ref.mixed_batch. -> (oracle, bb [6, samples])"""
    esn0 = {0: 0.0, 8: 3.0, 13: 15.0}[cfg]
    t = B.mixed_batch(cfg, esn0, explicit)
    if cfg != 8 or explicit:
        return t["orc"], t["bb"]
    return t["orc"], np.concatenate([W.two_path_delay(8, 0.0, 0, 32)["bb"][:2], W.two_path_delay(8, 3.0, 12, 16)["bb"][:2], t["bb"][4:]])


def _check_choice(rx, cfg, explicit, out, F, first=0):
    """rows first .. first + F - 1 of the context's choice arrays against the twin on the grid tap of rows 0 .. F - 1 -> the designs"""
    from mercury_amd import host_wiener_select
    ch = rx.wiener_choice(first, F)
    for f in range(F):
        want = host_wiener_select(cfg, out["grid"][f], BANK, explicit=explicit)
        assert ch["design"][f] == want["design"], (f, ch["design"][f], want["design"])
        assert ch["corr"][f].tobytes() == want["corr"].tobytes(), (f, ch["corr"][f], want["corr"])
        assert (ch["n1"], ch["n2"]) == (want["n1"], want["n2"])
    return ch["design"]


# ---- choice and estimate are the twins' ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("cfg,explicit", [(8, None), (0, None), (8, W.DY5)])
def test_choice_and_estimate_equal_the_host_twins_bit_for_bit(cfg, explicit, threads, monkeypatch):
    from mercury_amd import host_wiener_estimate
    F = 6
    orc, bb = _mixed(cfg, tuple(sorted((explicit or {}).items())))
    pilots = np.flatnonzero(orc.frame_types() != 0)
    G = orc.Nsymb * orc.Nc
    monkeypatch.setenv(FE_THREADS, str(threads))
    rx = _rx(cfg, max_batch=F, explicit=explicit)
    monkeypatch.delenv(FE_THREADS)
    rx.set_estimator_ladder([BANK_RUNG])
    assert rx.estimator_ladder_ex == [("wiener", DESIGNS[-1])] and [d for d, _ in rx.wiener_bank(0)] == DESIGNS
    seen = set()
    for cfo in ("off", "pilots"):
        for demapper in ("maxlog", "csi", "nmap"):
            rx.set_cfo(cfo)
            rx.set_demapper(demapper)
            out = rx.receive(bb, taps=True)
            design = _check_choice(rx, cfg, explicit, out, F)
            print(cfg, explicit, threads, cfo, demapper, "designs", design.tolist())
            assert len(set(design.tolist())) >= 2
            want = np.ones((F, G), np.complex128)
            for f in range(F):
                want[f, pilots] = host_wiener_estimate(cfg, out["grid"][f], DESIGNS[design[f]], explicit=explicit)
            if demapper == "maxlog" and rx.amp_restore:      # the plain H tap is the estimate after restore_channel_amplitude
                rx._ck(rx.lib.mgpu_restore_channel_amplitude(rx.h, want.ctypes.data_as(C.c_void_p), F))
            assert np.array_equal(out["H"][:, pilots], want[:, pilots]), (cfo, demapper, np.abs(out["H"][:, pilots] - want[:, pilots]).max())
            seen.add(out["llr_ldpc"].tobytes())
    assert len(seen) == 6                                    # six kernels, six results
    rx.close()


# ---- a bank of one is the plain rung -----------------------------------------------------------------------------------------------------
def test_a_one_entry_bank_and_a_removed_bank_are_the_plain_rung():
    orc, bb = _mixed(8)
    F = bb.shape[0]
    rx = _rx(8, max_batch=F)
    rx.set_demapper("csi")
    plain = {}
    for d, design in enumerate(DESIGNS):
        rx.set_estimator_ladder([("wiener", design)])
        plain[d] = rx.receive(bb, want_llr=True)
    assert plain[0]["llr_ldpc"].tobytes() != plain[2]["llr_ldpc"].tobytes()
    rx.set_estimator_ladder([("wiener", DESIGNS[2])])
    for d in (0, 1):
        rx.set_wiener_bank(0, [BANK[d]])
        assert [e[0] for e in rx.wiener_bank(0)] == [DESIGNS[d]] and rx.estimator_ladder_ex == [("wiener", DESIGNS[2])]
        out = rx.receive(bb, want_llr=True)
        for key in ("payload", "stats", "llr_ldpc"):
            assert out[key].tobytes() == plain[d][key].tobytes(), (d, key)
        assert not rx.wiener_choice(0, F)["design"].any()
    rx.set_wiener_bank(0, BANK)
    banked = rx.receive(bb, want_llr=True)
    design = rx.wiener_choice(0, F)["design"]
    for f in range(F):                                      # and a frame of the bank is that frame under its design alone
        assert _record(banked, f) == _record(plain[design[f]], f) and banked["llr_ldpc"][f].tobytes() == plain[design[f]]["llr_ldpc"][f].tobytes(), f
    rx.set_wiener_bank(0, [])
    assert rx.wiener_bank(0) == []
    out = rx.receive(bb, want_llr=True)
    for key in ("payload", "stats", "llr_ldpc"):
        assert out[key].tobytes() == plain[2][key].tobytes(), key
    rx.close()


# ---- one record, whatever the batch and the entry point ------------------------------------------------------------------------------------
def test_a_frame_does_not_depend_on_its_batch_or_on_the_entry_point():
    import torch
    from mercury_amd import STATS_DTYPE
    orc, bb = _mixed(8)
    F = bb.shape[0]
    rx = _rx(8, max_batch=F)
    rx.set_estimator_ladder([BANK_RUNG])
    whole = rx.receive(bb, want_llr=True)
    design = rx.wiener_choice(0, F)["design"].copy()
    corr = rx.wiener_choice(0, F)["corr"].copy()
    assert len(set(design.tolist())) >= 2
    order = [3, 5, 0, 4, 1, 2]
    out = rx.receive(bb[order], want_llr=True)
    ch = rx.wiener_choice(0, F)
    for k, f in enumerate(order):
        assert _record(out, k) == _record(whole, f) and out["llr_ldpc"][k].tobytes() == whole["llr_ldpc"][f].tobytes(), (k, f)
        assert ch["design"][k] == design[f] and ch["corr"][k].tobytes() == corr[f].tobytes(), (k, f)
    for lo, hi in ((0, 2), (2, F)):
        out = rx.receive(bb[lo:hi], want_llr=True)
        ch = rx.wiener_choice(0, hi - lo)
        for k, f in enumerate(range(lo, hi)):
            assert _record(out, k) == _record(whole, f) and out["llr_ldpc"][k].tobytes() == whole["llr_ldpc"][f].tobytes(), (lo, f)
            assert ch["design"][k] == design[f] and ch["corr"][k].tobytes() == corr[f].tobytes(), (lo, f)
    for f in range(F):
        assert _record(rx.receive(bb[f:f + 1]), 0) == _record(whole, f), f
        assert rx.wiener_choice(0, 1)["design"][0] == design[f]
    d_bb = torch.from_numpy(bb.view(np.float64).copy()).cuda()
    d_payload = torch.zeros((F, rx.payload_stride), dtype=torch.uint8, device="cuda")
    d_stats = torch.zeros(F * STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    rx.receive_dev(d_bb.data_ptr(), F, d_payload.data_ptr(), d_stats.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)      # mgpu_rx_batch_dev
    torch.cuda.synchronize()
    dev = dict(payload=d_payload.cpu().numpy(), stats=d_stats.cpu().numpy().view(STATS_DTYPE))
    assert np.array_equal(rx.wiener_choice(0, F)["design"], design)
    taps = rx.receive(bb, taps=True)                                      # the taps entry point
    assert np.array_equal(_check_choice(rx, 8, None, taps, F), design)
    for f in range(F):
        assert _record(dev, f) == _record(whole, f) and _record(taps, f) == _record(whole, f), f
    assert taps["llr_ldpc"].tobytes() == whole["llr_ldpc"].tobytes()
    rx.close()


# ---- the ladder ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ladder_reference():
    """the delay-12 mode-8 frames at 20 dB of tests/test_gpu_estimator_ladder.py under the channel-aware demapper: per frame the chain of
    the oracle's 21 x 21 estimate, and the chain of the twins - the bank's choice, then the Wiener estimate of the chosen design -, each
    through host_demap_csi, the oracle's decoder and its tail"""
    from mercury_amd import host_wiener_estimate, host_wiener_select
    from test_gpu_estimator_ladder import F2, _two_path
    t = _two_path()
    orc = Oracle(8, 50)
    chains, choice = [], []
    for f in range(F2):
        ref = t["ref21"][f]
        rung0 = W.decode_with(orc, ref["grid"], ref["H_noamp"] if orc.amp_restore else ref["H"])
        d = host_wiener_select(8, ref["grid"], BANK)["design"]
        rung1 = W.decode_with(orc, ref["grid"], W.interpolate_cols(orc, host_wiener_estimate(8, ref["grid"], DESIGNS[d])))
        chains.append((rung0, rung1))
        choice.append(d)
    ok0 = np.array([tail(orc, c[0][2])[3] for c in chains], bool)
    ok1 = np.array([tail(orc, c[1][2])[3] for c in chains], bool)
    assert (~ok0).sum() >= 3 and ok1[~ok0].all(), (ok0.sum(), ok1.sum())
    return dict(bb=t["bb"], orc=orc, chains=chains, ok0=ok0, F=F2, choice=np.array(choice))


def test_ladder_21x21_bank_against_the_oracle_and_the_twins():
    from mercury_amd import MgpuError
    t = _ladder_reference()
    orc, F = t["orc"], t["F"]
    rx = _rx(8, max_batch=F)
    rx.set_demapper("csi")
    rx.set_estimator_ladder([(21, 21), BANK_RUNG])
    assert rx.estimator_ladder_ex == [(21, 21), ("wiener", DESIGNS[-1])] and len(rx.wiener_bank(1)) == 3
    out = rx.receive(t["bb"], want_llr=True)
    rungs = rx.last_rungs(F)
    for f in range(F):
        rung = 0 if t["ok0"][f] else 1
        assert rungs[f] == rung, (f, rungs[f])
        llr_ldpc = t["chains"][f][rung][1]
        assert _same_floats(out["llr_ldpc"][f][: orc.N], llr_ldpc), (f, rung, t["choice"][f])
        assert _check_decode(orc, out, f, llr_ldpc) == 1, f
    with pytest.raises(MgpuError):                          # rung 0 has no bank
        rx.wiener_choice(0, F)
    # as rung 0, with a retry behind it: the choices are rung 0's
    rx.set_estimator_ladder([BANK_RUNG, (5, 5)])
    bb = t["bb"][:8].copy()
    rng = np.random.default_rng(3)                           # noise alone, nothing to decode: the frame goes to the retry
    bb[1] = rng.standard_normal(bb.shape[1]) + 1j * rng.standard_normal(bb.shape[1])
    first = rx.receive(bb, taps=True)
    assert (rx.last_rungs(8) != 0).any()
    design = _check_choice(rx, 8, None, first, 8)
    assert np.array_equal(design[[0, 2, 3]], t["choice"][[0, 2, 3]])
    rx.close()


# ---- diversity -------------------------------------------------------------------------------------------------------------------------
def test_diversity_with_a_one_rung_bank_ladder_is_the_sum_of_its_branches():
    from mercury_amd import host_llr_combine
    from test_diversity_host import fixture_branches
    cfg, esn0, D, G = 12, 4.5, 2, 8
    orc, _, bb = fixture_branches(cfg, esn0, D, G)
    F = G * D
    rx = _rx(cfg, max_batch=F)
    rx.set_estimator_ladder([BANK_RUNG])
    rows = np.stack([rx.receive(bb[f:f + 1], want_llr=True)["llr_ldpc"][0] for f in range(F)])      # single calls
    plain = rx.receive(bb, want_llr=True)
    design = rx.wiener_choice(0, F)["design"].copy()
    assert plain["llr_ldpc"].tobytes() == rows.tobytes()
    div = rx.receive_div(bb, D, want_llr=True)
    assert div["llr_ldpc"].tobytes() == rows.tobytes()                    # the BRANCH LLRs
    assert np.array_equal(rx.wiener_choice(0, F)["design"], design)
    sums = host_llr_combine(rows, D=D)
    for g in range(G):
        for f in range(g * D, g * D + D):
            _check_decode(orc, div, f, sums[g][: orc.N])
    assert div["stats"]["variance"].tobytes() == plain["stats"]["variance"].tobytes()
    rx.set_estimator_ladder([("wiener", DESIGNS[-1])])
    wide = rx.receive_div(bb, D, want_llr=True)["llr_ldpc"]
    changed = [f for f in range(F) if wide[f].tobytes() != rows[f].tobytes()]
    assert sorted(changed) == sorted(np.flatnonzero(design != 2).tolist())
    rx.close()


# ---- what it is worth, on the device -------------------------------------------------------------------------------------------------
def test_value_on_the_device_is_the_cpu_verdict_frame_by_frame():
    """the 32-frame AWGN set at 0 dB (tests/test_wiener_bank_host.py: the bank decodes 31, the wide design alone 24): choice, estimate and
    LLRs are the twins' bit for bit, so the device decodes the frames the CPU chain decodes"""
    st = B.SETS[0]
    cfg, esn0, delay, frames, snr_db = st
    r = B.bank_counts(*st)
    t = W.two_path_delay(cfg, esn0, delay, frames)
    orc = t["orc"]
    rx = _rx(cfg, max_batch=frames)
    rx.set_demapper("csi")
    rx.set_estimator_ladder([("bank", dict(tau=B.INTERVALS, snr_db=snr_db))])
    out = rx.receive(t["bb"])
    design = rx.wiener_choice(0, frames)["design"]
    rx.close()
    want = r["ok"][r["choice"], np.arange(frames)]
    got = []
    for f in range(frames):
        sent = tail(orc, t["bits"][f])[0]
        got.append(bool(out["stats"]["message_decoded"][f] != 0 and np.array_equal(out["payload"][f][: sent.size], sent)))
    print("mode 8, 0 dB, AWGN on the device: bank", sum(got), "choices", np.bincount(design, minlength=3).tolist())
    assert np.array_equal(design, r["choice"])
    assert got == want.tolist() and sum(got) >= r["ok"][2].sum() + 5


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _set_bank(rx, rung, entries, n=None, size=None):
    from mercury_amd.physical_layer import WienerBankEntry, _bank_array
    arr, count = _bank_array(entries)
    return rx.lib.mgpu_set_wiener_bank(rx.h, rung, arr, count if n is None else n, C.sizeof(WienerBankEntry) if size is None else size)


def test_refusals_leave_the_context_untouched():
    from mercury_amd import MgpuError, physical_layer
    orc, bb = _mixed(8)
    for cfg in (15, 100):                                    # no ladder there, so no Wiener rung
        rx = _rx(cfg, max_batch=2)
        assert _set_bank(rx, 0, BANK) == 1
        rx.close()
    rx = _rx(8, max_batch=bb.shape[0])
    assert _set_bank(rx, 0, BANK) == 1                       # no ladder
    ladder = [(21, 21), ("wiener", dict(W.DEFAULT, snr_db=5.0)), BANK_RUNG]
    rx.set_estimator_ladder(ladder)
    set_to, bank_was = rx.estimator_ladder_ex, rx.wiener_bank(2)
    assert set_to == [(21, 21), ("wiener", dict(W.DEFAULT, snr_db=5.0)), ("wiener", DESIGNS[-1])]
    assert [d for d, _ in bank_was] == DESIGNS and np.allclose([r for _, r in bank_was[:2]], B.np_thresholds(BANK, 3), rtol=1e-13, atol=0)
    assert rx.wiener_bank(1) == []
    before = rx.receive(bb, want_llr=True)
    nan, inf = float("nan"), float("inf")
    wide = BANK[2]
    for rung in (-1, 0, 3, 4):                              # no such rung, an LS rung
        assert _set_bank(rx, rung, BANK) == 1, rung
    bad = [BANK[::-1], [BANK[0], BANK[0], wide], [(W.design(tau_min_us=10.0, tau_max_us=5.0), None), wide],
           [(W.design(tau_max_us=333.33, snr_db=41.0), None), wide], [(W.design(tau_max_us=333.33, doppler_hz=nan), None), wide],
           B.bank(5.0, rho=[-0.1]), B.bank(5.0, rho=[inf]), B.bank(5.0, rho=[0.9, -inf])]
    for entries in bad:
        for rung in (1, 2):
            assert _set_bank(rx, rung, entries) == 1, entries                       # MGPU_ERR_ARG
    assert _set_bank(rx, 2, BANK, n=5) == 1 and _set_bank(rx, 2, BANK, n=-1) == 1
    for size in (0, 32, 48):
        assert _set_bank(rx, 2, BANK, size=size) == 1, size
    arr, n = (physical_layer.WienerBankEntry * 4)(), C.c_int()
    assert rx.lib.mgpu_get_wiener_bank(rx.h, 2, arr, C.byref(n), 32) == 1 and rx.lib.mgpu_get_wiener_bank(rx.h, 0, arr, C.byref(n), 40) == 1
    with pytest.raises(MgpuError):
        rx.wiener_choice(0, 1)                               # rung 0 is an LS rung
    assert rx.estimator_ladder_ex == set_to and rx.wiener_bank(2) == bank_was and rx.wiener_bank(1) == []
    after = rx.receive(bb, want_llr=True)
    for key in ("payload", "stats", "llr_ldpc"):
        assert after[key].tobytes() == before[key].tobytes(), key
    # an explicit threshold is reported as given; setting any ladder removes every bank
    rx.set_wiener_bank(1, B.bank(5.0, rho=[0.9, None]))
    got = rx.wiener_bank(1)
    assert got[0][1] == 0.9 and abs(got[1][1] - 0.607) <= 1e-3
    rx.set_estimator_ladder([("wiener", {}), ("wiener", {})])
    assert rx.wiener_bank(0) == [] and rx.wiener_bank(1) == []
    with pytest.raises(MgpuError):
        rx.wiener_choice(0, 1)
    rx.close()

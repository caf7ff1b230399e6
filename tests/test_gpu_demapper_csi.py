"""GPU tests of the channel-aware demapper (include/mercury_demapper.h): max-log LLRs weighted by |H|^2 per cell.

Yardsticks: with the demapper off every byte is what it was; with it on the demapped LLRs against the host twin (which
tests/test_demapper_csi_host.py holds against a numpy restatement on the CPU oracle) bit for bit, the H tap against the oracle's full
estimate, the reported variance / SNR / mean_H against the plain run; the decode against twin -> the oracle's decoder -> the oracle's tail on
two-path frames the plain demapper loses; under an estimator ladder against one-rung runs; under diversity against the sum of its parts."""
import functools

import numpy as np
import pytest

from conftest import SEED
from demapper_csi_ref import CASES, full_estimate, llr_src, tail, two_path, two_path_twin
from oraclelib import CARRIER, Oracle, noise_amp_for

pytestmark = pytest.mark.gpu

FE_THREADS = "MERCURY_FE_THREADS"   # read by mgpu_create with getenv: per context


def _rx(cfg, **kw):
    from mercury_amd import RxPhy
    return RxPhy(cfg, **kw)


def _record(out, f):
    return (out["payload"][f].tobytes(), out["stats"][f].tobytes())


def _same_floats(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- 1. off is off -----------------------------------------------------------------------------------------------------------------
def test_off_is_off():
    orc = Oracle(8, 50)
    bb = np.stack([orc.gen_frame(SEED, f, noise_amp_for(3.5 if f < 32 else -15.0))[0] for f in range(64)])
    rx = _rx(8, max_batch=64)
    assert rx.demapper == "maxlog"
    never = rx.receive(bb, want_llr=True)
    decoded = never["stats"]["message_decoded"] != 0
    assert decoded[:32].sum() >= 24 and decoded[32:].sum() == 0          # both kinds of frame are there
    rx.set_demapper("maxlog")
    off = rx.receive(bb, want_llr=True)
    rx.set_demapper("csi")
    assert rx.demapper == "csi"
    on = rx.receive(bb, want_llr=True)
    rx.set_demapper("maxlog")
    assert rx.demapper == "maxlog"
    back = rx.receive(bb, want_llr=True)
    for key in ("payload", "stats", "llr_ldpc"):
        assert off[key].tobytes() == never[key].tobytes(), key
        assert back[key].tobytes() == never[key].tobytes(), key
    assert on["llr_ldpc"].tobytes() != never["llr_ldpc"].tobytes()
    single = rx.receive(bb[3:4])                                          # the one-frame call: captures its graph
    assert _record(single, 0) == _record(never, 3)
    rx.set_demapper("csi")
    assert _record(rx.receive(bb[3:4]), 0) == _record(on, 3)              # ... which the csi kernel is not part of
    rx.set_demapper("maxlog")
    assert _record(rx.receive(bb[3:4]), 0) == _record(never, 3)
    rx.close()


# ---- 2. the LLRs are the twin's ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("cfg,explicit", CASES)
def test_llrs_equal_the_host_twin_bit_for_bit(cfg, explicit, threads, monkeypatch):
    from mercury_amd import host_demap_csi
    orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
    bb = np.stack([orc.gen_frame(SEED, f, noise_amp_for(10.0))[0] for f in range(4)])
    monkeypatch.setenv(FE_THREADS, str(threads))
    rx = _rx(cfg, max_batch=4, explicit=explicit)
    monkeypatch.delenv(FE_THREADS)
    plain = rx.receive(bb, taps=True)
    rx.set_demapper("csi")
    out = rx.receive(bb, taps=True)
    src = llr_src(orc)
    for f in range(4):
        ref = orc.rx(bb[f])
        assert np.array_equal(out["grid"][f], plain["grid"][f]), f
        assert np.array_equal(out["H"][f], full_estimate(orc, ref)), (f, np.abs(out["H"][f] - full_estimate(orc, ref)).max())
        want, sigma2 = host_demap_csi(cfg, out["grid"][f], out["H"][f], explicit=explicit)
        assert _same_floats(out["llr_demod"][f], want), (f, sigma2, np.nanmax(np.abs(out["llr_demod"][f] - want)))
        assert _same_floats(out["llr_ldpc"][f][: orc.N], want[src]), f
        # e = g / h with the equaliser's division: the plain run's equalised cells wherever the plain run divides by the same h
        if not orc.amp_restore:
            assert np.array_equal(out["eq"][f], plain["eq"][f]), f
    # what is reported stays the plain front-end's
    assert out["variance"].tobytes() == plain["variance"].tobytes()
    assert out["stats"]["variance"].tobytes() == plain["stats"]["variance"].tobytes()
    both = (out["stats"]["message_decoded"] != 0) & (plain["stats"]["message_decoded"] != 0)
    assert out["stats"]["snr_db"][both].tobytes() == plain["stats"]["snr_db"][both].tobytes()
    assert out["agc_gain"].tobytes() == plain["agc_gain"].tobytes()
    if orc.amp_restore:
        assert not np.array_equal(out["H"], plain["H"])                  # the plain tap is the unit phasor
    rx.close()


# ---- 3. decode -----------------------------------------------------------------------------------------------------------------------
def test_decode_equals_twin_oracle_decoder_and_tail():
    t, twin = two_path(13, 15.0), two_path_twin(13, 15.0)
    orc, F = t["orc"], len(t["bb"])
    rx = _rx(13, max_batch=F)
    rx.set_estimator_ladder([(5, 5)])
    plain = rx.receive(t["bb"], want_llr=True)
    rx.set_demapper("csi")
    out = rx.receive(t["bb"], want_llr=True)
    rx.close()
    n_plain = n_csi = 0
    for f in range(F):
        ref = t["ref"][f]
        assert np.array_equal(plain["payload"][f], ref["bytes"].astype(np.uint8)), f
        assert plain["stats"]["iterations_done"][f] == ref["iterations"] and plain["stats"]["crc"][f] == ref["crc"], f
        n_plain += int(plain["stats"]["message_decoded"][f] != 0 and np.array_equal(ref["bits"], t["bits"][f]))
        llr_ldpc, bits, it = twin[f]
        payload, crc, all_zeros, decoded = tail(orc, bits)
        st = out["stats"][f]
        assert _same_floats(out["llr_ldpc"][f][: orc.N], llr_ldpc), f
        assert st["iterations_done"] == it and st["message_decoded"] == decoded and st["crc"] == crc and st["all_zeros"] == all_zeros, (f, st, it, decoded)
        assert np.array_equal(out["payload"][f][: payload.size], payload), f
        n_csi += int(decoded and np.array_equal(bits, t["bits"][f]))
    print("mode 13, two paths, 15 dB: plain decodes", n_plain, "of", F, "- csi", n_csi)
    assert n_plain <= 2 and n_csi >= 30, (n_plain, n_csi)


# ---- 4. with a ladder ----------------------------------------------------------------------------------------------------------------
F2 = 32


@functools.lru_cache(maxsize=None)
def _two_path_mode8():
    """mode 8, 32 clean frames of the generator through two equal-power static paths 12 samples (1 ms) apart with phases from
    default_rng(7), noise at 20 dB added here (the frames of tests/test_gpu_estimator_ladder.py)"""
    orc = Oracle(8, 50)
    rng = np.random.default_rng(7)
    amp = noise_amp_for(20.0)
    bb = []
    for f in range(F2):
        x, _ = orc.gen_frame(5, f, 0.0, 0)
        ph = np.exp(1j * rng.uniform(0, 2 * np.pi, 2))
        y = ph[0] * x
        y[12:] += ph[1] * x[:-12]
        y /= np.sqrt(2.0)
        y += amp * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
        bb.append(y)
    return np.stack(bb)


def test_ladder_records_equal_the_one_rung_run_of_the_winning_window():
    bb = _two_path_mode8()
    rx = _rx(8, max_batch=F2)
    rx.set_demapper("csi")
    one = []
    for window in ((21, 21), (5, 5)):
        rx.set_estimator_ladder([window])
        one.append(rx.receive(bb, want_llr=True))
    rx.set_estimator_ladder([(21, 21), (5, 5)])
    assert rx.demapper == "csi"
    whole = rx.receive(bb, want_llr=True)
    rungs = rx.last_rungs(F2)
    ok = [o["stats"]["message_decoded"] != 0 for o in one]
    print("csi, two paths, 20 dB: decoded with 21 x 21", int(ok[0].sum()), "with 5 x 5", int(ok[1].sum()), "rungs", np.bincount(rungs + 1, minlength=3))
    for f in range(F2):
        want = 0 if ok[0][f] else (1 if ok[1][f] else -1)
        assert rungs[f] == want, (f, rungs[f], want)
        src = one[max(want, 0)]
        assert _record(whole, f) == _record(src, f), f
        assert whole["llr_ldpc"][f].tobytes() == src["llr_ldpc"][f].tobytes(), f
    by, frames = rx.ladder_counters()
    assert frames == F2 and by[0] == (rungs == 0).sum() and by[1] == (rungs == 1).sum() and by[2:].sum() == 0
    # a frame does not depend on its batch: a slice, the chunked host path, one frame with LLRs, the one-frame call
    out = rx.receive(bb[5:9], want_llr=True)
    for k, f in enumerate(range(5, 9)):
        assert _record(out, k) == _record(whole, f) and out["llr_ldpc"][k].tobytes() == whole["llr_ldpc"][f].tobytes(), f
    out = rx.receive(bb)
    for f in range(F2):
        assert _record(out, f) == _record(whole, f), f
    picks = [int(np.flatnonzero(rungs == r)[0]) for r in (0, 1, -1) if (rungs == r).any()]
    for f in picks:
        alone = rx.receive(bb[f:f + 1], want_llr=True)
        assert _record(alone, 0) == _record(whole, f) and alone["llr_ldpc"][0].tobytes() == whole["llr_ldpc"][f].tobytes(), f
        single = rx.receive(bb[f:f + 1])                                  # the one-frame call
        assert _record(single, 0) == _record(whole, f), f
        assert rx.last_rungs(1)[0] == rungs[f]
    rx.set_estimator_ladder([])
    single = rx.receive(bb[0:1])                                          # the one-frame call without a ladder: still the csi kernel
    rx.set_estimator_ladder([(21, 21)])
    assert _record(single, 0) == _record(one[0], 0)
    rx.close()


# ---- 5. with diversity -----------------------------------------------------------------------------------------------------------------
def test_grouped_call_is_the_sum_of_csi_rows_received_one_by_one():
    import torch
    from mercury_amd import STATS_DTYPE
    from test_diversity_host import fixture_branches
    cfg, esn0, D, G = 12, 4.5, 2, 8
    orc, _, bb = fixture_branches(cfg, esn0, D, G)
    F = G * D
    rx = _rx(cfg, max_batch=F)
    rx.set_demapper("csi")
    rows = np.stack([rx.receive(bb[f:f + 1], want_llr=True)["llr_ldpc"][0] for f in range(F)])
    plain_rows = rx.receive(bb, want_llr=True)
    assert plain_rows["llr_ldpc"].tobytes() == rows.tobytes()
    div = rx.receive_div(bb, D, want_llr=True)
    assert div["llr_ldpc"].tobytes() == rows.tobytes()                    # the BRANCH LLRs
    sums = rx.llr_combine(rows, D=D)                                      # mgpu_llr_combine_dev
    d_llr = torch.from_numpy(sums).cuda()
    d_payload = torch.zeros((G, rx.payload_stride), dtype=torch.uint8, device="cuda")
    d_stats = torch.zeros(G * STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    rx.ldpc_decode_dev(d_llr.data_ptr(), G, d_payload=d_payload.data_ptr(), d_stats=d_stats.data_ptr())
    torch.cuda.synchronize()
    g_payload, g_stats = d_payload.cpu().numpy(), d_stats.cpu().numpy().view(STATS_DTYPE)
    for f in range(F):
        g = f // D
        assert np.array_equal(div["payload"][f], g_payload[g]), f
        for k in ("iterations_done", "crc", "all_zeros", "message_decoded"):
            assert div["stats"][k][f] == g_stats[k][g], (f, k)
    for g in range(G):
        bits, it = orc.ldpc_decode(sums[g])
        assert g_stats["iterations_done"][g] == it, g
    assert div["stats"]["variance"].tobytes() == plain_rows["stats"]["variance"].tobytes()
    rx.set_demapper("maxlog")
    assert rx.receive(bb, want_llr=True)["llr_ldpc"].tobytes() != rows.tobytes()
    rx.close()


# ---- 6. receive_byte -------------------------------------------------------------------------------------------------------------------
def test_receive_byte_on_clean_windows_is_unchanged_but_for_the_llrs():
    W = 8
    rx = _rx(8, max_batch=W)
    rng = np.random.default_rng(11)
    pl = rng.integers(0, 256, (W, rx.payload_stride)).astype(np.uint8)
    pl[:, rx.payload_bytes:] = 0
    audio = rx.transmit_byte(pl, CARRIER)
    n = rx.receive_buffer_samples()
    d = ((rx.preamble_nsymb + 2) * rx.Nofdm + 50) * 4                      # telecom_system.cc:242-249, :292
    wins = np.zeros((W, n))
    wins[:, d: d + audio.shape[1]] = audio
    plain = rx.receive_byte(wins, CARRIER)
    rx.set_demapper("csi")
    out = rx.receive_byte(wins, CARRIER)
    assert (plain["stats"]["message_decoded"] == 1).all()
    assert np.array_equal(out["payload"], plain["payload"])
    assert np.array_equal(out["payload"][:, : rx.payload_bytes], pl[:, : rx.payload_bytes])
    for key in ("message_decoded", "crc", "all_zeros", "snr_db", "mean_H", "delay", "freq_offset", "signal_strength_dbm"):
        assert out["stats"][key].tobytes() == plain["stats"][key].tobytes(), key
    rx.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_setting_in_place():
    from mercury_amd import MgpuError
    for cfg in (100, 101, 102):
        rx = _rx(cfg, max_batch=2)
        with pytest.raises(MgpuError) as e:
            rx.set_demapper("csi")
        assert e.value.code == 4, (cfg, str(e.value))                     # MGPU_ERR_UNSUPPORTED
        assert rx.demapper == "maxlog"
        rx.close()
    rx = _rx(8, max_batch=2)
    for before in ("csi", "maxlog"):
        rx.set_demapper(before)
        assert rx.lib.mgpu_set_demapper(rx.h, 7) == 1                     # MGPU_ERR_ARG
        assert rx.lib.mgpu_set_demapper(rx.h, -1) == 1
        assert rx.demapper == before
    with pytest.raises(MgpuError):
        rx.set_demapper("exact")
    rx.close()
    for cfg in (15, 16):                                                  # the zero-forcing modes take it
        rx = _rx(cfg, max_batch=2)
        rx.set_demapper("csi")
        assert rx.demapper == "csi"
        rx.close()

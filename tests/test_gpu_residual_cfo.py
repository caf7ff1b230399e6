"""GPU tests of the pilot-aided residual carrier-offset correction (include/mercury_cfo.h).

Yardsticks: with the mode off every byte is what it was; with it on the `grid` tap and the reported steps against the host twin (which
tests/test_residual_cfo_host.py holds against a numpy restatement on the CPU oracle) bit for bit; everything behind the turned grid against
the host LS twin, the one-stage entry points and the channel-aware demapper's twin fed that grid; the decode against the CPU oracle on offset
frames the plain front-end loses; under an estimator ladder against one-rung runs; under diversity against the sum of its parts; and
receive_byte on noisy passband windows whose preamble estimate is off by more than the 21-symbol window tolerates."""
import ctypes as C

import numpy as np
import pytest

from conftest import SEED
from oraclelib import CARRIER, Oracle, noise_amp_for
from residual_cfo_ref import CASES, decode_fixture, noisy_windows, offset_frame, offsets_for, step_to_hz

pytestmark = pytest.mark.gpu

FE_THREADS = "MERCURY_FE_THREADS"   # read by mgpu_create with getenv: per context


def _rx(cfg, **kw):
    from mercury_amd import RxPhy
    return RxPhy(cfg, **kw)


def _record(out, f):
    return (out["payload"][f].tobytes(), out["stats"][f].tobytes())


def _same_floats(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _offset_frames(orc, explicit, esn0_db=10.0):
    return np.stack([offset_frame(orc, k, f_hz, esn0_db)[0] for k, f_hz in enumerate(offsets_for(explicit))])


# ---- 1. off is off -----------------------------------------------------------------------------------------------------------------
def test_off_is_off():
    orc = Oracle(8, 50)
    bb = np.stack([orc.gen_frame(SEED, f, noise_amp_for(3.5 if f < 32 else -15.0))[0] for f in range(64)])
    rx = _rx(8, max_batch=64)
    assert rx.cfo == "off"
    never = rx.receive(bb, want_llr=True)
    decoded = never["stats"]["message_decoded"] != 0
    assert decoded[:32].sum() >= 24 and decoded[32:].sum() == 0          # both kinds of frame are there
    rx.set_cfo("off")
    off = rx.receive(bb, want_llr=True)
    rx.set_cfo("pilots")
    assert rx.cfo == "pilots"
    on = rx.receive(bb, want_llr=True)
    rx.set_cfo("off")
    assert rx.cfo == "off"
    back = rx.receive(bb, want_llr=True)
    for key in ("payload", "stats", "llr_ldpc"):
        assert off[key].tobytes() == never[key].tobytes(), key
        assert back[key].tobytes() == never[key].tobytes(), key
    assert on["llr_ldpc"].tobytes() != never["llr_ldpc"].tobytes()
    single = rx.receive(bb[3:4])                                          # the one-frame call: captures its graph
    assert _record(single, 0) == _record(never, 3)
    rx.set_cfo("pilots")
    assert _record(rx.receive(bb[3:4]), 0) == _record(on, 3)              # ... which the CFO kernel is not part of
    rx.set_cfo("off")
    assert _record(rx.receive(bb[3:4]), 0) == _record(never, 3)
    rx.close()


# ---- 2. the turned grid and the steps are the twin's ---------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("cfg,explicit", CASES)
def test_grid_tap_and_steps_equal_the_host_twin_bit_for_bit(cfg, explicit, threads, monkeypatch):
    from mercury_amd import host_cfo_pilots
    orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
    bb = _offset_frames(orc, explicit)
    F = len(bb)
    monkeypatch.setenv(FE_THREADS, str(threads))
    rx = _rx(cfg, max_batch=F, explicit=explicit)
    monkeypatch.delenv(FE_THREADS)
    plain = rx.receive(bb, taps=True)
    rx.set_cfo("pilots")
    assert not rx.cfo_steps(F).any()                                       # nothing measured yet
    out = rx.receive(bb, taps=True)
    steps = rx.cfo_steps(F)
    for f, f_hz in enumerate(offsets_for(explicit)):
        want, step = host_cfo_pilots(cfg, plain["grid"][f], explicit=explicit)
        print("mode %d, %d threads: %+.1f Hz measured as %+.4f" % (cfg, threads, f_hz, step_to_hz(steps[f])))
        assert steps[f].tobytes() == np.float64(step).tobytes(), (f, steps[f], step)
        assert out["grid"][f].tobytes() == want.tobytes(), (f, np.abs(out["grid"][f] - want).max())
    assert out["agc_gain"].tobytes() == plain["agc_gain"].tobytes()
    no_taps = rx.receive(bb, want_llr=True)                                # the entry point without taps: the same frames, the same steps
    assert no_taps["llr_ldpc"].tobytes() == out["llr_ldpc"].tobytes()
    assert rx.cfo_steps(F).tobytes() == steps.tobytes()
    piped = rx.receive(bb)                                                 # ... and the chunked host path, whose chunks have rows of their own
    assert piped["payload"].tobytes() == out["payload"].tobytes() and piped["stats"].tobytes() == out["stats"].tobytes()
    assert rx.cfo_steps(F).tobytes() == steps.tobytes()
    rx.close()


# ---- 3. downstream of the turned grid nothing is new ---------------------------------------------------------------------------------
def _stage_chain(rx, grid):
    """the one-stage entry points of mercury_stages.h (the plain stages) on a grid [F, G]: H, eq, variance, llr_demod"""
    lib, h, F = rx.lib, rx.h, grid.shape[0]
    grid = np.ascontiguousarray(grid, np.complex128)
    H, eq = np.zeros_like(grid), np.zeros_like(grid)
    rx._ck(lib.mgpu_channel_estimator(h, _p(grid), F, _p(H)))
    if rx.amp_restore:
        rx._ck(lib.mgpu_restore_channel_amplitude(h, _p(H), F))
    rx._ck(lib.mgpu_channel_equalizer(h, _p(grid), _p(H), F, _p(eq)))
    var = np.zeros(F, np.float64)
    rx._ck(lib.mgpu_measure_variance(h, _p(eq), F, _p(var)))
    data, syms = np.zeros((F, rx.nData), np.complex128), np.zeros((F, rx.nData), np.complex128)
    rx._ck(lib.mgpu_deframer(h, _p(eq), F, _p(data)))
    rx._ck(lib.mgpu_deinterleaver_c128(h, _p(data), F, rx.nData, rx.tf_blk, _p(syms)))
    var_f = var.astype(np.float32)
    llr = np.zeros((F, rx.nBits), np.float32)
    rx._ck(lib.mgpu_psk_demod(h, _p(syms), F, _p(var_f), _p(llr)))
    return H, eq, var, llr


@pytest.mark.parametrize("cfg,explicit", CASES)
def test_behind_the_turned_grid_the_stages_are_the_plain_ones(cfg, explicit):
    from mercury_amd import host_demap_csi, host_ls_estimate
    orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
    bb = _offset_frames(orc, explicit)
    F, G = len(bb), orc.Nsymb * orc.Nc
    pilots = np.flatnonzero(orc.frame_types() != 0)
    rx = _rx(cfg, max_batch=F, explicit=explicit)
    plain = rx.receive(bb, taps=True)
    rx.set_cfo("pilots")
    out = rx.receive(bb, taps=True)
    assert not np.array_equal(out["grid"], plain["grid"])
    H, eq, var, llr = _stage_chain(rx, out["grid"])
    assert np.array_equal(out["H"], H), np.abs(out["H"] - H).max()
    assert np.array_equal(out["eq"], eq), np.abs(out["eq"] - eq).max()
    assert out["variance"].tobytes() == var.tobytes()
    assert _same_floats(out["llr_demod"], llr)
    ls = rx.estimator != 0                                                  # (the zero-forcing modes have no LS window and take no ladder)

    def restored_at_pilots(width, height, grid):
        want = np.ones((F, G), np.complex128)
        for f in range(F):
            want[f, pilots] = host_ls_estimate(cfg, grid[f], width, height, explicit=explicit)
        if rx.amp_restore:
            rx._ck(rx.lib.mgpu_restore_channel_amplitude(rx.h, _p(want), F))
        return want[:, pilots]

    if ls:
        assert np.array_equal(out["H"][:, pilots], restored_at_pilots(rx.ls_window, rx.ls_window, out["grid"]))
        rx.set_estimator_ladder([(5, 21)])
        rung = rx.receive(bb, taps=True)
        assert rung["grid"].tobytes() == out["grid"].tobytes()
        assert np.array_equal(rung["H"][:, pilots], restored_at_pilots(5, 21, rung["grid"]))
        assert not np.array_equal(rung["H"], out["H"])
        rx.set_estimator_ladder([])
    # with the channel-aware demapper: its twin on the turned grid and the full estimate made from it
    rx.set_demapper("csi")
    both = rx.receive(bb, taps=True)
    assert both["grid"].tobytes() == out["grid"].tobytes()
    for f in range(F):
        want, _ = host_demap_csi(cfg, both["grid"][f], both["H"][f], explicit=explicit)
        assert _same_floats(both["llr_demod"][f], want), (f, np.nanmax(np.abs(both["llr_demod"][f] - want)))
    if ls:
        want = np.stack([host_ls_estimate(cfg, both["grid"][f], rx.ls_window, rx.ls_window, explicit=explicit) for f in range(F)])
        assert np.array_equal(both["H"][:, pilots], want)                  # the full estimate: no amplitude restoration
    assert both["variance"].tobytes() == out["variance"].tobytes()          # what is reported is the corrected frame's plain variance
    rx.close()


# ---- 4. decode ---------------------------------------------------------------------------------------------------------------------
F4 = 16


def _sent(t, out, f):
    orc = t["orc"]
    return bool(out["stats"]["message_decoded"][f] != 0 and np.array_equal(out["payload"][f][: orc.payload_bytes], t["payload"][f].astype(np.uint8)))


def test_offset_frames_the_plain_front_end_loses_decode():
    """mode 8 at 2 dB, 2 Hz (tests/test_residual_cfo_host.py: the oracle alone decodes 0 of 16, turned back 16)"""
    t = decode_fixture(2.0)
    rx = _rx(8, max_batch=F4)
    plain = rx.receive(t["bb"], want_llr=True)
    rx.set_cfo("pilots")
    out = rx.receive(t["bb"], want_llr=True)
    steps = rx.cfo_steps(F4)
    rx.close()
    for f in range(F4):
        ref = t["ref"][f]
        assert np.array_equal(plain["payload"][f], ref["bytes"].astype(np.uint8)), f
        assert plain["stats"]["iterations_done"][f] == ref["iterations"] and plain["stats"]["crc"][f] == ref["crc"], f
    n_plain = sum(_sent(t, plain, f) for f in range(F4))
    n_on = sum(_sent(t, out, f) for f in range(F4))
    err = step_to_hz(steps) - 2.0
    print("mode 8, 2 dB, 2 Hz: plain decodes %d of %d, corrected %d; step error rms %.4f Hz" % (n_plain, F4, n_on, np.sqrt(np.mean(err * err))))
    assert (np.abs(err) <= 0.15).all(), err
    assert n_plain == 0 and n_on >= 15, (n_plain, n_on)
    assert n_on == int((out["stats"]["message_decoded"] != 0).sum())     # no false decode


# ---- 5. with a ladder ----------------------------------------------------------------------------------------------------------------
def test_ladder_decodes_at_rung_0_what_it_decoded_at_rung_1():
    t = decode_fixture(2.0)
    bb = t["bb"]
    rx = _rx(8, max_batch=F4)
    for mode in ("off", "pilots"):
        rx.set_cfo(mode)
        one, one_steps = [], []
        for window in ((21, 21), (5, 5)):
            rx.set_estimator_ladder([window])
            one.append(rx.receive(bb, want_llr=True))
            one_steps.append(rx.cfo_steps(F4) if mode == "pilots" else None)
        rx.set_estimator_ladder([(21, 21), (5, 5)])
        assert rx.cfo == mode
        whole = rx.receive(bb, want_llr=True)
        rungs = rx.last_rungs(F4)
        ok = [o["stats"]["message_decoded"] != 0 for o in one]
        print("cfo", mode, "- decoded with 21 x 21", int(ok[0].sum()), "with 5 x 5", int(ok[1].sum()), "rungs", np.bincount(rungs + 1, minlength=3))
        for f in range(F4):
            want = 0 if ok[0][f] else (1 if ok[1][f] else -1)
            assert rungs[f] == want, (mode, f, rungs[f], want)
            src = one[max(want, 0)]
            assert _record(whole, f) == _record(src, f), (mode, f)
            assert whole["llr_ldpc"][f].tobytes() == src["llr_ldpc"][f].tobytes(), (mode, f)
            if want >= 0:
                assert _sent(t, whole, f), (mode, f)
        assert (rungs >= 0).sum() >= 15, rungs
        if mode == "off":
            assert (rungs[rungs >= 0] == 1).all(), rungs                   # every decode needs the second front-end and decode
        else:
            assert (rungs[rungs >= 0] == 0).all(), rungs                   # ... and none does with the grid turned back
            # a retry computes the same step and does not write it: the steps are rung 0's, which both one-rung runs also measured
            assert rx.cfo_steps(F4).tobytes() == one_steps[0].tobytes() == one_steps[1].tobytes()
            alone = rx.receive(bb[5:6], want_llr=True)                      # a frame does not depend on its batch
            assert _record(alone, 0) == _record(whole, 5) and alone["llr_ldpc"][0].tobytes() == whole["llr_ldpc"][5].tobytes()
            assert _record(rx.receive(bb[5:6]), 0) == _record(whole, 5)     # the one-frame call
    rx.close()


# ---- 6. with diversity -----------------------------------------------------------------------------------------------------------------
def test_grouped_call_is_the_sum_of_corrected_rows_received_one_by_one():
    import torch
    from mercury_amd import STATS_DTYPE
    from test_diversity_host import fixture_branches
    cfg, esn0, D, G = 12, 4.5, 2, 8
    orc, _, bb = fixture_branches(cfg, esn0, D, G)
    F = G * D
    rx = _rx(cfg, max_batch=F)
    rx.set_cfo("pilots")
    rows = np.stack([rx.receive(bb[f:f + 1], want_llr=True)["llr_ldpc"][0] for f in range(F)])
    plain_rows = rx.receive(bb, want_llr=True)
    steps = rx.cfo_steps(F)
    assert plain_rows["llr_ldpc"].tobytes() == rows.tobytes()
    div = rx.receive_div(bb, D, want_llr=True)
    assert div["llr_ldpc"].tobytes() == rows.tobytes()                    # the BRANCH LLRs
    assert rx.cfo_steps(F).tobytes() == steps.tobytes() and steps.all()   # every branch of the grouped span measured its own step
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
    rx.set_cfo("off")
    assert rx.receive(bb, want_llr=True)["llr_ldpc"].tobytes() != rows.tobytes()
    rx.close()


# ---- 7. receive_byte -------------------------------------------------------------------------------------------------------------------
def test_receive_byte_on_noisy_windows_no_longer_needs_the_short_window():
    """12 mode-8 capture windows at 4 dB in-band SNR, true carrier offset 0 (residual_cfo_ref.noisy_windows): the preamble estimator's own
    error is the offset. On the CPU oracle the default window decodes 6 of them and ls_window = 4 all 12."""
    t = noisy_windows()
    orc, wins, W = t["orc"], t["wins"], len(t["wins"])
    rx = _rx(8, max_batch=W)
    assert rx.receive_buffer_samples() == orc.buffer_samples()

    def count(out):
        ok = (out["stats"]["message_decoded"] == 1) & np.array([np.array_equal(out["payload"][w][: orc.payload_bytes], t["payload"][w]) for w in range(W)])
        assert ok.sum() == (out["stats"]["message_decoded"] == 1).sum()    # no false decode
        return int(ok.sum())

    plain = rx.receive_byte(wins, CARRIER)
    for w in range(W):
        ref = orc.receive_byte(wins[w], carrier=CARRIER)
        st = plain["stats"][w]
        for k in ("iterations_done", "crc", "all_zeros", "message_decoded", "delay", "sync_trials", "frame_overflow_symbols"):
            assert st[k] == ref[k], (w, k, st[k], ref[k])
        assert st["freq_offset"] == ref["freq_offset"], w
        assert np.array_equal(plain["payload"][w][: orc.payload_bytes], ref["payload"]), w
    rx.set_estimator_ladder([(5, 5)])
    short = rx.receive_byte(wins, CARRIER)
    rx.set_estimator_ladder([])
    rx.set_cfo("pilots")
    out = rx.receive_byte(wins, CARRIER)
    n_plain, n_short, n_on = count(plain), count(short), count(out)
    print("receive_byte, 12 windows at 4 dB: plain %d, 5 x 5 window %d, pilots %d; preamble freq_offset of the windows decoded with pilots: %s"
          % (n_plain, n_short, n_on, np.round(out["stats"]["freq_offset"][out["stats"]["message_decoded"] == 1], 2)))
    assert n_on >= n_short - 2 and n_on >= n_plain + 3, (n_plain, n_short, n_on)
    # freq_offset stays the preamble's measurement: up to the decode every window goes the way it went
    both = (plain["stats"]["message_decoded"] == 1) & (out["stats"]["message_decoded"] == 1)
    assert both.any() and out["stats"]["freq_offset"][both].tobytes() == plain["stats"]["freq_offset"][both].tobytes()
    rx.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_setting_in_place():
    from mercury_amd import MgpuError
    for cfg in (100, 101, 102):
        rx = _rx(cfg, max_batch=2)
        with pytest.raises(MgpuError) as e:
            rx.set_cfo("pilots")
        assert e.value.code == 4, (cfg, str(e.value))                     # MGPU_ERR_UNSUPPORTED
        rx.set_cfo("off")                                                 # off is what these modes have
        assert rx.cfo == "off"
        rx.close()
    rx = _rx(8, max_batch=2)
    with pytest.raises(MgpuError):
        rx.cfo_steps(2)                                                   # the mode has never been on
    for before in ("pilots", "off"):
        rx.set_cfo(before)
        assert rx.lib.mgpu_set_cfo(rx.h, 7) == 1                          # MGPU_ERR_ARG
        assert rx.lib.mgpu_set_cfo(rx.h, -1) == 1
        assert rx.cfo == before
    with pytest.raises(MgpuError):
        rx.set_cfo("tracking")
    with pytest.raises(MgpuError):
        rx.cfo_steps(3)                                                   # more rows than max_batch
    rx.close()
    for cfg in (15, 16):                                                  # the zero-forcing modes take it
        rx = _rx(cfg, max_batch=2)
        rx.set_cfo("pilots")
        assert rx.cfo == "pilots"
        rx.close()

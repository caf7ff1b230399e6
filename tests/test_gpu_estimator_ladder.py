"""GPU tests of the estimator ladder (include/mercury_estimator.h): rectangular LS windows in the front-end, and frames whose CRC fails
re-estimated and decoded again on the device with the next window.

Yardsticks: no ladder and the ladder [(21, 21)] are the same bytes; the rectangular estimate against its host twin (which
tests/test_estimator_ladder_host.py holds against the CPU oracle); the ladder [(21, 21), (5, 5)] against two CPU oracles, one per window, on a
two-path channel where the 21-wide window fails frames the 5-wide one decodes; per-frame results independent of the batch."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import SEED
from oraclelib import CARRIER, Oracle, noise_amp_for

pytestmark = pytest.mark.gpu

DY5 = dict(Dy=5, Nsymb=20)          # mode 8 on the reference's LOW_DENSITY pilot lattice


def _rx(cfg, **kw):
    from mercury_amd import RxPhy
    return RxPhy(cfg, **kw)


def _record(out, f):
    return (out["payload"][f].tobytes(), out["stats"][f].tobytes())


# ---- identity ----------------------------------------------------------------------------------------------------------------------
def test_a_one_rung_ladder_of_the_default_window_changes_nothing():
    orc = Oracle(8, 50)
    bb = np.stack([orc.gen_frame(SEED, f, noise_amp_for(3.5 if f < 32 else -15.0))[0] for f in range(64)])
    rx = _rx(8, max_batch=64)
    assert rx.estimator_ladder == []
    plain = rx.receive(bb, want_llr=True)
    decoded = plain["stats"]["message_decoded"] != 0
    assert decoded[:32].sum() >= 24 and decoded[32:].sum() == 0          # both kinds of frame are there
    rx.set_estimator_ladder([(21, 21)])
    assert rx.estimator_ladder == [(21, 21)]
    one = rx.receive(bb, want_llr=True)
    for key in ("payload", "stats", "llr_ldpc"):
        assert one[key].tobytes() == plain[key].tobytes(), key
    assert np.array_equal(rx.last_rungs(64), np.where(decoded, 0, -1))
    by, frames = rx.ladder_counters()
    assert frames == 64 and by[0] == decoded.sum() and by[1:].sum() == 0
    taps = rx.receive(bb[:8], taps=True)                                 # the stage-tap entry point and the one-frame call, same bytes
    assert taps["payload"].tobytes() == plain["payload"][:8].tobytes() and taps["stats"].tobytes() == plain["stats"][:8].tobytes()
    single = rx.receive(bb[3:4])
    assert _record(single, 0) == _record(plain, 3)
    rx.set_estimator_ladder([(20, 20)])                                  # an even side is incremented (telecom_system.cc:2802-2809)
    assert rx.estimator_ladder == [(21, 21)]
    rx.set_estimator_ladder([])
    assert rx.estimator_ladder == []
    again = rx.receive(bb, want_llr=True)
    for key in ("payload", "stats", "llr_ldpc"):
        assert again[key].tobytes() == plain[key].tobytes(), key
    rx.close()


# ---- the rectangular estimate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,explicit", [(0, None), (8, None), (11, None), (8, DY5)])
def test_rung_0_estimate_equals_the_host_twin_bit_for_bit(cfg, explicit):
    """Taps describe rung 0. H at the pilot cells is the LS estimate of the 5 x 21 window - in the PSK modes after
    restore_channel_amplitude, which is applied to the host twin's values through the stage entry point (the device's own atan / sincos)."""
    from mercury_amd import host_ls_estimate
    x = dict(explicit or {})
    orc = Oracle(cfg, 50, explicit=x)
    bb = np.stack([orc.gen_frame(SEED, f, noise_amp_for(10.0), 1)[0] for f in range(4)])
    rx = _rx(cfg, max_batch=4, explicit=explicit)
    square = rx.receive(bb, taps=True)
    rx.set_estimator_ladder([(5, 21)])
    out = rx.receive(bb, taps=True)
    pilots = np.flatnonzero(orc.frame_types() != 0)
    G = orc.Nsymb * orc.Nc
    want = np.ones((4, G), np.complex128)
    for f in range(4):
        assert np.array_equal(out["grid"][f], square["grid"][f])
        want[f, pilots] = host_ls_estimate(cfg, out["grid"][f], 5, 21, explicit=explicit)
    if rx.amp_restore:
        rx._ck(rx.lib.mgpu_restore_channel_amplitude(rx.h, want.ctypes.data_as(C.c_void_p), 4))
    assert np.array_equal(out["H"][:, pilots], want[:, pilots]), np.abs(out["H"][:, pilots] - want[:, pilots]).max()
    assert not np.array_equal(out["H"], square["H"])
    rx.close()


# ---- the ladder against the oracle -------------------------------------------------------------------------------------------------
F2 = 32


@functools.lru_cache(maxsize=None)
def _two_path():
    """Mode 8, 32 clean frames of the generator through two equal-power static paths 12 samples (1 ms) apart with phases from
    default_rng(7), noise at 20 dB added here; what the CPU oracle makes of each frame with the 21 x 21 and with the 5 x 5 window."""
    o21, o5 = Oracle(8, 50), Oracle(8, 50, explicit=dict(ls_window=5))
    rng = np.random.default_rng(7)
    amp = noise_amp_for(20.0)
    bb, sent = [], []
    for f in range(F2):
        x, pl = o21.gen_frame(5, f, 0.0, 0)
        ph = np.exp(1j * rng.uniform(0, 2 * np.pi, 2))
        y = ph[0] * x
        y[12:] += ph[1] * x[:-12]
        y /= np.sqrt(2.0)
        y += amp * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
        bb.append(y)
        sent.append(pl.astype(np.uint8))
    bb = np.stack(bb)
    ref21 = [o21.rx(bb[f]) for f in range(F2)]
    ref5 = [o5.rx(bb[f]) for f in range(F2)]
    nb = o21.payload_bytes
    ok21 = np.array([np.array_equal(ref21[f]["bytes"][:nb].astype(np.uint8), sent[f]) and ref21[f]["iterations"] <= 50 for f in range(F2)])
    ok5 = np.array([np.array_equal(ref5[f]["bytes"][:nb].astype(np.uint8), sent[f]) and ref5[f]["iterations"] <= 50 for f in range(F2)])
    # measured on the CPU oracle with this construction: the 21-wide window decodes 25 of the 32 frames, the 5-wide one all 32
    assert (~ok21).sum() >= 3 and ok5.all(), (ok21.sum(), ok5.sum())
    return dict(bb=bb, sent=np.stack(sent), ref21=ref21, ref5=ref5, ok21=ok21, nb=nb)


@functools.lru_cache(maxsize=None)
def _two_path_gpu():
    t = _two_path()
    rx = _rx(8, max_batch=F2)
    rx.set_estimator_ladder([(21, 21), (5, 5)])
    out = rx.receive(t["bb"], want_llr=True)
    out["rungs"] = rx.last_rungs(F2)
    out["counters"] = rx.ladder_counters()
    rx.close()
    return out


def test_ladder_records_equal_the_oracle_of_the_winning_window():
    t, out = _two_path(), _two_path_gpu()
    for f in range(F2):
        rung = 0 if t["ok21"][f] else 1
        ref = (t["ref21"] if rung == 0 else t["ref5"])[f]
        assert out["rungs"][f] == rung, (f, out["rungs"][f])
        st = out["stats"][f]
        assert st["message_decoded"] == 1, f
        assert np.array_equal(out["payload"][f], ref["bytes"].astype(np.uint8)), f
        assert st["iterations_done"] == ref["iterations"] and st["crc"] == ref["crc"], (f, st, ref["iterations"], ref["crc"])
        assert np.float32(st["variance"]) == np.float32(ref["variance_f"]), f
        assert np.array_equal(out["payload"][f][: t["nb"]], t["sent"][f]), f
    by, frames = out["counters"]
    assert frames == F2 and by[0] == t["ok21"].sum() and by[1] == (~t["ok21"]).sum() and by[2:].sum() == 0 and by.sum() == frames


def test_a_frame_does_not_depend_on_its_batch():
    t, whole = _two_path(), _two_path_gpu()
    rx = _rx(8, max_batch=F2)
    rx.set_estimator_ladder([(21, 21), (5, 5)])

    def same(out, rungs, frames):
        for k, f in enumerate(frames):
            assert _record(out, k) == _record(whole, f), (k, f)
            assert out["llr_ldpc"][k].tobytes() == whole["llr_ldpc"][f].tobytes(), (k, f)
            assert rungs[k] == whole["rungs"][f], (k, f)

    order = list(range(F2))[::-1]
    out = rx.receive(t["bb"][order], want_llr=True)
    same(out, rx.last_rungs(F2), order)
    for lo, hi in ((0, 5), (5, F2)):
        out = rx.receive(t["bb"][lo:hi], want_llr=True)
        same(out, rx.last_rungs(hi - lo), list(range(lo, hi)))
    out = rx.receive(t["bb"])                                       # no LLRs asked for: the chunked host path
    for f in range(F2):
        assert _record(out, f) == _record(whole, f), f
    assert np.array_equal(rx.last_rungs(F2), whole["rungs"])
    for f in (int(np.flatnonzero(t["ok21"])[0]), int(np.flatnonzero(~t["ok21"])[0])):      # one-frame calls: a rung-0 and a rung-1 frame
        out = rx.receive(t["bb"][f:f + 1])
        assert _record(out, 0) == _record(whole, f), f
        assert rx.last_rungs(1)[0] == whole["rungs"][f]
    rx.close()


@pytest.mark.parametrize("pinned", [False, True])
def test_a_retry_reads_a_chunk_before_the_next_copy_lands_on_it(pinned, monkeypatch):
    """The chunked host path with a ladder whose retries read a chunk's input again, in several chunks (a ragged tail of 2 frames behind
    six chunks of 5; two chunks of 16): page-locked input has a copy stream running ahead into the buffer of chunk k-2, which must wait
    for that chunk's retry and not only for its front-end; pageable input alternates two streams. Same records and rungs as one piece."""
    from mercury_amd.physical_layer import pinned_empty
    t, whole = _two_path(), _two_path_gpu()
    bb = t["bb"]
    if pinned:
        buf = pinned_empty(bb.shape, np.complex128)
        buf[...] = bb
        bb = buf
    rx = _rx(8, max_batch=F2)
    rx.set_estimator_ladder([(21, 21), (5, 5)])
    for chunk in ("5", "16"):
        monkeypatch.setenv("MERCURY_RX_CHUNK", chunk)
        for rep in range(2):
            out = rx.receive(bb)
            for f in range(F2):
                assert _record(out, f) == _record(whole, f), (chunk, rep, f)
            assert np.array_equal(rx.last_rungs(F2), whole["rungs"]), (chunk, rep)
    monkeypatch.delenv("MERCURY_RX_CHUNK", raising=False)
    rx.close()


def test_nothing_to_retry_and_everything_to_retry():
    orc = Oracle(8, 50)
    clean = np.stack([orc.gen_frame(SEED, f, 0.0)[0] for f in range(16)])
    rng = np.random.default_rng(3)
    noise = rng.standard_normal((16, orc.frame_samples)) + 1j * rng.standard_normal((16, orc.frame_samples))
    rx = _rx(8, max_batch=16)
    plain_clean, plain_noise = rx.receive(clean, want_llr=True), rx.receive(noise, want_llr=True)
    assert np.all(plain_clean["stats"]["message_decoded"] == 1) and np.all(plain_noise["stats"]["message_decoded"] == 0)
    rx.set_estimator_ladder([(21, 21), (5, 21), (5, 5)])
    out = rx.receive(clean, want_llr=True)
    assert np.array_equal(rx.last_rungs(16), np.zeros(16, np.int32))
    for key in ("payload", "stats", "llr_ldpc"):
        assert out[key].tobytes() == plain_clean[key].tobytes(), key
    out = rx.receive(noise, want_llr=True)                          # no rung decodes: rung 0's failing record is what is reported
    assert np.array_equal(rx.last_rungs(16), np.full(16, -1, np.int32))
    for key in ("payload", "stats", "llr_ldpc"):
        assert out[key].tobytes() == plain_noise[key].tobytes(), key
    by, frames = rx.ladder_counters(reset=True)
    assert frames == 32 and list(by) == [16, 0, 0, 0]
    by, frames = rx.ladder_counters()
    assert frames == 0 and by.sum() == 0
    rx.close()


def test_the_baseband_self_simulation_runs_the_ladder():
    """a two-path channel 1 ms apart in the baseband loop: the loop's frames are counted by the ladder, and none is lost to it"""
    from mercury_amd import HfChannel
    ch = HfChannel(((0.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0)))
    rx = _rx(8, max_batch=64)
    before = rx.baseband_test_esn0([20.0], 64, seed=5, hf_channel=ch)[0]
    rx.set_estimator_ladder([(21, 21), (5, 21)])
    after = rx.baseband_test_esn0([20.0], 64, seed=5, hf_channel=ch)[0]
    by, frames = rx.ladder_counters()
    print("baseband loop: frame errors without the ladder", before["Error_frames_total"], "with it", after["Error_frames_total"], "by rung", list(by))
    assert frames == 64 and by[0] == before["crc_ok_frames"] and by[2:].sum() == 0          # the loop's frames went through the ladder
    assert after["crc_ok_frames"] == by[0] + by[1]
    assert after["Error_frames_total"] <= before["Error_frames_total"]
    rx.close()


# ---- receive_byte and what is built on it --------------------------------------------------------------------------------------------
TWO_PATH_1MS = (((0.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0)))       # static, equal gains, 1 ms apart


def test_receive_byte_retries_inside_a_trial():
    """16 capture windows of transmit_byte audio through the static two-path channel, noise 20 dB below the signal. On the CPU oracle
    (morc receive_byte on the same construction, ls_window 21 / 5) the 21-wide window decodes 0 of the 16 windows and the 5-wide one 16:
    a static channel puts the notches on the same carriers in every window. Four more windows without the channel are there for the
    other half of the claim: what decodes without the ladder decodes with it, same payload."""
    from mercury_amd import HfChannel
    F = 16
    rx = _rx(8, max_batch=F + 4)
    rng = np.random.default_rng(11)
    pl = rng.integers(0, 256, (F + 4, rx.payload_stride)).astype(np.uint8)
    pl[:, rx.payload_bytes:] = 0
    audio = rx.transmit_byte(pl, CARRIER)
    n = rx.receive_buffer_samples()
    d = ((rx.preamble_nsymb + 2) * rx.Nofdm + 50) * 4                      # telecom_system.cc:242-249, :292
    wins = np.zeros((F + 4, n))
    wins[:, d: d + audio.shape[1]] = audio
    wins[:F] = rx.hf_channel_apply(wins[:F], HfChannel(TWO_PATH_1MS), seed=3)
    wins += rng.standard_normal(wins.shape) * np.sqrt(np.mean(audio ** 2)) * 10 ** (-20 / 20)
    plain = rx.receive_byte(wins, CARRIER)
    rx.set_estimator_ladder([(21, 21), (5, 21)])
    out = rx.receive_byte(wins, CARRIER)
    was = plain["stats"]["message_decoded"] == 1
    now = out["stats"]["message_decoded"] == 1
    print("decoded without the ladder", int(was.sum()), "with it", int(now.sum()))
    assert was[F:].all()
    assert now[was].all() and np.array_equal(out["payload"][was], plain["payload"][was])
    assert now.sum() >= was.sum() + 1
    assert np.array_equal(out["payload"][now][:, : rx.payload_bytes], pl[now][:, : rx.payload_bytes])
    by, frames = rx.ladder_counters()
    assert by[1] >= 1 and frames >= F + 4
    rx.close()


def test_capture_and_link_simulator_take_a_ladder():
    """one LinkSim and one RxCapture end to end on the static two-path channel: with the ladder at least as many frames are delivered and
    no decode is false"""
    from mercury_amd import HfChannel, LinkSim, RxCapture, linksim_config
    S, H = 4, 90                                                            # three slots of mode 8's 28 hops + 2
    ch = HfChannel(TWO_PATH_1MS)

    def sim(ladder):
        rx = _rx(8, max_iters=10, max_batch=16)
        s = LinkSim(rx, linksim_config(S, CARRIER, 0x4C414444, channel=ch, gap_hops=2, output_power_watt=1.0), np.full(S, 30.0), ladder=ladder)
        events, audio = s.run(H, want_samples=True)
        counters = s.counters()
        s.close()
        return rx, events, audio, counters

    rx0, ev0, audio, c0 = sim(None)
    rx1, ev1, audio1, c1 = sim([(21, 21), (5, 21)])
    assert np.array_equal(audio, audio1)
    assert c1["false_decodes"].sum() == 0 and c0["false_decodes"].sum() == 0
    assert c1["delivered"].sum() >= c0["delivered"].sum() and c1["delivered"].sum() >= 1, (c0["delivered"], c1["delivered"])
    print("link simulator: delivered without the ladder", int(c0["delivered"].sum()), "with it", int(c1["delivered"].sum()))
    cap0 = RxCapture(rx0, S, CARRIER)
    got0 = cap0.run(audio)
    cap0.close()
    cap1 = RxCapture(rx0, S, CARRIER, ladder=[(21, 21), (5, 21)])          # sets the ladder on the context it is given
    assert rx0.estimator_ladder == [(21, 21), (5, 21)]
    got1 = cap1.run(audio)
    cap1.close()
    assert len(got0) == len(ev0) and len(got1) == len(ev1) >= len(got0)
    rx0.close(), rx1.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_untouched():
    from mercury_amd import MgpuError, physical_layer
    for cfg in (15, 16, physical_layer.cfg_explicit(32, 8, 1, 0), 100, 102):
        rx = _rx(cfg, max_batch=2)
        with pytest.raises(MgpuError) as e:
            rx.set_estimator_ladder([(21, 21), (5, 21)])
        assert "mgpu error 4" in str(e.value), (cfg, str(e.value))            # MGPU_ERR_UNSUPPORTED
        rx.set_estimator_ladder([])                                           # no ladder is what these modes have
        assert rx.estimator_ladder == []
        rx.close()
    rx = _rx(8, max_batch=2)
    rx.set_estimator_ladder([(21, 21), (5, 21)])
    for bad in ([(23, 21)], [(21, 21), (5, 0)], [(21, 21)] * 5, [(0, 5)], [(5, 22)]):
        with pytest.raises(MgpuError) as e:
            rx.set_estimator_ladder(bad)
        assert "mgpu error 1" in str(e.value), (bad, str(e.value))            # MGPU_ERR_ARG
        assert rx.estimator_ladder == [(21, 21), (5, 21)]
    with pytest.raises(MgpuError):
        rx.last_rungs(3)                                                     # no call yet
    rx.close()

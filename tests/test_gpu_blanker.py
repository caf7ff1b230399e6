"""GPU tests of the impulse blanker (include/mercury_blanker.h): the median-gated blanking kernel at the head of the fused receive span.

Yardsticks: the stage on its own against the host twin (which tests/test_blanker_host.py holds against a numpy restatement) byte for byte,
output and report, on impulse frames, a clean frame, a frame over the cap and NaN / zero-block frames; the span with the stage on, fed the
frames, against the span with the stage off fed the twin's output, every key byte for byte - plain, under a ladder, with the noise map and the
carrier-offset stage, grouped, on a zero-forcing and on an MFSK mode; the one-frame call against its row; off again against the records taken
before; the decode against the CPU oracle on the twin's samples frame by frame; receive_byte on passband windows with clicks; refusals."""
import ctypes as C

import numpy as np
import pytest

from blanker_ref import DY5, MFSK, POINTS, WINDOWS, click_windows, decoded, impulse_frames, mixed_batch

pytestmark = pytest.mark.gpu

FE_THREADS = "MERCURY_FE_THREADS"   # read by mgpu_create with getenv: per context
F = 8
CASES = [(13, None), (8, None), (0, None), (MFSK, None), (8, DY5)]


def _rx(cfg, **kw):
    from mercury_amd import RxPhy
    return RxPhy(cfg, **kw)


def _twin(cfg, explicit, bb, **prm):
    from mercury_amd import BLANKER_REPORT_DTYPE, host_blank
    out, rep = np.zeros_like(bb), np.zeros(len(bb), BLANKER_REPORT_DTYPE)
    for f in range(len(bb)):
        out[f], r = host_blank(cfg, bb[f], explicit=explicit, **prm)
        rep[f] = (r["marked"], r["blanked"])
    return out, rep


def _record(out, f):
    return (out["payload"][f].tobytes(), out["stats"][f].tobytes())


# ---- 1. the stage on its own is the twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,explicit,threads", [(c, e, 512) for c, e in CASES] + [(8, None, 1024)])
def test_blank_equals_the_host_twin_byte_for_byte(cfg, explicit, threads, monkeypatch):
    orc, bb = mixed_batch(cfg, explicit, F)
    monkeypatch.setenv(FE_THREADS, str(threads))
    rx = _rx(cfg, max_batch=F, explicit=explicit)
    monkeypatch.delenv(FE_THREADS)
    assert rx.blanker == ("off", {"threshold": 24.0, "guard": 4, "max_share": 0.125})
    for prm in ({}, dict(threshold=12.0, guard=16, max_share=0.5), dict(guard=0)):
        if prm:
            rx.set_blanker("median", **prm)
            rx.set_blanker("off")                                          # the stage on its own runs with the parameters last set, on or off
        want, want_rep = _twin(cfg, explicit, bb, **prm)
        got, rep = rx.blank(bb)
        assert rep.tobytes() == want_rep.tobytes(), (prm, rep, want_rep)
        assert got.tobytes() == want.tobytes(), prm
    print("mode %d %s, %d threads: marked %s, blanked %s" % (cfg, explicit, threads, want_rep["marked"], want_rep["blanked"]))
    assert want_rep["blanked"][0] > 0 and want_rep["marked"][1] == 0 and want_rep["marked"][2] > want_rep["blanked"][2] == 0      # (guard 0: the batch's kinds)
    # an input stride larger than the frame: the rows' tails are never read into the output
    rx.set_blanker("median")                                               # the defaults again
    rx.set_blanker("off")
    want, want_rep = _twin(cfg, explicit, bb)
    wide = np.full((F, bb.shape[1] + 37), complex(1e6, -1e6), np.complex128)
    wide[:, : bb.shape[1]] = bb
    got, rep = rx.blank(wide, frame_stride=wide.shape[1])
    assert rep.tobytes() == want_rep.tobytes() and got.tobytes() == want.tobytes()
    rx.close()


# ---- 2. the span behind the blanker is the span on the twin's output ---------------------------------------------------------------------------
def _span_pair(rx, cfg, explicit, bb, call, keys, report=True):
    """call(rx, frames) with the stage on, fed bb, against the stage off, fed twin(bb)"""
    clean, want_rep = _twin(cfg, explicit, bb)
    rx.set_blanker("off")
    want = call(rx, clean)
    rx.set_blanker("median")
    assert rx.blanker[0] == "median"
    got = call(rx, bb)
    for key in keys:
        assert got[key].tobytes() == want[key].tobytes(), key
    if report:
        assert rx.blanker_report(0, len(bb)).tobytes() == want_rep.tobytes()
    rx.set_blanker("off")
    return got, want


TAP_KEYS = ("payload", "stats", "llr_ldpc", "grid", "H", "eq", "variance", "agc_gain")


@pytest.mark.parametrize("cfg,explicit", [(13, None), (8, DY5)])
def test_span_with_the_stage_on_is_the_plain_span_on_the_twins_output(cfg, explicit):
    orc, bb = mixed_batch(cfg, explicit, F)
    rx = _rx(cfg, max_batch=F, explicit=explicit)
    got, _ = _span_pair(rx, cfg, explicit, bb, lambda r, x: r.receive(x, taps=True), TAP_KEYS)
    _span_pair(rx, cfg, explicit, bb, lambda r, x: r.receive(x, want_llr=True), ("payload", "stats", "llr_ldpc"))
    _span_pair(rx, cfg, explicit, bb, lambda r, x: r.receive(x), ("payload", "stats"))          # the pipelined host path
    # a window of the report's rows
    rx.set_blanker("median")
    rx.receive(bb)
    assert rx.blanker_report(2, 3).tobytes() == _twin(cfg, explicit, bb)[1][2:5].tobytes()
    assert rx.receive(bb[:F], taps=True)["grid"].tobytes() == got["grid"].tobytes()
    rx.close()


def test_span_under_a_ladder():
    orc, bb = mixed_batch(8, None, F)
    rx = _rx(8, max_batch=F)
    rx.set_estimator_ladder([(21, 21), (5, 21)])
    rungs = {}

    def call(r, x):
        out = r.receive(x, want_llr=True)
        rungs[r.blanker[0]] = r.last_rungs(F)
        return out

    _span_pair(rx, 8, None, bb, call, ("payload", "stats", "llr_ldpc"))
    assert np.array_equal(rungs["median"], rungs["off"]), rungs
    print("ladder rungs of the batch:", rungs["median"])
    rx.close()


def test_span_with_the_noise_map_and_the_carrier_offset_stage():
    orc, bb = mixed_batch(8, None, F)
    rx = _rx(8, max_batch=F)
    rx.set_demapper("nmap")
    rx.set_cfo("pilots")
    steps = {}

    def call(r, x):
        out = r.receive(x, taps=True)
        steps[r.blanker[0]] = (r.cfo_steps(F).tobytes(), r.noise_map()[0].tobytes())
        return out

    _span_pair(rx, 8, None, bb, call, TAP_KEYS)
    assert steps["median"] == steps["off"]
    rx.close()


def test_span_grouped():
    orc, bb = mixed_batch(8, None, F)
    rx = _rx(8, max_batch=F)
    _span_pair(rx, 8, None, bb, lambda r, x: r.receive_div(x, 2, want_llr=True), ("payload", "stats", "llr_ldpc"))
    rx.close()


@pytest.mark.parametrize("cfg", [16, MFSK])
def test_span_on_a_zero_forcing_and_on_an_mfsk_mode(cfg):
    orc, bb = mixed_batch(cfg, None, F)
    rx = _rx(cfg, max_batch=F)
    keys = ("payload", "stats", "llr_ldpc", "grid", "variance", "agc_gain") + (() if cfg == MFSK else ("H", "eq"))
    _span_pair(rx, cfg, None, bb, lambda r, x: r.receive(x, taps=True), keys)
    _span_pair(rx, cfg, None, bb, lambda r, x: r.receive(x), ("payload", "stats"))
    rx.close()


# ---- 3. one frame, and off again -----------------------------------------------------------------------------------------------------------
def test_one_frame_is_its_row_and_off_is_off_again():
    orc, bb = mixed_batch(13, None, F)
    rx = _rx(13, max_batch=F)
    before = rx.receive(bb, want_llr=True)
    one_before = [_record(rx.receive(bb[f: f + 1]), 0) for f in (0, 3)]      # the one-frame call: captures its graph
    assert one_before == [_record(before, f) for f in (0, 3)]
    rx.set_blanker("median")
    on = rx.receive(bb, want_llr=True)
    assert on["llr_ldpc"].tobytes() != before["llr_ldpc"].tobytes()
    for f in (0, 1, 3):
        assert _record(rx.receive(bb[f: f + 1]), 0) == _record(on, f), f     # mgpu_rx_batch with one frame: not the captured graph
        assert rx.blanker_report(0, 1).tobytes() == _twin(13, None, bb[f: f + 1])[1].tobytes()
        assert rx.receive(bb[f: f + 1], want_llr=True)["llr_ldpc"][0].tobytes() == on["llr_ldpc"][f].tobytes()
    rx.set_blanker("off")
    assert rx.blanker[0] == "off"
    again = rx.receive(bb, want_llr=True)
    for key in ("payload", "stats", "llr_ldpc"):
        assert again[key].tobytes() == before[key].tobytes(), key
    assert [_record(rx.receive(bb[f: f + 1]), 0) for f in (0, 3)] == one_before       # through its graph again
    rx.close()


# ---- 4. what it is worth, on the device ------------------------------------------------------------------------------------------------------
def test_decode_count_on_the_device_is_the_host_tests_frame_by_frame():
    """mode 13 at 14 dB, 25 dB impulses every 100 samples (tests/test_blanker_host.py: the oracle alone 0 of 16, on the twin's output 16)"""
    from mercury_amd import host_blank
    esn0, db, width = POINTS[13]
    t = impulse_frames(13, None, esn0, db, width, frames=16)
    orc, bb = t["orc"], t["bb"]
    rx = _rx(13, max_batch=16)
    plain = rx.receive(bb)
    rx.set_blanker("median")
    out = rx.receive(bb, want_llr=True)
    rx.close()
    n = n_host = 0
    for f in range(16):
        ref = orc.rx(host_blank(13, bb[f])[0])
        st = out["stats"][f]
        assert np.array_equal(out["llr_ldpc"][f][: orc.N], ref["llr_ldpc"][: orc.N], equal_nan=True), f
        ok = decoded(orc, ref, t["bits"][f])
        assert st["iterations_done"] == ref["iterations"] and bool(st["message_decoded"]) == bool(ref["crc"] == 0 and not ref["all_zeros"]), (f, st)
        if ok:
            assert np.array_equal(out["payload"][f][: orc.payload_bytes], t["payload"][f].astype(np.uint8)), f
        n_host += int(ok)
        n += int(st["message_decoded"] != 0 and np.array_equal(out["payload"][f][: orc.payload_bytes], t["payload"][f].astype(np.uint8)))
    n_plain = int((plain["stats"]["message_decoded"] != 0).sum())
    print("mode 13 at 14 dB, 25 dB impulses every 100 samples: plain decodes %d of 16, behind the blanker %d (host %d)" % (n_plain, n, n_host))
    assert n == n_host and n_plain <= 2 and n >= 14, (n_plain, n, n_host)


# ---- 5. receive_byte -------------------------------------------------------------------------------------------------------------------------
def test_receive_byte_on_windows_with_clicks():
    """8 mode-13 capture windows at 20 dB in-band SNR with clicks every 800 passband samples over the data symbols, 25 dB above the
    transmission at baseband scale (blanker_ref.click_windows). On the CPU oracle the windows decode 8 of 8 without the clicks and 0 of 8
    with them; the host twin on the extracted frames zeroes 207 to 222 samples per frame and all 8 decode."""
    from oraclelib import CARRIER
    t = click_windows()
    orc, W = t["orc"], WINDOWS
    rx = _rx(13, max_batch=W)

    def count(out):
        ok = np.array([out["stats"]["message_decoded"][w] == 1 and np.array_equal(out["payload"][w][: orc.payload_bytes], t["payload"][w]) for w in range(W)])
        assert ok.sum() == (out["stats"]["message_decoded"] == 1).sum()    # no false decode
        return int(ok.sum())

    off = rx.receive_byte(t["clicks"], CARRIER)
    clean_off = rx.receive_byte(t["clean"], CARRIER)
    rx.set_blanker("median")
    on = rx.receive_byte(t["clicks"], CARRIER)
    rep = rx.blanker_report(0, W)
    clean_on = rx.receive_byte(t["clean"], CARRIER)
    clean_rep = rx.blanker_report(0, W)
    rx.close()
    print("receive_byte, 8 windows with clicks: off %d, on %d decoded (without clicks %d); blanked per window %s"
          % (count(off), count(on), count(clean_off), rep["blanked"]))
    assert (rep["blanked"] > 0).all() and count(on) >= count(off)
    assert clean_on["payload"].tobytes() == clean_off["payload"].tobytes() and clean_on["stats"].tobytes() == clean_off["stats"].tobytes()
    assert (clean_rep["marked"] == 0).all()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    from mercury_amd import BlankerParams, MgpuError
    rx = _rx(8, max_batch=2)
    with pytest.raises(MgpuError):
        rx.blanker_report()                                               # never set: no report
    for before in (("off", {}), ("median", dict(threshold=30.0, guard=2, max_share=0.25))):
        rx.set_blanker(before[0], **before[1])
        state = rx.blanker
        for kw in (dict(threshold=1.5), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(guard=-1), dict(guard=17),
                   dict(max_share=0.0), dict(max_share=0.6)):
            with pytest.raises(MgpuError) as e:
                rx.set_blanker("median", **kw)
            assert e.value.code == 1, kw                                  # MGPU_ERR_ARG
            assert rx.blanker == state
        prm = BlankerParams(24.0, 4, 0.125)
        for size in (0, 8, C.sizeof(prm) + 8):
            assert rx.lib.mgpu_set_blanker(rx.h, 1, C.byref(prm), size) == 1
        assert rx.lib.mgpu_set_blanker(rx.h, 2, C.byref(prm), C.sizeof(prm)) == 1
        assert rx.lib.mgpu_set_blanker(rx.h, -1, C.byref(prm), C.sizeof(prm)) == 1
        assert rx.blanker == state
    assert rx.lib.mgpu_set_blanker(rx.h, 1, None, C.sizeof(BlankerParams)) == 0            # NULL: the defaults
    assert rx.blanker == ("median", {"threshold": 24.0, "guard": 4, "max_share": 0.125})
    with pytest.raises(MgpuError):
        rx.set_blanker("clip")
    rx.close()

"""GPU tests of the carrier excisor (include/ext/mercury_excisor.h): the three kernels at the head of receive_byte.

Yardsticks: the stage on its own against the host twin (which tests/test_excisor_host.py holds against a numpy restatement) bit for bit, output
and report, at window lengths on either side of the block size and at a capture window's; receive_byte with the stage on against the CPU
oracle's receive_byte on the twin's output, window for window on every field tests/test_receive_byte.py compares, from device memory, host
doubles and INT16 samples; the stage set and taken off again against a context that never had it; a capture run with a clean and a toned
capture; refusals."""
import ctypes as C

import numpy as np
import pytest

import excisor_ref as er
from oraclelib import CARRIER

pytestmark = pytest.mark.gpu


def _rx(cfg, **kw):
    from mercury_amd import RxPhy
    return RxPhy(cfg, **kw)


def _twin(x, carrier, **prm):
    from mercury_amd import EXCISOR_REPORT_DTYPE, host_excise
    out, rep = np.zeros_like(x), np.zeros(len(x), EXCISOR_REPORT_DTYPE)
    for w in range(len(x)):
        out[w], r = host_excise(x[w], carrier, **prm)
        for name in EXCISOR_REPORT_DTYPE.names:
            rep[name][w] = r[name]
    return out, rep


def _same_report(got, want):
    for name in want.dtype.names:
        assert got[name].tobytes() == want[name].tobytes(), (name, got[name], want[name])


# ---- 1. the stage on its own is the twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 513, 1537, 92480])
def test_excise_equals_the_host_twin_bit_for_bit(n):
    x = er.batch(n)
    rx = _rx(8, max_batch=8)
    assert rx.excisor() == ("off", {"threshold": 12.0, "guard": 1, "max_bins": 16})
    for prm in ({}, dict(threshold=8.0, guard=4, max_bins=32), dict(guard=0, max_bins=3)):
        if prm:
            rx.set_excisor("welch", **prm)
            rx.set_excisor("off")                                          # the stage on its own runs with the parameters last set, on or off
        for carrier in (CARRIER, 9000.0):
            want, want_rep = _twin(x, carrier, **prm)
            got, rep = rx.excise(x, carrier)
            _same_report(rep, want_rep)
            assert got.tobytes() == want.tobytes(), (prm, carrier)
    rx.set_excisor("welch")
    rx.set_excisor("off")
    want, want_rep = _twin(x, CARRIER)
    print("n = %d: bins removed %s, mask bits %s" % (n, want_rep["excised"], [bin(m).count("1") for m in want_rep["mask"]]))
    if n == 92480:                                                           # the batch's kinds: three cleaned, one clean, one over the cap
        assert (want_rep["excised"][:3] > 0).all() and want_rep["mask"][3] == 0 and want_rep["excised"][4] == 0 and bin(want_rep["mask"][4]).count("1") > 16
    # a window's result does not depend on its place in the batch
    for w in (0, 4):
        alone, rep_alone = rx.excise(x[w: w + 1], CARRIER)
        assert alone[0].tobytes() == want[w].tobytes() and rep_alone.tobytes() == rx.excise(x, CARRIER)[1][w: w + 1].tobytes()
        others = np.delete(x, w, axis=0)
        first, _ = rx.excise(np.concatenate([x[w: w + 1], others]), CARRIER)
        last, rep_last = rx.excise(np.concatenate([others, x[w: w + 1]]), CARRIER)
        assert first[0].tobytes() == want[w].tobytes() and last[-1].tobytes() == want[w].tobytes()
        _same_report(rep_last[-1:], want_rep[w: w + 1])
    rx.close()


def test_excise_over_more_windows_than_one_launch_takes():
    x = np.tile(er.batch(1537), (27, 1))                                     # 135 windows: three launches of at most 64
    rx = _rx(8, max_batch=2)
    want, want_rep = _twin(x[:5], CARRIER)
    got, rep = rx.excise(x, CARRIER)
    assert got.tobytes() == np.tile(want, (27, 1)).tobytes()
    _same_report(rep, np.tile(want_rep, 27))
    rx.close()


# ---- 2. receive_byte behind the excisor is receive_byte on the twin's output ----------------------------------------------------------------
def _int16_windows(cfg):
    """toned at SIR 0 and -10 dB, clean, noise only (mode 100: toned at 0 dB and clean) as the audio device's INT16 samples and as the doubles
    they widen to"""
    sigma, df = {8: (0.02, 317.0), 13: (0.01, 100.0), 100: (0.05, 100.0)}[cfg]
    t = er.toned_windows(cfg, 0.0, sigma, df, count=2)
    orc = t["orc"]
    if cfg == 100:
        wins, pls = [t["toned"][0], t["clean"][1]], [t["payload"][0], t["payload"][1]]
    else:
        rng = np.random.default_rng(cfg)
        wins = [t["toned"][0], er.add_tone(orc, t["clean"][1: 2], -10.0, df, CARRIER)[0], t["clean"][0], 0.05 * rng.standard_normal(t["clean"].shape[1])]
        pls = [t["payload"][0], t["payload"][1], t["payload"][0], None]
    wins = np.stack(wins)
    scale = 0.9 / np.max(np.abs(wins))                                       # inside the integer format's full scale, no clipping
    q = np.rint(wins * min(1.0, scale) * 32767.0).astype(np.int16)
    return orc, q, q.astype(np.float64) / 32768.0, pls


@pytest.mark.parametrize("cfg", [8, 13, 100])
def test_receive_byte_with_the_stage_on_is_the_oracle_on_the_twins_output(cfg):
    import torch
    orc, q, wins, pls = _int16_windows(cfg)
    W = len(wins)
    prm = dict(threshold=8.0) if cfg != 13 else {}
    clean, want_rep = _twin(wins, CARRIER, **prm)
    refs = [orc.receive_byte(clean[w], carrier=CARRIER) for w in range(W)]
    raw = [orc.receive_byte(wins[w], carrier=CARRIER) for w in range(W)]
    rx = _rx(cfg, max_batch=W)
    rx.set_excisor("welch", **prm)
    d = torch.from_numpy(wins).cuda()
    outs = {"device": rx.receive_byte_dev(d.data_ptr(), W, CARRIER)}
    reps = {"device": rx.excisor_report(0, W)}
    outs["host"] = rx.receive_byte(wins, CARRIER)
    reps["host"] = rx.excisor_report(0, W)
    outs["int16"] = rx.receive_byte(q, CARRIER)
    reps["int16"] = rx.excisor_report(0, W)
    rx.close()
    for src, out in outs.items():
        _same_report(reps[src], want_rep)
        for w in range(W):
            ref, st = refs[w], out["stats"][w]
            for k in ("iterations_done", "crc", "all_zeros", "message_decoded", "delay", "sync_trials", "frame_overflow_symbols"):
                assert st[k] == ref[k], (cfg, src, w, k, st[k], ref[k])
            if cfg < 100:
                assert st["coarse_metric"] == ref["coarse_metric"], (cfg, src, w)
                assert st["signal_strength_dbm"] == ref["signal_strength_dbm"], (cfg, src, w)
                assert st["freq_offset"] == ref["freq_offset"], (cfg, src, w)
                assert abs(st["mean_H"] - ref["mean_H"]) <= 1e-9 * max(1.0, abs(ref["mean_H"])), (cfg, src, w)
                assert abs(st["snr_db"] - ref["snr_db"]) <= 1e-4 * max(1.0, abs(ref["snr_db"])), (cfg, src, w)
            else:
                assert st["snr_db"] == ref["snr_db"]
            assert np.array_equal(out["payload"][w][: orc.payload_bytes], ref["payload"]), (cfg, src, w)
            assert out["state"][w]["delay_of_last_decoded_message"] == ref["state"].delay_of_last_decoded_message
    got = [bool(er.decoded(orc, refs[w], pls[w])) if pls[w] is not None else None for w in range(W)]
    before = [bool(er.decoded(orc, raw[w], pls[w])) if pls[w] is not None else None for w in range(W)]
    print("mode %d: decoded raw %s, behind the excisor %s; bins removed %s" % (cfg, before, got, want_rep["excised"]))
    assert want_rep["excised"][0] > 0 and want_rep["mask"][W - 1] == 0          # the toned window is cleaned, the last one is left alone
    if cfg == 8:
        assert before[:2] == [False, False] and got[:3] == [True, True, True]


def test_a_pipelined_host_call_keeps_the_reports_by_the_windows_row():
    """from 512 windows on a call from host memory is received in sub-batches: every window's result and report are those of the small call,
    and the reports lie at the window's row in the whole call"""
    orc, q, wins, pls = _int16_windows(8)
    rx = _rx(8, max_batch=520)
    rx.set_excisor("welch", threshold=8.0)
    small = rx.receive_byte(q, CARRIER)
    rep_small = rx.excisor_report(0, 4)
    assert rep_small["excised"][0] > 0
    big = rx.receive_byte(np.tile(q, (130, 1)), CARRIER)
    rep_big = rx.excisor_report(0, 520)
    rx.close()
    _same_report(rep_big, np.tile(rep_small, 130))
    for name in small["stats"].dtype.names:
        assert big["stats"][name].tobytes() == np.tile(small["stats"][name], 130).tobytes(), name
    assert big["payload"].tobytes() == np.tile(small["payload"], (130, 1)).tobytes()


# ---- 3. off is off again ---------------------------------------------------------------------------------------------------------------------
def test_on_then_off_is_a_context_that_never_had_the_stage():
    from oraclelib import Oracle
    from test_receive_byte import SPECS, make_windows
    wins, _ = make_windows(Oracle(8), SPECS, seed=108)
    plain = _rx(8, max_batch=len(SPECS))
    want = plain.receive_byte(wins, CARRIER + 5.0)
    plain.close()
    rx = _rx(8, max_batch=len(SPECS))
    rx.set_excisor("welch", threshold=4.0, guard=2)
    on = rx.receive_byte(wins, CARRIER + 5.0)
    assert rx.excisor() == ("welch", {"threshold": 4.0, "guard": 2, "max_bins": 16})
    rx.set_excisor("off")
    assert rx.excisor()[0] == "off"
    for _ in range(2):
        again = rx.receive_byte(wins, CARRIER + 5.0)
        for key in ("payload", "stats", "state"):
            assert again[key].tobytes() == want[key].tobytes(), key
    assert int(on["stats"]["message_decoded"].sum()) >= 1
    # measure_signal_only keeps the raw window whatever the setting
    level = rx.measure_signal_only(wins[:2], CARRIER)
    rx.set_excisor("welch")
    assert rx.measure_signal_only(wins[:2], CARRIER).tobytes() == level.tobytes()
    rx.close()


# ---- 4. a capture run ------------------------------------------------------------------------------------------------------------------------
def test_capture_run_with_a_clean_and_a_toned_capture():
    from mercury_amd import RxCapture
    from oraclelib import Oracle
    orc = Oracle(8)
    rx = _rx(8, max_batch=4)
    P = rx.Nofdm * 4
    hops = rx.receive_buffer_samples() // P + 45
    rng = np.random.default_rng(77)
    pl = rng.integers(0, 256, orc.payload_bytes)
    pb = orc.tx_passband(orc.payload_to_bits(pl))
    x = 0.02 * rng.standard_normal((2, hops * P))
    x[:, 60 * P + 123: 60 * P + 123 + pb.size] += pb
    x[1] = er.add_tone(orc, x[1: 2], 0.0, 317.0, CARRIER)[0]

    def run(setting):
        rx.set_excisor(setting)
        cap = RxCapture(rx, 2, CARRIER)
        ev = cap.run(x)
        cap.close()
        # (a structured scalar's padding bytes are whatever the library's stack held: the fields' own bytes)
        return [[(hop, b"".join(st[k].tobytes() for k in st.dtype.names), p.tobytes()) for s, hop, st, p in ev if s == which] for which in (0, 1)]

    off, on = run("off"), run("welch:thr=8")
    rx.close()
    print("capture run: events of the clean capture off / on %d / %d, of the toned capture %d / %d" % (len(off[0]), len(on[0]), len(off[1]), len(on[1])))
    assert len(off[0]) >= 1 and off[0] == on[0]
    assert all(p == pl.astype(np.uint8).tobytes() for _, _, p in off[0])
    assert len(off[1]) == 0 and len(on[1]) >= 1 and all(p == pl.astype(np.uint8).tobytes() for _, _, p in on[1])


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    from mercury_amd import ExcisorParams, MgpuError
    rx = _rx(8, max_batch=2)
    with pytest.raises(MgpuError):
        rx.excisor_report()                                               # never set: no report
    for before in (("off", {}), ("welch", dict(threshold=30.0, guard=2, max_bins=8))):
        rx.set_excisor(before[0], **before[1])
        state = rx.excisor()
        for kw in (dict(threshold=1.5), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(guard=-1), dict(guard=5),
                   dict(max_bins=0), dict(max_bins=33)):
            with pytest.raises(MgpuError) as e:
                rx.set_excisor("welch", **kw)
            assert e.value.code == 1, kw                                  # MGPU_ERR_ARG
            assert rx.excisor() == state
        prm = ExcisorParams(12.0, 1, 16)
        for size in (0, 8, C.sizeof(prm) + 8):
            assert rx.lib.mgpu_set_excisor(rx.h, 1, C.byref(prm), size) == 1
            assert rx.lib.mgpu_get_excisor(rx.h, C.byref(C.c_int()), C.byref(prm), size) == 1
        assert rx.lib.mgpu_set_excisor(rx.h, 2, C.byref(prm), C.sizeof(prm)) == 1
        assert rx.lib.mgpu_set_excisor(rx.h, -1, C.byref(prm), C.sizeof(prm)) == 1
        assert rx.excisor() == state
    assert rx.lib.mgpu_set_excisor(rx.h, 1, None, C.sizeof(ExcisorParams)) == 0            # NULL: the defaults
    assert rx.excisor() == ("welch", {"threshold": 12.0, "guard": 1, "max_bins": 16})
    assert rx.excisor_report(0, 2)["excised"].tolist() == [0, 0] and rx.lib.mgpu_get_excisor_report(rx.h, 1, 2, None) == 1
    with pytest.raises(MgpuError):
        rx.set_excisor("median")
    with pytest.raises(MgpuError):
        rx.excise(np.zeros((1, 16)), float("nan"))
    assert rx.lib.mgpu_excise_dev(rx.h, None, 1, 16, CARRIER, None, None, None) == 1
    rx.close()

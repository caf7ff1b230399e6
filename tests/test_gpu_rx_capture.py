"""The reference's receive loop over continuous captures, batched on the GPU (include/mercury_capture.h, mercury_amd.RxCapture).

Yardsticks: the host twins (tests/test_rx_capture_host.py pins them to the capture thread and to the reference's loop on the CPU), the
reference's own RX_RAND_process_main driven hop by hop (oracle/_ref, pass-through mode: its object code on the CPU), and the same loop
restated in Python over mgpu_receive_byte_batch_samples on windows built on the host."""
import numpy as np
import pytest

import capture_ref as cr
from band_links import canon as _canon
from mercury_amd import RxCapture, RxPhy
from mercury_amd.physical_layer import host_capture_init_state, host_capture_process
from oraclelib import MODE_REFERENCE, RefTelecomSystemGpu

pytestmark = pytest.mark.gpu
MAX_ITERS = 10
FORMATS = (np.float64, np.int32, np.int16, np.float32)


def _torch():
    import torch
    return torch


def _samples(rng, shape, fmt):
    fmt = np.dtype(fmt)
    if fmt == np.int32:
        return rng.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)
    if fmt == np.int16:
        return rng.integers(-2 ** 15, 2 ** 15, shape).astype(np.int16)
    return rng.standard_normal(shape).astype(fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("on_device", [False, True])
def test_device_windows_equal_the_host_twin(fmt, on_device):
    """after sequences of feeds every window is the capture thread's (closed form, pinned to the host twin) bit for bit: all formats, host and
    device input, H in {1, 3, 17}, S in {1, 5, 300} (max_batch 128: the gathers split; max_hops 4: feeds split; > 71 hops: the ring wraps)"""
    rx = RxPhy(16, max_iters=MAX_ITERS, max_batch=128)
    rng = np.random.default_rng(17 + FORMATS.index(fmt) + 10 * on_device)
    for H, S in ((1, 5), (3, 300), (17, 1), (17, 300)):
        sp = rx.receive_buffer_samples()
        init = (rng.integers(0, 1000, (S, sp)) - 500) / 1000.0
        cap = RxCapture(rx, S, 1500.0, initial_windows=init, max_hops=4)
        P = cap.P
        fed = [[] for _ in range(S)]
        n_feeds = -(-80 // H)
        for f in range(n_feeds):
            x = _samples(rng, (S, H * P), fmt)
            cap.feed(_torch().from_numpy(x).cuda() if on_device else x)
            for s in range(S):
                fed[s].append(cr.widen(x[s]))
            if f in (0, n_feeds // 2, n_feeds - 1):
                for s in sorted({0, S // 2, S - 1}):
                    want = cr.closed_form(init[s], np.concatenate(fed[s]))
                    assert np.array_equal(cap.window(s).view(np.uint64), want.view(np.uint64)), (H, S, f, s)
        st = cap.state(S - 1)
        assert st["data_ready"] == 1 and st["frames_to_read"] == 0 and st["n_under"] == n_feeds * H - 1
        cap.close()
    rx.close()


def _compare_held(cfg, where, st, held, attempted):
    h = st["held"]
    ints = dict(iterations_done=h["iterations_done"], delay=h["delay"], delay_of_last_decoded_message=st["link"]["delay_of_last_decoded_message"],
                sync_trials=h["sync_trials"], message_decoded=h["message_decoded"], crc=h["crc"], all_zeros=h["all_zeros"],
                mfsk_search_raw=st["mfsk_search_raw"], frame_overflow_symbols=h["frame_overflow_symbols"])
    for k, v in ints.items():
        if k in ("crc", "all_zeros") and not attempted:       # not set by the reference's constructor (telecom_system.cc:38-51)
            continue
        assert int(v) == held[k], (cfg, where, k, int(v), held[k])
    dbl = dict(freq_offset=h["freq_offset"], freq_offset_of_last_decoded_message=st["link"]["freq_offset_of_last_decoded_message"], SNR=h["snr_db"],
               signal_stregth_dbm=h["signal_strength_dbm"], coarse_metric=h["coarse_metric"])
    for k, v in dbl.items():
        if k == "coarse_metric" and cfg >= 100:                # never written in the MFSK modes, nor initialised by the constructor
            continue
        a, b = float(v), held[k]
        # bit for bit where the device restates the host's libm; the mixer / Moose / signal-level doubles to 1e-9, as
        # tests/test_reference_dropin.py::test_reference_receive_byte_replaced_wholesale
        assert a == b or abs(a - b) <= 1e-9 * max(1.0, abs(b)), (cfg, where, k, a, b)


def _content(ref, rng, S, hops, fmt=np.int32):
    """S captures: noise with frames (two back to back, one later) in every capture, as the audio device's samples"""
    P = ref.info["Nofdm"] * 4
    streams, sent = [], []
    for s in range(S):
        x, pl = cr.capture_stream(ref, rng, hops, cr.frame_plan(ref, hops, rng))
        streams.append(cr.to_format(x, fmt).reshape(hops, P))
        sent.append(pl)
    return np.stack(streams), sent


@pytest.mark.parametrize("cfg", [0, 8, 13, 16, 100, 101, "100ctrl"])
def test_run_equals_the_reference_loop(cfg):
    """per hop and per capture, feed(1) + process() gives what the reference's RX_RAND_process_main gives on the restated windows (whether
    receive_byte ran, decoded, payload, frames_to_read, every held receive_stats field), and run(H) gives the same decoded frames and final
    state in one call. "100ctrl": MFSK control mode (short frames on the air; the loop still counts data_container.Nsymb)."""
    ctrl = cfg == "100ctrl"
    cfg = 100 if ctrl else cfg
    S = 1 if ctrl else 2
    refs = [RefTelecomSystemGpu(cfg, MODE_REFERENCE, max_iters=MAX_ITERS) for _ in range(S)]
    if ctrl:
        refs[0].set_ctrl_mode(True)
    rx = RxPhy(cfg, max_iters=MAX_ITERS, max_batch=8, mfsk_ctrl_mode=ctrl)
    P = rx.Nofdm * 4
    bufn = rx.receive_buffer_samples() // P
    hops = 2 * bufn
    rng = np.random.default_rng(4000 + cfg + ctrl)
    x, sent = _content(refs[0], rng, S, hops)
    init = (rng.integers(0, 1000, (S, bufn * P)) - 500) / 1000.0
    a = RxCapture(rx, S, refs[0].carrier(), initial_windows=init)
    b = RxCapture(rx, S, refs[0].carrier(), initial_windows=init)
    per_hop = []
    for h in range(hops):
        a.feed(x[:, h: h + 1].reshape(S, P))
        per_hop.append((a.process(), [a.state(s) for s in range(S)]))
    events = b.run(x.reshape(S, hops * P))
    decoded = 0
    for s in range(S):
        recs = cr.reference_loop(refs[s], init[s], x[s])
        attempted = ran_once = False
        for rec in recs:
            out, sts = per_hop[rec["hop"]]
            where = (s, rec["hop"])
            assert bool(out["ran"][s]) == rec["ran"], where
            assert bool(out["ran"][s] and out["stats"][s]["message_decoded"]) == (rec["decoded"] is not None), where
            if rec["decoded"]:
                assert list(out["payload"][s][: rx.payload_bytes]) == rec["decoded"][1], where
                assert int(out["stats"][s]["iterations_done"]) == rec["decoded"][0], where
                assert ctrl or any(rec["decoded"][1] == list(p) for p in sent[s]), where
                decoded += 1
            assert int(sts[s]["frames_to_read"]) == rec["frames_to_read"], where
            attempted = attempted or rec["held"]["iterations_done"] != -1
            ran_once = ran_once or rec["ran"]
            if ran_once:                                      # before, the reference holds what its constructor left, partly uninitialised
                _compare_held(cfg, where, sts[s], rec["held"], attempted)
        refs[s].close()
        assert _canon(b.state(s)) == _canon(a.state(s))
    want = [(s, h, out["stats"][s], out["payload"][s][: rx.payload_bytes]) for h, (out, _) in enumerate(per_hop) for s in range(S)
            if out["ran"][s] and out["stats"][s]["message_decoded"]]
    assert len(events) == len(want) == decoded >= (1 if ctrl else 2), (cfg, len(events), decoded)
    for e, w in zip(events, want):
        assert e[0] == w[0] and e[1] == w[1] and _canon(e[2]) == _canon(w[2]) and np.array_equal(e[3], w[3])
    a.close(), b.close(), rx.close()


@pytest.mark.parametrize("cfg,k,search_raw", [(8, 3, 0), (13, 4, 0), (100, 5, 40)])
def test_lagging_process_equals_the_reference(cfg, k, search_raw):
    """feed(k) + process(): the reference's loop k - 1 hops behind, nUnder_processing_events carried as the capture thread carries it
    (growing past k - 1 over calls without a decode) and, in cfg 100, the MFSK search start max(0, mfsk_search_raw - nUnder)"""
    ref = RefTelecomSystemGpu(cfg, MODE_REFERENCE, max_iters=MAX_ITERS)
    rx = RxPhy(cfg, max_iters=MAX_ITERS, max_batch=8)
    P = rx.Nofdm * 4
    bufn = rx.receive_buffer_samples() // P
    hops = 2 * bufn - (2 * bufn) % k
    rng = np.random.default_rng(4500 + cfg)
    x, sent = _content(ref, rng, 1, hops, np.float32)
    init = (rng.integers(0, 1000, bufn * P) - 500) / 1000.0
    cap = RxCapture(rx, 1, ref.carrier(), initial_windows=init[None])
    st = cap.state(0)
    st["mfsk_search_raw"] = search_raw
    cap.set_state(0, st)
    recs = cr.reference_loop(ref, init, x[0], k=k, search_raw=search_raw)
    attempted, ran_once, decoded = False, False, 0
    for c, rec in enumerate(recs):
        cap.feed(x[:, c * k: (c + 1) * k].reshape(1, k * P))
        out = cap.process()
        s = cap.state(0)
        assert bool(out["ran"][0]) == rec["ran"] and bool(out["ran"][0] and out["stats"][0]["message_decoded"]) == (rec["decoded"] is not None), c
        if rec["decoded"]:
            assert list(out["payload"][0][: rx.payload_bytes]) == rec["decoded"][1]
            decoded += 1
        assert (int(s["frames_to_read"]), int(s["n_under"])) == (rec["frames_to_read"], rec["n_under"]), c
        attempted = attempted or rec["held"]["iterations_done"] != -1
        ran_once = ran_once or rec["ran"]
        if ran_once:
            _compare_held(cfg, c, s, rec["held"], attempted)
    assert decoded >= 1 and max(r["n_under"] for r in recs) > k - 1
    ref.close(), cap.close(), rx.close()


def test_mixed_active_sets_at_scale():
    """1024 captures x 64 hops of mode 8, staggered frames_to_read, frames in an eighth of them: per hop, the captures that ran, their
    statistics and payloads equal the loop restated in Python (host twins) over mgpu_receive_byte_batch_samples on host-built windows"""
    S, hops = 1024, 64
    rx = RxPhy(8, max_iters=MAX_ITERS, max_batch=S)
    ref = RefTelecomSystemGpu(8, MODE_REFERENCE)
    P = rx.Nofdm * 4
    sp = rx.receive_buffer_samples()
    rng = np.random.default_rng(99)
    hist = np.round(rng.standard_normal((S, sp - 1 + hops * P), dtype=np.float32) * np.float32(0.01 * 2 ** 30)).astype(np.int32)
    frame = ref.transmit_byte(rng.integers(0, 256, ref.payload_bytes))
    for s in range(0, S, 8):
        off = int(rng.integers(0, hist.shape[1] - frame.size))
        hist[s, off: off + frame.size] = np.clip(hist[s, off: off + frame.size] + np.round(frame * 2 ** 30), -2 ** 31 + 1, 2 ** 31 - 1).astype(np.int32)
    ref.close()
    last = rng.integers(-1000, 1000, S).astype(np.int32)
    init = np.concatenate([cr.widen(hist[:, : sp - 1]), cr.widen(last)[:, None]], axis=1)
    cap = RxCapture(rx, S, 1500.0, initial_windows=init)
    del init
    g = cap.geometry
    states = []
    for s in range(S):
        st = host_capture_init_state(g)
        st["frames_to_read"] = int(rng.integers(0, 30))
        cap.set_state(s, st)
        states.append(st)
    mixed = 0
    for h in range(hops):
        new = hist[:, sp - 1 + h * P: sp - 1 + (h + 1) * P]
        cap.feed(np.ascontiguousarray(new))
        out = cap.process()
        for st in states:                                            # capture prep's counters (pinned by the host tests)
            if st["data_ready"] == 1:
                st["n_under"] += 1
            st["frames_to_read"] = max(0, int(st["frames_to_read"]) - 1)
            st["data_ready"] = 1
        act = [s for s in range(S) if states[s]["frames_to_read"] == 0]
        mixed += 0 < len(act) < S
        if act:
            win = np.concatenate([hist[act, (h + 1) * P: (h + 1) * P + sp - 1], last[act, None]], axis=1)
            links = np.stack([np.array(states[s]["link"]) for s in act])
            links["mfsk_search_start"] = [max(0, int(states[s]["mfsk_search_raw"]) - int(states[s]["n_under"])) for s in act]
            res = rx.receive_byte(np.ascontiguousarray(win), 1500.0, state=links)
            for i, s in enumerate(act):
                host_capture_process(g, states[s], res["stats"][i], res["state"][i])
        for s in range(S):
            if states[s]["data_ready"]:
                host_capture_process(g, states[s])
        assert sorted(np.flatnonzero(out["ran"])) == act, h
        for i, s in enumerate(act):
            assert _canon(out["stats"][s]) == _canon(res["stats"][i]), (h, s)
            assert np.array_equal(out["payload"][s], res["payload"][i]), (h, s)
        if h % 16 == 15:
            for s in range(0, S, 97):
                assert _canon(cap.state(s)) == _canon(states[s]), (h, s)
    assert mixed >= 8
    cap.close(), rx.close()


def test_run_is_feed_and_process_per_hop_and_state_round_trips():
    """run(H) = H x (feed(1) + process()): the same decoded frames, states and windows; get_state / set_state round-trip"""
    rx = RxPhy(16, max_iters=MAX_ITERS, max_batch=16)
    ref = RefTelecomSystemGpu(16, MODE_REFERENCE)
    S, hops = 4, 80
    rng = np.random.default_rng(5)
    x, _ = _content(ref, rng, S, hops, np.int16)
    carrier = ref.carrier()
    ref.close()
    init = rng.standard_normal((S, rx.receive_buffer_samples())) * 0.01
    a = RxCapture(rx, S, carrier, initial_windows=init, max_hops=7)
    b = RxCapture(rx, S, carrier, initial_windows=init)
    events = a.run(x.reshape(S, -1))
    want = []
    for h in range(hops):
        b.feed(x[:, h])
        out = b.process()
        want += [(s, h, _canon(out["stats"][s]), out["payload"][s][: rx.payload_bytes].tobytes()) for s in range(S)
                 if out["ran"][s] and out["stats"][s]["message_decoded"]]
    assert [(e[0], e[1], _canon(e[2]), e[3].tobytes()) for e in events] == want and len(want) >= 1
    for s in range(S):
        assert _canon(a.state(s)) == _canon(b.state(s))
        assert np.array_equal(a.window(s), b.window(s))
    st = a.state(1)
    st["mfsk_search_raw"], st["n_under"] = 7, 3
    a.set_state(2, st)
    assert _canon(a.state(2)) == _canon(st)
    bad = st.copy()
    bad["data_ready"] = 5
    with pytest.raises(Exception):
        a.set_state(0, bad)
    a.close(), b.close(), rx.close()


def test_create_use_destroy_gives_the_memory_back():
    """create / feed / process / run / window / destroy cycles (rings, gather buffer, staging) leave the device's free memory where it was"""
    import gc
    torch = _torch()

    def free_hbm():
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info()[0]

    rx = RxPhy(16, max_iters=MAX_ITERS, max_batch=64)
    rng = np.random.default_rng(6)
    S = 64
    P = rx.Nofdm * 4

    def cycle():
        cap = RxCapture(rx, S, 1500.0)
        x = (rng.standard_normal((S, 30 * P)) * 2 ** 20).astype(np.int32)
        cap.run(x)
        cap.feed(x[:, : 3 * P])
        cap.process()
        cap.window(3)
        return cap

    cycle().close()                                       # the context's receive_byte workspace is sized on first use
    first = free_hbm()
    for c in range(6):
        cap = cycle()
        in_use = first - free_hbm()
        cap.close()
        assert in_use >= S * rx.receive_buffer_samples() * 8, in_use
        after = free_hbm()
        assert abs(after - first) < 64 << 20, (c, first, after)
    rx.close()

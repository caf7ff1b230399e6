"""The continuous-capture receive loop's host twins (include/mercury_capture.h), without a GPU.

mgpu_host_capture_prep is one hop of the reference's capture-prep thread (audioio.c:1035-1057) and mgpu_host_capture_process the
bookkeeping of RX_SHM_process_main / RX_RAND_process_main around one receive_byte result (telecom_system.cc:2304-2377). The device path
(mgpu_capture_*) runs the same two functions. Here they are pinned against a numpy restatement of the capture thread and against the
reference's own receive loop (its object code, pass-through mode), hop by hop over continuous captures with frames in them."""
import numpy as np
import pytest

import capture_ref as cr
from mercury_amd.physical_layer import (CAPTURE_STATE_DTYPE, LINK_STATE_DTYPE, RECEIVE_STATS_DTYPE, CaptureGeometry, host_capture_init_state,
                                        host_capture_prep, host_capture_process)
from oraclelib import MODE_REFERENCE, RefTelecomSystemGpu

FORMATS = (np.float64, np.int32, np.int16, np.float32)


def _geometry(buffer_nsymb, nsymb, pre, P, mfsk=0):
    return CaptureGeometry(buffer_nsymb, nsymb, pre, P, mfsk)


def _random_samples(rng, n, fmt):
    fmt = np.dtype(fmt)
    if fmt == np.int32:
        return rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    if fmt == np.int16:
        return rng.integers(-2 ** 15, 2 ** 15, n).astype(np.int16)
    return rng.standard_normal(n).astype(fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("H", [1, 2, 7])
def test_capture_prep_twin_is_the_capture_thread(fmt, H):
    """shift_left, the write at sp - P - 1 and the counters, hop by hop, equal the numpy restatement of audioio.c:1035-1057 bit for bit;
    the window is also the closed form (the last sp - 1 samples of history, window[sp-1] pinned at its initial value)"""
    rng = np.random.default_rng(100 + H)
    P, bufn = 24, 9
    g = _geometry(bufn, 4, 2, P)
    init = (rng.integers(0, 1000, bufn * P) - 500) / 1000.0           # data_container.cc:168-171
    w_twin, w_ref = init.copy(), init.copy()
    st = host_capture_init_state(g)
    assert st["frames_to_read"] == 6 and st["n_under"] == 0 and st["data_ready"] == 0 and st["link"]["delay_of_last_decoded_message"] == -1
    st["frames_to_read"] = 1000                                          # no process step below runs receive_byte
    ref = dict(n_under=0, frames_to_read=1000, data_ready=0)
    fed = []
    for call in range(4):
        for h in range(H):
            hop = _random_samples(rng, P, fmt)
            host_capture_prep(g, w_twin, hop, st)
            cr.prep(w_ref, ref, hop, P)
            fed.append(cr.widen(hop))
            assert np.array_equal(w_twin.view(np.uint64), w_ref.view(np.uint64)), (call, h)
            assert (int(st["n_under"]), int(st["frames_to_read"]), int(st["data_ready"])) == (ref["n_under"], ref["frames_to_read"], 1)
        assert np.array_equal(w_twin, cr.closed_form(init, np.concatenate(fed)))
        assert w_twin[-1] == init[-1]
        assert not host_capture_process(g, st) and st["data_ready"] == 0
        ref["data_ready"] = 0
    assert ref["n_under"] == 4 * (H - 1)


def test_process_twin_rules():
    """the decode branch with its fallback formula and the n_under reset; the no-decode branch; data_ready == 0 does nothing"""
    g = _geometry(85, 24, 4, 1088)
    st = host_capture_init_state(g)
    st["frames_to_read"], st["data_ready"], st["n_under"] = 0, 1, 3
    r = np.zeros((), RECEIVE_STATS_DTYPE)
    link = np.zeros((), LINK_STATE_DTYPE)
    r["message_decoded"], r["delay"], r["iterations_done"] = 1, 40 * 1088 + 5, 7
    link["delay_of_last_decoded_message"] = r["delay"]
    assert host_capture_process(g, st, r, link)
    # frames_left = 85 - (40 + 28) = 17, frames_to_read = 28 - 17 - 3 = 8
    assert st["frames_to_read"] == 8 and st["n_under"] == 0 and st["data_ready"] == 0
    assert st["link"]["delay_of_last_decoded_message"] == r["delay"] + 20 * 1088 and st["held"]["iterations_done"] == 7
    st2 = host_capture_init_state(g)
    st2["frames_to_read"], st2["data_ready"], st2["n_under"] = 0, 1, 30        # 28 - 17 - 30 < 0: the fallback
    assert host_capture_process(g, st2, r, link) and st2["frames_to_read"] == 11
    st3 = host_capture_init_state(g)
    st3["frames_to_read"], st3["data_ready"] = 0, 1
    st3["link"]["delay_of_last_decoded_message"] = 1500
    r["message_decoded"], r["iterations_done"] = 0, -1
    link["delay_of_last_decoded_message"] = 1500
    assert host_capture_process(g, st3, r, link) and st3["link"]["delay_of_last_decoded_message"] == 1500 - 1088
    st3["data_ready"] = 1
    assert host_capture_process(g, st3, r, np.array(st3["link"])) and st3["link"]["delay_of_last_decoded_message"] == -1
    assert st3["held"]["iterations_done"] == -1
    assert not host_capture_process(g, st3)                                    # data_ready == 0
    with pytest.raises(Exception):
        st3["data_ready"] = 1
        host_capture_process(g, st3)                                           # it would run: the result is required


def _twin_over_reference(cfg, k, seed):
    ref = RefTelecomSystemGpu(cfg, MODE_REFERENCE, max_iters=10)
    info = ref.info
    P = info["Nofdm"] * 4
    bufn = ref.buffer_samples() // P
    mfsk = 1 if cfg >= 100 else 0
    g = _geometry(bufn, info["Nsymb"], info["preamble_nsymb"], P, mfsk)
    rng = np.random.default_rng(seed)
    hops = 2 * bufn
    x, sent = cr.capture_stream(ref, rng, hops, cr.frame_plan(ref, hops, rng))
    stream = x.reshape(hops, P)
    init = (rng.integers(0, 1000, bufn * P) - 500) / 1000.0
    w = init.copy()
    st = host_capture_init_state(g)
    hop_iter = iter(range(hops))

    def on_call(rec, w_ref):
        for _ in range(k):
            host_capture_prep(g, w, stream[next(hop_iter)], st)
        assert np.array_equal(w, w_ref)
        h = rec["held"]
        r = np.zeros((), RECEIVE_STATS_DTYPE)
        link = np.array(st["link"])
        if rec["ran"]:
            r["message_decoded"] = 1 if rec["decoded"] else 0
            r["delay"], r["iterations_done"], r["sync_trials"] = h["delay"], h["iterations_done"], h["sync_trials"]
            r["crc"], r["all_zeros"], r["snr_db"], r["signal_strength_dbm"] = h["crc"], h["all_zeros"], h["SNR"], h["signal_stregth_dbm"]
            r["freq_offset"], r["coarse_metric"] = h["freq_offset"], h["coarse_metric"]
            if rec["decoded"]:                                             # receive_byte's own update (telecom_system.cc:1427)
                link["delay_of_last_decoded_message"] = h["delay"]
                link["freq_offset_of_last_decoded_message"] = h["freq_offset_of_last_decoded_message"]
        assert host_capture_process(g, st, r, link) == rec["ran"]
        assert int(st["frames_to_read"]) == rec["frames_to_read"], (cfg, k, rec["hop"])
        assert int(st["n_under"]) == rec["n_under"]
        assert int(st["link"]["delay_of_last_decoded_message"]) == h["delay_of_last_decoded_message"], (cfg, k, rec["hop"])
        if rec["ran"]:
            assert int(st["held"]["delay"]) == h["delay"] and int(st["held"]["message_decoded"]) == h["message_decoded"]

    recs = cr.reference_loop(ref, init, stream, k=k, on_call=on_call)
    ref.close()
    decoded = [r for r in recs if r["decoded"]]
    assert len(decoded) >= 2, (cfg, k, len(decoded))
    for d in decoded:
        assert any(d["decoded"][1] == list(s) for s in sent)
    return recs


pytestmark_ref = pytest.mark.skipif(not RefTelecomSystemGpu.available(), reason="oracle/_ref/libmercury_ref_ts_gpu.so not built (needs the reference)")


@pytestmark_ref
@pytest.mark.parametrize("cfg", [8, 16, 100])
def test_bookkeeping_twin_follows_the_reference_loop(cfg):
    """hop by hop over a continuous capture (noise, two frames back to back, a third later), the twin's frames_to_read and
    delay_of_last_decoded_message after every process step equal those of the reference's RX_RAND_process_main"""
    _twin_over_reference(cfg, 1, 500 + cfg)


@pytestmark_ref
@pytest.mark.parametrize("cfg,k", [(8, 3), (16, 4), (100, 5)])
def test_bookkeeping_twin_follows_the_reference_loop_when_it_lags(cfg, k):
    """the process thread k - 1 hops behind: nUnder_processing_events grows by k - 1 per call until a decode resets it, and steers both
    the frames_to_read after the next decode and the MFSK search start"""
    recs = _twin_over_reference(cfg, k, 700 + cfg)
    assert max(r["n_under"] for r in recs) > k - 1

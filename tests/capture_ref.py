"""The reference's receive loop over a continuous capture, restated for the tests of include/mercury_capture.h.

capture prep (audioio.c:1035-1057) is restated in numpy; the process step is the reference's own RX_RAND_process_main
(telecom_system.cc:2102-2190, the same bookkeeping as RX_SHM_process_main :2304-2377) on a RefTelecomSystemGpu in pass-through mode,
driven hop by hop with frames_to_read and nUnder_processing_events carried as the capture thread carries them."""
import re

import numpy as np

WIDEN = {np.dtype(np.int32): 2147483647.0, np.dtype(np.int16): 32768.0}


def widen(samples):
    """audioio.c:893-936 (and mgpu_widen_capture_kernel): INT32 / INT_MAX, INT16 / 32768.0, FLOAT32 widened, doubles as they are"""
    x = np.asarray(samples)
    d = WIDEN.get(x.dtype)
    return x.astype(np.float64) / d if d else x.astype(np.float64)


def prep(window, state, hop, P):
    """one hop of radio_capture_prep_thread on a numpy window (in place); state: dict(n_under, frames_to_read, data_ready)"""
    sp = window.size
    if state["data_ready"] == 1:
        state["n_under"] += 1
    window[: sp - P] = window[P:].copy()                     # shift_left (misc.cc:26-32)
    window[sp - P - 1: sp - 1] = widen(hop)                  # loc = sp - P - 1 (:1035, :1051)
    state["frames_to_read"] = max(0, state["frames_to_read"] - 1)
    state["data_ready"] = 1


def closed_form(initial, fed):
    """window[0 .. sp-2] = the last sp-1 samples of initial[0 .. sp-2] followed by everything fed; window[sp-1] = initial[sp-1]"""
    sp = initial.size
    h = np.concatenate([initial[: sp - 1], fed])
    return np.concatenate([h[-(sp - 1):], initial[-1:]])


def decoded_lines(text):
    """what RX_RAND_process_main prints for a decoded frame (telecom_system.cc:2130-2146): iterations, bytes, statistics"""
    m = re.search(r"Frame decoded in (\d+) iterations\. Data: \n((?:0x[0-9a-f]+, )*)\n(.*)", text)
    return None if not m else (int(m.group(1)), [int(t, 16) for t in m.group(2).replace(",", " ").split()], m.group(3).strip())


def frame_hops(ref):
    return ref.info["preamble_nsymb"] + ref.info["Nsymb"]


def capture_stream(ref, rng, hops, starts, noise=0.01):
    """[hops * P] doubles of noise with the reference's transmit_byte frames added at the sample offsets `starts`; -> (stream, payloads)"""
    P = ref.info["Nofdm"] * 4
    x = rng.standard_normal(hops * P) * noise
    sent = []
    for s in starts:
        pl = rng.integers(0, 256, ref.payload_bytes).astype(np.int32)
        pb = ref.transmit_byte(pl)
        n = min(pb.size, x.size - s)
        x[s: s + n] += pb[:n]
        sent.append(pl.astype(np.uint8))
    return x, sent


def frame_plan(ref, hops, rng):
    """sample offsets of three frames: two back to back (the second arrives while frames_to_read > 0), one later at a random offset"""
    P, F = ref.info["Nofdm"] * 4, frame_hops(ref)
    a = 2 * P + int(rng.integers(0, P))
    b = a + F * P + int(rng.integers(0, P // 4))
    c = b + F * P + int(rng.integers(3, 8)) * P + int(rng.integers(0, P))
    return [s for s in (a, b, c) if s + F * P <= hops * P]


def to_format(x, fmt):
    """the doubles of a stream as the audio device's samples of dtype fmt (float64 unchanged)"""
    fmt = np.dtype(fmt)
    if fmt == np.float64:
        return x.copy()
    if fmt == np.float32:
        return x.astype(np.float32)
    scale = 2147483647.0 if fmt == np.int32 else 32767.0
    return np.clip(np.round(x * scale * 0.5), -scale, scale).astype(fmt)


def reference_loop(ref, initial, stream, k=1, search_raw=0, on_call=None):
    """The reference's receive loop over one capture: k hops of capture prep (restated) per RX_RAND_process_main call (the reference's
    object code). stream: [hops, P] samples (any format, widened here); initial: the starting window. Returns one dict per call:
    ran, decoded (None or (iterations, bytes, stats line)), frames_to_read, n_under (as the call left them), held receive_stats."""
    P = stream.shape[1]
    w = np.array(initial, np.float64)
    st = dict(n_under=0, frames_to_read=frame_hops(ref), data_ready=0)
    out = []
    for h0 in range(0, stream.shape[0] - k + 1, k):
        for j in range(k):
            prep(w, st, stream[h0 + j], P)
        ref.set_loop_members(n_under=st["n_under"], search_raw=search_raw)
        ran = st["frames_to_read"] == 0
        text, st["frames_to_read"] = ref.rx_rand_process_main(w, st["frames_to_read"])
        dec = decoded_lines(text)
        if dec:
            st["n_under"] = 0                                      # telecom_system.cc:2158
        st["data_ready"] = 0
        rec = dict(hop=h0 + k - 1, ran=ran, decoded=dec, frames_to_read=st["frames_to_read"], n_under=st["n_under"],
                   held=ref.held_receive_stats())
        out.append(rec)
        if on_call:
            on_call(rec, w)
    return out

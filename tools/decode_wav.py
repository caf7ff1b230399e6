#!/usr/bin/env python3
"""Decode a PCM WAV recording of Mercury audio at whatever rate it was made: every channel of the file becomes one continuous capture,
the samples go through the rational resampler into the receive loop (RxCapture.run_resampled, include/ext/mercury_resampler.h) and the
decoded frames are printed, one JSON line each, with the time of the hop after which each was decoded.

Any rate the resampler's rule accepts (8000, 11025, 12000, 16000, 22050, 32000, 44100, 48000, 96000, 192000 Hz ...), 16- or 32-bit PCM.
usage: decode_wav.py FILE --mode N [--carrier 1471.875] [--trials 2] [--block 8192] [--tail-hops 4]"""
import argparse
import json
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mercury_amd import MgpuError, Resampler, RxCapture, RxPhy  # noqa: E402


def read_wav(path):
    """-> (rate, samples [channels, n] int16 or int32)"""
    with wave.open(path, "rb") as w:
        if w.getcomptype() != "NONE":
            raise SystemExit("%s: compressed WAV (%s): PCM only" % (path, w.getcomptype()))
        width, channels, rate = w.getsampwidth(), w.getnchannels(), w.getframerate()
        if width not in (2, 4):
            raise SystemExit("%s: %d-bit samples: 16- or 32-bit PCM only" % (path, 8 * width))
        raw = w.readframes(w.getnframes())
    x = np.frombuffer(raw, "<i2" if width == 2 else "<i4").reshape(-1, channels)
    return rate, np.ascontiguousarray(x.T.astype(np.int16 if width == 2 else np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("file")
    ap.add_argument("--mode", type=int, required=True, help="the Mercury configuration (0..16)")
    ap.add_argument("--carrier", type=float, default=48000.0 * 50 / 256 / 4 / 2 + 300, help="carrier in Hz (1471.875)")
    ap.add_argument("--trials", type=int, default=2, help="time_sync_trials_max")
    ap.add_argument("--block", type=int, default=8192, help="input samples per call (at most the resampler's max_in)")
    ap.add_argument("--tail-hops", type=int, default=4, help="hops of silence fed behind the file, for a frame that ends with it")
    a = ap.parse_args()
    rate, x = read_wav(a.file)
    S, n = x.shape
    rx = RxPhy(a.mode, max_batch=max(S, 2))
    try:
        rs = Resampler(rx, rate, 48000, S=S)
    except MgpuError as e:
        raise SystemExit("%s: %d Hz: %s" % (a.file, rate, e))
    cap = RxCapture(rx, S, a.carrier, trials_max=a.trials)
    tail = np.zeros((S, -(-a.tail_hops * cap.P * rs.M // rs.L)), x.dtype)
    x = np.concatenate([x, tail], axis=1)
    block, hop0, decoded = min(a.block, rs.max_in), 0, 0
    for at in range(0, x.shape[1], block):
        events, hops = cap.run_resampled(rs, np.ascontiguousarray(x[:, at: at + block]))
        for capture, hop, stats, payload in events:
            decoded += 1
            print(json.dumps({"channel": capture, "hop": hop0 + hop, "time_s": round((hop0 + hop + 1) * cap.P / 48000.0, 4),
                              "crc": int(stats["crc"]), "iterations": int(stats["iterations_done"]), "snr_db": round(float(stats["snr_db"]), 2),
                              "payload_hex": payload.tobytes().hex()}), flush=True)
        hop0 += hops
    print(json.dumps({"file": a.file, "rate": rate, "channels": S, "samples": n, "L": rs.L, "M": rs.M, "delay_out_samples": rs.delay,
                      "hops": hop0, "decoded": decoded}))
    rs.close(), cap.close(), rx.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the rational resampler (include/ext/mercury_resampler.h) costs. Two measurements, one JSON line each:

  stage   mgpu_resamp_process_dev alone at 44100 -> 48000, float32 samples resident on the device, the inputs of 16 hops (15994) per
          stream and call, S in --streams: device-event time per call over --reps calls on one stream, and input samples per second;
  loop    RxCapture.run_resampled on 44.1 kHz audio against RxCapture.run on audio already at 48 kHz, 16 hops per call, S in --loop-streams,
          device-resident float32 noise at -40 dBFS (every capture runs receive_byte every hop and decodes nothing): wall time per call, the
          median of --reps calls after a warm-up that takes the captures past their first frames_to_read. The difference is the stage's cost
          to the loop.

usage: bench_resampler.py [--streams 1 64 1024] [--loop-streams 64 256] [--reps 20] [--loop-reps 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mercury_amd import Resampler, RxCapture, RxPhy  # noqa: E402

CARRIER = 1500.0
FIN = 44100


def stage(rx, S, reps):
    import torch
    rs = Resampler(rx, FIN, S=S)
    n_in = rs.max_in
    x = (0.01 * torch.randn((S, n_in), dtype=torch.float32, device="cuda"))
    out = torch.zeros((S, rs.max_out), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream()
    n_out = 0
    for _ in range(3):
        n_out = rs.process(x, out=out, stream=s.cuda_stream)
    s.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        rs.process(x, out=out, stream=s.cuda_stream)
    e1.record(s)
    e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    res = {"bench": "stage", "fin": FIN, "fout": 48000, "S": S, "n_in": n_in, "n_out": n_out, "tp": rs.tp, "tile": rs.tile, "reps": reps,
           "us_per_call": round(us, 2), "input_samples_per_s": round(S * n_in / (us * 1e-6)), "fma_per_s": round(S * n_out * rs.tp / (us * 1e-6))}
    rs.close()
    return res


def loop(rx, S, reps, hops=16):
    import torch
    cap48, cap44 = RxCapture(rx, S, CARRIER, max_hops=hops), RxCapture(rx, S, CARRIER, max_hops=hops)
    rs = Resampler(rx, FIN, S=S)
    P = cap48.P
    g = torch.Generator(device="cuda").manual_seed(7)
    x48 = 0.01 * torch.randn((S, hops * P), dtype=torch.float32, device="cuda", generator=g)
    x44 = 0.01 * torch.randn((S, rs.max_in), dtype=torch.float32, device="cuda", generator=g)
    warm = -(-(cap48.geometry.nsymb + cap48.geometry.preamble_nsymb) // hops) + 1

    def wall(fn):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(sorted(ts)[len(ts) // 2], 3), round(min(ts), 3)

    run_ms, run_min = wall(lambda: cap48.run(x48))
    hops_run = []
    rs_ms, rs_min = wall(lambda: hops_run.append(cap44.run_resampled(rs, x44)[1]))
    res = {"bench": "loop", "fin": FIN, "S": S, "hops_per_call": hops, "n_in": rs.max_in, "reps": reps, "run_ms": run_ms, "run_min_ms": run_min,
           "run_resampled_ms": rs_ms, "run_resampled_min_ms": rs_min, "hops_run": sorted(set(hops_run)),
           "stage_cost_ms": round(rs_ms - run_ms, 3), "stage_cost_share": round((rs_ms - run_ms) / run_ms, 4)}
    rs.close(), cap48.close(), cap44.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--loop-streams", type=int, nargs="*", default=[64, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=5)
    a = ap.parse_args()
    rx = RxPhy(8, max_batch=max(a.loop_streams + [8]))
    for S in a.streams:
        print(json.dumps(stage(rx, S, a.reps)), flush=True)
    for S in a.loop_streams:
        print(json.dumps(loop(rx, S, a.loop_reps)), flush=True)
    rx.close()


if __name__ == "__main__":
    main()

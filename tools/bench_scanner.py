#!/usr/bin/env python3
"""The band scanner's numbers (include/ext/mercury_scanner.h, profiles/scanner.md).

    python tools/bench_scanner.py --threshold [--lines 2048] [--seed 1]
    python tools/bench_scanner.py [--log2n 10,12] [--formats cs16,cf32,cf64] [--blocks 256] [--steps 20] [--warmup 3] [--rounds 3] [--window 0.3]

--threshold needs no GPU: the host twin over at least `--lines` lines of white Gaussian noise at the default N and A, the highest ratio
of a usable bin to the line's level; the default threshold is that ratio times 1.5, rounded up. Every call feeds a fresh scanner, whose
first block has half a block of silence in front of it: the first line of every call is left out.

The timing: per (N, format), `--blocks` blocks of device IQ in one mgpu_scan_process_dev call (device output), in `--rounds` rounds of at
least `--steps` calls and `--window` seconds after `--warmup`, a host clock around calls that end in a device synchronise; IQ samples
per second; the algorithmic bytes over that time (every sample is read twice and each block writes N doubles); the rate as a multiple of
real time at D = 64 (3.072 MHz); and, for scale, the channeliser's time per IQ sample at S = 1, D = 64 in the same run. The first call is
compared bit for bit with the twin. One JSON line per shape.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mercury_amd import (BandScanner, Channelizer, RxPhy, SCAN_REPORT_DTYPE, device_props, host_scan_process, scan_config)  # noqa: E402

SAMPLE_BYTES = {"cs16": 4, "cf32": 8, "cf64": 16}


def threshold(a):
    k = scan_config(4)
    N, A, H = 1 << k.log2n, k.blocks_per_line, (1 << k.log2n) // 2
    f = np.arange(N)
    usable = (f >= k.edge_bins) & (f <= N - 1 - k.edge_bins) & (np.abs(f - N // 2) > k.dc_bins)
    rng = np.random.default_rng(a.seed)
    per_call, worst, lines, false_runs = 33, 0.0, 0, 0
    while lines < a.lines:
        x = rng.standard_normal(per_call * A * H) + 1j * rng.standard_normal(per_call * A * H)
        L, rep = host_scan_process(x, 4)
        for line, r in zip(L[1:], rep[1:]):
            worst = max(worst, float(np.max(line[usable]) / r["level"]))
            false_runs += int(r["n_runs"])
        lines += per_call - 1
    print(json.dumps({"N": N, "blocks_per_line": A, "lines": lines, "usable_bins": int(usable.sum()), "highest_bin_to_level_ratio": round(worst, 4),
                      "times_1.5": round(worst * 1.5, 4), "default_threshold": math.ceil(worst * 1.5), "threshold_in_use": k.threshold,
                      "runs_reported_on_noise": false_runs}), flush=True)


def timed(rx, fn, a):
    for _ in range(a.warmup):
        fn()
    rx.lib.mgpu_synchronize(rx.h, None)
    steps = a.steps
    while True:                                                         # a window of at least --window seconds
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        rx.lib.mgpu_synchronize(rx.h, None)
        dt = time.perf_counter() - t0
        if dt >= a.window:
            return dt / steps * 1e3
        steps = int(steps * max(2.0, 1.2 * a.window / max(dt, 1e-6)))


def timing(a):
    import torch
    props = device_props(0)
    rx = RxPhy(8, max_batch=8)
    D = 64
    # the channeliser at S = 1 for scale: 16 hops of 1088 outputs
    n_chan = 16 * 1088 * D
    rng = np.random.default_rng(1)
    d_ciq = torch.from_numpy((rng.standard_normal(n_chan) + 1j * rng.standard_normal(n_chan)).astype(np.complex64)).cuda()
    ch = Channelizer(rx, D, [(0, 0, 1.0)], max_out=16 * 1088)
    d_cout = torch.zeros((1, 16 * 1088), dtype=torch.float64, device="cuda")
    for log2n in (int(v) for v in a.log2n.split(",")):
        N, H = 1 << log2n, (1 << log2n) // 2
        n_in = a.blocks * H
        for fmt in a.formats.split(","):
            rng = np.random.default_rng(log2n)
            if fmt == "cs16":
                x = rng.integers(-2 ** 15, 2 ** 15, (n_in, 2)).astype(np.int16)
            else:
                x = (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)).astype(np.complex64 if fmt == "cf32" else np.complex128)
            sc = BandScanner(rx, D, log2n=log2n, max_in=n_in)
            room = a.blocks // sc.A + 1
            d_x = torch.from_numpy(x).cuda()
            d_lines = torch.zeros((room, N), dtype=torch.float64, device="cuda")
            d_rep = torch.zeros((room, SCAN_REPORT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            n = sc.process_raw(d_x, d_lines, d_rep)
            rx.lib.mgpu_synchronize(rx.h, None)
            want_l, want_r = host_scan_process(x, D, log2n=log2n)
            same = bool(n == len(want_l) and d_lines[:n].cpu().numpy().tobytes() == want_l.tobytes()
                        and d_rep[:n].cpu().numpy().tobytes() == want_r.tobytes())
            scan_ms, chan_ms = [], []
            for _ in range(a.rounds):                                   # alternating: what shares the machine moves both alike
                scan_ms.append(timed(rx, lambda: sc.process_raw(d_x, d_lines, d_rep), a))
                chan_ms.append(timed(rx, lambda: ch.process(d_ciq, out=d_cout), a))
            sm, cm = min(scan_ms), min(chan_ms)
            rate = n_in / (sm * 1e-3)
            nbytes = 2 * n_in * SAMPLE_BYTES[fmt] + a.blocks * N * 8
            print(json.dumps({"N": N, "format": fmt, "blocks": a.blocks, "iq_samples": n_in, "blocks_per_line": sc.A, "ms_per_call": round(sm, 4),
                              "ms_rounds": [round(v, 4) for v in scan_ms], "iq_msamples_per_s": round(rate / 1e6, 1),
                              "algorithmic_gb_per_s": round(nbytes / (sm * 1e-3) / 1e9, 1), "times_real_time_at_D64": round(rate / (48000.0 * D), 1),
                              "ns_per_iq_sample": round(sm * 1e6 / n_in, 4), "channeliser_S1_D64_ns_per_iq_sample": round(cm * 1e6 / n_chan, 4),
                              "channeliser_ms_rounds": [round(v, 4) for v in chan_ms], "bit_identical_to_twin": same, "device": props["name"]}),
                  flush=True)
            sc.close()
    ch.close()
    rx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threshold", action="store_true")
    ap.add_argument("--lines", type=int, default=2048)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--log2n", default="10,12")
    ap.add_argument("--formats", default="cs16,cf32,cf64")
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    a = ap.parse_args()
    (threshold if a.threshold else timing)(a)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The carrier tuner's numbers (include/ext/mercury_tuner.h, profiles/tuner.md).

    python tools/bench_tuner.py --min-metric [--blocks 1024] [--seed 2027]
    python tools/bench_tuner.py --search-limit [--draws 160] [--seed 1]
    python tools/bench_tuner.py [--D 4,64] [--S 1,16] [--steps 20] [--warmup 3] [--rounds 3] [--window 0.3]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_tuner.py --calls 20 [--D 64] [--S 16]

--min-metric and --search-limit need no GPU. The first runs the host twin over `--blocks` blocks of white Gaussian CF64 noise at the
default configuration (D = 1) and prints the highest metric; the default min_metric is that times 1.5, rounded up to two decimals. The
second draws generated frames (tests/tuner_ref.py) at displacements over the whole +-1125 Hz that search = 24 reaches, D 1 and 4, both
sidebands, noise at -30 and -10 dB, and prints per 100 Hz of |displacement| how many draws the twin tuned to within 1 Hz.

The timing: per (D, S), one block of device CF32 IQ per mgpu_tune_process call at the defaults (J = 32: 4 D 8976 samples), in `--rounds`
rounds of at least `--steps` calls and `--window` seconds after `--warmup`, a host clock around blocking calls; the first call is
compared bit for bit with the twin. For scale the channeliser's time per output at the same D and S in the same run: stage 1 is the
same arithmetic at a quarter of the outputs. One JSON line per shape. --calls N runs N calls per shape and nothing else: under
rocprofv3's kernel trace the mean duration of each mgpu_tune_*_kernel is its per-kernel time.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mercury_amd import (Channelizer, RxPhy, Tuner, TUNE_DEFAULT_MIN_METRIC, device_props, host_tune_process, tune_reports,  # noqa: E402
                         tune_samples)


def min_metric(a):
    rng = np.random.default_rng(a.seed)
    n = tune_samples(1)
    seen = []
    for _ in range(a.blocks):
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        seen.append(float(host_tune_process(x, 1, [(0, 0, 1.0)], min_metric=1.0)[0]["metric"]))
    top = max(seen)
    print(json.dumps({"D": 1, "symbols": 32, "blocks": a.blocks, "highest_metric": round(top, 4), "mean_metric": round(float(np.mean(seen)), 4),
                      "times_1.5": round(top * 1.5, 4), "default_min_metric": math.ceil(top * 150.0) / 100.0,
                      "min_metric_in_use": TUNE_DEFAULT_MIN_METRIC}), flush=True)


def search_limit(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tuner_ref as ref
    rng = np.random.default_rng(a.seed)
    held, drawn = {}, {}
    for i in range(a.draws):
        D, sb, noise = (1, 4)[i % 2], (i // 2) % 2, (-30, -10)[(i // 4) % 2]
        half, d = 24000 * D, int(round(rng.uniform(-1125, 1125)))
        lo, hi = (-half + 1127, half - 2945 - 1126) if sb == 0 else (-half + 2945 + 1126, half - 1127)
        true = int(rng.integers(lo, hi + 1))
        x = ref.block(1000 + i, D, [(true, sb, 1.0)], noise_db=noise)
        r = tune_reports(host_tune_process(x, D, [(true + d, sb, 1.0)], search=24))[0]
        b = abs(d) // 100 * 100
        drawn[b] = drawn.get(b, 0) + 1
        held[b] = held.get(b, 0) + int(r["valid"] == 1 and abs(r["offset_hz"] - true) <= 1)
    for b in sorted(drawn):
        print(json.dumps({"displacement_hz_from": b, "draws": drawn[b], "tuned_within_1_hz": held[b]}), flush=True)


def timed(fn, a):
    for _ in range(a.warmup):
        fn()
    steps = a.steps
    while True:                                                         # a window of at least --window seconds; the calls block
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        dt = time.perf_counter() - t0
        if dt >= a.window:
            return dt / steps * 1e3
        steps = int(steps * max(2.0, 1.2 * a.window / max(dt, 1e-6)))


def timing(a):
    import torch
    props = device_props(0)
    rx = RxPhy(8, max_batch=8)
    for D in (int(v) for v in a.D.split(",")):
        for S in (int(v) for v in a.S.split(",")):
            rng = np.random.default_rng(D + S)
            step = max((48000 * D - 8000) // S, 1)
            plan = [(-24000 * D + 2000 + step * s, 0, 1.0) for s in range(S)]
            n_in = tune_samples(D)
            x = (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)).astype(np.complex64)
            d_x = torch.from_numpy(x).cuda()
            torch.cuda.synchronize()
            tn = Tuner(rx, D, plan)
            if a.calls:
                for _ in range(a.calls):
                    tn.process_raw(d_x)
                tn.close()
                continue
            got = tn.process_raw(d_x)
            same = bool(got.tobytes() == host_tune_process(x, D, plan).tobytes()) if D * S <= 64 else None
            n_out = 8 * 1088
            ch = Channelizer(rx, D, plan, max_out=n_out)
            d_out = torch.zeros((S, n_out), dtype=torch.float64, device="cuda")
            d_c = d_x[: n_out * D]
            tune_ms, chan_ms = [], []
            for _ in range(a.rounds):                                   # alternating: what shares the machine moves both alike
                tune_ms.append(timed(lambda: tn.process_raw(d_x), a))
                chan_ms.append(timed(lambda: (ch.process(d_c, out=d_out), rx.lib.mgpu_synchronize(rx.h, None)), a))
            tm, cm = min(tune_ms), min(chan_ms)
            outputs = S * 272 * 33
            print(json.dumps({"D": D, "S": S, "symbols": 32, "iq_samples": n_in, "ms_per_call": round(tm, 4),
                              "ms_rounds": [round(v, 4) for v in tune_ms], "us_per_channel": round(tm * 1e3 / S, 2),
                              "outputs_12k": outputs, "ns_per_12k_output_whole_call": round(tm * 1e6 / outputs, 2),
                              "channeliser_ns_per_output": round(cm * 1e6 / (S * n_out), 2),
                              "channeliser_ms_rounds": [round(v, 4) for v in chan_ms], "reports_bit_identical_to_twin": same,
                              "device": props["name"]}), flush=True)
            tn.close(), ch.close()
    rx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-metric", action="store_true")
    ap.add_argument("--search-limit", action="store_true")
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--draws", type=int, default=160)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--D", default="4,64")
    ap.add_argument("--S", default="1,16")
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    a = ap.parse_args()
    if a.seed is None:
        a.seed = 2027 if a.min_metric else 1
    (min_metric if a.min_metric else search_limit if a.search_limit else timing)(a)


if __name__ == "__main__":
    main()

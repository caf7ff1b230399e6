"""Continuous-capture receive (include/mercury_capture.h) against whole windows from the host (mgpu_receive_byte_batch_samples).

Mode 8, pageable host INT32 samples, S captures. Three workloads, alternated within one run:
  active   fresh noise, every capture's frames_to_read held at 0: each hop runs receive_byte on all S windows (nothing decodes, nothing skips);
           RxCapture.run(H) uploads S x H hops, the baseline uploads the same S windows per hop (the content the captures hold)
  mixed    noise with a frame in every eighth capture and staggered frames_to_read: captures skip hops after their decodes
Prints one JSON line per (S, workload, path, repeat) and a summary line. Kernel times of the feed and gather kernels come from a separate
    rocprofv3 --kernel-trace --stats -- python tools/bench_rx_capture.py --S 1024 --hops 4 --repeats 1 --no-baseline
run (profiles/rx_capture.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mercury_amd import RxCapture, RxPhy  # noqa: E402

CARRIER = 1500.0


def history(rng, S, n):
    return np.round(rng.standard_normal((S, n), dtype=np.float32) * np.float32(0.01 * 2 ** 31)).astype(np.int32)


def bench(rx, S, H, repeats, baseline, mixed, rng):
    P = rx.Nofdm * 4
    sp = rx.receive_buffer_samples()
    hist = history(rng, S, sp - 1 + H * P)
    last = np.zeros(S, np.int32)
    if mixed:                                   # the library's own transmit_byte frames in every eighth capture, anywhere in its history
        frame = np.asarray(rx.transmit_byte(np.zeros((1, rx.payload_stride), np.uint8), CARRIER)).reshape(-1)
        for s in range(0, S, 8):
            off = int(rng.integers(0, hist.shape[1] - frame.size))
            hist[s, off: off + frame.size] += np.round(frame * 2 ** 30).astype(np.int32)
    init = np.concatenate([hist[:, : sp - 1] / 2147483647.0, last[:, None] / 2147483647.0], axis=1)
    new = np.ascontiguousarray(hist[:, sp - 1:])
    out = []
    for rep in range(repeats):
        cap = RxCapture(rx, S, CARRIER, initial_windows=init, max_hops=H)
        for s in range(S):
            st = cap.state(s)
            st["frames_to_read"] = int(rng.integers(0, 29)) if mixed else 0
            cap.set_state(s, st)
        t = time.perf_counter()
        ev = cap.run(new)
        dt = time.perf_counter() - t
        cap.close()
        out.append(dict(S=S, hops=H, workload="mixed" if mixed else "active", path="capture", repeat=rep, seconds=dt,
                        capture_hops_per_s=S * H / dt, decoded=len(ev)))
        print(json.dumps(out[-1]), flush=True)
        if baseline and not mixed:
            dt = 0.0
            for h in range(H):
                win = np.concatenate([hist[:, (h + 1) * P: (h + 1) * P + sp - 1], last[:, None]], axis=1)
                t = time.perf_counter()
                rx.receive_byte(win, CARRIER)
                dt += time.perf_counter() - t
            out.append(dict(S=S, hops=H, workload="active", path="whole_windows_int32", repeat=rep, seconds=dt, capture_hops_per_s=S * H / dt))
            print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--hops", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--max-iters", type=int, default=50)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    rx = RxPhy(8, max_iters=args.max_iters, max_batch=max(args.S))
    res = []
    for S in args.S:
        res += bench(rx, S, args.hops, args.repeats, not args.no_baseline, False, rng)
        res += bench(rx, S, args.hops, args.repeats, False, True, rng)
    summary = {}
    for r in res:
        k = "%s/%s/S%d" % (r["workload"], r["path"], r["S"])
        summary.setdefault(k, []).append(round(r["capture_hops_per_s"]))
    print(json.dumps({"summary_capture_hops_per_s": summary}))
    rx.close()


if __name__ == "__main__":
    main()

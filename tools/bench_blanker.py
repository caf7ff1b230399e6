#!/usr/bin/env python3
"""What the impulse blanker (include/mercury_blanker.h) costs: the whole-call time of mgpu_rx_batch_dev on device buffers, stage off and
stage on, and the blanker kernel alone (mgpu_blank_dev), event-timed on one stream. The frames are the generator's (mgpu_txgen_dev) at the
mode's operating point; every 100th sample of every frame gets a 25 dB impulse unless --clean. A library without the stage (an older
build through MERCURY_GPU_LIB) measures the stage-off call only. Prints one JSON line.
usage: bench_blanker.py [--cfg 8] [--esn0 3.5] [--frames 4096] [--iters 20] [--warmup 5] [--clean]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mercury_amd import RxPhy  # noqa: E402
from mercury_amd.physical_layer import STATS_DTYPE  # noqa: E402

HBM_PEAK = 8.0e12                   # MI355X HBM3E bytes/s (spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", type=int, default=8)
    ap.add_argument("--esn0", type=float, default=3.5)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clean", action="store_true")
    a = ap.parse_args()
    import torch
    F = a.frames
    rx = RxPhy(a.cfg, max_batch=F)
    n = rx.frame_samples
    bb = torch.empty((F, n, 2), dtype=torch.float64, device="cuda")
    out = torch.empty_like(bb)
    payload = torch.empty((F, rx.payload_stride), dtype=torch.uint8, device="cuda")
    stats = torch.empty((F, STATS_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()
    rx.txgen_dev(7, 0, F, 10.0 ** (-a.esn0 / 20.0) / 2.0 ** 0.5, bb.data_ptr(), stream=s.cuda_stream)
    if not a.clean:
        amp = float(bb.pow(2).sum(dim=2).mean().sqrt()) * 10.0 ** (25.0 / 20.0)
        bb[:, 37::100, 0] += amp
    s.synchronize()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        s.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(a.iters):
            fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    span = lambda: rx.receive_dev(bb.data_ptr(), F, payload.data_ptr(), stats.data_ptr(), stream=s.cuda_stream)
    res = {"cfg": a.cfg, "esn0_db": a.esn0, "frames": F, "frame_samples": n, "impulses": not a.clean, "lib": "other" if os.environ.get("MERCURY_GPU_LIB") else "this"}
    res["span_off_ms"] = round(timed(span), 4)
    res["decoded_off"] = int((stats.cpu().numpy().view(STATS_DTYPE)["message_decoded"] != 0).sum())
    if hasattr(rx.lib, "mgpu_set_blanker"):
        alone = lambda: rx._ck(rx.lib.mgpu_blank_dev(rx.h, bb.data_ptr(), F, 0, out.data_ptr(), None, s.cuda_stream))
        res["blanker_ms"] = round(timed(alone), 4)
        traffic = 32.0 * n * F
        res["blanker_bytes_per_s"] = traffic / (res["blanker_ms"] * 1e-3)
        res["blanker_share_of_hbm_peak"] = round(res["blanker_bytes_per_s"] / HBM_PEAK, 4)
        rx.set_blanker("median")
        res["span_on_ms"] = round(timed(span), 4)
        res["decoded_on"] = int((stats.cpu().numpy().view(STATS_DTYPE)["message_decoded"] != 0).sum())
        rep = rx.blanker_report(0, F)
        res["blanked_per_frame_mean"] = float(rep["blanked"].mean())
        rx.set_blanker("off")
        res["span_off_again_ms"] = round(timed(span), 4)
    print(json.dumps(res))
    rx.close()


if __name__ == "__main__":
    main()

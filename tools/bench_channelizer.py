#!/usr/bin/env python3
"""Time the wideband channeliser (include/mercury_channelizer.h) at the shapes of profiles/channelizer.md.

Per (S, D): H hops of 1088 outputs per channel in one mgpu_chan_process_dev call (device CF32 input, device output), the mean of `--steps`
calls after `--warmup`; link-seconds of audio produced per second of wall time; the fraction of the device's fp64 vector peak as
8 T n_out S flops over the time, the peak being compute units x clock x 128 flops per clock (64 fp64 lanes, a fused multiply-add each);
and the host twin on the same input as the baseline a user has without the channeliser: timed on `--twin-channels` of the S channels and
scaled to S (the twin's work is the same for every channel). One JSON line per shape.

    python tools/bench_channelizer.py [--shapes 16x4,64x16,256x16] [--hops 16] [--steps 20] [--warmup 3] [--twin-channels 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mercury_amd import Channelizer, RxPhy, device_props, host_chan_process  # noqa: E402

P = 1088


def channels(S, D):
    """S USB channels on a 3 kHz raster from the band's lower edge up (closer where S of them do not fit the band at 3 kHz)"""
    lo, step = -24000 * D + 1000, min(3000, (48000 * D - 5000) // S)
    return [(lo + step * s, 0, 1.0) for s in range(S)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x4,64x16,256x16")
    ap.add_argument("--hops", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--twin-channels", type=int, default=1)
    ap.add_argument("--tp", type=int, default=320)
    a = ap.parse_args()
    import torch

    props = device_props(0)
    peak = props["compute_units"] * props["clock_khz"] * 1e3 * 128
    rx = RxPhy(8, max_batch=8)
    for shape in a.shapes.split(","):
        S, D = (int(v) for v in shape.split("x"))
        n_out = a.hops * P
        rng = np.random.default_rng(S + D)
        iq = (rng.standard_normal(n_out * D) + 1j * rng.standard_normal(n_out * D)).astype(np.complex64)
        chs = channels(S, D)
        ch = Channelizer(rx, D, chs, max_out=n_out)
        d_iq = torch.from_numpy(iq).cuda()
        d_out = torch.zeros((S, n_out), dtype=torch.float64, device="cuda")
        for _ in range(a.warmup):
            ch.process(d_iq, out=d_out)
        rx.lib.mgpu_synchronize(rx.h, None)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            ch.process(d_iq, out=d_out)
        rx.lib.mgpu_synchronize(rx.h, None)
        ms = (time.perf_counter() - t0) / a.steps * 1e3
        T = a.tp * D + 1
        flops = 8.0 * T * n_out * S
        nt = max(1, min(a.twin_channels, S))
        t0 = time.perf_counter()
        want = host_chan_process(D, chs[:nt], iq)
        twin_ms = (time.perf_counter() - t0) * 1e3 * S / nt
        ch.seek(0)
        got = ch.process(d_iq, out=d_out).cpu().numpy()
        same = bool(np.array_equal(got[:nt].view(np.uint64), want.view(np.uint64)))
        print(json.dumps({"S": S, "D": D, "hops": a.hops, "n_out": n_out, "taps": T, "ms_per_call": round(ms, 4),
                          "link_seconds_per_second": round(S * n_out / 48000.0 / (ms * 1e-3), 1),
                          "gflops": round(flops / (ms * 1e-3) / 1e9, 1), "fp64_peak_gflops": round(peak / 1e9, 1),
                          "fraction_of_fp64_peak": round(flops / (ms * 1e-3) / peak, 4),
                          "host_twin_ms_scaled_to_S": round(twin_ms, 1), "twin_channels_timed": nt, "speedup_over_twin": round(twin_ms / ms, 1),
                          "bit_identical_to_twin": same, "device": props["name"]}), flush=True)
        ch.close()
    rx.close()


if __name__ == "__main__":
    main()

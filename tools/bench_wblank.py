#!/usr/bin/env python3
"""The wideband impulse blanker's timing (include/ext/mercury_wideband_blanker.h, profiles/wideband_blanker.md).

    python tools/bench_wblank.py [--shapes 4:16,64:16] [--formats cf32,cf64] [--steps 20] [--warmup 3] [--rounds 3] [--window 0.3]

Per (D, hops) and format: `hops` hops of 1088 audio samples, hops * 1088 * D IQ samples of noise with clicks at 100 Hz on the device, in
one mgpu_wblank_process_dev call (device output, device reports) at the default block, threshold and guard, next to one
mgpu_chan_process_dev call of a channeliser of S = 1 on the same stream in the same run, in `--rounds` alternating rounds of at least
`--steps` calls and `--window` seconds after `--warmup`, a host clock around calls that end in a device synchronise. The blanker's time
per call, its algorithmic bytes over that time (every sample is read twice and written once), and its share of the channeliser's time.
The first call is compared byte for byte with the twin. One JSON line per shape.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mercury_amd import (Channelizer, RxPhy, WBLANK_REPORT_DTYPE, WidebandBlanker, device_props, host_wblank_process)  # noqa: E402

SAMPLE_BYTES = {"cs16": 4, "cf32": 8, "cf64": 16}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4:16,64:16")
    ap.add_argument("--formats", default="cf32,cf64")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    a = ap.parse_args()
    import torch
    props = device_props(0)
    rx = RxPhy(8, max_batch=8)
    for D, hops in ((int(v) for v in shape.split(":")) for shape in a.shapes.split(",")):
        n_in = hops * 1088 * D
        for fmt in a.formats.split(","):
            rng = np.random.default_rng(D)
            x = rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)
            x[240 * D:: 480 * D] += 300.0 * np.exp(2j * np.pi * rng.random(x[240 * D:: 480 * D].size))
            x = (np.stack([x.real, x.imag], 1) * 64).astype(np.int16) if fmt == "cs16" else x.astype(np.complex64 if fmt == "cf32" else np.complex128)
            wb = WidebandBlanker(rx, D, fmt, max_in=n_in)
            ch = Channelizer(rx, D, [(0, 0, 1.0)], max_out=hops * 1088)
            d_x = torch.from_numpy(x).cuda()
            d_out = torch.zeros_like(d_x)
            d_rep = torch.zeros((n_in // wb.B, WBLANK_REPORT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
            d_audio = torch.zeros((1, hops * 1088), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            n = wb.process_raw(d_x, d_out, d_rep)
            rx.lib.mgpu_synchronize(rx.h, None)
            want_o, want_r = host_wblank_process(x, D)
            same = bool(n == len(want_r) and d_out.cpu().numpy().tobytes() == want_o.tobytes() and d_rep.cpu().numpy().tobytes() == want_r.tobytes())
            blank_ms, chan_ms = [], []
            for _ in range(a.rounds):                                   # alternating: what shares the machine moves both alike
                blank_ms.append(timed(rx, lambda: wb.process_raw(d_x, d_out, d_rep), a))
                chan_ms.append(timed(rx, lambda: ch.process(d_out, out=d_audio), a))
            bm, cm = min(blank_ms), min(chan_ms)
            nbytes = 3 * n_in * SAMPLE_BYTES[fmt]
            print(json.dumps({"D": D, "hops": hops, "format": fmt, "block": wb.B, "iq_samples": n_in, "blocks": n_in // wb.B,
                              "clicks_blanked": int(want_r["exceeding"].sum()), "samples_zeroed": int(want_r["blanked"].sum()),
                              "blanker_ms_per_call": round(bm, 4), "blanker_ms_rounds": [round(v, 4) for v in blank_ms],
                              "channeliser_S1_ms_per_call": round(cm, 4), "channeliser_ms_rounds": [round(v, 4) for v in chan_ms],
                              "blanker_share_of_channeliser": round(bm / cm, 4), "algorithmic_gb_per_s": round(nbytes / (bm * 1e-3) / 1e9, 1),
                              "times_real_time": round(n_in / (bm * 1e-3) / (48000.0 * D), 1), "byte_identical_to_twin": same,
                              "device": props["name"]}), flush=True)
            wb.close(), ch.close()
    rx.close()


if __name__ == "__main__":
    main()

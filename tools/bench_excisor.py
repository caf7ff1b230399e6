#!/usr/bin/env python3
"""What the carrier excisor (include/ext/mercury_excisor.h) costs: the wall time of mgpu_receive_byte_batch on W capture windows of the
library's own passband self-simulation at a clean point, device-resident doubles and INT16 samples from host memory, stage off and stage
on; with the stage on also on the same windows plus a carrier as strong as the frame at the carrier + 317 Hz; and the stage alone
(mgpu_excise_dev), event-timed on one stream. A library without the stage (an older tree) measures the stage-off calls only; the digest of
the stage-off results lets two trees be compared. --stage-only runs nothing but the stage alone (for a kernel trace). Prints one JSON line.
usage: bench_excisor.py [--cfg 8] [--windows 1024] [--reps 7] [--stage-only]"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mercury_amd import RxPhy  # noqa: E402

CARRIER = 1500.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", type=int, default=8)
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--stage-only", action="store_true")
    a = ap.parse_args()
    import torch
    W = a.windows
    rx = RxPhy(a.cfg, max_batch=W)
    _, wins, _ = rx.passband_test_esn0([30.0], W, CARRIER, seed=0x4D455243, want_windows=True)
    # The self-simulation's level puts a frame's symbols 0.4 dB above the reference's absolute energy gate (mean |x|^2 of 0.001 at the delay):
    # a window that loses 4 of its 50 carriers to the excisor falls under it and is never decoded (profiles/excisor.md). 2 dB of gain, the
    # same on every window of every run, keep the toned windows comparable; nothing reaches the integer format's full scale.
    wins = 1.25 * wins
    assert np.max(np.abs(wins)) < 1.0
    n = wins.shape[1]
    loud = np.sort(wins[0] ** 2)[-n // 3:].mean()                # the frame fills a third of its window
    toned = wins + np.sqrt(2.0 * loud) * np.cos(2 * np.pi * (CARRIER + 317.0) * np.arange(n) / 48000.0 + 0.2)      # doubles only: never clipped
    has = hasattr(rx.lib, "mgpu_set_excisor")

    def wall(fn):
        fn(); fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(sorted(ts)[len(ts) // 2], 3), round(min(ts), 3), r

    def digest(r):
        return hashlib.sha256(b"".join(r["stats"][k].tobytes() for k in r["stats"].dtype.names) + r["payload"].tobytes()).hexdigest()[:16]

    def decoded(r):
        return int((r["stats"]["message_decoded"] == 1).sum())

    res = {"cfg": a.cfg, "windows": W, "window_samples": n, "stage": has}
    d_clean, d_toned = torch.from_numpy(wins).cuda(), torch.from_numpy(toned).cuda()
    if not a.stage_only:
        q = np.rint(wins * 32767.0).astype(np.int16)
        dev = lambda d: (lambda: rx.receive_byte_dev(d.data_ptr(), W, CARRIER))
        res["dev_off_ms"], res["dev_off_min_ms"], r = wall(dev(d_clean))
        res["dev_off_digest"], res["dev_off_decoded"] = digest(r), decoded(r)
        res["int16_off_ms"], res["int16_off_min_ms"], r = wall(lambda: rx.receive_byte(q, CARRIER))
        res["int16_off_digest"] = digest(r)
        if has:
            res["dev_off_toned_decoded"] = decoded(rx.receive_byte_dev(d_toned.data_ptr(), W, CARRIER))
            rx.set_excisor("welch")
            res["dev_on_clean_ms"], res["dev_on_clean_min_ms"], r = wall(dev(d_clean))
            res["dev_on_clean_same_as_off"] = digest(r) == res["dev_off_digest"]
            res["int16_on_clean_ms"], res["int16_on_clean_min_ms"], r = wall(lambda: rx.receive_byte(q, CARRIER))
            res["dev_on_toned_ms"], res["dev_on_toned_min_ms"], r = wall(dev(d_toned))
            res["dev_on_toned_decoded"] = decoded(r)
            res["toned_bins_removed_mean"] = float(rx.excisor_report(0, W)["excised"].mean())
            rx.set_excisor("off")
            res["dev_off_again_ms"], res["dev_off_again_min_ms"], _ = wall(dev(d_clean))
    if has:
        out = torch.empty_like(d_clean)
        s = torch.cuda.current_stream()
        for name, d in (("clean", d_clean), ("toned", d_toned)):
            run = lambda: rx._ck(rx.lib.mgpu_excise_dev(rx.h, d.data_ptr(), W, n, CARRIER, out.data_ptr(), None, s.cuda_stream))
            for _ in range(3):
                run()
            s.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.reps):
                run()
            e1.record(s)
            e1.synchronize()
            res["stage_alone_%s_ms" % name] = round(e0.elapsed_time(e1) / a.reps, 4)
    print(json.dumps(res))
    rx.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Find the stations, then receive them: S links send through transmit_byte -> Synthesizer -> AWGN; the BandScanner looks at the wideband
IQ and reports the occupied runs; BandScanner.plan turns them into a channel plan; the Channelizer is built from the FOUND plan, not from
the one the links were placed with, and RxCapture.run_wideband receives through it.

    python tools/band_scan.py [--links 3] [--D 4] [--raster 9000] [--frames 2] [--noise-db -40] [--mode 8] [--seed 1] [--log2n 12]
                              [--blocks-per-line 16] [--tune]

Every link is USB (the scanner finds a band, not its sideband: the plan is made for the sideband the user names). One JSON line per
link: the true offset, the found offset (of the found channel nearest to it), their difference, the run's width in bins, and the frames
sent, delivered through the found plan and, as the control, delivered from the same IQ through the plan the links were placed with. Whether receive_byte tolerates the planning error of up to a bin is what this tool reports; nothing is asserted. Then a
summary line. A link is silent between its frames and a line in such a pause does not show it (the detection is static per line): the
plan is made from the line with the most power.

--tune adds a third pass: the found plan goes through the Tuner on the block of IQ that begins at the judged line's first sample (the
last block that fits, should the line lie too near the end), and the links are received once more through the tuned plan. Every link's
line gains tuned_offset_hz, tuned_error_hz, metric and delivered_through_the_tuned_plan. Without --tune the output is unchanged."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mercury_amd import BandScanner, Channelizer, RxCapture, RxPhy, Synthesizer, Tuner  # noqa: E402

P = 1088
CARRIER = 1471.875
HOPS_PER_CALL = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=3)
    ap.add_argument("--D", type=int, default=4)
    ap.add_argument("--raster", type=int, default=9000)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--noise-db", type=float, default=-40.0)
    ap.add_argument("--mode", type=int, default=8)
    ap.add_argument("--max-iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--log2n", type=int, default=12)
    ap.add_argument("--blocks-per-line", type=int, default=16)
    ap.add_argument("--tune", action="store_true")
    a = ap.parse_args()
    import torch
    S, D = a.links, a.D
    lo = -24000 * D + 7000
    step = min(a.raster, (48000 * D - 14000) // max(S, 1))
    offs = [lo + step * s + (37 * s) % 101 for s in range(S)]           # off any bin raster
    plan = [(o, 0, 1.0) for o in offs]
    rx = RxPhy(a.mode, max_iters=a.max_iters, max_batch=max(8, S))
    fsz = rx.transmit_frame_samples()
    fh = -(-fsz // P)
    rng = np.random.default_rng(a.seed)
    payloads = rng.integers(0, 256, (a.frames, S, rx.payload_bytes)).astype(np.uint8)
    starts = [[(5 + f * (fh + 3)) * P + int(rng.integers(1, P)) for s in range(S)] for f in range(a.frames)]
    H = -(-(max(starts[-1]) + fsz + 320 + 6 * P) // (P * HOPS_PER_CALL)) * HOPS_PER_CALL
    n = H * P
    d_audio = torch.zeros((S, n), dtype=torch.float64, device="cuda")
    d_frames = torch.zeros((S, fsz), dtype=torch.float64, device="cuda")
    for f in range(a.frames):
        d_pl = torch.from_numpy(payloads[f]).cuda()
        torch.cuda.synchronize()                                        # the library works on its own stream
        rx.transmit_byte_dev(d_pl.data_ptr(), rx.payload_bytes, S, d_frames.data_ptr(), CARRIER)
        rx.lib.mgpu_synchronize(rx.h, None)
        for s in range(S):
            d_audio[s, starts[f][s]: starts[f][s] + fsz] = d_frames[s]
    # 1. the band: synthesiser and noise, kept whole for the second pass
    sy = Synthesizer(rx, D, plan)
    step_a = HOPS_PER_CALL * P
    d_iq = torch.zeros(n * D, dtype=torch.complex64, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(a.seed)
    amp = 10 ** (a.noise_db / 20.0)
    torch.cuda.synchronize()
    for c in range(H // HOPS_PER_CALL):
        sy.process(d_audio[:, c * step_a: (c + 1) * step_a], fmt="cf32", out=d_iq[c * step_a * D: (c + 1) * step_a * D])
    rx.lib.mgpu_synchronize(rx.h, None)
    d_iq += amp * torch.view_as_complex(torch.randn((n * D, 2), dtype=torch.float32, device="cuda", generator=gen))
    torch.cuda.synchronize()
    # 2. the scan: every whole line of the signal. A link is silent between its frames, so the line judged is the one with the most power
    sc = BandScanner(rx, D, log2n=a.log2n, blocks_per_line=a.blocks_per_line)
    per_line = sc.H * sc.A
    per_call = max(sc.max_in // per_line, 1) * per_line
    whole = (n * D) // per_line * per_line
    lines, reports = [], []
    for at in range(0, whole, per_call):
        got = sc.process(d_iq[at: min(at + per_call, whole)])
        lines.append(got[0])
        reports += got[1]
    lines = np.concatenate(lines)
    best = int(np.argmax(lines.sum(axis=1)))
    report = reports[best]
    found = sc.plan(report, sideband=0)
    # 3. receive through the found plan: a found channel per link, the nearest; a link nothing was found for gets no channel
    nearest = []
    for o in offs:
        cand = sorted(found, key=lambda ch: abs(ch[0] - o))
        nearest.append(cand[0] if cand and abs(cand[0][0] - o) < 1500 else None)
    def receive(channels, links):
        """frames delivered per link through a channeliser made from `channels`, channel i being link links[i]'s"""
        got = [0] * S
        if not channels:
            return got
        ch = Channelizer(rx, D, channels)
        cap = RxCapture(rx, len(channels), CARRIER, max_hops=HOPS_PER_CALL)
        events = []
        for c in range(H // HOPS_PER_CALL):
            events += [(e[0], e[3].tobytes()) for e in cap.run_wideband(ch, d_iq[c * step_a * D: (c + 1) * step_a * D])]
        for row, s in enumerate(links):
            sent = [payloads[f, s].tobytes() for f in range(a.frames)]
            got[s] = sum(1 for pl in sent if any(e[0] == row and e[1] == pl for e in events))
        ch.close(), cap.close()
        return got

    links = [s for s in range(S) if nearest[s] is not None]
    delivered = receive([nearest[s] for s in links], links)
    control = receive(plan, list(range(S)))                             # the same band through the plan the links were placed with
    tuned, tuned_reports, through_tuned = {}, {}, [0] * S
    if a.tune and links:
        tn = Tuner(rx, D, [nearest[s] for s in links])
        at = min(best * per_line, n * D - tn.samples)
        reports_t = tn.process(d_iq[at: at + tn.samples])
        for s, ch, r in zip(links, tn.plan(reports_t), reports_t):
            tuned[s], tuned_reports[s] = ch, r
        tn.close()
        through_tuned = receive([tuned[s] for s in links], links)
    widths = {}                                                         # a planned channel's offset -> its run's bins
    for r in report["runs"]:
        for ch in sc.plan({"runs": [r]}, sideband=0):
            widths[ch[0]] = r["count"]
    for s in range(S):
        row = {"link": s, "true_offset_hz": offs[s], "found_offset_hz": nearest[s][0] if nearest[s] else None,
               "error_hz": nearest[s][0] - offs[s] if nearest[s] else None,
               "run_bins": widths.get(nearest[s][0]) if nearest[s] else None, "sent": a.frames, "delivered": delivered[s],
               "delivered_through_the_true_plan": control[s]}
        if a.tune:
            row.update({"tuned_offset_hz": tuned[s][0] if s in tuned else None,
                        "tuned_error_hz": tuned[s][0] - offs[s] if s in tuned else None,
                        "metric": tuned_reports[s]["metric"] if s in tuned else None,
                        "delivered_through_the_tuned_plan": through_tuned[s]})
        print(json.dumps(row), flush=True)
    summary = {"links": S, "D": D, "mode": a.mode, "noise_db": a.noise_db, "N": sc.N, "blocks_per_line": sc.A,
               "bin_hz": 48000.0 * D / sc.N, "lines": len(reports), "line_judged": best, "runs_in_it": report["n_runs"],
               "channels_planned": len(found), "sent": S * a.frames, "delivered": sum(delivered),
               "delivered_through_the_true_plan": sum(control)}
    if a.tune:
        summary["delivered_through_the_tuned_plan"] = sum(through_tuned)
    print(json.dumps(summary), flush=True)
    for o in (sy, sc, rx):
        o.close()


if __name__ == "__main__":
    main()

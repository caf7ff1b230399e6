#!/usr/bin/env python3
"""An occupied band on the device: S links send through transmit_byte -> Synthesizer -> optional AWGN -> Channelizer ->
RxCapture.run_wideband, and what each link sent and what arrived is printed. The adjacent-channel experiment: links on a 3 kHz raster
with gains of their own, USB next to LSB.

    python tools/band_loopback.py [--links 3] [--D 4] [--raster 3000 | --offsets HZ,HZ,..] [--gains-db 0,30,0] [--sidebands u,u,l] [--frames 4]
                                  [--noise-db -40] [--fmt cf32] [--mode 8] [--seed 1] [--impulses 100:60] [--wblank [thr=38,guard=4,block=256]]
                                  [--imbalance 0.83,5[,0.01,-0.01]] [--iqfix [memory=1024,block=4096]]
    python tools/band_loopback.py --time [--shapes 16x4,256x16] [--hops 16] [--steps 20] [--warmup 3] [--window 0.3]

Every link sends `--frames` frames, frame f of link s starting at hop 5 + f * (frame hops + 3) plus an offset of its own, in silence.
The audio never leaves the device. --noise-db adds white noise of that level (dB relative to full scale 1.0, per IQ component) to the IQ.
One JSON line per link, then a summary line. "delivered_without_the_band" is what the same receive loop delivers on the link's own audio
delayed by tp samples, with no neighbour and no filter: the receive loop loses some noise-free frames by their position on its hop grid
(tests/test_gpu_channelizer.py), and only what is delivered there and not through the band is the band's doing.

--impulses RATE_HZ:DB adds one-sample clicks of random phase, RATE_HZ of them a second, DB above the strongest link's rms in the IQ (measured
on that link's first frame synthesised alone), behind the noise. The band is then run click-free and clicked, and with --wblank a third
time clicked with a WidebandBlanker (ext/mercury_wideband_blanker.h; thr, guard, block: its threshold, guard and block, each optional) in
front of the channeliser; every link's line counts the frames delivered in each run ("delivered" is the click-free run's).

--imbalance GAIN_DB,PHASE_DEG[,DC_RE,DC_IM] impairs the synthesised IQ (behind the noise and the clicks) in numpy as a quadrature front end
does: I' = I + DC_RE, Q' = g (Q cos(phi) + I sin(phi)) + DC_IM with g = 10^(GAIN_DB / 20); 0.83,5 is gain 1.1 and 5 degrees, an image 23.8 dB
down. The band is then run once more, impaired (with the clicks and the blanker where those are asked for), and with --iqfix a further time
with an IqCorrector (ext/mercury_iq_corrector.h; memory, block: each optional; the default block is the greatest of 4096, 2048 and 1024
that divides a call) ahead of the blanker; every link's line counts the frames of those runs too, and the summary carries the corrector's
last report.

--time: mgpu_synth_process_dev against mgpu_chan_process_dev at the same S, D and signal length in one run (profiles/synthesizer.md):
per shape, `--hops` hops of 1088 samples per channel, CF32 IQ on the device, both alternating in `--rounds` rounds of at least `--steps`
calls and `--window` seconds after `--warmup`, a host clock around calls that end in a device synchronise; one JSON line per shape.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mercury_amd import (Channelizer, IQC_REPORT_DTYPE, IqCorrector, RxCapture, RxPhy, Synthesizer, WidebandBlanker, device_props,  # noqa: E402
                         iqc_image_db, iqc_reports)

P = 1088
CARRIER = 1471.875
HOPS_PER_CALL = 16


def raster(S, D, step=3000):
    """S channel offsets on a raster of `step` Hz from the band's lower edge up (closer where S of them do not fit the band)"""
    lo = -24000 * D + 3500
    step = min(step, (48000 * D - 7000) // max(S, 1))
    return [lo + step * s for s in range(S)]


def loopback(a):
    import torch
    S, D = a.links, a.D
    gains_db = [float(v) for v in a.gains_db.split(",")] if a.gains_db else [0.0]
    gains = [10 ** (gains_db[s % len(gains_db)] / 20.0) for s in range(S)]
    sbs = [1 if v.strip().lower().startswith("l") else 0 for v in a.sidebands.split(",")] if a.sidebands else [0]
    sbs = [sbs[s % len(sbs)] for s in range(S)]
    offs = raster(S, D, a.raster)
    offs = [o + 2944 if sb else o for o, sb in zip(offs, sbs)]           # an LSB channel's band lies below its dial frequency
    if a.offsets:                                                       # dial offsets of the caller's in place of the raster
        offs = [int(v) for v in a.offsets.split(",")]
        assert len(offs) == S, "--offsets wants one offset per link"
    plan = [(offs[s], sbs[s], gains[s]) for s in range(S)]
    rx = RxPhy(a.mode, max_iters=a.max_iters, max_batch=max(8, S))
    fsz = rx.transmit_frame_samples()
    fh = -(-fsz // P)
    rng = np.random.default_rng(a.seed)
    payloads = rng.integers(0, 256, (a.frames, S, rx.payload_bytes)).astype(np.uint8)
    starts = [[(5 + f * (fh + 3)) * P + int(rng.integers(1, P)) for s in range(S)] for f in range(a.frames)]        # never on the hop grid
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
    sy = Synthesizer(rx, D, plan)
    direct = RxCapture(rx, S, CARRIER, max_hops=HOPS_PER_CALL)          # the same loop on the audio itself, delayed as the band delays it
    d_delayed = torch.zeros_like(d_audio)
    d_delayed[:, sy.tp:] = d_audio[:, : n - sy.tp]
    step = HOPS_PER_CALL * P
    cdt = {"cf32": torch.complex64, "cf64": torch.complex128}[a.fmt]
    d_iq = torch.zeros(step * D, dtype=cdt, device="cuda")
    amp = 10 ** (a.noise_db / 20.0) if a.noise_db is not None else 0.0
    period, click_amp, wblank = 0, 0.0, None
    if a.impulses:
        rate, db = (float(v) for v in a.impulses.split(":"))
        period = int(48000.0 * D / rate)
        strongest = int(np.argmax(gains))
        alone_sy = Synthesizer(rx, D, [plan[strongest]])
        power, first = 0.0, starts[0][strongest]
        d_one = torch.zeros((1, n), dtype=torch.float64, device="cuda")
        d_one[0, first: first + fsz] = d_audio[strongest, first: first + fsz]
        torch.cuda.synchronize()
        for c in range(first // step, (first + fsz + sy.tp) // step + 1):      # the strongest link's first frame, synthesised alone
            alone_sy.process(d_one[:, c * step: (c + 1) * step], fmt=a.fmt, out=d_iq)
            rx.lib.mgpu_synchronize(rx.h, None)
            power += float((d_iq.real ** 2 + d_iq.imag ** 2).sum())
        alone_sy.close()
        click_amp = float(np.sqrt(power / (fsz * D))) * 10 ** (db / 20.0)
        if a.wblank is not None:
            names = {"thr": "threshold", "guard": "guard", "block": "block"}
            wblank = {names[k]: float(v) if k == "thr" else int(v) for k, v in (kv.split("=") for kv in a.wblank.split(",") if kv)}

    front_end, iqfix, last_report = None, None, []
    if a.imbalance:
        v = [float(t) for t in a.imbalance.split(",")]
        front_end = (10 ** (v[0] / 20.0), np.radians(v[1]), v[2] if len(v) > 2 else 0.0, v[3] if len(v) > 3 else 0.0)
        if a.iqfix is not None:
            iqfix = {k: int(t) for k, t in (kv.split("=") for kv in a.iqfix.split(",") if kv)}
            iqfix.setdefault("block", 4096 if D % 4 == 0 else 2048 if D % 2 == 0 else 1024)

    def run(clicks, blank, want_alone=False, impaired=False, fix=None):
        """the whole signal through the band -> (events, what the loop delivers on the audio alone)"""
        gen = torch.Generator(device="cuda")
        gen.manual_seed(a.seed)
        sy.seek(0)
        ch = Channelizer(rx, D, [(o, sb, 1.0 / g) for o, sb, g in plan])
        cap = RxCapture(rx, S, CARRIER, max_hops=HOPS_PER_CALL)
        wb = WidebandBlanker(rx, D, a.fmt, **blank) if blank is not None else None
        qc = IqCorrector(rx, D, a.fmt, **fix) if fix is not None else None
        d_out, d_fixed = torch.zeros_like(d_iq), torch.zeros_like(d_iq)
        d_rep = torch.zeros((step * D // qc.B, IQC_REPORT_DTYPE.itemsize), dtype=torch.uint8, device="cuda") if qc else None
        events, alone = [], []
        torch.cuda.synchronize()
        for c in range(H // HOPS_PER_CALL):
            sy.process(d_audio[:, c * step: (c + 1) * step], fmt=a.fmt, out=d_iq)
            if amp or clicks:
                rx.lib.mgpu_synchronize(rx.h, None)
                if amp:
                    d_iq.add_(amp * torch.view_as_complex(torch.randn((step * D, 2), dtype=d_iq.real.dtype, device="cuda", generator=gen)))
                if clicks:
                    at = torch.arange((period // 2 - c * step * D) % period, step * D, period, device="cuda")
                    phase = 2.0 * np.pi * torch.rand(at.numel(), dtype=d_iq.real.dtype, device="cuda", generator=gen)
                    d_iq[at] += click_amp * torch.complex(torch.cos(phase), torch.sin(phase))
                torch.cuda.synchronize()
            if impaired:
                rx.lib.mgpu_synchronize(rx.h, None)
                x = d_iq.cpu().numpy()
                g, phi, dc_re, dc_im = front_end
                x = ((x.real + dc_re) + 1j * (g * (x.imag * np.cos(phi) + x.real * np.sin(phi)) + dc_im)).astype(x.dtype)
                d_iq.copy_(torch.from_numpy(x))
                torch.cuda.synchronize()
            d_in = d_iq
            if qc:
                qc.process_raw(d_in, d_fixed, d_rep)                    # the context's stream, as the blanker's and run_wideband's
                d_in = d_fixed
            if wb:
                wb.process_raw(d_in, d_out)                             # the context's stream, as run_wideband's
                d_in = d_out
            events += [(e[0], e[1] + c * HOPS_PER_CALL, int(e[2]["crc"]), e[3].tobytes()) for e in cap.run_wideband(ch, d_in)]
            if want_alone:
                alone += [(e[0], e[3].tobytes()) for e in direct.run(d_delayed[:, c * step: (c + 1) * step].contiguous())]
        if qc:
            rx.lib.mgpu_synchronize(rx.h, None)
            last_report[:] = iqc_reports(d_rep.cpu().numpy().reshape(-1).view(IQC_REPORT_DTYPE))[-1:]
        for o in (ch, cap, wb, qc):
            if o:
                o.close()
        return events, alone

    def frames_delivered(ev, s):
        return sum(1 for f in range(a.frames) if any(e[0] == s and e[3] == payloads[f, s].tobytes() for e in ev))

    events, alone = run(False, None, True)
    clicked = run(True, None)[0] if period else None
    blanked = run(True, wblank)[0] if period and wblank is not None else None
    fullest = wblank if period and wblank is not None else None
    impaired = run(bool(period), fullest, impaired=True)[0] if front_end else None
    corrected = run(bool(period), fullest, impaired=True, fix=iqfix)[0] if front_end and iqfix is not None else None
    clamped = sy.status().clamped
    total, totals = 0, {"clicked": 0, "blanked": 0, "impaired": 0, "corrected": 0}
    for s in range(S):
        sent = [payloads[f, s].tobytes() for f in range(a.frames)]
        mine = [e for e in events if e[0] == s]
        delivered = frames_delivered(events, s)
        without = sum(1 for pl in sent if any(e[0] == s and e[1] == pl for e in alone))
        foreign = sum(1 for e in mine if any(e[3] == payloads[f, t].tobytes() for f in range(a.frames) for t in range(S) if t != s))
        total += delivered
        line = {"link": s, "offset_hz": offs[s], "sideband": "lsb" if sbs[s] else "usb", "gain_db": gains_db[s % len(gains_db)],
                "sent": a.frames, "delivered": delivered, "delivered_without_the_band": without, "events": len(mine),
                "foreign_payloads": foreign}
        for name, ev in (("clicked", clicked), ("blanked", blanked), ("impaired", impaired), ("corrected", corrected)):
            if ev is not None:
                line["delivered_" + name] = frames_delivered(ev, s)
                totals[name] += line["delivered_" + name]
        print(json.dumps(line), flush=True)
    summary = {"links": S, "D": D, "mode": a.mode, "hops": H, "fmt": a.fmt, "noise_db": a.noise_db, "sent": S * a.frames,
               "delivered": total, "cs16_clamped": int(clamped)}
    if clicked is not None:
        summary.update({"impulses": a.impulses, "click_amplitude": click_amp, "delivered_clicked": totals["clicked"]})
    if blanked is not None:
        summary.update({"wblank": wblank, "delivered_blanked": totals["blanked"]})
    if impaired is not None:
        g, phi = front_end[0], front_end[1]
        summary.update({"imbalance": a.imbalance, "image_db": round(iqc_image_db(g * np.sin(phi), 1.0 / (g * np.cos(phi))), 2),
                        "delivered_impaired": totals["impaired"]})
    if corrected is not None:
        summary.update({"iqfix": iqfix, "delivered_corrected": totals["corrected"], "iqfix_last_report": last_report[0]})
    print(json.dumps(summary), flush=True)
    for o in (sy, direct, rx):
        o.close()


def timing(a):
    import torch
    props = device_props(0)
    peak = props["compute_units"] * props["clock_khz"] * 1e3 * 128
    rx = RxPhy(8, max_batch=8)
    for shape in a.shapes.split(","):
        S, D = (int(v) for v in shape.split("x"))
        n = a.hops * P
        rng = np.random.default_rng(S + D)
        plan = [(o, 0, 1.0) for o in raster(S, D)]
        tp = 320
        sy = Synthesizer(rx, D, plan, max_in=n)
        ch = Channelizer(rx, D, plan, max_out=n)
        d_audio = torch.from_numpy(rng.standard_normal((S, n)) * 0.1).cuda()
        d_iq = torch.zeros(n * D, dtype=torch.complex64, device="cuda")
        d_back = torch.zeros((S, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def run(fn):
            for _ in range(a.warmup):
                fn()
            rx.lib.mgpu_synchronize(rx.h, None)
            steps = a.steps
            while True:                                                 # a window of at least --window seconds
                t0 = time.perf_counter()
                for _ in range(steps):
                    fn()
                rx.lib.mgpu_synchronize(rx.h, None)
                dt = time.perf_counter() - t0
                if dt >= a.window:
                    return dt / steps * 1e3
                steps = int(steps * max(2.0, 1.2 * a.window / max(dt, 1e-6)))

        synth_ms, chan_ms = [], []
        for _ in range(a.rounds):                                      # alternating: what shares the machine moves both alike
            synth_ms.append(run(lambda: sy.process(d_audio, fmt="cf32", out=d_iq)))
            chan_ms.append(run(lambda: ch.process(d_iq, out=d_back)))
        sm, cm = min(synth_ms), min(chan_ms)
        sflops, cflops = 4.0 * (tp + 1) * S * n * D, 8.0 * (tp * D + 1) * n * S
        print(json.dumps({"S": S, "D": D, "hops": a.hops, "audio_samples": n, "iq_samples": n * D, "tp": tp,
                          "synth_ms_per_call": round(sm, 4), "chan_ms_per_call": round(cm, 4),
                          "synth_ms_rounds": [round(v, 4) for v in synth_ms], "chan_ms_rounds": [round(v, 4) for v in chan_ms],
                          "synth_over_chan": round(sm / cm, 3), "synth_gflops": round(sflops / (sm * 1e-3) / 1e9, 1),
                          "chan_gflops": round(cflops / (cm * 1e-3) / 1e9, 1), "fp64_peak_gflops": round(peak / 1e9, 1),
                          "synth_fraction_of_fp64_peak": round(sflops / (sm * 1e-3) / peak, 4),
                          "chan_fraction_of_fp64_peak": round(cflops / (cm * 1e-3) / peak, 4),
                          "link_seconds_per_second": round(S * n / 48000.0 / (sm * 1e-3), 1), "device": props["name"]}), flush=True)
        sy.close(), ch.close()
    rx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=3)
    ap.add_argument("--D", type=int, default=4)
    ap.add_argument("--raster", type=int, default=3000)
    ap.add_argument("--offsets", default=None, metavar="HZ,HZ,..")
    ap.add_argument("--gains-db", default="0,30,0")
    ap.add_argument("--sidebands", default="u,u,l")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--noise-db", type=float, default=None)
    ap.add_argument("--fmt", default="cf32", choices=["cf32", "cf64"])
    ap.add_argument("--mode", type=int, default=8)
    ap.add_argument("--max-iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--impulses", default=None, metavar="RATE_HZ:DB")
    ap.add_argument("--wblank", nargs="?", const="", default=None, metavar="thr=..,guard=..,block=..")
    ap.add_argument("--imbalance", default=None, metavar="GAIN_DB,PHASE_DEG[,DC_RE,DC_IM]")
    ap.add_argument("--iqfix", nargs="?", const="", default=None, metavar="memory=..,block=..")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--shapes", default="16x4,256x16")
    ap.add_argument("--hops", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    a = ap.parse_args()
    (timing if a.time else loopback)(a)


if __name__ == "__main__":
    main()

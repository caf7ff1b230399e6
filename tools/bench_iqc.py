#!/usr/bin/env python3
"""The IQ corrector measured (include/ext/mercury_iq_corrector.h, profiles/iq_corrector.md).

    python tools/bench_iqc.py --cpu [--seeds 8] [--out profiles/iq_corrector.md]
    python tools/bench_iqc.py --gpu [--formats cs16,cf32,cf64] [--D 4,64] [--blocks 16,1024] [--steps 50] [--warmup 5] [--rounds 5] [--out ..]

--cpu (no GPU: the host twin, which the device equals byte for byte): a station in one sideband (band-limited complex noise at
30.3 .. 32.7 kHz, R = 192 kHz, unit power), alone and under white noise as strong as the station, through a front end of gain 1.1, 5
degrees and DC (0.3, -0.2), CF64, the stage's defaults. The station's image ratio (its band's power over its mirror band's) after the
coefficients the twin reports for the block that ends at 4096 .. 2^20 samples are applied to the impaired station alone, over `--seeds`
draws; the DC's error; the same at 65536 samples from CS16 (the signal at an eighth of full scale).

--gpu: per format, D and blocks per call (B = 4096): one mgpu_iqc_process_dev call per step on a stream of the caller's, device output
and reports, timed by device events around `--steps` calls after `--warmup`, the median of `--rounds` rounds; the same for the fixed
mode (the apply kernel alone), and as yardsticks in the same rounds one mgpu_wblank_process_dev call and one mgpu_chan_process_dev call
of a channeliser of S = 1 on the same samples. The first call is compared byte for byte with the twin. Algorithmic bytes: every sample
is read twice and written once.

Each part prints its section and, with --out, puts it into that file between its markers (the rest of the file stays)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import iqc_ref as ref  # noqa: E402
from mercury_amd import host_iqc_process, iqc_image_db  # noqa: E402

SAMPLE_BYTES = {"cs16": 4, "cf32": 8, "cf64": 16}
LENGTHS = (4096, 16384, 65536, 262144, 1 << 20)


def put_section(path, name, text):
    """text between <!-- name --> and <!-- /name --> of the file (appended where the file has no such markers)"""
    begin, end = "<!-- %s -->" % name, "<!-- /%s -->" % name
    body = "%s\n%s\n%s" % (begin, text.rstrip("\n"), end)
    old = open(path).read() if os.path.exists(path) else ""
    if begin in old and end in old:
        new = old[: old.index(begin)] + body + old[old.index(end) + len(end):]
    else:
        new = old + ("\n" if old and not old.endswith("\n") else "") + body + "\n"
    with open(path, "w") as f:
        f.write(new)


def cpu_part(a):
    n = LENGTHS[-1]
    rows = {}
    for noisy in (False, True):
        for seed in range(1, a.seeds + 1):
            s = ref.station(n, seed)
            alone = ref.impair(s)
            x = ref.impair(s + ref.white(n, 1000 + seed)) if noisy else alone
            _, reports = host_iqc_process(x, 4)
            for length in LENGTHS:
                r = reports[length // 4096 - 1]
                after = ref.image_db(ref.apply(alone, r["dc_re"], r["dc_im"], r["skew"], r["gain"]))
                rows.setdefault((noisy, length), []).append((after, float(np.hypot(r["dc_re"] - ref.DC[0], r["dc_im"] - ref.DC[1])),
                                                             iqc_image_db(r["skew"], r["gain"]), int(r["flags"])))
    before = ref.image_db(ref.impair(ref.station(n, 1)))
    out = ["Uncorrected image ratio %.2f dB (`iqc_image_db` of the planted coefficients: %.2f dB). %d seeds; image ratio after correction in dB"
           % (before, iqc_image_db(ref.GAIN * np.sin(np.radians(ref.PHASE_DEG)), 1.0 / (ref.GAIN * np.cos(np.radians(ref.PHASE_DEG)))), a.seeds),
           "(least / median / greatest over the seeds), the DC's error (median, greatest), what `iqc_image_db` says of the reported",
           "coefficients (least .. greatest), blocks flagged.", "",
           "| noise | samples seen | image ratio after: least | median | greatest | DC error: median | greatest | described dB | flagged |",
           "|---|---|---|---|---|---|---|---|---|"]
    for noisy in (False, True):
        for length in LENGTHS:
            v = np.array(rows[(noisy, length)])
            out.append("| %s | %d | %.1f | %.1f | %.1f | %.2e | %.2e | %.2f .. %.2f | %d |"
                       % ("as strong as the station" if noisy else "none", length, v[:, 0].min(), np.median(v[:, 0]), v[:, 0].max(),
                          np.median(v[:, 1]), v[:, 1].max(), v[:, 2].min(), v[:, 2].max(), int((v[:, 3] != 0).sum())))
    # CS16: the noisy input at an eighth of full scale, 65536 samples
    cs = []
    for seed in range(1, a.seeds + 1):
        s = ref.station(65536, seed)
        x = ref.to_format(ref.impair(s + ref.white(65536, 1000 + seed)), "cs16", 0.125)
        o, reports = host_iqc_process(x, 4)
        r = reports[-1]
        after = ref.image_db(ref.apply(ref.impair(s), r["dc_re"] * 8.0, r["dc_im"] * 8.0, r["skew"], r["gain"]))
        cs.append((after, float(np.hypot(r["dc_re"] * 8.0 - ref.DC[0], r["dc_im"] * 8.0 - ref.DC[1])), int(reports["clamped"].sum()),
                   int(np.abs(x.astype(np.int32)).max())))
    cs = np.array(cs)
    out += ["", "CS16, the noisy input at an eighth of full scale (greatest |component| %d of 32768), 65536 samples: image ratio after %.1f / %.1f / %.1f"
            % (int(cs[:, 3].max()), cs[:, 0].min(), np.median(cs[:, 0]), cs[:, 0].max()),
            "dB (least / median / greatest), DC error (in the unscaled signal's units) median %.2e, greatest %.2e; clamped components %d."
            % (np.median(cs[:, 1]), cs[:, 1].max(), int(cs[:, 2].sum()))]
    return "\n".join(out)


def gpu_part(a):
    import torch
    from mercury_amd import (IQC_REPORT_DTYPE, WBLANK_REPORT_DTYPE, Channelizer, IqCorrector, RxPhy, WidebandBlanker, device_props)
    props = device_props(0)
    rx = RxPhy(8, max_batch=8)
    stream = torch.cuda.Stream()

    def timed(fn):
        """ms per call: device events on the stream around a.steps calls, after a.warmup"""
        for _ in range(a.warmup):
            fn()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            start.record()
            for _ in range(a.steps):
                fn()
            stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / a.steps

    lines = []
    out = ["| D | format | blocks | IQ samples | corrector ms per call | rounds (least .. greatest) | fixed mode (apply alone) ms | blanker ms | channeliser S = 1 ms | share of the channeliser | algorithmic GB/s | GS/s | × real time | equals the twin |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for D in (int(v) for v in a.D.split(",")):
        for blocks in (int(v) for v in a.blocks.split(",")):
            n_in = blocks * 4096
            for fmt in a.formats.split(","):
                z = ref.impair(0.1 * ref.white(n_in, D + blocks, 2.0))
                x = ref.to_format(z, fmt)
                qc = IqCorrector(rx, D, fmt, max_in=n_in)
                fx = IqCorrector(rx, D, fmt, max_in=n_in, fixed=1, fixed_dc_re=0.03, fixed_dc_im=-0.02, fixed_skew=0.0959, fixed_gain=0.9126)
                wb = WidebandBlanker(rx, D, fmt, block=4096, max_in=n_in)
                ch = Channelizer(rx, D, [(0, 0, 1.0)], max_out=n_in // D)
                d_x = torch.from_numpy(x).cuda()
                d_out = torch.zeros_like(d_x)
                d_rep = torch.zeros((blocks, IQC_REPORT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
                d_wrep = torch.zeros((blocks, WBLANK_REPORT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
                d_audio = torch.zeros((1, n_in // D), dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                s = stream.cuda_stream
                n = qc.process_raw(d_x, d_out, d_rep, stream=s)
                stream.synchronize()
                want_o, want_r = host_iqc_process(x, D)
                same = bool(n == len(want_r) and d_out.cpu().numpy().tobytes() == want_o.tobytes() and d_rep.cpu().numpy().tobytes() == want_r.tobytes())
                t = {"iqc": [], "fixed": [], "wblank": [], "chan": []}
                for _ in range(a.rounds):                               # alternating: what shares the machine moves all alike
                    t["iqc"].append(timed(lambda: qc.process_raw(d_x, d_out, d_rep, stream=s)))
                    t["fixed"].append(timed(lambda: fx.process_raw(d_x, d_out, d_rep, stream=s)))
                    t["wblank"].append(timed(lambda: wb.process_raw(d_x, d_out, d_wrep, stream=s)))
                    t["chan"].append(timed(lambda: ch.process(d_x, out=d_audio, stream=s)))
                med = {k: float(np.median(v)) for k, v in t.items()}
                nbytes = 3 * n_in * SAMPLE_BYTES[fmt]
                line = {"D": D, "format": fmt, "blocks": blocks, "iq_samples": n_in, "iqc_ms_per_call": round(med["iqc"], 5),
                        "iqc_ms_rounds": [round(v, 5) for v in t["iqc"]], "iqc_fixed_ms_per_call": round(med["fixed"], 5),
                        "wblank_ms_per_call": round(med["wblank"], 5), "channeliser_S1_ms_per_call": round(med["chan"], 5),
                        "algorithmic_gb_per_s": round(nbytes / (med["iqc"] * 1e-3) / 1e9, 1), "gs_per_s": round(n_in / (med["iqc"] * 1e-3) / 1e9, 3),
                        "times_real_time": round(n_in / (med["iqc"] * 1e-3) / (48000.0 * D), 1), "byte_identical_to_twin": same,
                        "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "device": props["name"]}
                lines.append(line)
                print(json.dumps(line), flush=True)
                out.append("| %d | %s | %d | %d | %.4f | %.4f .. %.4f | %.4f | %.4f | %.4f | %.1f %% | %.0f | %.2f | %.0f | %s |"
                           % (D, fmt.upper(), blocks, n_in, med["iqc"], min(t["iqc"]), max(t["iqc"]), med["fixed"], med["wblank"], med["chan"],
                              100.0 * med["iqc"] / med["chan"], line["algorithmic_gb_per_s"], line["gs_per_s"], line["times_real_time"],
                              "yes" if same else "NO"))
                for h in (qc, fx, wb, ch):
                    h.close()
    rx.close()
    head = ("One %s; device events around %d calls after %d warm-up calls, the median of %d alternating rounds; B = 4096, memory 1024, the"
            "\nsame input every step (read from the caches, not from HBM, where it fits them).\n\n" % (props["name"], a.steps, a.warmup, a.rounds))
    return head + "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--formats", default="cs16,cf32,cf64")
    ap.add_argument("--D", default="4,64")
    ap.add_argument("--blocks", default="16,1024")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not (a.cpu or a.gpu):
        ap.error("--cpu or --gpu")
    for name, part in (("cpu", cpu_part), ("gpu", gpu_part)):
        if getattr(a, name):
            text = part(a)
            print(text, flush=True)
            if a.out:
                put_section(a.out, "bench_iqc --" + name, text)


if __name__ == "__main__":
    main()

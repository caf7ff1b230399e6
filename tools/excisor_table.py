#!/usr/bin/env python3
"""What the carrier excisor (include/ext/mercury_excisor.h) is worth: the sweep of profiles/excisor.md. Per scenario and
signal-to-interference ratio, --windows seeded capture windows (tests/excisor_ref.py: a frame at a varying delay in noise, plus the carrier)
go through the CPU oracle's receive_byte raw and behind the host twin (mgpu_host_excise); with --gpu they go through RxPhy.receive_byte with
the stage off and on instead. Tone power is relative to the frame's own power. Prints the markdown table, entries "decoded raw -> excised",
and with --clean the worst ratio of the highest bin to the band median on windows without a carrier, per mode.

usage: excisor_table.py [--windows 32] [--thr 8,12] [--jobs 8] [--gpu] [--clean] [--only N]"""
import argparse
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import excisor_ref as er  # noqa: E402

# (mode, noise sigma, [tone offsets from the carrier in Hz], keyed on / off in ms or None)
SCENARIOS = [(8, 0.02, [317.0], None), (8, 0.1, [317.0], None), (8, 0.02, [317.0, -600.0], None), (8, 0.02, [317.0], 60.0),
             (0, 0.1, [-450.0], None), (13, 0.01, [100.0], None), (100, 0.05, [100.0], None)]
SIRS = [10.0, 0.0, -10.0, -20.0]


def _name(sc):
    cfg, sigma, tones, key = sc
    what = " and ".join("%+g Hz" % f for f in tones)
    return "mode %d%s, noise sigma %g, %s%s" % (cfg, " (MFSK)" if cfg >= 100 else "", sigma, "tones at carrier " + what if len(tones) > 1 else "tone at carrier " + what,
                                                ", keyed %g ms on / %g ms off" % (key, key) if key else "")


def _windows(sc, sir, count):
    from oraclelib import CARRIER
    cfg, sigma, tones, key = sc
    t = er.toned_windows(cfg, 0.0, sigma, tones[0], count=count, seed=1)
    x = np.array(t["clean"])
    for j, f in enumerate(tones):
        x = er.add_tone(t["orc"], x, sir, f, CARRIER, key_ms=key, phase=0.2 + 1.3 * j)
    return t["orc"], x, t["payload"]


def cell(job):
    """-> (raw decoded, {thr: (decoded, most bins removed, windows over the cap)})"""
    from mercury_amd import host_excise
    from oraclelib import CARRIER
    sc, sir, count, thrs, gpu = job
    orc, x, pls = _windows(sc, sir, count)
    if gpu:
        from mercury_amd import RxPhy
        rx = RxPhy(sc[0], max_batch=count)
        good = lambda out: sum(out["stats"]["message_decoded"][w] == 1 and np.array_equal(out["payload"][w][: orc.payload_bytes], pls[w]) for w in range(count))
        raw, res = good(rx.receive_byte(x, CARRIER)), {}
        for thr in thrs:
            rx.set_excisor("welch", threshold=thr)
            n = good(rx.receive_byte(x, CARRIER))
            rep = rx.excisor_report(0, count)
            res[thr] = (n, int(rep["excised"].max()), int(((rep["mask"] != 0) & (rep["excised"] == 0)).sum()))
            rx.set_excisor("off")
        rx.close()
        return raw, res
    raw = sum(er.decoded(orc, orc.receive_byte(x[w], carrier=CARRIER), pls[w]) for w in range(count))
    res = {}
    for thr in thrs:
        n = most = over = 0
        for w in range(count):
            y, rep = host_excise(x[w], CARRIER, threshold=thr)
            n += er.decoded(orc, orc.receive_byte(y, carrier=CARRIER), pls[w])
            most = max(most, rep["excised"])
            over += int(rep["mask"] != 0 and rep["excised"] == 0)
        res[thr] = (n, most, over)
    return raw, res


def clean_ratio(cfg):
    """the highest-bin / median ratio of the summed spectrum on windows without a carrier -> (cfg, [(kind, ratio, mask bits at the defaults)]).
    OFDM modes: a strong clean frame, two equal static paths 1 and 2 ms apart, noise only, a short window; MFSK modes: three noise levels
    (an MFSK frame under two equal paths is listed too, apart: its tones are carriers, and a notch between them lowers the median)."""
    from mercury_amd import host_excise
    from oraclelib import CARRIER
    rng = np.random.default_rng(cfg)

    def frame(sigma):
        return np.array(er.toned_windows(cfg, 0.0, sigma, 0.0, count=1, seed=2)["clean"][0])

    x = frame(0.001)
    if cfg < 100:
        kinds = {"strong clean frame": x, "two equal paths 1 ms apart": x + np.roll(x, 48), "two equal paths 2 ms apart": x + np.roll(x, 96),
                 "noise only": 0.05 * rng.standard_normal(x.size), "short window": x[np.argmax(np.abs(x) > 0.1):][:8192]}
    else:
        kinds = {"noise sigma %g" % sigma: frame(sigma) for sigma in (0.001, 0.05, 0.5)}
        kinds.update({"(two equal paths 1 ms apart)": x + np.roll(x, 48), "(two equal paths 2 ms apart)": x + np.roll(x, 96)})
    rows = []
    for kind, w in kinds.items():
        _, rep = host_excise(w, CARRIER)
        rows.append((kind, float(np.max(er.ref_excise(w, CARRIER)[1]["A"]) / rep["level"]), bin(rep["mask"]).count("1")))
    return cfg, rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=32)
    ap.add_argument("--thr", default="8,12")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--clean", action="store_true")
    ap.add_argument("--only", type=int, default=None, help="one scenario (0-based)")
    a = ap.parse_args()
    thrs = [float(v) for v in a.thr.split(",")]
    rows = SCENARIOS if a.only is None else [SCENARIOS[a.only]]
    jobs = [(sc, sir, a.windows, thrs, a.gpu) for sc in rows for sir in SIRS]
    if a.gpu:
        done = [cell(j) for j in jobs]                       # one process holds the GPU
    else:
        with Pool(a.jobs) as pool:
            done = pool.map(cell, jobs, chunksize=1)
    print("| scenario (%d windows per cell%s) | thr | %s |" % (a.windows, ", on the GPU" if a.gpu else "", " | ".join("SIR %g dB" % s for s in SIRS)))
    print("|---|---|%s" % ("---|" * len(SIRS)))
    for i, sc in enumerate(rows):
        for thr in thrs:
            cells = []
            for j in range(len(SIRS)):
                raw, res = done[i * len(SIRS) + j]
                n, most, over = res[thr]
                cells.append("%d -> %d (%d bins%s)" % (raw, n, most, ", %d over the cap" % over if over else ""))
            print("| %s | %g | %s |" % (_name(sc), thr, " | ".join(cells)), flush=True)
    if a.clean:
        modes = list(range(17)) + [100, 101, 102]
        with Pool(a.jobs) as pool:
            ratios = pool.map(clean_ratio, modes, chunksize=1)
        print("\n| mode | worst highest bin / band median on windows without a carrier | on | flagged at the defaults |\n|---|---|---|---|")
        for cfg, rows in ratios:
            own = [r for r in rows if not r[0].startswith("(")]
            kind, ratio, _ = max(own, key=lambda r: r[1])
            flagged = ", ".join("%s: %.2f, %d bins" % r for r in rows if r[2]) or "none"
            print("| %d | %.2f | %s | %s |" % (cfg, ratio, kind, flagged))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the impulse blanker (include/mercury_blanker.h) is worth, CPU only: the frames of tests/blanker_ref.py (clean frames
of the generator, seed 5; an optional Rayleigh-like gain, noise, and impulses at a fixed period from default_rng(11), their power relative to
the clean frame's mean power) through the CPU oracle alone, through the noise-map twin alone (mgpu_host_demap_nmap on the oracle's grid and
estimate, into the oracle's decoder), and through the blanker's host twin (mgpu_host_blank) into the oracle. Prints the markdown table of
profiles/blanker.md: frames decoded with the sent bits, the samples zeroed per frame, and the samples marked on frames without impulses.

usage: blanker_table.py [--frames 32] [--thr 24] [--guard 4] [--share 0.125]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from blanker_ref import decoded, impulse_frames  # noqa: E402
from demapper_csi_ref import full_estimate, llr_src  # noqa: E402

# (cfg, Es/N0 dB, impulse dB or None, width, period, Doppler of the gain in Hz or 0)
ROWS = [(13, 14.0, 25.0, 1, 100, 0.0), (11, 10.0, 25.0, 1, 100, 0.0), (8, 6.0, 30.0, 2, 100, 0.0), (8, 6.0, 25.0, 1, 100, 0.0),
        (8, 6.0, 25.0, 2, 120, 0.0), (13, 14.0, 25.0, 2, 120, 0.0),
        (8, 6.0, None, 1, 100, 0.0), (13, 14.0, None, 1, 100, 0.0), (11, 10.0, None, 1, 100, 0.0), (0, 6.0, None, 1, 100, 0.0),
        (8, 12.0, 25.0, 1, 100, 1.0), (8, 12.0, None, 1, 100, 1.0), (8, 12.0, None, 1, 100, 5.0),
        (0, 6.0, None, 1, 100, 1.0), (0, 6.0, None, 1, 100, 5.0), (0, 12.0, None, 1, 100, 1.0), (0, 12.0, None, 1, 100, 5.0)]


def main():
    from mercury_amd import host_blank, host_demap_nmap
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--thr", type=float, default=24.0)
    ap.add_argument("--guard", type=int, default=4)
    ap.add_argument("--share", type=float, default=0.125)
    a = ap.parse_args()
    prm = dict(threshold=a.thr, guard=a.guard, max_share=a.share)
    print("| mode | Es/N0 | gain | disturbance | oracle alone | noise-map twin alone | oracle on blanked samples | marked per frame (max) / cap | frames over the cap |")
    print("|---|---|---|---|---|---|---|---|---|")
    for cfg, esn0, db, width, period, fd in ROWS:
        t = impulse_frames(cfg, None, esn0, db, width, period, a.frames, fd)
        orc, src = t["orc"], llr_src(t["orc"])
        plain = nmap = fixed = most = over = 0
        for f in range(a.frames):
            ref = orc.rx(t["bb"][f])
            plain += decoded(orc, ref, t["bits"][f])
            llr = host_demap_nmap(cfg, ref["grid"], full_estimate(orc, ref))[0]
            nmap += int(np.array_equal(orc.ldpc_decode(llr[src])[0], t["bits"][f]))
            got, rep = host_blank(cfg, t["bb"][f], **prm)
            most = max(most, rep["marked"])
            over += int(rep["marked"] > rep["blanked"])
            fixed += decoded(orc, orc.rx(got), t["bits"][f])
        what = "noise only" if db is None else "%g dB impulses, %d sample%s, every %d" % (db, width, "s" if width > 1 else "", period)
        print("| %d | %g dB | %s | %s | %d / %d | %d / %d | %d / %d | %d / %d | %d |"
              % (cfg, esn0, "%g Hz" % fd if fd else "static", what, plain, a.frames, nmap, a.frames, fixed, a.frames, most,
                 int(np.floor(a.share * orc.frame_samples)), over), flush=True)


if __name__ == "__main__":
    main()

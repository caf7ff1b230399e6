#!/usr/bin/env python3
"""What the noise-map demapper (include/mercury_demapper.h MGPU_DEMAP_NMAP) is worth, CPU only: the CPU oracle's stage
outputs through the library's host twins (mgpu_host_demap_csi, mgpu_host_demap_nmap) and the oracle's decoder, 32 frames per point, on the
disturbed frames of tests/noise_map_ref.py (clean frames of the generator, seed 5; noise, a tone at a random off-bin frequency and a burst of
272 samples from default_rng(11), their powers relative to the clean frame's mean power). Prints the markdown table of
profiles/noise_map.md: frames decoded by the oracle alone, with the CSI rule, with the noise map.

usage: noise_map_table.py [--band 2] [--smooth 1] [--frames 32]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from noise_map_ref import DY5, decoded_count, disturbed, twin_decode  # noqa: E402

# (label, cfg, explicit, Es/N0 dB, tone dB, burst dB, delay of a second path in samples)
ROWS = [("mode 8, 6 dB, tone +5 dB", 8, None, 6.0, 5.0, None, 0),
        ("mode 8, 6 dB, tone +3 dB and burst +15 dB", 8, None, 6.0, 3.0, 15.0, 0),
        ("mode 8, Dy 5 / Nsymb 20, same", 8, DY5, 6.0, 3.0, 15.0, 0),
        ("mode 8, 3 dB, tone -3 dB and burst +8 dB", 8, None, 3.0, -3.0, 8.0, 0),
        ("mode 13, 14 dB, tone 0 dB", 13, None, 14.0, 0.0, None, 0),
        ("mode 13, 14 dB, burst +15 dB", 13, None, 14.0, None, 15.0, 0),
        ("mode 11, 12 dB, tone 0 dB and burst +12 dB", 11, None, 12.0, 0.0, 12.0, 0),
        ("mode 13, 15 dB, two paths 12 samples apart, 5 x 5 window, tone 0 dB", 13, dict(ls_window=5), 15.0, 0.0, None, 12),
        ("mode 8, AWGN only, 0 dB", 8, None, 0.0, None, None, 0),
        ("mode 8, AWGN only, -0.5 dB", 8, None, -0.5, None, None, 0)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--band", type=float, default=2.0)
    ap.add_argument("--smooth", type=int, default=1)
    ap.add_argument("--frames", type=int, default=32)
    a = ap.parse_args()
    print("| case | oracle alone | CSI twin | noise map, band %g, smooth %d |" % (a.band, a.smooth))
    print("|---|---|---|---|")
    for label, cfg, explicit, esn0, tone, burst, delay in ROWS:
        t = disturbed(cfg, explicit, esn0, tone, burst, a.frames, delay)
        csi = decoded_count(t, twin_decode(cfg, explicit, esn0, tone, burst, a.frames, "csi", delay=delay))
        nmap = decoded_count(t, twin_decode(cfg, explicit, esn0, tone, burst, a.frames, "nmap", a.band, a.smooth, delay))
        print("| %s | %d | %d | %d |" % (label, int(t["plain_ok"].sum()), csi, nmap), flush=True)


if __name__ == "__main__":
    main()

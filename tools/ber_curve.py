#!/usr/bin/env python3
"""The reference's BER_PLOT_baseband self-simulation (telecom_system.cc:2393-2480: 25 Es/N0 points, 100 frames each on the CPU) on the GPU:
prints EsN0;BER;FER lines like the reference does, for far more frames per point.   usage: ber_curve.py [cfg] [frames_per_point] [decoder]
                                                                        ber_curve.py --passband [cfg] [frames_per_point]
--passband: BER_PLOT_passband_process_main (:2432-2470: the audio path, transmit_byte -> AWGN with delay -> receive_byte; 25 points from
-10 dB in 0.5 dB steps x 100 frames for OFDM, 31 points from -25 dB x 3 frames for MFSK, output power 1 W).
--channel {awgn,good,moderate,poor,flutter} (either form): the Watterson HF channel of include/mercury_channel.h in front of the noise
(the CCIR 520 presets; awgn = identity, which gives exactly the plain loop's numbers). Without it the plain AWGN entry points run.
--threshold (with --passband: ber_curve.py --passband [--channel C] --threshold cfg [frames_per_point]): Es/N0 from 3 dB below the
reference's AWGN FER < 0.1 value (include/common/common_defines.h:130-147) to 40 dB above it in 1 dB steps, in one call; one JSON line
gives the first point of the first run of three with FER < 0.1 ("fer01_esn0_db", null if none) beside the AWGN value.
--ladder 21x21,5x21 (any form): an estimator ladder (include/mercury_estimator.h; windows as carriers x symbols, or `wiener` /
`wiener:tau=-333/2333,fd=0.5,snr=5` for the separable Wiener estimator, `bank:tau=-333/333|-333/1000|-333/2333,snr=5` for one that
chooses its design per frame, include/mercury_wiener_bank.h) on the context; the JSON
line then carries the frames each rung decoded.
--diversity D (baseband form; with --channel and at most a one-rung --ladder): D branches per payload, each with its own channel realisation
and noise, decoded from their summed LLRs (include/mercury_diversity.h); frames_per_point counts payloads, Es/N0 is per branch.
--points LO:HI:STEP (baseband form): the Es/N0 points instead of the reference's 25.
--demapper csi (any form, with any of the above): LLRs weighted by |H|^2 per cell (include/mercury_demapper.h) instead of the reference's
demapper; --demapper nmap[:band=2,smooth=1]: those divided by a noise factor per carrier and per symbol measured at the pilots.
--cfo pilots (any form, with any of the above): every frame's grid turned back by the phase step its own pilots measure (include/mercury_cfo.h).
--blanker median[:thr=24,guard=4,share=0.125] (any form, with any of the above): every frame through the median-gated impulse blanker ahead of
the front-end (include/mercury_blanker.h). The self-simulations have no impulse source: this measures what the stage costs a clean channel.
--excisor welch[:thr=12,guard=1,bins=16] (--passband only): every capture window through the carrier excisor ahead of the synchroniser
(include/ext/mercury_excisor.h). The self-simulations have no tone source either: what the stage costs a clean channel."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mercury_amd import RxPhy, physical_layer as pl  # noqa: E402


# EsN0 (dB) at FER < 0.1 on AWGN, include/common/common_defines.h:130-147 (the reference's mode ladder, get_configuration)
AWGN_FER01 = {0: -10.0, 1: -7.5, 2: -6.0, 3: -4.5, 4: -3.5, 5: -2.5, 6: -1.5, 7: -0.5, 8: 0.5, 9: 1.5, 10: 3.0, 11: 4.0, 12: 6.5, 13: 7.5,
              14: 9.0, 15: 12.5, 16: 13.5}


LADDER = []          # --ladder
DEMAPPER = ["maxlog"]   # --demapper
CFO = ["off"]           # --cfo
BLANKER = ["off"]       # --blanker
EXCISOR = ["off"]       # --excisor (the passband forms)


def _rung_names(rx):
    return ["wiener" if r[0] == "wiener" else "%dx%d" % r for r in rx.estimator_ladder_ex]


def _ladder_fields(rx):
    if not LADDER:
        return {}
    by, frames = rx.ladder_counters()
    return {"ladder": _rung_names(rx), "decoded_by_rung": [int(v) for v in by[: len(LADDER)]], "ladder_frames": frames}


def threshold(cfg, n, channel):
    """One call over Es/N0 = AWGN value - 3 dB ... + 40 dB in 1 dB steps; the first point of the first run of three with FER < 0.1."""
    rx = RxPhy(cfg, max_batch=min(n, 1024))
    rx.set_estimator_ladder(LADDER)
    rx.set_demapper(DEMAPPER[0])
    rx.set_cfo(CFO[0])
    rx.set_blanker(BLANKER[0])
    rx.set_excisor(EXCISOR[0])
    pts = AWGN_FER01.get(cfg, -20.0) - 3.0 + np.arange(44, dtype=np.float64)
    t0 = time.perf_counter()
    res = rx.passband_test_esn0(pts, n, 1500.0, seed=2024, output_power_watt=1.0, hf_channel=channel)
    extra = _ladder_fields(rx)
    rx.close()
    fer = [r["FER"] for r in res]
    first = next((float(pts[i]) for i in range(len(pts) - 2) if max(fer[i: i + 3]) < 0.1), None)
    print(json.dumps({"cfg": cfg, "channel": channel or "awgn", "frames_per_point": n, "fer01_esn0_db": first,
                      "awgn_reference_db": AWGN_FER01.get(cfg), "demapper": DEMAPPER[0], "cfo": CFO[0], "blanker": BLANKER[0], "excisor": EXCISOR[0], "fer_by_esn0": [[float(e), f] for e, f in zip(pts, fer)],
                      "seconds": round(time.perf_counter() - t0, 2), **extra}), flush=True)


def passband(argv, channel):
    if argv and argv[0] == "--threshold":
        return threshold(int(argv[1]) if len(argv) > 1 else 8, int(argv[2]) if len(argv) > 2 else 256, channel)
    cfg = int(argv[0]) if argv else 8
    n = int(argv[1]) if len(argv) > 1 else 4096
    rx = RxPhy(cfg, max_batch=min(n, 1024))
    rx.set_estimator_ladder(LADDER)
    rx.set_demapper(DEMAPPER[0])
    rx.set_cfo(CFO[0])
    rx.set_blanker(BLANKER[0])
    rx.set_excisor(EXCISOR[0])
    pts = np.arange(31) * 1.0 - 25.0 if cfg >= 100 else np.arange(25) * 0.5 - 10.0
    rx.passband_test_esn0(pts[-1:], min(n, 1024), 1500.0, output_power_watt=1.0, hf_channel=channel)
    t0 = time.perf_counter()
    res = rx.passband_test_esn0(pts, n, 1500.0, seed=2024, output_power_watt=1.0, hf_channel=channel)
    dt = time.perf_counter() - t0
    for r in res:
        print("%.1f;%.3e;%.3e;%d" % (r["esn0_db"], r["BER"], r["FER"], r["crc_ok_frames"]))
    print(json.dumps({"cfg": cfg, "mode": "passband", "channel": channel or "awgn", "points": len(res), "frames_per_point": n, "seconds": dt,
                      "frames_per_s": len(res) * n / dt, "demapper": DEMAPPER[0], "cfo": CFO[0], "blanker": BLANKER[0], "excisor": EXCISOR[0], **_ladder_fields(rx)}), file=sys.stderr)


def baseband(cfg, n, dec=pl.DEC_SPA, channel=None, diversity=None, pts=None, seed=2024, warm=True):
    """the baseband loop's records for one mode: (list of per-point dicts, summary dict)"""
    per = max(1, diversity or 1)
    rx = RxPhy(cfg, max_batch=min(n * per, 65536), agc=0, variance_source=0, decoder=dec)          # the variant baseband_test_EsN0 runs
    rx.set_estimator_ladder(LADDER)
    rx.set_demapper(DEMAPPER[0])
    rx.set_cfo(CFO[0])
    rx.set_blanker(BLANKER[0])
    if pts is None:
        pts = np.arange(-12.0, 13.0, 1.0)[:25] + (0.0 if cfg >= 7 else -6.0)
    if warm:
        rx.baseband_test_esn0(pts[:1], min(n, 4096), hf_channel=channel, diversity=diversity)
    t0 = time.perf_counter()
    res = rx.baseband_test_esn0(pts, n, seed=seed, hf_channel=channel, diversity=diversity)
    dt = time.perf_counter() - t0
    # a grouped span does not run the ladder's marking pass: with --diversity only the window is reported
    extra = {"diversity": diversity, "ladder": _rung_names(rx)} if diversity else _ladder_fields(rx)
    rx.close()
    return res, {"cfg": cfg, "channel": channel or "awgn", "points": len(res), "frames_per_point": n, "seconds": dt,
                 "frames_per_s": len(res) * n * per / dt, "demapper": DEMAPPER[0], "cfo": CFO[0], "blanker": BLANKER[0], **extra}


def _option(argv, name):
    """the value of --name V / --name=V, removed from argv; None when absent"""
    for i, a in enumerate(argv):
        if a == name or a.startswith(name + "="):
            value = a.split("=", 1)[1] if "=" in a else argv[i + 1]
            del argv[i: i + (1 if "=" in a else 2)]
            return value
    return None


def main():
    argv = sys.argv[1:]
    channel = None
    diversity = _option(argv, "--diversity")
    points = _option(argv, "--points")
    DEMAPPER[0] = _option(argv, "--demapper") or "maxlog"
    try:
        pl.parse_demapper(DEMAPPER[0])
    except ValueError as e:
        sys.exit("--" + str(e))
    CFO[0] = _option(argv, "--cfo") or "off"
    if CFO[0] not in pl.CFO_MODES:
        sys.exit("--cfo: one of " + ", ".join(pl.CFO_MODES))
    BLANKER[0] = _option(argv, "--blanker") or "off"
    try:
        pl.parse_blanker(BLANKER[0])
    except ValueError as e:
        sys.exit("--" + str(e))
    EXCISOR[0] = _option(argv, "--excisor") or "off"
    try:
        pl.parse_excisor(EXCISOR[0])
    except ValueError as e:
        sys.exit("--" + str(e))
    if EXCISOR[0] != "off" and "--passband" not in argv:
        sys.exit("--excisor: the stage sits ahead of the synchroniser, --passband only")
    for i, a in enumerate(argv):
        if a == "--channel" or a.startswith("--channel="):
            channel = a.split("=", 1)[1] if "=" in a else argv[i + 1]
            del argv[i: i + (1 if "=" in a else 2)]
            if channel not in pl.HF_PRESETS:
                sys.exit("--channel: one of " + ", ".join(pl.HF_PRESETS))
            break
    for i, a in enumerate(argv):
        if a == "--ladder" or a.startswith("--ladder="):
            LADDER[:] = pl.parse_ladder(a.split("=", 1)[1] if "=" in a else argv[i + 1])
            del argv[i: i + (1 if "=" in a else 2)]
            break
    if argv and argv[0] == "--passband":
        if diversity is not None:
            sys.exit("--diversity runs on the baseband loop (the passband loop's synchroniser does not combine)")
        return passband(argv[1:], channel)
    cfg = int(argv[0]) if argv else 8
    n = int(argv[1]) if len(argv) > 1 else 65536
    dec = {"spa": pl.DEC_SPA, "spa_fast": pl.DEC_SPA_FAST, "minsum": pl.DEC_MINSUM}[argv[2] if len(argv) > 2 else "spa"]
    if diversity is not None and len(LADDER) > 1:
        sys.exit("--diversity takes at most a one-rung --ladder (a ladder's retries do not combine)")
    pts = None
    if points:
        lo, hi, step = (float(v) for v in points.split(":"))
        pts = np.arange(lo, hi + step / 2, step)
    res, summary = baseband(cfg, n, dec, channel, int(diversity) if diversity is not None else None, pts)
    for r in res:
        print("%.1f;%.3e;%.3e;%.2f" % (r["esn0_db"], r["BER"], r["FER"], r["avg_iterations"]))
    print(json.dumps(summary), file=sys.stderr)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Link simulator (include/mercury_linksim.h): S transmitter -> streaming HF channel -> noise -> capture-receive links on one GPU.

usage: link_sim.py --cfg 8 --links 1024 --seconds 30 --channel moderate --esn0 0:20:2 [--gap-hops 0] [--seed 1]
The Es/N0 ladder A:B:step (or one number) is spread evenly over the links. Prints one JSON line per Es/N0 (frames sent, delivered,
duplicates, false decodes, mean iterations of the delivered frames) and a last line with simulated link-seconds per wall second.
  --dry-run    print the plan (slot, latency, device bytes) without a device
  --baseline   instead of the simulator, the composition available without it: a Python loop per round over transmit_byte (host),
               hf_channel_apply on the round's chunk (a whole-signal call per chunk: the Hilbert FIR and the path delays see zeros at every
               chunk edge, so this is wrong there) and RxCapture.run from host memory; no noise is added and nothing is counted
  --repeats N  run the measurement N times (with --compare: simulator and baseline alternating) and print every rate
  --stream-bench  time the streaming channel kernel alone on [links][max_hops * P] chunks: samples/s and its fp64 fraction by the cost
               model of DESIGN.md §6.1 / §6.2"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mercury_amd import HfStream, LinkSim, RxCapture, RxPhy, hf_channel_preset, linksim_config, load_library, parse_ladder  # noqa: E402
from mercury_amd.physical_layer import Info  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12          # MI355X fp64 vector FLOP/s (spec)
FS, LATENCY, HILBERT_HALF, HILBERT_ODD, TILE = 48000.0, 256, 215, 108, 1024


def ladder(text, S):
    parts = [float(v) for v in text.split(":")]
    pts = [parts[0]] if len(parts) == 1 else list(np.arange(parts[0], parts[1] + 1e-9, parts[2] if len(parts) > 2 else 1.0))
    return pts, np.array([pts[s * len(pts) // S] for s in range(S)])


def _excisor(text):
    """--excisor: the spec as RxPhy.set_excisor takes it, checked by the library's one parser"""
    from mercury_amd import parse_excisor
    try:
        parse_excisor(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return text


def _blanker(text):
    """--blanker: the spec as RxPhy.set_blanker takes it, checked by the library's one parser"""
    from mercury_amd import parse_blanker
    try:
        parse_blanker(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return text


def _demapper(text):
    """--demapper: the spec as RxPhy.set_demapper takes it, checked by the library's one parser"""
    from mercury_amd import parse_demapper
    try:
        parse_demapper(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return text


def carrier_of(info):
    return 48000.0 / 4 * info.Nc / info.Nfft / 2 + 300          # physical_config.cc:84: bandwidth / 2 + 300


def plan(a):
    """what a run needs, from the host tables alone"""
    i = Info()
    if load_library().mgpu_host_mode_info(a.cfg, 0, C.byref(i)) != 0:
        raise SystemExit("unknown configuration %d" % a.cfg)
    P, frame_hops = i.Nofdm * 4, i.Nsymb + i.preamble_nsymb
    frame, slot = frame_hops * P, (frame_hops + a.gap_hops) * P
    ch = hf_channel_preset(a.channel)
    dmax = max(round(ch.delay_ms[k] * FS / 1000.0) for k in range(ch.n_paths))
    hist = LATENCY + dmax + HILBERT_HALF
    buffer_nsymb = max(2 * frame_hops, frame_hops + math.ceil(1200.0 / (1000.0 * P / FS)) + 4, 32)
    max_hops = a.max_hops or 16
    round_hops = min(max_hops, slot // P)
    S = a.links
    dev = dict(frame_store=S * 2 * frame * 8, transmit_staging=S * 2 * frame * 8, round_in_out=2 * S * round_hops * P * 8, history=2 * S * hist * 8,
               capture_rings=S * (buffer_nsymb + max_hops) * P * 8, gathered_windows=min(S, a.max_batch or S) * buffer_nsymb * P * 8)
    hops = int(math.ceil(a.seconds * FS / P))
    return dict(cfg=a.cfg, links=S, channel=a.channel, gap_hops=a.gap_hops, symbol_period=P, frame_samples=frame, slot_samples=slot,
                slot_seconds=slot / FS, latency_samples=LATENCY, history_samples=hist, round_hops=round_hops, hops=hops,
                frames_per_link=hops * P // slot, device_bytes=dev, device_bytes_total=sum(dev.values()),
                whole_run_bytes_avoided=2 * S * hops * P * 8), i


def run_sim(rx, a, info, esn0, hops):
    k = linksim_config(a.links, carrier_of(info), a.seed, channel=a.channel, gap_hops=a.gap_hops, max_hops=a.max_hops, output_power_watt=a.power)
    sim = LinkSim(rx, k, esn0, ladder=parse_ladder(a.ladder))
    sim.run(min(hops, 2 * (a.max_hops or 16)), max_events=0)              # warm: workspaces, carrier table, first frames
    t = time.perf_counter()
    done = 0
    while done < hops:
        n = min(hops - done, 64 * (a.max_hops or 16))
        sim.run(n, max_events=0)
        done += n
    wall = time.perf_counter() - t
    c = sim.counters()
    sim.close()
    return c, wall


def run_baseline(rx, a, info, hops):
    """the parent-commit composition: per round, host transmit_byte, hf_channel_apply on the chunk, RxCapture.run from host memory"""
    S, P = a.links, info.Nofdm * 4
    frame = (info.Nsymb + info.preamble_nsymb) * P
    slot = frame + a.gap_hops * P
    carrier = carrier_of(info)
    rng = np.random.default_rng(a.seed)
    off = rng.integers(0, slot, S)
    cap = RxCapture(rx, S, carrier)
    ch = hf_channel_preset(a.channel)
    R = min(a.max_hops or 16, slot // P)
    store = np.zeros((S, 2, frame))
    nxt = np.zeros(S, np.int64)
    cols = np.arange(R * P)

    def one_round(h0, nh):
        pos, n = h0 * P, nh * P
        need = [(s, int(nxt[s])) for s in range(S) if off[s] + nxt[s] * slot < pos + n]
        if need:
            audio = rx.transmit_byte(rng.integers(0, 256, (len(need), info.payload_stride)).astype(np.uint8), carrier, output_power_watt=a.power)
            for (s, j), fr in zip(need, audio):
                store[s, j & 1] = fr
                nxt[s] += 1
        u = pos + cols[None, :n] - off[:, None]
        j, w = np.floor_divide(u, slot), np.mod(u, slot)
        x = np.where((u >= 0) & (w < frame), store[np.arange(S)[:, None], j & 1, np.minimum(w, frame - 1)], 0.0)
        y = rx.hf_channel_apply(x, ch, seed=a.seed, realisation0=0, t0=pos)
        return len(cap.run(y))

    one_round(0, R)
    t = time.perf_counter()
    done, decoded = R, 0
    while done < R + hops:
        nh = min(R, R + hops - done)
        decoded += one_round(done, nh)
        done += nh
    wall = time.perf_counter() - t
    cap.close()
    return decoded, wall


def stream_bench(rx, a, info):
    import torch
    S, n = a.links, (a.max_hops or 16) * info.Nofdm * 4
    ch = hf_channel_preset(a.channel)
    st = HfStream(rx, S, ch, a.seed)
    x = torch.randn((S, n), dtype=torch.float64, device="cuda")
    y = torch.empty_like(x)
    amp = None if a.no_noise else np.full(S, 0.1)
    s = torch.cuda.current_stream()
    for _ in range(3):
        st.apply(x, amp, out=y, stream=s.cuda_stream)
    s.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(a.iters):
        st.apply(x, amp, out=y, stream=s.cuda_stream)
    e1.record(s)
    e1.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    dmax = max(round(ch.delay_ms[k] * FS / 1000.0) for k in range(ch.n_paths))
    tiles = -(-n // TILE)
    f = 3.0 * HILBERT_ODD * (TILE + dmax) * tiles / n                 # Hilbert FIR on every tile and its delay halo (a last partial tile costs a whole one)
    for k in range(ch.n_paths):
        f += (32 if ch.spread_hz[k] > 0 else 1) * (8.0 + 6.0 / 4.0) + 10.0
    sps = S * n / (ms * 1e-3)
    print(json.dumps({"stream_bench": True, "noise": not a.no_noise, "channel": a.channel, "links": S, "chunk_samples": n, "ms_per_chunk": round(ms, 4), "samples_per_s": sps,
                      "model_flop_per_sample": f, "fp64_fraction": f * sps / FP64_VECTOR_PEAK,
                      "history_read_bytes_per_sample": 8.0 * tiles * (2 * HILBERT_HALF + dmax) / n, "link_seconds_per_s": sps / FS}))
    st.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cfg", type=int, default=8)
    ap.add_argument("--links", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--channel", default="awgn", choices=["awgn", "good", "moderate", "poor", "flutter"])
    ap.add_argument("--esn0", default="10")
    ap.add_argument("--gap-hops", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-hops", type=int, default=0)
    ap.add_argument("--max-iters", type=int, default=50)
    ap.add_argument("--max-batch", type=int, default=0, help="receive_byte windows per call (0: the number of links)")
    ap.add_argument("--power", type=float, default=1.0, help="output_power_watt (1: Es/N0 is the signal's own, BER_PLOT_passband's convention)")
    ap.add_argument("--ladder", default="", help="estimator ladder, e.g. 21x21,5x21 (carriers x symbols) or 21x21,wiener (include/mercury_estimator.h) or bank:tau=-333/333|-333/2333 (include/mercury_wiener_bank.h)")
    ap.add_argument("--demapper", default="maxlog", type=_demapper,
                    help="csi: LLRs weighted by |H|^2 per cell; nmap[:band=2,smooth=1]: those divided by a noise factor per carrier and per symbol (include/mercury_demapper.h)")
    ap.add_argument("--cfo", default="off", choices=["off", "pilots"], help="pilots: every frame's grid turned back by the phase step its own pilots measure (include/mercury_cfo.h)")
    ap.add_argument("--blanker", default="off", type=_blanker,
                    help="median[:thr=24,guard=4,share=0.125]: every frame through the median-gated impulse blanker ahead of the front-end (include/mercury_blanker.h)")
    ap.add_argument("--excisor", default="off", type=_excisor,
                    help="welch[:thr=12,guard=1,bins=16]: every capture window through the carrier excisor ahead of the synchroniser (include/ext/mercury_excisor.h)")
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--compare", action="store_true", help="simulator and baseline alternating, --repeats times each")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--stream-bench", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-noise", action="store_true", help="--stream-bench without the noise draws")
    a = ap.parse_args()
    p, info = plan(a)
    if a.dry_run:
        print(json.dumps(p))
        return
    pts, esn0 = ladder(a.esn0, a.links)
    rx = RxPhy(a.cfg, max_iters=a.max_iters, max_batch=a.max_batch or a.links)
    rx.set_demapper(a.demapper)
    rx.set_cfo(a.cfo)
    rx.set_blanker(a.blanker)
    rx.set_excisor(a.excisor)
    if a.stream_bench:
        stream_bench(rx, a, info)
        rx.close()
        return
    hops = p["hops"]
    sim_seconds = a.links * hops * p["symbol_period"] / FS
    rates = {"simulator": [], "baseline": []}
    for rep in range(a.repeats):
        for which in (["simulator", "baseline"] if a.compare else ["baseline"] if a.baseline else ["simulator"]):
            if which == "baseline":
                decoded, wall = run_baseline(rx, a, info, hops)
                print(json.dumps({"baseline": True, "repeat": rep, "decoded_events": decoded, "wall_s": wall, "link_seconds_per_s": sim_seconds / wall}))
            else:
                c, wall = run_sim(rx, a, info, esn0, hops)
                for e in pts:
                    m = esn0 == e
                    d = int(c["delivered"][m].sum())
                    print(json.dumps({"esn0_db": e, "repeat": rep, "links": int(m.sum()), "sent": int(c["frames_sent"][m].sum()), "delivered": d,
                                      "duplicates": int(c["duplicates"][m].sum()), "false_decodes": int(c["false_decodes"][m].sum()),
                                      "mean_iterations": float(c["iterations_sum"][m].sum()) / d if d else None,
                                      "delivered_share": d / max(1, int(c["frames_sent"][m].sum()))}))
            rates[which].append(sim_seconds / wall)
    out = {"cfg": a.cfg, "links": a.links, "channel": a.channel, "gap_hops": a.gap_hops, "simulated_seconds_per_link": hops * p["symbol_period"] / FS,
           "max_iters": a.max_iters, "ladder": a.ladder, "demapper": a.demapper, "cfo": a.cfo, "blanker": a.blanker, "excisor": a.excisor}
    if a.ladder:
        by, frames = rx.ladder_counters()
        out["decoded_by_rung"], out["ladder_frames"] = [int(v) for v in by], frames
    for which, r in rates.items():
        if r:
            out[which + "_link_seconds_per_s"] = r
    if rates["simulator"] and rates["baseline"]:
        out["ratio"] = float(np.mean(rates["simulator"]) / np.mean(rates["baseline"]))
    print(json.dumps(out))
    rx.close()


if __name__ == "__main__":
    main()

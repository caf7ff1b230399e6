"""What the tests of a Wiener rung's bank of designs (include/mercury_wiener_bank.h) share: a numpy restatement of the rule written from the
header (pair lists, the four sums, default thresholds, the two tests, the choice), the three-design bank and the four frame sets the
feature was sized on, batches that mix frames of different delay spread, and the CPU decode counts of the bank and of each design alone."""
import functools

import numpy as np

import wiener_ref as W
from oraclelib import Oracle, noise_amp_for

# narrow, mid, wide (the default interval): delay bounds in us
INTERVALS = [(-333.33, 333.33), (-333.33, 1000.0), (-333.33, 2333.33)]
# (cfg, Es/N0 dB, second path in samples, frames, design SNR dB) of wiener_ref.two_path_delay
SETS = [(8, 0.0, 0, 32, 0.0), (8, 3.0, 6, 16, 5.0), (8, 3.0, 12, 16, 5.0), (13, 15.0, 24, 24, 5.0)]


def bank(snr_db=0.0, rho=None, intervals=INTERVALS):
    """the bank as mercury_amd takes it: [(design dict, rho_min or None), ...]"""
    rho = list(rho or []) + [None] * len(intervals)
    return [(W.design(tau_min_us=lo, tau_max_us=hi, snr_db=snr_db), rho[i]) for i, (lo, hi) in enumerate(intervals)]


def np_pairs(orc):
    """-> (s, 1-pairs [n1, 2], 2-pairs [n2, 2]) as pilot indices (row-major pilot order), from the geometry alone"""
    Nc, Ns = orc.Nc, orc.Nsymb
    types = orc.frame_types().reshape(Ns, Nc) != 0
    index = np.cumsum(types.ravel()).reshape(Ns, Nc) - 1
    rows = []
    for i in range(Ns):
        cars = np.flatnonzero(types[i])
        rows.append((index[i, cars], W.carrier_bin(cars, Nc)))
    s = min(int(np.diff(k).min()) for _, k in rows if k.size > 1)
    one = [(p[j], p[j + 1]) for p, k in rows for j in range(k.size - 1) if k[j + 1] - k[j] == s]
    two = [(p[j], p[j + 2]) for p, k in rows for j in range(k.size - 2) if k[j + 2] - k[j] == 2 * s]
    return s, np.array(one, np.int64), np.array(two, np.int64)


def np_thresholds(entries, s):
    """rho_min as applied, for all entries but the last"""
    def g(x):
        return float(np.sinc(x)) if x < 1 else 0.0
    Wd = [(d["tau_max_us"] - d["tau_min_us"]) * 0.012 for d, _ in entries]
    m = [g(2 * s * w / 256.0) / g(s * w / 256.0) if g(s * w / 256.0) > 0 else 0.0 for w in Wd]
    return [(m[d] + m[d + 1]) / 2.0 if entries[d][1] is None else float(entries[d][1]) for d in range(len(entries) - 1)]


def np_select(orc, grid, entries):
    """the rule on one frame grid -> dict(design, corr [4], n1, n2, rho, margin: the smallest relative distance of a decisive comparison
    from equality - how far the frame is from the other choice)"""
    Nc, Ns = orc.Nc, orc.Nsymb
    types = orc.frame_types().ravel() != 0
    g, sign = np.asarray(grid, np.complex128).ravel()[types], np.sign(orc.pilot_seq().real)
    yr, yi = g.real * sign, g.imag * sign                                  # per component: exact, and an Inf stays an Inf
    pilot_sym = np.flatnonzero(types) // Nc
    s, one, two = np_pairs(orc)
    n1, n2 = len(one), len(two)

    def serial(v):
        return float(np.cumsum(np.concatenate([[0.0], v]))[-1])            # one term after the other from +0.0

    def corr(pairs):
        """the header's sums: a pair's term from its four products, per symbol in ascending a, then the symbols' sums in ascending symbols"""
        a, b = pairs[:, 0], pairs[:, 1]
        tr, ti = (yr[a] * yr[b]) + (yi[a] * yi[b]), (yr[a] * yi[b]) - (yi[a] * yr[b])
        sym = pilot_sym[a]
        return (serial([serial(tr[sym == i]) for i in range(Ns)]), serial([serial(ti[sym == i]) for i in range(Ns)]))

    (R1r, R1i), (R2r, R2i) = corr(one), corr(two)
    R1, R2 = complex(R1r, R1i), complex(R2r, R2i)
    # the header's sums of squares, not abs() ** 2: hypot(Inf, NaN) is Inf, and a sum with a NaN component must fail every comparison
    q2 = (R2r * R2r + R2i * R2i) * (float(n1) * float(n1))
    q1 = (R1r * R1r + R1i * R1i) * (float(n2) * float(n2))
    rho_min = np_thresholds(entries, s)
    choice, margin = len(entries) - 1, np.inf
    for d in range(len(entries) - 2, -1, -1):
        design = entries[d][0]
        Wd = (design["tau_max_us"] - design["tau_min_us"]) * 0.012
        ok = q2 >= rho_min[d] ** 2 * q1
        if np.isfinite(q1) and q1 > 0:
            margin = min(margin, abs(q2 - rho_min[d] ** 2 * q1) / q1)
        if s * Wd < 64:
            tau0, tau1 = design["tau_min_us"] * 12000.0 / 1e6, design["tau_max_us"] * 12000.0 / 1e6
            phi = -2.0 * np.pi * s * (tau0 + tau1) / 512.0
            z = complex(R1r * np.cos(phi) + R1i * np.sin(phi), R1i * np.cos(phi) - R1r * np.sin(phi))
            t = np.tan(np.pi * s * Wd / 256.0)
            ok = ok and z.real > 0 and abs(z.imag) <= t * z.real
            if np.isfinite(abs(z)) and abs(z) > 0:
                margin = min(margin, abs(z.real) / abs(z), abs(abs(z.imag) - t * z.real) / abs(z))
        if ok:
            choice = d
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = (np.float64(abs(R2)) / n2) / (np.float64(abs(R1)) / n1)
    return dict(design=choice, corr=np.array([R1r, R1i, R2r, R2i]), n1=n1, n2=n2, rho=float(rho), margin=float(margin))


@functools.lru_cache(maxsize=None)
def mixed_batch(cfg, esn0, explicit=()):
    """F = 6 frames that want different designs: two each with no second path, a second path 12 and 24 samples late, made the way
    wiener_ref.two_path_delay makes its frames (generator seed 5, phases and noise from default_rng(11)).
    -> dict(orc, bb [6, samples], grid: the oracle's grid after the AGC per frame)"""
    orc = Oracle(cfg, 50, explicit=dict(explicit))
    rng = np.random.default_rng(11)
    amp = 16.0 * noise_amp_for(esn0)
    bb = []
    for f, delay in enumerate((0, 0, 12, 12, 24, 24)):
        x, _ = orc.gen_frame(5, f, 0.0, 0)
        ph = np.exp(1j * rng.uniform(0, 2 * np.pi, 2))
        y = ph[0] * x
        if delay:
            y[delay:] += ph[1] * x[:-delay]
            y /= np.sqrt(2.0)
        y += amp * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
        bb.append(y)
    bb = np.stack(bb)
    return dict(orc=orc, bb=bb, grid=[orc.rx(b)["grid"] for b in bb])


@functools.lru_cache(maxsize=None)
def bank_counts(cfg, esn0, delay, frames, snr_db):
    """One of SETS through the library's twins: per frame the bank's choice (mgpu_host_wiener_select) and, for each design of the
    three-design bank alone, whether host_wiener_estimate -> interpolate_cols -> host_demap_csi -> the oracle's decoder gives the frame's
    bits. The bank's verdict on a frame is its chosen design's: the estimate is that design's bit for bit.
    -> dict(choice [frames], ok [3, frames] bool, rho [frames])"""
    from mercury_amd import host_wiener_estimate, host_wiener_select, wiener_sounding
    t = W.two_path_delay(cfg, esn0, delay, frames)
    orc = t["orc"]
    entries = bank(snr_db)
    s = np_pairs(orc)[0]
    choice, rho, ok = [], [], np.zeros((len(entries), frames), bool)
    for f in range(frames):
        grid = t["ref"][f]["grid"]
        sel = host_wiener_select(cfg, grid, entries)
        choice.append(sel["design"])
        rho.append(float(wiener_sounding(sel["corr"], sel["n1"], sel["n2"], s)[0]))
        for d, (design, _) in enumerate(entries):
            Hp = host_wiener_estimate(cfg, grid, design)
            ok[d, f] = np.array_equal(W.decode_with(orc, grid, W.interpolate_cols(orc, Hp))[2], t["bits"][f])
    return dict(choice=np.array(choice), ok=ok, rho=np.array(rho))

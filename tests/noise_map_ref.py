"""What the tests of the noise-map demapper (include/mercury_demapper.h MGPU_DEMAP_NMAP) share: a numpy restatement of its rule on the CPU
oracle's stage outputs, and the disturbed frames - a tone from another station inside the channel, a static crash over one OFDM symbol -
on which one variance per frame loses the frames and a variance per carrier and per symbol decodes them. The frames are built on the host
by one fixed recipe so that the CPU and the GPU tests see the same samples."""
import functools

import numpy as np

from demapper_csi_ref import CASES, DY5, full_estimate, llr_src, llr_tol, np_cdiv, np_maxlog, np_sigma2, same_bits, sym_src, tail  # noqa: F401  (shared with the tests)
from oraclelib import Oracle, noise_amp_for

LS_CASES = [(cfg, explicit) for cfg, explicit in CASES if cfg != 16]          # 0, 8, 11, 13 and (8, Dy 5 / Nsymb 20): the zero-forcing mode is refused
INF = float("inf")


def _serial(terms):
    """the sum of terms one after the other from +0.0 (np.cumsum adds serially), 0.0 for none"""
    with np.errstate(all="ignore"):
        return float(np.cumsum(np.asarray(terms, np.float64))[-1]) if len(terms) else 0.0


def _banded(v, n, sigma2, band):
    with np.errstate(all="ignore"):
        f = np.float64(v) / np.float64(sigma2)
        usable = sigma2 != 0 and np.isfinite(sigma2)
        return float(f) if (usable and n > 0 and (f > band or f * band < 1)) else 1.0


def np_noise_map(orc, grid, H, band=2.0, smooth=1):
    """the map in numpy: (sigma2, fc [Nc], fs [Nsymb], raw fc, raw fs) - the factors after the dead band and before it"""
    Nc, Ns = orc.Nc, orc.Nsymb
    pilots = np.flatnonzero(orc.frame_types() != 0)
    r, sigma2 = np_sigma2(orc, grid, H)
    car, sym = pilots % Nc, pilots // Nc
    S = [_serial(r[car == c]) for c in range(Nc)]                    # pilot order is ascending symbols within a carrier
    n = [int((car == c).sum()) for c in range(Nc)]
    fc, fs, raw_c, raw_s = np.ones(Nc), np.ones(Ns), np.ones(Nc), np.ones(Ns)
    with np.errstate(all="ignore"):
        for c in range(Nc):
            lo, hi = max(c - smooth, 0), min(c + smooth, Nc - 1)
            cnt = sum(n[lo: hi + 1])
            V = np.float64(_serial(S[lo: hi + 1])) / np.float64(cnt)
            raw_c[c] = V / np.float64(sigma2)
            fc[c] = _banded(V, cnt, sigma2, band)
        for s in range(Ns):
            terms = r[sym == s]                                      # ... and ascending carriers within a symbol
            U = np.float64(_serial(terms)) / np.float64(len(terms))
            raw_s[s] = U / np.float64(sigma2)
            fs[s] = _banded(U, len(terms), sigma2, band)
    return sigma2, fc, fs, raw_c, raw_s


def np_demap_nmap(orc, grid, H, band=2.0, smooth=1):
    """the rule in numpy: (llr_demod float32 [nBits], sigma2, fc, fs). Exact, as np_demap_csi: its division and minima, the scale formed as
    the twin forms it, (a[c] * b[s]) * wf with a = 1 / float32(sigma2 * fc) and b = 1 / float32(fs) - so it equals mgpu_host_demap_nmap bit
    for bit, NaN where it gives NaN; sigma2 and the factors are the same serial sums."""
    grid, H = np.asarray(grid, np.complex128).ravel(), np.asarray(H, np.complex128).ravel()
    sigma2, fc, fs, _, _ = np_noise_map(orc, grid, H, band, smooth)
    src = sym_src(orc)
    hs = H[src]
    er, ei = np_cdiv(grid[src], hs)
    with np.errstate(all="ignore"):
        a = np.float32(1.0) / (np.float64(sigma2) * fc).astype(np.float32)
        b = np.float32(1.0) / fs.astype(np.float32)
        wf = (hs.real * hs.real + hs.imag * hs.imag).astype(np.float32)
        scale = (a[src % orc.Nc] * b[src // orc.Nc]) * wf
    return np_maxlog(orc, er, ei, scale), sigma2, fc, fs


def _key(explicit):
    return tuple(sorted((explicit or {}).items()))


@functools.lru_cache(maxsize=None)
def _disturbed(cfg, explicit_key, esn0, tone_db, burst_db, frames, delay=0):
    explicit = dict(explicit_key)
    orc = Oracle(cfg, 50, explicit=dict(explicit))
    rng = np.random.default_rng(11)
    amp = 16.0 * noise_amp_for(esn0)
    bb, bits = [], []
    for f in range(frames):
        x, _ = orc.gen_frame(5, f, 0.0, 0)
        n = x.size
        bits.append(orc.rx(x)["bits"].copy())
        P = float(np.mean(np.abs(x) ** 2))
        if delay:                                                    # two equal static paths, as demapper_csi_ref.two_path: the phases are drawn first
            ph = np.exp(1j * rng.uniform(0, 2 * np.pi, 2))
            clean = x
            x = ph[0] * clean
            x[delay:] += ph[1] * clean[:-delay]
            x /= np.sqrt(2.0)
        noise_re = rng.standard_normal(n)
        y = x + amp * (noise_re + 1j * rng.standard_normal(n))
        if tone_db is not None:
            fb = rng.uniform(-24, 24)
            phase = rng.uniform(0, 6.28)
            y = y + np.sqrt(P * 10.0 ** (tone_db / 10.0)) * np.exp(1j * (2 * np.pi * fb * np.arange(n) / 256.0 + phase))
        if burst_db is not None:
            start = int(rng.integers(0, orc.Nsymb - 1)) * 272
            start += int(rng.integers(0, 272))
            burst_re = rng.standard_normal(272)
            y[start: start + 272] += np.sqrt(P * 10.0 ** (burst_db / 10.0) / 2.0) * (burst_re + 1j * rng.standard_normal(272))
        bb.append(y)
    bb = np.stack(bb)
    ref = [orc.rx(bb[f]) for f in range(frames)]
    plain_ok = np.array([np.array_equal(ref[f]["bits"], bits[f]) for f in range(frames)])
    return dict(orc=orc, explicit=explicit or None, bb=bb, bits=bits, ref=ref, plain_ok=plain_ok)


def disturbed(cfg, explicit, esn0, tone_db=None, burst_db=None, frames=32, delay=0):
    """`frames` clean frames of the generator (seed 5, x = gen_frame(5, f, 0.0, 0), P = mean |x|^2) disturbed with default_rng(11), used
    frame after frame in this order: noise 16 * noise_amp_for(esn0) * (standard_normal(n) + 1j standard_normal(n)); the tone, if any:
    fb = uniform(-24, 24) bins of the 256-point FFT, phase = uniform(0, 6.28), sqrt(P 10^(dB/10)) exp(j (2 pi fb t / 256 + phase)) over all n
    samples; the burst, if any: start = integers(0, Nsymb - 1) * 272 + integers(0, 272), 272 samples of
    sqrt(P 10^(dB/10) / 2) (standard_normal + 1j standard_normal). delay (tools/noise_map_table.py alone): the clean frame through two equal
    static paths that many samples apart first, their phases drawn before the noise.
    -> dict(orc, explicit, bb, bits: each clean frame's message bits, ref: the oracle's rx of each disturbed frame, plain_ok)"""
    return _disturbed(cfg, _key(explicit), float(esn0), tone_db, burst_db, frames, delay)


@functools.lru_cache(maxsize=None)
def _twin_decode(cfg, explicit_key, esn0, tone_db, burst_db, frames, which, band, smooth, delay=0):
    from mercury_amd import host_demap_csi, host_demap_nmap
    explicit = dict(explicit_key) or None
    t = _disturbed(cfg, explicit_key, esn0, tone_db, burst_db, frames, delay)
    orc, src = t["orc"], llr_src(t["orc"])
    out = []
    for f in range(frames):
        grid, H = t["ref"][f]["grid"], full_estimate(orc, t["ref"][f])
        if which == "csi":
            llr = host_demap_csi(cfg, grid, H, explicit=explicit)[0]
        else:
            llr = host_demap_nmap(cfg, grid, H, band, smooth, explicit=explicit)[0]
        llr_ldpc = llr[src]
        bits, it = orc.ldpc_decode(llr_ldpc)
        out.append((llr_ldpc, bits, it))
    return out


def twin_decode(cfg, explicit, esn0, tone_db=None, burst_db=None, frames=32, which="nmap", band=2.0, smooth=1, delay=0):
    """the library's host twin (which: "csi" or "nmap") on the oracle's grid and full estimate of those frames, its LLRs through llr_src
    into the oracle's decoder: per frame (llr_ldpc, bits, iterations)"""
    return _twin_decode(cfg, _key(explicit), float(esn0), tone_db, burst_db, frames, which, float(band), int(smooth), delay)


def decoded_count(t, twin):
    return sum(int(np.array_equal(bits, t["bits"][f])) for f, (_, bits, _) in enumerate(twin))

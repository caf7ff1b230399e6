"""The carrier tuner's rule (include/ext/mercury_tuner.h) in NumPy and plain Python, written from the header and not from the C++: what
tests/test_tuner_host.py holds the host twin to, bit for bit. Every product, sum and difference below is one operation on float64
values, so each is rounded on its own, as the rule has it; the fused multiply-adds of stage 1 are the host libm's. The tap rows and the
phasor table are the channeliser's own (host_chan_tables), the transform is the scanner's statement (tests/scanner_ref.py). A plain
module: no test lives here.

Also the input the tuner's tests share: a small generator of Mercury-geometry OFDM audio, put into the IQ by host_synth_process so that
the offset a frame truly lies at is exact."""
import ctypes as C
import ctypes.util
import functools
import math

import numpy as np

import mercury_amd as M
import scanner_ref

NFFT, SYM, GI, SPACING = 256, 272, 16, 46.875
CARRIERS = [c for c in range(-25, 26) if c != 0]

try:
    fma = math.fma                                  # Python 3.13 on: the C library's fma
except AttributeError:
    _libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    _libm.fma.restype, _libm.fma.argtypes = C.c_double, [C.c_double] * 3
    fma = _libm.fma


def lround(x):
    """C's lround: to the nearest integer, halves away from zero"""
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def accepted(D, a_c, offset, sideband):
    """whether the channeliser accepts the channel: its band stays inside (-R/2, R/2)"""
    R = 48000 * D
    lo, hi = (offset - 2 * a_c, offset) if sideband else (offset, offset + 2 * a_c)
    return 2 * lo > -R and 2 * hi < R


def mix(xr, xi, g, D, Mn):
    """stage 1: z[m] = the channeliser's accumulator pair at output 4 m, zeros before the block's start"""
    T = len(g)
    gr, gi = g.real.tolist(), g.imag.tolist()
    ngi = [-v for v in gi]
    xr, xi = [0.0] * (T - 1) + xr.tolist(), [0.0] * (T - 1) + xi.tolist()
    zr, zi = np.zeros(Mn), np.zeros(Mn)
    for m in range(Mn):
        at = 4 * m * D + T - 1
        re = im = 0.0
        for k in range(T):
            vr, vi = xr[at - k], xi[at - k]
            re = fma(gr[k], vr, re)
            re = fma(ngi[k], vi, re)
            im = fma(gr[k], vi, im)
            im = fma(gi[k], vr, im)
        zr[m], zi[m] = re, im
    return zr, zi


def fold(zr, zi, J):
    """stage 2 -> Gr, Gi, E [272]"""
    n = SYM * J + GI - 1                            # the lag products that are read: m < 272 J + 15
    ar, ai, br, bi = zr[:n], zi[:n], zr[NFFT: NFFT + n], zi[NFFT: NFFT + n]
    p = (ar * br + ai * bi, ai * br - ar * bi, 0.5 * ((ar * ar + ai * ai) + (br * br + bi * bi)))
    first = SYM * np.arange(J)[:, None] + np.arange(SYM)[None, :]
    out = []
    for v in p:
        inner = np.zeros((J, SYM))
        for i in range(GI):
            inner = inner + v[first + i]
        acc = np.zeros(SYM)
        for j in range(J):
            acc = acc + inner[j]
        out.append(acc)
    return out


def comb(zr, zi, W, J, phase, index):
    """stage 3 -> Q [256]"""
    Q = np.zeros(NFFT)
    for j in range(J):
        m = SYM * j + phase + GI // 2 + np.arange(NFFT)
        w = W[(index * m) % 48000]
        ar, ai = scanner_ref.transform(zr[m] * w.real + zi[m] * w.imag, zi[m] * w.real - zr[m] * w.imag, 8)
        Q = Q + (ar * ar + ai * ai)
    return Q


def process(iq, D, channels, symbols=32, search=8, taps=None, audio_centre_hz=1472, carrier_hz=M.TUNE_DEFAULT_CARRIER_HZ,
            min_metric=M.TUNE_DEFAULT_MIN_METRIC):
    """one block -> (reports TUNE_REPORT_DTYPE [S], G complex128 [S, 272], E [S, 272], Q [S, 256])"""
    J, K, a_c, S = symbols, search, audio_centre_hz, len(channels)
    Mn = SYM * (J + 1)
    xr, xi = scanner_ref.widen(iq)
    assert xr.size == 4 * D * Mn
    reports = np.zeros(S, M.TUNE_REPORT_DTYPE)
    G, E, Q = np.zeros((S, SYM), np.complex128), np.zeros((S, SYM)), np.zeros((S, NFFT))
    for s, (offset, sideband, gain) in enumerate(channels):
        sigma = -1 if sideband else 1
        F = offset + sigma * a_c
        g, W = M.host_chan_tables(D, (offset, sideband, gain), taps, a_c, want_phasor=True)
        zr, zi = mix(xr, xi, g, D, Mn)
        Gr, Gi, Es = fold(zr, zi, J)
        G[s], E[s] = Gr + 1j * Gi, Es
        r = reports[s]
        r["offset_hz"] = offset
        phase = turn = 0
        bad = not (np.isfinite(Gr).all() and np.isfinite(Gi).all() and np.isfinite(Es).all())
        if not bad:
            mag = Gr * Gr + Gi * Gi
            phase = int(np.argmax(mag))
            r["phase"] = phase
            r["metric"] = np.sqrt(mag[phase]) / Es[phase] if Es[phase] > 0.0 else 0.0
            raw = (-math.atan2(float(Gi[phase]), float(Gr[phase])) * 12000.0) / (2.0 * math.pi * 256.0)
            frac = raw - float((8 * F) % 375) / 8.0
            if frac < -SPACING / 2:
                frac = frac + SPACING
            r["frac_hz"] = frac
            turn = lround(frac)
        Q[s] = comb(zr, zi, W, J, phase, (4 * (F + turn)) % 48000)
        if bad or not np.isfinite(Q[s]).all():
            reports[s] = np.zeros((), M.TUNE_REPORT_DTYPE)
            reports[s]["offset_hz"], reports[s]["nonfinite"] = offset, 1
            continue
        q = Q[s].tolist()
        score = []
        for d in range(-K, K + 1):
            acc = 0.0
            for c in CARRIERS:
                acc = acc + q[(c + d) % NFFT]
            score.append(acc)
        best = 0
        for i in range(1, 2 * K + 1):
            if score[i] > score[best]:
                best = i
        others = [v for i, v in enumerate(score) if i != best]
        second = max(others) if others else 0.0
        frac = float(r["frac_hz"])
        r["shift"] = best - K
        r["contrast"] = score[best] / second if second > 0.0 else 0.0
        delta = float(best - K) * SPACING + ((frac - float(turn)) + float(turn))
        r["delta_hz"] = delta
        moved, lead = float(offset) + delta, carrier_hz - float(a_c)
        refined = lround(moved + lead if sideband else moved - lead)
        r["valid"] = int(float(r["metric"]) >= min_metric and accepted(D, a_c, refined, sideband))
        if r["valid"]:
            r["offset_hz"] = refined
    return reports, G, E, Q


def same(got, want):
    """(reports, G, E, Q) of two statements, bit for bit"""
    return all(np.asarray(a).shape == np.asarray(b).shape and np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, want))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def ofdm_audio(rng, n_symbols, n, start, carrier_hz=M.TUNE_DEFAULT_CARRIER_HZ):
    """n samples of 48 kHz audio, silent but for one frame of n_symbols Mercury-geometry OFDM symbols from sample `start`: random QPSK
    on the 50 carriers -25..-1, 1..25 (DC empty), IFFT 256 and a prefix of 16 at 12 kHz, here made at four times the rate directly
    (IFFT 1024 of the same 50 bins, prefix 64: the same symbols, interpolated exactly), on a carrier of carrier_hz"""
    assert 0 <= start and start + n_symbols * 4 * SYM <= n
    spec = np.zeros((n_symbols, 4 * NFFT), np.complex128)
    spec[:, CARRIERS] = (rng.integers(0, 2, (n_symbols, 50)) * 2 - 1 + 1j * (rng.integers(0, 2, (n_symbols, 50)) * 2 - 1)) / np.sqrt(2.0)
    useful = np.fft.ifft(spec, axis=1) * (4 * NFFT) / np.sqrt(50.0)            # unit power
    base = np.concatenate([useful[:, -4 * GI:], useful], axis=1).reshape(-1)
    t = start + np.arange(base.size)
    audio = np.zeros(n)
    audio[t] = np.sqrt(2.0) * (base * np.exp(2j * np.pi * carrier_hz * t / 48000.0)).real
    return audio


def block(seed, D, channels, symbols=32, n_symbols=None, noise_db=None, fmt="cf64", taps=None, audio_centre_hz=1472,
          carrier_hz=M.TUNE_DEFAULT_CARRIER_HZ):
    """One tuner block, tune_samples(D, symbols) IQ samples: one frame per channel of `channels` (the offsets the stations truly lie at),
    each of n_symbols symbols (None: drawn from 12..40, cut to what the block holds) at a random start in silence, synthesised by
    host_synth_process, plus white noise over the whole span whose power per IQ sample is noise_db relative to the mean power of the
    frames' samples (None: none). fmt 'cs16' scales the block to a peak of 0.5 first."""
    rng = np.random.default_rng(seed)
    n = 4 * SYM * (symbols + 1)
    audio = np.zeros((len(channels), n))
    for s in range(len(channels)):
        room = n // (4 * SYM) - 1
        count = min(int(rng.integers(12, 41)) if n_symbols is None else n_symbols, room)
        start = int(rng.integers(0, n - count * 4 * SYM - 600))                 # the synthesiser's and the prototype's delay stay inside
        audio[s] = ofdm_audio(rng, count, n, start, carrier_hz)
    iq = M.host_synth_process(D, channels, audio, taps=taps, audio_centre_hz=audio_centre_hz)
    if noise_db is not None:
        power = np.mean(np.abs(iq[np.abs(iq) > 0]) ** 2) if np.any(iq) else 1.0
        amp = np.sqrt(power * 10 ** (noise_db / 10.0) / 2.0)
        iq = iq + amp * (rng.standard_normal(iq.size) + 1j * rng.standard_normal(iq.size))
    return to_format(iq, fmt)


def to_format(iq, fmt):
    if fmt == "cf64":
        return iq
    if fmt == "cf32":
        return iq.astype(np.complex64)
    scaled = iq * (0.5 / max(np.abs(iq.real).max(), np.abs(iq.imag).max(), 1e-300))
    return np.stack([np.round(scaled.real * 32768.0), np.round(scaled.imag * 32768.0)], 1).astype(np.int16)


@functools.lru_cache(maxsize=None)
def noise_block(seed, D=1, symbols=32):
    rng = np.random.default_rng(seed)
    n = M.tune_samples(D, symbols)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    x.setflags(write=False)
    return x

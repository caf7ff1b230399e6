"""What the resampler's tests share (include/ext/mercury_resampler.h): a numpy restatement of the rule with unfused products and sums,
the tabled ratios, the prototype's frequency response, band-limited test signals that can be synthesised at any rate and delay, and the
tests' own FFT resampler (spectrum truncation / zero padding), which shares nothing with the stage."""
import math

import numpy as np

# fin -> fout of the rule's table, with L / M
TABLED = [(44100, 48000, 160, 147), (22050, 48000, 320, 147), (11025, 48000, 640, 147), (8000, 48000, 6, 1), (12000, 48000, 4, 1),
          (16000, 48000, 3, 1), (32000, 48000, 3, 2), (96000, 48000, 1, 2), (192000, 48000, 1, 4), (2048000, 1536000, 3, 4),
          (250000, 240000, 24, 25), (48000, 48000, 1, 1)]


def ratio(fin, fout):
    g = math.gcd(fin, fout)
    return fout // g, fin // g


def default_tp(L, M):
    """32 max(1, ceil(M / L)), and at least the even tp at which 1.5 transition widths (half the transition and a stop-band one width
    wide) fit between the default cutoff and the design rate's Nyquist frequency: in units of fin the room is L / 2 - 0.45 min(1, L / M)
    and a width is (60 - 7.95) / (14.36 tp). Of all ratios the rule accepts only 1/1 is lengthened (to 110)."""
    fit = math.ceil(1.5 * (60 - 7.95) / (14.36 * (0.5 * L - 0.45 * min(1.0, L / M))))
    return max(32 * max(1, -(-M // L)), fit + (fit & 1))


def count(L, M, m0, n_in):
    """outputs of a call: ceil((m0 + n_in) L / M) - ceil(m0 L / M), in Python integers"""
    return -(-(m0 + n_in) * L // M) - -(-m0 * L // M)


def model(h, L, M, x, m0=0):
    """The rule on one real stream x (float64 [n_in]) seeked to input position m0, with numpy's products and sums (no fused multiply-add,
    no fixed order) -> (y, bound): the outputs and sum |h| |x| of each, which scales the tests' tolerance."""
    h = np.asarray(h, np.float64)
    tp = (h.size - 1) // L
    assert h.size == tp * L + 1
    n0 = -(-m0 * L // M)
    n = count(L, M, m0, x.size)
    xp = np.concatenate([np.zeros(tp + 1), np.asarray(x, np.float64)])     # xp[k] = x[k - tp - 1]
    y, bound = np.zeros(n), np.zeros(n)
    for i in range(n):
        q = (n0 + i) * M
        b, rho = q // L - m0, q % L
        taps = h[rho::L]                                                    # h[rho + j L], j = 0 .. tp - 1 (and tp for rho = 0)
        seg = xp[b + tp + 1 - np.arange(taps.size)]                         # x[b - j]
        y[i] = np.dot(taps, seg)
        bound[i] = np.dot(np.abs(taps), np.abs(seg))
    return y, bound


def response(h, L, fin, nfft=1 << 19):
    """(frequencies in Hz, |H| / L) of the prototype at rate fin * L, from an FFT of the taps"""
    H = np.abs(np.fft.rfft(h, nfft)) / L
    return np.arange(H.size) * (float(fin) * L / nfft), H


def kaiser_transition_hz(fin, tp, atten_db=60.0):
    """the Kaiser design formula's transition width for tp * L taps at rate fin * L: (A - 7.95) / (14.36 N) of the rate"""
    return (atten_db - 7.95) * fin / (14.36 * tp)


TONES_HZ =(300.0, 611.0, 1033.0, 1472.0, 1999.0, 2377.0, 2700.0)


def tones(rate, n, delay=0.0, seed=5):
    """a sum of tones in 300 .. 2700 Hz at `rate`: sample k is the signal at time (k - delay) / rate (delay in samples, fractional: a
    phase ramp per tone)"""
    rng = np.random.default_rng(seed)
    amp, ph = rng.uniform(0.5, 1.0, len(TONES_HZ)), rng.uniform(0, 2 * np.pi, len(TONES_HZ))
    t = (np.arange(n) - delay) / float(rate)
    return sum(a * np.cos(2 * np.pi * f * t + p) for a, f, p in zip(amp, TONES_HZ, ph)) / len(TONES_HZ)


def error_db(got, want):
    return 10 * np.log10(np.sum((got - want) ** 2) / np.sum(want ** 2))


def fft_resample(x, fin, fout):
    """x (last axis: n samples at fin, n * fout / fin an integer) at fout by truncating or zero-padding its spectrum: exact for a signal
    that is periodic in n and band-limited below both Nyquist rates"""
    n = x.shape[-1]
    assert (n * fout) % fin == 0
    m = n * fout // fin
    X = np.fft.rfft(x, axis=-1)
    Y = np.zeros(x.shape[:-1] + (m // 2 + 1,), np.complex128)
    k = min(X.shape[-1], Y.shape[-1])
    Y[..., :k] = X[..., :k]
    return np.fft.irfft(Y, m, axis=-1) * (m / n)


def fft_delay(x, d):
    """x (periodic in its length) delayed by a fractional d samples: a phase ramp on its spectrum"""
    n = x.shape[-1]
    return np.fft.irfft(np.fft.rfft(x, axis=-1) * np.exp(-2j * np.pi * np.arange(n // 2 + 1) * d / n), n, axis=-1)


def delayed(x, d):
    """x delayed by d >= 0 whole samples (last axis), same length"""
    out = np.zeros_like(x)
    out[..., d:] = x[..., : x.shape[-1] - d]
    return out

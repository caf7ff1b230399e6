"""Helpers of the wideband synthesiser's tests (include/ext/mercury_synth.h): the rule in its textbook form in numpy longdouble, its own
tables from the formulas, zero-stuffing and a direct convolution; the error bound that goes with it; the prototype's response.
Nothing here calls the library."""
import numpy as np

FS = 48000
AUDIO_CENTRE = 1472
LD = np.longdouble
CLD = np.clongdouble
TWO_PI = 2 * np.arctan2(LD(0), LD(-1))


def _cis(t, R):
    """exp(2 pi i t / R) for Python integers t in [0, R), in longdouble"""
    ang = TWO_PI * np.array(t, LD) / LD(R)
    return (np.cos(ang) + 1j * np.sin(ang)).astype(CLD)


def carrier(offset_hz, position, n):
    """e^(2 pi i offset (position + k) / 48000), k < n, the index reduced in Python integers"""
    return _cis([(int(offset_hz) * (int(position) + k)) % FS for k in range(n)], FS)


def kernel(h, D, offset_hz, sideband, audio_centre=AUDIO_CENTRE):
    """h[k] e^(2 pi i (offset k + sigma a_c (k - c)) / R): the band-pass centred on c, the carrier not delayed"""
    T = len(h)
    c, R = (T - 1) // 2, FS * D
    sig = -1 if sideband else 1
    return np.asarray(h, LD) * _cis([(int(offset_hz) * k + sig * audio_centre * (k - c)) % R for k in range(T)], R)


def outputs_to_check(n_in, D, T, limit=3e7, seed=0):
    """every output where the direct convolution is affordable (n_in D T <= limit); else the first and the last 2 D outputs (every phase,
    the shortest and the longest sums) and 150 more drawn at random"""
    M = n_in * D
    if M * T <= limit:
        return np.arange(M)
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([np.arange(min(2 * D, M)), np.arange(max(M - 2 * D, 0), M), rng.integers(0, M, 150)]))


def textbook(D, channels, audio, h, position=0, ms=None, audio_centre=AUDIO_CENTRE):
    """The definition: per channel, zero-stuff a_s[n] e^(2 pi i offset n / 48000) to rate 48000 D, convolve with kernel(), scale by
    G = 2 D gain, add the channels. Evaluated at the outputs `ms` (None: all) by the convolution sum itself, in longdouble.
    -> (IQ clongdouble [len(ms)], weight float64 [len(ms)]) with weight[m] = sum_s G_s sum_j |h[j D + r]| |a_s[n - j]|, what the error
    bound of the twin scales with."""
    audio = np.atleast_2d(np.asarray(audio, np.float64))
    S, n_in = audio.shape
    M, T = n_in * D, len(h)
    ms = np.arange(M) if ms is None else np.asarray(ms)
    iq = np.zeros(ms.size, CLD)
    weight = np.zeros(ms.size, LD)
    habs = np.abs(np.asarray(h, LD))
    for s, (off, sb, gain) in enumerate(channels):
        u = np.zeros(M, CLD)
        u[::D] = audio[s].astype(LD) * carrier(off, position, n_in)
        uabs = np.zeros(M, LD)
        uabs[::D] = np.abs(audio[s]).astype(LD)
        kern = kernel(h, D, off, sb, audio_centre)
        G = LD(2 * D) * LD(gain)
        for i, m in enumerate(ms):
            K = min(int(m), T - 1)                          # y[m] = sum_{k <= K} kern[k] u[m - k]
            seg = slice(int(m) - K, int(m) + 1)
            iq[i] += G * np.dot(kern[: K + 1][::-1], u[seg])
            weight[i] += abs(G) * np.dot(habs[: K + 1][::-1], uabs[seg])
    return iq, weight.astype(np.float64)


def tones(n, freqs, amps, phases):
    """a sum of tones at 48 kHz, float64 [n]"""
    t = np.arange(n) / float(FS)
    return sum(a * np.cos(2 * np.pi * f * t + p) for f, a, p in zip(freqs, amps, phases))


def response(h, D):
    """(f, |H(f)|) of the real taps h at rate 48000 D from 0 to the Nyquist frequency, on a grid of at most 48000 D / (8 T) Hz"""
    h = np.asarray(h, np.float64)
    nfft = 1 << int(np.ceil(np.log2(8 * h.size)))
    return np.fft.rfftfreq(nfft, 1.0 / (FS * D)), np.abs(np.fft.rfft(h, nfft))

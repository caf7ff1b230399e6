"""Helpers of the wideband channeliser's tests (include/mercury_channelizer.h): an independent numpy model of the rule, a numpy wideband
synthesiser, band-limited test audio and the error measure. Nothing here calls the library."""
import numpy as np

FS = 48000
AUDIO_CENTRE = 1472


def widen(iq):
    """the rule's x[m]: complex128 from complex64 / complex128 / int16 [..., 2] (/ 32768.0)"""
    x = np.asarray(iq)
    if x.dtype == np.int16:
        return (x[..., 0].astype(np.float64) / 32768.0 + 1j * (x[..., 1].astype(np.float64) / 32768.0)).ravel()
    return x.astype(np.complex128).ravel()


def tap_row(h, D, offset_hz, sideband, audio_centre=AUDIO_CENTRE):
    """g[k] = h[k] exp(2 pi i ((F (k - c)) mod R) / R) with the indices in Python integers"""
    T = len(h)
    c, R = (T - 1) // 2, FS * D
    F = int(offset_hz) + (-audio_centre if sideband else audio_centre)
    q = np.array([(F * (k - c)) % R for k in range(T)], np.float64)
    return np.asarray(h, np.float64) * np.exp(2j * np.pi * q / R)


def model(D, channels, iq, h, position=0, audio_centre=AUDIO_CENTRE):
    """the rule by np.convolve (another summation order than the twin's: agreement to rounding, not to the bit): float64 [S, n_in // D]"""
    x = widen(iq)
    T = len(h)
    L, N = (T - 1) // D // 2, x.size // D
    out = np.zeros((len(channels), N))
    for s, (off, sb, gain) in enumerate(channels):
        z = np.convolve(x, tap_row(h, D, off, sb, audio_centre))[: N * D: D]         # z[j] = sum_k g[k] x[j D - k]
        p = np.array([(int(off) * (int(position) + j - L)) % FS for j in range(N)], np.float64)
        out[s] = gain * np.real(z * np.exp(-2j * np.pi * p / FS))
    return out


def band_noise(rng, n, lo=300.0, hi=2644.0):
    """real noise of n samples at 48 kHz, band-limited to Mercury's audio band, unit rms"""
    X = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / FS)
    X[(f < lo) | (f > hi)] = 0
    a = np.fft.irfft(X, n)
    return a / np.sqrt(np.mean(a ** 2))


def synthesise(audio, D, offsets, sidebands=None, gains=None):
    """The wideband IQ, complex128 [n * D] at 48000 * D, of real 48 kHz audio [S, n] transmitted on single-sideband channels: 1. the analytic
    signal by FFT (its conjugate for a lower sideband), 2. interpolation by D by zero-padding the spectrum, 3. a shift by offset_hz,
    4. the sum over the channels. (Periodic in n: compare away from the ends.)"""
    audio = np.atleast_2d(np.asarray(audio, np.float64))
    S, n = audio.shape
    m = n * D
    t = np.arange(m) / float(FS * D)
    iq = np.zeros(m, np.complex128)
    for s in range(S):
        X = np.fft.fft(audio[s])
        A = np.zeros(n, np.complex128)
        A[0] = X[0]
        A[1: (n + 1) // 2] = 2 * X[1: (n + 1) // 2]
        if n % 2 == 0:
            A[n // 2] = X[n // 2]
        U = np.zeros(m, np.complex128)                 # spectrum at the high rate: positive frequencies only
        U[: n // 2 + 1] = A[: n // 2 + 1]
        a = np.fft.ifft(U) * D
        if sidebands is not None and sidebands[s]:
            a = np.conj(a)
        iq += (1.0 if gains is None else gains[s]) * a * np.exp(2j * np.pi * offsets[s] * t)
    return iq


def error_db(got, audio, L, margin):
    """10 log10 of the energy of got[n] - audio[n - L] over that of audio[n - L], away from both ends by `margin` samples"""
    n = min(len(got), len(audio) + L)
    idx = np.arange(margin + L, n - margin)
    ref = np.asarray(audio)[idx - L]
    return 10 * np.log10(np.sum((np.asarray(got)[idx] - ref) ** 2) / np.sum(ref ** 2))


def response_db(h, D):
    """(f, |H(f)| in dB) of the real taps h at rate 48000 * D on a grid of at most 48000 D / (8 T) Hz from 0 to the Nyquist frequency
    (a zero-padded FFT: 8 points per lobe of the window; real taps: the response at -f is the one at f)"""
    h = np.asarray(h, np.float64)
    nfft = 1 << int(np.ceil(np.log2(8 * h.size)))
    H = np.abs(np.fft.rfft(h, nfft))
    return np.fft.rfftfreq(nfft, 1.0 / (FS * D)), 20 * np.log10(np.maximum(H, 1e-300))

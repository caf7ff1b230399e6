"""The wideband impulse blanker's rule (include/ext/mercury_wideband_blanker.h) in NumPy, written from the header and not from the C++:
what tests/test_wideband_blanker_host.py holds the host twin to, byte for byte. Every product and sum below is one NumPy operation on
float64 arrays, so each is rounded on its own, as the rule has it. The guard is a difference of running counts here and a walk over the
flags in the twin. A plain module: no test lives here and it does not load the library.

Also the inputs the blanker's tests share: noise with clicks planted where the rule can go wrong, and one station with a click train."""
import functools

import numpy as np

KEY_MASK = np.uint64(0x7FFFFFFFFFFFFFFF)
REPORT_DTYPE = np.dtype([("block", np.int64), ("level", np.float64), ("exceeding", np.int32), ("blanked", np.int32), ("capped", np.int32),
                         ("pad", np.int32)])
DEFAULT_THRESHOLD = 38.0
NOISE_SEEDS = {1: 20260001, 4: 20260004, 64: 20260064}          # profiles/wideband_blanker.md: the seeds of the threshold's measurement


def default_block(D):
    """the least multiple of 64 D that is >= 256"""
    step = 64 * D
    return -(-256 // step) * step


def widen(x):
    """IQ samples, int16 [n, 2] or complex [n] -> (re, im) float64"""
    if x.dtype == np.int16:
        return x[:, 0].astype(np.float64) / 32768.0, x[:, 1].astype(np.float64) / 32768.0
    return x.real.astype(np.float64), x.imag.astype(np.float64)


def powers(iq):
    x = np.asarray(iq)
    x = x.reshape(-1, 2) if x.dtype == np.int16 else x.ravel()
    re, im = widen(x)
    with np.errstate(all="ignore"):
        return re * re + im * im


def analyse(iq, B, threshold, cap):
    """per block: level, exceeding, capped; and the exceed flags [n] that are left after the cap"""
    p = powers(iq)
    m = p.size // B
    keys = (p.view(np.uint64) & KEY_MASK).reshape(m, B)
    level = np.sort(keys, axis=1)[:, B // 2].copy().view(np.float64)
    with np.errstate(invalid="ignore"):
        limit = np.float64(threshold) * level
        exceeds = ~(p.reshape(m, B) <= limit[:, None])
    exceeding = exceeds.sum(axis=1)
    capped = exceeding > cap
    exceeds[capped] = False
    return level, exceeding, capped, exceeds.ravel()


def process(iq, D=4, position=0, block=0, threshold=DEFAULT_THRESHOLD, guard=4, max_share=0.125):
    """a fresh stage seeked to `position` (a multiple of B) and fed iq whole -> (out, the input's dtype and shape; reports REPORT_DTYPE [m])"""
    x = np.asarray(iq)
    x = x.reshape(-1, 2) if x.dtype == np.int16 else x.ravel()
    n = x.shape[0]
    B = block or default_block(D)
    assert n and n % B == 0 and position % B == 0
    m = n // B
    cap = int(np.floor(np.float64(max_share) * np.float64(B)))
    level, exceeding, capped, flags = analyse(x, B, threshold, cap)
    count = np.concatenate([[0], np.cumsum(flags)])
    i = np.arange(n)
    marked = count[np.minimum(i + guard + 1, n)] - count[np.maximum(i - guard, 0)] > 0
    y = x.copy()
    y[marked] = 0
    out = np.concatenate([np.zeros((B,) + x.shape[1:], x.dtype), y[: n - B]])
    reports = np.zeros(m, REPORT_DTYPE)
    reports["block"] = position // B - 1 + np.arange(m)
    reports["level"][1:] = level[: m - 1]
    reports["exceeding"][1:] = exceeding[: m - 1]
    reports["capped"][1:] = capped[: m - 1]
    reports["blanked"][1:] = marked.reshape(m, B).sum(axis=1)[: m - 1]
    return out, reports


def highest_ratio(x, B):
    """the highest p / med_b over the blocks of x"""
    p = powers(x).reshape(-1, B)
    return float((p.max(axis=1) / np.sort(p, axis=1)[:, B // 2]).max())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def noise(seed, n, fmt="cf64"):
    """white Gaussian noise of unit variance per component (CS16: of 1024 units, so that a click has room above it)"""
    rng = np.random.default_rng(seed)
    if fmt == "cs16":
        return np.clip(np.round(1024 * rng.standard_normal((n, 2))), -32768, 32767).astype(np.int16)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return x.astype(np.complex64 if fmt == "cf32" else np.complex128)


def _click(x, i, height=30.0):
    """a click `height` times the noise's standard deviation on sample i"""
    if x.dtype == np.int16:
        x[i] = (min(int(1024 * height), 32767), -min(int(1024 * height), 32767))
    else:
        x[i] = height * (1 + 1j)


PLANTED_BLOCKS = 12


def planted(seed, B, fmt, cap, nonfinite=True):
    """PLANTED_BLOCKS blocks of noise with, by block:
    0 a click on the block's last sample, 1 one on its first (the guard crosses the border both ways);
    2 exactly `cap` clicks, 3 `cap` + 1 (capped: passes whole); 4 constant modulus (every sample ties with the median);
    5 all zero; 6 all zero but three samples; 7 NaN, +Inf, -Inf and -0.0 samples (not CS16); 8 more NaN than half (the median is NaN;
    not CS16); 9 and 10 plain noise; 11, the last block fed, a click on its first sample, whose leading guard reaches into block 10"""
    x = noise(seed, PLANTED_BLOCKS * B, fmt)
    at = lambda b, i: b * B + i
    _click(x, at(0, B - 1))
    _click(x, at(1, 0))
    for j in range(cap):
        _click(x, at(2, 3 + 2 * j))
    for j in range(cap + 1):
        _click(x, at(3, 3 + j))
    x[at(4, 0): at(5, 0)] = (2896, -2896) if fmt == "cs16" else (3 - 4j) / 5
    x[at(5, 0): at(7, 0)] = 0
    for i in (0, B // 2, B - 1):
        _click(x, at(6, i), 0.01)
    if fmt != "cs16" and nonfinite:
        x[at(7, 9)] = complex(np.nan, 1.0)
        x[at(7, 20)] = complex(np.inf, 0.0)
        x[at(7, 31)] = complex(1.0, -np.inf)
        x[at(7, 40)] = complex(-0.0, -0.0)
        x[at(7, 41)] = complex(0.0, -0.0)
        x[at(8, 0): at(8, B // 2 + 1)] = complex(np.nan, np.nan)
    _click(x, at(11, 0))
    return x


STATION = (12000, 0, 1.0)            # a multiple of R / B = 750 Hz: a delay of B samples turns no carrier
STATION_D = 4
STATION_AUDIO = (300.0, 2643.75)


@functools.lru_cache(maxsize=None)
def station(n_audio, seed=11):
    """one station's unit-rms audio, Gaussian noise confined to Mercury's band: float64 [1, n_audio]"""
    rng = np.random.default_rng(seed)
    spec = np.fft.rfft(rng.standard_normal((1, n_audio)))
    hz = np.fft.rfftfreq(n_audio, 1.0 / 48000.0)
    spec[:, (hz < STATION_AUDIO[0]) | (hz > STATION_AUDIO[1])] = 0.0
    audio = np.fft.irfft(spec, n_audio)
    audio /= np.sqrt(np.mean(audio ** 2))
    audio.setflags(write=False)
    return audio


def clicks(n, rate_hz, sample_rate, amplitude, seed=12):
    """one-sample clicks of random phase every sample_rate / rate_hz samples: complex128 [n]"""
    rng = np.random.default_rng(seed)
    at = np.arange(int(sample_rate / rate_hz) // 2, n, int(sample_rate / rate_hz))
    x = np.zeros(n, np.complex128)
    x[at] = amplitude * np.exp(2j * np.pi * rng.random(at.size))
    return x

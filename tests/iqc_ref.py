"""The IQ corrector's rule (include/ext/mercury_iq_corrector.h) in NumPy, written from the header and not from the C++: what
tests/test_iq_corrector_host.py holds the host twin to, byte for byte. The 256 partial sums of a term are a row, and a block's rows are
added one after another; the fold is vectorised over the partials; the recursion over the blocks runs in Python floats and the estimate
in float64 scalars, each operation rounded on its own. A plain module: no test lives here and it does not load the library.

Also the inputs the corrector's tests share: a stream planted where the rule can go wrong, and one station with its impairment."""
import functools

import numpy as np

REPORT_DTYPE = np.dtype([("block", np.int64), ("dc_re", np.float64), ("dc_im", np.float64), ("skew", np.float64), ("gain", np.float64),
                         ("flags", np.int32), ("clamped", np.int32)])
SKIPPED, NO_BALANCE = 1, 2
MAX_SKEW, MAX_GAIN = 0.5, 2.0
DEFAULT_BLOCK, DEFAULT_MEMORY = 4096, 1024


def widen(x):
    """IQ samples, int16 [n, 2] or complex [n] -> (I, Q) float64"""
    if x.dtype == np.int16:
        return x[:, 0].astype(np.float64) / 32768.0, x[:, 1].astype(np.float64) / 32768.0
    return x.real.astype(np.float64), x.imag.astype(np.float64)


def block_sums(I, Q):
    """I, Q [m, B] -> S [m, 5]"""
    m, B = I.shape
    with np.errstate(all="ignore"):
        terms = np.stack([I, Q, I * I, I * Q, Q * Q], axis=1).reshape(m, 5, B // 256, 256)
        p = terms[:, :, 0, :].copy()
        for i in range(1, B // 256):
            p = p + terms[:, :, i, :]
        s = 128
        while s >= 1:
            p[:, :, :s] = p[:, :, :s] + p[:, :, s: 2 * s]
            s //= 2
    return p[:, :, 0]


def estimate(T, dc=1, balance=1):
    """the state's estimate -> (dc_re, dc_im, skew, gain, flags)"""
    tI, tQ, tII, tIQ, tQQ, N = (np.float64(t) for t in T)
    if N == 0.0:
        return 0.0, 0.0, 0.0, 1.0, NO_BALANCE
    with np.errstate(all="ignore"):
        mI, mQ = tI / N, tQ / N
        cII, cQQ, cIQ = tII / N - mI * mI, tQQ / N - mQ * mQ, tIQ / N - mI * mQ
        skew = cIQ / cII
        r = cQQ / cII - skew * skew
        gain = np.float64(1.0) / np.sqrt(r)
        valid = bool(cII > 0 and r > 0 and np.isfinite(skew) and np.isfinite(gain) and abs(skew) <= MAX_SKEW and 1.0 / MAX_GAIN <= gain <= MAX_GAIN)
    d = (float(mI), float(mQ)) if dc else (0.0, 0.0)
    if not valid:
        return d + (0.0, 1.0, NO_BALANCE)
    return d + ((float(skew), float(gain)) if balance else (0.0, 1.0)) + (0,)


def narrow(yI, yQ, like):
    """-> (samples in like's dtype, clamped components)"""
    if like.dtype == np.int16:
        with np.errstate(all="ignore"):
            r = np.rint(np.stack([yI, yQ], axis=1) * 32768.0)
        bad = (r > 32767.0) | (r < -32768.0) | np.isnan(r)
        r = np.where(np.isnan(r), 0.0, np.clip(r, -32768.0, 32767.0))
        return r.astype(np.int16), int(bad.sum())
    with np.errstate(all="ignore"):
        out = np.empty(yI.size, like.dtype)
        out.real = yI.astype(out.real.dtype)
        out.imag = yQ.astype(out.imag.dtype)
    return out, 0


def process(iq, D=4, position=0, block=0, memory=DEFAULT_MEMORY, dc=1, balance=1, fixed=0, fixed_dc_re=0.0, fixed_dc_im=0.0, fixed_skew=0.0,
            fixed_gain=1.0, state=None):
    """a fresh stage (or one in `state`, six floats) seeked to `position` and fed iq whole ->
    (out, the input's dtype and shape; reports REPORT_DTYPE [m]; the state after, six floats)"""
    x = np.asarray(iq)
    x = x.reshape(-1, 2) if x.dtype == np.int16 else x.ravel()
    n = x.shape[0]
    B = block or DEFAULT_BLOCK
    assert n and n % B == 0 and position % B == 0
    m = n // B
    lam = 1.0 - 1.0 / float(memory) if memory else 1.0
    I, Q = widen(x)
    I, Q = I.reshape(m, B), Q.reshape(m, B)
    S = None if fixed else block_sums(I, Q)
    T = [0.0] * 6 if state is None else [float(t) for t in state]
    reports = np.zeros(m, REPORT_DTYPE)
    outs = []
    for b in range(m):
        flags = 0
        if fixed:
            e = (fixed_dc_re if dc else 0.0, fixed_dc_im if dc else 0.0, fixed_skew if balance else 0.0, fixed_gain if balance else 1.0, 0)
        else:
            if not np.isfinite(S[b]).all():
                flags = SKIPPED
            else:
                for t in range(5):
                    decayed = lam * T[t]
                    T[t] = decayed + float(S[b, t])
                decayed = lam * T[5]
                T[5] = decayed + float(B)
            e = estimate(T, dc, balance)
        mI, mQ, skew, gain = (np.float64(v) for v in e[:4])
        with np.errstate(all="ignore"):
            yI = I[b] - mI
            yQ = gain * ((Q[b] - mQ) - skew * yI)
        yI, yQ = np.where(np.isnan(yI), np.float64("nan"), yI), np.where(np.isnan(yQ), np.float64("nan"), yQ)    # the one positive quiet NaN
        o, clamped = narrow(yI, yQ, x)
        outs.append(o)
        reports[b] = (position // B + b, e[0], e[1], e[2], e[3], flags | e[4], clamped)
    out = np.concatenate(outs)
    return out.reshape(np.asarray(iq).shape), reports, T


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
GAIN, PHASE_DEG, DC = 1.1, 5.0, (0.3, -0.2)                     # the impairment of the tests: 23.8 dB of image


def impair(x, gain=GAIN, phase_deg=PHASE_DEG, dc=DC):
    """a front end's IQ for the perfect complex128 signal x: I' = I + dc_re, Q' = g (Q cos(phi) + I sin(phi)) + dc_im"""
    phi = np.radians(phase_deg)
    return (x.real + dc[0]) + 1j * (gain * (x.imag * np.cos(phi) + x.real * np.sin(phi)) + dc[1])


def to_format(x, fmt, scale=1.0):
    """complex128 -> the format's samples (CS16: x * scale * 32768, rounded and clipped)"""
    if fmt == "cs16":
        return np.clip(np.rint(np.stack([x.real, x.imag], axis=1) * (scale * 32768.0)), -32768, 32767).astype(np.int16)
    return (x * scale).astype(np.complex64 if fmt == "cf32" else np.complex128)


PLANTED_BLOCKS = 10


def planted(seed, B, fmt):
    """PLANTED_BLOCKS blocks, by block: 0 all zero (no balance: the output is the input); 1 pure I, Q = 0 (r <= 0: no balance);
    2 to 4 impaired noise (a valid balance); 5 a NaN (floats) or full-scale samples that clamp (CS16); 6 impaired noise; 7 an infinity
    (floats; CS16: more full-scale samples); 8 -0.0 samples (floats) in noise; 9 impaired noise"""
    rng = np.random.default_rng(seed)
    z = 0.2 * (rng.standard_normal(PLANTED_BLOCKS * B) + 1j * rng.standard_normal(PLANTED_BLOCKS * B))
    z = impair(z)
    z[:B] = 0
    z[B: 2 * B] = z[B: 2 * B].real
    x = to_format(z, fmt)
    at = lambda b, i: b * B + i
    if fmt == "cs16":
        for b in (5, 7):
            x[at(b, 3)] = (32767, 32767)
            x[at(b, B - 1)] = (-32768, -32768)
            x[at(b, B // 2)] = (-32768, 32767)
    else:
        x[at(5, 9)] = complex(np.nan, 1.0)
        x[at(7, B - 1)] = complex(1.0, -np.inf)
        x[at(8, 40)] = complex(-0.0, -0.0)
        x[at(8, 41)] = complex(0.0, -0.0)
        x[at(8, 42)] = complex(-0.0, 0.25)
    return x


# what the stage is for: one station in one sideband at R = 192 kHz, white noise as strong as the station, the impairment above
STATION_RATE = 192000.0
STATION_BAND = (30300.0, 32700.0)


@functools.lru_cache(maxsize=None)
def station(n, seed):
    """band-limited complex noise in STATION_BAND of unit power: complex128 [n], read-only"""
    rng = np.random.default_rng(seed)
    spec = np.fft.fft(rng.standard_normal(n) + 1j * rng.standard_normal(n))
    hz = np.fft.fftfreq(n, 1.0 / STATION_RATE)
    spec[(hz < STATION_BAND[0]) | (hz > STATION_BAND[1])] = 0.0
    x = np.fft.ifft(spec)
    x /= np.sqrt(np.mean(np.abs(x) ** 2))
    x.setflags(write=False)
    return x


def white(n, seed, power=1.0):
    rng = np.random.default_rng(seed)
    return np.sqrt(power / 2.0) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def image_db(x):
    """the power in STATION_BAND over the power in its mirror band, in dB"""
    spec = np.abs(np.fft.fft(x)) ** 2
    hz = np.fft.fftfreq(x.size, 1.0 / STATION_RATE)
    own = spec[(hz >= STATION_BAND[0]) & (hz <= STATION_BAND[1])].sum()
    mirror = spec[(hz <= -STATION_BAND[0]) & (hz >= -STATION_BAND[1])].sum()
    return 10.0 * np.log10(own / mirror)


def apply(x, dc_re, dc_im, skew, gain):
    """the correction with given coefficients on complex128 x (what the test measures an estimate by)"""
    yI = x.real - dc_re
    return yI + 1j * (gain * ((x.imag - dc_im) - skew * yI))

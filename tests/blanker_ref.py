"""What the tests of the impulse blanker (include/mercury_blanker.h) share: a numpy restatement of its rule, the impulse frames - one-sample
impulses far above the frame's power at a fixed repetition period, which the FFT spreads over every carrier of every symbol -, the faded
noise-only frames on which a blanker must stay silent, and the hand-made frames of the rule's edges. The frames are built on the host by
one fixed recipe so that the CPU and the GPU tests see the same samples."""
import functools

import numpy as np

from oraclelib import Oracle, noise_amp_for

DY5 = {"Dy": 5, "Nsymb": 20}
MFSK = 100
DEFAULT = dict(threshold=24.0, guard=4, max_share=0.125)
FS_BB = 12000.0
# the points of the table in profiles/blanker.md: mode -> (Es/N0 dB, impulse dB above the frame's mean power, width in samples)
POINTS = {13: (14.0, 25.0, 1), 11: (10.0, 25.0, 1), 8: (6.0, 25.0, 1), 0: (6.0, 25.0, 1), MFSK: (6.0, 25.0, 1)}
PERIOD = 100


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------
def np_blank(frame, L, threshold=24.0, guard=4, max_share=0.125):
    """the rule in numpy: (output complex128 [n], marked, blanked). np.sort per block for the median, boolean dilation for the guard."""
    x = np.asarray(frame, np.complex128).ravel()
    n = x.size
    with np.errstate(all="ignore"):
        p = x.real * x.real + x.imag * x.imag                      # three roundings: numpy fuses nothing
    key = p.view(np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF)
    exceed = np.zeros(n, bool)
    for base in range(0, n, L):
        k = key[base: base + L]
        med = np.sort(k)[k.size // 2: k.size // 2 + 1].view(np.float64)[0]
        with np.errstate(all="ignore"):
            limit = np.float64(threshold) * med
            exceed[base: base + L] = ~(p[base: base + L] <= limit)
    mark = exceed.copy()
    for d in range(1, guard + 1):
        mark[d:] |= exceed[:-d]
        mark[:-d] |= exceed[d:]
    marked = int(mark.sum())
    cap = int(np.floor(np.float64(max_share) * np.float64(n)))
    if marked > cap:
        return x.copy(), marked, 0
    out = x.copy()
    out[mark] = 0.0 + 0.0j
    return out, marked, marked


# ---- the frames -----------------------------------------------------------------------------------------------------------------------------
def _key(explicit):
    return tuple(sorted((explicit or {}).items()))


def fading_gain(rng, n, fd):
    """a Rayleigh-like gain: 8 unit sinusoids of Doppler fd cos(theta_k), theta_k = pi (k + 1/2) / 8, phases uniform(0, 2 pi, 8), over
    t = i / 12000, divided by sqrt(8) (unit mean power)"""
    phase = rng.uniform(0, 2 * np.pi, 8)
    theta = np.pi * (np.arange(8) + 0.5) / 8
    t = np.arange(n) / FS_BB
    return np.exp(1j * (2 * np.pi * fd * np.cos(theta)[:, None] * t[None, :] + phase[:, None])).sum(axis=0) / np.sqrt(8.0)


@functools.lru_cache(maxsize=None)
def _frames(cfg, explicit_key, esn0, impulse_db, width, period, frames, fd):
    explicit = dict(explicit_key)
    orc = Oracle(cfg, 50, explicit=dict(explicit))
    rng = np.random.default_rng(11)
    amp = 16.0 * noise_amp_for(esn0)
    bb, bits, payload = [], [], []
    for f in range(frames):
        x, pl = orc.gen_frame(5, f, 0.0, 0)
        n = x.size
        bits.append(orc.rx(x)["bits"].copy())
        payload.append(pl)
        P = float(np.mean(np.abs(x) ** 2))
        if fd:
            x = x * fading_gain(rng, n, fd)
        noise_re = rng.standard_normal(n)
        y = x + amp * (noise_re + 1j * rng.standard_normal(n))
        if impulse_db is not None:
            start = int(rng.integers(0, period))
            at = np.arange(start, n, period)
            for w in range(width):
                pos = at[at + w < n] + w
                y[pos] += np.sqrt(P * 10.0 ** (impulse_db / 10.0)) * np.exp(1j * rng.uniform(0, 2 * np.pi, pos.size))
        bb.append(y)
    return dict(orc=orc, explicit=explicit or None, bb=np.stack(bb), bits=bits, payload=payload)


def impulse_frames(cfg, explicit=None, esn0=6.0, impulse_db=25.0, width=1, period=PERIOD, frames=16, fd=0.0):
    """`frames` clean frames of the generator (seed 5, x = gen_frame(5, f, 0.0, 0), P = mean |x|^2) disturbed with default_rng(11), used
    frame after frame in this order: with fd, the gain's 8 phases (fading_gain), which multiplies x; the noise 16 * noise_amp_for(esn0) *
    (standard_normal(n) + 1j standard_normal(n)); with impulse_db, start = integers(0, period) and, for each of `width` adjacent samples,
    sqrt(P 10^(dB/10)) exp(1j uniform(0, 2 pi, k)) added at start, start + period, ... impulse_db None: noise only.
    -> dict(orc, explicit, bb [frames, n], bits: each clean frame's message bits, payload)"""
    return _frames(cfg, _key(explicit), float(esn0), impulse_db, int(width), int(period), int(frames), float(fd))


def decoded(orc, ref, bits):
    """the oracle's rx output `ref` decodes, with the sent bits"""
    return bool(ref["crc"] == 0 and not ref["all_zeros"] and np.array_equal(ref["bits"], bits))


def block_len(orc):
    return int(orc.Nofdm)


def hand_made(orc, rng_seed=3):
    """frames of the rule's edges, on unit-power noise: name -> frame. L = the symbol length, n = the frame's samples."""
    n, L = int(orc.frame_samples), block_len(orc)
    rng = np.random.default_rng(rng_seed)

    def noise():
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)

    out = {}
    x = noise(); x[L + 7] = complex(np.nan, 1.0); out["a NaN sample"] = x
    x = noise(); x[2 * L + 9] = complex(np.inf, 0.0); out["an inf sample"] = x
    x = noise(); x[L: 2 * L] = 0; x[L + 40] = 1e-3; out["a block of zeros with one small sample"] = x
    x = noise(); x[0: L] = 0; out["a block of zeros"] = x
    x = noise(); x[L: L + L // 2 + 3] = complex(np.nan, np.nan); out["a block more than half NaN"] = x
    x = noise(); x[-1] = complex(-np.nan, 0.0); x[5] = complex(0.0, -np.nan); out["NaNs of either sign at the ends"] = x
    x = noise(); x[2 * L: 3 * L] = 1.0; x[2 * L + 100] = 5.0; x[2 * L + 200] = 4.8; out["equal powers at the median"] = x
    x = noise(); x[0] = 30.0; x[-1] = 30.0j; out["impulses on the first and last sample"] = x
    x = noise(); x[L - 1] = 30.0; x[3 * L] = -30.0; out["impulses on both sides of a block border"] = x
    x = noise(); x[2 * L - 2] = 30.0; x[2 * L + 1] = 30.0; out["impulses whose guards meet across a border"] = x
    return out


def cap_frames(orc, guard=0, max_share=0.125):
    """(a frame with marked == cap, one with marked == cap + 1): unit-magnitude samples with isolated impulses about 7 samples apart (far fewer than half
    of a block, so every median stays 1)"""
    n = int(orc.frame_samples)
    cap = int(np.floor(max_share * n))
    step = 2 * guard + 3
    pos = np.arange(0, n, max(step, n // (cap + 2)))
    assert guard == 0 and pos.size >= cap + 1, "the fixture marks one sample per impulse"
    x = np.exp(1j * np.linspace(0, 50, n))
    at, over = x.copy(), x.copy()
    at[pos[:cap]] *= 30.0
    over[pos[: cap + 1]] *= 30.0
    return at, over, cap


def mixed_batch(cfg, explicit=None, frames=8):
    """the GPU tests' batch: impulse frames of the mode's point, a clean frame, a frame over the cap, and the NaN / zero-block frames"""
    esn0, db, width = POINTS.get(cfg, POINTS[8])
    t = impulse_frames(cfg, explicit, esn0, db, width, frames=frames)
    orc = t["orc"]
    bb = t["bb"].copy()
    hm = hand_made(orc)
    bb[1] = impulse_frames(cfg, explicit, esn0, None, frames=2)["bb"][1]            # a clean frame
    over = bb[2].copy()                                                            # over the cap: every sixth sample 32 dB up is more than n / 8 marked samples, with or without the guard
    over[::6] *= 40.0
    bb[2] = over
    bb[3] = hm["a NaN sample"]
    bb[4] = hm["a block of zeros with one small sample"]
    bb[5] = hm["a block more than half NaN"]
    return orc, bb


# ---- receive_byte on passband windows with clicks ---------------------------------------------------------------------------------------------
WINDOWS = 8
INBAND_DB = 20.0
CLICK_PERIOD = 800                   # passband samples at 48 kHz: every 200 samples of the 12 kHz baseband (a 60 Hz source); the receive filter
                                     # smears a click over 8 to 9 baseband samples, so with the guard every 100 would mark more than the default cap


@functools.lru_cache(maxsize=None)
def click_windows(cfg=13, impulse_db=25.0):
    """8 capture windows: transmit_byte(output_power_watt = 1) placed at ((preamble_nsymb + 2) Nofdm + 50) 4 in white noise at 20 dB in-band
    SNR (as residual_cfo_ref.noisy_windows), and the same windows with one-sample clicks every 800 passband samples over the data symbols
    (the synchroniser reads unblanked samples - a stated limit of the stage - so the preamble is left alone), at baseband scale: the click's amplitude is such that its peak behind the receive filter (the oracle's passband_to_baseband of a unit
    click, data filter, decimation 1) is sqrt(P 10^(dB/10)), P the transmission's mean power behind the same filter. default_rng(3); per
    window the payload bytes, then the noise, then the clicks' start = integers(0, 800) and signs.
    -> dict(orc, clean [8, n], clicks [8, n], payload [8, payload_bytes])"""
    from oraclelib import CARRIER
    orc = Oracle(cfg, 50)
    rng = np.random.default_rng(3)
    n = orc.buffer_samples()
    d = ((orc.preamble_nsymb + 2) * orc.Nofdm + 50) * 4
    unit = np.zeros(4096)
    unit[2048] = 1.0
    peak = float(np.abs(orc.passband_to_baseband(unit, CARRIER, 1, 1)).max())
    clean, clicks, payloads = [], [], []
    for _ in range(WINDOWS):
        pl = rng.integers(0, 256, orc.payload_bytes).astype(np.uint8)
        audio = np.asarray(orc.transmit_byte(pl, CARRIER, output_power_watt=1.0), np.float64).ravel()
        sigma = np.sqrt(np.mean(audio * audio) / (10.0 ** (INBAND_DB / 10.0) * 2343.75 / 24000.0))
        w = sigma * rng.standard_normal(n)
        w[d: d + audio.size] += audio
        P = float(np.mean(np.abs(orc.passband_to_baseband(audio, CARRIER, 1, 1)) ** 2))
        data = d + orc.preamble_nsymb * orc.Nofdm * 4
        at = np.arange(data + int(rng.integers(0, CLICK_PERIOD)), d + audio.size, CLICK_PERIOD)
        c = w.copy()
        c[at] += np.sqrt(P * 10.0 ** (impulse_db / 10.0)) / peak * rng.choice([-1.0, 1.0], at.size)
        clean.append(w)
        clicks.append(c)
        payloads.append(pl)
    return dict(orc=orc, clean=np.stack(clean), clicks=np.stack(clicks), payload=np.stack(payloads))

"""What the tests of the pilot-aided residual carrier-offset correction (include/mercury_cfo.h) share: a numpy restatement of its rule
(the reference platform's atan and sincos through Oracle.libm_atan_sincos), frames of the generator turned by a carrier offset, and the
noisy passband windows on which receive_byte's own offset estimate is what loses the frame."""
import functools

import numpy as np

from demapper_csi_ref import CASES
from oraclelib import CARRIER, Oracle, noise_amp_for

FS_BB = 12000.0
SEED_CFO = 77
OFFSETS = {3: (0.0, 0.7, -2.0, 6.5), 5: (0.0, 0.7, -2.0, 4.0)}          # Hz, by Dy: inside 12000 / (2 Dy Nofdm) = 7.35 / 4.4 Hz


def offsets_for(explicit):
    return OFFSETS[(explicit or {}).get("Dy", 3)]


def step_to_hz(step, nofdm=272):
    return step * FS_BB / (2.0 * np.pi * nofdm)


def offset_frame(orc, frame, f_hz, esn0_db, seed=SEED_CFO):
    """the generator's clean frame `frame`, turned by f_hz at the 12 kHz baseband rate, plus the generator's own noise for that frame
    -> (samples, payload bytes)"""
    clean, payload = orc.gen_frame(seed, frame, 0.0, 0)
    n = np.arange(clean.size)
    return orc.channel(clean * np.exp(2j * np.pi * f_hz * n / FS_BB), seed, frame, noise_amp_for(esn0_db), 0), payload


def _get_angle(orc, re, im):
    """misc.cc:34-56 with the platform's atan"""
    with np.errstate(all="ignore"):
        a = float(orc.libm_atan_sincos(np.array([np.float64(im) / np.float64(re)]))[0][0])
    if re == 0:
        return np.pi / 2
    if re > 0:
        return a
    return a + np.pi if im >= 0 else a - np.pi


def np_cfo_pilots(orc, grid, dy=3):
    """the rule in numpy / Python floats (IEEE double, one operation after the other): (turned grid complex128 [Nsymb * Nc], step)"""
    Ns, Nc = orc.Nsymb, orc.Nc
    types = orc.frame_types().reshape(Ns, Nc)
    sign = np.zeros(Ns * Nc)
    sign[np.flatnonzero(types.ravel() != 0)] = np.where(orc.pilot_seq().real < 0, -1.0, 1.0)
    g = np.asarray(grid, np.complex128).reshape(Ns, Nc)
    sign = sign.reshape(Ns, Nc)
    zr, zi = g.real * sign, g.imag * sign                                  # exact: +-1 (data cells are not read)
    rr = ri = 0.0
    with np.errstate(all="ignore"):
        for c in range(Nc):
            ar = ai = 0.0
            rows = np.flatnonzero(types[:, c] != 0)
            for s0, s1 in zip(rows[:-1], rows[1:]):
                if s1 - s0 != dy:
                    continue
                z0r, z0i, z1r, z1i = float(zr[s0, c]), float(zi[s0, c]), float(zr[s1, c]), float(zi[s1, c])
                ar = ar + (z1r * z0r + z1i * z0i)
                ai = ai + (z1i * z0r - z1r * z0i)
            rr = rr + ar
            ri = ri + ai
    if not (np.isfinite(rr) and np.isfinite(ri)) or (rr == 0 and ri == 0):
        return g.ravel().copy(), 0.0
    step = _get_angle(orc, rr, ri) / float(dy)
    _, sn, cs = orc.libm_atan_sincos(-step * np.arange(Ns, dtype=np.float64))
    sn, cs = sn[:, None], cs[:, None]
    with np.errstate(all="ignore"):
        out = (g.real * cs - g.imag * sn) + 1j * (g.real * sn + g.imag * cs)
    return out.ravel(), float(step)


def derotate_samples(orc, bb, step):
    """symbol s of the samples multiplied by exp(-j step s): what the stage does to the grid, applied in front of the FFT"""
    s = np.arange(bb.size) // orc.Nofdm
    return bb * np.exp(-1j * step * s)


def decoded(orc, ref, payload):
    return bool(ref["crc"] == 0 and not ref["all_zeros"] and np.array_equal(ref["bytes"][: orc.payload_bytes], payload))


@functools.lru_cache(maxsize=None)
def decode_fixture(f_hz, frames=16, cfg=8, esn0_db=2.0):
    """mode 8 at 2 dB, seed 77, frames 0 .. 15 turned by f_hz -> dict(orc, bb [frames, samples], payload, ref: the oracle's rx per frame)"""
    orc = Oracle(cfg, 50)
    made = [offset_frame(orc, f, f_hz, esn0_db) for f in range(frames)]
    bb = np.stack([m[0] for m in made])
    return dict(orc=orc, bb=bb, payload=[m[1] for m in made], ref=[orc.rx(bb[f]) for f in range(frames)])


# ---- receive_byte on noisy passband windows ----------------------------------------------------------------------------------------
WINDOWS = 12
INBAND_DB = 4.0


@functools.lru_cache(maxsize=None)
def noisy_windows(cfg=8):
    """12 capture windows: transmit_byte(output_power_watt = 1) placed at ((preamble_nsymb + 2) Nofdm + 50) 4 in white noise at 4 dB in-band
    SNR (sigma = sqrt(P / (10^0.4 * 2343.75 / 24000)), P the audio's mean square), true carrier offset 0. default_rng(3); per window the
    payload bytes are drawn first, then the noise. -> dict(orc, wins [12, n], payload [12, payload_bytes])"""
    orc = Oracle(cfg, 50)
    rng = np.random.default_rng(3)
    n = orc.buffer_samples()
    d = ((orc.preamble_nsymb + 2) * orc.Nofdm + 50) * 4
    wins, payloads = [], []
    for _ in range(WINDOWS):
        pl = rng.integers(0, 256, orc.payload_bytes).astype(np.uint8)
        audio = np.asarray(orc.transmit_byte(pl, CARRIER, output_power_watt=1.0), np.float64).ravel()
        sigma = np.sqrt(np.mean(audio * audio) / (10.0 ** (INBAND_DB / 10.0) * 2343.75 / 24000.0))
        w = sigma * rng.standard_normal(n)
        w[d: d + audio.size] += audio
        wins.append(w)
        payloads.append(pl)
    return dict(orc=orc, wins=np.stack(wins), payload=np.stack(payloads))


__all__ = ["CASES", "offsets_for", "offset_frame", "np_cfo_pilots", "derotate_samples", "decoded", "decode_fixture", "noisy_windows", "step_to_hz"]

"""What the carrier excisor's tests share (include/ext/mercury_excisor.h): a numpy restatement of the rule with np.fft, and the seeded
window builders. Everything here is computed once per process and handed out read-only."""
import functools

import numpy as np

FS = 48000.0
N, H, BAND = 1024, 512, 64
BIN_HZ = FS / N                                  # 46.875
DEFAULT = dict(threshold=12.0, guard=1, max_bins=16)
LENGTHS = (1, 100, 511, 512, 513, 1024, 1537, 4096, 92480)
CONTENTS = ("tone", "two", "keyed", "centre", "between")
MARGIN = 1e-9                                    # a case whose decision hangs on a rounding is no case: see twin_cases
WIN = np.sin(np.pi * np.arange(N) / N)


def band_lo(carrier_hz):
    return int(min(448, max(1, int(np.floor(carrier_hz / BIN_HZ + 0.5)) - 32)))


def ref_excise(x, carrier_hz, threshold=12.0, guard=1, max_bins=16):
    """The rule, restated with numpy's FFT -> (y, report dict + "A" the 64 summed powers). Not bit-exact: np.fft orders its sums its own way."""
    x = np.asarray(x, np.float64)
    n = x.size
    B = -(-n // H) + 1
    lo = band_lo(carrier_hz)
    xp = np.zeros((B + 1) * H)
    xp[H: H + n] = x
    blocks = np.stack([xp[b * H: b * H + N] for b in range(B)]) * WIN
    X = np.fft.fft(blocks, axis=1)[:, lo: lo + BAND]
    A = (X.real ** 2 + X.imag ** 2).sum(0)
    rep = dict(exceeding=0, mask=0, band_lo=lo, excised=0, nonfinite=0, level=0.0, A=A)
    if not np.isfinite(A).all():
        rep["nonfinite"] = 1
        return x.copy(), rep
    level = float(np.sort(A)[BAND // 2])
    exc = ~(A <= threshold * level)
    mask = exc.copy()
    for d in range(1, guard + 1):
        mask[d:] |= exc[:-d]
        mask[:-d] |= exc[d:]
    rep.update(level=level, exceeding=sum(1 << k for k in range(BAND) if exc[k]), mask=sum(1 << k for k in range(BAND) if mask[k]))
    bits = int(mask.sum())
    if bits == 0 or bits > max_bins:
        return x.copy(), rep
    rep["excised"] = bits
    k = lo + np.flatnonzero(mask)
    E = np.exp(2j * np.pi * np.outer(k, np.arange(N)) / N)
    e = (X[:, mask] @ E).real * WIN / 512.0                # [B, N]
    ola = np.zeros((B + 1) * H)
    for b in range(B):
        ola[b * H: b * H + N] += e[b]
    return x - ola[H: H + n], rep


def margin(rep, threshold):
    """the smallest relative distance of a summed power to the limit"""
    limit = threshold * rep["level"]
    if limit == 0:
        return 0.0
    return float(np.min(np.abs(rep["A"] - limit)) / limit)


def tone(n, hz, amp=1.0, phase=0.0):
    return amp * np.cos(2 * np.pi * hz * np.arange(n) / FS + phase)


def keyed(n, hz, amp=1.0, on_ms=60.0):
    gate = (np.arange(n) // int(FS * on_ms / 1000.0)) % 2 == 0
    return tone(n, hz, amp) * gate


def content(kind, n, rng, sigma=0.01):
    """one window of the twin's test set: noise sigma plus the named carrier(s) at unit amplitude"""
    x = sigma * rng.standard_normal(n)
    if kind == "tone":
        x += tone(n, 1471.875 + 317.0, 1.0, 0.3)
    elif kind == "two":
        x += tone(n, 1471.875 + 317.0, 1.0, 0.3) + tone(n, 1471.875 - 600.0, 0.7, 1.1)
    elif kind == "keyed":
        x += keyed(n, 1471.875 + 317.0)
    elif kind == "centre":
        x += tone(n, 1500.0, 1.0, 0.7)              # bin 32 exactly
    elif kind == "between":
        x += tone(n, 1523.4375, 1.0, 0.7)           # half-way between bins 32 and 33
    elif kind == "twenty":
        # over max_bins: not a narrowband problem. Twenty carriers on neighbouring bin centres, 30 dB over the noise of a bin: a block of
        # some 24 bins exceeds and the other 40 keep the median at the noise (twenty strong carriers anywhere in a band of 64 bins raise
        # the median itself with their skirts, and nothing exceeds)
        for j in range(20):
            x += tone(n, (20 + j) * BIN_HZ, 3.0 * sigma, 0.37 * j * j)
    elif kind != "clean":
        raise ValueError(kind)
    return x


@functools.lru_cache(maxsize=None)
def twin_cases(carrier_hz=1471.875):
    """[(kind, n, x, y_ref, rep_ref)] over LENGTHS x CONTENTS, without the cases whose decision a rounding could turn (a summed power within
    MARGIN of the limit): the twin's FFT and numpy's round differently at 1e-16. No more than one case in ten may go that way."""
    out, dropped = [], 0
    for n in LENGTHS:
        for j, kind in enumerate(CONTENTS):
            x = content(kind, n, np.random.default_rng(1000 * n + j))
            y, rep = ref_excise(x, carrier_hz, **DEFAULT)
            if margin(rep, DEFAULT["threshold"]) <= MARGIN:
                dropped += 1
                continue
            x.setflags(write=False)
            y.setflags(write=False)
            out.append((kind, n, x, y, rep))
    assert dropped * 10 <= len(LENGTHS) * len(CONTENTS), dropped
    return tuple(out)


BATCH_KINDS = ("tone", "two", "keyed", "clean", "twenty")


@functools.lru_cache(maxsize=None)
def batch(n, seed=7):
    """[5, n]: tone, two tones, keyed, clean, over the cap"""
    rng = np.random.default_rng(seed + n)
    x = np.stack([content(kind, n, rng) for kind in BATCH_KINDS])
    x.setflags(write=False)
    return x


def add_tone(orc, wins, sir_db, df_hz, carrier_hz, key_ms=None, phase=0.2):
    """the windows plus a carrier at carrier_hz + df_hz whose power is the transmitted frame's own power less sir_db"""
    pb = orc.tx_passband(orc.payload_to_bits(np.zeros(orc.payload_bytes, np.int64)))
    amp = float(np.sqrt(2.0 * np.mean(pb ** 2) * 10.0 ** (-sir_db / 10.0)))
    n = wins.shape[1]
    t = keyed(n, carrier_hz + df_hz, amp, key_ms) if key_ms else tone(n, carrier_hz + df_hz, amp, phase)
    return wins + t


@functools.lru_cache(maxsize=None)
def toned_windows(cfg, sir_db, sigma, df_hz, count=8, seed=0):
    """count capture windows of mode cfg as tests/test_receive_byte.py make_windows builds them (a frame at a varying delay in noise sigma), and
    the same windows plus the tone -> dict(orc, clean, toned, payload)"""
    from oraclelib import CARRIER, Oracle
    from test_receive_byte import make_windows
    orc = Oracle(cfg)
    room = orc.buffer_samples() - orc.tx_passband(orc.payload_to_bits(np.zeros(orc.payload_bytes, np.int64))).size
    rng = np.random.default_rng(seed + 31 * cfg)
    # (the reference's bounds check wants the preamble more than `preamble` symbols into the window: delays from 5 symbols on)
    specs = [("frame", int(rng.integers(5 * 1088 + 1, min(room, 44 * 1088))), sigma, 100 + seed + i) for i in range(count)]
    clean, pls = make_windows(orc, specs, seed=500 + seed + cfg)
    toned = add_tone(orc, clean, sir_db, df_hz, CARRIER)
    for a in (clean, toned):
        a.setflags(write=False)
    return dict(orc=orc, clean=clean, toned=toned, payload=pls)


def decoded(orc, res, payload):
    return res["message_decoded"] == 1 and np.array_equal(res["payload"][: orc.payload_bytes], np.asarray(payload, np.uint8))

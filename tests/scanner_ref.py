"""The band scanner's rule (include/ext/mercury_scanner.h) in NumPy and plain Python, written from the header and not from the C++: what
tests/test_scanner_host.py holds the host twin to, byte for byte. Every product, sum and difference below is one NumPy operation on
float64 arrays, so each is rounded on its own, as the rule has it. A plain module: no test lives here.

Also the inputs the scanner's tests share: tones that fall into exactly two bins, and three synthesised links in noise."""
import functools

import numpy as np

import mercury_amd as M

KEY_MASK = np.uint64(0x7FFFFFFFFFFFFFFF)
KEY_INF = np.uint64(0x7FF0000000000000)
DEFAULTS = dict(log2n=12, blocks_per_line=16, threshold=M.SCAN_DEFAULT_THRESHOLD, edge_bins=None, dc_bins=2, gap=2, min_bins=2, max_runs=32)


def settings(**config):
    k = dict(DEFAULTS, **config)
    if k["edge_bins"] is None:
        k["edge_bins"] = (1 << k["log2n"]) // 32
    return k


@functools.lru_cache(maxsize=None)
def tables(log2n):
    N = 1 << log2n
    a = 2.0 * np.pi * np.arange(N, dtype=np.float64) / np.float64(N)
    return np.cos(a), np.sin(a), np.sin(np.pi * np.arange(N, dtype=np.float64) / np.float64(N))


@functools.lru_cache(maxsize=None)
def bit_reversal(log2n):
    i = np.arange(1 << log2n)
    r = np.zeros_like(i)
    for b in range(log2n):
        r |= ((i >> b) & 1) << (log2n - 1 - b)
    return r


def widen(iq):
    """IQ samples as Channelizer.process takes them -> (re, im) float64"""
    x = np.asarray(iq)
    if x.dtype == np.int16:
        x = x.reshape(-1, 2)
        return x[:, 0].astype(np.float64) / 32768.0, x[:, 1].astype(np.float64) / 32768.0
    x = x.ravel()
    return x.real.astype(np.float64), x.imag.astype(np.float64)


def transform(vr, vi, log2n):
    """the rule's radix-2 network on v -> a (re, im), bins in the transform's order k"""
    N = 1 << log2n
    cos, sin, _ = tables(log2n)
    rev = bit_reversal(log2n)
    ar, ai = np.empty(N), np.empty(N)
    ar[rev], ai[rev] = vr, vi
    size = 2
    while size <= N:
        half, step = size // 2, N // size
        wr, wi = cos[np.arange(half) * step], -sin[np.arange(half) * step]
        ar, ai = ar.reshape(-1, size), ai.reshape(-1, size)
        lor, loi, hir, hii = ar[:, :half].copy(), ai[:, :half].copy(), ar[:, half:].copy(), ai[:, half:].copy()
        tr = wr * hir - wi * hii
        ti = wr * hii + wi * hir
        ar[:, :half], ai[:, :half] = lor + tr, loi + ti
        ar[:, half:], ai[:, half:] = lor - tr, loi - ti
        ar, ai = ar.reshape(N), ai.reshape(N)
        size *= 2
    return ar, ai


def usable_bins(k):
    N = 1 << k["log2n"]
    f = np.arange(N)
    ok = (f >= k["edge_bins"]) & (f <= N - 1 - k["edge_bins"])
    if k["dc_bins"]:
        ok &= np.abs(f - N // 2) > k["dc_bins"]
    return ok


def detect(L, k, first_block):
    """one line's report as a SCAN_REPORT_DTYPE scalar"""
    N = 1 << k["log2n"]
    r = np.zeros((), M.SCAN_REPORT_DTYPE)
    r["first_block"] = first_block
    use = usable_bins(k)
    keys = L.view(np.uint64)[use] & KEY_MASK
    if np.any(keys >= KEY_INF):
        r["nonfinite"] = 1
        return r
    level = np.sort(keys)[keys.size // 2].view(np.float64)
    r["level"] = level
    with np.errstate(invalid="ignore"):
        occ = use & ~(L <= np.float64(k["threshold"]) * level)
    closed = occ.copy()
    f = 0
    while f < N:                                # a stretch of unoccupied usable bins with an occupied bin directly on both sides
        if occ[f] or not use[f]:
            f += 1
            continue
        e = f
        while e < N and use[e] and not occ[e]:
            e += 1
        if f > 0 and occ[f - 1] and e < N and occ[e] and e - f <= k["gap"]:
            closed[f:e] = True
        f = e
    runs, f = [], 0
    while f < N:
        if not closed[f]:
            f += 1
            continue
        e = f
        while e < N and closed[e]:
            e += 1
        if e - f >= k["min_bins"]:
            runs.append((f, e - f))
        f = e
    r["n_runs"], r["reported"] = len(runs), min(len(runs), k["max_runs"])
    for i, (first, count) in enumerate(runs[: k["max_runs"]]):
        power = np.float64(0.0)
        for v in L[first: first + count]:
            power = power + v
        r["runs"][i] = (first, count, first + int(np.argmax(L[first: first + count])), 0, power)
    return r


def process(iq, position=0, **config):
    """a fresh scanner seeked to `position` (a multiple of H A) and fed iq whole -> (lines [n, N], reports SCAN_REPORT_DTYPE [n])"""
    k = settings(**config)
    N, A = 1 << k["log2n"], k["blocks_per_line"]
    H = N // 2
    re, im = widen(iq)
    assert re.size % H == 0 and position % (H * A) == 0
    _, _, win = tables(k["log2n"])
    re, im = np.concatenate([np.zeros(H), re]), np.concatenate([np.zeros(H), im])       # zeros before the seek
    j, m = position // H, (re.size - H) // H
    lines, reports = [], []
    acc = np.zeros(N)
    for b in range(m):
        ar, ai = transform(re[b * H: b * H + N] * win, im[b * H: b * H + N] * win, k["log2n"])
        P = ar * ar + ai * ai
        acc = acc + np.roll(P, N // 2)          # f = (k + N / 2) mod N
        if (j + b + 1) % A == 0:
            lines.append(acc)
            reports.append(detect(acc, k, j + b + 1 - A))
            acc = np.zeros(N)
    return np.array(lines).reshape(-1, N), np.array(reports, M.SCAN_REPORT_DTYPE).reshape(-1)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def two_bin_tones(log2n, n, firsts, amplitude=1.0):
    """the sum of one tone per entry of `firsts`, each half-way between the bins f and f + 1: under the sine window, whose transform is two
    lines half a bin either side, a full block of such a tone falls into exactly those two bins (and rounding into the others)"""
    N = 1 << log2n
    i = np.arange(n, dtype=np.float64)
    x = np.zeros(n, np.complex128)
    for f in firsts:
        x += amplitude * np.exp(2j * np.pi * ((f - N // 2 + 0.5) / N) * i)
    return x


def floor_noise(seed, n, amplitude=1e-3):
    rng = np.random.default_rng(seed)
    return amplitude * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


LINK_D = 4
LINK_PLAN = ((-61000, 0, 1.0), (12500, 0, 1.0), (70250, 1, 1.0))           # two USB links and one LSB link in a 192 kHz span
LINK_AUDIO = (300.0, 2643.75)                                               # Mercury's audio band
LINK_CENTRE = 1472


def link_centres():
    """the true centre of each link's band: offset + sigma a_c"""
    return [off + (-1 if sb else 1) * LINK_CENTRE for off, sb, _ in LINK_PLAN]


@functools.lru_cache(maxsize=None)
def three_links(snr_db, lines=2, seed=7):
    """three links (Gaussian noise confined to Mercury's audio band, unit power each) through host_synth_process at D = 4, plus white
    noise: complex128 IQ for `lines` lines of the default scanner. snr_db: a link's power over the noise power inside its own
    2343.75 Hz."""
    rng = np.random.default_rng(seed)
    n_audio = lines * 16 * 2048 // LINK_D
    spec = np.fft.rfft(rng.standard_normal((3, n_audio)))
    hz = np.fft.rfftfreq(n_audio, 1.0 / 48000.0)
    spec[:, (hz < LINK_AUDIO[0]) | (hz > LINK_AUDIO[1])] = 0.0
    audio = np.fft.irfft(spec, n_audio)
    audio /= np.sqrt(np.mean(audio ** 2, axis=1, keepdims=True))
    iq = M.host_synth_process(LINK_D, LINK_PLAN, audio)
    p_link = np.mean(np.abs(iq) ** 2) / 3.0
    R = 48000.0 * LINK_D
    p_noise = p_link / 10 ** (snr_db / 10.0) * R / (LINK_AUDIO[1] - LINK_AUDIO[0])      # over the whole span
    noise = np.sqrt(p_noise / 2.0) * (rng.standard_normal(iq.size) + 1j * rng.standard_normal(iq.size))
    out = iq + noise
    out.setflags(write=False)
    return out

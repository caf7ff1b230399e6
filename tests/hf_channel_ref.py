"""The Watterson HF channel's definition for the tests, in one place, and the error budget a double-precision evaluation of
it is held to.

* ``_numpy_channel``: the composition of the library's own host definitions (host taps, host Hilbert FIR) in double precision.
* ``taps_longdouble`` / ``channel_longdouble``: the closed form from the host draws with time and phase in 80-bit extended precision, so
  that the reference stays exact where the phase 2 pi f t is large (a stream position beyond 2^32 samples: about 1e7 rad).
* ``phase_bound``: what a double-precision evaluation may differ from that by, per sample.

The budget. The device and the host twin each form 2 pi f, t = (t0 + i) / fs, their product and the sum with phi in double precision: four
roundings of a value of magnitude at most Phi = max |2 pi f t + phi|, each at most 2^-53 relative, so a sinusoid's phase is off by at most
4 * 2^-53 * Phi and its value by no more. Path k sums ns_k sinusoids of amplitude amp_k onto the delayed input, so sample i may be off by
sum_k amp_k ns_k 4 2^-53 Phi_k |a[i - d_k]|. On top of that comes the project's 1e-10 x RMS for the Hilbert sum's order and sincos itself
(tests/test_gpu_hf_channel.py). The 80-bit reference's own four roundings are 2^-64 relative each, 2048 times below the budget.
Not counted: the kernel's one rounding of f + df where the channel has a frequency offset, and the double nearest pi that both use
(0.35 * 2^-53 off). Measured, the device uses under 0.04 of the budget at a position of 2^32 + 320 and the host twin's worst path 0.65 of
its own (profiles/hf_channel.md)."""
import numpy as np

U = 2.0 ** -53                          # unit roundoff of a double
PHASE_ROUNDINGS = 4                     # 2 pi f, t, their product, the sum with phi


def _numpy_channel(x, ch, seed, r0, fs, t0=0):
    """y = Re / (.)(e^{j 2 pi df t} sum_k g_k(t) a[i - d_k]), a = x + j Hx (real x) or x, from the host taps and the host Hilbert FIR."""
    from mercury_amd import host_hf_channel_taps, host_hilbert_taps
    W, n = x.shape
    real = not np.iscomplexobj(x)
    h = host_hilbert_taps()
    M = (h.size - 1) // 2
    t = (t0 + np.arange(n)) / fs
    rot = np.exp(2j * np.pi * ch.freq_offset_hz * t)
    out = np.zeros_like(x)
    for w in range(W):
        a = x[w] + 1j * np.convolve(x[w], h)[M: M + n] if real else x[w]
        g = host_hf_channel_taps(ch, fs, seed, r0 + w, n, t0=t0)
        y = np.zeros(n, np.complex128)
        for k in range(ch.n_paths):
            d = int(round(ch.delay_ms[k] * fs / 1000.0))
            y[d:] += g[k, d:] * a[: n - d]
        y *= rot
        out[w] = y.real if real else y
    return out


def _ld(v):
    return np.asarray(v, np.longdouble)


def _two_pi():
    """2 pi to the 64 bits of an x87 extended: the double nearest pi plus what it leaves."""
    assert np.finfo(np.longdouble).nmant >= 63, "the reference needs an 80-bit long double"
    return 2 * (_ld(3.141592653589793) + _ld(1.2246467991473532e-16))


def path_delays(ch, fs):
    return [int(round(ch.delay_ms[k] * fs / 1000.0)) for k in range(ch.n_paths)]


def path_amps(ch):
    """(amplitude of one sinusoid, number of sinusoids) per path: g_k's normalisation, 1/sqrt(32) included for a fading path."""
    gains = np.array([ch.gain_db[k] for k in range(ch.n_paths)])
    norm = np.sqrt(np.sum(10.0 ** (gains / 10.0)))
    out = []
    for k in range(ch.n_paths):
        a = 10.0 ** (gains[k] / 20.0) / norm
        out.append((a / np.sqrt(32.0), 32) if ch.spread_hz[k] > 0 else (a, 1))
    return out


def _draws(ch, seed, r, k):
    """(frequencies, phases) of path k's sinusoids: 32 for a fading path, (shift, 0) for a static one."""
    from mercury_amd import host_hf_channel_draws
    f, ph = host_hf_channel_draws(ch, seed, r, k)
    return (f, ph) if ch.spread_hz[k] > 0 else (f[:1], ph[:1])


def _omega_phi(ch, seed, r, k, offset):
    f, ph = _draws(ch, seed, r, k)
    return _two_pi() * (_ld(f) + _ld(offset)), _ld(ph)


def _phases(ch, fs, seed, r, idx, t0, k, offset):
    """2 pi (f + offset) t_i + phi in 80-bit for the sample indices idx: [len(idx), ns]"""
    om, ph = _omega_phi(ch, seed, r, k, offset)
    t = (_ld(int(t0)) + _ld(idx)) / _ld(fs)
    return np.multiply.outer(t, om) + ph


def _phi_max(ch, fs, seed, r, n, t0, k, offset):
    """max |2 pi f t_i + phi| over the n samples and the path's sinusoids: the phase is linear in i, so it is at one of the two ends."""
    return float(np.max(np.abs(_phases(ch, fs, seed, r, np.array([0, n - 1]), t0, k, offset))))


BLOCK = 256


def taps_longdouble(ch, fs, seed, r, n, t0=0, offset=0.0, block=BLOCK):
    """g_k(t_i) of DESIGN.md §6.1, complex128 [n_paths, n], t_i = (t0 + i) / fs: time, phase, sine and cosine in 80-bit, rounded to double
    at the end. offset: a frequency added to every sinusoid's (the channel's frequency offset folded in, as the kernel does).
    block = None evaluates every sample's sine and cosine directly. Otherwise t_i = (t0 + block b) / fs + j / fs and the angle-addition
    formula, in 80-bit as well, give the same sums from n / block + block sines per sinusoid (three more 2^-64 roundings): a capture window
    of 92,480 samples in a third of a second, not three."""
    amps = path_amps(ch)
    g = np.zeros((ch.n_paths, n), np.complex128)
    for k in range(ch.n_paths):
        a = _ld(amps[k][0])
        if block is None:
            p = _phases(ch, fs, seed, r, np.arange(n), t0, k, offset)
            c, s = np.cos(p).sum(axis=1), np.sin(p).sum(axis=1)
        else:
            om, _ = _omega_phi(ch, seed, r, k, offset)
            pa = _phases(ch, fs, seed, r, np.arange(0, n, block), t0, k, offset)          # anchors [nb, ns]
            pr = np.multiply.outer(_ld(np.arange(block)) / _ld(fs), om)                    # rotations [block, ns]
            ca, sa, cr, sr = np.cos(pa), np.sin(pa), np.cos(pr), np.sin(pr)
            c = (ca @ cr.T - sa @ sr.T).ravel()[:n]
            s = (sa @ cr.T + ca @ sr.T).ravel()[:n]
        g[k] = (a * c).astype(np.float64) + 1j * (a * s).astype(np.float64)
    return g


def analytic(x):
    """a = x + j (h * x) with the host Hilbert FIR for a real signal (zero outside [0, n)), x itself for a complex one."""
    from mercury_amd import host_hilbert_taps
    if np.iscomplexobj(x):
        return x
    h = host_hilbert_taps()
    M = (h.size - 1) // 2
    return x + 1j * np.convolve(x, h)[M: M + x.size]


def channel_longdouble(x, ch, seed, r0, fs, t0=0):
    """_numpy_channel with taps_longdouble's gains (the frequency offset inside them): [W, n] real or complex, signal w is realisation r0 + w."""
    W, n = x.shape
    real = not np.iscomplexobj(x)
    delays = path_delays(ch, fs)
    out = np.zeros_like(x)
    for w in range(W):
        a = analytic(x[w])
        g = taps_longdouble(ch, fs, seed, r0 + w, n, t0, offset=ch.freq_offset_hz)
        y = np.zeros(n, np.complex128)
        for k, d in enumerate(delays):
            if d < n:
                y[d:] += g[k, d:] * a[: n - d]
        out[w] = y.real if real else y
    return out


def phase_bound(ch, fs, seed, r, n, t0, a, rms):
    """The per-sample error budget [n] of a double-precision evaluation of realisation r on the analytic signal a[n] (module docstring).
    rms: the RMS of the reference output, which the 1e-10 term scales with as in tests/test_gpu_hf_channel.py."""
    amps, delays = path_amps(ch), path_delays(ch, fs)
    mag = np.abs(a)
    b = np.full(n, 1e-10 * float(rms))
    for k, d in enumerate(delays):
        if d < n:
            phi_max = _phi_max(ch, fs, seed, r, n, t0, k, ch.freq_offset_hz)
            b[d:] += amps[k][0] * amps[k][1] * PHASE_ROUNDINGS * U * phi_max * mag[: n - d]
    return b


def tap_bound(ch, fs, seed, r, n, t0):
    """(budget [n_paths], Phi [n_paths]) for the tap gains themselves (the host twin's g_k against taps_longdouble, no signal and no
    frequency offset): per sinusoid the phase budget and 2 u for a libm sine or cosine within one ulp; (ns - 1) additions whose partial
    sums are at most ns, u each; one more u for the product with the amplitude."""
    out, phis = [], []
    for k, (amp, ns) in enumerate(path_amps(ch)):
        phi_max = _phi_max(ch, fs, seed, r, n, t0, k, 0.0)
        out.append(amp * (ns * (PHASE_ROUNDINGS * U * phi_max + 2 * U) + (ns - 1) * ns * U + ns * U))
        phis.append(phi_max)
    return np.array(out), np.array(phis)


def worst_ratio(got, x, ch, seed, r0, fs, t0=0, ref=None):
    """max over signals and samples of |got - channel_longdouble| / phase_bound, for got shaped like x [W, n]."""
    W, n = x.shape
    ref = channel_longdouble(x, ch, seed, r0, fs, t0) if ref is None else ref
    worst = 0.0
    for w in range(W):
        b = phase_bound(ch, fs, seed, r0 + w, n, t0, analytic(x[w]), np.sqrt(np.mean(np.abs(ref[w]) ** 2)))
        worst = max(worst, float(np.max(np.abs(got[w] - ref[w]) / b)))
    return worst

"""What the tests of the separable Wiener estimator (include/mercury_estimator.h: MGPU_RUNG_WIENER) share: a numpy restatement of its tables
and of the estimate written from the header's rule, the column interpolation behind it (interpolator.cc:163-254) so that an estimate at the
pilots can go through host_demap_csi, and two-path frames with a delay of their own."""
import functools

import numpy as np

from demapper_csi_ref import llr_src
from oraclelib import Oracle, noise_amp_for

DY5 = dict(Dy=5, Nsymb=20)
DEFAULT = dict(tau_min_us=-333.33, tau_max_us=2333.33, doppler_hz=0.5, snr_db=0.0)
# the designs the table and twin tests cover: the default, both ends of the SNR range (40 dB is the worst conditioned), another interval
DESIGNS = [dict(DEFAULT), dict(DEFAULT, snr_db=40.0), dict(DEFAULT, snr_db=-20.0), dict(tau_min_us=-100.0, tau_max_us=1200.0, doppler_hz=2.0, snr_db=5.0)]
GEOMETRIES = [(0, None), (8, None), (11, None), (13, None), (8, DY5)]


def design(**kw):
    return dict(DEFAULT, **kw)


def carrier_bin(c, Nc=50):
    """carrier c's FFT bin relative to DC (the zero padder skips DC: the lower half sits at the negative bins)"""
    return np.where(np.asarray(c) < Nc // 2, np.asarray(c) - Nc // 2, np.asarray(c) - Nc // 2 + 1)


def np_tables(orc, d):
    """-> dict(time: {rows tuple: A}, freq: {carriers tuple: B}, cond: the largest condition number of a regularised correlation matrix,
    s2, s2b). np.linalg.inv (LAPACK) stands for the library's own elimination."""
    Nc, Ns = orc.Nc, orc.Nsymb
    types = orc.frame_types().reshape(Ns, Nc) != 0
    boost = float(np.abs(orc.pilot_seq()[0].real))
    tau0, tau1 = d["tau_min_us"] * 12000.0 / 1e6, d["tau_max_us"] * 12000.0 / 1e6
    Ts = 272.0 / 12000.0
    s2 = 10.0 ** (-d["snr_db"] / 10.0) / (boost * boost)
    cond = 0.0
    time, gain_sq = {}, {}
    for c in range(Nc):
        rows = tuple(int(r) for r in np.flatnonzero(types[:, c]))
        if not rows or rows in time:
            continue
        r = np.array(rows, np.float64)
        Rt = np.sinc(2.0 * d["doppler_hz"] * Ts * (r[:, None] - r[None, :]))
        M = Rt + s2 * np.eye(len(rows))
        cond = max(cond, np.linalg.cond(M))
        A = Rt @ np.linalg.inv(M)
        A = A / np.einsum("ik,ki->i", A, Rt)[:, None]
        gain_sq[rows] = (A * A).sum(axis=1)
        time[rows] = A * (1.0 / boost)
    acc, n = 0.0, 0
    for i in range(Ns):
        for c in range(Nc):
            if types[i, c]:
                rows = tuple(int(r) for r in np.flatnonzero(types[:, c]))
                acc += gain_sq[rows][rows.index(i)]
                n += 1
    s2b = s2 * (acc / n)
    freq = {}
    for i in range(Ns):
        cars = tuple(int(c) for c in np.flatnonzero(types[i]))
        if not cars or cars in freq:
            continue
        k = carrier_bin(np.array(cars), Nc).astype(np.float64)
        dk = k[:, None] - k[None, :]
        Rf = np.sinc((tau1 - tau0) * dk / 256.0) * np.exp(-2j * np.pi * dk * (tau0 + tau1) / 512.0)
        M = Rf + s2b * np.eye(len(cars))
        cond = max(cond, np.linalg.cond(M))
        B = Rf @ np.linalg.inv(M)
        B = B / np.einsum("ik,ki->i", B, Rf).real[:, None]
        freq[cars] = B
    return dict(time=time, freq=freq, cond=float(cond), s2=s2, s2b=s2b)


def np_estimate(orc, grid, tables):
    """the rule on one frame grid with the restatement's tables (matrix products: the sums in numpy's grouping) -> Hp [nPilots]"""
    Nc, Ns = orc.Nc, orc.Nsymb
    types = orc.frame_types().reshape(Ns, Nc) != 0
    sign = np.zeros((Ns, Nc))
    sign[types] = np.sign(orc.pilot_seq().real)
    g = np.asarray(grid, np.complex128).reshape(Ns, Nc)
    t = np.zeros((Ns, Nc), np.complex128)
    for c in range(Nc):
        rows = np.flatnonzero(types[:, c])
        if rows.size:
            # the sign and the real taps applied per component, as the rule has them: a complex product with (x + 0j) would turn an
            # infinite component into a NaN in the other one
            A = tables["time"][tuple(int(r) for r in rows)]
            col = np.zeros(rows.size, np.complex128)
            col.real = A @ (g.real[rows, c] * sign[rows, c])
            col.imag = A @ (g.imag[rows, c] * sign[rows, c])
            t[rows, c] = col
    H = np.zeros((Ns, Nc), np.complex128)
    for i in range(Ns):
        cars = np.flatnonzero(types[i])
        if cars.size:
            # four real products, for the same reason (a BLAS complex product scales by alpha = 1 + 0j at the end)
            B, row = tables["freq"][tuple(int(c) for c in cars)], t[i, cars]
            out = np.zeros(cars.size, np.complex128)
            out.real = B.real @ row.real - B.imag @ row.imag
            out.imag = B.real @ row.imag + B.imag @ row.real
            H[i, cars] = out
    return H[types]


def interpolate_cols(orc, Hp):
    """interpolate_linear_col (interpolator.cc:163-254) as the front-end applies it per data cell: between the nearest pilot rows above and
    below in the cell's column, beyond the column's first / last pilot row from its first / last two; a + ((b - a) * (i - ia)) / (ib - ia)
    per component, the kernel's operations in its order. -> the estimate at every cell [Nsymb * Nc]"""
    Nc, Ns = orc.Nc, orc.Nsymb
    types = orc.frame_types().reshape(Ns, Nc) != 0
    H = np.zeros((Ns, Nc), np.complex128)
    H[types] = Hp
    with np.errstate(all="ignore"):                                        # (an estimate may hold Inf and NaN: the degenerate-frame tests)
        for c in range(Nc):
            rows = np.flatnonzero(types[:, c])
            for i in range(Ns):
                if types[i, c]:
                    continue
                k = int(np.searchsorted(rows, i))
                k = min(max(k, 1), rows.size - 1)
                ia, ib = int(rows[k - 1]), int(rows[k])
                a, b = H[ia, c], H[ib, c]
                m, q = float(i - ia), float(ib - ia)
                H[i, c] = complex(a.real + ((b.real - a.real) * m) / q, a.imag + ((b.imag - a.imag) * m) / q)
    return H.ravel()


@functools.lru_cache(maxsize=None)
def two_path_delay(cfg, esn0, delay, frames):
    """demapper_csi_ref.two_path with the second path `delay` samples late (0: one path, AWGN): clean frames of the generator (seed 5) through two
    equal static paths, each divided by sqrt 2, phases and noise from default_rng(7) in that function's draw order (the phases are drawn for
    one path too), noise 16 * noise_amp_for(esn0) per component. -> dict(orc: the oracle with the 5 x 5 LS window, bb [frames, samples],
    bits: each clean frame's message bits, ref: the oracle's rx of each noisy frame)"""
    orc = Oracle(cfg, 50, explicit=dict(ls_window=5))
    rng = np.random.default_rng(7)
    amp = 16.0 * noise_amp_for(esn0)
    bb, bits = [], []
    for f in range(frames):
        x, _ = orc.gen_frame(5, f, 0.0, 0)
        bits.append(orc.rx(x)["bits"].copy())
        ph = np.exp(1j * rng.uniform(0, 2 * np.pi, 2))
        if delay > 0:
            y = ph[0] * x
            y[delay:] += ph[1] * x[:-delay]
            y /= np.sqrt(2.0)
        else:
            y = ph[0] * x
        y += amp * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
        bb.append(y)
    bb = np.stack(bb)
    ref = [orc.rx(bb[f]) for f in range(frames)]
    return dict(orc=orc, bb=bb, bits=bits, ref=ref)


def decode_with(orc, grid, H):
    """a frame grid and an estimate at every cell through the library's channel-aware demapper twin and the oracle's decoder
    -> (llr_demod, llr_ldpc, bits, iterations)"""
    from mercury_amd import host_demap_csi
    llr, _ = host_demap_csi(orc.cfg, grid, H, explicit=dict(ls_window=5))
    llr_ldpc = llr[llr_src(orc)]
    bits, it = orc.ldpc_decode(llr_ldpc)
    return llr, llr_ldpc, bits, it


@functools.lru_cache(maxsize=None)
def value_counts(cfg, esn0, delay, frames, snr_db):
    """frames of two_path_delay whose bits come out right -> (with the 5 x 5 oracle estimate, with the Wiener twin's estimate of design
    SNR snr_db), both through host_demap_csi and the oracle's decoder; and the per-frame verdicts of the Wiener chain"""
    from mercury_amd import host_wiener_estimate
    t = two_path_delay(cfg, esn0, delay, frames)
    orc = t["orc"]
    ls_ok, w_ok = [], []
    for f in range(frames):
        ref = t["ref"][f]
        ls = ref["H_noamp"] if orc.amp_restore else ref["H"]
        ls_ok.append(np.array_equal(decode_with(orc, ref["grid"], ls)[2], t["bits"][f]))
        Hp = host_wiener_estimate(cfg, ref["grid"], design(snr_db=snr_db))
        w_ok.append(np.array_equal(decode_with(orc, ref["grid"], interpolate_cols(orc, Hp))[2], t["bits"][f]))
    return int(np.sum(ls_ok)), int(np.sum(w_ok)), tuple(bool(v) for v in w_ok)

"""What the tests of the channel-aware demapper (include/mercury_demapper.h) share: a numpy restatement of its rule on the CPU oracle's
stage outputs, the receive gathers restated from the interleaver's definition (interleaver.cc:77-109, telecom_system.cc:1300-1308), the
oracle's integer tail behind the decoder, and the two-path frames on which the plain demapper fails and the weighted one decodes."""
import functools

import numpy as np

from oraclelib import Oracle, noise_amp_for

DY5 = dict(Dy=5, Nsymb=20)
CASES = [(0, None), (8, None), (11, None), (13, None), (16, None), (8, DY5)]


def _deint_src(n, bs):
    src = np.arange(n)
    nb = n // bs
    i, j = np.meshgrid(np.arange(nb), np.arange(bs), indexing="ij")
    src[: nb * bs] = (j * nb + i).ravel()
    return src


def sym_src(orc):
    """grid cell of demapped symbol k: deframer (the first nData data cells) + time/frequency de-interleaver"""
    data_cell = np.flatnonzero(orc.frame_types() == 0)[: orc.nData]
    return data_cell[_deint_src(orc.nData, orc.tf_blk)]


def llr_src(orc):
    """index into the demapper's LLR vector of decoder input p: bit de-interleaver + shortening re-pack"""
    bd = _deint_src(orc.nBits, orc.bit_blk)
    p = np.arange(orc.N)
    d = np.where(p < orc.nReal, p, np.where(p < orc.nReal + orc.nVirtual, p - orc.nReal, p - orc.nVirtual))
    return bd[d]


def full_estimate(orc, ref):
    """the oracle's channel estimate at every cell before restore_channel_amplitude"""
    return ref["H_noamp"] if orc.amp_restore else ref["H"]


def np_cdiv(n, d):
    """fe_math.h's cdiv (libgcc's __divdc3 main path) component-wise in real numpy arithmetic, operation for operation: the operands
    swapped where |d.re| < |d.im|, one ratio, the same five operations. Every numpy operation is one IEEE double operation, so this is
    the equaliser's division bit for bit, NaN where it gives NaN."""
    a, b, c, dd = n.real, n.imag, d.real, d.imag
    with np.errstate(all="ignore"):
        sw = np.abs(c) < np.abs(dd)
        p, q = np.where(sw, c, dd), np.where(sw, dd, c)
        ratio = p / q
        denom = (p * ratio) + q
        u, v = np.where(sw, a, b), np.where(sw, b, a)
        x = ((u * ratio) + v) / denom
        t = v * ratio
        y = np.where(sw, t - a, b - t) / denom
    return x, y


def np_maxlog(orc, er, ei, scale):
    """the demapping both twins share: squared distances to the constellation in double narrowed to float, per bit the running minima taken
    with np.fmin (which keeps the minimum on a NaN distance, as std::fmin does) from +Inf in constellation order, LLR = scale * (d1 - d0)
    in float. er, ei: the equalised symbols' components [nData]; scale: float32 [nData]. -> llr_demod float32 [nBits]"""
    cons = orc.constellation()
    bps = orc.bits_per_symbol
    d0 = np.full((bps, er.size), np.inf, np.float32)
    d1 = np.full((bps, er.size), np.inf, np.float32)
    with np.errstate(all="ignore"):
        for j in range(orc.M):
            dr, di = er - cons[j].real, ei - cons[j].imag
            D = (dr * dr + di * di).astype(np.float32)
            for b in range(bps):
                side = d1 if (j >> b) & 1 else d0
                side[b] = np.fmin(side[b], D)
        llr = np.zeros((er.size, bps), np.float32)
        for b in range(bps):
            llr[:, bps - 1 - b] = scale * (d1[b] - d0[b])
    return llr.ravel()


def np_sigma2(orc, grid, H):
    """(the pilots' residuals |g - h x|^2 in pilot order, their serial sum over nPilots) - np.cumsum adds one term after the other"""
    pilots = np.flatnonzero(orc.frame_types() != 0)
    x = orc.pilot_seq().real
    g, h = grid[pilots], H[pilots]
    with np.errstate(all="ignore"):
        dr, di = g.real - h.real * x, g.imag - h.imag * x
        r = dr * dr + di * di
        return r, float(np.cumsum(r)[-1] / float(orc.nPilots))


def np_demap_csi(orc, grid, H):
    """the rule in numpy: (llr_demod float32 [nBits], sigma2). Exact: the division is np_cdiv, the minima np_maxlog's, the scale formed as
    the twin forms it, (float32(1) / float32(sigma2)) * wf - so it equals mgpu_host_demap_csi bit for bit, NaN where it gives NaN, on
    degenerate grids too (tests/test_frontend_degenerate_host.py)."""
    grid, H = np.asarray(grid, np.complex128).ravel(), np.asarray(H, np.complex128).ravel()
    _, sigma2 = np_sigma2(orc, grid, H)
    src = sym_src(orc)
    hs = H[src]
    er, ei = np_cdiv(grid[src], hs)
    with np.errstate(all="ignore"):
        wf = (hs.real * hs.real + hs.imag * hs.imag).astype(np.float32)
        scale = (np.float32(1.0) / np.float64(sigma2).astype(np.float32)) * wf
    return np_maxlog(orc, er, ei, scale), sigma2


def same_bits(got, want):
    """bit for bit where `want` is a number - signs of zeros and infinities included -, NaN exactly where it is NaN (x86 and CDNA differ in
    the sign bit of a generated NaN, so NaNs are compared as positions)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind == "c":
        got, want = got.view(got.real.dtype), want.view(want.real.dtype)
    nan = np.isnan(want)
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(bits), want[~nan].view(bits)))


def llr_tol(ref):
    return 1e-5 * np.maximum(1.0, np.abs(np.asarray(ref, np.float64)))


def tail(orc, bits):
    """what follows the decoder: de-scrambling, bit_to_byte, CRC -> (payload bytes uint8, crc, all_zeros, message_decoded)"""
    nreal = orc.nReal
    desc = np.asarray(bits[:nreal], np.int32) ^ orc.scrambler()[:nreal]
    packed = np.zeros((nreal + 7) // 8, np.int32)
    for i in range(nreal):
        packed[i // 8] |= int(desc[i]) << (i % 8)
    all_zeros = int(not packed[: nreal // 8].any())
    crc = 0 if all_zeros else orc.crc16(packed[: nreal // 8])
    return packed.astype(np.uint8), crc, all_zeros, int(not (all_zeros or crc != 0))


@functools.lru_cache(maxsize=None)
def two_path(cfg, esn0, frames=32):
    """`frames` clean frames of the generator (seed 5) through two equal static paths 12 samples apart, each divided by sqrt 2, phases from
    default_rng(7); noise 16 * noise_amp_for(esn0) per component (16 is the oracle's 1 / sqrt(Nfft) scale, which its own channel applies
    internally). -> dict(orc: the oracle with the 5 x 5 LS window, bb, bits: each clean frame's message bits, ref: the oracle's rx of each
    noisy frame, plain_ok: whether the oracle alone recovers the bits)."""
    orc = Oracle(cfg, 50, explicit=dict(ls_window=5))
    rng = np.random.default_rng(7)
    amp = 16.0 * noise_amp_for(esn0)
    bb, bits = [], []
    for f in range(frames):
        x, _ = orc.gen_frame(5, f, 0.0, 0)
        bits.append(orc.rx(x)["bits"].copy())
        ph = np.exp(1j * rng.uniform(0, 2 * np.pi, 2))
        y = ph[0] * x
        y[12:] += ph[1] * x[:-12]
        y /= np.sqrt(2.0)
        y += amp * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
        bb.append(y)
    bb = np.stack(bb)
    ref = [orc.rx(bb[f]) for f in range(frames)]
    plain_ok = np.array([np.array_equal(ref[f]["bits"], bits[f]) for f in range(frames)])
    return dict(orc=orc, bb=bb, bits=bits, ref=ref, plain_ok=plain_ok)


@functools.lru_cache(maxsize=None)
def two_path_twin(cfg, esn0, frames=32):
    """the library's host twin on those frames, its LLRs through llr_src into the oracle's decoder: per frame (llr_ldpc, bits, iterations)"""
    from mercury_amd import host_demap_csi
    t = two_path(cfg, esn0, frames)
    orc, src = t["orc"], llr_src(t["orc"])
    out = []
    for f in range(frames):
        llr, _ = host_demap_csi(cfg, t["ref"][f]["grid"], full_estimate(orc, t["ref"][f]), explicit=dict(ls_window=5))
        llr_ldpc = llr[src]
        bits, it = orc.ldpc_decode(llr_ldpc)
        out.append((llr_ldpc, bits, it))
    return out

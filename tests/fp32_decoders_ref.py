"""numpy models of the two fp32 LDPC decoders (mercury_amd/csrc/ldpc.hip: spa_fast_decode<512, RULE>), of the rule each kernel itself
evaluates - not of the fp64 sum-product decoder the other tests measure them against.

The models read the Tanner graph from the table blob (mercury_amd/data/mercury_ldpc_tables.bin) and nothing else of the project:
  * minsum_ref: normalised min-sum in float32, operation for operation what the kernel does - it must give the kernel's bits and counts;
  * spa_fast_ref(dtype=float64): the kernel's tanh rule with the kernel's clamps in double precision ("the model");
  * spa_fast_ref(dtype=float32): the same in float32 with the kernel's own form of the others' product (the check's total times the
    reciprocal of the own factor), optionally with every transcendental's result moved by up to an ulp ("the emulation"). The distance
    between model and emulation says which posteriors the rounding of an fp32 evaluation can push across zero.

What both tests of these models share (the operating points, the LLR batches with their seeds) is at the end of the file."""
import functools
import os
import struct

import numpy as np

N = 1600
BLOB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mercury_amd", "data", "mercury_ldpc_tables.bin")
# Es/N0 (dB) of BPSK LLRs a little above each rate's threshold: batches around it mix early exits, late convergence and failures
BASE_DB = {100: -9.5, 200: -7.0, 300: -5.3, 400: -4.0, 500: -2.9, 600: -1.9, 800: -0.2, 1400: 5.6}
# the modes the decoder tests run and their K: every code rate (modes 5 and 8 share rate 6/16, with frames of their own)
CFG_K = {0: 100, 1: 200, 2: 300, 3: 400, 4: 500, 5: 600, 8: 600, 11: 800, 16: 1400}


@functools.lru_cache(maxsize=None)
def blob_codes():
    """K -> dict(K, P, N, E, cdeg[P], cflat[E], vdeg[N], vflat[E]): the blob's records as they are stored. cflat: the checks' variables,
    check-major, in row order; vflat: per variable the checks it belongs to, in slot order."""
    b = open(BLOB, "rb").read()
    assert b[:4] == b"MLDP"
    out = {}
    off = 12
    for _ in range(struct.unpack_from("<I", b, 8)[0]):
        k, P, n, E, _cw, _vw = struct.unpack_from("<6I", b, off)
        off += 24
        cdeg = np.frombuffer(b, "u1", P, off)
        off += P
        cflat = np.frombuffer(b, "<u2", E, off)
        off += 2 * E
        vdeg = np.frombuffer(b, "u1", n, off)
        off += n
        vflat = np.frombuffer(b, "<u2", E, off)
        off += 2 * E
        assert int(cdeg.sum()) == E and int(vdeg.sum()) == E
        out[k] = dict(K=k, P=P, N=n, E=E, cdeg=cdeg, cflat=cflat, vdeg=vdeg, vflat=vflat)
    return out


class Graph:
    """Index tables of one code. Edges are numbered check-major in row order (edge e belongs to check cchk[e] and variable cvar[e]).
    cmat[P, dmax]: the edges of every check, padded with E; vmat[N, vmax]: the edge behind slot j of every variable, padded with E;
    the edge of (variable v, slot j) is the position of v in check vflat[vptr[v] + j]."""

    def __init__(self, K):
        c = blob_codes()[K]
        self.K, self.P, self.N, self.E = K, c["P"], c["N"], c["E"]
        E = self.E
        self.cdeg = c["cdeg"].astype(np.int64)
        self.vdeg = c["vdeg"].astype(np.int64)
        self.cvar = c["cflat"].astype(np.int64)
        self.cptr = np.concatenate(([0], np.cumsum(self.cdeg)))
        self.vptr = np.concatenate(([0], np.cumsum(self.vdeg)))
        self.cchk = np.repeat(np.arange(self.P), self.cdeg)
        self.dmax, self.vmax = int(self.cdeg.max()), int(self.vdeg.max())
        pos = np.arange(E) - self.cptr[self.cchk]
        self.cmat = np.full((self.P, self.dmax), E, np.int64)
        self.cmat[self.cchk, pos] = np.arange(E)
        self.cvalid = self.cmat < E                       # row-major, its True entries are the edges 0 .. E-1 in order
        self.vmat = np.full((self.N, self.vmax), E, np.int64)
        vflat = c["vflat"].astype(np.int64)
        for v in range(self.N):
            for j in range(self.vdeg[v]):
                chk = vflat[self.vptr[v] + j]
                row = self.cvar[self.cptr[chk]:self.cptr[chk + 1]]
                hit = np.flatnonzero(row == v)
                assert hit.size >= 1, "the blob's two adjacency lists disagree"
                self.vmat[v, j] = self.cptr[chk] + hit[0]
        assert sorted(self.vmat[self.vmat < E]) == list(range(E))


@functools.lru_cache(maxsize=None)
def graph(K):
    return Graph(K)


def _odd_checks(g, negative):
    """negative [f, N] bool -> [f, P] bool: the checks with an odd number of negative posteriors"""
    pad = np.concatenate([negative[:, g.cvar], np.zeros((negative.shape[0], 1), bool)], axis=1)
    return np.bitwise_xor.reduce(pad[:, g.cmat], axis=2)


def _variable_sums(g, llr, R):
    """s = llr; s = s + R[slot j] for j ascending, in the arrays' type; a slot the variable does not have adds nothing (not even +0)"""
    s = llr.copy()
    Rp = np.concatenate([R, np.zeros((R.shape[0], 1), R.dtype)], axis=1)
    for j in range(g.vmax):
        s = np.where(g.vdeg > j, s + Rp[:, g.vmat[:, j]], s)
    return s


def minsum_ref(K, llr, max_iters, alpha=np.float32(0.8)):
    """Normalised min-sum, every operation in float32: (bits [F, K] uint8, iterations [F] int32, posteriors [F, 1600] float32).
    Look it = 1, 2, ... first tests the syndrome of `posterior < 0`: no odd check ends the frame with it - 1 iterations, a look past
    max_iters with max_iters + 1. A check's message to an edge: magnitude min(float32(m * alpha), 4096) with m the smallest |q| among the
    check's OTHER edges (+Inf when there is none), sign the parity of the others' sign bits; q = posterior - message."""
    g = graph(K)
    llr = np.ascontiguousarray(llr, np.float32).reshape(-1, N)
    alpha = np.float32(alpha)
    F, E = llr.shape[0], g.E
    post = llr.copy()
    R = np.zeros((F, E), np.float32)
    iters = np.full(F, -1, np.int32)
    open_ = np.ones(F, bool)
    inf_col = lambda f: np.full((f, 1), np.inf, np.float32)
    it = 0
    with np.errstate(over="ignore", invalid="raise"):
        while open_.any():
            it += 1
            idx = np.flatnonzero(open_)
            odd = _odd_checks(g, post[idx] < 0).any(axis=1)
            iters[idx[~odd]] = it - 1
            if it > max_iters:
                iters[idx[odd]] = max_iters + 1
                odd[:] = False
            open_[idx[~odd]] = False
            idx = idx[odd]
            if idx.size == 0:
                break
            q = post[idx][:, g.cvar] - R[idx]
            mag = np.concatenate([np.abs(q), inf_col(idx.size)], axis=1)[:, g.cmat]                       # [f, P, dmax], padding +Inf
            neg = np.concatenate([np.signbit(q), np.zeros((idx.size, 1), bool)], axis=1)[:, g.cmat]
            # the smallest magnitude among the others: of everything before the edge and everything behind it
            edge = np.full(mag.shape[:2] + (1,), np.inf, np.float32)
            before = np.concatenate([edge, np.minimum.accumulate(mag, axis=2)[:, :, :-1]], axis=2)
            behind = np.concatenate([np.minimum.accumulate(mag[:, :, ::-1], axis=2)[:, :, ::-1][:, :, 1:], edge], axis=2)
            m = np.minimum(before, behind)
            out = np.minimum((m * alpha).astype(np.float32), np.float32(4096.0))
            flip = np.bitwise_xor.reduce(neg, axis=2)[:, :, None] ^ neg
            out = np.where(flip, -out, out).astype(np.float32)
            R[idx] = out[:, g.cvalid]
            post[idx] = _variable_sums(g, llr[idx], R[idx])
    return (post[:, :K] < 0).astype(np.uint8), iters, post


def _ulp_moves(rng, x):
    """every element moved by -1, 0 or +1 float32 ulp, equally likely"""
    d = rng.integers(-1, 2, x.shape)
    up, down = np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))
    return np.where(d > 0, up, np.where(d < 0, down, x)).astype(np.float32)


T_LO, T_HI = 2.0 ** -30, 1.0 - 2.0 ** -24


def spa_fast_ref(K, llr, max_iters, dtype=np.float64, perturb=None, widened=False, messages=None, t_lo=T_LO):
    """The fp32 sum-product decoder's own rule: (bits [F, K] uint8, iterations [F] int32, looks), looks[l - 1] = the posteriors [F, 1600]
    every frame had at look l (a frame that has left keeps the ones it left with). Schedule and count convention as minsum_ref.
        t = copysign(clip((1 - e) / (1 + e), 2^-30, 1 - 2^-24), q), e = exp(-|q|), q = posterior - message, an LLR of 0 enters as +0
        message = copysign(ln((1 + pa) / (1 - pa)), p), pa = min(|p|, 1 - 2^-24), p = the product of the check's other t
    dtype float64 ("the model"): the others' product in ascending row order. dtype float32 ("the emulation"): every operation rounded
    to float32 in the kernel's form - exp2(-log2(e) |q|), reciprocals instead of divisions, p = (the product of the whole check) *
    1 / (the own t), ln2 * log2 - and with perturb = seed the result of every exp2, reciprocal and log2 moved by -1, 0 or +1 ulp at
    random: hardware transcendentals are accurate to about an ulp, not correctly rounded.
    widened (float64 only): the fp64 decoder's clamps instead - t unclamped, p = +-1 replaced by +-0.9999999.
    t_lo: the lower clamp of |t| (the kernel's 2^-30; the host test shows with another value that an input is sensitive to it).
    messages: a list that receives, per look, the messages [F, E] (edges check-major) the look's posteriors were summed from."""
    g = graph(K)
    f32 = np.dtype(dtype) == np.float32
    assert not (widened and f32)
    rng = np.random.default_rng(perturb) if perturb is not None else None
    tr = (lambda x: _ulp_moves(rng, x)) if rng is not None else (lambda x: x)
    llr = np.ascontiguousarray(llr, np.float32).reshape(-1, N)
    llr = np.where(llr == 0, np.float32(0.0), llr).astype(dtype)
    ft = np.dtype(dtype).type
    F, E, one = llr.shape[0], g.E, ft(1.0)
    post = llr.copy()
    R = np.zeros((F, E), dtype)
    iters = np.full(F, -1, np.int32)
    open_ = np.ones(F, bool)
    looks = []
    it = 0
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        while open_.any():
            it += 1
            looks.append(post.copy())
            if messages is not None:
                messages.append(R.copy())
            idx = np.flatnonzero(open_)
            odd = _odd_checks(g, post[idx] < 0).any(axis=1)
            iters[idx[~odd]] = it - 1
            if it > max_iters:
                iters[idx[odd]] = max_iters + 1
                odd[:] = False
            open_[idx[~odd]] = False
            idx = idx[odd]
            if idx.size == 0:
                break
            q = post[idx][:, g.cvar] - R[idx]
            if f32:
                x = (np.float32(-1.44269504088896341) * np.abs(q)).astype(np.float32)
                e = tr(np.exp2(x.astype(np.float64)).astype(np.float32))
                rc = tr((1.0 / (one + e).astype(np.float64)).astype(np.float32))
                a = ((one - e) * rc).astype(np.float32)
            else:
                e = np.exp(-np.abs(q))
                a = (one - e) / (one + e)
            if not widened:
                a = np.clip(a, ft(t_lo), ft(T_HI))
            t = np.copysign(a, q)
            tp = np.concatenate([t, np.ones((idx.size, 1), dtype)], axis=1)[:, g.cmat]                    # [f, P, dmax], padding 1
            if f32:
                total = np.ones(tp.shape[:2], np.float32)
                for i in range(g.dmax):
                    total = (total * tp[:, :, i]).astype(np.float32)
                own = tr((1.0 / tp.astype(np.float64)).astype(np.float32))
                p = (total[:, :, None] * own).astype(np.float32)
            else:
                p = np.ones_like(tp)
                for j in range(g.dmax):
                    for i in range(g.dmax):
                        if i != j:
                            p[:, :, j] *= tp[:, :, i]
            if widened:
                pa = np.where(np.abs(p) == 1.0, 0.9999999, np.abs(p))
            else:
                pa = np.minimum(np.abs(p), ft(T_HI))
            if f32:
                rc = tr((1.0 / (one - pa).astype(np.float64)).astype(np.float32))
                arg = ((one + pa) * rc).astype(np.float32)
                l2 = tr(np.log2(arg.astype(np.float64)).astype(np.float32))
                r = (np.float32(0.693147180559945309) * l2).astype(np.float32)
            else:
                r = np.log((one + pa) / (one - pa))
            R[idx] = np.copysign(r, p)[:, g.cvalid]
            post[idx] = _variable_sums(g, llr[idx], R[idx])
    return (post[:, :K] < 0).astype(np.uint8), iters, looks


def at_cap(iters, looks, k):
    """What a run capped at k iterations returns, from a run capped higher: (iterations [F], the posteriors [F, 1600] it decides from,
    the look each frame ends at). The trajectory does not depend on the cap; only where it is cut does."""
    it = np.where(iters <= k, iters, k + 1).astype(np.int32)
    last = np.minimum(it, k) + 1                               # a frame with `it` iterations is decided at look it + 1, an open one at look k + 1
    post = np.stack([looks[last[f] - 1][f] for f in range(len(it))])
    return it, post, last


# ---- the fragile set of the fp32 sum-product (what the rounding of an fp32 evaluation may decide either way) --------------------------
FRAGILE_FACTOR = 8.0                                           # a rule of the test, not a measurement of the kernel
EMULATION_SEEDS = (None, 1, 2, 3)
SPA_CAPS = (1, 2, 3, 5, 10)


def spa_fast_verdicts(K, llr, cap=max(SPA_CAPS), rule="variable"):
    """One run of the model and of every emulation at the highest cap; per cap k in SPA_CAPS a dict:
         iterations [F], bits [F, K] (the model's), compare [F, K] bool (information bits that are not fragile at the frame's last look),
         determinate [F] bool, D [looks] (the batch-wide distance); compare_batch / determinate_batch: the same by the other rule.
    rule "batch": D(look) = the largest |posterior(model) - posterior(emulation)| over all 1600 variables, all frames the model still has
    open at that look and all emulations; a variable is fragile at a look if |posterior(model)| < 8 D. A frame's count is determinate if
    each of its looks is robustly odd (some odd check has no fragile variable) or robustly clean (no odd check, no fragile variable).
    rule "variable" (what the tests use) asks more of the decoder, never less - its fragile set is a subset of the batch rule's: the
    batch-wide D is set by the few variables that receive messages near the 1 - 2^-24 clamp (there one ulp of p moves the message by
    ln 2), whose own posteriors are far from zero, and it would declare fragile every weakly decided variable of every frame of the batch.
    A variable's own D is the smaller of the batch's and
        max over the emulations |posterior(model) - posterior(emulation)| of THAT variable  +  sum over its messages of err(message),
        err = (1 + degree / 8) 2^-24 sinh(|message|): what a relative deviation of (1 + degree / 8) ulps in p moves the message by
        (|p| = tanh(|message| / 2), d/dp ln((1 + p) / (1 - p)) = 2 / (1 - p^2), so |p| 2 / (1 - p^2) = sinh(|message|)) - so that with the
        factor 8 a deviation of 8 + degree ulps in the check's product is covered even where none of the four emulations happened to
        show it (a product of `degree` rounded factors, each (1 - e) * rcp(1 + e) two to three roundings, is typically sqrt(degree) ulps
        off and at worst 2.5 degree)."""
    g = graph(K)
    msgs = []
    _, iters, looks = spa_fast_ref(K, llr, cap, np.float64, messages=msgs)
    emu = [spa_fast_ref(K, llr, cap, np.float32, perturb=s)[2] for s in EMULATION_SEEDS]
    F = len(iters)
    ulps = (1.0 + g.cdeg[g.cchk] / 8.0) * 2.0 ** -24
    D, fragile, robust = [], {"variable": [], "batch": []}, {"variable": [], "batch": []}
    for l in range(1, len(looks) + 1):
        m = looks[l - 1]
        o = np.minimum(iters, cap) + 1 >= l                   # a frame with `it` iterations (or cap + 1) takes looks 1 .. min(it, cap) + 1
        # an emulation that has ended every frame keeps its last posteriors
        dv = np.max([np.abs(m - lk[min(l, len(lk)) - 1].astype(np.float64)) for lk in emu], axis=0)
        batch = float(dv[o].max()) if o.any() else 0.0
        D.append(batch)
        err = np.concatenate([ulps * np.sinh(np.abs(msgs[l - 1])), np.zeros((F, 1))], axis=1)
        odd = _odd_checks(g, m < 0)
        for name, d in (("variable", np.minimum(dv + err[:, g.vmat].sum(axis=2), batch)), ("batch", np.full_like(dv, batch))):
            fr = np.abs(m) < FRAGILE_FACTOR * d
            fragile[name].append(fr)
            touched = np.concatenate([fr[:, g.cvar], np.zeros((F, 1), bool)], axis=1)[:, g.cmat].any(axis=2)
            robust[name].append((odd & ~touched).any(axis=1) | (~odd.any(axis=1) & ~fr.any(axis=1)))
    out = {}
    for k in [k for k in SPA_CAPS if k <= cap]:
        it, post, last = at_cap(iters, looks, k)
        out[k] = dict(iterations=it, bits=(post[:, :K] < 0).astype(np.uint8), D=np.array(D[:k + 1]))
        for name in ("variable", "batch"):
            det = np.array([all(robust[name][l - 1][f] for l in range(1, last[f] + 1)) for f in range(F)])
            frag_last = np.stack([fragile[name][last[f] - 1][f] for f in range(F)])
            suffix = "" if name == rule else "_" + name
            out[k]["compare" + suffix] = ~frag_last[:, :K]
            out[k]["determinate" + suffix] = det
    return out


# ---- inputs both test files use (the host test asserts on exactly these what the GPU test relies on) ------------------------------------
def codewords(K, F, seed):
    """F random codewords [F, 1600] uint8 from the oracle's encoder (cl_ldpc::encode restated); every check is satisfied"""
    import oraclelib
    cfg = min(c for c, v in CFG_K.items() if v == K)
    orc = oraclelib.Oracle(cfg, 50)
    assert orc.K == K
    rng = np.random.default_rng(seed)
    if F == 0:
        return np.zeros((0, N), np.uint8)
    cw = np.stack([orc.ldpc_encode(rng.integers(0, 2, K)) for _ in range(F)]).astype(np.uint8)
    assert not _odd_checks(graph(K), cw.astype(bool)).any() and cw.any(axis=1).all()
    return cw


def bpsk_llrs(K, offsets_db, seed, flip_half=True):
    """BPSK LLRs 2y / sigma^2, frame f at BASE_DB[K] + offsets_db[f]; every second frame carries a random non-zero codeword (the LLR signs
    flipped along it), the others the all-zero word. Returns (llr [F, 1600] float32, sent [F, 1600] uint8)."""
    rng = np.random.default_rng(seed)
    F = len(offsets_db)
    llr = np.zeros((F, N), np.float32)
    for f, off in enumerate(offsets_db):
        snr = 10 ** ((BASE_DB[K] + off) / 10)
        sigma = np.sqrt(1 / (2 * snr))
        llr[f] = (2 * (1.0 + sigma * rng.standard_normal(N)) / sigma ** 2).astype(np.float32)
    sent = np.zeros((F, N), np.uint8)
    if flip_half:
        sent[1::2] = codewords(K, len(sent[1::2]), seed + 1)
        llr = (llr * (1.0 - 2.0 * sent).astype(np.float32)).astype(np.float32)
    return llr, sent


MINSUM_CAPS = (1, 2, 5, 50)
MINSUM_MAIN_OFFSETS = tuple([-1.0] * 8 + [0.25 * i for i in range(8)] + [2.0] * 8)
SPA_OFFSETS = tuple([-1.0] * 8 + [1.5] * 8)


@functools.lru_cache(maxsize=None)
def minsum_main_llrs(cfg):
    llr, sent = bpsk_llrs(CFG_K[cfg], MINSUM_MAIN_OFFSETS, 1000 + cfg)
    llr.setflags(write=False)
    return llr, sent


@functools.lru_cache(maxsize=None)
def spa_llrs(cfg):
    llr, sent = bpsk_llrs(CFG_K[cfg], SPA_OFFSETS, 2000 + cfg)
    llr.setflags(write=False)
    return llr, sent


@functools.lru_cache(maxsize=None)
def spa_verdicts(cfg):
    return spa_fast_verdicts(CFG_K[cfg], spa_llrs(cfg)[0])


@functools.lru_cache(maxsize=None)
def minsum_edge_llrs(cfg):
    """name -> LLRs [F, 1600] float32 for the min-sum decoder's edge cases (all finite or +-Inf; no NaN, no denormal)"""
    K = CFG_K[cfg]
    rng = np.random.default_rng(3000 + cfg)
    noisy = bpsk_llrs(K, [0.5] * 4, 3100 + cfg)[0]
    out = {}
    # ties: three magnitudes only, so that almost every check has m1 == m2 and many q become +-0 after the first update
    out["ties"] = (rng.choice(np.array([0.5, 1.0, 2.0], np.float32), (8, N)) * np.where(rng.random((8, N)) < np.linspace(0.02, 0.16, 8)[:, None], np.float32(-1.0), np.float32(1.0))).astype(np.float32)
    z = np.zeros((2, N), np.float32)
    z[1] = -0.0                                                  # every LLR -0.0: decides 0 everywhere, a codeword at once
    out["zeros"] = z
    nz = noisy.copy()
    for f in range(4):
        nz[f, rng.choice(N, 60, replace=False)] = -0.0
        nz[f, rng.choice(N, 20, replace=False)] = 0.0
    out["negative_zero"] = nz
    big = np.sign(noisy).astype(np.float32)
    sat = np.stack([big[0] * np.float32(5000.0), big[1] * np.float32(3e38), noisy[2], noisy[3]]).astype(np.float32)
    where = rng.choice(N, 40, replace=False)
    sat[2, where] = np.where(noisy[2, where] > 0, np.inf, -np.inf).astype(np.float32)     # the sign the channel gave: mostly the sent one
    sat[3, rng.choice(N, 200, replace=False)] *= np.float32(5000.0)
    flips = rng.choice(N, 12, replace=False)                     # sign errors at full magnitude: the saturated messages have work to do
    sat[0, flips] = -sat[0, flips]
    sat[1, flips[:4]] = -sat[1, flips[:4]]
    out["saturation"] = sat
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def minsum_batch_llrs(cfg, F):
    """F distinct frames from below the threshold to well above it"""
    llr = bpsk_llrs(CFG_K[cfg], [(-1.0, 0.0, 0.5, 1.0, 2.0)[f % 5] for f in range(F)], 4000 + 7 * F + cfg)[0]
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def minsum_degree_one_llrs():
    """Rate 1/16 (its graph has a check of degree 1, whose message is the 4096 saturation itself) above the threshold: frames that converge,
    but late, so that the saturated message has walked down the accumulator chain"""
    llr = bpsk_llrs(100, [4.0] * 4 + [5.0] * 4, 5000)[0]
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def tail_llrs(cfg):
    """LLRs of whole frames (payload with its CRC, scrambled, through the oracle's front-end) at three Es/N0 above the mode's operating point
    and one far below, then the first 8 frames of the main batch (random words: their CRC fails)"""
    import oraclelib
    from conftest import OPERATING_ESN0
    orc = oraclelib.Oracle(cfg, 50)
    real = [orc.rx(orc.gen_frame(1234, i, oraclelib.noise_amp_for(snr))[0], oraclelib.FLAGS_BASEBAND_TEST | oraclelib.FLAG_NO_LDPC)["llr_ldpc"]
            for i, snr in enumerate((OPERATING_ESN0[cfg] + 0.5, OPERATING_ESN0[cfg] + 2.0, OPERATING_ESN0[cfg] + 4.0, -15.0))]
    llr = np.concatenate([np.stack(real).astype(np.float32), minsum_main_llrs(cfg)[0][12:20]])
    llr.setflags(write=False)
    return llr


CLAMP_CFG, CLAMP_LLR = 2, np.float32(-1.4e-6)


@functools.lru_cache(maxsize=None)
def spa_clamp_llrs():
    """Frames whose decisions after ONE iteration depend on the lower clamp of |t| (2^-30), at rate 3/16: (llr [4, 1600], probes [4, 8]).
    A probe is an information variable of degree d with LLR -1.4e-6 d. In each of its checks one other variable has LLR exactly 0, which
    enters the check's product as +2^-30, and the rest have LLR +20 (t at the upper clamp). Every message to the probe is then 2^-29; in
    float32 it vanishes next to 1 inside ln((1 + p) / (1 - p)), where a reciprocal that is an ulp off leaves at most 1.2e-7 per message,
    a twelfth of the probe's LLR: the probe stays negative, bit 1, outside the fragile set. With a clamp of 2^-20 every message is
    2^-19 = 1.9e-6, their sum outweighs the LLR, and the probe decides 0. All other LLRs: the all-zero word three dB above the threshold."""
    K = CFG_K[CLAMP_CFG]
    g = graph(K)
    rng = np.random.default_rng(6000)
    llr = bpsk_llrs(K, [3.0] * 4, 6001, flip_half=False)[0]
    vchecks = [set(g.cchk[g.vmat[v, :g.vdeg[v]]]) for v in range(N)]
    probes = np.zeros((4, 8), np.int64)
    for f in range(4):
        used_checks, taken, found = set(), set(), []
        for v in rng.permutation(K):
            if len(found) == 8:
                break
            around = set(int(u) for c in vchecks[v] for u in g.cvar[g.cptr[c]:g.cptr[c + 1]])
            if around & taken or vchecks[v] & used_checks:
                continue
            zeros = []
            for c in sorted(vchecks[v]):
                cand = [u for u in g.cvar[g.cptr[c]:g.cptr[c + 1]] if u != v and u not in taken and u not in zeros]
                if not cand:
                    break
                zeros.append(cand[-1])
            else:
                found.append(v)
                used_checks |= vchecks[v]
                taken |= around
                for c in vchecks[v]:
                    llr[f, g.cvar[g.cptr[c]:g.cptr[c + 1]]] = 20.0
                llr[f, zeros] = 0.0
                llr[f, v] = CLAMP_LLR * np.float32(g.vdeg[v])
        assert len(found) == 8
        probes[f] = found
    llr.setflags(write=False)
    return llr, probes


@functools.lru_cache(maxsize=None)
def spa_clamp_verdict():
    return spa_fast_verdicts(CFG_K[CLAMP_CFG], spa_clamp_llrs()[0], cap=1)[1]

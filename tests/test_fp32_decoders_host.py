"""CPU tests of the models the fp32 decoders are held to (tests/fp32_decoders_ref.py): a model is only worth trusting if something independent
holds it. The min-sum model against a deliberately naive scalar implementation, bit pattern for bit pattern; the sum-product model, with its
clamps widened to the fp64 decoder's, against the oracle's decoder; both on codewords, on pure noise and above the threshold; and, for the
exact seeds and shapes tests/test_gpu_fp32_decoders.py uses, the conditions that test relies on - how much the fragile set leaves out, that
the edge-case inputs are the edge cases they are named after, that the models produce no NaN on them."""
import numpy as np
import pytest

import fp32_decoders_ref as R
import oraclelib

CFGS = sorted(R.CFG_K)


def test_the_modes_cover_every_rate_of_the_blob_and_every_group_size():
    assert {oraclelib.Oracle(cfg, 50).K for cfg in CFGS} == set(R.blob_codes()) == set(R.BASE_DB)
    assert all(oraclelib.Oracle(cfg, 50).K == K for cfg, K in R.CFG_K.items())
    # the grouped layout gives a check of degree d a group of the next power of two >= max(d, 2) lanes: 2 ... 64 all occur
    sizes = set()
    for K in R.blob_codes():
        sizes |= {max(2, 1 << int(d - 1).bit_length()) for d in R.graph(K).cdeg}
    assert sizes == {2, 4, 8, 16, 32, 64}
    assert 1 in R.graph(100).cdeg and R.graph(1400).cdeg.max() == 46
    assert {int(R.graph(K).vdeg.max()) for K in R.blob_codes()} >= {6, 8, 9}


def _naive_minsum(K, llr, iterations, alpha):
    """Python loops over checks and edges, min over a list: posteriors after exactly `iterations` iterations"""
    g = R.graph(K)
    f32, inf, cap = np.float32, np.float32(np.inf), np.float32(4096.0)
    checks = [[int(v) for v in g.cvar[g.cptr[c]:g.cptr[c + 1]]] for c in range(g.P)]
    slots = [[] for _ in range(R.N)]                            # per variable (check, position) in slot order
    c = R.blob_codes()[K]
    off = 0
    for v in range(R.N):
        for j in range(int(c["vdeg"][v])):
            chk = int(c["vflat"][off + j])
            slots[v].append((chk, checks[chk].index(v)))
        off += int(c["vdeg"][v])
    post = [f32(x) for x in llr]
    msg = [[f32(0.0)] * len(row) for row in checks]
    with np.errstate(over="ignore"):
        for _ in range(iterations):
            new = []
            for ci, row in enumerate(checks):
                q = [f32(post[v] - msg[ci][j]) for j, v in enumerate(row)]
                out = []
                for j in range(len(row)):
                    others = [abs(q[i]) for i in range(len(row)) if i != j]
                    m = min(others) if others else inf
                    mag = min(f32(m * alpha), cap)
                    odd = sum(1 for i in range(len(row)) if i != j and np.signbit(q[i])) & 1
                    out.append(f32(-mag) if odd else f32(mag))
                new.append(out)
            msg = new
            for v in range(R.N):
                s = f32(llr[v])
                for chk, pos in slots[v]:
                    s = f32(s + msg[chk][pos])
                post[v] = s
    return np.array(post, np.float32)


@pytest.mark.parametrize("K", [100, 1400])
def test_minsum_model_equals_a_naive_scalar_implementation(K):
    """2 frames x 3 iterations below the threshold (still open at the cap, so the model's posteriors are those after exactly 3
    iterations), one of them with ties and zeros of both signs: the posteriors' bit patterns are equal."""
    cfg = min(c for c, k in R.CFG_K.items() if k == K)
    llr = np.stack([R.bpsk_llrs(K, [-2.5], 9000 + K)[0][0], R.minsum_edge_llrs(cfg)["ties"][7]]).copy()
    llr[1, 5:400:7] = -0.0
    llr[1, 6:400:11] = 0.0
    bits, iters, post = R.minsum_ref(K, llr, 3)
    assert (iters == 4).all()
    for f in range(2):
        want = _naive_minsum(K, llr[f], 3, np.float32(0.8))
        assert np.array_equal(post[f].view(np.uint32), want.view(np.uint32)), (K, f, int((post[f].view(np.uint32) != want.view(np.uint32)).sum()))
        assert np.array_equal(bits[f], (want[:K] < 0).astype(np.uint8))


@pytest.mark.parametrize("cfg", [2, 8])
def test_sum_product_model_with_the_fp64_clamps_is_the_oracles_decoder(cfg):
    """The float64 model with t unclamped and p = +-1 -> +-0.9999999 is the fp64 decoder's rule in another form ((1 - e) / (1 + e) for tanh,
    ln((1 + p) / (1 - p)) for 2 atanh): on 8 frames across the waterfall its bits and iteration counts are the oracle's. (The two forms
    round differently in the last place; a frame would differ only where a posterior is within that of zero, and none of these does.)"""
    K = R.CFG_K[cfg]
    llr = R.bpsk_llrs(K, [0.25 * i for i in range(8)], 7000 + cfg)[0]
    bits, iters, _ = R.spa_fast_ref(K, llr, 50, np.float64, widened=True)
    orc = oraclelib.Oracle(cfg, 50)
    for f in range(8):
        rb, ri = orc.ldpc_decode(llr[f])
        assert iters[f] == ri, (cfg, f, int(iters[f]), ri)
        assert np.array_equal(bits[f], rb.astype(np.uint8)), (cfg, f)
    assert (iters <= 50).any() and iters.max() >= 5


def _decoders(K):
    return (("minsum", lambda llr, cap: R.minsum_ref(K, llr, cap)[:2]),
            ("spa_fast", lambda llr, cap: R.spa_fast_ref(K, llr, cap, np.float64)[:2]),
            ("spa_fast emulation", lambda llr, cap: R.spa_fast_ref(K, llr, cap, np.float32, perturb=5)[:2]))


@pytest.mark.parametrize("cfg", [8, 16])
def test_models_on_codewords_on_noise_and_above_the_threshold(cfg):
    """A noiseless codeword takes 0 iterations; -15 dB noise takes max_iters + 1 at caps of 1 and 5; 8 frames 1.5 dB above the rate's
    threshold decode to the sent word. (Rates 6/16 and 14/16: at the low rates normalised min-sum's own threshold lies further up - at rate
    1/16 most frames 2 dB above BASE_DB stay open - so "both decode" holds only from the middle rates on.)"""
    K = R.CFG_K[cfg]
    cw = R.codewords(K, 4, 8000 + cfg)
    clean = ((1.0 - 2.0 * cw) * 6.0).astype(np.float32)
    rng = np.random.default_rng(8100 + cfg)
    sigma = np.sqrt(1 / (2 * 10 ** -1.5))
    noise = (2 * (1.0 + sigma * rng.standard_normal((4, R.N))) / sigma ** 2).astype(np.float32)
    good, sent = R.bpsk_llrs(K, [1.5] * 8, 8200 + cfg)
    assert sent[1::2].any(axis=1).all() and not sent[0::2].any()
    for name, dec in _decoders(K):
        bits, iters = dec(clean, 50)
        assert (iters == 0).all() and np.array_equal(bits, cw[:, :K]), (cfg, name)
        for cap in (1, 5):
            assert (dec(noise, cap)[1] == cap + 1).all(), (cfg, name, cap)
        bits, iters = dec(good, 50)
        assert (iters <= 50).all() and (iters >= 1).any() and np.array_equal(bits, sent[:, :K]), (cfg, name, iters.tolist())


# ---- what tests/test_gpu_fp32_decoders.py relies on, for its own seeds and shapes ---------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS)
def test_fragile_set_of_the_fp32_sum_product_stays_inside_its_caps(cfg):
    """Per cap k: fragile information bits <= 0.5 % of those compared, indeterminate frames <= 2 of 16 - and what the per-variable rule
    compares is a superset of what the batch-wide rule compares, its determinate frames a superset of that rule's."""
    verdicts = R.spa_verdicts(cfg)
    assert sorted(verdicts) == list(R.SPA_CAPS)
    for k, v in verdicts.items():
        fragile, frames = int((~v["compare"]).sum()), int((~v["determinate"]).sum())
        print(cfg, k, "fragile", fragile, "of", v["compare"].size, "indeterminate", frames, "batch rule:", int((~v["compare_batch"]).sum()),
              int((~v["determinate_batch"]).sum()), "D", ["%.2g" % d for d in v["D"]])
        assert fragile <= 0.005 * v["compare"].size, (cfg, k, fragile)
        assert frames <= 2, (cfg, k, frames)
        assert not (v["compare_batch"] & ~v["compare"]).any() and not (v["determinate_batch"] & ~v["determinate"]).any(), (cfg, k)
        assert len(v["iterations"]) == 16 and v["iterations"].max() <= k + 1 and (v["D"][1:] > 0).all()
    assert (verdicts[1]["iterations"] == 2).any()                # some frames are cut at the cap, and (but for rate 1/16, which needs longer) some converge
    assert (verdicts[10]["iterations"][8:] <= 10).any() or cfg == 0


def test_emulations_differ_from_each_other_and_from_the_model():
    """The perturbation does something: after 3 iterations no two emulations have the same posteriors, and none has the model's."""
    K = 600
    llr = R.spa_llrs(8)[0][:4]
    runs = [R.spa_fast_ref(K, llr, 3, np.float32, perturb=s)[2][-1].astype(np.float64) for s in R.EMULATION_SEEDS]
    runs.append(R.spa_fast_ref(K, llr, 3, np.float64)[2][-1])
    for i in range(len(runs)):
        for j in range(i):
            d = np.abs(runs[i] - runs[j]).max()
            assert 0 < d < 0.5, (i, j, d)


def test_probe_frames_decide_by_the_lower_clamp():
    llr, probes = R.spa_clamp_llrs()
    v = R.spa_clamp_verdict()
    K = R.CFG_K[R.CLAMP_CFG]
    rows = np.arange(len(llr))[:, None]
    assert v["determinate"].all() and v["compare"][rows, probes].all() and (v["bits"][rows, probes] == 1).all()
    assert (~v["compare"]).sum() <= 0.005 * v["compare"].size
    for dtype in (np.float32, np.float64):
        assert (R.spa_fast_ref(K, llr, 1, dtype)[0][rows, probes] == 1).all()
        assert (R.spa_fast_ref(K, llr, 1, dtype, t_lo=2.0 ** -20)[0][rows, probes] == 0).all()


@pytest.mark.parametrize("cfg", CFGS)
def test_minsum_inputs_are_what_they_are_named_after(cfg):
    K = R.CFG_K[cfg]
    g = R.graph(K)
    llr, sent = R.minsum_main_llrs(cfg)
    assert llr.shape == (24, R.N) and sent[1::2].any(axis=1).all() and not sent[0::2].any()
    _, it, post = R.minsum_ref(K, llr, 50)
    assert not np.isnan(post).any()
    assert (it == 51).any() or cfg >= 4, it.tolist()             # open frames at every cap (the high rates converge even a dB down: caps 1 and 2 cut them)
    assert (it <= 50).any() and R.minsum_ref(K, llr, 2)[1].max() == 3
    edge = R.minsum_edge_llrs(cfg)
    # ties: three magnitudes, so a check of degree d has a unique smallest magnitude with probability d (2^(d-1) + 1) / 3^d only (0.56 at
    # d = 3, 0.27 at d = 6, 0.02 at d = 15): the two smallest are equal in about half of the low rates' checks and nearly all of rate 14/16's,
    # and after the first update some q are +-0
    mag = np.concatenate([np.abs(edge["ties"]), np.full((8, 1), np.inf, np.float32)], axis=1)[:, np.where(g.cmat < g.E, g.cvar[np.minimum(g.cmat, g.E - 1)], R.N)]
    two = np.sort(mag, axis=2)[:, :, :2]
    share = (two[:, g.cdeg >= 3, 0] == two[:, g.cdeg >= 3, 1]).mean()
    assert share > (0.95 if K == 1400 else 0.4), (cfg, share)
    _, _, p1 = R.minsum_ref(K, edge["ties"], 1)
    assert ((p1 == 0).sum() > 0) or cfg == 16
    for name, x in edge.items():
        assert not np.isnan(x).any() and (x[x != 0] == 0).sum() == 0 and (np.abs(x[(x != 0) & np.isfinite(x)]) >= 2.0 ** -126).all(), (cfg, name)
        for cap in (2, 50):
            _, it, post = R.minsum_ref(K, x, cap)
            assert not np.isnan(post).any(), (cfg, name, cap)
            assert np.isfinite(post[np.isfinite(x)]).all(), (cfg, name, cap)
    assert (R.minsum_ref(K, edge["zeros"], 50)[1] == 0).all() and np.signbit(edge["zeros"][1]).all()
    assert np.isinf(edge["saturation"][2]).sum() == 40 and np.abs(edge["saturation"][1]).min() > 2.9e38
    nz = edge["negative_zero"]
    assert ((nz == 0) & np.signbit(nz)).sum() >= 200 and ((nz == 0) & ~np.signbit(nz)).sum() >= 40


def test_minsum_special_batches():
    it = R.minsum_ref(100, R.minsum_degree_one_llrs(), 50)[1]
    assert (it >= 5).sum() >= 4 and (it <= 50).sum() >= 4, it.tolist()
    assert len(set(R.minsum_ref(600, R.minsum_batch_llrs(8, 65), 50)[1].tolist())) >= 5
    assert len(np.unique(R.minsum_batch_llrs(8, 65), axis=0)) == 65
    for cfg in (0, 8, 16):
        orc = oraclelib.Oracle(cfg, 50)
        bits, it, _ = R.minsum_ref(R.CFG_K[cfg], R.tail_llrs(cfg), 50)
        ok = [int(not (z or crc != 0)) for _, crc, z in (oraclelib.payload_tail(orc, b) for b in bits)]
        assert 1 <= sum(ok) < len(ok), (cfg, ok)
    # alpha matters on the frames the alpha test uses: the four values give four different sets of posteriors
    for cfg in (8, 16):
        llr = R.minsum_main_llrs(cfg)[0][8:16]
        posts = [R.minsum_ref(R.CFG_K[cfg], llr, 3, np.float32(a))[2] for a in (0.8, 1.0, 0.75, 0.8125)]
        assert all(not np.array_equal(posts[i], posts[j]) for i in range(4) for j in range(i))

"""GPU tests of the two fp32 LDPC decoders (ldpc.hip: mgpu_ldpc_minsum_kernel_t512, mgpu_ldpc_spa_fast_kernel_t512, both spa_fast_decode<512,
RULE> on the grouped layout of tables.cpp) against models of the rule each of them evaluates (tests/fp32_decoders_ref.py), not against the
fp64 sum-product decoder, which is another algorithm.

Min-sum is exactly reproducible - float32 subtractions, integer minima, one multiplication, one saturation, additions in the variables'
slot order - so its bits and iteration counts must EQUAL the model's, frame for frame, at every iteration cap (a cap of k on a frame that
is still open exposes the sign of every information bit's posterior after exactly k iterations). The contract covers finite and infinite
LLRs and both zeros; NaN and denormal LLRs are not part of it and are left out.

The fp32 sum-product uses the hardware's exp2 / log2 / rcp and is not bit-reproducible: it is held to the float64 model of its own rule
wherever the model's posterior is not within rounding of zero (fp32_decoders_ref.spa_fast_verdicts; the margin is computed from the
references alone). tests/test_fp32_decoders_host.py checks the models themselves, and for these very inputs how much the margin leaves
out."""
import functools

import numpy as np
import pytest

import fp32_decoders_ref as R
import oraclelib

pytestmark = pytest.mark.gpu

CFGS = sorted(R.CFG_K)


def _decode(cfg, llr, decoder, cap, max_batch=None, **kw):
    from mercury_amd import RxPhy
    rx = RxPhy(cfg, max_iters=cap, decoder=decoder, max_batch=max_batch or max(32, len(llr)), **kw)
    try:
        bits, iters = rx.ldpc_decode(llr)
    finally:
        rx.close()
    return bits, iters


@functools.lru_cache(maxsize=None)
def _minsum_model(cfg, name, cap, alpha=0.8):
    llr = _minsum_inputs(cfg, name)
    bits, iters, post = R.minsum_ref(R.CFG_K[cfg], llr, cap, np.float32(alpha))
    assert np.isfinite(post[np.isfinite(llr)]).all() and not np.isnan(post).any()
    return bits, iters


def _minsum_inputs(cfg, name):
    if name == "main":
        return R.minsum_main_llrs(cfg)[0]
    if name == "degree_one":
        return R.minsum_degree_one_llrs()
    if name == "tail":
        return R.tail_llrs(cfg)
    if name.startswith("batch"):
        return R.minsum_batch_llrs(cfg, int(name[5:]))
    return R.minsum_edge_llrs(cfg)[name]


def _assert_minsum_equal(cfg, name, cap, alpha=0.0, max_batch=None):
    from mercury_amd import DEC_MINSUM
    llr = _minsum_inputs(cfg, name)
    ref_bits, ref_it = _minsum_model(cfg, name, cap, alpha if alpha > 0 else 0.8)
    bits, iters = _decode(cfg, llr, DEC_MINSUM, cap, max_batch=max_batch, minsum_alpha=alpha)
    wrong = [f for f in range(len(llr)) if iters[f] != ref_it[f] or not np.array_equal(bits[f], ref_bits[f])]
    print(cfg, name, cap, alpha, "iterations", iters.tolist(), "model", ref_it.tolist(), "frames that differ", wrong,
          "bits that differ", int((bits != ref_bits).sum()))
    assert np.array_equal(iters, ref_it), (cfg, name, cap, alpha, iters.tolist(), ref_it.tolist())
    assert np.array_equal(bits, ref_bits), (cfg, name, cap, alpha, wrong, int((bits != ref_bits).sum()))
    return ref_it


@pytest.mark.parametrize("cap", R.MINSUM_CAPS)
@pytest.mark.parametrize("cfg", CFGS)
def test_minsum_equals_its_model_at_every_rate_and_cap(cfg, cap):
    """24 frames per rate - 8 below the threshold, 8 across it, 8 well above; every second one carries a random non-zero codeword - at caps
    of 1, 2, 5 and 50 iterations: bits [F, K] and iteration counts identical. Between them the rates hold every group size of the grouped
    layout (2 to 64 lanes), every variable degree and every row block of the variable records."""
    _assert_minsum_equal(cfg, "main", cap)


@pytest.mark.parametrize("cap", [2, 50])
@pytest.mark.parametrize("name", ["ties", "zeros", "negative_zero", "saturation"])
@pytest.mark.parametrize("cfg", CFGS)
def test_minsum_equals_its_model_on_edge_llrs(cfg, name, cap):
    """ties: LLRs from {+-0.5, +-1, +-2}, so that almost every check's two smallest magnitudes are equal and many q are +-0 after the first
    update. zeros: all +0.0 and all -0.0 (a codeword at once: `posterior < 0` is false for both). negative_zero: -0.0 and +0.0 sprinkled
    into noisy frames (its sign bit counts in a check's sign parity, not in the syndrome). saturation: every LLR +-5000, every LLR +-3e38,
    forty LLRs +-Inf, two hundred LLRs scaled by 5000 - messages never exceed 4096, so no Inf - Inf arises."""
    it = _assert_minsum_equal(cfg, name, cap)
    if name == "zeros":
        assert (it == 0).all()


@pytest.mark.parametrize("cap", [5, 6, 9, 50])
def test_minsum_rate_1_16_saturated_message_of_the_degree_one_check(cap):
    """The rate-1/16 graph's check of degree 1 sends min over no edge = +Inf, saturated to 4096, which walks down the accumulator chain one
    variable per iteration: frames that run 5 and more iterations, cut at caps around that."""
    it = _assert_minsum_equal(0, "degree_one", cap)
    if cap == 50:
        assert (it >= 5).sum() >= 4 and (it <= 50).sum() >= 4, it.tolist()


@pytest.mark.parametrize("alpha", [0.0, 1.0, 0.75, 0.8125])
@pytest.mark.parametrize("cfg", [8, 16])
def test_minsum_alpha_is_the_configured_one(cfg, alpha):
    """minsum_alpha 1.0, 0.75 and 0.8125 next to the default (0.0 selects 0.8f): the first 8 frames of the main batch, caps 3 and 50."""
    from mercury_amd import DEC_MINSUM
    llr = R.minsum_main_llrs(cfg)[0][8:16]
    for cap in (3, 50):
        ref_bits, ref_it, _ = R.minsum_ref(R.CFG_K[cfg], llr, cap, np.float32(alpha if alpha > 0 else 0.8))
        bits, iters = _decode(cfg, llr, DEC_MINSUM, cap, minsum_alpha=alpha)
        print(cfg, alpha, cap, iters.tolist(), ref_it.tolist(), int((bits != ref_bits).sum()))
        assert np.array_equal(iters, ref_it), (cfg, alpha, cap, iters.tolist(), ref_it.tolist())
        assert np.array_equal(bits, ref_bits), (cfg, alpha, cap)


@pytest.mark.parametrize("F", [1, 3, 65])
def test_minsum_every_frame_of_a_ragged_batch_gets_its_own_result(F):
    """1, 3 and 65 distinct frames through a context whose max_batch is larger"""
    it = _assert_minsum_equal(8, "batch%d" % F, 50, max_batch=128)
    if F == 65:
        assert len(set(it.tolist())) >= 5


@pytest.mark.parametrize("cfg", [0, 8, 16])
def test_minsum_tail_follows_the_models_bits(cfg):
    """ldpc_decode_dev's payload bytes, CRC, all_zeros and iterations_done are those of the model's hard decisions, through the
    reference's de-scrambling, packing and CRC as oraclelib.payload_tail restates them: whole frames with a valid CRC, one buried in noise, and
    random codewords."""
    import torch
    from mercury_amd import DEC_MINSUM, RxPhy
    dev = torch.device("cuda")
    llr = R.tail_llrs(cfg)
    F = len(llr)
    ref_bits, ref_it = _minsum_model(cfg, "tail", 50)
    orc = oraclelib.Oracle(cfg, 50)
    rx = RxPhy(cfg, max_iters=50, decoder=DEC_MINSUM, max_batch=32)
    stride = rx.payload_stride
    d_llr = torch.from_numpy(np.array(llr)).to(dev)
    bits = torch.full((F, rx.K), 7, dtype=torch.uint8, device=dev)
    iters = torch.full((F,), -5, dtype=torch.int32, device=dev)
    pay = torch.full((F, stride), 0xEE, dtype=torch.uint8, device=dev)
    st = torch.full((F, 6), -7, dtype=torch.int32, device=dev)
    rx.ldpc_decode_dev(d_llr.data_ptr(), F, d_bits=bits.data_ptr(), d_iters=iters.data_ptr(), d_payload=pay.data_ptr(), d_stats=st.data_ptr())
    torch.cuda.synchronize()
    bits, iters, pay, st = bits.cpu().numpy(), iters.cpu().numpy(), pay.cpu().numpy(), st.cpu().numpy()
    rx.close()
    decoded = 0
    for f in range(F):
        by, crc, all_zeros = oraclelib.payload_tail(orc, ref_bits[f])
        assert np.array_equal(bits[f], ref_bits[f]) and iters[f] == ref_it[f], (cfg, f)
        assert np.array_equal(pay[f, :len(by)], by), (cfg, f)
        ok = int(not (all_zeros or crc != 0))
        assert list(st[f, :4]) == [ref_it[f], crc, all_zeros, ok], (cfg, f, list(st[f, :4]))
        decoded += ok
    assert 1 <= decoded < F                 # the stats of decoded and of failed frames are both exercised


@pytest.mark.parametrize("k", R.SPA_CAPS)
@pytest.mark.parametrize("cfg", CFGS)
def test_spa_fast_equals_the_float64_model_of_its_rule_outside_the_fragile_set(cfg, k):
    """16 frames per rate (8 one dB below the threshold, 8 one and a half above) at caps of 1, 2, 3, 5 and 10 iterations. For every frame whose
    count is determinate: the iteration count equals the model's, and so does every information bit that is not fragile at the frame's last
    look. What is fragile and what is determinate follows from the model and its float32 emulations alone (spa_fast_verdicts); the host
    test holds the share that leaves out under 0.5 % of the bits and 2 of the 16 frames."""
    from mercury_amd import DEC_SPA_FAST
    llr = R.spa_llrs(cfg)[0]
    v = R.spa_verdicts(cfg)[k]
    bits, iters = _decode(cfg, llr, DEC_SPA_FAST, k)
    det = v["determinate"]
    cmp_ = v["compare"] & det[:, None]
    diff = (bits != v["bits"])
    print(cfg, k, "iterations", iters.tolist(), "model", v["iterations"].tolist(), "determinate", det.astype(int).tolist(),
          "bits compared", int(cmp_.sum()), "of", cmp_.size, "differ where compared", int((diff & cmp_).sum()), "differ anywhere", int(diff.sum()),
          "D", ["%.2g" % d for d in v["D"]])
    assert np.array_equal(iters[det], v["iterations"][det]), (cfg, k, iters.tolist(), v["iterations"].tolist(), det.tolist())
    assert not (diff & cmp_).any(), (cfg, k, np.argwhere(diff & cmp_)[:10].tolist())


def test_spa_fast_lower_clamp_of_the_tanh_is_two_to_the_minus_thirty():
    """Frames with probe variables whose bit after one iteration is 1 with the clamp of |t| at 2^-30 and 0 with a clamp a thousand times
    larger (fp32_decoders_ref.spa_clamp_llrs; the host test shows both on the model), none of them fragile."""
    from mercury_amd import DEC_SPA_FAST
    llr, probes = R.spa_clamp_llrs()
    v = R.spa_clamp_verdict()
    bits, iters = _decode(R.CLAMP_CFG, llr, DEC_SPA_FAST, 1)
    rows = np.arange(len(llr))[:, None]
    print("probes", bits[rows, probes].tolist(), "iterations", iters.tolist(), "differ anywhere", int((bits != v["bits"]).sum()))
    assert v["determinate"].all() and v["compare"][rows, probes].all()
    assert np.array_equal(iters, v["iterations"])
    assert (bits[rows, probes] == 1).all(), bits[rows, probes].tolist()
    assert not ((bits != v["bits"]) & v["compare"]).any()


def test_spa_fast_zero_llrs_enter_as_plus_zero():
    """All-zero LLRs of either sign: every posterior is +0, the frame is a codeword at once and every bit is 0."""
    from mercury_amd import DEC_SPA_FAST
    z = np.zeros((2, R.N), np.float32)
    z[1] = -0.0
    for cfg in (0, 16):
        bits, iters = _decode(cfg, z, DEC_SPA_FAST, 10)
        assert (iters == 0).all() and not bits.any(), cfg

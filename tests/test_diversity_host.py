"""CPU tests of diversity combining (include/mercury_diversity.h): the host twin of the combine kernel against a sequential float32 sum,
what it refuses, the exported symbols, and the fixtures the GPU tests (tests/test_gpu_diversity.py) are built on, pinned on the CPU oracle:
branches no decoder gets through alone, decoded from the float sum of their LLRs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import SEED
from oraclelib import Oracle, noise_amp_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = 1600


def salted_rows(F, seed=11):
    """F LLR rows with the values float addition treats specially: +-Inf (and Inf - Inf = NaN where two meet), NaN, -0.0 (alone and against
    +0.0), denormals (alone, summed with each other and with normal numbers), the largest finite float (overflow to Inf)."""
    rng = np.random.default_rng(seed)
    llr = (rng.standard_normal((F, ROW)) * 8).astype(np.float32)
    special = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, -5.9e-39, 3.4028235e38, -3.4028235e38], np.float32)
    pick = rng.integers(0, special.size, (F, ROW))
    where = rng.random((F, ROW)) < 0.3
    llr[where] = special[pick[where]]
    llr[:, :special.size] = special                    # every row meets every other row's same special value ...
    for f in range(F):                                 # ... and, rotated, every other one
        llr[f, special.size:2 * special.size] = np.roll(special, f)
    return llr


def sequential_sum(llr, groups):
    """(..(r0 + r1) + r2 ..) in float32, one addition at a time; a group of one is a copy"""
    out = np.zeros((len(groups), ROW), np.float32)
    with np.errstate(all="ignore"):
        for g, members in enumerate(groups):
            acc = llr[members[0]].copy()
            for m in members[1:]:
                acc = (acc + llr[m]).astype(np.float32)
            out[g] = acc
    return out


def same_floats(got, want):
    """equal as bit patterns wherever the result is a number (so -0.0 is not +0.0, a denormal is not 0), NaN in the same places"""
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def scattered_groups(F, seed=5):
    """CSR groups of sizes 1..8 (twice, in a shuffled order) whose members are spread over the F rows, in no order, some rows in several groups"""
    rng = np.random.default_rng(seed)
    sizes = rng.permutation(np.repeat(np.arange(1, 9), 2))
    return [[int(m) for m in rng.choice(F, int(n), replace=False)] for n in sizes]


# ---- the host twin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3, 8])
def test_host_combine_uniform_groups_equal_a_sequential_float_sum(D):
    from mercury_amd import host_llr_combine
    G = 5
    llr = salted_rows(G * D, seed=D)
    got = host_llr_combine(llr, D=D)
    want = sequential_sum(llr, [list(range(g * D, g * D + D)) for g in range(G)])
    assert np.isnan(want).any() and np.isinf(want).any() and (want.view(np.uint32) == 0x80000000).any()
    assert same_floats(got, want)
    if D == 1:
        assert got.tobytes() == llr.tobytes()                    # a group of one is a copy, NaN payloads included


def test_host_combine_csr_groups_equal_a_sequential_float_sum():
    from mercury_amd import host_llr_combine
    F = 37
    llr = salted_rows(F)
    groups = scattered_groups(F)
    assert sorted(len(g) for g in groups) == sorted(list(range(1, 9)) * 2)
    assert same_floats(host_llr_combine(llr, groups=groups), sequential_sum(llr, groups))
    # member order is the order of the additions: float addition is not associative, so some element of some group tells the orders apart
    rev = [g[::-1] for g in groups]
    assert same_floats(host_llr_combine(llr, groups=rev), sequential_sum(llr, rev))
    assert not same_floats(sequential_sum(llr, rev), sequential_sum(llr, groups))


def test_host_combine_refuses_bad_groups_and_leaves_the_output_alone():
    from mercury_amd import load_library
    lib = load_library()
    F = 16
    llr = salted_rows(F)
    out = np.full((F, ROW), 7.25, np.float32)
    before = out.tobytes()

    def call(D, first=None, member=None, G=0, F_=F, llr_=llr, out_=out):
        f = None if first is None else np.array(first, np.int32)
        m = None if member is None else np.array(list(member) + [0], np.int32)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        return lib.mgpu_host_llr_combine(p(llr_), F_, D, p(f), p(m), G, p(out_))

    refused = [
        call(0), call(-1), call(9),                                       # D outside 1..8
        call(3), call(5), call(2, F_=15),                                 # F % D != 0
        call(2, F_=-2),
        call(0, [1, 2, 3], [0, 1, 2], 2),                                 # first does not start at 0
        call(0, [0, 3, 2, 4], [0, 1, 2, 3], 3),                           # first decreases
        call(0, [0, 2, 2, 3], [0, 1, 2], 3),                              # an empty group
        call(0, [0, 9], list(range(9)), 1),                               # nine members
        call(0, [0, 2], [0, F], 1), call(0, [0, 2], [-1, 3], 1),          # a member outside [0, F)
        call(0, [0, 1], None, 1), call(0, None, [0], 1),                  # half a CSR
        call(2, llr_=None), call(2, out_=None),
    ]
    assert refused == [1] * len(refused), refused
    assert out.tobytes() == before
    assert call(2) == 0 and call(8) == 0 and call(0, [0, 8], list(range(8)), 1) == 0 and call(1, F_=0) == 0
    assert call(0, [0], [], 0) == 0                                      # no groups: nothing to do


def test_python_wrapper_raises_with_the_status_code():
    from mercury_amd import MgpuError, host_llr_combine
    llr = np.zeros((4, ROW), np.float32)
    for kw in (dict(D=3), dict(D=9), dict(groups=[[0, 4]]), dict(groups=[[]]), dict(), dict(D=2, groups=[[0]])):
        with pytest.raises(MgpuError):
            host_llr_combine(llr, **kw)
    with pytest.raises(MgpuError) as e:
        host_llr_combine(llr, D=3)
    assert e.value.code == 1


# ---- the header --------------------------------------------------------------------------------------------------------------------
def test_library_exports_what_mercury_diversity_h_declares():
    from mercury_amd import DIVERSITY_MAX, DIVERSITY_SYMBOLS, load_library
    text = open(os.path.join(ROOT, "include", "mercury_diversity.h")).read()
    assert int(re.search(r"#define MGPU_DIVERSITY_MAX (\d+)", text).group(1)) == DIVERSITY_MAX == 8
    for word in ("mgpu_receive_byte_batch", "mgpu_capture_", "mgpu_linksim_", "mgpu_pool_", "MGPU_ERR_UNSUPPORTED", "pipelined", "maximal-ratio"):
        assert word in text, word                                         # the rule's limits are said where a caller reads them
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mgpu_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(DIVERSITY_SYMBOLS)
    lib = load_library()
    for name in declared:
        assert hasattr(lib, name), name


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------
#: (mode, Es/N0 dB, D, G, the iterations a combined decode takes where that is pinned): branch (g, d) is the clean frame g through the generator's channel
#: with noise index 1000 + g * D + d
FIXTURES = [(8, -1.0, 2, 16, (4, 8)), (12, 4.5, 2, 8, (2, 3)), (8, -4.0, 4, 8, None)]


def fixture_branches(cfg, esn0, D, G):
    """(oracle, clean frames [G], branch frames [G * D])"""
    orc = Oracle(cfg)
    clean = [orc.gen_frame(SEED, g, 0.0, 0)[0] for g in range(G)]
    amp = noise_amp_for(esn0)
    return orc, clean, np.stack([orc.channel(clean[g], SEED, 1000 + g * D + d, amp, 0) for g in range(G) for d in range(D)])


@pytest.mark.parametrize("cfg,esn0,D,G,iters", FIXTURES)
def test_fixture_no_branch_decodes_alone_and_every_float_sum_does(cfg, esn0, D, G, iters):
    from mercury_amd import host_llr_combine
    orc, clean, bb = fixture_branches(cfg, esn0, D, G)
    sent = [orc.rx(x)["bits"] for x in clean]
    assert all(orc.rx(clean[g])["iterations"] <= 50 for g in range(0, G, 5))
    alone = [orc.rx(bb[f]) for f in range(G * D)]
    decoded_alone = sum(bool(alone[f]["iterations"] <= 50 and np.array_equal(alone[f]["bits"], sent[f // D])) for f in range(G * D))
    sums = host_llr_combine(np.stack([r["llr_ldpc"] for r in alone]), D=D)
    combined = [orc.ldpc_decode(sums[g]) for g in range(G)]
    decoded = sum(bool(np.array_equal(bits, sent[g])) for g, (bits, it) in enumerate(combined))
    print("mode %d %.1f dB D=%d: %d of %d alone, %d of %d combined, iterations %s" % (cfg, esn0, D, decoded_alone, G * D, decoded, G, [it for _, it in combined]))
    assert decoded_alone == 0
    assert decoded == G
    if iters:
        assert all(iters[0] <= it <= iters[1] for _, it in combined), [it for _, it in combined]

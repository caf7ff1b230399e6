"""GPU tests of diversity combining (include/mercury_diversity.h): D branches of a frame decoded from the sum of their LLRs.

Yardsticks: D = 1 against the plain span, byte for byte (this is what checks the scatter); a grouped call against its own parts - the plain
call's branch LLRs, the host twin of the sum (tests/test_diversity_host.py holds it against a sequential float sum), the decoder entry point
and the CPU oracle's decoder on those sums; the combine kernel against the host twin on special values, both of its paths; per-group results
independent of the batch; the self-simulation against itself (D = 1, two batch sizes) and against counts taken on the CPU oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import OPERATING_ESN0, SEED
from oraclelib import Oracle, noise_amp_for
from test_diversity_host import FIXTURES, ROW, fixture_branches, salted_rows, same_floats, scattered_groups

pytestmark = pytest.mark.gpu

INT_FIELDS = ("iterations_done", "crc", "all_zeros", "message_decoded")
NO_SNR = np.float32(-99.9)


def _rx(cfg, **kw):
    from mercury_amd import RxPhy
    return RxPhy(cfg, **kw)


@functools.lru_cache(maxsize=None)
def _fixture(cfg, esn0, D, G):
    return fixture_branches(cfg, esn0, D, G)


def _same(a, b, keys=("payload", "stats", "llr_ldpc")):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- 1. D = 1 is the plain span ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,kw", [(8, {}), (13, {}), (100, {}), (15, dict(agc=0, variance_source=0))])
def test_one_branch_per_group_is_the_plain_span_byte_for_byte(cfg, kw):
    orc = Oracle(cfg, 50)
    if cfg == 8:         # the decoded path and the -99.9 path
        bb = np.stack([orc.gen_frame(SEED, f, noise_amp_for(3.5 if f < 32 else -15.0))[0] for f in range(64)])
    else:
        bb = np.stack([orc.gen_frame(SEED, f, noise_amp_for(OPERATING_ESN0[cfg]))[0] for f in range(16)])
    rx = _rx(cfg, max_batch=len(bb), **kw)
    plain = rx.receive(bb, want_llr=True)
    one = rx.receive_div(bb, 1, want_llr=True)
    decoded = plain["stats"]["message_decoded"] != 0
    if cfg == 8:
        assert decoded[:32].sum() >= 24 and decoded[32:].sum() == 0
        assert (plain["stats"]["snr_db"][32:] == NO_SNR).all()
    else:
        assert decoded.sum() >= 12, decoded.sum()
    _same(one, plain)
    rx.close()


# ---- 2. composition ----------------------------------------------------------------------------------------------------------------
def _check_composition(rx, orc, bb, D, pinned):
    """the grouped call on bb against its parts; pinned: no branch decodes alone and every group does"""
    import torch
    from mercury_amd import STATS_DTYPE, host_llr_combine
    F, G = len(bb), len(bb) // D
    plain = rx.receive(bb, want_llr=True)
    div = rx.receive_div(bb, D, want_llr=True)
    assert div["llr_ldpc"].tobytes() == plain["llr_ldpc"].tobytes()              # the BRANCH LLRs
    sums = host_llr_combine(div["llr_ldpc"], D=D)
    d_llr = torch.from_numpy(sums).cuda()
    d_bits = torch.zeros((G, rx.K), dtype=torch.uint8, device="cuda")
    d_payload = torch.zeros((G, rx.payload_stride), dtype=torch.uint8, device="cuda")
    d_stats = torch.zeros(G * STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    rx.ldpc_decode_dev(d_llr.data_ptr(), G, d_bits=d_bits.data_ptr(), d_payload=d_payload.data_ptr(), d_stats=d_stats.data_ptr())
    torch.cuda.synchronize()
    g_payload, g_bits = d_payload.cpu().numpy(), d_bits.cpu().numpy()
    g_stats = d_stats.cpu().numpy().view(STATS_DTYPE)
    ok = g_stats["message_decoded"] != 0
    for g in range(G):
        bits, it = orc.ldpc_decode(sums[g])
        assert np.array_equal(g_bits[g], bits.astype(np.uint8)) and g_stats["iterations_done"][g] == it, (g, it, g_stats["iterations_done"][g])
    for f in range(F):
        g = f // D
        assert np.array_equal(div["payload"][f], g_payload[g]), f
        for k in INT_FIELDS:
            assert div["stats"][k][f] == g_stats[k][g], (f, k)
    assert div["stats"]["variance"].tobytes() == plain["stats"]["variance"].tobytes()
    group_ok = np.repeat(ok, D)
    both = group_ok & (plain["stats"]["message_decoded"] != 0)
    assert np.array_equal(div["stats"]["snr_db"][both].view(np.uint32), plain["stats"]["snr_db"][both].view(np.uint32))
    assert (div["stats"]["snr_db"][~group_ok] == NO_SNR).all()
    if pinned:
        assert (plain["stats"]["message_decoded"] != 0).sum() == 0 and ok.sum() == G, ((plain["stats"]["message_decoded"] != 0).sum(), ok.sum())
    return div


@pytest.mark.parametrize("cfg,esn0,D,G,pinned", [f[:4] + (True,) for f in FIXTURES] + [(100, -10.0, 2, 8, False)])
def test_a_grouped_call_is_the_sum_of_its_parts(cfg, esn0, D, G, pinned):
    orc, _, bb = _fixture(cfg, esn0, D, G)
    rx = _rx(cfg, max_batch=G * D)
    _check_composition(rx, orc, bb, D, pinned)
    rx.close()


# ---- 3. the combine kernel ---------------------------------------------------------------------------------------------------------
def test_device_combine_equals_the_host_twin_on_both_paths():
    import torch
    from mercury_amd import host_llr_combine
    F = 37
    llr = salted_rows(F)
    groups = scattered_groups(F)
    rx = _rx(8, max_batch=F)
    cases = [dict(groups=groups)] + [dict(D=D) for D in (1, 2, 3, 8)]
    for kw in cases:
        n = F if "groups" in kw else (F // kw["D"]) * kw["D"]
        want = host_llr_combine(llr[:n], **kw)
        assert same_floats(rx.llr_combine(llr[:n], **kw), want), kw                  # 16-byte aligned rows: the float4 path
        # a base pointer 4 bytes off (the input, the output, both): the scalar path
        d_in = torch.zeros(n * ROW + 1, dtype=torch.float32, device="cuda")
        d_in[1:] = torch.from_numpy(llr[:n].ravel()).cuda()
        d_al = torch.from_numpy(llr[:n]).cuda()
        for in_off, out_off in ((4, 0), (0, 4), (4, 4)):
            d_out = torch.full((len(want) * ROW + 1,), 3.0, dtype=torch.float32, device="cuda")
            rx.llr_combine_dev((d_in if in_off else d_al).data_ptr() + in_off, n, d_out.data_ptr() + out_off, **kw)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            got, spare = (got[1:], got[0]) if out_off else (got[:-1], got[-1])
            assert same_floats(got.reshape(-1, ROW), want), (kw, in_off, out_off)
            assert spare == 3.0                                                       # nothing written outside the G rows
    rx.close()


# ---- 4. batch independence ---------------------------------------------------------------------------------------------------------
def test_group_records_do_not_depend_on_the_batch():
    cfg, esn0, D, G, _ = FIXTURES[0]
    _, _, bb = _fixture(cfg, esn0, D, G)
    rx = _rx(cfg, max_batch=G * D)
    groups = bb.reshape(G, D, -1)
    whole = rx.receive_div(bb, D, want_llr=True)
    rec = lambda out, g: tuple(out[k][g * D:(g + 1) * D].tobytes() for k in ("payload", "stats", "llr_ldpc"))
    rev = rx.receive_div(groups[::-1].reshape(G * D, -1), D, want_llr=True)
    for g in range(G):
        assert rec(rev, G - 1 - g) == rec(whole, g), g
    for g in (0, 7, 15):
        assert rec(rx.receive_div(groups[g], D, want_llr=True), 0) == rec(whole, g), g
    rx.close()


# ---- 5. host form = device form ----------------------------------------------------------------------------------------------------
def test_host_and_device_entry_points_agree():
    import torch
    from mercury_amd import STATS_DTYPE
    cfg, esn0, D, G, _ = FIXTURES[0]
    _, _, bb = _fixture(cfg, esn0, D, G)
    F = G * D
    rx = _rx(cfg, max_batch=F)
    host = rx.receive_div(bb, D, want_llr=True)
    bare = rx.receive_div(bb, D)
    _same(bare, host, ("payload", "stats"))
    d_bb = torch.from_numpy(bb.view(np.float64)).cuda()
    for with_llr in (True, False):
        d_payload = torch.zeros((F, rx.payload_stride), dtype=torch.uint8, device="cuda")
        d_stats = torch.zeros(F * STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_llr = torch.zeros((F, ROW), dtype=torch.float32, device="cuda") if with_llr else None
        rx.receive_div_dev(d_bb.data_ptr(), F, D, d_payload.data_ptr(), d_stats.data_ptr(), d_llr.data_ptr() if with_llr else None)
        torch.cuda.synchronize()
        assert d_payload.cpu().numpy().tobytes() == host["payload"].tobytes()
        assert d_stats.cpu().numpy().tobytes() == host["stats"].tobytes()
        if with_llr:
            assert d_llr.cpu().numpy().tobytes() == host["llr_ldpc"].tobytes()
    rx.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    from mercury_amd import MgpuError
    cfg, esn0, D, G, _ = FIXTURES[0]
    orc, _, bb = _fixture(cfg, esn0, D, G)
    rx = _rx(cfg, max_batch=G * D)
    plain = rx.receive(bb, want_llr=True)

    def refused(code, fn):
        with pytest.raises(MgpuError) as e:
            fn()
        assert e.value.code == code, (e.value.code, str(e.value))
        _same(rx.receive(bb, want_llr=True), plain)

    refused(1, lambda: rx.receive_div(bb[:31], 2))                        # F % D != 0
    refused(1, lambda: rx.receive_div(bb[:27], 9))                        # D = 9
    refused(1, lambda: rx.receive_div(bb, 0))
    refused(1, lambda: rx.receive_div(np.concatenate([bb, bb[:2]]), 2))   # F > max_batch
    refused(1, lambda: rx.llr_combine(plain["llr_ldpc"], D=3))
    refused(1, lambda: rx.llr_combine(plain["llr_ldpc"], groups=[[0, 1], [2, 32]]))
    refused(1, lambda: rx.llr_combine(plain["llr_ldpc"], groups=[[0, 1], []]))
    refused(1, lambda: rx.baseband_test_esn0([-1.0], 4, diversity=9))
    rx.set_estimator_ladder([(21, 21), (5, 21)])
    with_ladder = rx.receive(bb, want_llr=True)
    for fn in (lambda: rx.receive_div(bb, 2), lambda: rx.baseband_test_esn0([-1.0], 4, diversity=2)):
        with pytest.raises(MgpuError) as e:
            fn()
        assert e.value.code == 4, str(e.value)                            # MGPU_ERR_UNSUPPORTED
        _same(rx.receive(bb, want_llr=True), with_ladder)
    rx.set_estimator_ladder([])
    _same(rx.receive(bb, want_llr=True), plain)
    rx.close()


def test_a_one_rung_ladder_is_accepted_and_its_window_is_the_front_ends():
    cfg, esn0, D, G, _ = FIXTURES[0]
    orc, _, bb = _fixture(cfg, esn0, D, G)
    rx = _rx(cfg, max_batch=G * D)
    square = rx.receive(bb, want_llr=True)
    rx.set_estimator_ladder([(5, 21)])
    div = _check_composition(rx, orc, bb, D, pinned=False)
    assert div["llr_ldpc"].tobytes() != square["llr_ldpc"].tobytes()      # the 5 x 21 window's LLRs, not the context's own
    rx.close()


# ---- 7. self-simulation ------------------------------------------------------------------------------------------------------------
def test_self_simulation_with_one_branch_is_the_hf_loop():
    from mercury_amd import hf_channel_preset
    rx = _rx(8, max_batch=32)
    for name in ("moderate", "awgn"):
        ch = hf_channel_preset(name)
        want = rx.baseband_test_esn0([2.5, -1.0], 48, seed=SEED, frame0=5, hf_channel=ch)
        got = rx.baseband_test_esn0([2.5, -1.0], 48, seed=SEED, frame0=5, hf_channel=ch, diversity=1)
        assert got == want, (name, got, want)
        assert 0 < want[0]["crc_ok_frames"]
    rx.close()


def test_self_simulation_two_branches_decode_what_one_does_not():
    """Mode 8, AWGN, -1.0 dB, 64 payloads. The CPU twin (Oracle.gen_frame(SEED, g, 0) through Oracle.channel with noise index g * D + d, the host
    sum, Oracle.ldpc_decode) leaves 0 error frames of 64 with D = 2 and 63 with D = 1; the slack (2 and 56) covers the device generator's libm
    ulps in the noise."""
    big, small = _rx(8, max_batch=128), _rx(8, max_batch=24)
    two = big.baseband_test_esn0([-1.0], 64, seed=SEED, diversity=2)
    one = big.baseband_test_esn0([-1.0], 64, seed=SEED, diversity=1)
    print("error frames of 64: D = 2: %d, D = 1: %d" % (two[0]["Error_frames_total"], one[0]["Error_frames_total"]))
    assert two[0]["Frames_total"] == 64 and one[0]["Frames_total"] == 64
    assert two[0]["Bits_total"] == 64 * big.nReal
    assert two[0]["Error_frames_total"] <= 2
    assert one[0]["Error_frames_total"] >= 56
    assert two[0]["crc_ok_frames"] >= 62
    # 12 groups a batch (five batches and a rest of four) against one batch of 64
    assert small.baseband_test_esn0([-1.0], 64, seed=SEED, diversity=2) == two
    big.close()
    small.close()

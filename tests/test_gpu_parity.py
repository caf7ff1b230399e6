"""GPU parity tests: the HIP path (through the C-ABI) against the CPU oracle on the same inputs.

Bar (BASELINE.json north_star): bit-exact interleaver indexing / hard decisions / CRC / payload;
soft LLRs within 1e-5 (absolute, scaled by max(1,|LLR|) as SURVEY.md §7.3-2 specifies).
"""
import os

import numpy as np
import pytest

import oraclelib
from conftest import OPERATING_ESN0, SEED
from oraclelib import FLAGS_BASEBAND_TEST, FLAGS_RECEIVE_BYTE, Oracle, noise_amp_for

pytestmark = pytest.mark.gpu

LLR_TOL = 1e-5


def _host_runs_the_restated_libm():
    try:
        flags = open("/proc/cpuinfo").read()
    except OSError:
        return False
    return " fma " in flags and " avx2 " in flags


EXACT_TRIG = _host_runs_the_restated_libm()


def _rx(cfg, **kw):
    from mercury_amd import RxPhy
    return RxPhy(cfg, **kw)


def _frames(orc, snrs, seed=SEED, channel=0, start=0):
    bb, pl = [], []
    for i, snr in enumerate(snrs):
        b, p = orc.gen_frame(seed, start + i, noise_amp_for(snr), channel)
        bb.append(b)
        pl.append(p)
    return np.stack(bb), pl


def _llr_close(got, ref):
    tol = LLR_TOL * np.maximum(1.0, np.abs(ref.astype(np.float64)))
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= tol


def _variants(cfg):
    # the reference's receive_byte variant divides by a ~1e-33 variance for the ZF modes (the
    # equalised pilots equal the pilots exactly), which turns every LLR into rounding noise; the
    # ZF modes are therefore exercised the way the reference's own BER loop runs them.
    if cfg in (15, 16):
        return [(0, 0, FLAGS_BASEBAND_TEST)]
    return [(1, 1, FLAGS_RECEIVE_BYTE), (0, 0, FLAGS_BASEBAND_TEST)]


def stages_match_oracle(rx, orc, bb, payloads, snrs, flags):
    """What test_all_stages_match_oracle holds one context to: every stage tap, the float variance, payload, CRC and iteration count of
    receive(bb, taps=True) against the CPU oracle run with `flags`. snrs: the Es/N0 each frame was made at (60.0 or more: it must decode)."""
    cfg = rx.cfg
    out = rx.receive(bb, taps=True)
    for f in range(len(snrs)):
        ref = orc.rx(bb[f], flags)
        # FP64 front-end: the reference's operations in the reference's order, its libm's atan / sincos restated
        # (csrc/glibc_trig.h) -> every stage BIT-IDENTICAL where the host runs the libm build that was restated
        # (FMA-capable x86-64, see tests/test_glibc_trig.py); elsewhere the PSK modes' phasors may differ in the last ulp
        exact = EXACT_TRIG or not orc.amp_restore
        for key in ("grid", "H", "eq", "syms"):        # H: the channel grid after estimate + interpolation + amplitude restoration (rows a4-a7)
            d = np.abs(out[key][f] - ref[key]).max()
            scale = np.abs(ref[key]).max()
            assert d <= (0.0 if exact or key == "grid" else 1e-12) * scale, (cfg, flags, f, key, d, scale)
        if exact and np.isfinite(ref["variance"]):
            assert out["variance"][f] == ref["variance"], (cfg, f)
            assert np.float32(out["stats"]["variance"][f]) == np.float32(ref["variance_f"])
            assert np.array_equal(out["llr_demod"][f], ref["llr_demod"], equal_nan=True), (cfg, flags, f, "llr_demod")
            assert np.array_equal(out["llr_ldpc"][f], ref["llr_ldpc"], equal_nan=True), (cfg, flags, f, "llr_ldpc")
        else:
            assert abs(out["variance"][f] - ref["variance"]) <= 1e-12 * abs(ref["variance"]), (cfg, f)
        assert _llr_close(out["llr_demod"][f], ref["llr_demod"]).all(), (cfg, flags, f, "llr_demod")
        assert _llr_close(out["llr_ldpc"][f], ref["llr_ldpc"]).all(), (cfg, flags, f, "llr_ldpc")
        # integer / byte outputs: bit exact
        assert out["stats"]["iterations_done"][f] == ref["iterations"], (cfg, flags, f, "iterations")
        assert np.array_equal(out["payload"][f], ref["bytes"].astype(np.uint8)), (cfg, flags, f, "payload")
        assert out["stats"]["crc"][f] == ref["crc"], (cfg, flags, f)
        assert out["stats"]["all_zeros"][f] == ref["all_zeros"], (cfg, flags, f)
        if ref["iterations"] <= 50 and snrs[f] > 0 or snrs[f] >= 60.0:
            assert np.array_equal(out["payload"][f][: orc.payload_bytes], payloads[f].astype(np.uint8))
    return out


@pytest.mark.parametrize("cfg", list(range(17)))
def test_all_stages_match_oracle(cfg):
    orc = Oracle(cfg, 50)
    op = OPERATING_ESN0[cfg]
    snrs = [op, op, op + 1.0, -15.0, 60.0]
    bb, payloads = _frames(orc, snrs)
    for agc, vs, flags in _variants(cfg):
        rx = _rx(cfg, max_iters=50, agc=agc, variance_source=vs, max_batch=len(snrs))
        stages_match_oracle(rx, orc, bb, payloads, snrs, flags)
        rx.close()


def test_live_contexts_report_the_reference_mode_table():
    """mgpu_get_info of a context on the device equals what the compiled reference printed after the real
    load_configuration(cfg) (transcribed into tests/golden/survey_mode_table.json) for all 17 modes."""
    import json
    tab = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "survey_mode_table.json")))
    for cfg in range(17):
        rx = _rx(cfg, max_batch=1)
        for k, v in dict(tab["modes"][str(cfg)], **tab["fixed"]).items():
            assert getattr(rx, k) == v, (cfg, k, getattr(rx, k), v)
        rx.close()


@pytest.mark.parametrize("M,rate16,pre,est,esn0", __import__("conftest").EXPLICIT_COMBOS)
def test_explicit_configurations_match_oracle(M, rate16, pre, est, esn0):
    """MGPU_CFG_EXPLICIT: (constellation, LDPC rate, preamble length, estimator) combinations load_configuration does not pair
    (SURVEY.md §8b "cfg id or explicit"), the whole span against the oracle (pinned to the reference's classes configured the same
    way, tests/test_oracle_vs_ref.py): same bar as the 17 modes; plus transmit_byte -> receive_byte with the explicit preamble."""
    from mercury_amd.physical_layer import cfg_explicit
    cfg = cfg_explicit(M, rate16, pre, est)
    orc = Oracle(cfg, 50)
    snrs = [esn0, esn0 + 1.0, esn0 - 2.5, -15.0, 60.0]
    bb, payloads = _frames(orc, snrs)
    variants = [(0, 0, FLAGS_BASEBAND_TEST)] if est == 0 else [(1, 1, FLAGS_RECEIVE_BYTE), (0, 0, FLAGS_BASEBAND_TEST)]
    for agc, vs, flags in variants:
        rx = _rx(cfg, max_iters=50, agc=agc, variance_source=vs, max_batch=len(snrs))
        assert (rx.M, rx.K, rx.preamble_nsymb, rx.estimator) == (M, 100 * rate16, pre, est)
        out = rx.receive(bb, taps=True)
        for f in range(len(snrs)):
            ref = orc.rx(bb[f], flags)
            for key, rtol in (("grid", 0.0), ("eq", 1e-12), ("syms", 1e-12)):
                assert np.abs(out[key][f] - ref[key]).max() <= rtol * np.abs(ref[key]).max(), (cfg, flags, f, key)
            assert _llr_close(out["llr_ldpc"][f], ref["llr_ldpc"]).all(), (cfg, flags, f, "llr_ldpc")
            assert out["stats"]["iterations_done"][f] == ref["iterations"], (cfg, flags, f, "iterations")
            assert np.array_equal(out["payload"][f], ref["bytes"].astype(np.uint8)), (cfg, flags, f, "payload")
            assert (out["stats"]["crc"][f], out["stats"]["all_zeros"][f]) == (ref["crc"], ref["all_zeros"]), (cfg, flags, f)
        assert np.array_equal(out["payload"][0][: orc.payload_bytes], payloads[0].astype(np.uint8))
        if agc:      # audio round trip through the explicit mode's own preamble and receive_byte
            msg = np.random.default_rng(cfg).integers(0, 256, (1, rx.payload_bytes), dtype=np.uint8)
            audio = rx.transmit_byte(msg, oraclelib.CARRIER)
            want = orc.transmit_byte(msg[0].astype(np.int32))
            assert np.array_equal(audio[0], want)
            n = rx.receive_buffer_samples()
            win = np.random.default_rng(1).standard_normal(n) * 1e-3
            d = (pre + 3) * rx.Nofdm * 4 + 123           # receive_byte wants the preamble beyond symbol `preamble_nSymb` of the window
            win[d: d + audio.shape[1]] += 2.0 * audio[0]
            r = rx.receive_byte(win[None, :], oraclelib.CARRIER)
            ref_r = orc.receive_byte(win, carrier=oraclelib.CARRIER)
            assert r["stats"]["message_decoded"][0] == ref_r["message_decoded"] == 1
            assert np.array_equal(r["payload"][0][: rx.payload_bytes], msg[0]) and r["stats"]["delay"][0] == ref_r["delay"]
        rx.close()


def _explicit_cases():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg.EXPLICIT_CASES


@pytest.mark.parametrize("cfg,x", _explicit_cases())
def test_explicit_parameters_match_oracle(cfg, x):
    """mgpu_create_explicit (pilot boost, LS window, PRNG seeds of physical_config.cc:35-65 varied): every stage of the span,
    the synthetic generator, the transmit chain and the pre-equalization channel against the oracle configured the same way, which
    tests/golden/golden_explicit.json pins to the reference's classes (tests/test_oracle_golden.py)."""
    orc = Oracle(cfg, 50, explicit=x)
    op = OPERATING_ESN0[cfg]
    snrs = [op, op + 1.0, op - 1.5, -15.0, 60.0]
    bb, payloads = _frames(orc, snrs)
    for agc, vs, flags in _variants(cfg):
        rx = _rx(cfg, max_iters=50, agc=agc, variance_source=vs, max_batch=len(snrs), explicit=x)
        assert rx.ls_window == orc.ls_window
        out = rx.receive(bb, taps=True)
        exact = EXACT_TRIG or not orc.amp_restore
        for f in range(len(snrs)):
            ref = orc.rx(bb[f], flags)
            for key in ("grid", "H", "eq", "syms"):
                d, scale = np.abs(out[key][f] - ref[key]).max(), np.abs(ref[key]).max()
                assert d <= (0.0 if exact or key == "grid" else 1e-12) * scale, (cfg, flags, f, key, d, scale)
            if exact and np.isfinite(ref["variance"]):
                assert out["variance"][f] == ref["variance"], (cfg, f)
                assert np.array_equal(out["llr_ldpc"][f], ref["llr_ldpc"], equal_nan=True), (cfg, flags, f, "llr_ldpc")
            assert _llr_close(out["llr_ldpc"][f], ref["llr_ldpc"]).all(), (cfg, flags, f, "llr_ldpc")
            assert out["stats"]["iterations_done"][f] == ref["iterations"], (cfg, flags, f, "iterations")
            assert np.array_equal(out["payload"][f], ref["bytes"].astype(np.uint8)), (cfg, flags, f, "payload")
            assert (out["stats"]["crc"][f], out["stats"]["all_zeros"][f]) == (ref["crc"], ref["all_zeros"]), (cfg, flags, f)
        assert np.array_equal(out["payload"][4][: orc.payload_bytes], payloads[4].astype(np.uint8))      # the noiseless frame comes back
        if agc:
            import torch
            # the device generator builds frames with this set's pilots and scrambler
            dbb = torch.empty((2, rx.frame_samples, 2), dtype=torch.float64, device="cuda:0")
            dpl = torch.empty((2, rx.payload_stride), dtype=torch.uint8, device="cuda:0")
            rx.txgen_dev(SEED, 40, 2, noise_amp_for(op + 1.0), dbb.data_ptr(), dpl.data_ptr())
            torch.cuda.synchronize()
            for k in range(2):
                want_bb, want_pl = orc.gen_frame(SEED, 40 + k, noise_amp_for(op + 1.0), 0)
                got = dbb[k].cpu().numpy().view(np.complex128).reshape(-1)
                assert np.abs(got - want_bb).max() <= 1e-9 * np.abs(want_bb).max()
                assert np.array_equal(dpl[k].cpu().numpy()[: orc.payload_bytes], want_pl.astype(np.uint8))
            # transmit_byte: this set's preamble, pilots, scrambler and pre-equalization channel, down to the audio samples
            assert rx.pre_equalization_channel(oraclelib.CARRIER).tobytes() == orc.get_pre_equalization_channel(oraclelib.CARRIER).tobytes()
            msg = np.random.default_rng(cfg).integers(0, 256, (1, rx.payload_bytes), dtype=np.uint8)
            assert np.array_equal(rx.transmit_byte(msg, oraclelib.CARRIER)[0], orc.transmit_byte(msg[0].astype(np.int32)))
        rx.close()


def test_explicit_parameters_are_checked():
    from mercury_amd.physical_layer import MgpuError
    for bad in (dict(Nc=64), dict(Nfft=512), dict(Dx=2), dict(Dy=4), dict(Dy=5), dict(Nsymb=30), dict(Nsymb=64, Dy=2), dict(ls_window=23), dict(pilot_boost=-1.0)):
        with pytest.raises(MgpuError):
            _rx(8, explicit=bad)
    with pytest.raises(MgpuError):
        _rx(100, explicit=dict(Nsymb=100))                          # the MFSK modes take their frame length from the codeword
    rx = _rx(8, explicit=dict(Nc=50, Nfft=256, Dx=1, Dy=3, Nsymb=24))       # the reference's geometry spelled out = the defaults
    assert rx.ls_window == 21 and rx.Nsymb == 24 and rx.nPilots == 400
    rx.close()
    rx = _rx(8, explicit=dict(Nsymb=20, Dy=5))                      # the reference's LOW_DENSITY option for QPSK (telecom_system.cc:1828-1865)
    assert (rx.Nsymb, rx.nPilots, rx.nData, rx.nBits, rx.frame_samples) == (20, 200, 800, 1600, 20 * 272)
    rx.close()


@pytest.mark.parametrize("cfg", [0, 3, 5, 8, 9, 12])
def test_ldpc_spa_bit_exact_on_identical_llrs(cfg):
    """cl_ldpc::decode parity: same float LLRs in -> same hard bits and iteration count out, including
    frames that never converge (the GPU evaluates tanh/atanh with the reference libm's algorithm)."""
    orc = Oracle(cfg, 50)
    op = OPERATING_ESN0[cfg]
    snrs = [op - 1.0] * 6 + [op + 0.5] * 6 + [-15.0] * 3 + [op - 2.5] * 5
    bb, _ = _frames(orc, snrs, seed=77)
    llr = np.stack([orc.rx(b, FLAGS_BASEBAND_TEST | oraclelib.FLAG_NO_LDPC)["llr_ldpc"] for b in bb])
    rx = _rx(cfg, max_iters=50, max_batch=len(snrs))
    bits, iters = rx.ldpc_decode(llr)
    for f in range(len(snrs)):
        rb, ri = orc.ldpc_decode(llr[f])
        assert iters[f] == ri, (cfg, f, iters[f], ri)
        assert np.array_equal(bits[f], rb.astype(np.uint8)), (cfg, f, "bits differ", ri)


@pytest.mark.parametrize("cfg", [0, 1, 2, 4, 5, 8, 11, 16])          # one mode per code rate
def test_ldpc_spa_special_value_llrs_decode_like_the_reference(cfg):
    """cl_ldpc::decode on LLR words salted with +-Inf, NaN (a single one too: s_tanh.c keeps it a NaN and it spreads through the checks
    it touches), +-0, float denormals, FLT_MAX-scale values and exact ties: bits and iteration counts are the CPU's, whatever libm's
    tanh / atanh make of them (tests/tools/fuzz_special_values.py is the longer form; round 4 found tanh(NaN) = +-1 with it)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    from fuzz_special_values import salted_words
    orc = Oracle(cfg, 50)
    words = salted_words(np.random.default_rng(1000 + cfg), 32, orc.K, orc.N)
    rx = _rx(cfg, max_iters=50, max_batch=len(words))
    with np.errstate(all="ignore"):
        bits, iters = rx.ldpc_decode(words)
        for w in range(len(words)):
            rb, ri = orc.ldpc_decode(words[w])
            assert iters[w] == ri, (cfg, w, iters[w], ri)
            assert np.array_equal(bits[w], rb.astype(np.uint8)), (cfg, w, "bits differ", ri)
    rx.close()


@pytest.mark.parametrize("cfg", [0, 8, 16])
def test_hard_frames_are_decided_without_iterating_and_counted(cfg):
    """Every |LLR| >= 200 (what the zero-forcing modes hand over behind RX_SHM): tanh is +-1 for ever and the reference's iterations change no
    bit. The kernel skips them; bits and iteration counts stay the CPU's (which does iterate), and mgpu_decoder_hard_frames counts exactly the
    frames that were skipped - a clean hard word leaves at iteration 0 like any clean word and is not one of them."""
    orc = Oracle(cfg, 50)
    rng = np.random.default_rng(4200 + cfg)
    words = np.where(rng.random((10, orc.N)) < 0.03, -1.0, 1.0).astype(np.float32) * np.float32(1e30)       # the all-zero codeword with sign errors
    words[3] = np.float32(250.0) * np.sign(words[3])
    words[4] = np.where(words[4] < 0, -np.inf, np.inf).astype(np.float32)
    words[8] = np.float32(1e30)                                           # clean: parity holds at the first look
    words[9] = np.float32(np.inf)
    words[7, orc.N - 3] = np.float32(150.0)                               # not hard: iterates (and still cannot change a bit)
    words[6, rng.integers(0, orc.N, 40)] = np.float32(0.5)                # not hard either, and these bits CAN change
    # The shortcut's bound at its edge: every |LLR| EXACTLY the threshold 200, and the variable of highest degree (9 in these codes:
    # device_tables.h kSpaMaxVarDegree) attacked on every edge - one sign error among the other members of each of its checks, so all its incoming
    # messages are -16.81 against its +200: |Q| = 200 - 8 x 16.81 = 65.5 on its edges, still inside tanh's saturated range, no bit may change.
    checks, variables = oraclelib.ldpc_graph(orc.K)
    v_star = int(np.argmax([len(c) for c in variables]))
    assert len(variables[v_star]) == max(len(c) for c in variables) <= 9
    words[2] = np.float32(200.0)
    mine, taken = set(int(c) for c in variables[v_star]), set()
    for c in variables[v_star]:
        u = next(int(u) for u in checks[c] if u != v_star and u not in taken and not (set(int(x) for x in variables[u]) - {int(c)}) & mine)
        taken.add(u)
        words[2, u] = np.float32(-200.0)
    rx = _rx(cfg, max_iters=50, max_batch=len(words))
    before = rx.decoder_hard_frames()
    bits, iters = rx.ldpc_decode(words)
    assert rx.decoder_hard_frames() - before == 6
    assert bits[2].sum() == sum(u < orc.K for u in taken) and v_star < orc.K and bits[2][v_star] == 0      # the attacked variable and everybody else kept their signs (information positions)
    for w in range(len(words)):
        rb, ri = orc.ldpc_decode(words[w])
        assert iters[w] == ri and np.array_equal(bits[w], rb.astype(np.uint8)), (cfg, w, iters[w], ri)
    assert list(iters[[8, 9]]) == [0, 0] and all(i == 51 for i in iters[[0, 1, 2, 3, 4, 5, 7]])
    rx.close()


@pytest.mark.parametrize("cfg", [15, 16])
def test_zf_modes_in_the_receive_byte_variant_match_the_reference(cfg):
    """What RX_SHM feeds the decoder in the zero-forcing modes: the equalised pilots equal the pilots, the measured variance is ~1e-33 and
    the float LLRs are +-Inf / rounding noise. LLR bit patterns (NaNs in the same places), iteration counts, CRC and payload bytes are the
    CPU's from 60 dB down into the noise (the other tests run these two modes in the baseband_test variant, as the reference's BER loop does)."""
    orc = Oracle(cfg, 50)
    snrs = [60.0, 40.0, 30.0, 24.0, 20.0, 18.0, 16.0, 14.0, 12.0, 10.0, 6.0, 0.0, -15.0]
    bb, _ = _frames(orc, snrs, seed=78)
    rx = _rx(cfg, max_iters=50, agc=1, variance_source=1, max_batch=len(snrs))
    with np.errstate(all="ignore"):
        out = rx.receive(bb, want_llr=True)
        for f in range(len(snrs)):
            ref = orc.rx(bb[f], FLAGS_RECEIVE_BYTE)
            nan = np.isnan(ref["llr_ldpc"])
            got = out["llr_ldpc"][f]
            assert np.array_equal(np.isnan(got), nan), (cfg, f)
            assert np.array_equal(got[~nan].view(np.uint32), ref["llr_ldpc"][~nan].view(np.uint32)), (cfg, f)
            st = out["stats"][f]
            assert (st["iterations_done"], st["crc"], st["all_zeros"]) == (ref["iterations"], ref["crc"], ref["all_zeros"]), (cfg, f)
            assert np.array_equal(out["payload"][f], ref["bytes"].astype(np.uint8)), (cfg, f)
    rx.close()


@pytest.mark.parametrize("max_iters", [5, 20])
def test_ldpc_iteration_cap(max_iters):
    orc = Oracle(8, max_iters)
    bb, _ = _frames(orc, [0.0, 1.0, -15.0, 2.5], seed=5)
    llr = np.stack([orc.rx(b, oraclelib.FLAG_NO_LDPC)["llr_ldpc"] for b in bb])
    rx = _rx(8, max_iters=max_iters, max_batch=4)
    bits, iters = rx.ldpc_decode(llr)
    for f in range(4):
        rb, ri = orc.ldpc_decode(llr[f])
        assert iters[f] == ri and np.array_equal(bits[f], rb.astype(np.uint8))
    assert iters[2] == max_iters + 1


@pytest.mark.parametrize("weights", ["100,230,45,150", "0", "1000000", "20,40,5,10", "1000000,1000000,0,0", "0,1000000,1000000,1000000", "60,1000000,0,30"])
@pytest.mark.parametrize("cfg,max_iters", [(8, 50), (8, 1), (8, 2), (8, 3), (8, 4), (8, 9), (12, 50), (12, 2), (0, 12)])
def test_ldpc_spa_look_policy_changes_no_bit_and_no_count(cfg, max_iters, weights, monkeypatch):
    """ldpc.hip "adaptive": in a frame's first iterations the syndrome of an iteration's posteriors is tested either by a pass of its own or
    inside the next check pass; a judged look's sampled syndrome weight decides how many of the following looks (0, 1 or 2) are taken the
    second way (create.hip: MERCURY_SPA_SPEC_WEIGHT="first look: one, two; later looks: one, two"). Whatever the thresholds - the defaults,
    always inside the check pass, never, and mixtures that switch forms from look to look - bits and iteration counts are the reference's
    (ldpc_decoder_SPA.cc:176-196), at iteration caps that end a frame in either form."""
    monkeypatch.setenv("MERCURY_SPA_SPEC_WEIGHT", weights)
    orc = Oracle(cfg, max_iters)
    op = OPERATING_ESN0[cfg]
    snrs = [op + 6.0] * 3 + [op + 2.0] * 5 + [op + 0.5] * 5 + [op - 1.0] * 5 + [op - 2.5] * 3 + [-15.0] * 2
    bb, _ = _frames(orc, snrs, seed=1234)
    llr = np.stack([orc.rx(b, FLAGS_BASEBAND_TEST | oraclelib.FLAG_NO_LDPC)["llr_ldpc"] for b in bb])
    rx = _rx(cfg, max_iters=max_iters, max_batch=len(snrs))
    bits, iters = rx.ldpc_decode(llr)
    seen = set()
    for f in range(len(snrs)):
        rb, ri = orc.ldpc_decode(llr[f])
        seen.add(ri)
        assert iters[f] == ri, (cfg, max_iters, weights, f, iters[f], ri)
        assert np.array_equal(bits[f], rb.astype(np.uint8)), (cfg, max_iters, weights, f, "bits differ", ri)
    assert max_iters + 1 in seen and len(seen) >= 2        # the batch holds frames that leave early and frames that never do


@pytest.mark.parametrize("cfg", [2, 8, 13, 16])
def test_gbf_decoder_bit_exact(cfg):
    from mercury_amd import DEC_GBF
    orc = Oracle(cfg, 50)
    op = OPERATING_ESN0[cfg]
    bb, _ = _frames(orc, [op + 3, op + 4, op + 6, -15.0, 60.0], seed=9)
    llr = np.stack([orc.rx(b, FLAGS_BASEBAND_TEST | oraclelib.FLAG_NO_LDPC)["llr_ldpc"] for b in bb])
    rx = _rx(cfg, decoder=DEC_GBF, max_batch=8)
    bits, iters = rx.ldpc_decode(llr)
    for f in range(len(bb)):
        rb, ri = orc.ldpc_decode(llr[f], alg=0)
        assert iters[f] == ri, (cfg, f, iters[f], ri)
        assert np.array_equal(bits[f], rb.astype(np.uint8)), (cfg, f)


@pytest.mark.parametrize("cfg", [5, 8, 9, 13, 16])
def test_minsum_agrees_where_both_converge(cfg):
    """Min-sum is not the reference's algorithm: parity is defined on frames both decoders converge on
    (a converged word is a codeword)."""
    from mercury_amd import DEC_MINSUM
    orc = Oracle(cfg, 50)
    op = OPERATING_ESN0[cfg]
    snrs = [op + 1.0] * 16
    bb, payloads = _frames(orc, snrs, seed=21)
    variant = _variants(cfg)[0]
    rx = _rx(cfg, decoder=DEC_MINSUM, agc=variant[0], variance_source=variant[1], max_batch=len(snrs))
    out = rx.receive(bb)
    both = 0
    for f in range(len(snrs)):
        ref = orc.rx(bb[f], variant[2])
        if ref["iterations"] <= 50 and out["stats"]["iterations_done"][f] <= 50:
            both += 1
            assert np.array_equal(out["payload"][f], ref["bytes"].astype(np.uint8)), (cfg, f)
            assert out["stats"]["crc"][f] == 0
    assert both >= len(snrs) // 2


@pytest.mark.parametrize("cfg", list(range(17)))
def test_spa_fast_agrees_with_oracle_where_both_converge(cfg):
    """The fp32 sum-product decoder (MGPU_DEC_SPA_FAST) is not the reference's arithmetic: its parity is defined like the
    min-sum decoder's, on frames both it and the reference decoder converge on (a converged word is a codeword), and it
    must converge on at least as many of them as the reference decoder minus one frame in 16."""
    from mercury_amd import DEC_SPA_FAST
    orc = Oracle(cfg, 50)
    op = OPERATING_ESN0[cfg]
    snrs = [op + 1.0] * 12 + [op - 1.0] * 4
    bb, payloads = _frames(orc, snrs, seed=23)
    variant = _variants(cfg)[0]
    rx = _rx(cfg, decoder=DEC_SPA_FAST, agc=variant[0], variance_source=variant[1], max_batch=len(snrs))
    out = rx.receive(bb)
    both = ref_ok = 0
    for f in range(len(snrs)):
        ref = orc.rx(bb[f], variant[2])
        ref_ok += ref["iterations"] <= 50
        if ref["iterations"] <= 50 and out["stats"]["iterations_done"][f] <= 50:
            both += 1
            assert np.array_equal(out["payload"][f], ref["bytes"].astype(np.uint8)), (cfg, f)
            assert out["stats"]["crc"][f] == ref["crc"]
            assert abs(int(out["stats"]["iterations_done"][f]) - ref["iterations"]) <= 2
    assert both >= ref_ok - 1 and both >= 8


@pytest.mark.parametrize("cfg", [0, 8, 13, 16])
def test_fp32_decoders_track_the_fp64_posteriors_iteration_by_iteration(cfg):
    """The deterministic leg of the fp32 decoders' parity (their arithmetic is not the reference's, so bit-identity is not defined): on the
    SAME decoder-input LLRs, stopped after exactly k flooding iterations (max_iters = k, frames below the waterfall so that nothing
    converges earlier), the sign of every information bit's posterior must agree with the bit-exact fp64 decoder's on >= 99.9 % of the bits
    for the fp32 sum-product decoder (same rule, fp32 rounding: only posteriors within rounding of zero may differ) and >= 85 % for
    normalised min-sum (a different check-node rule: 95.8 % after one iteration on the rate-1/16 code, 89.8 % after ten; it also converges on
    other frames, so only the sum-product decoder is required to leave the same frames open). Same inputs, same schedule, k = 1, 2, 5, 10."""
    from mercury_amd import DEC_MINSUM, DEC_SPA, DEC_SPA_FAST
    orc = Oracle(cfg, 50)
    F = 64
    bb, _ = _frames(orc, [OPERATING_ESN0[cfg] - 2.5] * F, seed=31)
    flags = FLAGS_BASEBAND_TEST if cfg in (15, 16) else oraclelib.FLAGS_RECEIVE_BYTE
    llr = np.stack([orc.rx(b, flags | oraclelib.FLAG_NO_LDPC)["llr_ldpc"] for b in bb])
    for k in (1, 2, 5, 10):
        ref_bits, ref_it = _rx(cfg, max_iters=k, decoder=DEC_SPA, max_batch=F).ldpc_decode(llr)
        open_frames = ref_it == k + 1                        # the frames that ran all k iterations in the reference decoder
        assert open_frames.sum() >= F // 2, (cfg, k, int(open_frames.sum()))
        for dec, floor in ((DEC_SPA_FAST, 0.999), (DEC_MINSUM, 0.85)):
            bits, it = _rx(cfg, max_iters=k, decoder=dec, max_batch=F).ldpc_decode(llr)
            both = open_frames & (it == k + 1)
            agree = float((bits[both] == ref_bits[both]).mean())
            assert agree >= floor, (cfg, k, dec, agree)
            if dec == DEC_SPA_FAST:
                assert both.sum() >= open_frames.sum() - 2, (cfg, k, dec)       # and it leaves (almost) the same frames open


def test_negative_zero_llr_decides_bit_zero_in_every_decoder():
    """An LLR of -0.0: `LLR < 0` is false in the reference (ldpc_decoder_SPA.cc:211-214), so the hard decision is 0. A codeword of the
    all-zero word whose LLRs are +1 with -0.0 sprinkled in is therefore already a codeword (iterations 0, all bits 0) - in the fp64 kernel and
    in the fp32 decoders alike (round 4's fp32 sum-product took the sign bit of the clamped tanh and decided 1)."""
    from mercury_amd import DEC_MINSUM, DEC_SPA, DEC_SPA_FAST
    rng = np.random.default_rng(5)
    llr = np.ones((8, 1600), np.float32)
    for f in range(8):
        llr[f, rng.choice(1600, 40 * f, replace=False)] = -0.0
    assert np.signbit(llr).sum() == 40 * 28
    for cfg in (0, 8, 16):
        for dec in (DEC_SPA, DEC_SPA_FAST, DEC_MINSUM):
            bits, it = _rx(cfg, decoder=dec, max_batch=8).ldpc_decode(llr)
            assert not bits.any() and not it.any(), (cfg, dec, int(bits.sum()), it)


@pytest.mark.parametrize("max_iters", [1, 2, 5, 50])
def test_fast_decoders_keep_the_iteration_count_convention(max_iters):
    """cl_ldpc::decode's return value (ldpc_decoder_SPA.cc:25-218): 0 = the input already was a codeword, k = converged after k iterations,
    max+1 = never. The fp32 decoders test the syndrome inside every check pass (one pass more than iterations, no syndrome-only pass): at
    every max_iters their counts must stay in 0..max+1, be the fp64 decoder's on almost every frame (the arithmetic differs, so a frame
    may converge one iteration earlier or later), and a frame they report as converged must carry a CRC-clean payload as often as the
    reference decoder's does."""
    import torch
    from mercury_amd import DEC_MINSUM, DEC_SPA, DEC_SPA_FAST
    cfg, F = 8, 1024
    rx = {n: _rx(cfg, decoder=d, max_iters=max_iters, max_batch=F) for n, d in (("spa", DEC_SPA), ("fast", DEC_SPA_FAST), ("minsum", DEC_MINSUM))}
    st = torch.cuda.current_stream().cuda_stream
    bb = torch.empty((F, rx["spa"].frame_samples, 2), dtype=torch.float64, device="cuda")
    for esn0 in (OPERATING_ESN0[cfg] + 1.0, 40.0):
        rx["spa"].txgen_dev(SEED, 99 << 20, F, noise_amp_for(esn0), bb.data_ptr(), None, stream=st)
        torch.cuda.synchronize()
        res = {}
        for n, phy in rx.items():
            payload = torch.zeros((F, phy.payload_stride), dtype=torch.uint8, device="cuda")
            stats = torch.zeros((F, 6), dtype=torch.int32, device="cuda")
            phy.receive_dev(bb.data_ptr(), F, payload.data_ptr(), stats.data_ptr(), stream=st)
            torch.cuda.synchronize()
            res[n] = stats.cpu().numpy()
        it_ref = res["spa"][:, 0]
        assert it_ref.min() >= 0 and it_ref.max() <= max_iters + 1
        if esn0 == 40.0:
            assert (it_ref == 0).all()                              # noiseless: already a codeword
        for n in ("fast", "minsum"):
            it = res[n][:, 0]
            assert it.min() >= 0 and it.max() <= max_iters + 1, (n, max_iters)
            if esn0 == 40.0:
                assert (it == 0).all(), (n, max_iters)
            if n == "fast":
                assert (np.abs(it - it_ref) <= 1).mean() >= 0.99 and (it == it_ref).mean() >= 0.9, (max_iters, esn0, (it == it_ref).mean())
            conv = it <= max_iters
            assert (res[n][conv, 3] != 0).all(), (n, max_iters)    # converged on a codeword: the CRC of a mode-8 frame at this SNR holds
    for phy in rx.values():
        phy.close()


@pytest.mark.parametrize("cfg", list(range(17)) + [100, 101, 102])
def test_spa_fast_decode_rate_matches_reference_decoder(cfg):
    """on every mode, at its operating point and 1.5 dB below (inside the waterfall), the fp32
    sum-product decoder decodes at least the reference decoder's fraction of frames minus 0.5 %, and every frame both
    decode has the same payload. 2048 frames per point, generated on the device; the reference side is the bit-exact fp64
    kernel (itself checked against the CPU oracle by the tests above)."""
    import torch
    from mercury_amd import DEC_SPA, DEC_SPA_FAST
    F = 2048
    agc, vs = (0, 0) if cfg in (15, 16) else (1, 1)
    rx = {n: _rx(cfg, decoder=d, agc=agc, variance_source=vs, max_batch=F) for n, d in (("spa", DEC_SPA), ("fast", DEC_SPA_FAST))}
    st = torch.cuda.current_stream().cuda_stream
    bb = torch.empty((F, rx["spa"].frame_samples, 2), dtype=torch.float64, device="cuda")
    for off in (0.0, -1.5):
        amp = noise_amp_for(OPERATING_ESN0[cfg] + off)
        rx["spa"].txgen_dev(SEED, 77 << 20, F, amp, bb.data_ptr(), None, stream=st)
        torch.cuda.synchronize()
        res = {}
        for n, phy in rx.items():
            payload = torch.zeros((F, phy.payload_stride), dtype=torch.uint8, device="cuda")
            stats = torch.zeros((F, 6), dtype=torch.int32, device="cuda")
            phy.receive_dev(bb.data_ptr(), F, payload.data_ptr(), stats.data_ptr(), stream=st)
            torch.cuda.synchronize()
            res[n] = (payload.cpu().numpy(), stats.cpu().numpy())
        ok_ref, ok_fast = res["spa"][1][:, 3] != 0, res["fast"][1][:, 3] != 0
        assert ok_fast.mean() >= ok_ref.mean() - 0.005, (cfg, off, ok_ref.mean(), ok_fast.mean())
        both = ok_ref & ok_fast
        assert np.array_equal(res["spa"][0][both], res["fast"][0][both]), (cfg, off)
    for phy in rx.values():
        phy.close()


def test_txgen_matches_cpu_generator_and_round_trips():
    """The on-device generator follows the same Philox streams as the oracle's: identical payload bytes,
    time-domain samples equal up to libm ulps in the Box-Muller noise; and everything it makes decodes."""
    import torch
    cfg, F = 8, 64
    orc = Oracle(cfg, 50)
    rx = _rx(cfg, max_batch=F)
    amp = noise_amp_for(4.0)
    bb = torch.empty((F, rx.frame_samples, 2), dtype=torch.float64, device="cuda")
    pl = torch.empty((F, rx.payload_stride), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rx.txgen_dev(SEED, 1000, F, amp, bb.data_ptr(), pl.data_ptr(), stream=st)
    torch.cuda.synchronize()
    bbh = bb.cpu().numpy().view(np.complex128).reshape(F, -1)
    plh = pl.cpu().numpy()
    for f in (0, 1, 63):
        ref_bb, ref_pl = orc.gen_frame(SEED, 1000 + f, amp)
        assert np.array_equal(plh[f][: orc.payload_bytes], ref_pl.astype(np.uint8))
        assert np.abs(bbh[f] - ref_bb).max() <= 1e-9 * np.abs(ref_bb).max()
    out = rx.receive(bbh)
    assert (out["stats"]["message_decoded"] == 1).all()
    assert np.array_equal(out["payload"], plh)


def test_full_batch_round_trip_mode8():
    """BASELINE.json config[1] size (4096 mode-8 frames) through size-independent properties:
    every frame generated on the device at +2.5 dB must come back with CRC==0 and the sent payload,
    and a sample of frames is re-checked against the oracle bit for bit."""
    import torch
    cfg, F = 8, 4096
    rx = _rx(cfg, max_batch=F)
    amp = noise_amp_for(2.5)
    bb = torch.empty((F, rx.frame_samples, 2), dtype=torch.float64, device="cuda")
    sent = torch.empty((F, rx.payload_stride), dtype=torch.uint8, device="cuda")
    got = torch.empty((F, rx.payload_stride), dtype=torch.uint8, device="cuda")
    stats = torch.empty((F, 6), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rx.txgen_dev(SEED, 0, F, amp, bb.data_ptr(), sent.data_ptr(), stream=st)
    rx.receive_dev(bb.data_ptr(), F, got.data_ptr(), stats.data_ptr(), stream=st)
    torch.cuda.synchronize()
    s = stats.cpu().numpy()
    decoded = s[:, 3] == 1
    assert decoded.mean() > 0.97, decoded.mean()
    assert torch.equal(got[torch.from_numpy(decoded).cuda()], sent[torch.from_numpy(decoded).cuda()])
    orc = Oracle(cfg, 50)
    bbh = bb[:12].cpu().numpy().view(np.complex128).reshape(12, -1)
    for f in range(12):
        ref = orc.rx(bbh[f], FLAGS_RECEIVE_BYTE)
        assert s[f, 0] == ref["iterations"] and s[f, 1] == ref["crc"]
        assert np.array_equal(got[f].cpu().numpy(), ref["bytes"].astype(np.uint8))


def test_empty_and_oversize_batches():
    from mercury_amd import MgpuError
    rx = _rx(8, max_batch=4)
    out = rx.receive(np.zeros((0, rx.frame_samples), np.complex128))
    assert out["payload"].shape[0] == 0
    with pytest.raises(MgpuError):
        rx.receive(np.zeros((5, rx.frame_samples), np.complex128))
    # all-zero input: pilots vanish, variance/LLRs are NaN/inf in the reference too; must not hang
    out = rx.receive(np.zeros((2, rx.frame_samples), np.complex128))
    assert out["stats"]["message_decoded"].sum() == 0


def test_multipath_channel_mode16():
    """BASELINE.json config[3] shape at test size: 2-path channel, mode 16 (ZF estimator)."""
    cfg = 16
    orc = Oracle(cfg, 50)
    bb, payloads = _frames(orc, [30.0] * 6, seed=3, channel=1)
    rx = _rx(cfg, agc=0, variance_source=0, max_batch=8)
    out = rx.receive(bb, taps=True)
    for f in range(6):
        ref = orc.rx(bb[f], FLAGS_BASEBAND_TEST)
        assert _llr_close(out["llr_ldpc"][f], ref["llr_ldpc"]).all()
        assert out["stats"]["iterations_done"][f] == ref["iterations"]
        assert np.array_equal(out["payload"][f], ref["bytes"].astype(np.uint8))


@pytest.mark.parametrize("cfg", list(range(17)))
def test_gpu_against_committed_reference_vectors(cfg):
    """The HIP path against tests/golden/ (outputs of the compiled reference itself), no oracle in between
    except as the seeded input generator whose output digest is checked."""
    import hashlib
    import json
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    meta = json.load(open(os.path.join(here, "golden", "golden_rx.json")))
    arr = np.load(os.path.join(here, "golden", "golden_rx.npz"))
    orc = Oracle(cfg, 50)
    recs = meta["modes"][str(cfg)]["frames"]
    bbs = []
    for rec in recs:
        bb, _ = orc.gen_frame(SEED, rec["frame"], noise_amp_for(rec["esn0_db"]), rec["channel"])
        assert hashlib.sha256(bb.tobytes()).hexdigest() == rec["input_sha256"]
        bbs.append(bb)
    bbs = np.stack(bbs)
    for vname, agc, vs in (("baseband_test", 0, 0), ("receive_byte", 1, 1)):
        if cfg in (15, 16) and vname == "receive_byte":
            continue   # degenerate in the reference (variance ~1e-33), see _variants()
        rx = _rx(cfg, agc=agc, variance_source=vs, max_batch=len(recs))
        out = rx.receive(bbs, want_llr=True)
        for idx, rec in enumerate(recs):
            g = rec["variants"][vname]
            key = "cfg%d_f%d_%s" % (cfg, idx, vname)
            assert _llr_close(out["llr_ldpc"][idx], arr[key + "_llr_ldpc"]).all(), (cfg, idx, vname)
            assert out["stats"]["iterations_done"][idx] == g["iterations"], (cfg, idx, vname)
            assert out["stats"]["crc"][idx] == g["crc"] and out["stats"]["all_zeros"][idx] == g["all_zeros"]
            assert np.array_equal(out["payload"][idx], arr[key + "_bytes"]), (cfg, idx, vname)
        rx.close()


@pytest.mark.skipif(not EXACT_TRIG, reason="the host libm selects a non-FMA atan on this CPU")
def test_glibc_trig_on_device_matches_host_libm():
    """csrc/glibc_trig.h on the device: atan and sincos bit for bit the host libm's (what get_angle / set_complex and the receive
    mixer call, misc.cc:34-71, ofdm.cc:2331-2332) on 6 * 10^6 arguments over every range of both routines."""
    rx = _rx(8, max_batch=1)
    orc = Oracle(8, 50)
    rng = np.random.default_rng(11)
    n = 1 << 20
    sg = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    for xs in (sg * np.exp((rng.random(n) * 120 - 60) * np.log(2.0)), sg * rng.random(n), sg * (1 + 15 * rng.random(n)), sg * rng.random(n) / 16,
               sg * rng.random(n) * 3.15, sg * rng.random(n) * 2e4):
        a, s, c = rx.debug_glibc_trig(xs)
        ha, hs, hc = orc.libm_atan_sincos(xs)                       # the C library's own routines (numpy has SIMD ones of its own)
        ok = np.abs(xs) < 105414350.0                                # beyond: another reduction in glibc, not needed on this path
        assert np.array_equal(a, ha) and np.array_equal(s[ok], hs[ok]) and np.array_equal(c[ok], hc[ok])
        assert np.isnan(s[~ok]).all()
    rx.close()


def test_spa_math_on_device_matches_host_libm():
    """The decoder's device tanh/atanh (fdlibm restatement + guard-free division) against the host libm the
    reference calls, bit for bit, on a few million arguments spanning every branch and the decoder's ranges."""
    rx = _rx(8, max_batch=1)
    rng = np.random.default_rng(12345)
    n = 1 << 21
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    xs = np.concatenate([
        sign * np.exp2(rng.uniform(-60, 6, n)),                 # tanh arguments over 66 octaves
        rng.uniform(-25, 25, n),
        rng.uniform(-1, 1, n),                                  # atanh arguments
        np.tanh(rng.uniform(-20, 20, n)) * np.tanh(rng.uniform(-20, 20, n)),   # products of tanh's, as in the check update
        sign * (1.0 - np.exp(-rng.uniform(0, 36, n))),          # close to +-1
        sign * np.exp(-rng.uniform(0, 40, n)),
        np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 0.9999999, -0.9999999, 22.0, -22.0, 21.999999, 2.0 ** -55, 2.0 ** -54,
                  2.0 ** -28, 2.0 ** -29, 0.34657359027997264, 1.0397207708399179, 19.061547465398498, 38.0, 44.0, 1e300]),
        # round 5: the routines carry power-of-two multiples of fdlibm's intermediates and tanh lost its tiny-argument branch - every binade
        # down to the smallest denormal (the device's own division sequences and denormal handling are what this checks beyond the host test),
        # the smallest denormals themselves, and atanh around log1p's direct / normalised switch (x = 0.17157...) and its u = 2^k steps
        np.concatenate([s * np.ldexp(1.0 + rng.random(64), e) for e in range(-1074, -19) for s in (1.0, -1.0)]),
        np.arange(0, 4096, dtype=np.uint64).view(np.float64), -np.arange(0, 4096, dtype=np.uint64).view(np.float64),
        0.17157287525380990 * (1.0 + (rng.random(n >> 3) - 0.5) * 1e-6),
        np.concatenate([(2.0 ** k - 1) / (2.0 ** k + 1) * (1.0 + (rng.random(4096) - 0.5) * 1e-7) for k in range(1, 26)]),
    ])
    t, a = rx.debug_spa_math(xs)
    ref_t, ref_a = Oracle(8).libm_tanh_atanh(xs)      # the host libm, called from C exactly as the reference does
    bad_t = np.flatnonzero(t.view(np.uint64) != ref_t.view(np.uint64))
    bad_a = np.flatnonzero(a.view(np.uint64) != ref_a.view(np.uint64))
    assert bad_t.size == 0, (bad_t.size, xs[bad_t[:5]], t[bad_t[:5]], ref_t[bad_t[:5]])
    assert bad_a.size == 0, (bad_a.size, xs[bad_a[:5]], a[bad_a[:5]], ref_a[bad_a[:5]])


def test_bench_two_ranks_on_one_gpu():
    """The N>1 code path of bench.py (frame sharding by rank, barrier, MAX-time and counter reductions, one
    JSON line from rank 0) with two ranks sharing GPU 0 over gloo — the driver's 8-GPU run uses the same
    code with backend nccl and one GPU per rank."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29633", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--frames", "256", "--esn0", "2.5", "--backend", "gloo", "--share-device", "--no-extras"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2, r.stdout                # the full record, then the compact contract record as the LAST line
    j, c = json.loads(lines[0]), json.loads(lines[1])
    assert j["bench_full_record"] and r.stdout.rstrip().endswith(lines[1]) and len(lines[1]) <= 4096
    assert c["n_gpus"] == 2 and c["scaling"] == "weak" and c["unit"] == "frames/s" and c["steps"] == 2 and c["warmup"] == 1
    assert abs(c["value"] / j["value"] - 1) < 1e-5 and c["roofline"]["bound"] == "hbm" and 0 < c["roofline"]["frac"] < 1
    assert len(c["per_device"]) == 2 and all(row[3] > 0 and row[5] > 0 for row in c["per_device"])      # clock / power / kernel ms / wall ms of every rank
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["unit"] == "frames/s"
    assert j["decoded_fraction"] > 0.97            # both ranks' frames decode (disjoint frame ranges, same seed)
    assert abs(j["value"] - 2 * 256 * 2 / (j["ms_per_step"] * 2 / 1e3)) < 1e-6 * j["value"]
    assert "roofline" in j and "cpu_baseline" not in j
    assert [r["rank"] for r in j["per_rank"]] == [0, 1] and all(r["ldpc_kernel_ms"] > 0 and r["wall_ms"] > 0 for r in j["per_rank"])   # clock / power / kernel time of every rank


def test_bench_collective_path_over_rccl_and_two_ranks_share_one_gpu_fairly():
    """8-GPU readiness on a one-GPU box. (1) The collective code path of bench.py over RCCL itself (backend nccl: process group on the
    device, barrier, MAX / SUM all-reduces of device tensors) with one rank - RCCL refuses two ranks on one device, so the two-rank run
    stays on gloo. (2) Two ranks time-sharing GPU 0 (gloo) process together what one rank processes alone (measured: within 10 %; the test
    allows 30 %, two processes' kernels interleave at the driver's discretion and this suite must not fail on a timing): sharding adds
    nothing but the barrier (the per-rank share of the N = 2 line is half of the N = 1 line)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--steps", "6", "--warmup", "2", "--frames", "2048", "--esn0", "-15", "--no-extras", "--no-cpu-baseline"]

    def line(cmd, env=None):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        ls = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(ls) == 1, r.stdout
        return json.loads(ls[0])

    common += ["--line", "full"]

    one = line([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--force-dist", "--backend", "nccl"] + common,
               env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29641", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0"))
    assert one["n_gpus"] == 1 and one["avg_iters_per_frame"] == 50.0 and one["machine"]["compute_units"] == 256
    two = line([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29643",
                os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-device"] + common)
    assert two["n_gpus"] == 2 and two["avg_iters_per_frame"] == 50.0
    assert abs(two["value"] / one["value"] - 1.0) < 0.30, (one["value"], two["value"])


def test_bench_pool_two_contexts_on_one_gpu():
    """bench.py --pool: ONE process drives the devices through the C-ABI pool (include/mercury_pool.h), shards resident in each
    device's memory - the host shape of the reference's RX_SHM loop (telecom_system.cc:2266-2390). Two contexts sharing GPU 0
    here; `python bench.py --gpus N` (no torchrun) runs the same code on N GPUs. Also the decoder-only soak form."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for extra in ([], ["--ldpc-only", "--iters", "5"]):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--pool", "--share-device", "--steps", "2", "--warmup", "1",
               "--frames", "256", "--esn0", "2.5", "--no-extras"] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 2, r.stdout                 # full record, then the compact contract record (the last line)
        j, c = json.loads(lines[0]), json.loads(lines[1])
        assert len(lines[1]) <= 4096 and abs(c["value"] / j["value"] - 1) < 1e-5 and c["n_gpus"] == 2 and len(c["per_device"]) == 2
        assert "hard_frames_per_step" in c and all(row[3] > 0 for row in c["per_device"])
        assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["unit"] == "frames/s" and j["config"]["parallelism"].startswith("pool x2")
        assert abs(j["value"] - 2 * 256 * 2 / (j["ms_per_step"] * 2 / 1e3)) < 1e-6 * j["value"]
        assert "roofline" in j and len(j["pool_device_ms_per_step"]) == 2
        if extra:
            assert j["avg_iters_per_frame"] == 5.0           # noise-only LLRs: every codeword runs all 5 iterations
        else:
            assert j["decoded_fraction"] > 0.97               # both devices' frames decode (disjoint frame numbers, same seed)
    # one device through the pool: the CPU leg cross-checks the very frames the pool decoded
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--pool", "--steps", "2", "--warmup", "1", "--frames", "128",
           "--esn0", "2.5", "--cpu-sample-per-core", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])        # the compact record carries the CPU leg
    assert j["cpu_baseline"]["gpu_vs_cpu_mismatches"] == 0 and j["n_gpus"] == 1 and j["cpu_baseline"]["kind"] == "port"


def test_bench_dump_outputs_are_the_last_timed_step(tmp_path):
    """bench.py --dump-outputs DIR: the payload and stats of the LAST timed step. With two input batches cycled, 1 and 3 timed steps end on
    the same batch and must dump identical files (same arguments, same inputs, deterministic decoder), 2 steps end on the other batch; the
    contract line reports the steps it timed and ms_per_step."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps, lines = {}, {}
    for steps in (1, 2, 3):
        d = tmp_path / ("s%d" % steps)
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--frames", "256",
               "--esn0", "2.5", "--nbuf", "2", "--no-extras", "--no-cpu-baseline", "--line", "compact", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        lines[steps] = json.loads(r.stdout.strip().splitlines()[-1])
        dumps[steps] = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    for steps, c in lines.items():
        assert c["steps"] == steps and c["ms_per_step"] > 0
    one = dumps[1]
    assert set(one) == {"payload", "iterations_done", "crc", "all_zeros", "message_decoded", "variance", "snr_db"}
    assert all(v.dtype in (np.float32, np.float64) and len(v) == 256 for v in one.values())
    assert one["payload"].shape[1] >= Oracle(8, 50).payload_bytes and np.array_equal(one["payload"], one["payload"].astype(np.uint8))
    assert abs(one["message_decoded"].mean() - lines[1]["decoded_fraction"]) < 1e-5 and lines[1]["decoded_fraction"] > 0.97
    assert all(np.array_equal(one[k], dumps[3][k], equal_nan=True) for k in one)
    assert not np.array_equal(one["payload"], dumps[2]["payload"])


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5, 6, 12])
def test_decoder_only_all_eight_rates_bpsk_llrs(cfg):
    """every LDPC rate with BPSK LLRs llr = 2y/sigma^2 around the waterfall, so that the
    batch mixes early exits, late convergence and failures; all-zero codeword + noise (linear code)."""
    orc = Oracle(cfg, 50)
    rng = np.random.default_rng(100 + cfg)
    rate = orc.K / 1600.0
    F = 24
    # Es/N0 for BPSK ~ a bit above capacity for the rate; spread over a few tenths of a dB
    base_db = {100: -9.5, 200: -7.0, 300: -5.3, 400: -4.0, 500: -2.9, 600: -1.9, 800: -0.2, 1400: 5.6}[orc.K]
    llr = np.zeros((F, 1600), np.float32)
    for f in range(F):
        snr = 10 ** ((base_db + 0.25 * (f % 8)) / 10)
        sigma = np.sqrt(1 / (2 * snr))
        y = 1.0 + sigma * rng.standard_normal(1600)
        llr[f] = (2 * y / sigma ** 2).astype(np.float32)
    rx = _rx(cfg, max_batch=F)
    bits, iters = rx.ldpc_decode(llr)
    conv = 0
    for f in range(F):
        rb, ri = orc.ldpc_decode(llr[f])
        assert iters[f] == ri, (cfg, f, iters[f], ri)
        assert np.array_equal(bits[f], rb.astype(np.uint8)), (cfg, f)
        conv += ri <= 50
    assert 0 < conv, "test SNRs should produce some converged frames"
    assert rate > 0


@pytest.mark.parametrize("F", [1, 3, 63, 65, 257])
def test_ragged_batch_sizes(F):
    cfg = 9
    orc = Oracle(cfg, 50)
    bb, payloads = _frames(orc, [OPERATING_ESN0[cfg] + (i % 3) for i in range(F)], seed=4242)
    rx = _rx(cfg, max_batch=300)
    out = rx.receive(bb)
    for f in sorted(set([0, F // 2, F - 1])):
        ref = orc.rx(bb[f], FLAGS_RECEIVE_BYTE)
        assert out["stats"]["iterations_done"][f] == ref["iterations"]
        assert np.array_equal(out["payload"][f], ref["bytes"].astype(np.uint8))
    assert (out["stats"]["message_decoded"] == 1).mean() > 0.9


@pytest.mark.parametrize("pinned", [False, True])
def test_host_path_in_several_chunks_equals_one_piece(pinned, monkeypatch):
    """mgpu_rx_batch's double-buffered host path (rx_batch.hip: input chunks on a copy stream, kernels on another, results through page-locked
    staging) cut into many chunks with a ragged tail - pageable and page-locked input take different stream schedules - returns what
    the same call in one piece returns, frame for frame (payload bytes, stats records, LLRs), and what the oracle returns."""
    from mercury_amd.physical_layer import pinned_empty
    cfg, F = 11, 203
    orc = Oracle(cfg, 50)
    op = OPERATING_ESN0[cfg]
    bb, _ = _frames(orc, [op + (i % 4) - 1.0 for i in range(F)], seed=515)
    if pinned:
        buf = pinned_empty(bb.shape, np.complex128)
        buf[...] = bb
        bb = buf
    rx = _rx(cfg, max_batch=256)
    monkeypatch.delenv("MERCURY_RX_CHUNK", raising=False)
    whole = rx.receive(bb, want_llr=True)
    for chunk in ("16", "37", "64"):
        monkeypatch.setenv("MERCURY_RX_CHUNK", chunk)
        for rep in range(2):
            cut = rx.receive(bb, want_llr=True)
            assert np.array_equal(cut["payload"], whole["payload"]), (chunk, rep)
            assert (cut["stats"] == whole["stats"]).all(), (chunk, rep)
            assert np.array_equal(cut["llr_ldpc"].view(np.uint32), whole["llr_ldpc"].view(np.uint32)), (chunk, rep)
    monkeypatch.delenv("MERCURY_RX_CHUNK", raising=False)
    for f in (0, 15, 16, 36, 37, 63, 64, 127, 128, 192, F - 1):
        ref = orc.rx(np.asarray(bb[f]), FLAGS_RECEIVE_BYTE)
        assert whole["stats"]["iterations_done"][f] == ref["iterations"] and whole["stats"]["crc"][f] == ref["crc"], f
        assert np.array_equal(whole["payload"][f], ref["bytes"].astype(np.uint8)), f
    rx.close()


@pytest.mark.parametrize("cfg", [2, 8, 16])
def test_front_end_and_decoder_halves_equal_the_fused_call(cfg):
    """mgpu_frontend_dev + mgpu_ldpc_batch_dev (device buffers, a caller's stream) = mgpu_rx_batch_dev: payload bytes, the stats records up to
    the variance and the LLRs in between, bit for bit; the launch timers (mgpu_enable_timing / kernel_ms_avg) report both kernels."""
    import torch
    rx = _rx(cfg, max_batch=96, agc=0 if cfg >= 15 else 1, variance_source=0 if cfg >= 15 else 1)
    F = 96
    dev = torch.device("cuda")
    bb = torch.empty((F, rx.frame_samples, 2), dtype=torch.float64, device=dev)
    rx.txgen_dev(SEED, 0, F, float(noise_amp_for(OPERATING_ESN0[cfg] + 0.5)), bb.data_ptr(), None)
    pay = [torch.zeros((F, rx.payload_stride), dtype=torch.uint8, device=dev) for _ in range(2)]
    st = [torch.zeros((F, 6), dtype=torch.int32, device=dev) for _ in range(2)]
    llr = [torch.zeros((F, 1600), dtype=torch.float32, device=dev) for _ in range(2)]
    var = torch.zeros((F,), dtype=torch.float32, device=dev)
    s = torch.cuda.Stream()
    rx.enable_timing(True)
    rx.receive_dev(bb.data_ptr(), F, pay[0].data_ptr(), st[0].data_ptr(), llr[0].data_ptr(), stream=s.cuda_stream)
    rx.frontend_dev(bb.data_ptr(), F, llr[1].data_ptr(), var.data_ptr(), stream=s.cuda_stream)
    rx.ldpc_decode_dev(llr[1].data_ptr(), F, d_payload=pay[1].data_ptr(), d_stats=st[1].data_ptr(), d_variance=var.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert torch.equal(llr[0].view(torch.int32), llr[1].view(torch.int32))
    assert torch.equal(pay[0], pay[1]) and torch.equal(st[0][:, :5], st[1][:, :5])       # all but snr_db (mercury_gpu.h: only the fused call
    if cfg == 16 or cfg == 8:                                                              # has the PSK / ZF modes' SNR inputs)
        assert not torch.equal(st[0][:, 5], st[1][:, 5])
    assert int((st[0][:, 3] == 1).sum()) > F * 0.9            # message_decoded
    fe_ms, dec_ms, launches = rx.kernel_ms_avg()
    assert 0 < fe_ms < 50 and 0 < dec_ms < 500 and launches >= 1
    rx.close()


@pytest.mark.parametrize("cfg", list(range(17)))
def test_fused_path_equals_the_reference_ber_loop_directly(cfg):
    """The frames the reference's OWN cl_telecom_system::baseband_test_EsN0 received (telecom_system.cc:95-229, compiled unmodified:
    oracle/ref_ts_harness.cc) through mgpu_rx_batch in that variant (agc = 0, variance from the un-equalised pilots): carrier grid,
    equalised grid, de-interleaved symbols, demapper LLRs and decoder-input LLRs against what the REAL run left in data_container - no
    restatement in between - bit for bit (the LLRs to 1e-5 where the host's libm is not the one the device restates), and the hard
    decisions of the real decoder through the payload bytes."""
    from oraclelib import RefTelecomSystem
    if not RefTelecomSystem.available():
        pytest.skip("oracle/_ref/libmercury_ref_ts.so not built")
    orc, ref = Oracle(cfg), RefTelecomSystem(cfg)
    op = OPERATING_ESN0[cfg]
    runs = [ref.baseband_test_one_frame(e) for e in (op, op + 1.0, op + 2.0, op - 3.0)]
    rx = _rx(cfg, max_iters=50, agc=0, variance_source=0, max_batch=len(runs))
    out = rx.receive(np.stack([r["baseband"] for r in runs]), taps=True)
    for f, r in enumerate(runs):
        for k in ("grid", "eq", "syms"):
            assert np.array_equal(out[k][f].view(np.uint64), r[k].view(np.uint64)), (cfg, f, k)
        for k in ("llr_demod", "llr_ldpc"):
            if EXACT_TRIG:
                assert np.array_equal(out[k][f].view(np.uint32), r[k].view(np.uint32)), (cfg, f, k)
            else:
                assert _llr_close(out[k][f], r[k]).all(), (cfg, f, k)
        # the real decoder's hard decisions = the data bits before de-scrambling; the library's payload is de-scrambled and packed: compare through the oracle's packing
        want = orc.rx(r["baseband"], FLAGS_BASEBAND_TEST)
        assert np.array_equal(want["bits"][: orc.nReal], r["decoded_bits"])
        assert np.array_equal(out["payload"][f], want["bytes"].astype(np.uint8)), (cfg, f)
        assert out["stats"]["iterations_done"][f] == want["iterations"], (cfg, f)
    rx.close()
    ref.close()


def test_descrambler_crc_and_stats_fields():
    """bit_energy_dispersal / bit_to_byte / CRC16 / all_zeros / SNR against the oracle for decoded, failed and
    all-zero outcomes (telecom_system.cc:1313-1372)."""
    cfg = 8
    orc = Oracle(cfg, 50)
    zeros = np.zeros(orc.payload_bytes, np.int32)
    frames = [orc.gen_frame(1, 1, noise_amp_for(6.0))[0], orc.gen_frame(1, 2, noise_amp_for(-15.0))[0]]
    # a frame carrying the all-zero PAYLOAD still has a non-zero CRC; the all_zeros flag needs every byte zero
    bits0 = orc.payload_to_bits(zeros)
    frames.append(orc.channel(orc.tx(bits0, 1), 5, 5, noise_amp_for(20.0)))
    bb = np.stack(frames)
    rx = _rx(cfg, max_batch=4)
    out = rx.receive(bb)
    for f in range(3):
        ref = orc.rx(bb[f], FLAGS_RECEIVE_BYTE)
        st = out["stats"][f]
        assert (st["iterations_done"], st["crc"], st["all_zeros"]) == (ref["iterations"], ref["crc"], ref["all_zeros"])
        decoded = not (ref["all_zeros"] or ref["crc"] != 0)
        assert st["message_decoded"] == int(decoded)
        if not decoded:
            assert abs(st["snr_db"] + 99.9) < 1e-4
        else:
            assert 0 < st["snr_db"] < 40


@pytest.mark.parametrize("cfg,esn0", [(0, -6.0), (8, 4.0), (10, 8.0), (13, 12.0), (15, 40.0), (16, 40.0), (16, 24.0)])
def test_receive_stats_snr_matches_reference_definition(cfg, esn0):
    """receive_stats.SNR (telecom_system.cc:1343-1396): 10log10(1/variance) for the LS modes (variance of the
    non-amplitude-restored equalisation for PSK), re-encode + measure_SNR for the zero-forcing modes,
    -99.9 when the frame did not decode."""
    orc = Oracle(cfg, 50)
    bb, _ = _frames(orc, [esn0, esn0 + 1, -15.0], seed=31)
    rx = _rx(cfg, max_batch=4)
    out = rx.receive(bb)
    for f in range(3):
        ref = orc.rx(bb[f], FLAGS_RECEIVE_BYTE)
        st = out["stats"][f]
        assert st["message_decoded"] == int(not (ref["all_zeros"] or ref["crc"] != 0))
        assert abs(float(st["snr_db"]) - ref["snr_db"]) <= 2e-5 * max(1.0, abs(ref["snr_db"])), (cfg, f, st["snr_db"], ref["snr_db"])


@pytest.mark.parametrize("cfg", list(range(17)))
def test_degenerate_inputs_behave_like_the_reference(cfg):
    """All-zero, denormal-scale, 1e150-scale, NaN / Inf polluted, sign-flipped and DC-only frames: whatever the
    reference arithmetic does with them (divisions by zero in the AGC, NaN variances, ...) the GPU does too —
    integer outputs identical, LLRs bit-identical where they are numbers, NaNs in the same places (x86 and CDNA
    differ only in the sign bit of a generated NaN)."""
    orc = Oracle(cfg, 50)
    n = orc.frame_samples
    good, _ = orc.gen_frame(5, 1, noise_amp_for(OPERATING_ESN0[cfg] + 6.0))
    cases = [np.zeros(n, np.complex128), good * 1e-300, good * 1e150, good.copy(), good.copy(), -good,
             np.full(n, 1 + 1j, np.complex128)]
    cases[3][100] = np.nan
    cases[4][200] = np.inf
    agc, vs, flags = _variants(cfg)[0]
    rx = _rx(cfg, max_batch=len(cases), agc=agc, variance_source=vs)
    with np.errstate(all="ignore"):
        out = rx.receive(np.stack(cases), want_llr=True)
        for i, x in enumerate(cases):
            ref = orc.rx(x, flags)
            got = out["llr_ldpc"][i]
            nan = np.isnan(ref["llr_ldpc"])
            assert np.array_equal(np.isnan(got), nan), (cfg, i)
            assert np.array_equal(got[~nan].view(np.uint32), ref["llr_ldpc"][~nan].view(np.uint32)), (cfg, i)
            st = out["stats"][i]
            assert (st["iterations_done"], st["crc"], st["all_zeros"]) == (ref["iterations"], ref["crc"], ref["all_zeros"]), (cfg, i)
            assert np.array_equal(out["payload"][i], ref["bytes"].astype(np.uint8)), (cfg, i)
    rx.close()


def test_single_frame_graph_path_equals_batched_path():
    """mgpu_rx_batch with F = 1 replays a captured hipGraph over fixed staging buffers (rx_batch.hip:rx_one_frame): many
    different frames through it, interleaved with batched calls, give exactly what the batched path gives."""
    cfg = 8
    orc = Oracle(cfg, 50)
    op = OPERATING_ESN0[cfg]
    snrs = [op, op + 2.0, -15.0, 60.0, op - 1.0, op + 0.5]
    bb, _ = _frames(orc, snrs, seed=4321)
    rx = _rx(cfg, max_batch=len(snrs))
    batch = rx.receive(bb)
    for rep in range(2):
        for f in range(len(snrs)):
            one = rx.receive(bb[f:f + 1])
            assert np.array_equal(one["payload"][0], batch["payload"][f]), (rep, f)
            assert one["stats"][0] == batch["stats"][f], (rep, f)
        again = rx.receive(bb)                     # the batched path still works after graph launches
        assert np.array_equal(again["payload"], batch["payload"]) and (again["stats"] == batch["stats"]).all()
    rx.close()


def test_single_frame_graph_survives_a_larger_batch_in_between():
    """on a FRESH context the order F = 1 (graph captured), F = max_batch (workspaces grow), F = 1 (graph replayed)
    must not replay the graph against a freed buffer: the graph owns its one-frame device buffer."""
    cfg = 8
    orc = Oracle(cfg, 50)
    op = OPERATING_ESN0[cfg]
    bb, _ = _frames(orc, [op, op + 1.0, -15.0, op + 3.0, 40.0, op - 1.0, op + 0.5, op + 2.0], seed=99)
    ref = _rx(cfg, max_batch=len(bb))
    want = ref.receive(bb)
    ref.close()
    rx = _rx(cfg, max_batch=len(bb))
    first = rx.receive(bb[2:3])                     # captures the graph before any batched workspace exists
    assert np.array_equal(first["payload"][0], want["payload"][2]) and first["stats"][0] == want["stats"][2]
    for rep in range(3):
        big = rx.receive(bb)                        # allocates / reuses the batched buffers
        assert np.array_equal(big["payload"], want["payload"]) and (big["stats"] == want["stats"]).all()
        for f in (0, 5, 7):
            one = rx.receive(bb[f:f + 1])           # replays the graph
            assert np.array_equal(one["payload"][0], want["payload"][f]) and one["stats"][0] == want["stats"][f], (rep, f)
    rx.close()


def test_generator_and_receiver_are_invariant_to_how_frames_are_sharded():
    """Frame-range sharding: frames are keyed by their global index, so generating / receiving them in one
    call, in two halves or rank by rank (frame_range) gives identical samples, payloads and statistics."""
    import torch
    from mercury_amd.sharding import frame_range
    cfg, F = 13, 96
    rx = _rx(cfg, max_batch=F)
    amp = noise_amp_for(OPERATING_ESN0[cfg] + 1.0)
    st = torch.cuda.current_stream().cuda_stream

    def run(frame0, n):
        bb = torch.empty((n, rx.frame_samples, 2), dtype=torch.float64, device="cuda")
        sent = torch.empty((n, rx.payload_stride), dtype=torch.uint8, device="cuda")
        got = torch.empty((n, rx.payload_stride), dtype=torch.uint8, device="cuda")
        stats = torch.empty((n, 6), dtype=torch.int32, device="cuda")
        rx.txgen_dev(SEED, frame0, n, amp, bb.data_ptr(), sent.data_ptr(), stream=st)
        rx.receive_dev(bb.data_ptr(), n, got.data_ptr(), stats.data_ptr(), stream=st)
        torch.cuda.synchronize()
        return bb, sent, got, stats

    whole = run(5000, F)
    for world in (2, 3, 8):
        parts = [run(5000 + frame_range(r, world, F)[0], frame_range(r, world, F)[1] - frame_range(r, world, F)[0]) for r in range(world)]
        for i in range(4):
            assert torch.equal(torch.cat([p[i] for p in parts]), whole[i]), (world, i)
    rx.close()


def _load_graph(K):
    """check -> variable lists of the rate with K information bits, from the library's derived table blob."""
    import struct
    blob = open(oraclelib.TABLES, "rb").read()
    assert blob[:4] == b"MLDP"
    nrates = struct.unpack_from("<I", blob, 8)[0]
    off = 12
    for _ in range(nrates):
        k, P, N, E, cw, vw = struct.unpack_from("<6I", blob, off)
        off += 24
        cdeg = np.frombuffer(blob, np.uint8, P, off)
        C = np.frombuffer(blob, np.uint16, E, off + P)
        if k == K:
            rows, e = [], 0
            for d in cdeg:
                rows.append(C[e: e + int(d)].astype(int))
                e += int(d)
            return rows, P, N
        off += P + 2 * E + N + 2 * E
    raise AssertionError("rate not in blob")


@pytest.mark.parametrize("cfg,decoder", [(6, "spa"), (12, "spa"), (0, "spa"), (6, "minsum"), (12, "minsum")])
def test_decoder_symmetry_under_codeword_sign_flips(cfg, decoder):
    """Linearity of the code + sign symmetry of belief propagation: flipping the LLR signs along ANY codeword c turns the
    decoder's output into output XOR c with the SAME iteration count — bit for bit, converged or not (tanh / atanh are odd
    and IEEE rounding is symmetric). Size-independent property; c is built by IRA-encoding random information bits with
    the graph from the library's table blob (ldpc.cc:111-132)."""
    from mercury_amd import DEC_MINSUM, DEC_SPA
    orc = Oracle(cfg, 50)
    rows, P, N = _load_graph(orc.K)
    K = orc.K
    rng = np.random.default_rng(cfg)
    F = 24
    sigma = {6: 0.82, 12: 0.40, 0: 1.6}[cfg]
    llr0 = (2.0 * (1.0 + sigma * rng.standard_normal((F, N))) / sigma ** 2).astype(np.float32)     # all-zero codeword + AWGN
    llr0[-4:] = rng.standard_normal((4, N)).astype(np.float32)                                      # pure noise: never converges
    cw = np.zeros((F, N), np.uint8)
    cw[:, :K] = rng.integers(0, 2, (F, K))
    for i in range(P):                                        # parity i = XOR of the other entries of check row i
        acc = np.zeros(F, np.uint8)
        for v in rows[i]:
            if v != K + i:
                acc ^= cw[:, v]
        cw[:, K + i] = acc
    for i in range(P):                                        # every check is satisfied: c is a codeword
        assert not np.bitwise_xor.reduce(cw[:, rows[i]], axis=1).any()
    rx = _rx(cfg, max_iters=50, decoder=DEC_SPA if decoder == "spa" else DEC_MINSUM, max_batch=F)
    b0, i0 = rx.ldpc_decode(llr0)
    b1, i1 = rx.ldpc_decode(llr0 * (1.0 - 2.0 * cw).astype(np.float32))
    assert np.array_equal(i0, i1)
    assert np.array_equal(b1, b0 ^ cw[:, :K])
    assert (i0[:-4] <= 50).sum() >= F // 2 and (i0[-4:] == 51).all()       # both regimes are exercised
    rx.close()


def test_entry_points_reject_bad_arguments_without_crashing():
    """Every entry point returns MGPU_ERR_ARG (1) with a message for null pointers, F / W beyond max_batch or negative
    sizes, and MGPU_ERR_ARG / UNSUPPORTED for mode mismatches — never a crash, never exit() (the reference exits on bad
    set-up, ldpc.cc:246-256)."""
    import ctypes as C
    from mercury_amd import load_library
    lib = load_library()
    rx = _rx(8, max_batch=4)
    h = rx.h
    buf = np.zeros(4 * rx.frame_samples * 2)
    pay = np.zeros(4 * rx.payload_stride, np.uint8)
    st = np.zeros(4 * 24, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    calls = [
        lambda: lib.mgpu_rx_batch(h, None, 1, p(pay), p(st), None),
        lambda: lib.mgpu_rx_batch(h, p(buf), 5, p(pay), p(st), None),               # F > max_batch
        lambda: lib.mgpu_rx_batch(h, p(buf), -1, p(pay), p(st), None),
        lambda: lib.mgpu_ldpc_batch(h, None, 1, p(pay), p(st)),
        lambda: lib.mgpu_ldpc_batch(h, p(buf), 9, p(pay), p(st)),
        lambda: lib.mgpu_rx_batch_dev(h, None, 1, None, None, None, None),
        lambda: lib.mgpu_frontend_dev(h, None, 1, None, None, None),
        lambda: lib.mgpu_ldpc_batch_dev(h, None, 1, None, None, None, None, None, None),
        lambda: lib.mgpu_txgen_dev(h, 1, 0, 1, 0.1, 7, None, None, None),
        lambda: lib.mgpu_passband_to_baseband(h, None, 1, 100, None, 0, None, 10, 1, None),
        lambda: lib.mgpu_passband_to_baseband(h, p(buf), 1, 100, p(buf), 3, None, 10, 1, p(buf)),   # filter id
        lambda: lib.mgpu_time_sync_preamble(h, p(buf), 1, 10, 1, 0, 1, p(st), None),                # window shorter than the preamble
        lambda: lib.mgpu_freq_sync(h, p(buf), 1, 3, p(buf)),
        lambda: lib.mgpu_time_sync_mfsk(h, p(buf), 1, 100000, 0, p(st)),                             # OFDM mode
        lambda: lib.mgpu_detect_ack_pattern(h, p(buf), 1, 20000, 3, p(buf), None),                  # pattern id
        lambda: lib.mgpu_receive_byte_batch(h, p(buf), 1, None, None, p(pay), p(st)),
        lambda: lib.mgpu_receive_byte_batch(h, p(buf), 9, p(buf), None, p(pay), p(st)),
        lambda: lib.mgpu_symbol_demod(h, None, 1, None),
        lambda: lib.mgpu_psk_demod(h, None, 1, None, None),
        lambda: lib.mgpu_deinterleaver_f32(h, p(buf), 1, 10, 20, p(buf)),                           # block larger than the vector
        lambda: lib.mgpu_kernel_ms_avg(h, None, None),
    ]
    for i, call in enumerate(calls):
        rc = call()
        assert rc in (1, 4), (i, rc)
        assert lib.mgpu_last_error(h), i
    assert lib.mgpu_get_info(None, None) == 1 and lib.mgpu_enable_timing(None, 0) == 1
    lib.mgpu_destroy(None)                                        # no-op
    out = rx.receive(np.zeros((1, rx.frame_samples), np.complex128))   # the context is still usable afterwards
    assert out["stats"]["iterations_done"][0] == 0
    mf = _rx(100, max_batch=1)
    assert lib.mgpu_symbol_demod(mf.h, p(buf), 1, p(buf)) == 0     # plain FFT stage works in any mode
    assert lib.mgpu_channel_estimator(mf.h, p(buf), 1, p(buf)) == 1   # the estimator stages exist for the OFDM modes only
    mf.close()
    rx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [0, 1, 2, 4, 5, 8, 11, 16, 100, 102])     # the 8 code rates (+ the MFSK modes' reuse of 1/16 and 4/16)
def test_ldpc_encode_matches_oracle_and_decodes_back(cfg):
    """cl_ldpc::encode (ldpc.cc:111-132) for a batch: bit-exact parity bits; every encoded word is a codeword (0 iterations) and a
    word with a few weak wrong bits decodes back to the data."""
    from mercury_amd import RxPhy
    orc = oraclelib.Oracle(cfg)
    rx = RxPhy(cfg, max_batch=8)
    rng = np.random.default_rng(cfg)
    data = rng.integers(0, 2, (6, orc.K)).astype(np.uint8)
    data[0] = 0
    data[1] = 1
    enc = rx.ldpc_encode(data)
    assert enc.shape == (6, 1600)
    for f in range(6):
        assert np.array_equal(enc[f], orc.ldpc_encode(data[f].astype(np.int32))), (cfg, f)
    llr = np.where(enc == 1, -4.0, 4.0).astype(np.float32)            # the reference's sign convention: negative LLR = bit 1
    bits, iters = rx.ldpc_decode(llr)
    assert np.array_equal(bits, data) and not np.any(iters)
    noisy = llr.copy()
    noisy[:, rng.choice(1600, 12, replace=False)] *= -0.25
    bits, iters = rx.ldpc_decode(noisy)
    assert np.array_equal(bits, data) and np.all(iters >= 1) and np.all(iters <= 50)


@pytest.mark.parametrize("cfg", [8, 0, 16, 101])
def test_baseband_test_esn0_counts_match_the_oracle_frame_for_frame(cfg):
    """mgpu_baseband_test_esn0 (the reference's BER_PLOT_baseband self-simulation, telecom_system.cc:96-229, :2393-2480) against the CPU
    oracle fed the very same generated frames: bit errors, frame errors and iteration totals per Es/N0 point must be equal, across
    batch boundaries (max_batch 40, 96 frames per point) and with the points' frame ranges laid end to end."""
    agc, vs, flags = _variants(cfg)[-1] if cfg < 100 else (1, 1, oraclelib.FLAGS_RECEIVE_BYTE)
    orc = Oracle(cfg, 50)
    rx = _rx(cfg, max_batch=40, agc=agc, variance_source=vs)
    pts = [OPERATING_ESN0[cfg] - 3.0, OPERATING_ESN0[cfg] - 1.5, OPERATING_ESN0[cfg] + 2.0]
    n, seed, frame0 = 96, 77, 1000
    res = rx.baseband_test_esn0(pts, n, seed=seed, frame0=frame0)
    nreal = rx.nReal
    for p, esn0 in enumerate(pts):
        be = fe = it = 0
        for k in range(n):
            bb, pl = orc.gen_frame(seed, frame0 + p * n + k, noise_amp_for(esn0))
            ref = orc.rx(bb, flags)
            crc = 0xffff                                         # CRC16 (Modbus RTU) of the payload, as every frame carries it
            for byte in pl.astype(np.uint8).tolist():
                crc ^= byte
                for _ in range(8):
                    crc = (crc >> 1) ^ 0xA001 if crc & 1 else crc >> 1
            full = np.concatenate([pl.astype(np.uint8), np.array([crc & 0xff, crc >> 8], np.uint8), np.zeros(2, np.uint8)])   # spare bits are sent as 0
            sent = np.unpackbits(full, bitorder="little")[:nreal]
            got = np.unpackbits(ref["bytes"].astype(np.uint8), bitorder="little")[:nreal]
            e = int((sent != got).sum())
            be += e
            fe += e != 0
            it += ref["iterations"]
        r = res[p]
        assert (r["Error_bits_total"], r["Error_frames_total"], r["Frames_total"], r["Bits_total"]) == (be, fe, n, n * nreal), (cfg, esn0, r, be, fe)
        assert abs(r["avg_iterations"] * n - it) < 1e-6 and r["BER"] == be / (n * nreal) and r["FER"] == fe / n
    assert res[0]["Error_frames_total"] > 0 and res[2]["Error_frames_total"] <= res[0]["Error_frames_total"]      # a curve, not a constant
    rx.close()


def test_closing_a_context_releases_everything_it_made():
    """mgpu_destroy releases every resource of a context, the lazily created ones included (max_batch workspaces, the one-frame graph and its
    staging, the pipelined host path's streams / buffers / page-locked staging, the stage-tap buffers, receive_byte's workspace, upload
    staging and mixer table, the transmit state): eight cycles of create / use each once / close leave the device's free memory where it was."""
    import gc
    import torch
    from mercury_amd.physical_layer import pinned_empty
    from oraclelib import CARRIER
    W, F = 512, 64                  # 512 windows: receive_byte from host memory takes the pipelined upload (rb_stage / rb_compact)

    def free_hbm():
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info()[0]

    rng = np.random.default_rng(SEED)
    pb = rng.standard_normal((W, 1)) * 0.01
    first = free_hbm()
    for cycle in range(8):
        rx = _rx(8, max_batch=W)
        bb = (rng.standard_normal((F, rx.frame_samples)) + 1j * rng.standard_normal((F, rx.frame_samples))) * 0.1
        pinned = pinned_empty(bb.shape, np.complex128)
        pinned[...] = bb
        rx.receive(bb[:1])                                   # F = 1: the captured graph
        rx.receive(bb)                                       # F > 1, pageable: pipelined
        rx.receive(pinned)                                   # F > 1, page-locked: pipelined on the other schedule
        rx.receive(bb[:2], taps=True)
        passband = np.broadcast_to(pb, (W, rx.receive_buffer_samples())) * rng.standard_normal(rx.receive_buffer_samples())
        rx.receive_byte((passband * 32768).astype(np.int16), CARRIER)          # host memory, compact samples
        d_pass = torch.from_numpy(np.ascontiguousarray(passband)).cuda()
        rx.receive_byte_dev(d_pass.data_ptr(), W, CARRIER)                     # device memory
        rx.transmit_byte(np.zeros((2, rx.payload_stride), np.uint8), CARRIER)
        rx.passband_to_baseband(passband[:2], CARRIER)
        del d_pass, pinned
        in_use = first - free_hbm()
        rx.close()
        assert in_use >= 1 << 30, in_use                     # the context did hold its workspaces
        after = free_hbm()
        assert abs(after - first) < 256 << 20, (cycle, first, after)

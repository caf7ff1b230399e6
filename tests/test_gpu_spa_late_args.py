"""GPU tests of the fp64 sum-product kernels' late argument reads (ldpc.hip: SpaKernArgs / spa_late_args, profiles/NOTES.md R8.1): the epilogue's
tables, sizes and pointers are read from the kernel-argument segment behind the iteration loop, the iteration cap and the look thresholds
once per iteration. Every pointer the C ABI allows to be null is passed present and absent, one to three frames per launch, at iteration caps
that end a frame in every branch of the loop, for one mode of every kernel instance - bits, iteration counts, payload bytes and stats records
against the CPU oracle, bit for bit."""
import functools

import numpy as np
import pytest

import oraclelib
from conftest import OPERATING_ESN0
from oraclelib import FLAGS_BASEBAND_TEST, FLAGS_RECEIVE_BYTE, Oracle, noise_amp_for

CFGS = [0, 2, 8, 6, 16]             # rates 1/16, 3/16, 6/16, 8/16, 14/16: kernel instances ne4, ne5, ne6, ne6 (95 bins), ne8
CAPS = [1, 2, 9, 50]
KINDS = ("converges", "never", "hard")


@functools.lru_cache(maxsize=None)
def _words(cfg):
    """Three LLR words: a frame at the mode's operating Es/N0, one at -15 dB, a hard one (every |LLR| = 250, the all-zero codeword with one
    sign error, so a check is odd and the frame is decided before its first iteration)."""
    orc = Oracle(cfg, 50)
    llr = [orc.rx(orc.gen_frame(4711, i, noise_amp_for(snr))[0], FLAGS_BASEBAND_TEST | oraclelib.FLAG_NO_LDPC)["llr_ldpc"]
           for i, snr in enumerate((OPERATING_ESN0[cfg] + 0.5, -15.0))]
    hard = np.full(1600, 250.0, np.float32)
    hard[17] = -250.0
    out = np.stack(llr + [hard]).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(cfg, cap):
    """Per word: bits [K], iterations, payload bytes, crc, all_zeros - the oracle's decoder, then the reference's de-scrambling, bit packing
    and CRC restated with the oracle's scrambler and CRC (oraclelib.payload_tail)."""
    orc = Oracle(cfg, cap)
    ref = []
    for w in _words(cfg):
        bits, it = orc.ldpc_decode(w)
        by, crc, all_zeros = oraclelib.payload_tail(orc, bits)
        ref.append(dict(bits=bits.astype(np.uint8), iterations=it, bytes=by, crc=crc, all_zeros=all_zeros))
    return ref


def test_reference_frames_are_the_three_kinds():
    """(CPU) the oracle's verdict on the words the GPU tests use."""
    for cfg in CFGS:
        ref = _reference(cfg, 50)
        assert ref[0]["iterations"] <= 50 and ref[0]["crc"] == 0, (cfg, ref[0]["iterations"])       # converges, and decodes
        assert ref[1]["iterations"] == 51 and ref[2]["iterations"] == 51, cfg                          # never / hard with an odd check
        assert _reference(cfg, 1)[1]["iterations"] == 2 and _reference(cfg, 9)[2]["iterations"] == 10


# which optional pointers a launch gets: bits, iterations, payload, stats, variance
COMBOS = {"bits_only": (1, 1, 0, 0, 0), "payload_only": (0, 1, 1, 0, 0), "stats_variance_no_iterations": (0, 0, 1, 1, 1),
          "all_but_variance": (1, 1, 1, 1, 0), "stats_alone": (0, 0, 0, 1, 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("cfg", CFGS)
def test_every_output_combination_one_to_three_frames(cfg, cap):
    import torch
    from mercury_amd import RxPhy
    dev = torch.device("cuda")
    ref = _reference(cfg, cap)
    words = _words(cfg)
    rx = RxPhy(cfg, max_iters=cap, max_batch=4)
    K, nbytes, stride = rx.K, len(ref[0]["bytes"]), rx.payload_stride
    assert nbytes <= stride
    hard_before = rx.decoder_hard_frames()
    hard_expected = 0
    for F in (1, 2, 3):
        for first in range(3):                               # every kind of frame is frame 0 of a launch, and the last one
            order = [(first + i) % 3 for i in range(F)]
            d_llr = torch.from_numpy(np.ascontiguousarray(words[order])).to(dev)
            var_host = np.array([0.25, 0.5, 2.0], np.float32)[:F]
            for name, (wb, wi, wp, ws, wv) in COMBOS.items():
                bits = torch.full((F, K), 7, dtype=torch.uint8, device=dev)
                iters = torch.full((F,), -5, dtype=torch.int32, device=dev)
                pay = torch.full((F, stride), 0xEE, dtype=torch.uint8, device=dev)
                st = torch.full((F, 6), -7, dtype=torch.int32, device=dev)
                var = torch.from_numpy(var_host).to(dev)
                rx.ldpc_decode_dev(d_llr.data_ptr(), F, d_bits=bits.data_ptr() if wb else None, d_iters=iters.data_ptr() if wi else None,
                                   d_payload=pay.data_ptr() if wp else None, d_stats=st.data_ptr() if ws else None,
                                   d_variance=var.data_ptr() if wv else None)
                torch.cuda.synchronize()
                hard_expected += sum(1 for k in order if KINDS[k] == "hard")
                bits, iters, pay, st = bits.cpu().numpy(), iters.cpu().numpy(), pay.cpu().numpy(), st.cpu().numpy()
                for f, k in enumerate(order):
                    r, tag = ref[k], (cfg, cap, F, name, f, KINDS[k])
                    if wb:
                        assert np.array_equal(bits[f], r["bits"]), tag
                    else:
                        assert (bits[f] == 7).all(), tag                 # an absent output is not written
                    assert iters[f] == (r["iterations"] if wi else -5), tag + (int(iters[f]), r["iterations"])
                    if wp:
                        assert np.array_equal(pay[f, :nbytes], r["bytes"]), tag
                    else:
                        assert (pay[f] == 0xEE).all(), tag
                    if ws:
                        decoded = int(not (r["all_zeros"] or r["crc"] != 0))
                        assert list(st[f, :4]) == [r["iterations"], r["crc"], r["all_zeros"], decoded], tag + (list(st[f, :4]),)
                        variance, snr = st[f, 4:].view(np.float32)
                        assert variance == (var_host[f] if wv else 0.0), tag
                        with np.errstate(divide="ignore"):
                            want = np.float32(10.0 * np.log10(1.0 / np.float64(variance))) if decoded else np.float32(-99.9)
                        assert snr == want or abs(snr - want) <= 1e-5 * abs(want), tag + (snr, want)
                    else:
                        assert (st[f] == -7).all(), tag
    assert rx.decoder_hard_frames() - hard_before == hard_expected
    rx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [8, 16])
def test_chunked_host_path_hands_the_tail_each_chunks_own_pointers(cfg, monkeypatch):
    """mgpu_rx_batch cut into chunks of two frames (the ragged last chunk holds one): every chunk's launch gets its own payload / stats /
    variance pointers, both variance inputs present - frame for frame the oracle's payload bytes, iteration counts, CRC, variance and SNR."""
    from mercury_amd import RxPhy
    orc = Oracle(cfg, 50)
    op = OPERATING_ESN0[cfg]
    agc, vs, flags = (0, 0, FLAGS_BASEBAND_TEST) if cfg >= 15 else (1, 1, FLAGS_RECEIVE_BYTE)
    snrs = [op + 0.5, -15.0, op + 2.0, op - 1.0, op + 0.5]
    bb = np.stack([orc.gen_frame(99, i, noise_amp_for(s))[0] for i, s in enumerate(snrs)])
    rx = RxPhy(cfg, max_iters=50, agc=agc, variance_source=vs, max_batch=8)
    monkeypatch.setenv("MERCURY_RX_CHUNK", "2")
    out = rx.receive(bb)
    monkeypatch.delenv("MERCURY_RX_CHUNK", raising=False)
    for f in range(len(snrs)):
        ref = orc.rx(bb[f], flags)
        st = out["stats"][f]
        assert (st["iterations_done"], st["crc"], st["all_zeros"]) == (ref["iterations"], ref["crc"], ref["all_zeros"]), (cfg, f)
        assert np.array_equal(out["payload"][f][: len(ref["bytes"])], ref["bytes"].astype(np.uint8)), (cfg, f)
        # the two variance inputs, as the tail read them through its late-loaded pointers: stats.variance is the float the front-end left
        # (to two float ulps: where the host's libm is not the restated one the double behind it may differ in its last bits) and, in the PSK
        # mode, stats.snr_db comes from the OTHER input (snr_variance_in: the variance of the equalisation without amplitude restoration),
        # to the bound tests/test_gpu_parity.py holds this field to (float rounding of 10 log10)
        assert st["message_decoded"] == int(not (ref["all_zeros"] or ref["crc"] != 0)), (cfg, f)
        if np.isfinite(ref["variance_f"]):
            assert abs(np.float64(st["variance"]) - np.float64(np.float32(ref["variance_f"]))) <= 2.0 ** -22 * abs(np.float64(ref["variance_f"])), (cfg, f, st["variance"], ref["variance_f"])
        if flags == FLAGS_RECEIVE_BYTE:
            assert abs(float(st["snr_db"]) - ref["snr_db"]) <= 2e-5 * max(1.0, abs(ref["snr_db"])), (cfg, f, st["snr_db"], ref["snr_db"])
    rx.close()

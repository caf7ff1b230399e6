"""The yardsticks of tests/stages_ref.py against the CPU oracle - and against the reference's own objects where they were built - before
tests/test_gpu_stages.py lets them judge a kernel. No GPU.

One mode per constellation size and both estimators of the mode table, one explicit combination, noisy frames in both variants of the span:
the stage outputs the oracle hands out are tied to one another by the numpy models, so a model that is wrong cannot agree with them."""
import numpy as np
import pytest

import stages_ref as S
from conftest import EXPLICIT_COMBOS, OPERATING_ESN0, SEED
from oraclelib import FLAG_NO_LDPC, FLAGS_BASEBAND_TEST, FLAGS_RECEIVE_BYTE, Oracle, RefLib, noise_amp_for


def _explicit_cfg(row):
    from mercury_amd.physical_layer import cfg_explicit
    return cfg_explicit(*row[:4]), row[4]


X_CFG, X_ESN0 = _explicit_cfg(EXPLICIT_COMBOS[3])          # 8PSK, rate 3/16, LS
MODES = [(0, OPERATING_ESN0[0]), (8, OPERATING_ESN0[8]), (11, OPERATING_ESN0[11]), (13, OPERATING_ESN0[13]), (15, OPERATING_ESN0[15]),
         (16, OPERATING_ESN0[16]), (X_CFG, X_ESN0)]


def _checkers(cfg):
    return [Oracle(cfg, 50)] + ([RefLib(cfg, 50)] if RefLib.available() else [])


@pytest.mark.parametrize("cfg,esn0", MODES, ids=[str(c) for c, _ in MODES])
def test_the_models_tie_the_oracles_stage_outputs_together(cfg, esn0):
    gen = Oracle(cfg, 50)
    frames = [gen.gen_frame(SEED, f, noise_amp_for(snr))[0] for f, snr in enumerate((esn0, esn0 - 2.0, esn0 + 1.0))]
    for chk in _checkers(cfg):
        assert (chk.M, chk.nData, chk.nBits, chk.tf_blk, chk.bit_blk) == (gen.M, gen.nData, gen.nBits, gen.tf_blk, gen.bit_blk)
        data_cells = np.flatnonzero(chk.frame_types() == 0)
        assert data_cells.size == chk.nData and chk.nReal + chk.nVirtual == chk.K and chk.K + chk.P == chk.N == 1600
        assert chk.nReal + chk.P <= chk.nBits <= chk.N
        scr, const = chk.scrambler(), chk.constellation()
        for flags in (FLAGS_RECEIVE_BYTE, FLAGS_BASEBAND_TEST):
            for f, bb in enumerate(frames):
                ref = chk.rx(bb, flags)
                where = (cfg, type(chk).__name__, flags, f)
                assert S.same_bits(S.deinterleave(ref["eq"][data_cells], chk.tf_blk), ref["syms"]), where
                assert np.float32(ref["variance"]) == np.float32(ref["variance_f"])
                llr = S.psk_demod(ref["syms"], [ref["variance_f"]], const)[0]
                assert S.same_bits(llr, ref["llr_demod"]), (where, np.flatnonzero(llr != ref["llr_demod"])[:8])
                dei = S.deinterleave(ref["llr_demod"], chk.bit_blk)
                assert S.same_bits(S.repack(dei, chk.nReal, chk.nVirtual, chk.P)[: chk.N], ref["llr_ldpc"][: chk.N]), where
                bits = ref["bits"][: chk.nReal]
                assert np.array_equal(S.bit_to_byte(S.dispersal(bits, scr)), ref["bytes"].astype(np.uint8)), where
                assert ref["bytes"].max() <= 255
                if not ref["all_zeros"]:
                    assert int(S.crc16(ref["bytes"][: chk.nReal // 8])) == ref["crc"], where


def test_the_psk_model_sees_what_the_reference_does_with_special_values():
    """The oracle's own cl_psk::demod restatement is reachable only through rx(); the model is held to it on noise-only and on degenerate
    frames too (all zero: the AGC makes NaN of everything; one NaN sample), where the minima start at a NaN or an infinity."""
    for cfg in (8, 13, 16):
        orc = Oracle(cfg, 50)
        rng = np.random.default_rng(cfg)
        noise = rng.standard_normal(orc.frame_samples) + 1j * rng.standard_normal(orc.frame_samples)
        nan = orc.gen_frame(SEED, 1, noise_amp_for(OPERATING_ESN0[cfg]))[0]
        nan[3 * orc.Nofdm + orc.Ngi + orc.Nfft // 2] = complex(np.nan, np.nan)
        for bb in (noise, np.zeros(orc.frame_samples, np.complex128), nan, 1e160 * noise):
            for flags in (FLAGS_RECEIVE_BYTE, FLAGS_BASEBAND_TEST):
                ref = orc.rx(bb, flags | FLAG_NO_LDPC)
                llr = S.psk_demod(ref["syms"], [ref["variance_f"]], orc.constellation())[0]
                assert S.same_bits(llr, ref["llr_demod"]), (cfg, flags)


@pytest.mark.parametrize("cfg", [8, 11, 16])
def test_the_crc_model_is_the_oracles(cfg):
    orc = Oracle(cfg, 50)
    rng = np.random.default_rng(100 + cfg)
    assert int(S.crc16(np.zeros(0, np.uint8))) == 0xFFFF == orc.crc16(np.zeros(0, np.int32))
    for n in (0, 1, 2, orc.nReal // 8):
        rows = rng.integers(0, 256, (5, n), dtype=np.uint8)
        got = S.crc16(rows)
        assert got.shape == (5,) and got.dtype == np.uint16
        for r in range(5):
            assert int(got[r]) == orc.crc16(rows[r].astype(np.int32)), (cfg, n, r)
    if RefLib.available():
        ref = RefLib(cfg, 50)
        row = rng.integers(0, 256, orc.nReal // 8, dtype=np.uint8)
        assert int(S.crc16(row)) == ref.crc16(row.astype(np.int32))
    assert int(S.crc16(np.frombuffer(b"123456789", np.uint8))) == 0x4B37          # the catalogue's check value of CRC-16/MODBUS


@pytest.mark.parametrize("n,bs", [(7, 7), (7, 1), (10, 3), (1, 1), (257, 16), (1599, 159)])
def test_the_deinterleave_model_is_the_literal_double_loop(n, bs):
    x = np.random.default_rng(n * 100 + bs).standard_normal((3, n))
    want = x.copy()                                        # the tail stays
    nb = n // bs
    for r in range(3):
        for i in range(nb):
            for j in range(bs):
                want[r, i * bs + j] = x[r, j * nb + i]
    assert np.array_equal(S.deinterleave(x, bs), want)
    assert np.array_equal(S.deinterleave(x[1], bs), want[1])
    assert (n % bs == 0) or np.array_equal(want[:, nb * bs:], x[:, nb * bs:])


def test_bit_to_byte_model_packs_lsb_first_and_keeps_a_partial_byte():
    assert S.bit_to_byte(np.array([1, 0, 0, 0, 0, 0, 0, 0, 1, 1])).tolist() == [1, 3]
    assert S.bit_to_byte(np.array([[0, 1, 1]])).tolist() == [[6]]
    bits = np.random.default_rng(2).integers(0, 2, (4, 257), dtype=np.uint8)
    assert np.array_equal(S.bit_to_byte(bits), np.packbits(bits, axis=-1, bitorder="little"))

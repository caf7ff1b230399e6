"""GPU tests of the per-method RX stage entry points (include/mercury_stages.h; csrc/stages.hip, csrc/stages_api.hip) at more than one frame
per call, on explicit geometries and at the edges of their arguments.

a. every stage against the CPU oracle, fed the oracle's own previous stage (exactness as test_gpu_parity.stages_match_oracle has it);
b. the header's promise: the chained stage calls equal the taps of mgpu_rx_batch_taps, bit for bit (device against device);
c. row f of a 65-frame call equals the one-frame call on frame f, byte for byte, for every stage;
d. the free functions (symbol_demod, the de-interleavers, the integer tail) at sizes that are no multiple of anything;
e. psk_demod on ties, infinities, NaNs, overflowing distances and degenerate variances against the float32 model of cl_psk::demod;
f. bad arguments are refused with MGPU_ERR_ARG and a message, and the context goes on working.

The numpy models are tests/stages_ref.py's, proven on the CPU by tests/test_stages_host.py.
Batches: 65 frames at the mode's operating Es/N0 with a noiseless, an all-zero and a single-NaN frame at 31, 32, 33; the 3-frame batch is
(NaN, noisy, zero) and the 1-frame batch frame 0, so a frame that leaks into its neighbour shows."""
import functools

import numpy as np
import pytest

import stages_ref as S
from conftest import EXPLICIT_COMBOS, OPERATING_ESN0, SEED
from oraclelib import FLAG_AGC, FLAG_NO_LDPC, FLAG_VAR_EQ, FLAGS_RECEIVE_BYTE, Oracle, noise_amp_for
from stages_ref import Stages, same_bits
from test_gpu_parity import EXACT_TRIG, _llr_close, _variants

pytestmark = pytest.mark.gpu

DY5 = dict(Dy=5, Nsymb=20)          # test_gpu_estimator_ladder.DY5: mode 8 on the reference's LOW_DENSITY pilot lattice (the general lattice)
MFSK = 100


def _x_cfg():
    from mercury_amd.physical_layer import cfg_explicit
    return cfg_explicit(*EXPLICIT_COMBOS[3][:4])        # 8PSK, rate 3/16, 3 preamble symbols, LS


# one table mode per constellation size (16: zero forcing; 0, 8, 11: amplitude restoring; 13: LS without), an EXPLICIT_COMBOS row, and the
# Dy = 5 lattice with a 9-cell window (clipped at every edge) and another pilot boost
MODES = {"0": (0, None, OPERATING_ESN0[0]), "8": (8, None, OPERATING_ESN0[8]), "11": (11, None, OPERATING_ESN0[11]),
         "13": (13, None, OPERATING_ESN0[13]), "16": (16, None, OPERATING_ESN0[16]), "x-8psk-3/16": (_x_cfg(), None, EXPLICIT_COMBOS[3][4]),
         "8-dy5-w9": (8, dict(DY5, ls_window=9, pilot_boost=1.7), OPERATING_ESN0[8])}
BATCH = {1: [0], 3: [33, 34, 32], 65: list(range(65))}
CLEAN, ZERO, NAN = 31, 32, 33


def _rx(cfg, **kw):
    from mercury_amd import RxPhy
    return RxPhy(cfg, **kw)


@functools.lru_cache(maxsize=None)
def _case(mode):
    """-> (oracle, the 65 frames [65, samples]) of a mode; read only"""
    cfg, explicit, esn0 = MODES[mode]
    orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
    bb = np.stack([orc.gen_frame(SEED, f, 0.0 if f == CLEAN else noise_amp_for(esn0))[0] for f in range(65)])
    bb[ZERO] = 0
    bb[NAN, 3 * orc.Nofdm + orc.Ngi + orc.Nfft // 2] = complex(np.nan, np.nan)
    bb.setflags(write=False)
    return orc, bb


@functools.lru_cache(maxsize=None)
def _refs(mode, flags):
    """the oracle's stage outputs of the 65 frames, stacked: {key: [65, ...]}; read only"""
    orc, bb = _case(mode)
    with np.errstate(all="ignore"):
        rows = [orc.rx(b, flags | FLAG_NO_LDPC) for b in bb]
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in ("grid", "H", "H_noamp", "eq", "syms", "llr_demod", "llr_ldpc", "variance", "variance_f")}
    out["variance_f"] = out["variance_f"].astype(np.float32)
    for v in out.values():
        v.setflags(write=False)
    return out


def _exact(orc):
    return EXACT_TRIG or not orc.amp_restore


def _complex_ok(got, ref, exact):
    """stages_match_oracle's bar for H, eq and syms, frame by frame, with the NaNs and infinities of the degenerate frames held in place"""
    if exact:
        return same_bits(got, ref)
    for g, r in zip(got, ref):
        g, r = g.view(np.float64), r.view(np.float64)
        fin = np.isfinite(r)
        if not same_bits(g[~fin], r[~fin]):
            return False
        if fin.any() and not np.abs(g[fin] - r[fin]).max() <= 1e-12 * np.abs(r[fin]).max():
            return False
    return True


def _llr_ok(got, ref, exact):
    if exact:
        return same_bits(got, ref)
    fin = np.isfinite(ref)
    return same_bits(got[~fin], ref[~fin]) and bool(_llr_close(got[fin], ref[fin]).all())


def _variance_ok(got, ref, exact):
    if exact:
        return same_bits(got, ref)
    fin = np.isfinite(ref)
    return same_bits(got[~fin], ref[~fin]) and bool((np.abs(got[fin] - ref[fin]) <= 1e-12 * np.abs(ref[fin])).all())


def _repack_rows(orc, dei):
    return np.stack([S.repack(row, orc.nReal, orc.nVirtual, orc.P) for row in dei])


def _hard_bits(orc, dei):
    """a frame's own bits for the integer tail: the signs of its de-interleaved LLRs"""
    return (dei[:, : orc.nReal] < 0).astype(np.uint8)


def _chain(st, orc, bb, agc, vs):
    """telecom_system.cc:1132-1345 one method at a time, every intermediate kept -> {stage: [F, ...]}"""
    o = {}
    o["raw"] = st.frame_grid(bb)
    o["agc"] = st.agc(o["raw"])                       # these two run whatever the mode: the row-independence test wants every entry point
    o["grid"] = o["agc"] if agc else o["raw"]
    o["H_est"] = st.estimator(o["grid"])
    o["restored"] = st.restore(o["H_est"])
    o["H"] = o["restored"] if orc.amp_restore else o["H_est"]
    o["eq"] = st.equalizer(o["grid"], o["H"])
    o["variance"] = st.variance(o["eq"] if vs else o["grid"])
    o["deframed"] = st.deframer(o["eq"])
    o["syms"] = st.deint_c128(o["deframed"], orc.tf_blk)
    o["llr_demod"] = st.psk_demod(o["syms"], o["variance"].astype(np.float32))
    o["dei"] = st.deint_f32(o["llr_demod"], orc.bit_blk)
    o["llr_ldpc"] = _repack_rows(orc, o["dei"])
    o["descrambled"] = st.dispersal(_hard_bits(orc, o["dei"]))
    o["bytes"] = st.bit_to_byte(o["descrambled"])
    o["crc"] = st.crc16(o["bytes"][:, : orc.nReal // 8])
    return o


# ---- a: every stage against the CPU oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_each_stage_equals_the_oracle_on_the_oracles_own_input(mode):
    cfg, explicit, _ = MODES[mode]
    orc, bb65 = _case(mode)
    exact = _exact(orc)
    rx = _rx(cfg, max_batch=1, explicit=explicit)
    st = Stages(rx)
    assert (rx.nData, rx.nBits, rx.tf_blk, rx.bit_blk, rx.amp_restore, rx.ls_window) == (orc.nData, orc.nBits, orc.tf_blk, orc.bit_blk, orc.amp_restore, orc.ls_window)
    raw65, agc65 = _refs(mode, 0)["grid"], _refs(mode, FLAGS_RECEIVE_BYTE)["grid"]
    with np.errstate(all="ignore"):
        for F, idx in BATCH.items():
            bb = bb65[idx]
            assert same_bits(st.frame_grid(bb), raw65[idx]), (mode, F, "symbol_demod")
            assert same_bits(st.agc(raw65[idx]), agc65[idx]), (mode, F, "agc")
            for _, _, flags in _variants(cfg):
                ref = {k: v[idx] for k, v in _refs(mode, flags).items()}
                where = (mode, F, flags)
                assert same_bits(ref["grid"], (agc65 if flags & FLAG_AGC else raw65)[idx])
                est = ref["H_noamp"] if orc.amp_restore else ref["H"]
                assert _complex_ok(st.estimator(ref["grid"]), est, exact), (where, "estimator")
                if orc.amp_restore:
                    assert _complex_ok(st.restore(est), ref["H"], exact), (where, "restore")
                assert _complex_ok(st.equalizer(ref["grid"], ref["H"]), ref["eq"], exact), (where, "equalizer")
                got_var = st.variance(ref["eq"] if flags & FLAG_VAR_EQ else ref["grid"])
                assert _variance_ok(got_var, ref["variance"], exact), (where, "variance", got_var, ref["variance"])
                assert _complex_ok(st.deint_c128(st.deframer(ref["eq"]), orc.tf_blk), ref["syms"], exact), (where, "deframer + deinterleaver")
                assert _llr_ok(st.psk_demod(ref["syms"], ref["variance_f"]), ref["llr_demod"], exact), (where, "psk_demod")
                llr_ldpc = _repack_rows(orc, st.deint_f32(ref["llr_demod"], orc.bit_blk))
                assert _llr_ok(llr_ldpc[:, : orc.N], ref["llr_ldpc"][:, : orc.N], exact), (where, "deinterleaver_f32")
        # the integer tail on what the oracle's decoder made of five of the frames (the three degenerate ones among them)
        flags = _variants(cfg)[0][2]
        full = [orc.rx(bb65[f], flags) for f in (0, CLEAN, ZERO, NAN, 64)]
    bits = np.stack([r["bits"][: orc.nReal] for r in full]).astype(np.uint8)
    got = st.bit_to_byte(st.dispersal(bits))
    assert np.array_equal(got, np.stack([r["bytes"] for r in full]).astype(np.uint8)), mode
    crc = st.crc16(got[:, : orc.nReal // 8])
    for r, c in zip(full, crc):
        assert int(c) == orc.crc16(r["bytes"][: orc.nReal // 8]) and (r["all_zeros"] or int(c) == r["crc"]), mode
    assert full[1]["crc"] == 0 and not full[1]["all_zeros"]         # the noiseless frame decodes: its CRC is a real one
    rx.close()


# ---- b: the header's promise -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_the_chained_stages_equal_the_taps_of_the_fused_span(mode):
    cfg, explicit, _ = MODES[mode]
    orc, bb65 = _case(mode)
    for agc, vs, _ in _variants(cfg):
        rx = _rx(cfg, max_iters=50, agc=agc, variance_source=vs, max_batch=65, explicit=explicit)
        st = Stages(rx)
        for F, idx in BATCH.items():
            bb = bb65[idx]
            with np.errstate(all="ignore"):
                taps, mine = rx.receive(bb, taps=True), _chain(st, orc, bb, agc, vs)
            for key in ("grid", "H", "eq", "syms", "variance", "llr_demod", "llr_ldpc"):
                assert same_bits(mine[key], taps[key]), (mode, agc, vs, F, key)
            assert same_bits(mine["variance"].astype(np.float32), taps["stats"]["variance"].astype(np.float32)), (mode, agc, vs, F)
            if F == 3:
                assert np.isnan(mine["grid"][0]).any() and np.isfinite(mine["grid"][1]).all() and np.isfinite(mine["syms"][1]).all()
        rx.close()


# ---- c: batch independence -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_row_f_of_a_65_frame_call_is_the_one_frame_call_on_frame_f(mode):
    cfg, explicit, _ = MODES[mode]
    orc, bb65 = _case(mode)
    agc, vs, _ = _variants(cfg)[0]
    rx = _rx(cfg, max_batch=1, explicit=explicit)
    st = Stages(rx)
    with np.errstate(all="ignore"):
        full = _chain(st, orc, bb65, agc, vs)
        for f in (0, 1, 63, 64):
            one = _chain(st, orc, bb65[f:f + 1], agc, vs)
            assert sorted(one) == sorted(full)
            for key in full:
                assert full[key].shape[0] == 65 and one[key].shape[0] == 1
                assert full[key][f].tobytes() == one[key][0].tobytes(), (mode, f, key)
    assert len({full["bytes"][f].tobytes() for f in (0, 1, 63, 64)}) == 4           # four different frames
    rx.close()


# ---- d: shapes of the free functions ---------------------------------------------------------------------------------------------------
def test_symbol_demod_at_symbol_counts_around_its_four_per_workgroup():
    orc = Oracle(8, 50)
    rx, mfsk = _rx(8, max_batch=1), _rx(MFSK, max_batch=1)
    assert (mfsk.Nofdm, mfsk.Nc) == (rx.Nofdm, rx.Nc) == (272, 50) and mfsk.mfsk_M
    n_max = 4 * orc.Nsymb + 1
    frames = -(-n_max // orc.Nsymb)
    rng = np.random.default_rng(41)
    x = rng.standard_normal((frames * orc.Nsymb, orc.Nofdm)) + 1j * rng.standard_normal((frames * orc.Nsymb, orc.Nofdm))
    want = np.stack([orc.rx(b, FLAG_NO_LDPC)["grid"] for b in x.reshape(frames, -1)]).reshape(-1, orc.Nc)
    for n in (1, 3, 4, 5, n_max):
        got = Stages(rx).symbol_demod(x[:n])
        assert got.shape == (n, orc.Nc) and same_bits(got, want[:n]), n
        assert Stages(mfsk).symbol_demod(x[:n]).tobytes() == got.tobytes(), n
    rx.close(), mfsk.close()


def _shapes(rx):
    return [(1, 1), (7, 7), (7, 1), (10, 3), (257, 16), (rx.nData, rx.tf_blk), (rx.nBits, rx.bit_blk)]


@pytest.mark.parametrize("cfg", [8, 11])
def test_the_deinterleavers_move_every_item_once_whatever_the_tail(cfg):
    """(7, 1) and (7, 7): one block or blocks of one; (10, 3), (257, 16), mode 11's (533, 53) and (1599, 159): a tail that stays where it is."""
    rx = _rx(cfg, max_batch=1)
    st = Stages(rx)
    rng = np.random.default_rng(cfg)
    for n, bs in _shapes(rx):
        z = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
        assert st.deint_c128(z, bs).tobytes() == S.deinterleave(z, bs).tobytes(), (n, bs)
        # float items that no arithmetic would keep: quiet and signalling NaNs with a payload each, +-0, +-Inf, denormals
        w = (np.arange(3 * n, dtype=np.uint32) * np.uint32(2654435761) & np.uint32(0x003FFFFF)) | np.uint32(0x7F800001)
        w[rng.random(3 * n) < 0.5] |= np.uint32(0x80000000)
        w[1::5] = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001], np.uint32)[np.arange(w[1::5].size) % 5]
        w = w.reshape(3, n)
        got = st.deint_f32(w.view(np.float32), bs).view(np.uint32)
        assert np.array_equal(got, S.deinterleave(w, bs)), (n, bs)
        assert n < 3 or len({r.tobytes() for r in got}) == 3
    rx.close()


@pytest.mark.parametrize("cfg", [8, 11])
def test_the_integer_tail_at_lengths_that_are_no_multiple_of_eight_or_of_the_workgroup(cfg):
    orc = Oracle(cfg, 50)
    rx = _rx(cfg, max_batch=1)
    st = Stages(rx)
    rng = np.random.default_rng(50 + cfg)
    scr = orc.scrambler()
    for nbits in (1, 7, 8, 9, 255, 257, orc.nReal):
        bits = rng.integers(0, 2, (3, nbits), dtype=np.uint8)
        got = st.bit_to_byte(bits)
        assert got.shape == (3, (nbits + 7) // 8) and np.array_equal(got, S.bit_to_byte(bits)), nbits
    for n in (1, 255, 257, orc.N):
        bits = rng.integers(0, 2, (3, n), dtype=np.uint8)
        assert np.array_equal(st.dispersal(bits), S.dispersal(bits, scr)), n
    for F in (3, 65):
        for n in (0, 1, 2, 255, orc.nReal // 8):
            data = rng.integers(0, 256, (F, n), dtype=np.uint8)
            got = st.crc16(data)
            assert got.shape == (F,) and np.array_equal(got, S.crc16(data)), (F, n)
            assert n or (got == 0xFFFF).all()
    check = np.tile(np.frombuffer(b"123456789", np.uint8), (65, 1))
    assert (st.crc16(check) == 0x4B37).all()
    # 65 rows through the other two as well: one workgroup per row, rows of odd length
    bits = rng.integers(0, 2, (65, 257), dtype=np.uint8)
    assert np.array_equal(st.bit_to_byte(bits), S.bit_to_byte(bits)) and np.array_equal(st.dispersal(bits), S.dispersal(bits, scr))
    rx.close()


# ---- e: psk_demod at its edges ---------------------------------------------------------------------------------------------------------
VARIANCES = np.array([1.0, 0.0, -1.0, np.inf, np.nan, 1e-40, 3e38], np.float32)       # 1e-40: subnormal; 1 / 3e38: a subnormal reciprocal


def _edge_symbols(const, n, rng):
    """-> [rows, n]: the constellation, every midpoint of two of its points (exact ties), 0 / +-Inf / NaN in either part, symbols at 1.8e19
    and 1.85e19 (squared distances on either side of FLT_MAX: some overflow as floats, some do not), padded with noise around the points"""
    mids = [(const[a] + const[b]) / 2 for a in range(const.size) for b in range(a + 1, const.size)]
    parts = (0.0, np.inf, -np.inf, np.nan, 0.3)
    special = [complex(re, im) for re in parts for im in parts]
    big = [complex(m * re, m * im) for m in (1.8e19, 1.85e19) for re in (1, 0, -1) for im in (1, 0, -1) if re or im]
    pool = np.array(list(const) + mids + special + big, np.complex128)
    rows = -(-pool.size // n)
    pad = rows * n - pool.size
    noise = const[rng.integers(0, const.size, pad)] + 0.3 * (rng.standard_normal(pad) + 1j * rng.standard_normal(pad))
    return np.concatenate([pool, noise]).reshape(rows, n)


@pytest.mark.parametrize("cfg", [0, 8, 11, 13, 16])
def test_psk_demod_on_ties_infinities_and_degenerate_variances_is_the_float_model(cfg):
    """cl_psk::demod starts its minima at D[0] / D[mask], the kernel at +Inf: the same on every input, NaN and overflowing distances
    included (a NaN symbol makes every distance NaN, and an infinite minimum is never beaten by a strict `<`). The kernel keeps float
    denormals (no flush flag in mercury_amd/build.py, correctly rounded division): the subnormal variance and reciprocal rows are exact too."""
    orc = Oracle(cfg, 50)
    const = orc.constellation()
    rx = _rx(cfg, max_batch=1)
    sym = _edge_symbols(const, orc.nData, np.random.default_rng(cfg))
    syms = np.tile(sym, (VARIANCES.size, 1))                        # frame v * rows + r: symbols r, variance v
    var = np.repeat(VARIANCES, sym.shape[0])
    with np.errstate(all="ignore"):
        want = S.psk_demod(syms, var, const)
        got = Stages(rx).psk_demod(syms, var)
        sub = want[np.flatnonzero(var == VARIANCES[6])]
        assert ((sub != 0) & (np.abs(sub) < np.finfo(np.float32).tiny)).any()          # subnormal LLRs are among the expected values
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any() and (want == 0).any()
    bad = np.flatnonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).ravel())
    assert same_bits(got, want), (cfg, bad.size, bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])
    rx.close()


# ---- f: refusals -----------------------------------------------------------------------------------------------------------------------
def _valid_args(rx, F=2, n=10, bs=3):
    """{entry point: (arguments of a call that succeeds, the positions of its pointers, of its frame count, of n and of the block size)}"""
    G = rx.Nsymb * rx.Nc
    c = lambda *shape: np.zeros(shape, np.complex128) + 1          # noqa: E731
    u = lambda *shape: np.zeros(shape, np.uint8)                   # noqa: E731
    return {
        "mgpu_symbol_demod": ([c(F, rx.Nofdm), F, c(F, rx.Nc)], (0, 2), 1, None, None),
        "mgpu_automatic_gain_control": ([c(F, G), F], (0,), 1, None, None),
        "mgpu_channel_estimator": ([c(F, G), F, c(F, G)], (0, 2), 1, None, None),
        "mgpu_restore_channel_amplitude": ([c(F, G), F], (0,), 1, None, None),
        "mgpu_channel_equalizer": ([c(F, G), c(F, G), F, c(F, G)], (0, 1, 3), 2, None, None),
        "mgpu_measure_variance": ([c(F, G), F, np.zeros(F)], (0, 2), 1, None, None),
        "mgpu_deframer": ([c(F, G), F, c(F, rx.nData)], (0, 2), 1, None, None),
        "mgpu_deinterleaver_c128": ([c(F, n), F, n, bs, c(F, n)], (0, 4), 1, 2, 3),
        "mgpu_deinterleaver_f32": ([np.zeros((F, n), np.float32), F, n, bs, np.zeros((F, n), np.float32)], (0, 4), 1, 2, 3),
        "mgpu_psk_demod": ([c(F, rx.nData), F, np.ones(F, np.float32), np.zeros((F, rx.nBits), np.float32)], (0, 2, 3), 1, None, None),
        "mgpu_bit_energy_dispersal": ([u(F, n), F, n, u(F, n)], (0, 3), 1, 2, None),
        "mgpu_bit_to_byte": ([u(F, n), F, n, u(F, (n + 7) // 8)], (0, 3), 1, 2, None),
        "mgpu_crc16_modbus_rtu": ([u(F, n), F, n, np.zeros(F, np.uint16)], (0, 3), 1, 2, None),
    }


def _still_works(rx):
    st = Stages(rx)
    assert int(st.crc16(np.frombuffer(b"123456789", np.uint8)[None, :])[0]) == 0x4B37
    x = np.arange(20, dtype=np.float32).reshape(2, 10)
    assert np.array_equal(st.deint_f32(x, 3), S.deinterleave(x, 3))


def _refused(rx, name, args, what):
    rc = S.call(rx, name, *args)
    assert rc == S.MGPU_ERR_ARG and S.last_error(rx), (name, what, rc, S.last_error(rx))
    _still_works(rx)


def test_bad_arguments_are_refused_and_the_context_goes_on_working():
    rx = _rx(8, max_batch=1)
    calls = _valid_args(rx)
    assert sorted(calls) == sorted(S.SIGNATURES)
    for name, (args, pointers, f_at, n_at, bs_at) in calls.items():
        assert S.call(rx, name, *args) == S.MGPU_OK, (name, S.last_error(rx))
        for p in pointers:
            _refused(rx, name, args[:p] + [None] + args[p + 1:], "null pointer %d" % p)
        for F in (0, -1):
            _refused(rx, name, args[:f_at] + [F] + args[f_at + 1:], "F = %d" % F)
        if n_at is not None:
            _refused(rx, name, args[:n_at] + [-1] + args[n_at + 1:], "n = -1")
            if name != "mgpu_crc16_modbus_rtu":             # the CRC of no bytes is a value
                _refused(rx, name, args[:n_at] + [0] + args[n_at + 1:], "n = 0")
        if bs_at is not None:
            for bs in (0, -1, args[n_at] + 1):
                _refused(rx, name, args[:bs_at] + [bs] + args[bs_at + 1:], "bs = %d" % bs)
        assert S.call(rx, name, *args) == S.MGPU_OK, (name, S.last_error(rx))
        bound = getattr(rx.lib, name)
        assert bound(None, *[S.ptr(a) if isinstance(a, np.ndarray) else a for a in args]) == S.MGPU_ERR_ARG, name      # no context at all
    n = rx.N + 1
    _refused(rx, "mgpu_bit_energy_dispersal", [np.zeros((2, n), np.uint8), 2, n, np.zeros((2, n), np.uint8)], "n = N + 1")
    assert S.call(rx, "mgpu_bit_energy_dispersal", np.zeros((2, rx.N), np.uint8), 2, rx.N, np.zeros((2, rx.N), np.uint8)) == S.MGPU_OK
    rx.close()


def test_the_ofdm_stages_refuse_an_mfsk_context():
    rx = _rx(MFSK, max_batch=1)
    assert rx.mfsk_M
    import types
    ofdm = _rx(0, max_batch=1)
    # buffers as large as either geometry wants them: nothing a stage could read is out of bounds
    big = _valid_args(types.SimpleNamespace(Nofdm=rx.Nofdm, Nc=rx.Nc, **{k: max(getattr(rx, k), getattr(ofdm, k)) for k in ("Nsymb", "nData", "nBits")}))
    ofdm.close()
    for name in S.OFDM_ONLY:
        _refused(rx, name, big[name][0], "MFSK context")
        assert "OFDM" in S.last_error(rx), name
    for name in sorted(set(S.SIGNATURES) - set(S.OFDM_ONLY)):       # the geometry-free ones serve any context
        assert S.call(rx, name, *_valid_args(rx)[name][0]) == S.MGPU_OK, (name, S.last_error(rx))
    rx.close()

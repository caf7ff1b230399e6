"""What the tests of the front-end's opt-in forms on degenerate and edge-scale frames share (tests/test_frontend_degenerate_host.py on the
CPU, tests/test_gpu_frontend_degenerate.py on the device): the batch of degenerate baseband frames, built on the host by one fixed recipe so
that both see the same samples; the degenerate grids of the CPU test; the host twins chained as the kernel chains its stages; and the
comparison "bit for bit where the yardstick gives a number, NaN exactly where it gives NaN".

The forms are no reference configurations: their host twins are the normative statement (include/mercury_cfo.h, mercury_demapper.h,
mercury_estimator.h, mercury_wiener_bank.h), and the CPU test holds the twins to exact numpy restatements on these very inputs."""
import functools

import numpy as np

import wiener_bank_ref as WB
import wiener_ref as W
from demapper_csi_ref import DY5, llr_src, same_bits, tail  # noqa: F401  (shared with the tests)
from oraclelib import FLAGS_BASEBAND_TEST, FLAGS_RECEIVE_BYTE, Oracle, noise_amp_for

# Es/N0 (dB) of the good frame: every form decodes it (asserted by the tests on row "good")
ESN0 = {0: -6.0, 8: 3.0, 11: 9.0, 13: 12.0, 16: 24.0}
# The fp32-subnormal row's own Es/N0, by (mode, Dy). With the grid of the agc = 0 context scaled by the row's s the twin chain (own window,
# no carrier-offset stage, CSI) has a nonzero subnormal float32(sigma2), a nonzero subnormal float32(|h|^2) at every data cell and LLRs that
# are all finite and nonzero - subnormal_row asserts it. Such an s exists only where max |h|^2 / sigma2 stays below about 4
# (1 / float32(sigma2) overflows below 2.94e-39, a float32 is normal from 1.18e-38), so the 8PSK and QAM modes take a lower Es/N0 for this
# row than for the good frame. The zero-forcing mode 16 has no such scale: its estimate passes through its own pilots, sigma2 is rounding
# noise (1e-33 of |h|^2) and is zero as a float long before |h|^2 is subnormal - the row is left out there.
SUBNORMAL_ESN0 = {(0, 3): -6.0, (8, 3): 3.0, (11, 3): 3.0, (13, 3): 3.0, (8, 5): 3.0}
F32_TINY = 1.1754943508222875e-38           # the smallest normal float32

FE_THREADS = "MERCURY_FE_THREADS"     # read by mgpu_create with getenv: per context


def key_of(explicit):
    return tuple(sorted((explicit or {}).items()))


@functools.lru_cache(maxsize=None)
def oracle(cfg, key=()):
    return Oracle(cfg, 50, explicit=dict(key))


def good_frame(cfg, explicit=None, esn0=None):
    orc = oracle(cfg, key_of(explicit))
    return orc.gen_frame(5, 1, noise_amp_for(ESN0[cfg] if esn0 is None else esn0))


def _own_window_estimate(cfg, explicit, orc, grid):
    """the estimate at the pilots of the context's own window: the 21 x 21 LS mean, or in the zero-forcing modes Y / (x + 0i), which
    __divdc3 reduces to two real divisions (frontend.hip)"""
    from mercury_amd import host_ls_estimate
    if orc.estimator:
        return host_ls_estimate(cfg, grid, 21, 21, explicit=explicit)
    pilots = np.flatnonzero(orc.frame_types() != 0)
    x = orc.pilot_seq().real
    g = np.asarray(grid, np.complex128).ravel()[pilots]
    Hp = np.zeros(g.size, np.complex128)
    with np.errstate(all="ignore"):
        Hp.real, Hp.imag = g.real / x, g.imag / x                          # per component: 1j * Inf would put a NaN into the real part
    return Hp


def chain(cfg, explicit, grid, demapper="csi", cfo=False, estimator="own", bank=None):
    """The host twins chained as the kernel chains its stages, on one frame grid after the AGC: mgpu_host_cfo_pilots if cfo ->
    mgpu_host_ls_estimate(w, h) (estimator "own": 21 x 21, or (w, h)) or mgpu_host_wiener_estimate (estimator "wiener"; with `bank` the
    design mgpu_host_wiener_select chooses) -> wiener_ref.interpolate_cols -> mgpu_host_demap_csi / _nmap (demapper "maxlog": none).
    -> dict(grid: the turned grid, step, Hp, H, choice (bank), llr_demod, llr_ldpc [N], sigma2, fc, fs - what applies)"""
    from mercury_amd import host_cfo_pilots, host_demap_csi, host_demap_nmap, host_ls_estimate, host_wiener_estimate, host_wiener_select
    orc = oracle(cfg, key_of(explicit))
    out = dict(step=None)
    grid = np.ascontiguousarray(grid, np.complex128).ravel()
    if cfo:
        grid, out["step"] = host_cfo_pilots(cfg, grid, explicit=explicit)
    out["grid"] = grid
    if estimator == "wiener":
        design = None
        if bank:
            out["choice"] = host_wiener_select(cfg, grid, bank, explicit=explicit)
            design = bank[out["choice"]["design"]][0]
        Hp = host_wiener_estimate(cfg, grid, design, explicit=explicit)
    elif estimator == "own":
        Hp = _own_window_estimate(cfg, explicit, orc, grid)
    else:
        Hp = host_ls_estimate(cfg, grid, estimator[0], estimator[1], explicit=explicit)
    out["Hp"] = Hp
    out["H"] = H = W.interpolate_cols(orc, Hp)
    if demapper == "csi":
        out["llr_demod"], out["sigma2"] = host_demap_csi(cfg, grid, H, explicit=explicit)
    elif demapper == "nmap":
        out["llr_demod"], out["sigma2"], out["fc"], out["fs"] = host_demap_nmap(cfg, grid, H, explicit=explicit)
    if "llr_demod" in out:
        out["llr_ldpc"] = out["llr_demod"][llr_src(orc)]
    return out


# ---- the fp32-subnormal scale ------------------------------------------------------------------------------------------------------------------
def subnormal_conditions(cfg, explicit, grid):
    """the three conditions of the subnormal row on one (scaled) grid of the agc = 0 context, from the CSI twin chain with the context's own
    window -> (float32(sigma2) is a nonzero subnormal, float32(|h|^2) is one at every data cell, every LLR is finite and nonzero)"""
    orc = oracle(cfg, key_of(explicit))
    c = chain(cfg, explicit, grid, "csi")
    h = c["H"][np.flatnonzero(orc.frame_types() == 0)]
    with np.errstate(all="ignore"):
        wf = (h.real * h.real + h.imag * h.imag).astype(np.float32)
        s2 = np.float64(c["sigma2"]).astype(np.float32)
    sub = lambda v: bool(((v != 0) & (np.abs(v) < np.float32(F32_TINY))).all())      # noqa: E731
    return sub(s2), sub(wf), bool((np.isfinite(c["llr_demod"]) & (c["llr_demod"] != 0)).all())


@functools.lru_cache(maxsize=None)
def subnormal_row(cfg, key=()):
    """(the row's samples, its scale s, its Es/N0), or None where the mode has no such scale (the zero-forcing modes: see SUBNORMAL_ESN0).
    s puts the larger of sigma2 and the largest |h|^2 of the twin chain on the oracle's agc = 0 grid at 0.9 of the smallest normal float32,
    and the three conditions are asserted here, on the CPU twin, so that a drift of the fixture fails loudly instead of silently testing
    nothing."""
    explicit = dict(key) or None
    orc = oracle(cfg, key)
    dy = (explicit or {}).get("Dy", 3)
    if (cfg, dy) not in SUBNORMAL_ESN0:
        assert not orc.estimator, (cfg, dy)                                # only the zero-forcing modes go without
        return None
    esn0 = SUBNORMAL_ESN0[(cfg, dy)]
    frame, _ = good_frame(cfg, explicit, esn0)
    c = chain(cfg, explicit, orc.rx(frame, FLAGS_BASEBAND_TEST)["grid"], "csi")
    H = c["H"][np.flatnonzero(orc.frame_types() == 0)]
    s = float(np.sqrt(0.9 * F32_TINY / max(float(np.max(H.real * H.real + H.imag * H.imag)), c["sigma2"])))
    row = frame * s
    ok = subnormal_conditions(cfg, explicit, orc.rx(row, FLAGS_BASEBAND_TEST)["grid"])
    assert ok == (True, True, True), (cfg, explicit, esn0, s, ok)
    return row, s, esn0


# ---- the batch of degenerate baseband frames -------------------------------------------------------------------------------------------------------
ROWS = ("good", "zeros", "tiny", "big", "huge", "nan_mid", "inf_last", "nan_guard", "negated", "dc", "sym5_zero", "sym5_big")


@functools.lru_cache(maxsize=None)
def batch(cfg, key=(), subnormal=False):
    """-> dict(orc, bb [rows, samples], names, row: name -> index, payload: the good frame's). The rows, from one good frame
    gen_frame(5, 1, noise_amp_for(ESN0[cfg])):
      good       the frame itself: the control
      zeros      all zeros: AGC boost / 0, carrier-offset sums both zero, sigma2 0 or NaN
      tiny       x 1e-300: pilot products underflow to 0 while the pilots do not
      big        x 1e150: products finite, |h|^2 as a float +Inf
      huge       x 1e154: each pilot product finite, their sum not
      nan_mid    one NaN sample in the middle of symbol 3: one grid row without the AGC, everything with it
      inf_last   one Inf sample in the middle of the last symbol: the extrapolating end of the column interpolation
      nan_guard  one NaN sample inside the guard interval of symbol 0 (index 5 < Ngi): stripped, so the row equals "good" in every byte
      negated    the frame negated: steps and factors as "good"
      dc         constant 1 + 1j: all carriers exactly or nearly 0
      sym5_zero  symbol 5's samples zero: a symbol factor far above the band
      sym5_big   symbol 5's samples x 1e200: sigma2 Inf
      subnormal  (with subnormal=True, for the agc = 0 context only, where the mode has one) x s: subnormal_row"""
    explicit = dict(key) or None
    orc = oracle(cfg, key)
    good, payload = good_frame(cfg, explicit)
    n, No, Ngi, Nfft = orc.frame_samples, orc.Nofdm, orc.Ngi, orc.Nfft
    assert n == orc.Nsymb * No and Ngi > 5 and orc.Nsymb > 6
    mid = Ngi + Nfft // 2
    rows = dict(good=good, zeros=np.zeros(n, np.complex128), tiny=good * 1e-300, big=good * 1e150, huge=good * 1e154, nan_mid=good.copy(),
                inf_last=good.copy(), nan_guard=good.copy(), negated=-good, dc=np.full(n, 1 + 1j, np.complex128), sym5_zero=good.copy(),
                sym5_big=good.copy())
    rows["nan_mid"][3 * No + mid] = np.nan
    rows["inf_last"][(orc.Nsymb - 1) * No + mid] = np.inf
    rows["nan_guard"][5] = np.nan
    rows["sym5_zero"][5 * No: 6 * No] = 0
    rows["sym5_big"][5 * No: 6 * No] *= 1e200
    names = list(ROWS)
    if subnormal:
        made = subnormal_row(cfg, key)
        if made is not None:
            rows["subnormal"] = made[0]
            names.append("subnormal")
    return dict(orc=orc, bb=np.stack([rows[k] for k in names]), names=names, row={k: i for i, k in enumerate(names)}, payload=payload)


# ---- the degenerate grids of the CPU test ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grids(cfg, key=()):
    """-> (names, [grid]): the good frame's grid as the oracle's receive-byte variant gives it (after the AGC), and what the CPU test
    makes of it: all zeros; scaled by 1e-300, 1e-160, 1e150 and 1e154; scaled so that every float32(|h|^2) is subnormal (the largest
    |h|^2 of the own-window estimate at 0.9 of the smallest normal float32; sigma2 may be zero as a float there: that is the twin's
    business); one NaN pilot, one Inf pilot, one NaN data cell, one carrier's pilots zeroed."""
    explicit = dict(key) or None
    orc = oracle(cfg, key)
    g = orc.rx(good_frame(cfg, explicit)[0], FLAGS_RECEIVE_BYTE)["grid"]
    types = orc.frame_types()
    pilots, data = np.flatnonzero(types != 0), np.flatnonzero(types == 0)
    H = chain(cfg, explicit, g, "maxlog")["H"][data]
    s = float(np.sqrt(0.9 * F32_TINY / float(np.max(H.real * H.real + H.imag * H.imag))))
    out = dict(ordinary=g, zeros=np.zeros_like(g), x1e_300=g * 1e-300, x1e_160=g * 1e-160, x1e150=g * 1e150, x1e154=g * 1e154, subnormal=g * s)
    for name, cell, value in (("nan_pilot", pilots[pilots.size // 2], np.nan), ("inf_pilot", pilots[pilots.size // 3], np.inf),
                              ("nan_data", data[data.size // 2], np.nan)):
        out[name] = g.copy()
        out[name][cell] = value
    out["carrier_zeroed"] = g.copy()
    out["carrier_zeroed"][pilots[pilots % orc.Nc == 7]] = 0
    return list(out), [out[k] for k in out]


# ---- the decode behind the LLRs ------------------------------------------------------------------------------------------------------------------------
_DECODED = {}


def decode(cfg, explicit, llr_ldpc):
    """the oracle's decoder and integer tail on llr_ldpc [N] -> (iterations, payload bytes, crc, all_zeros, message_decoded); kept by the
    LLRs' bytes, since many degenerate rows and forms give the same ones (all NaN, all zero)"""
    orc = oracle(cfg, key_of(explicit))
    k = (cfg, key_of(explicit), np.ascontiguousarray(llr_ldpc, np.float32).tobytes())
    if k not in _DECODED:
        bits, it = orc.ldpc_decode(llr_ldpc)
        _DECODED[k] = (it,) + tail(orc, bits)
    return _DECODED[k]


def check_decode(cfg, explicit, out, f, llr_ldpc, where=None):
    """payload, iteration count, CRC, all_zeros and message_decoded of row f of a receive call against the oracle's decoder and tail on
    llr_ldpc (tests/test_gpu_noise_map.py: _check_decode) -> message_decoded"""
    it, payload, crc, all_zeros, decoded = decode(cfg, explicit, llr_ldpc)
    st = out["stats"][f]
    assert (st["iterations_done"], st["message_decoded"], st["crc"], st["all_zeros"]) == (it, decoded, crc, all_zeros), (where, f, st, it, decoded, crc, all_zeros)
    assert np.array_equal(out["payload"][f][: payload.size], payload), (where, f)
    return decoded


def bank():
    return WB.bank()

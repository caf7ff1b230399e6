"""What the tests of the front-end's form table share (tests/test_frontend_forms_host.py on the CPU, tests/test_gpu_frontend_form_order.py
on the device): the form bits of csrc/ls_rect.h, two ordinary frames, and what a span must give for a set of options - the host twins
chained as the kernel chains its stages (frontend_degenerate_ref.chain) and, behind them, the part every form shares with the plain one,
restated in numpy: restore_channel_amplitude, the equaliser at the pilots, the two variances, the plain max-log demapper."""
import functools

import numpy as np

import frontend_degenerate_ref as D
from demapper_csi_ref import np_cdiv, np_maxlog, same_bits, sym_src  # noqa: F401  (same_bits: shared with the tests)
from oraclelib import FLAGS_RECEIVE_BYTE, noise_amp_for

RECT, CSI, CFO, WIENER, NMAP = 1, 2, 4, 8, 16                                          # MGPU_FE_* (csrc/ls_rect.h)
VALID_FORMS = [0] + [RECT | a | b | c for a in (0, CSI) for b in (0, CFO) for c in (0, WIENER)] + \
              [RECT | CSI | NMAP | b | c for b in (0, CFO) for c in (0, WIENER)]


@functools.lru_cache(maxsize=None)
def frames(cfg):
    """two frames of the generator at the Es/N0 every form decodes (frontend_degenerate_ref.ESN0) -> complex128 [2, samples]"""
    orc = D.oracle(cfg)
    return np.stack([orc.gen_frame(5, k, noise_amp_for(D.ESN0[cfg]))[0] for k in (1, 2)])


def unit_phasor(orc, h):
    """restore_channel_amplitude (ofdm.cc:1453-1466; get_angle / set_complex misc.cc:34-71) with the platform's atan and sincos"""
    with np.errstate(all="ignore"):
        a = orc.libm_atan_sincos(h.imag / h.real)[0]
    th = np.where(h.real == 0, np.pi / 2, np.where(h.real > 0, a, np.where(h.imag >= 0, a + np.pi, a - np.pi)))
    _, s, c = orc.libm_atan_sincos(th)
    out = np.zeros(h.size, np.complex128)
    out.real, out.imag = 1 * c, 1 * s
    return out


def plain_tail(orc, grid, H):
    """Behind the estimate H [G] (before amplitude restoration) on the grid [G], with agc = 1 and variance_source = 1 as the oracle's
    receive-byte variant: the variance of the equalised pilots after amplitude restoration (what scales the plain LLRs and is reported),
    the one before it (the SNR's; the same where the mode restores nothing), the plain demapper's LLRs. One IEEE operation after the
    other, the sums in pilot order (np.cumsum). -> dict(variance (double), snr_variance, snr_db, llr_demod, llr_ldpc)"""
    grid, H = np.asarray(grid, np.complex128).ravel(), np.asarray(H, np.complex128).ravel()
    pilots = np.flatnonzero(orc.frame_types() != 0)
    x = orc.pilot_seq().real
    g, h = grid[pilots], H[pilots]

    def variance_of(er, ei):
        dr, di = er - x, ei - 0.0
        return float(np.cumsum(dr * dr + di * di)[-1] / float(orc.nPilots))

    out = {}
    hu = unit_phasor(orc, h) if orc.amp_restore else h
    out["variance"] = variance_of(*np_cdiv(g, hu))
    out["snr_variance"] = variance_of(*np_cdiv(g, h)) if orc.amp_restore else out["variance"]
    var_f = np.float64(out["variance"]).astype(np.float32)
    sv_f = np.float64(out["snr_variance"]).astype(np.float32) if orc.amp_restore else var_f
    out["snr_db"] = float(np.float32(10.0 * np.log10(1.0 / np.float64(sv_f))))
    src = sym_src(orc)
    hs = unit_phasor(orc, H[src]) if orc.amp_restore else H[src]
    er, ei = np_cdiv(grid[src], hs)
    out["llr_demod"] = np_maxlog(orc, er, ei, np.float32(1.0) / var_f)
    out["llr_ldpc"] = out["llr_demod"][D.llr_src(orc)]
    return out


@functools.lru_cache(maxsize=None)
def expected(cfg, f, wiener, cfo, nmap):
    """frame f of frames(cfg) with the one-rung Wiener ladder, MGPU_CFO_PILOTS and MGPU_DEMAP_NMAP on or off: the oracle's grid through the
    chained twins, the plain tail behind their estimate -> the chain's dict with variance, snr_variance, snr_db added, and with the plain
    demapper's llr_demod / llr_ldpc where the noise map is off"""
    orc = D.oracle(cfg)
    grid = orc.rx(frames(cfg)[f], FLAGS_RECEIVE_BYTE)["grid"]
    c = D.chain(cfg, None, grid, "nmap" if nmap else "maxlog", cfo, "wiener" if wiener else "own")
    t = plain_tail(orc, c["grid"], c["H"])
    for k in ("variance", "snr_variance", "snr_db"):
        c[k] = t[k]
    if not nmap:
        c["llr_demod"], c["llr_ldpc"] = t["llr_demod"], t["llr_ldpc"]
    return c

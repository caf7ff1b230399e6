"""CPU tests of the host twins of the front-end's opt-in forms on degenerate and edge-scale grids: the chain mgpu_host_cfo_pilots ->
mgpu_host_ls_estimate(21, 21) or mgpu_host_wiener_estimate -> column interpolation -> mgpu_host_demap_csi / mgpu_host_demap_nmap, with
mgpu_host_wiener_select beside it, held to exact numpy restatements bit for bit, NaN where NaN. The twins are the normative statement of
forms the reference does not have; tests/test_gpu_frontend_degenerate.py holds the kernels to them on the same kind of input, so what is
pinned here is the yardstick of that test.

One restatement is not exact: wiener_ref.np_estimate groups its sums as numpy's matrix product does, so it agrees with
mgpu_host_wiener_estimate only to rounding. For it the NaN and Inf positions are asserted, and its existing tolerance
(tests/test_wiener_host.py: 1e-12 max|Hp| with the library's own tables) on the numbers."""
import numpy as np
import pytest

import frontend_degenerate_ref as D
import wiener_bank_ref as WB
import wiener_ref as W
from demapper_csi_ref import CASES, np_demap_csi, same_bits
from noise_map_ref import LS_CASES, np_demap_nmap, np_noise_map
from residual_cfo_ref import np_cfo_pilots

# grids whose summed pilot products are zero (all zeros; 1e-300: every product underflows), not finite (1e154: each product is finite, their
# sum is not; an Inf pilot) or NaN (a NaN pilot): the carrier-offset twin must pass them through
CFO_PASSES = ("zeros", "x1e_300", "x1e154", "nan_pilot", "inf_pilot")


def _same_scalar(a, b):
    return same_bits(np.array([a], np.float64), np.array([b], np.float64))


def _library_tables(cfg, explicit):
    from mercury_amd import host_wiener_tables
    tc, fc = host_wiener_tables(cfg, None, explicit=explicit)
    return dict(time={tuple(m.tolist()): A for m, A in tc}, freq={tuple(m.tolist()): B for m, B in fc})


@pytest.mark.parametrize("cfg,explicit", CASES)
def test_chained_twins_equal_the_exact_restatements_on_degenerate_grids(cfg, explicit):
    from mercury_amd import host_cfo_pilots
    orc = D.oracle(cfg, D.key_of(explicit))
    ls = (cfg, explicit) in LS_CASES
    names, grids = D.grids(cfg, D.key_of(explicit))
    dy = (explicit or {}).get("Dy", 3)
    pilots = np.flatnonzero(orc.frame_types() != 0)
    tables = _library_tables(cfg, explicit) if ls else None
    bank = WB.bank()
    seen = dict(nan_llr=0, number_llr=0, unit_map=0, moved_map=0, passed=0, turned=0)
    for name, g0 in zip(names, grids):
        # ---- the carrier-offset twin: the turned grid and the step against np_cfo_pilots
        turned, step = host_cfo_pilots(cfg, g0, explicit=explicit)
        want_grid, want_step = np_cfo_pilots(orc, g0, dy)
        assert same_bits(turned, want_grid) and _same_scalar(step, want_step), (name, step, want_step)
        if name in CFO_PASSES:
            assert step == 0.0 and not np.signbit(step) and turned.tobytes() == g0.tobytes(), (name, step)
            seen["passed"] += 1
        elif step != 0.0:
            seen["turned"] += 1
        for cfo in (False, True):
            grid = turned if cfo else g0
            for estimator in (("own", "wiener") if ls else ("own",)):
                where = (cfg, explicit, name, cfo, estimator)
                c = D.chain(cfg, explicit, g0, "csi", cfo, estimator)
                assert c["grid"].tobytes() == grid.tobytes(), where
                H = c["H"]
                if estimator == "wiener":
                    # not exact (numpy's grouping of the sums): NaN and Inf where the twin has them, the numbers within 1e-12 max|Hp|
                    with np.errstate(all="ignore"):
                        want = W.np_estimate(orc, grid, tables)
                    got = c["Hp"]
                    for part in ("real", "imag"):
                        a, b = getattr(got, part), getattr(want, part)
                        assert np.array_equal(np.isnan(a), np.isnan(b)), where
                        assert np.array_equal(np.isinf(a), np.isinf(b)) and np.array_equal(a[np.isinf(a)], b[np.isinf(b)]), where
                    fin = np.isfinite(got.real) & np.isfinite(got.imag) & np.isfinite(want.real) & np.isfinite(want.imag)
                    if fin.any():
                        assert np.abs(got[fin] - want[fin]).max() <= 1e-12 * np.abs(want[fin]).max(), where
                    # ... and the bank's choice beside it: np_select's, the fallback whenever a sounded pilot is NaN
                    sel = D.chain(cfg, explicit, g0, "maxlog", cfo, "wiener", bank=bank)["choice"]
                    with np.errstate(all="ignore"):
                        want_sel = WB.np_select(orc, grid, bank)
                    assert sel["design"] == want_sel["design"] and same_bits(sel["corr"], want_sel["corr"]), (where, sel, want_sel)
                    if np.isnan(grid[pilots].real).any() or np.isnan(grid[pilots].imag).any():
                        assert sel["design"] == len(bank) - 1, (where, sel)
                # ---- the channel-aware twin: LLRs and sigma2
                want_llr, want_sigma2 = np_demap_csi(orc, grid, H)
                assert same_bits(c["llr_demod"], want_llr) and _same_scalar(c["sigma2"], want_sigma2), (where, c["sigma2"], want_sigma2)
                seen["nan_llr"] += int(np.isnan(want_llr).any())
                seen["number_llr"] += int(not np.isnan(want_llr).all())
                if not ls:
                    continue
                # ---- the noise-map twin: LLRs, sigma2 and the factors
                m = D.chain(cfg, explicit, g0, "nmap", cfo, estimator)
                want_llr, want_sigma2, want_fc, want_fs = np_demap_nmap(orc, grid, H)
                assert same_bits(m["llr_demod"], want_llr) and _same_scalar(m["sigma2"], want_sigma2), where
                assert _same_scalar(m["sigma2"], c["sigma2"]), where
                assert m["fc"].tobytes() == want_fc.tobytes() and m["fs"].tobytes() == want_fs.tobytes(), where
                assert not np.isnan(m["fc"]).any() and not np.isnan(m["fs"]).any(), where
                if m["sigma2"] == 0 or not np.isfinite(m["sigma2"]):
                    assert (m["fc"] == 1.0).all() and (m["fs"] == 1.0).all(), (where, m["sigma2"])
                    seen["unit_map"] += 1
                elif (m["fc"] != 1.0).any() or (m["fs"] != 1.0).any():
                    seen["moved_map"] += 1
                assert np_noise_map(orc, grid, H)[0] == want_sigma2 or np.isnan(want_sigma2)
    print("mode %d %s:" % (cfg, explicit), seen)
    # the cases are there: LLRs that are NaN and LLRs that are numbers, grids that pass the carrier-offset stage and grids it turns, and in
    # the LS modes maps that are all ones because sigma2 is unusable and maps with a factor outside the band
    assert seen["nan_llr"] > 0 and seen["number_llr"] > 0 and seen["passed"] == len(CFO_PASSES) and seen["turned"] >= 3, seen
    if ls:
        assert seen["unit_map"] > 0 and seen["moved_map"] > 0, seen


@pytest.mark.parametrize("cfg,explicit", CASES)
def test_the_degenerate_batch_is_what_its_recipe_says(cfg, explicit):
    """the baseband rows the GPU test runs: their places in the batch, the subnormal row's three conditions (asserted by the helper), and the
    guard-interval row, whose NaN the oracle never sees"""
    orc = D.oracle(cfg, D.key_of(explicit))
    b = D.batch(cfg, D.key_of(explicit), subnormal=True)
    assert b["names"][: len(D.ROWS)] == list(D.ROWS) and b["bb"].shape == (len(b["names"]), orc.frame_samples)
    made = D.subnormal_row(cfg, D.key_of(explicit))
    assert (made is None) == (not orc.estimator) and ("subnormal" in b["row"]) == (made is not None)
    if made is not None:
        assert 1e-20 < made[1] < 2e-19, made[1:]
    good, guard = orc.rx(b["bb"][b["row"]["good"]]), orc.rx(b["bb"][b["row"]["nan_guard"]])
    assert np.isnan(b["bb"][b["row"]["nan_guard"]]).sum() == 1
    for key in ("grid", "llr_ldpc", "bytes"):
        assert good[key].tobytes() == guard[key].tobytes(), key
    assert good["crc"] == 0 and not good["all_zeros"] and np.array_equal(good["bytes"][: orc.payload_bytes], b["payload"])

"""GPU tests of the front-end's opt-in forms - the channel-aware (CSI) and noise-map (NMAP) demappers, the pilot carrier-offset stage (CFO),
the Wiener rung and its bank - on degenerate and edge-scale frames, in all thirteen kernels at both workgroup sizes.

The forms are no reference configurations; their host twins are the normative statement, and tests/test_frontend_degenerate_host.py holds
those to exact numpy restatements on such inputs. Yardstick here, as test_kernel_combinations_equal_twins_chained_on_the_host of
tests/test_gpu_noise_map.py: the PLAIN context's grid tap (which test_degenerate_inputs_behave_like_the_reference holds to the oracle)
through the twins chained on the host (frontend_degenerate_ref.chain), row by row. Everything is compared bit for bit where the chain gives
a number - the signs of zeros and infinities included - and as NaN positions where it gives NaN: x86 and CDNA differ in the sign bit of
a generated NaN. The batch is frontend_degenerate_ref.batch: the good frame and eleven degenerate ones, plus the fp32-subnormal row on the
agc = 0 context."""
import numpy as np
import pytest

import frontend_degenerate_ref as D
from frontend_degenerate_ref import DY5, FE_THREADS, check_decode, same_bits

pytestmark = pytest.mark.gpu

UNSUPPORTED = 4                                                           # MGPU_ERR_UNSUPPORTED
CONTEXTS = [dict(agc=1, variance_source=1), dict(agc=0, variance_source=0)]      # the receive-byte variant; scale and a single NaN survive into the grid
DEMAPPERS, ESTIMATORS = ("maxlog", "csi", "nmap"), ("own", (5, 5), "wiener")
ALL_FORMS = [(d, cfo, e) for d in DEMAPPERS for cfo in (False, True) for e in ESTIMATORS]           # together: all thirteen kernels
SOME_FORMS = [("csi", True, "own"), ("nmap", True, "wiener")]
ZF_FORMS = [("csi", False, "own"), ("csi", True, "own")]
STEP_IS_ZERO = ("zeros", "huge", "nan_mid", "dc")                        # rows whose carrier-offset sums are zero, not finite or NaN on either context


def _context(cfg, explicit, threads, ctx, monkeypatch, max_batch):
    from mercury_amd import RxPhy
    monkeypatch.setenv(FE_THREADS, str(threads))
    rx = RxPhy(cfg, max_batch=max_batch, explicit=explicit, **ctx)
    monkeypatch.delenv(FE_THREADS)
    return rx


def _set_form(rx, demapper, cfo, estimator, bank=None):
    """-> False where the library refuses the combination with MGPU_ERR_UNSUPPORTED (the context is then as it was)"""
    from mercury_amd import MgpuError
    try:
        rx.set_estimator_ladder([] if estimator == "own" else [("wiener", {})] if estimator == "wiener" else [estimator])
        if bank:
            rx.set_wiener_bank(0, bank)
        rx.set_demapper(demapper)
        rx.set_cfo("pilots" if cfo else "off")
    except MgpuError as e:
        assert e.code == UNSUPPORTED, str(e)
        return False
    return True


def _scalar_same(a, b):
    return same_bits(np.array([a], np.float64), np.array([b], np.float64))


def _reports(rx, form, F, bank=None):
    """what the context reports beside the call's outputs: the steps, the map's rows, the bank's choice"""
    demapper, cfo, _ = form
    return dict(steps=rx.cfo_steps(F) if cfo else None, maps=rx.noise_map(0, F) if demapper == "nmap" else None,
                choice=rx.wiener_choice(0, F) if bank else None)


def _check_row(cfg, explicit, form, plain, out, rep, f, name, bank=None):
    """row f of a taps call and of the context's reports against the chain on the plain grid tap -> the chain"""
    orc = D.oracle(cfg, D.key_of(explicit))
    demapper, cfo, estimator = form
    where = (cfg, explicit, form, name)
    c = D.chain(cfg, explicit, plain["grid"][f], demapper, cfo, estimator, bank)
    assert same_bits(out["grid"][f], c["grid"]), where
    if cfo:
        assert _scalar_same(rep["steps"][f], c["step"]), (where, rep["steps"][f], c["step"])
        if name in STEP_IS_ZERO:
            assert c["step"] == 0.0, (where, c["step"])
        if c["step"] == 0.0:                                              # the grid passes through byte for byte
            assert rep["steps"][f] == 0.0 and not np.signbit(rep["steps"][f]) and out["grid"][f].tobytes() == plain["grid"][f].tobytes(), where
    if bank:
        ch = rep["choice"]
        assert ch["design"][f] == c["choice"]["design"] and same_bits(ch["corr"][f], c["choice"]["corr"]), (where, ch["design"][f], c["choice"])
        pilots = out["grid"][f][np.flatnonzero(orc.frame_types() != 0)]
        if np.isnan(pilots.real).any() or np.isnan(pilots.imag).any():
            assert ch["design"][f] == len(bank) - 1, where                # a NaN sounding takes the fallback
    if demapper != "maxlog" or not orc.amp_restore:                      # (the plain forms of the PSK modes show the restored unit phasor)
        assert same_bits(out["H"][f], c["H"]), where
    if demapper == "maxlog":
        return c
    assert same_bits(out["llr_demod"][f], c["llr_demod"]), (where, c["sigma2"])
    assert same_bits(out["llr_ldpc"][f][: orc.N], c["llr_ldpc"]), where
    check_decode(cfg, explicit, out, f, c["llr_ldpc"], where)
    if demapper == "nmap":
        fc, fs = rep["maps"][0][f], rep["maps"][1][f]
        assert fc.tobytes() == c["fc"].tobytes() and fs.tobytes() == c["fs"].tobytes(), where
        assert not np.isnan(fc).any() and not np.isnan(fs).any(), where
        if c["sigma2"] == 0 or not np.isfinite(c["sigma2"]):
            assert (fc == 1.0).all() and (fs == 1.0).all(), (where, c["sigma2"])
    return c


def _check_guard_row(b, out, rep, where):
    """the NaN in the guard interval is stripped: the row equals the good frame's in every output byte, taps and reports included"""
    a, h = b["row"]["good"], b["row"]["nan_guard"]
    for key, v in out.items():
        if key != "cycles":
            assert v[h].tobytes() == v[a].tobytes(), (where, key)
    if rep["steps"] is not None:
        assert rep["steps"][h].tobytes() == rep["steps"][a].tobytes(), where
    if rep["maps"] is not None:
        assert rep["maps"][0][h].tobytes() == rep["maps"][0][a].tobytes() and rep["maps"][1][h].tobytes() == rep["maps"][1][a].tobytes(), where
    if rep["choice"] is not None:
        assert rep["choice"]["design"][h] == rep["choice"]["design"][a] and rep["choice"]["corr"][h].tobytes() == rep["choice"]["corr"][a].tobytes(), where


def _run_forms(cfg, explicit, threads, ctx, forms, monkeypatch, bank=None):
    from mercury_amd import MgpuError, host_demap_nmap
    orc = D.oracle(cfg, D.key_of(explicit))
    b = D.batch(cfg, D.key_of(explicit), subnormal=ctx["agc"] == 0)
    bb, F = b["bb"], len(b["names"])
    rx = _context(cfg, explicit, threads, ctx, monkeypatch, F)
    ran = 0
    with np.errstate(all="ignore"):
        plain = rx.receive(bb, taps=True)
        for form in forms:
            if not _set_form(rx, *form, bank=bank):
                if form[0] == "nmap" and form[2] == "own":               # the twin refuses what the library refuses
                    with pytest.raises(MgpuError) as e:
                        host_demap_nmap(cfg, plain["grid"][0], plain["grid"][0], explicit=explicit)
                    assert e.value.code == UNSUPPORTED
                assert not orc.estimator, form                            # only the zero-forcing modes are refused anything here
                continue
            ran += 1
            out = rx.receive(bb, taps=True)
            rep = _reports(rx, form, F, bank)
            where = (cfg, explicit, threads, ctx["agc"], form)
            for f, name in enumerate(b["names"]):
                _check_row(cfg, explicit, form, plain, out, rep, f, name, bank)
                if name == "good" and form[0] != "maxlog":               # the control decodes, to its own payload
                    assert out["stats"][f]["message_decoded"] == 1 and np.array_equal(out["payload"][f][: orc.payload_bytes], b["payload"]), where
                if name == "negated":                                    # every step and factor as the good frame's
                    a = b["row"]["good"]
                    assert not form[1] or rep["steps"][f].tobytes() == rep["steps"][a].tobytes(), where
                    assert form[0] != "nmap" or (rep["maps"][0][f].tobytes() == rep["maps"][0][a].tobytes() and
                                                 rep["maps"][1][f].tobytes() == rep["maps"][1][a].tobytes()), where
            _check_guard_row(b, out, rep, where)
    rx.close()
    return ran


# ---- 1. every kernel, both workgroup sizes, both contexts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx", CONTEXTS, ids=["agc", "noagc"])
@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("cfg,explicit", [(8, None), (0, None)])
def test_every_form_equals_the_chained_twins_on_the_degenerate_batch(cfg, explicit, threads, ctx, monkeypatch):
    assert _run_forms(cfg, explicit, threads, ctx, ALL_FORMS, monkeypatch) == len(ALL_FORMS)


@pytest.mark.parametrize("ctx", CONTEXTS, ids=["agc", "noagc"])
@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("cfg,explicit", [(13, None), (11, None), (8, DY5)])
def test_csi_cfo_and_nmap_cfo_wiener_in_the_qam_8psk_and_dy5_geometries(cfg, explicit, threads, ctx, monkeypatch):
    assert _run_forms(cfg, explicit, threads, ctx, SOME_FORMS, monkeypatch) == len(SOME_FORMS)


@pytest.mark.parametrize("ctx", CONTEXTS, ids=["agc", "noagc"])
@pytest.mark.parametrize("threads", [512, 1024])
def test_csi_forms_in_the_zero_forcing_mode_and_what_it_refuses(threads, ctx, monkeypatch):
    """mode 16: 32 points, the estimate passes through its own pilots. The noise map and every ladder are refused there - asked of the
    library, which must answer MGPU_ERR_UNSUPPORTED and leave the context as it was."""
    refused = [("nmap", False, "own"), ("csi", False, (5, 5)), ("csi", True, "wiener")]
    assert _run_forms(16, None, threads, ctx, ZF_FORMS + refused, monkeypatch) == len(ZF_FORMS)


# ---- 2. the bank's choice ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx", CONTEXTS, ids=["agc", "noagc"])
@pytest.mark.parametrize("threads", [512, 1024])
def test_the_bank_chooses_as_its_twin_and_falls_back_on_a_nan_sounding(threads, ctx, monkeypatch):
    """rx.wiener_choice() against mgpu_host_wiener_select on every row (the four sums bit for bit), the fallback where a sounded pilot is
    NaN, and the estimate mgpu_host_wiener_estimate's with the chosen design (the H tap, through _check_row)"""
    forms = [("csi", True, "wiener"), ("nmap", False, "wiener")]
    assert _run_forms(8, None, threads, ctx, forms, monkeypatch, bank=D.bank()) == len(forms)


# ---- 3. a degenerate row does not touch its neighbours ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,bank", [(("csi", True, "own"), False), (("nmap", True, "wiener"), True)], ids=["csi_cfo", "nmap_cfo_wiener_bank"])
def test_a_degenerate_row_does_not_touch_its_neighbours(form, bank, monkeypatch):
    """The batch, the batch in reverse order, and the good frame alone on the context that has just run the batch: the good frame's payload,
    stats, LLRs, step, map rows and choice are the same bytes in all three. In the one-frame call rows 1 .. of the steps and of the choice
    still hold the previous call's values: include/mercury_cfo.h and mercury_wiener_bank.h promise that rows a span did not write keep what
    an earlier span left. include/mercury_demapper.h promises nothing of the kind for the noise map, so only its row 0 is asserted."""
    cfg, ctx = 8, CONTEXTS[1]
    b = D.batch(cfg, (), subnormal=True)
    bb, F = b["bb"], len(b["names"])
    assert F == 13
    entries = D.bank() if bank else None
    rx = _context(cfg, None, 512, ctx, monkeypatch, F)
    assert _set_form(rx, *form, bank=entries)

    def good_row(out, rep, f):
        got = [out["payload"][f].tobytes(), out["stats"][f].tobytes(), out["llr_ldpc"][f].tobytes(), rep["steps"][f].tobytes()]
        if rep["maps"] is not None:
            got += [rep["maps"][0][f].tobytes(), rep["maps"][1][f].tobytes()]
        if rep["choice"] is not None:
            got += [int(rep["choice"]["design"][f]), rep["choice"]["corr"][f].tobytes()]
        return got

    with np.errstate(all="ignore"):
        fwd = rx.receive(bb[::-1], want_llr=True)
        rev_rep = _reports(rx, form, F, entries)
        rev = good_row(fwd, rev_rep, F - 1 - b["row"]["good"])
        out = rx.receive(bb, want_llr=True)
        rep = _reports(rx, form, F, entries)
        want = good_row(out, rep, b["row"]["good"])
        assert rev == want
        assert out["stats"][b["row"]["good"]]["message_decoded"] == 1
        one = rx.receive(bb[b["row"]["good"]][None, :], want_llr=True)
        one_rep = _reports(rx, form, F, entries)
        assert good_row(one, one_rep, 0) == want
        assert one_rep["steps"][1:].tobytes() == rep["steps"][1:].tobytes()
        if entries:
            assert np.array_equal(one_rep["choice"]["design"][1:], rep["choice"]["design"][1:])
            assert one_rep["choice"]["corr"][1:].tobytes() == rep["choice"]["corr"][1:].tobytes()
    rx.close()


# ---- 4. under a ladder --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx", CONTEXTS, ids=["agc", "noagc"])
def test_ladder_retries_degenerate_rows_rung_by_rung(ctx, monkeypatch):
    """[(21, 21), (5, 5), "wiener"] with CSI and the carrier-offset stage: a row's record is that of the first rung whose host chain decodes
    it; a row no rung decodes - every degenerate row that fails its CRC is retried at each rung and fails there too - reports rung 0's record
    and rung -1, as include/mercury_estimator.h states. The steps reported are rung 0's: a retry does not write them out."""
    cfg, rungs = 8, [(21, 21), (5, 5), "wiener"]
    orc = D.oracle(cfg)
    b = D.batch(cfg, (), subnormal=ctx["agc"] == 0)
    bb, F = b["bb"], len(b["names"])
    rx = _context(cfg, None, 512, ctx, monkeypatch, F)
    with np.errstate(all="ignore"):
        plain = rx.receive(bb, taps=True)
        rx.set_demapper("csi")
        rx.set_cfo("pilots")
        rx.set_estimator_ladder([(21, 21), (5, 5), ("wiener", {})])
        out = rx.receive(bb, want_llr=True)
        won, steps = rx.last_rungs(F), rx.cfo_steps(F)
        retried = 0
        for f, name in enumerate(b["names"]):
            chains = [D.chain(cfg, None, plain["grid"][f], "csi", True, "own" if r == (21, 21) else r) for r in rungs]
            decoded = [D.decode(cfg, None, c["llr_ldpc"])[4] for c in chains]
            want = decoded.index(1) if 1 in decoded else -1
            assert won[f] == want, (name, won[f], decoded)
            rec = chains[max(want, 0)]
            assert same_bits(out["llr_ldpc"][f][: orc.N], rec["llr_ldpc"]), (name, want)
            check_decode(cfg, None, out, f, rec["llr_ldpc"], name)
            assert _scalar_same(steps[f], chains[0]["step"]), name
            retried += int(want != 0)
        assert won[b["row"]["good"]] == 0 and won[b["row"]["nan_guard"]] == 0 and retried >= 6, won
    rx.close()


# ---- 5. under diversity -------------------------------------------------------------------------------------------------------------------------------
def test_grouped_call_sums_degenerate_branches_as_floats(monkeypatch):
    """receive_div with D = 2 on (good, good), (good, NaN row), (zero row, good): the branch LLRs are the twins' rows, the decode is the
    oracle's on their float32 sum - NaN where the sum is NaN."""
    cfg, ctx = 8, CONTEXTS[1]
    orc = D.oracle(cfg)
    b = D.batch(cfg, (), subnormal=True)
    order = [b["row"][k] for k in ("good", "good", "good", "nan_mid", "zeros", "good")]
    bb = b["bb"][order]
    rx = _context(cfg, None, 512, ctx, monkeypatch, len(order))
    with np.errstate(all="ignore"):
        plain = rx.receive(bb, taps=True)
        assert _set_form(rx, "csi", True, "own")
        rows = np.stack([D.chain(cfg, None, plain["grid"][f], "csi", True, "own")["llr_ldpc"] for f in range(len(order))])
        div = rx.receive_div(bb, 2, want_llr=True)
        for f in range(len(order)):
            assert same_bits(div["llr_ldpc"][f][: orc.N], rows[f]), f     # the BRANCH LLRs
        sums = rows[0::2] + rows[1::2]                                    # float32
        assert not np.isnan(sums[0]).any() and np.isnan(sums[1]).any()
        for f in range(len(order)):
            check_decode(cfg, None, div, f, sums[f // 2], f)
        assert div["stats"]["message_decoded"][0] == 1 and np.array_equal(div["payload"][0][: orc.payload_bytes], b["payload"])
    rx.close()

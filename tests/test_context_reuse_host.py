"""The inputs of the context-reuse tests (tests/context_reuse_cases.py) held to their intended properties with the CPU oracle and the host
twins, so that tests/test_gpu_context_reuse.py cannot go vacuous if a generator changes: the good frames decode and the lost frame does
not, the frame window decodes and the noise window does not, the poison frames are what they are called, and the settings the sensitivity
check leaves on do act on the probes' inputs. No GPU."""
import numpy as np
import pytest

import context_reuse_cases as cases
from oraclelib import CARRIER, FLAGS_RECEIVE_BYTE


@pytest.mark.parametrize("cfg", cases.MODES)
def test_the_good_frames_decode_and_the_lost_frame_does_not(cfg):
    orc = cases.oracle(cfg)
    fr = cases.frames(cfg)
    for bb, payload in fr["good"]:
        ref = orc.rx(bb, FLAGS_RECEIVE_BYTE)
        # decoded: the payload comes back. (Mode 16 in the receive_byte variant divides by a ~1e-33 variance, tests/test_gpu_parity.py
        # _variants: its first frame's decoder runs to the cap on LLRs of rounding noise and the hard decisions are right all the same.)
        assert np.array_equal(ref["bytes"][: orc.payload_bytes], payload), cfg
        assert ref["iterations"] <= cases.MAX_ITERS or cfg == 16, (cfg, ref["iterations"])
    bb, payload = fr["lost"]
    ref = orc.rx(bb, FLAGS_RECEIVE_BYTE)
    assert ref["iterations"] == cases.MAX_ITERS + 1, (cfg, ref["iterations"])
    assert not np.array_equal(ref["bytes"][: orc.payload_bytes], payload), cfg
    span = cases.span_frames(cfg)
    assert span.shape == (3, orc.frame_samples)
    assert span[0].tobytes() == fr["good"][0][0].tobytes() and span[1].tobytes() == fr["lost"][0].tobytes() and span[2].tobytes() == fr["good"][1][0].tobytes()


@pytest.mark.parametrize("cfg", cases.MODES)
def test_the_poison_frames_are_poison_and_fill_the_batch_behind_the_probes_rows(cfg):
    good = cases.frames(cfg)["good"][0][0]
    p = cases.poison_frames(cfg)
    assert np.isfinite(p[0]).all() and np.abs(p[0]).max() > 1e148
    assert np.isnan(p[1][100]) and np.isfinite(np.delete(p[1], 100)).all()
    assert np.isinf(p[2][200].real) and p[2][200].real > 0 and np.isfinite(np.delete(p[2], 200)).all()
    assert not p[3].any()
    bb = cases.full_batch(cfg)
    assert bb.shape == (cases.MAX_BATCH, good.size) and bb[:3].tobytes() == cases.span_frames(cfg).tobytes()
    for row in range(3, cases.MAX_BATCH):
        assert any(bb[row].tobytes() == q.tobytes() for q in p), row
    assert all(any(bb[row].tobytes() == q.tobytes() for row in range(3, cases.MAX_BATCH)) for q in p)


@pytest.mark.parametrize("cfg", [8, 100])
def test_the_frame_window_decodes_and_the_noise_window_does_not(cfg):
    orc = cases.oracle(cfg)
    wins, payload = cases.windows(cfg)
    assert wins.shape == (2, orc.buffer_samples())
    got = orc.receive_byte(wins[0])
    assert got["message_decoded"] == 1 and np.array_equal(got["payload"], payload.astype(np.uint8)), (cfg, got["message_decoded"])
    assert orc.receive_byte(wins[1])["message_decoded"] != 1, cfg
    w16 = cases.windows_int16(cfg)
    assert w16.dtype == np.int16 and np.abs(w16.astype(np.int32)).max() == 20000
    got = orc.receive_byte(w16[0] / 32768.0)
    assert got["message_decoded"] == 1 and np.array_equal(got["payload"], payload.astype(np.uint8)), cfg
    assert orc.receive_byte(w16[1] / 32768.0)["message_decoded"] != 1, cfg
    assert cases.tx_payloads(cfg).shape == (2, orc.payload_bytes) and cases.tx_payloads(cfg)[0].tobytes() != cases.tx_payloads(cfg)[1].tobytes()


def test_the_settings_left_on_act_on_the_probes_inputs():
    """mode 8: the blanker's and the excisor's non-default settings change the span's frames and the frame window (by the host twins),
    so that a context on which they are left on cannot give the baseline's bytes; the defaults the `stages` probe uses stay apart"""
    from mercury_amd import host_blank, host_excise
    cfg = 8
    touched = 0
    for bb in cases.span_frames(cfg):
        out, rep = host_blank(cfg, bb, **cases.BLANKER_ON)
        assert rep["blanked"] == int(np.count_nonzero(out != bb))
        touched += rep["blanked"]
    assert touched > 0
    # the excisor: no bin of mode 8's clean windows stands twice above the band's median, the lowest threshold there is, so the check
    # that a left-on excisor is seen runs on mode 100, whose tones do (cases.EXCISOR_SEEN_ON)
    wins, _ = cases.windows(cases.EXCISOR_SEEN_ON)
    out, rep = host_excise(wins[0], CARRIER, **cases.EXCISOR_ON)
    assert rep["excised"] > 0 and out.tobytes() != wins[0].tobytes()
    assert cases.BLANKER_ON != cases.BLANKER_OFF and cases.EXCISOR_ON != cases.EXCISOR_OFF and cases.NMAP_ON != cases.NMAP_OFF


def test_the_tables_name_every_probe_and_disturbance_of_the_issue():
    assert [n for n, _, _ in cases.PROBES] == ["span_host", "span_one", "span_dev", "span_div", "sync", "rxbyte", "tx", "patterns", "selfsim", "stages", "hf", "extras"]
    assert {n: m for n, _, m in cases.PROBES}["span_host"] == cases.MODES
    assert [n[0] for n, _, _ in cases.DISTURBANCES] == list("abcdefghij")
    assert [cfg for cfg, name in cases.pairs() if name.startswith("i_")] == [8]
    assert len(cases.pairs()) == 4 * 9 + 1
    for cfg in cases.MODES:
        orders = cases.switch_orders(cfg)
        assert len(orders) == 2 and orders[0] != orders[1] and all(sorted(on) == sorted(off) == sorted(cases.SWITCHES) for on, off in orders)
    # a probe leaves out nothing but what the exceptions table allows: the shader-clock stamps
    assert cases.DROPPED_FIELDS == {"span_host": ("cycles",)} and "cycles" in cases.EXCEPTIONS[0][1]
    # fields(): structured arrays field by field, nested containers by name
    rec = np.zeros(2, np.dtype([("a", "<i4"), ("b", "<f8")], align=True))
    rec["a"], rec["b"] = [1, 2], [0.5, -0.0]
    got = cases.fields("x", {"r": rec, "t": (np.arange(3, dtype=np.int16), 2.5)})
    assert got == {"x.r.a": rec["a"].tobytes(), "x.r.b": rec["b"].tobytes(), "x.t[0]": np.arange(3, dtype=np.int16).tobytes(), "x.t[1]": np.float64(2.5).tobytes()}
    assert cases.differences({"p": {"f": b"1", "g": b"2"}}, {"p": {"f": b"1", "g": b"3", "h": b""}}) == [("p", "g"), ("p", "h")]

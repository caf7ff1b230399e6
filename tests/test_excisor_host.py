"""CPU tests of the carrier excisor's host twin, mgpu_host_excise (include/ext/mercury_excisor.h): the normative statement of the rule.

Yardsticks: a numpy restatement of the rule with np.fft (tests/excisor_ref.py) on windows of every length class and carrier kind; the input's
own bytes where the rule says the window passes; the noise floor for what a removed carrier leaves; the CPU oracle's receive_byte for what
the stage buys; the header's ranges for the refusals."""
import ctypes as C

import numpy as np
import pytest

import excisor_ref as er

CARRIER = 1471.875


def _twin(x, carrier=CARRIER, **prm):
    from mercury_amd import host_excise
    return host_excise(x, carrier, **prm)


def test_twin_equals_the_numpy_restatement():
    """Decisions equal; level within 1e-12 relative; output within 1e-12 max|x| (a 1024-point fp64 transform rounds at about 1e-15: the
    margin is a thousandfold)."""
    cases = er.twin_cases()
    assert {n for _, n, *_ in cases} == set(er.LENGTHS) and {k for k, *_ in cases} == set(er.CONTENTS)
    worst_out = worst_level = 0.0
    removed = 0
    for kind, n, x, y, ref in cases:
        out, rep = _twin(x)
        for k in ("exceeding", "mask", "band_lo", "excised", "nonfinite"):
            assert rep[k] == ref[k], (kind, n, k, rep[k], ref[k])
        assert abs(rep["level"] - ref["level"]) <= 1e-12 * ref["level"], (kind, n)
        err = float(np.max(np.abs(out - y)) / np.max(np.abs(x)))
        assert err <= 1e-12, (kind, n, err)
        worst_out, worst_level = max(worst_out, err), max(worst_level, abs(rep["level"] - ref["level"]) / ref["level"])
        removed += rep["excised"] > 0
    print("%d cases, %d with bins removed: worst output error %.2e max|x|, worst level error %.2e" % (len(cases), removed, worst_out, worst_level))
    assert removed >= len(cases) // 2


def test_output_may_be_the_input_and_the_report_may_be_left_out():
    from mercury_amd import load_library
    from mercury_amd.physical_layer import _ptr
    lib = load_library()
    x = np.array(er.batch(1537)[0])
    want, _ = _twin(x)
    assert want.tobytes() != x.tobytes()
    inplace = x.copy()
    assert lib.mgpu_host_excise(None, CARRIER, _ptr(inplace), inplace.size, _ptr(inplace), None) == 0       # NULL: the defaults
    assert inplace.tobytes() == want.tobytes()


@pytest.mark.parametrize("cfg", [0, 8, 13, 16, 100])
def test_a_clean_strong_frame_passes_byte_for_byte(cfg):
    t = er.toned_windows(cfg, 0.0, 0.01, 317.0, count=1)
    from oraclelib import CARRIER as carrier
    x = t["clean"][0]
    out, rep = _twin(x, carrier)
    ratio = float(np.max(er.ref_excise(x, carrier)[1]["A"]) / rep["level"])
    print("mode %d: highest bin %.2f band medians" % (cfg, ratio))
    assert rep["exceeding"] == 0 and rep["mask"] == 0 and rep["excised"] == 0 and rep["nonfinite"] == 0 and rep["level"] > 0
    assert out.tobytes() == x.tobytes()


def test_windows_the_rule_passes_come_back_byte_for_byte():
    rng = np.random.default_rng(5)
    n = 92480
    noise = 0.05 * rng.standard_normal(n)
    out, rep = _twin(noise)
    assert out.tobytes() == noise.tobytes() and rep["mask"] == 0 and rep["excised"] == 0
    zero = np.zeros(n)
    out, rep = _twin(zero)
    assert out.tobytes() == zero.tobytes() and rep["mask"] == 0 and rep["level"] == 0.0 and rep["nonfinite"] == 0
    twenty = er.content("twenty", n, rng)
    out, rep = _twin(twenty)
    assert out.tobytes() == twenty.tobytes() and rep["excised"] == 0 and bin(rep["mask"]).count("1") > 16, rep
    for one in (np.array([0.7]), np.array([-0.0])):
        out, rep = _twin(one)
        assert out.tobytes() == one.tobytes() and rep["excised"] == 0 and rep["nonfinite"] == 0
    for bad in (np.nan, np.inf, -np.inf):
        x = np.array(er.batch(4096)[0])
        x[1234] = bad
        out, rep = _twin(x)
        assert out.tobytes() == x.tobytes(), bad
        assert rep["nonfinite"] == 1 and rep["exceeding"] == 0 and rep["mask"] == 0 and rep["excised"] == 0 and rep["level"] == 0.0, (bad, rep)


def test_a_carrier_is_removed_down_to_the_noise():
    """a unit tone in noise sigma 0.01 over 92,480 samples: what is left is within a factor 2 of the noise power"""
    rng = np.random.default_rng(1)
    n = 92480
    x = er.tone(n, 1817.0, 1.0, 0.3) + 0.01 * rng.standard_normal(n)
    out, rep = _twin(x, 1500.0)
    left = float(np.mean(out ** 2))
    print("power left %.3e beside noise 1e-4; %d bins removed" % (left, rep["excised"]))
    assert rep["excised"] > 0 and 0.5e-4 <= left <= 2e-4, left


def test_what_it_buys_mode_8_at_sir_0_db():
    """The first row of profiles/excisor.md: mode 8, noise sigma 0.02, a tone at the carrier + 317 Hz as strong as the frame, threshold 8.
    The oracle decodes none of the eight raw windows and at least seven of them after the twin."""
    from oraclelib import CARRIER as carrier
    t = er.toned_windows(8, 0.0, 0.02, 317.0)
    orc = t["orc"]
    raw = sum(er.decoded(orc, orc.receive_byte(t["toned"][w]), t["payload"][w]) for w in range(8))
    cleaned = [_twin(t["toned"][w], carrier, threshold=8.0) for w in range(8)]
    got = sum(er.decoded(orc, orc.receive_byte(cleaned[w][0]), t["payload"][w]) for w in range(8))
    print("mode 8, SIR 0 dB: decoded raw %d of 8, excised %d of 8; bins removed %s" % (raw, got, [r["excised"] for _, r in cleaned]))
    assert raw == 0 and got >= 7, (raw, got)


def test_parameters_and_arguments_are_refused_as_stated():
    from mercury_amd import ExcisorParams, MgpuError, load_library, parse_excisor
    from mercury_amd.physical_layer import _ptr
    lib = load_library()
    x = np.array(er.batch(513)[0])
    out = np.zeros_like(x)

    def rc(prm, carrier=CARRIER, n=None):
        return lib.mgpu_host_excise(C.byref(prm) if prm is not None else None, carrier, _ptr(x), x.size if n is None else n, _ptr(out), None)

    for good in (ExcisorParams(2.0, 0, 1), ExcisorParams(1e300, 4, 32), ExcisorParams(12.0, 1, 16)):
        assert rc(good) == 0
    for bad in (ExcisorParams(1.999, 1, 16), ExcisorParams(float("nan"), 1, 16), ExcisorParams(float("inf"), 1, 16), ExcisorParams(-12.0, 1, 16),
                ExcisorParams(12.0, -1, 16), ExcisorParams(12.0, 5, 16), ExcisorParams(12.0, 1, 0), ExcisorParams(12.0, 1, 33)):
        assert rc(bad) == 1, (bad.threshold, bad.guard, bad.max_bins)            # MGPU_ERR_ARG
    assert rc(None, n=0) == 1 and rc(None, n=-3) == 1
    assert rc(None, carrier=float("nan")) == 1 and rc(None, carrier=float("inf")) == 1
    assert lib.mgpu_host_excise(None, CARRIER, None, 4, _ptr(out), None) == 1 and lib.mgpu_host_excise(None, CARRIER, _ptr(x), 4, None, None) == 1
    with pytest.raises(MgpuError):
        _twin(x, guard=7)
    # without a context every context call is refused before it looks at anything else (params_size: tests/test_gpu_excisor.py)
    prm, mode = ExcisorParams(12.0, 1, 16), C.c_int()
    assert lib.mgpu_set_excisor(None, 1, C.byref(prm), C.sizeof(prm)) == 1 and lib.mgpu_get_excisor(None, C.byref(mode), C.byref(prm), C.sizeof(prm)) == 1
    assert lib.mgpu_get_excisor_report(None, 0, 0, None) == 1 and lib.mgpu_excise_dev(None, None, 0, 1, CARRIER, None, None, None) == 1
    assert C.sizeof(ExcisorParams) == 16
    # the band's clamp at either end
    assert _twin(x, 0.0)[1]["band_lo"] == 1 and _twin(x, 23000.0)[1]["band_lo"] == 448 and _twin(x, 3000.0)[1]["band_lo"] == 32
    # the tools' form
    assert parse_excisor("off") == ("off", None) and parse_excisor("welch")[1] == dict(threshold=12.0, guard=1, max_bins=16)
    assert parse_excisor("welch:thr=8,guard=2,bins=24") == ("welch", dict(threshold=8.0, guard=2, max_bins=24))
    for text in ("median", "off:thr=3", "welch:share=1"):
        with pytest.raises(ValueError):
            parse_excisor(text)

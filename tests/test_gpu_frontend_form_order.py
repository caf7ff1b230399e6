"""GPU test of the front-end's LDS limits: whichever order a context's options are set in, every form they make together must be allowed its
whole LDS carve (launch.hip frontend_raise_lds_limits). Mode 0 is where a forgotten form shows - the BPSK geometry's carve exceeds the
default dynamic-LDS limit, so its launch fails -, at both workgroup sizes.

Per order of enabling {one-rung Wiener ladder, MGPU_CFO_PILOTS, MGPU_DEMAP_NMAP}: a span of two frames after each step, then the options
off again in reverse and the plain form once more. Yardstick: frontend_forms_ref.expected - the CPU oracle's grid through the host twins
chained on the host (frontend_degenerate_ref.chain, as tests/test_gpu_frontend_degenerate.py) and the numpy restatement of the part all
forms share behind them, which tests/test_frontend_forms_host.py holds to the oracle. Bit for bit: the grid, the LLRs before and behind the
de-interleaver, the variance as a double and as the float the stats carry, the steps, the factors, and the decode behind the LLRs. The SNR
variance leaves the library only as stats.snr_db = float(10 log10(1 / it)): compared within 2e-5 relative, the bound
tests/test_gpu_parity.py gives the device's log10 against the reference's - mode 0 restores the amplitude, so the SNR variance is not the
reported variance, and a span that took the one for the other is some dB off."""
import itertools

import numpy as np
import pytest

import frontend_degenerate_ref as D
import frontend_forms_ref as R
from frontend_degenerate_ref import FE_THREADS, check_decode, same_bits

pytestmark = pytest.mark.gpu

CFG, F = 0, 2
ON = dict(wiener=lambda rx: rx.set_estimator_ladder([("wiener", {})]), cfo=lambda rx: rx.set_cfo("pilots"), nmap=lambda rx: rx.set_demapper("nmap"))
OFF = dict(wiener=lambda rx: rx.set_estimator_ladder([]), cfo=lambda rx: rx.set_cfo("off"), nmap=lambda rx: rx.set_demapper("maxlog"))


def _check_span(rx, on, where):
    orc = D.oracle(CFG)
    out = rx.receive(R.frames(CFG), taps=True)
    steps = rx.cfo_steps(F) if "cfo" in on else None
    maps = rx.noise_map(0, F) if "nmap" in on else None
    for f in range(F):
        e = R.expected(CFG, f, "wiener" in on, "cfo" in on, "nmap" in on)
        at = (where, sorted(on), f)
        st = out["stats"][f]
        assert same_bits(out["grid"][f], e["grid"]), at
        assert same_bits(out["llr_demod"][f], e["llr_demod"]), at
        assert same_bits(out["llr_ldpc"][f][: orc.N], e["llr_ldpc"]), at
        assert np.float64(out["variance"][f]).tobytes() == np.float64(e["variance"]).tobytes(), at
        assert np.float32(st["variance"]).tobytes() == np.float64(e["variance"]).astype(np.float32).tobytes(), at
        if check_decode(CFG, None, out, f, e["llr_ldpc"], at):
            assert abs(float(st["snr_db"]) - e["snr_db"]) <= 2e-5 * max(1.0, abs(e["snr_db"])), at
        assert e["variance"] != e["snr_variance"], at
        if steps is not None:
            assert np.float64(steps[f]).tobytes() == np.float64(e["step"]).tobytes() and e["step"] != 0.0, (at, steps[f], e["step"])
        if maps is not None:
            assert same_bits(out["H"][f], e["H"]), at                          # the noise map shows the full estimate
            assert maps[0][f].tobytes() == e["fc"].tobytes() and maps[1][f].tobytes() == e["fs"].tobytes(), at
    assert out["stats"][0]["message_decoded"] == 1, (where, sorted(on))      # frame 0 is the frame every form decodes


@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("order", list(itertools.permutations(("wiener", "cfo", "nmap"))), ids="-".join)
def test_every_order_of_setting_the_options_runs_every_form_they_make(order, threads, monkeypatch):
    from mercury_amd import RxPhy
    monkeypatch.setenv(FE_THREADS, str(threads))
    rx = RxPhy(CFG, max_batch=F)
    monkeypatch.delenv(FE_THREADS)
    on = set()
    for option in order:                                                     # a setter that fails raises MgpuError: every call is MGPU_OK
        ON[option](rx)
        on.add(option)
        _check_span(rx, on, (order, threads))
    for option in reversed(order):
        OFF[option](rx)
    _check_span(rx, set(), (order, threads))
    rx.close()

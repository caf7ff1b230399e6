"""CPU test of the HF channel reference the GPU tests use (tests/hf_channel_ref.py): the library's host twin mgpu_host_hf_channel_taps and
the numpy composition of the host definitions against the closed form in 80-bit extended precision, within the derived budget, from the
origin to a stream position beyond 2^32 samples where the phase is about 1e7 rad. Run with -s for the measured fractions of the budget."""
import numpy as np
import pytest

from hf_channel_ref import (U, _numpy_channel, channel_longdouble, path_amps, tap_bound, taps_longdouble, worst_ratio)

T0S = [0, -700, 98765, 2 ** 32 + 320]
N = 2049


def _channels():
    from mercury_amd import HfChannel, hf_channel_preset
    return {"flutter48": (hf_channel_preset("flutter"), 48000.0),
            "shifts192": (HfChannel(((0.0, 0.0, 0.0, 7.5), (10.0, -3.0, 1.0, -7.5))), 192000.0)}


@pytest.mark.parametrize("t0", T0S)
@pytest.mark.parametrize("name", ["flutter48", "shifts192"])
def test_host_taps_lie_within_the_phase_budget_of_the_80_bit_closed_form(name, t0):
    from mercury_amd import host_hf_channel_taps
    ch, fs = _channels()[name]
    for seed, r in ((21, 100), (0x4D455243, 2 ** 33 + 5)):
        got = host_hf_channel_taps(ch, fs, seed, r, N, t0=t0)
        ref = taps_longdouble(ch, fs, seed, r, N, t0)
        direct = taps_longdouble(ch, fs, seed, r, N, t0, block=None)
        bound, phi = tap_bound(ch, fs, seed, r, N, t0)
        err = np.abs(got - ref).max(axis=1)
        per_u_phi = err / np.array([a * ns * U * p for (a, ns), p in zip(path_amps(ch), phi)])
        print("%s t0 = %d: error %s, of the budget %s, in units of amp ns 2^-53 Phi %s (Phi %s)" % (name, t0, err, err / bound, per_u_phi, phi))
        assert np.all(err <= bound), (name, t0, err, bound)
        # the blocked evaluation and the direct one are the same 80-bit closed form: eight 2^-64 roundings of the phase between them and the
        # final rounding to double of either
        same = np.array([a * ns * (8 * 2.0 ** -64 * p + 2 * U) for (a, ns), p in zip(path_amps(ch), phi)])
        assert np.all(np.abs(ref - direct).max(axis=1) <= same), (name, t0)
    if t0 > 2 ** 32:
        assert np.all(phi > 1e6)             # the case is what it says: ~1e7 rad, where 1e-10 x RMS is no yardstick
        assert err.max() > 1e-11


@pytest.mark.parametrize("t0", T0S)
@pytest.mark.parametrize("name", ["flutter48", "shifts192"])
def test_numpy_composition_equals_the_80_bit_composition_within_the_budget(name, t0):
    ch, fs = _channels()[name]
    rng = np.random.default_rng(abs(t0) % 1000)
    for x in (rng.standard_normal((2, N)), rng.standard_normal((2, N)) + 1j * rng.standard_normal((2, N))):
        got = _numpy_channel(x, ch, 21, 100, fs, t0=t0)
        ratio = worst_ratio(got, x, ch, 21, 100, fs, t0)
        print("%s t0 = %d %s: error / budget %.3f" % (name, t0, "complex" if np.iscomplexobj(x) else "real", ratio))
        assert ratio <= 1.0, (name, t0, ratio)


def test_the_80_bit_composition_is_the_definition_on_a_case_done_by_hand():
    """One static path, 3 samples of delay, a shift and an offset: y[i] = e^{j 2 pi (shift + offset) t_i} x[i - 3], nothing else."""
    from mercury_amd import HfChannel
    ch = HfChannel(((0.25, -20.0, 0.0, 2.5),), freq_offset_hz=1.0)
    x = np.arange(1, 9) * (1 + 0.5j)
    y = channel_longdouble(x[None], ch, 1, 0, 12000.0, t0=-4)[0]
    t = (np.arange(8) - 4) / 12000.0
    want = np.zeros(8, np.complex128)
    want[3:] = np.exp(2j * np.pi * 3.5 * t[3:]) * x[:5]
    assert np.max(np.abs(y - want)) <= 1e-15 * 8

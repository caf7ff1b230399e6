"""The carrier tuner on the GPU (include/ext/mercury_tuner.h, mercury_amd.Tuner): G, E, Q and every report against the normative host
twin, bit for bit, over the shapes at which the kernels take another path; statelessness; a NaN block; memory; and three links end to
end: synthesiser -> noise -> scanner -> plan -> tuner -> channeliser with the tuned plan -> captures.

The mix kernel's LDS image depends on D and T: D = 1 and 3 have one block of steps, D = 16 with the default taps and D = 64 stream the
steps through in two (D = 64 at the image's limit of 256 rows by 17 columns); S = 1 runs one wavefront, S = 3 one with three channels,
S = 17 two groups of channels, the second with one."""
import numpy as np
import pytest

import tuner_ref as ref
from band_links import CARRIER, ThreeLinks, iq as make_iq, rx as _rx, taps, torch as _torch
from mercury_amd import (BandScanner, Channelizer, MgpuError, RxCapture, Synthesizer, Tuner, host_tune_process, tune_reports,
                         tune_samples)

pytestmark = pytest.mark.gpu


def _plan(rng, D, S):
    """S channels anywhere a band fits, both sidebands"""
    half = 24000 * D
    out = []
    for s in range(S):
        sb = s % 2
        lo, hi = (-half + 1, half - 2945) if sb == 0 else (-half + 2945, half - 1)
        out.append((int(rng.integers(lo, hi + 1)), sb, 1.0))
    return out


def _device_equals_twin(tn, x, plan, **config):
    got = (tn.process_raw(x),) + tn.arrays()
    want = host_tune_process(x, tn.D, plan, want_arrays=True, **config)
    assert want[0]["nonfinite"].max() == 0
    for name, a, b in zip(("reports", "G", "E", "Q"), got, want):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), name
    return got


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("D", [1, 3])
def test_arrays_and_reports_equal_the_twin_in_every_format_from_host_and_device_memory(D, S):
    """tp = 8, J = 4: a generated frame per channel with the plan a few hertz to a carrier off, so that the reports decide something"""
    torch = _torch()
    rng = np.random.default_rng(10 * D + S)
    true = _plan(rng, D, S)
    plan = [(o + int(rng.integers(-60, 61)), sb, g) for o, sb, g in true]
    config = dict(symbols=4, search=8, taps=taps(D, 8))
    tn = Tuner(_rx(), D, plan, **config)
    assert tn.samples == tune_samples(D, 4) and tn.channels == plan
    for fmt in ("cs16", "cf32", "cf64"):
        x = ref.block(100 + D, D, true, symbols=4, n_symbols=3, noise_db=-30, fmt=fmt, taps=taps(D, 8))
        if fmt == "cs16":
            x[3], x[-1] = (-32768, 32767), (32767, -32768)
        _device_equals_twin(tn, x, plan, **config)
        d_x = torch.from_numpy(x).cuda()
        torch.cuda.synchronize()                                        # the library works on its own stream
        _device_equals_twin(tn, d_x, plan, **config)
    tn.close()


@pytest.mark.parametrize("D,tp,J,S", [(1, None, 4, 3), (3, 8, 32, 3), (16, None, 4, 1), (64, 8, 4, 2), (1, 8, 5, 17), (2, 8, 7, 1)])
def test_arrays_and_reports_equal_the_twin_at_the_shapes_the_kernels_change_at(D, tp, J, S):
    """the default taps; J = 32; two blocks of steps (D = 16 with the default taps; D = 64, the largest image); more channels than a
    workgroup has; J = 5 and 7, no multiple of the comb kernel's four symbols at a time"""
    rng = np.random.default_rng(1000 * D + J)
    plan = _plan(rng, D, S)
    config = dict(symbols=J, search=24 if S == 17 else 8, taps=None if tp is None else taps(D, tp))
    x = make_iq(rng, tune_samples(D, J), "cf32")
    tn = Tuner(_rx(), D, plan, **config)
    _device_equals_twin(tn, x, plan, **config)
    tn.close()


def test_a_call_stands_alone():
    """two calls in a row, the first block again, and a call after retune: each equals a fresh twin"""
    D, config = 3, dict(symbols=4, search=8, taps=taps(3, 8))
    rng = np.random.default_rng(5)
    plan = _plan(rng, D, 3)
    a, b = (make_iq(rng, tune_samples(D, 4), "cf64") for _ in range(2))
    tn = Tuner(_rx(), D, plan, **config)
    first = _device_equals_twin(tn, a, plan, **config)
    _device_equals_twin(tn, b, plan, **config)
    again = _device_equals_twin(tn, a, plan, **config)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))
    plan[1] = (plan[1][0] + 777, 0, 2.0)
    tn.retune(1, plan[1])
    assert tn.channels == plan
    _device_equals_twin(tn, a, plan, **config)
    for bad in ((24000 * D, 0, 1.0), (0, 2, 1.0)):
        with pytest.raises(MgpuError) as e:
            tn.retune(0, bad)
        assert e.value.code == 1
    with pytest.raises(MgpuError):
        tn.retune(3, plan[0])
    _device_equals_twin(tn, b, plan, **config)
    for wrong in (a[:-1], np.concatenate([a, a[:1]])):
        with pytest.raises(MgpuError) as e:
            tn.process_raw(wrong)
        assert e.value.code == 1
    tn.close()


def test_a_bad_configuration_is_refused_with_a_context_and_says_why():
    rx = _rx()
    for bad, why in ((dict(symbols=3), "symbols must be 4..256"), (dict(search=25), "search must be 0..24"),
                     (dict(min_metric=0.0), "min_metric must lie in (0, 1]"), (dict(carrier_hz=24000.0), "carrier_hz must lie in (0, 24000)"),
                     (dict(taps=np.ones(8)), "ntaps must be tp * D + 1 with tp even, 2..512")):
        with pytest.raises(MgpuError) as e:
            Tuner(rx, 1, [(0, 0, 1.0)], **bad)
        assert e.value.code == 1 and rx.lib.mgpu_last_error(rx.h).decode() == "mgpu_tune_create: " + why
    for channels in ([], [(24000 - 2944, 0, 1.0)], [(0, 2, 1.0)]):
        with pytest.raises(MgpuError) as e:
            Tuner(rx, 1, channels)
        assert e.value.code == 1


def test_arrays_before_the_first_call_are_refused():
    tn = Tuner(_rx(), 1, [(0, 0, 1.0)], symbols=4, taps=taps(1, 8))
    with pytest.raises(MgpuError) as e:
        tn.arrays()
    assert e.value.code == 1
    tn.close()


def test_a_nan_block_is_reported_nonfinite_and_the_next_call_is_clean():
    D, config = 1, dict(symbols=4, search=8, taps=taps(1, 8))
    rng = np.random.default_rng(6)
    plan = _plan(rng, D, 3)
    x = make_iq(rng, tune_samples(D, 4), "cf64")
    bad = x.copy()
    bad[len(bad) // 2] = complex(np.nan, 0.0)
    tn = Tuner(_rx(), D, plan, **config)
    reports = tn.process_raw(bad)
    assert reports.tobytes() == host_tune_process(bad, D, plan, **config).tobytes()
    assert list(reports["nonfinite"]) == [1, 1, 1] and list(reports["valid"]) == [0, 0, 0]
    assert [int(o) for o in reports["offset_hz"]] == [p[0] for p in plan]
    assert tn.plan(reports) == plan
    _device_equals_twin(tn, x, plan, **config)
    tn.close()


def test_create_use_destroy_gives_the_memory_back():
    """50 create / process / destroy cycles (tables, the 12 kHz workspace, staging, the arrays) leave the device's free memory where it
    was"""
    import gc
    torch = _torch()

    def free_hbm():
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info()[0]

    rx = _rx()
    D, S = 16, 8
    plan = _plan(np.random.default_rng(8), D, S)
    x = make_iq(np.random.default_rng(9), tune_samples(D, 32), "cf32")

    def cycle():
        tn = Tuner(rx, D, plan)
        tn.process_raw(x)
        return tn

    cycle().close()
    first = free_hbm()
    tn = cycle()
    in_use = first - free_hbm()
    tn.close()
    assert in_use >= x.nbytes, in_use                                   # the staging area alone
    for _ in range(50):
        cycle().close()
    after = free_hbm()
    assert abs(after - first) < 64 << 20, (first, after)


# ---- three links end to end -------------------------------------------------------------------------------------------------------------
HOPS_PER_CALL = 16
LINK_D = 4
LINK_PLAN = [(-61000, 0, 1.0), (12500, 0, 1.0), (70250, 1, 1.0)]          # tests/scanner_ref.py's: two USB links and one LSB link
NOISE_DB = -40.0
LINKS = ThreeLinks(seed=2024, tail=320, hops_per_call=HOPS_PER_CALL)      # synthesiser and channeliser delay a frame by tp = 320 samples


def _band(starts):
    """the three links' frames at their starts through the synthesiser, plus noise at -40 dB (seeded) -> complex64 IQ on the device"""
    torch = _torch()
    audio = LINKS.audio(starts)
    sy = Synthesizer(_rx(), LINK_D, LINK_PLAN)
    step = HOPS_PER_CALL * 1088
    assert audio.shape[1] % step == 0
    iq = np.concatenate([sy.process(np.ascontiguousarray(audio[:, at: at + step]), fmt="cf32") for at in range(0, audio.shape[1], step)])
    sy.close()
    rng = np.random.default_rng(77)
    amp = np.float32(10 ** (NOISE_DB / 20.0))
    iq = iq + amp * (rng.standard_normal(iq.size, np.float32) + 1j * rng.standard_normal(iq.size, np.float32))
    d_iq = torch.from_numpy(iq.astype(np.complex64)).cuda()
    torch.cuda.synchronize()
    return d_iq


def _delivered(d_iq, plan):
    """the links that arrive through a channeliser made from `plan`"""
    rx = _rx()
    ch = Channelizer(rx, LINK_D, plan)
    cap = RxCapture(rx, 3, CARRIER, max_hops=HOPS_PER_CALL)
    step = HOPS_PER_CALL * cap.P * LINK_D
    events = []
    for c in range(d_iq.numel() // step):
        events += [(e[0], c, None, e[3].tobytes()) for e in cap.run_wideband(ch, d_iq[c * step: (c + 1) * step])]
    ch.close(), cap.close()
    return LINKS.delivered(events)


def _starts_the_true_plan_delivers_a_hertz_either_side():
    """Per link the first of FIRST_STARTS + 156 k, k = 0 .. 5, at which the existing stages (Synthesizer, Channelizer, RxCapture) deliver
    the link through the plan it was placed with and through that plan shifted by -1 and by +1 Hz: what is chosen by is the existing
    loop on plans that are known, never the tuner's output (band_links.ThreeLinks.starts_the_loop_delivers)."""
    from band_links import FIRST_STARTS
    chosen = [None] * 3
    for k in range(6):
        cand = tuple(FIRST_STARTS[s] + 156 * k for s in range(3))
        d_iq = _band(cand)
        ok = {0, 1, 2}
        for shift in (-1, 0, 1):
            ok &= _delivered(d_iq, [(o + shift, sb, g) for o, sb, g in LINK_PLAN])
        for s in ok:
            if chosen[s] is None:
                chosen[s] = cand[s]
        if all(c is not None for c in chosen):
            break
    assert all(c is not None for c in chosen), ("the loop delivers no candidate of a link a hertz either side", chosen)
    print("starts the true plan delivers at -1, 0 and +1 Hz:", chosen)
    return tuple(chosen)


def test_three_links_end_to_end_through_the_tuned_plan():
    """Mode 8, three links, D = 4, noise at -40 dB: the scanner's line with the most power gives the found plan (each link's own
    sideband), the tuner refines it on the block that begins with that line (the last block that fits, should the line lie near the
    end), and the channeliser receives through the tuned plan. Every link's tuned offset is within 1 Hz of the offset it was placed at,
    and every link that the true plan delivers is delivered through the tuned plan. What the untuned found plan delivers is printed."""
    rx = _rx()
    d_iq = _band(_starts_the_true_plan_delivers_a_hertz_either_side())
    sc = BandScanner(rx, LINK_D)
    per_line = sc.H * sc.A
    whole = d_iq.numel() // per_line * per_line
    per_call = max(sc.max_in // per_line, 1) * per_line
    lines, reports = [], []
    for at in range(0, whole, per_call):
        got = sc.process(d_iq[at: min(at + per_call, whole)])
        lines.append(got[0])
        reports += got[1]
    best = int(np.argmax(np.concatenate(lines).sum(axis=1)))
    usb, lsb = sc.plan(reports[best], sideband=0), sc.plan(reports[best], sideband=1)
    sc.close()
    assert len(usb) == len(lsb) == 3
    found = [(lsb if sb else usb)[i] for i, (_, sb, _) in enumerate(sorted(LINK_PLAN))]
    assert sorted(LINK_PLAN) == LINK_PLAN
    tn = Tuner(rx, LINK_D, found)
    at = min(best * per_line, d_iq.numel() - tn.samples)
    tuned_reports = tn.process(d_iq[at: at + tn.samples])
    tuned = tn.plan(tuned_reports)
    tn.close()
    print("found", found, "tuned", tuned, "reports", tuned_reports)
    for (offset, sb, _), t, r in zip(LINK_PLAN, tuned, tuned_reports):
        assert r["valid"] == 1 and t[1] == sb and abs(t[0] - offset) <= 1, (t, offset, r)
    control, through = _delivered(d_iq, LINK_PLAN), _delivered(d_iq, tuned)
    print("delivered through the true plan", sorted(control), "the tuned plan", sorted(through), "the found plan untuned",
          sorted(_delivered(d_iq, found)))
    assert control <= through

"""Host-only parts of the wideband synthesiser (include/ext/mercury_synth.h): the normative twin against the rule's textbook form in
longdouble, the round trip through the channeliser's twin, cutting the stream, the refusals and the CS16 output. No GPU."""
import ctypes as C

import numpy as np
import pytest

import synth_ref as sr
from band_links import create_without_a_context, refused as _refused
from mercury_amd import (SYNTH_SYMBOLS, MgpuError, chan_channels, host_chan_design, host_chan_process, host_synth_process, host_synth_tables,
                         load_library, synth_config)
from mercury_amd.physical_layer import SynthConfig, SynthState

POSITION = 2 ** 40 + 7


def test_symbols_are_exported_and_the_struct_layouts_are_the_headers():
    lib = load_library()
    assert len(SYNTH_SYMBOLS) == 10
    for name in SYNTH_SYMBOLS:
        assert hasattr(lib, name), name
    assert C.sizeof(SynthConfig) == 40          # 5 ints, padding, a pointer, int, padding
    assert C.sizeof(SynthState) == 40           # two uint64, six ints


def _plan(D, S, first):
    """S channels that fit (-R/2, R/2) at any D: a negative offset on USB, a positive one on LSB, one near the band's lower edge"""
    half = 24000 * D
    chs = [(-half // 3 - 7, 0, 0.7), (half // 2 + 11, 1, 1.3), (-half + 2945, 1, 2.1)]
    return (chs[first:] + chs[:first])[:S]


@pytest.mark.parametrize("tp", [2, 8, 320])
@pytest.mark.parametrize("D", [1, 3, 4, 16, 64])
def test_twin_equals_the_textbook_form(D, tp):
    """S in {1, 3}, USB and LSB, negative offsets, position 0 and 2^40 + 7. Per output |twin - ref| <= (tp + 16 + S) 2^-52 W with
    W = sum_s G_s sum_j |h[j D + r]| |a_s[n - j]|: a chain of up to tp + 1 fused multiply-adds is off by at most (tp + 1) 2^-53 W, the
    tables q, W and P by a few 2^-52 each (an angle below 2 pi from three rounded operations), the products E, v E, G z and the S - 1
    additions by 2^-53 each; the count is doubled. n_in = tp + 9: outputs on fewer than tp + 1 samples and on all of them."""
    h = host_chan_design(D, tp)
    rng = np.random.default_rng(10 * D + tp)
    n_in = tp + 9
    worst = 0.0
    for S, position, first in ((1, 0, 0), (1, POSITION, 1), (3, 0, 2), (3, POSITION, 0)):
        chs = _plan(D, S, first)
        audio = rng.standard_normal((S, n_in))
        got = host_synth_process(D, chs, audio, position=position, taps=h)
        assert got.shape == (n_in * D,) and got.dtype == np.complex128
        ms = sr.outputs_to_check(n_in, D, h.size, seed=S)
        want, weight = sr.textbook(D, chs, audio, h, position=position, ms=ms)
        err = np.abs(got[ms].astype(sr.CLD) - want).astype(np.float64)
        bound = (tp + 16 + S) * 2.0 ** -52 * weight
        assert np.abs(want).max() > 1e-3
        live = weight > 0
        worst = max(worst, float((err[live] / bound[live]).max()))
        assert np.all(err <= bound), (S, position, float((err[live] / bound[live]).max()))
        if position:                                                    # the position matters
            assert np.abs(got - host_synth_process(D, chs, audio, taps=h)).max() > 1e-3
    print("D = %d, tp = %d: worst error / bound %.3f" % (D, tp, worst))


def test_tables_are_the_rule():
    """q, P, G and W as the device reads them against the definition with Python integers; q- is q+'s conjugate to the bit and h sits on
    the centre tap. 4e-15: an angle below 2 pi from three rounded operations is off by at most 1.3e-15, and so are its cosine and sine"""
    D, h = 4, host_chan_design(4, 8)
    c, R = (h.size - 1) // 2, 48000 * D
    qu, Pu, Gu, W = host_synth_tables(D, (-90001, 0, 0.3), taps=h, want_phasor=True)
    ql, Pl, Gl = host_synth_tables(D, (88888, 1, 1.0), taps=h)
    want = h * np.exp(2j * np.pi * np.array([(1472 * (k - c)) % R for k in range(h.size)], np.float64) / R)
    assert np.abs(qu - want).max() <= 4e-15 and qu[c] == h[c]
    assert np.array_equal(ql.real, qu.real) and np.array_equal(ql.imag, -qu.imag)
    for P, off in ((Pu, -90001), (Pl, 88888)):
        assert np.abs(P - np.exp(2j * np.pi * np.array([(off * r) % R for r in range(D)], np.float64) / R)).max() <= 4e-15 and P[0] == 1.0
    assert Gu == (2.0 * D) * 0.3 and Gl == 2.0 * D
    assert np.abs(W - np.exp(2j * np.pi * np.arange(48000) / 48000)).max() <= 4e-15 and W[0] == 1.0


FREQS, AMPS, PHASES = (310.0, 700.0, 1471.0, 2100.0, 2640.0), (0.3, 0.25, 0.2, 0.15, 0.1), (0.0, 1.0, 2.0, 3.0, 4.0)


@pytest.mark.parametrize("sideband", [0, 1])
def test_round_trip_through_the_channeliser_is_a_delay_of_tp(sideband):
    """Tones inside 300 .. 2650 Hz through host_synth_process -> host_chan_process with the same plan and prototype come back delayed by
    tp samples. The allowed error comes from the prototype's own response, evaluated from the taps: its largest deviation from 1 within
    1178 Hz of the band centre (the tones' band around a_c = 1472) plus its largest level from 2 a_c - 1172 = 1772 Hz on (the nearest
    edge of the opposite sideband's image, the audio's negative frequencies), doubled for the two filters, times the sum of the tones'
    amplitudes. A neighbour 3 kHz away and 30 dB stronger moves the first channel's audio by no more than that stop-band level times
    its gain ratio times the sum of its tones' amplitudes."""
    D, n = 4, 3000
    h = host_chan_design(D)
    tp = (h.size - 1) // D
    f, H = sr.response(h, D)
    ripple, stop = np.abs(H[f <= 1178.0] - 1.0).max(), H[f >= 1772.0].max()
    tol = 2 * (ripple + stop) * sum(AMPS)
    print("ripple %.3e, stop band %.3e (%.1f dB): allowed %.3e" % (ripple, stop, 20 * np.log10(stop), tol))
    assert tol < 0.02 * sum(AMPS)                                        # a bound that says something
    audio = sr.tones(n, FREQS, AMPS, PHASES)
    off = 20000 if sideband else -30000
    ch = (off, sideband, 1.0)
    back = host_chan_process(D, [ch], host_synth_process(D, [ch], audio, taps=h), taps=h)[0]
    err = np.abs(back[2 * tp:] - audio[tp: n - tp]).max()               # behind both filters' transients
    print("sideband %d: round trip error %.3e" % (sideband, err))
    assert err <= tol, (err, tol)
    assert np.abs(back[2 * tp:] - audio[2 * tp:]).max() > 10 * tol      # and it is a delay: not the input undelayed
    # the neighbour: its band starts 3 kHz from ours, on the side ours grows to
    ratio = 10 ** (30 / 20.0)
    other = (off - 3000 if sideband else off + 3000, sideband, ratio)
    theirs = sr.tones(n, FREQS[::-1], AMPS, PHASES[::-1])
    iq = host_synth_process(D, [ch, other], np.stack([audio, theirs]), taps=h)
    beside = host_chan_process(D, [ch], iq, taps=h)[0]
    moved = np.abs(beside - back)[2 * tp:].max()                        # the tones start abruptly: behind that transient too
    print("sideband %d: moved by the neighbour %.3e, allowed %.3e" % (sideband, moved, stop * ratio * sum(AMPS)))
    assert moved <= stop * ratio * sum(AMPS), (moved, stop * ratio * sum(AMPS))


def test_cutting_the_stream_at_a_seek():
    """the twin fed whole equals, from the cut on, the twin seeked to the cut's position and fed the rest, bit for bit, where the tp
    samples before the cut are zeros (what a seek makes of the history)"""
    D, tp, cut, n = 3, 8, 40, 90
    h = host_chan_design(D, tp)
    chs = _plan(D, 3, 0)
    audio = np.random.default_rng(3).standard_normal((3, n))
    audio[:, cut - tp: cut] = 0.0
    for fmt in ("cf64", "cf32", "cs16"):
        whole = host_synth_process(D, chs, audio * 0.05, position=POSITION, fmt=fmt, taps=h)
        rest = host_synth_process(D, chs, audio[:, cut:] * 0.05, position=POSITION + cut, fmt=fmt, taps=h)
        assert whole[cut * D:].tobytes() == rest.tobytes(), fmt
    audio[:, cut - 1] = 1.0                                             # a sample the seek forgets
    whole = host_synth_process(D, chs, audio, position=POSITION, taps=h)
    assert whole[cut * D:].tobytes() != host_synth_process(D, chs, audio[:, cut:], position=POSITION + cut, taps=h).tobytes()


def test_refusals_need_no_device():
    D = 4
    audio = np.random.default_rng(1).standard_normal((1, 16))
    good = [(0, 0, 1.0)]
    assert host_synth_process(D, good, audio, taps=host_chan_design(D, 2)).shape == (16 * D,)
    _refused(lambda: host_synth_process(D, good, audio, taps=np.ones(3 * D + 1)))           # odd tp
    _refused(lambda: host_synth_process(D, good, audio, taps=np.ones(2 * D + 2)))           # T is not tp D + 1
    _refused(lambda: host_synth_process(D, good, audio, taps=np.ones(2 * D)))
    _refused(lambda: host_synth_process(D, good, audio, taps=np.ones(514 * D + 1)))         # tp > 512
    _refused(lambda: host_synth_process(0, good, audio))
    _refused(lambda: host_synth_process(65, good, audio))
    _refused(lambda: host_synth_process(D, good, audio, struct_size=36))                    # another version of the struct
    with pytest.raises(MgpuError):
        host_synth_process(D, good, audio, fmt=3)                                           # no such format: the binding's refusal
    k, _ = synth_config(D, 1)
    out = np.zeros(16 * D, np.complex128)
    args = (C.byref(k), chan_channels(good), audio.ctypes.data_as(C.c_void_p), 16, 16, 0)
    assert load_library().mgpu_host_synth_process(*args, 2, out.ctypes.data_as(C.c_void_p), None) == 0
    assert load_library().mgpu_host_synth_process(*args, 3, out.ctypes.data_as(C.c_void_p), None) == 1     # and the library's
    assert load_library().mgpu_host_synth_process(C.byref(k), chan_channels(good), audio.ctypes.data_as(C.c_void_p), 15, 16, 0, 2,
                                                  out.ctypes.data_as(C.c_void_p), None) == 1                # in_stride < n_in
    _refused(lambda: host_synth_process(D, good, audio, position=2 ** 62))                  # the chunk would pass 2^62
    R = 48000 * D
    for ch in ((R // 2 - 2944, 0, 1.0), (-R // 2, 0, 1.0), (R // 2, 1, 1.0), (-R // 2 + 2944, 1, 1.0), (0, 2, 1.0), (0, 0, float("nan"))):
        _refused(lambda: host_synth_process(D, [ch], audio))
        _refused(lambda: host_synth_tables(D, ch))
    for ch in ((R // 2 - 2945, 0, 1.0), (-R // 2 + 1, 0, 1.0), (R // 2 - 1, 1, 1.0), (-R // 2 + 2945, 1, 1.0)):      # the band's edge just inside
        assert host_synth_tables(D, ch, taps=host_chan_design(D, 2))[0].size == 2 * D + 1


def test_create_without_a_device_refuses_bad_arguments_and_reports_the_device():
    """without a context (no device could be opened) a bad configuration is still MGPU_ERR_ARG, a good one MGPU_ERR_DEVICE"""
    lib = load_library()

    def create(k, chs):
        return create_without_a_context(lib.mgpu_synth_create, C.byref(k), chs)    # and the handle is null

    chs = chan_channels([(0, 0, 1.0), (3000, 1, 1.0)])
    k, _ = synth_config(4, 2)
    assert create(k, chs) == 2                                                                     # MGPU_ERR_DEVICE
    for change in (dict(struct_size=44), dict(D=0), dict(D=65), dict(S=0), dict(audio_centre_hz=0), dict(max_in=-1)):
        k, _ = synth_config(4, 2)
        for name, v in change.items():
            setattr(k, name, v)
        assert create(k, chs) == 1, change                                                         # MGPU_ERR_ARG
    k, keep = synth_config(4, 2, taps=np.ones(14))
    assert create(k, chs) == 1
    k, _ = synth_config(4, 2)
    assert create(k, chan_channels([(0, 0, 1.0), (96000, 0, 1.0)])) == 1
    assert create(k, None) == 1
    assert lib.mgpu_synth_latency(None) < 0 and lib.mgpu_synth_destroy(None) == 1 and lib.mgpu_synth_seek(None, 0) == 1
    assert lib.mgpu_synth_status(None, None) == 1


def test_cs16_rounds_ties_to_even_and_counts_both_clamps():
    """D = 1, h = (0, 1, 0), offset 0, gain 0.5: IQ[n] = (a[n - 1], 0) exactly, so the CS16 conversion is seen alone:
    clamp(nearbyint(x * 32768), -32768, 32767), ties to even, every clamped component counted"""
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3.49, 32767.0, 32767.49, 32767.5, 32768.0, 40000.0, -32768.0, -32768.5, -32768.51, -32769.0, 1e300,
                  -1e300]) / 32768.0
    want = np.array([0, 2, 2, 0, -2, 3, 32767, 32767, 32767, 32767, 32767, -32768, -32768, -32768, -32768, 32767, -32768], np.int16)
    clamps = 4 + 3                              # 32767.5, 32768, 40000 and 1e300; -32768.51, -32769 and -1e300 (-32768.5 rounds to -32768)
    audio = np.concatenate([x, [0.0]])[None, :]
    h = np.array([0.0, 1.0, 0.0])
    ref = host_synth_process(1, [(0, 0, 0.5)], audio, taps=h)
    assert np.array_equal(ref[1:].real, x) and not ref.imag.any() and ref[0] == 0
    got, n = host_synth_process(1, [(0, 0, 0.5)], audio, fmt="cs16", taps=h, want_clamped=True)
    assert got.dtype == np.int16 and got.shape == (x.size + 1, 2)
    assert np.array_equal(got[1:, 0], want) and not got[:, 1].any()
    assert n == clamps
    f32 = host_synth_process(1, [(0, 0, 0.5)], audio, fmt="cf32", taps=h)
    assert f32.dtype == np.complex64 and np.array_equal(f32[1:].real[:-2], x[:-2].astype(np.float32))

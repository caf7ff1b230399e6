"""Host-only parts of the wideband channeliser (include/mercury_channelizer.h): the default prototype, the tables, the normative twin
against an independent numpy model, what the rule recovers from a synthesised wideband signal, and the refusals. No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import channelizer_ref as cz
from band_links import create_without_a_context, iq as _iq, refused as _refused
from mercury_amd import (CHANNELIZER_SYMBOLS, chan_channels, chan_config, host_chan_design, host_chan_process, host_chan_tables,
                         load_library)
from mercury_amd.physical_layer import ChanConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_the_struct_layouts_are_the_headers():
    lib = load_library()
    for name in CHANNELIZER_SYMBOLS:
        assert hasattr(lib, name), name
    assert C.sizeof(ChanConfig) == 40          # 5 ints, padding, a pointer, int, padding
    assert C.sizeof(chan_channels([(0, 0, 1.0)])) == 16


@pytest.mark.parametrize("D", [1, 4, 16, 64])
def test_default_design_meets_its_mask(D):
    """<= 0.05 dB of ripple over +-1200 Hz (our own signal's edge), <= -58 dB from +-1800 Hz on (the nearest edge of a neighbour 3 kHz
    away), symmetric taps that sum to 1 (323 .. 20481 taps of one sign pattern: the sum's rounding error is far below 1e-12)"""
    h = host_chan_design(D)
    assert h.size == 320 * D + 1
    assert np.array_equal(h, h[::-1])
    assert abs(h.sum() - 1.0) <= 1e-12, h.sum()
    f, db = cz.response_db(h, D)
    ripple = np.abs(db[f <= 1200.0]).max()
    stop = db[f >= 1800.0].max()
    print("D = %d: ripple %.4f dB, stop band %.2f dB" % (D, ripple, stop))
    assert ripple <= 0.05, ripple
    assert stop <= -58.0, stop
    # the default of mgpu_host_chan_default_taps is this design
    taps = np.zeros(h.size)
    n = C.c_int()
    assert load_library().mgpu_host_chan_default_taps(D, taps.ctypes.data_as(C.c_void_p), C.byref(n)) == 0
    assert n.value == h.size and np.array_equal(taps, h)


CHANNELS = {1: [(-9000, 0, 1.0), (0, 0, 0.5), (7001, 1, 2.0), (-20000, 0, 1.0)],
            3: [(-60000, 0, 1.0), (0, 1, 0.25), (50003, 0, 3.0), (-3, 1, 1.0)],
            4: [(-90001, 0, 1.0), (0, 0, 1.5), (88888, 1, 0.5), (12345, 1, 1.0)]}


@pytest.mark.parametrize("D", [1, 3, 4])
@pytest.mark.parametrize("tp", [2, 8])
def test_twin_equals_the_numpy_model(D, tp):
    """the twin against np.convolve of the widened input with g, every D-th sample, times the phasor: USB and LSB, negative, zero and
    positive offsets, every input format. 1e-12 of the output's scale: both sum at most 8 D + 1 products of about that scale in double
    (2^-53 each), in different orders"""
    rng = np.random.default_rng(100 * D + tp)
    h = host_chan_design(D, tp)
    for fmt in ("cf64", "cf32", "cs16"):
        iq = _iq(rng, 57 * D, fmt)
        got = host_chan_process(D, CHANNELS[D], iq, taps=h)
        want = cz.model(D, CHANNELS[D], iq, h)
        assert got.shape == want.shape == (4, 57)
        scale = np.abs(want).max()
        assert scale > 1e-3 and np.abs(got - want).max() <= 1e-12 * scale, (fmt, np.abs(got - want).max(), scale)


def test_tables_are_the_rule():
    """g and W as the device reads them against the definition evaluated with Python integers; h sits on the centre tap. 4e-15: an angle
    below 2 pi from three rounded operations is off by at most 3 * 2^-51 = 1.3e-15 on either side, and so are its cosine and sine"""
    D, h = 4, host_chan_design(4, 8)
    for off, sb in ((-90001, 0), (0, 1), (88888, 1)):
        g, W = host_chan_tables(D, (off, sb, 1.0), taps=h, want_phasor=True)
        assert np.abs(g - cz.tap_row(h, D, off, sb)).max() <= 4e-15
        c = (h.size - 1) // 2
        assert g[c] == h[c]                                         # q = 0 at the centre: the band-pass is a pure delay
    assert np.abs(W - np.exp(2j * np.pi * np.arange(48000) / 48000)).max() <= 4e-15 and W[0] == 1.0


def _recover(sidebands, with_neighbour):
    D, n = 4, 24000
    rng = np.random.default_rng(7 + with_neighbour + 10 * sidebands[0])
    audio = np.stack([cz.band_noise(rng, n), cz.band_noise(rng, n)])
    offs = [-30000, -27000] if not sidebands[0] else [-27000, -30000]      # the neighbour's band starts 3 kHz from ours, on the side ours grows to
    gains = [1.0, 10 ** (30 / 20.0)]
    S = 2 if with_neighbour else 1
    iq = cz.synthesise(audio[:S], D, offs[:S], sidebands[:S], gains[:S]).astype(np.complex64)
    y = host_chan_process(D, [(offs[0], sidebands[0], 1.0)], iq)[0]
    return cz.error_db(y, audio[0], 160, 1000)


@pytest.mark.parametrize("sideband", [0, 1])
def test_twin_recovers_the_transmitted_audio(sideband):
    """band-limited noise audio (300 .. 2644 Hz) through the synthesiser at D = 4, float32 IQ: the twin returns the audio delayed by L = 160
    samples. Alone: error <= -50 dB (0.05 dB of pass-band ripple is an amplitude error of 0.6 %, -44.8 dB, at its worst frequency; the
    measured ripple of 0.011 dB is -58 dB, averaged over the band less). Beside a neighbour 3 kHz away and 30 dB stronger: <= -27 dB
    (-58 dB of stop band + 30 dB, with 1 dB for the own-channel term). A missing (k - c) centring or (n - L) in the phasor turns the audio
    by a constant phase: an error of several dB above 0."""
    alone = _recover([sideband, sideband], False)
    beside = _recover([sideband, sideband], True)
    print("sideband %d: alone %.1f dB, beside a neighbour 30 dB stronger %.1f dB" % (sideband, alone, beside))
    assert alone <= -50.0, alone
    assert beside <= -27.0, beside


def test_twin_at_a_large_position_equals_the_model():
    """position 2^40 + 7: the phasor index with the indices computed in Python integers (negative and positive offsets)"""
    D, tp = 3, 8
    h = host_chan_design(D, tp)
    iq = _iq(np.random.default_rng(5), 40 * D, "cf64")
    pos = 2 ** 40 + 7
    got = host_chan_process(D, CHANNELS[D], iq, position=pos, taps=h)
    want = cz.model(D, CHANNELS[D], iq, h, position=pos)
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-12 * scale
    assert np.abs(got - cz.model(D, CHANNELS[D], iq, h, position=0)).max() > 1e-3 * scale       # the position matters
    # the largest position there is
    assert host_chan_process(D, CHANNELS[D], iq, position=2 ** 62 - 40, taps=h).shape == (4, 40)


def test_a_retuned_channel_has_a_fresh_channels_tables():
    """what mgpu_chan_retune rebuilds is mgpu_host_chan_tables' row of the new channel: a row depends on its own channel alone"""
    D, h = 4, host_chan_design(4, 8)
    a = host_chan_tables(D, (12345, 0, 1.0), taps=h)
    b = host_chan_tables(D, (-5000, 1, 2.0), taps=h)
    assert np.array_equal(host_chan_tables(D, (12345, 0, 7.0), taps=h), a)         # the gain is not in the taps
    assert not np.array_equal(a, b)
    iq = _iq(np.random.default_rng(6), 30 * D, "cf32")
    both = host_chan_process(D, [(12345, 0, 1.0), (-5000, 1, 2.0)], iq, taps=h)
    assert np.array_equal(both[1], host_chan_process(D, [(-5000, 1, 2.0)], iq, taps=h)[0])


def test_refusals_need_no_device():
    D = 4
    iq = _iq(np.random.default_rng(1), 16 * D, "cf64")
    good = [(0, 0, 1.0)]
    assert host_chan_process(D, good, iq, taps=host_chan_design(D, 2)).shape == (1, 16)
    _refused(lambda: host_chan_design(D, 3))                                            # odd tp
    _refused(lambda: host_chan_design(D, 514))
    _refused(lambda: host_chan_design(65, 2))
    _refused(lambda: host_chan_process(D, good, iq, taps=np.ones(3 * D + 1)))           # odd tp
    _refused(lambda: host_chan_process(D, good, iq, taps=np.ones(2 * D + 2)))           # T is not tp D + 1
    _refused(lambda: host_chan_process(D, good, iq, taps=np.ones(2 * D)))
    _refused(lambda: host_chan_process(D, good, iq[:-1], taps=host_chan_design(D, 2)))  # n_in is no multiple of D
    _refused(lambda: host_chan_process(D, good, iq, struct_size=36))                    # another version of the struct
    R = 48000 * D
    for ch in ((R // 2 - 2944, 0, 1.0), (-R // 2, 0, 1.0), (R // 2, 1, 1.0), (-R // 2 + 2944, 1, 1.0), (0, 2, 1.0), (0, 0, float("nan"))):
        _refused(lambda: host_chan_process(D, [ch], iq))
        _refused(lambda: host_chan_tables(D, ch))
    for ch in ((R // 2 - 2945, 0, 1.0), (-R // 2 + 1, 0, 1.0), (R // 2 - 1, 1, 1.0), (-R // 2 + 2945, 1, 1.0)):      # the band's edge just inside
        assert host_chan_tables(D, ch, taps=host_chan_design(D, 2)).size == 2 * D + 1


def test_create_without_a_device_refuses_bad_arguments_and_reports_the_device():
    """without a context (no device could be opened: tests/test_abi.py) a bad configuration is still MGPU_ERR_ARG, a good one MGPU_ERR_DEVICE"""
    lib = load_library()

    def create(k, chs):
        return create_without_a_context(lib.mgpu_chan_create, C.byref(k), chs)     # and the handle is null

    chs = chan_channels([(0, 0, 1.0), (3000, 1, 1.0)])
    k, _ = chan_config(4, 2)
    assert create(k, chs) == 2                                                                     # MGPU_ERR_DEVICE
    for change in (dict(struct_size=44), dict(D=0), dict(D=65), dict(S=0), dict(audio_centre_hz=0), dict(max_out=-1)):
        k, _ = chan_config(4, 2)
        for name, v in change.items():
            setattr(k, name, v)
        assert create(k, chs) == 1, change                                                         # MGPU_ERR_ARG
    k, keep = chan_config(4, 2, taps=np.ones(14))
    assert create(k, chs) == 1
    k, _ = chan_config(4, 2)
    assert create(k, chan_channels([(0, 0, 1.0), (96000, 0, 1.0)])) == 1
    assert create(k, None) == 1
    assert lib.mgpu_chan_latency(None) < 0 and lib.mgpu_chan_destroy(None) == 1 and lib.mgpu_chan_seek(None, 0) == 1


def test_the_example_compiles_against_the_public_headers(tmp_path):
    """examples/rx_wideband.cpp uses the C-ABI only: it compiles with g++ against include/ (linking needs the library's HIP runtime)"""
    subprocess.run(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                    os.path.join(ROOT, "examples", "rx_wideband.cpp"), "-o", str(tmp_path / "rx_wideband.o")], check=True)

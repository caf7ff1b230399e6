"""GPU tests of the Watterson HF channel (include/mercury_channel.h, csrc/hfchannel.hip): the apply kernels against a numpy composition of
the host definitions, batch independence and determinism, the identity channel inside both self-simulations (bit for bit the AWGN
entry points), and the channel end to end through the real receiver."""
import numpy as np
import pytest

from hf_channel_ref import _numpy_channel
from oraclelib import CARRIER


@pytest.mark.gpu
def test_gpu_apply_matches_numpy_composition():
    from mercury_amd import RxPhy, hf_channel_preset
    rx = RxPhy(8, max_batch=64)
    rng = np.random.default_rng(7)
    ch = hf_channel_preset("moderate")
    ch.freq_offset_hz = 3.0
    x = rng.standard_normal((64, 5000))                                   # five tiles, the last one partial
    got = rx.hf_channel_apply(x, ch, seed=21, realisation0=100, fs=48000.0)
    ref = _numpy_channel(x, ch, 21, 100, 48000.0)
    assert got.dtype == np.float64 and got.shape == x.shape
    assert np.max(np.abs(got - ref)) <= 1e-10 * np.sqrt(np.mean(ref ** 2)), np.max(np.abs(got - ref))
    chp = hf_channel_preset("poor")
    z = rng.standard_normal((64, 3000)) + 1j * rng.standard_normal((64, 3000))
    got = rx.hf_channel_apply(z, chp, seed=22, realisation0=5, fs=12000.0, t0=98765)
    ref = _numpy_channel(z, chp, 22, 5, 12000.0, t0=98765)
    assert got.dtype == np.complex128
    assert np.max(np.abs(got - ref)) <= 1e-10 * np.sqrt(np.mean(np.abs(ref) ** 2)), np.max(np.abs(got - ref))
    rx.close()


@pytest.mark.gpu
def test_gpu_apply_is_batch_independent_and_deterministic():
    from mercury_amd import MgpuError, RxPhy, hf_channel_preset
    rx = RxPhy(8, max_batch=64)
    rng = np.random.default_rng(8)
    ch = hf_channel_preset("poor")
    ch.freq_offset_hz = -1.5
    for x in (rng.standard_normal((64, 2500)), rng.standard_normal((64, 1200)) + 1j * rng.standard_normal((64, 1200))):
        fs = 12000.0 if np.iscomplexobj(x) else 48000.0
        y = rx.hf_channel_apply(x, ch, seed=3, realisation0=40, fs=fs)
        for w in (0, 17, 63):
            one = rx.hf_channel_apply(x[w: w + 1], ch, seed=3, realisation0=40 + w, fs=fs)
            assert np.array_equal(one[0], y[w]), w                        # bit for bit, whatever the batch
        assert np.array_equal(rx.hf_channel_apply(x, ch, seed=3, realisation0=40, fs=fs), y)
        other = rx.hf_channel_apply(x, ch, seed=3, realisation0=41, fs=fs)
        assert not np.any([np.array_equal(other[w], y[w]) for w in range(64)])
        assert not np.array_equal(rx.hf_channel_apply(x, ch, seed=4, realisation0=40, fs=fs)[0], y[0])
        ident = rx.hf_channel_apply(x, "awgn", seed=3, fs=fs)
        assert np.array_equal(ident, x)                                   # the identity channel: the input, bit for bit
    bad = hf_channel_preset("poor")
    bad.delay_ms[1] = 11.0
    with pytest.raises(MgpuError):
        rx.hf_channel_apply(rng.standard_normal((2, 100)), bad, seed=1)
    rx.close()


@pytest.mark.gpu
def test_gpu_apply_dev_equals_host_form():
    import torch
    from mercury_amd import RxPhy, hf_channel_preset
    rx = RxPhy(8, max_batch=8)
    x = np.random.default_rng(9).standard_normal((8, 3000))
    ch = hf_channel_preset("flutter")
    want = rx.hf_channel_apply(x, ch, seed=5, realisation0=2)
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.empty_like(d_in)
    s = torch.cuda.current_stream()
    rx.hf_channel_apply_dev(d_in.data_ptr(), d_out.data_ptr(), 8, 3000, ch, 5, 0, realisation0=2, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)
    rx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [8, 100])
def test_gpu_passband_test_identity_channel_is_bit_identical(cfg):
    from mercury_amd import RxPhy
    pts = [30.0, 2.5] if cfg == 8 else [-5.0, -13.0]
    rx = RxPhy(cfg, max_batch=256)
    a, wa, sa = rx.passband_test_esn0(pts, 256, CARRIER, seed=31, frame0=1000, want_windows=True)
    b, wb, sb = rx.passband_test_esn0(pts, 256, CARRIER, seed=31, frame0=1000, want_windows=True, hf_channel="awgn")
    assert np.array_equal(wa, wb) and np.array_equal(sa, sb)
    for ra, rb in zip(a, b):
        assert ra == rb, (ra, rb)
    rx.close()


@pytest.mark.gpu
def test_gpu_baseband_test_identity_channel_equals_awgn_loop():
    from mercury_amd import RxPhy
    rx = RxPhy(8, max_batch=4096, agc=0, variance_source=0)
    pts = [-3.0, 2.5]
    a = rx.baseband_test_esn0(pts, 4096, seed=41, frame0=7, channel=0)
    b = rx.baseband_test_esn0(pts, 4096, seed=41, frame0=7, hf_channel="awgn")
    assert a == b
    assert a[0]["Error_frames_total"] > 0                               # the points say something
    c = rx.baseband_test_esn0(pts, 4096, seed=41, frame0=7, hf_channel="poor")
    assert c != a
    rx.close()


@pytest.mark.gpu
def test_gpu_frequency_offset_through_the_real_receiver():
    """transmit_byte frames in capture windows at 30 dB (where passband_test_esn0 puts them), +4 Hz through the channel (one identity path),
    receive_byte: every frame decodes and Moose reads +4 Hz (the sign convention of tests/test_receive_byte.py: a receiver carrier df above
    the signal reads -df)."""
    from mercury_amd import HfChannel, RxPhy
    F = 16
    rx = RxPhy(8, max_batch=F)
    rng = np.random.default_rng(10)
    pl = rng.integers(0, 256, (F, rx.payload_stride)).astype(np.uint8)
    pl[:, rx.payload_bytes:] = 0
    audio = rx.transmit_byte(pl, CARRIER)
    n = rx.receive_buffer_samples()
    sigma = np.sqrt(np.mean(audio ** 2)) * 10 ** (-30 / 20)
    wins = rng.standard_normal((F, n)) * sigma
    d = ((rx.preamble_nsymb + 2) * rx.Nofdm + 50) * 4                      # telecom_system.cc:242-249, :292
    wins[:, d: d + audio.shape[1]] += audio
    shifted = rx.hf_channel_apply(wins, HfChannel(((0.0, 0.0, 0.0, 0.0),), freq_offset_hz=4.0), seed=1)
    assert not np.array_equal(shifted, wins)
    out = rx.receive_byte(shifted, CARRIER)
    st = out["stats"]
    assert np.all(st["message_decoded"] == 1), st["message_decoded"]
    assert np.array_equal(out["payload"][:, : rx.payload_bytes], pl[:, : rx.payload_bytes])
    assert np.all(np.abs(st["freq_offset"] - 4.0) < 1.0), st["freq_offset"]
    rx.close()


@pytest.mark.gpu
def test_gpu_flat_rayleigh_costs_frames_at_the_operating_point():
    """Mode 8 at its operating point (mean Es/N0 2.5 dB in the baseband loop, the reference's baseband_test_EsN0 receiver): flat Rayleigh
    fading (one path, 1 Hz) loses frames the identity channel does not."""
    from mercury_amd import HfChannel, RxPhy
    rx = RxPhy(8, max_batch=1024, agc=0, variance_source=0)
    flat = HfChannel(((0.0, 0.0, 1.0, 0.0),))
    awgn = rx.baseband_test_esn0([2.5], 1024, seed=51, frame0=0, hf_channel="awgn")[0]
    ray = rx.baseband_test_esn0([2.5], 1024, seed=51, frame0=0, hf_channel=flat)[0]
    assert ray["FER"] > awgn["FER"], (ray["FER"], awgn["FER"])
    rx.close()


@pytest.mark.gpu
def test_gpu_good_channel_decodes_at_30_db_through_receive_byte():
    """CCIR 520 GOOD at 30 dB through the whole receiver (passband loop at the reference's BER_PLOT_passband output power of 1 W, the
    convention in which Es/N0 is the signal's own; at the 0.1 W default the noise stands 10 dB higher)."""
    from mercury_amd import RxPhy
    rx = RxPhy(8, max_batch=1024)
    good = rx.passband_test_esn0([30.0], 1024, CARRIER, seed=52, frame0=0, output_power_watt=1.0, hf_channel="good")[0]
    assert good["FER"] <= 0.25, good
    rx.close()

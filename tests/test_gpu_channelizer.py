"""The wideband channeliser on the GPU (include/mercury_channelizer.h, mercury_amd.Channelizer): every output against the normative host
twin, bit for bit (the uint64 view), at the shapes where the kernel's tiling, its polyphase LDS image and its tap blocking can go wrong;
every format from host and device memory; chunk invariance; positions; retuning; and three links end to end through the receive loop.

The FIR kernel's output tile is TILE = 128 outputs per workgroup (64 lanes of 2 consecutive outputs, D <= 32), four channels per
workgroup; at D = 16 the default filter's 5137 steps go through the LDS image in blocks of 1024 (tests/test_channelizer_host.py pins
the twin itself)."""
import ctypes as C
import functools

import numpy as np
import pytest

import channelizer_ref as cz
from band_links import FIRST_STARTS, ThreeLinks, bits as _bits, channels as _channels, iq as _iq, last_error, other_rx, rx as _rx, \
    taps as _taps, torch as _torch
from mercury_amd import (Channelizer, MgpuError, Resampler, RxCapture, Synthesizer, chan_channels, chan_config, host_chan_process,
                         host_resamp_process, host_synth_process, resamp_config, synth_config)
from oraclelib import CARRIER

pytestmark = pytest.mark.gpu
TILE = 128


@pytest.mark.parametrize("tp", [2, 320])
@pytest.mark.parametrize("D", [1, 3, 4, 16])
def test_outputs_equal_the_twin_at_the_tile_edges(D, tp):
    """S in {1, 2, 5} (one workgroup's channels not full, full with the next one's partly used) x n_out in {1, TILE - 1, TILE, TILE + 1}
    (a lone output, a tile not full, full, and a second one with one output): tp = 2 is the shortest filter there is (T = 2 D + 1, all
    steps but one are edge steps), tp = 320 the default (at D = 16: six tap blocks)"""
    rx, h = _rx(), _taps(D, tp)
    rng = np.random.default_rng(1000 * D + tp)
    for S in (1, 2, 5):
        chs = _channels(rng, D, S)
        ch = Channelizer(rx, D, chs, taps=h)
        assert ch.latency == tp // 2
        for n_out in (1, TILE - 1, TILE, TILE + 1):
            iq = _iq(rng, n_out * D, "cf64")
            ch.seek(0)
            got = ch.process(iq)
            want = host_chan_process(D, chs, iq, taps=h)
            assert got.shape == want.shape == (S, n_out)
            assert np.abs(want).max() > 0
            assert np.array_equal(_bits(got), _bits(want)), (S, n_out, np.abs(got - want).max())
        ch.close()


@pytest.mark.parametrize("D,tp", [(33, 2), (64, 2), (64, 8)])
def test_outputs_equal_the_twin_above_d32(D, tp):
    """D > 32 runs the kernel's other form: one output per lane, a tile of 64 outputs, an LDS image of up to 69 KiB (more than a
    kernel gets without asking); at D = 64, tp = 8 the 513 steps go through it in three blocks of 256"""
    rx, h = _rx(), _taps(D, tp)
    rng = np.random.default_rng(3000 * D + tp)
    for S in (1, 5):
        chs = _channels(rng, D, S)
        ch = Channelizer(rx, D, chs, taps=h)
        for n_out in (1, 63, 64, 65):
            iq = _iq(rng, n_out * D, "cf32")
            ch.seek(0)
            got = ch.process(iq)
            want = host_chan_process(D, chs, iq, taps=h)
            assert np.array_equal(_bits(got), _bits(want)), (S, n_out, np.abs(got - want).max())
        ch.close()


@pytest.mark.parametrize("fmt", ["cs16", "cf32", "cf64"])
def test_every_format_from_host_and_device_memory(fmt):
    """CS16, CF32 and CF64 through process() from host memory and from a device tensor, and through process_dev (device in and out)"""
    torch = _torch()
    rx, D, S, n_out = _rx(), 4, 3, 2 * TILE + 37
    h = _taps(D, 8)
    rng = np.random.default_rng(40 + len(fmt) + ord(fmt[2]))
    chs = _channels(rng, D, S)
    iq = _iq(rng, n_out * D, fmt)
    want = host_chan_process(D, chs, iq, taps=h)
    ch = Channelizer(rx, D, chs, taps=h)
    d_iq = torch.from_numpy(iq).cuda()
    ch.seek(0)
    assert np.array_equal(_bits(ch.process(iq)), _bits(want))
    ch.seek(0)
    assert np.array_equal(_bits(ch.process(d_iq)), _bits(want))
    ch.seek(0)
    d_out = torch.zeros((S, n_out), dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    ch.process(d_iq, out=d_out, stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(want))
    ch.seek(0)
    ch.process(d_iq, out=d_out.zero_())                  # the context's stream
    rx.lib.mgpu_synchronize(rx.h, None)
    assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(want))
    ch.close()


@pytest.mark.parametrize("D,tp", [(4, 320), (16, 320), (3, 2)])
def test_chunking_does_not_change_an_output(D, tp):
    """one call of N D inputs equals the same stream cut into chunks of D, 7 D, T - 1 rounded down to a multiple of D, and 1088 D inputs
    (the first three shorter than the history of T - 1), in turn"""
    rx, h = _rx(), _taps(D, tp)
    rng = np.random.default_rng(77 + D)
    S = 2
    chs = _channels(rng, D, S)
    T = h.size
    cuts = [1, 7, (T - 1) // D, 1088]
    N = 2 * sum(cuts) + 5
    iq = _iq(rng, N * D, "cf32")
    ch = Channelizer(rx, D, chs, taps=h)
    whole = ch.process(iq)
    assert np.array_equal(_bits(whole), _bits(host_chan_process(D, chs, iq, taps=h)))
    ch.seek(0)
    parts, at, i = [], 0, 0
    while at < N:
        n = min(cuts[i % len(cuts)], N - at)
        parts.append(ch.process(iq[at * D: (at + n) * D]))
        at, i = at + n, i + 1
    assert np.array_equal(_bits(np.concatenate(parts, axis=1)), _bits(whole))
    # a bad n_in is refused and changes nothing: the next chunk continues the stream
    ch.seek(0)
    first = ch.process(iq[: 7 * D])
    if D > 1:
        with pytest.raises(MgpuError) as e:
            ch.process(iq[7 * D: 9 * D - 1])
        assert e.value.code == 1
    second = ch.process(iq[7 * D: 20 * D])
    assert np.array_equal(_bits(np.concatenate([first, second], axis=1)), _bits(whole[:, :20]))
    ch.close()


def test_position_and_retune():
    """after seek(2^40 + 7) the output is the twin's at that position (the history is zeros again); after retune of one channel that
    channel is a fresh channeliser's on the same stream from the next call on, and the other channels do not move"""
    rx, D = _rx(), 4
    h = _taps(D, 320)
    rng = np.random.default_rng(9)
    chs = [(-30000, 0, 1.0), (-27000, 0, 0.7), (12345, 1, 1.3)]
    new = (55555, 1, 0.9)
    n1, n2 = 300, 500
    iq = _iq(rng, (n1 + n2) * D, "cf32")
    pos = 2 ** 40 + 7
    ch = Channelizer(rx, D, chs, taps=h)
    ch.process(iq[: 50 * D])                                            # a history to forget
    ch.seek(pos)
    a1 = ch.process(iq[: n1 * D])
    ch.retune(1, new)
    a2 = ch.process(iq[n1 * D:])
    old = host_chan_process(D, chs, iq, position=pos, taps=h)
    assert np.array_equal(_bits(a1), _bits(old[:, :n1]))
    assert not np.array_equal(_bits(a1), _bits(host_chan_process(D, chs, iq[: n1 * D], taps=h)))      # the position matters
    chs2 = [chs[0], new, chs[2]]
    want = host_chan_process(D, chs2, iq, position=pos, taps=h)
    assert np.array_equal(_bits(a2[1]), _bits(want[1, n1:]))
    assert np.array_equal(_bits(a2[[0, 2]]), _bits(old[[0, 2], n1:]))
    fresh = Channelizer(rx, D, chs2, taps=h)
    fresh.seek(pos)
    fresh.process(iq[: n1 * D])
    assert np.array_equal(_bits(fresh.process(iq[n1 * D:])), _bits(a2))
    with pytest.raises(MgpuError) as e:
        ch.retune(1, (96000, 0, 1.0))                                   # the band leaves (-R/2, R/2)
    assert e.value.code == 1
    with pytest.raises(MgpuError):
        ch.retune(3, new)
    ch.close(), fresh.close()


L_DEFAULT = 160                 # the default design's latency: tp / 2


OFFSETS, GAINS = (-30000, -27000, 12345), (1.0, 10 ** (30 / 20.0), 1.0)
HOPS_PER_CALL = 16
LINKS = ThreeLinks(seed=2024, tail=L_DEFAULT, hops_per_call=HOPS_PER_CALL)


def _starts_the_loop_delivers():
    """The channeliser's latency moves a frame by L = 160 samples on the loop's hop grid (band_links.ThreeLinks.starts_the_loop_delivers):
    the starts at which the loop delivers the transmitted audio delayed by L"""
    return LINKS.starts_the_loop_delivers((L_DEFAULT,))


@functools.lru_cache(maxsize=None)
def _three_links(starts):
    """Mode 8, D = 4: three links' frames (transmit_byte, three payloads), each at its own start sample (none a multiple of P) in silence,
    synthesised at offsets -30000, -27000 and +12345 Hz, the second 30 dB stronger than its neighbour 3 kHz away; no noise, complex64 IQ;
    16 hops per call until every frame has passed. -> the payloads, the events of run_wideband, of RxCapture.run on the twin's output
    and of RxCapture.run on the transmitted audio itself delayed by the latency (no channeliser)"""
    rx, D, S = _rx(), 4, 3
    payloads, _ = LINKS.frames()
    audio = LINKS.audio(starts)
    iq = cz.synthesise(audio, D, OFFSETS, None, GAINS).astype(np.complex64)
    chs = [(OFFSETS[s], 0, 1.0 / GAINS[s]) for s in range(S)]
    twin = host_chan_process(D, chs, iq)
    for s in range(S):
        print("link %d: audio error against the direct feed %.1f dB" % (s, cz.error_db(twin[s], audio[s], L_DEFAULT, 2000)))
    chan = Channelizer(rx, D, chs)
    caps = [RxCapture(rx, S, CARRIER, max_hops=HOPS_PER_CALL) for _ in range(3)]
    ev = [LINKS.run_in_calls(iq, lambda part: caps[0].run_wideband(chan, part), D=D), LINKS.run_in_calls(twin, caps[1].run),
          LINKS.run_in_calls(LINKS.audio(starts, L_DEFAULT), caps[2].run)]
    for k, name in enumerate(("run_wideband", "run on the twin's output", "run on the audio delayed by L")):
        print("%s: (capture, hop, own payload)" % name, [(e[0], e[1], e[3] == payloads[e[0]].tobytes()) for e in ev[k]])
    part = iq[: HOPS_PER_CALL * caps[0].P * D]
    with pytest.raises(MgpuError) as e:
        RxCapture(rx, 2, CARRIER).run_wideband(chan, part)                                     # the S of both objects must agree
    assert e.value.code == 1
    assert last_error(rx) == "mgpu_capture_run_wideband: the capture and the channeliser must have the same S"
    with pytest.raises(MgpuError) as e:
        RxCapture(other_rx(), S, CARRIER).run_wideband(chan, part)                             # and so must their contexts
    assert e.value.code == 1
    assert last_error(rx) == "mgpu_capture_run_wideband: the capture and the channeliser must belong to one context"
    chan.seek(0)                                                                               # a refused call ran nothing: the stream is whole
    assert np.array_equal(_bits(chan.process(iq[: 8 * D])), _bits(host_chan_process(D, chs, iq[: 8 * D])))
    chan.close()
    for c in caps:
        c.close()
    return payloads, ev[0], ev[1], ev[2]


def test_three_links_end_to_end_through_the_receive_loop():
    """Every link's payload is delivered on its own capture, no capture reports a CRC-good payload that is not its own link's, and
    run_wideband returns exactly the events and payloads RxCapture.run returns on the twin's output for the same IQ. The frames' start
    samples are those of _starts_the_loop_delivers: the second link 30 dB stronger than its neighbour 3 kHz away, no noise, complex64 IQ
    and the hops are as they were."""
    payloads, got, want, _ = _three_links(_starts_the_loop_delivers())
    assert got == want
    for e in got:
        crc = np.frombuffer(e[2], np.int32, 4)[1]               # RECEIVE_STATS_DTYPE: iterations_done, crc, ...
        assert not crc or e[3] == payloads[e[0]].tobytes(), "capture %d reports a payload that is not its link's" % e[0]
    for s in range(len(payloads)):
        assert any(e[0] == s and e[3] == payloads[s].tobytes() for e in got), "link %d was not delivered" % s


def test_wideband_delivers_what_the_loop_delivers_on_the_audio_delayed_by_the_latency():
    """At FIRST_STARTS the captures behind the channeliser decode the same links at the same hops as captures fed the transmitted audio
    itself, delayed by L samples: to the receive loop the channeliser is a delay of L and nothing else.

    Measured on the MI355X: both deliver links 0 and 2 (hops 34 and 41) and neither delivers link 1, the strong one, whose frame
    starts at 7 P + 17. The audio its capture sees is within -44.2 dB of the transmitted audio delayed by 160 samples (links 0 / 2:
    -18.4 dB beside the neighbour 30 dB stronger, -44.5 dB); undelayed the loop delivers all three (hops 34, 36, 40), and delayed it
    decodes link 2 at hop 41 with 3 iterations and SNR -3.2 dB against 0 iterations and 11.2 dB. Link 1 alone in the IQ, equal gains,
    complex128 IQ and 1e-4 of noise change nothing; 9 P + 500 behaves as 7 P + 17. The loss is the loop's synchroniser on a noise-free
    frame at 7 P + 177 on its hop grid, not the channeliser's latency or phase."""
    payloads, got, _, direct = _three_links(FIRST_STARTS)
    assert [(e[0], e[1], e[3]) for e in got] == [(e[0], e[1], e[3]) for e in direct]
    assert len(LINKS.delivered(got)) >= 2


def test_create_refusals_keep_their_words_and_the_smallest_stages_equal_their_twins():
    """The three stream stages share how a handle is made: a refused configuration gives MGPU_ERR_ARG, a null handle and
    "<function>: <reason>" as the context's last error, before any device work; the literals are the library's. Then one create / process /
    close of each stage at the smallest shape there is (channeliser and synthesiser D = 1, tp = 2, S = 1; resampler 44100 -> 48000,
    S = 1) equals its twin bit for bit."""
    rx, lib = _rx(), _rx().lib
    one = chan_channels([(0, 0, 1.0)])

    def refused(create, *args):
        h = C.c_void_p(1)
        assert create(rx.h, *args, C.byref(h)) == 1 and not h.value
        return last_error(rx)

    assert refused(lib.mgpu_chan_create, C.byref(chan_config(65, 1)[0]), one) == "mgpu_chan_create: D must be 1..64"
    assert refused(lib.mgpu_chan_create, C.byref(chan_config(4, 1)[0]), None) == "mgpu_chan_create: no channels"
    assert refused(lib.mgpu_chan_create, C.byref(chan_config(4, 1)[0]), chan_channels([(96000, 0, 1.0)])) \
        == "mgpu_chan_create: the channel's band leaves (-R/2, R/2)"
    assert refused(lib.mgpu_synth_create, C.byref(synth_config(4, 1, max_in=-1)[0]), one) == "mgpu_synth_create: max_in * D must be 0..2^30"
    assert refused(lib.mgpu_resamp_create, C.byref(resamp_config(48000, 48001)[0])) \
        == "mgpu_resamp_create: rates must be >= 1 with L <= 640, M <= 640 and M <= 16 L"
    rng = np.random.default_rng(31)
    h, plan = _taps(1, 2), [(-5000, 1, 1.7)]
    iq = _iq(rng, 64, "cf64")
    ch = Channelizer(rx, 1, plan, taps=h)
    assert np.array_equal(_bits(ch.process(iq)), _bits(host_chan_process(1, plan, iq, taps=h)))
    ch.close()
    audio = rng.standard_normal((1, 64))
    sy = Synthesizer(rx, 1, plan, taps=h)
    assert sy.process(audio).tobytes() == host_synth_process(1, plan, audio, taps=h).tobytes()
    sy.close()
    x = rng.standard_normal((1, 100))
    rs = Resampler(rx, 44100, 48000)
    assert np.array_equal(_bits(rs.process(x)), _bits(host_resamp_process(44100, 48000, x)))
    rs.close()


def test_create_use_destroy_gives_the_memory_back():
    """create / process / retune / run_wideband / destroy cycles (line buffers, tables, staging, the wideband workspace) leave the
    device's free memory where it was"""
    import gc
    torch = _torch()

    def free_hbm():
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info()[0]

    rx, D, S = _rx(), 16, 64
    P = rx.Nofdm * 4
    rng = np.random.default_rng(6)
    chs = _channels(rng, D, S)
    iq = _iq(rng, 2 * P * D, "cs16")

    def cycle():
        ch = Channelizer(rx, D, chs)
        cap = RxCapture(rx, S, CARRIER)
        ch.process(iq)
        ch.retune(5, chs[6])
        cap.run_wideband(ch, iq)
        return ch, cap

    for o in cycle():
        o.close()                                         # the context's receive_byte workspace is sized on first use
    first = free_hbm()
    for c in range(4):
        ch, cap = cycle()
        in_use = first - free_hbm()
        ch.close(), cap.close()
        # two line buffers of (T - 1 + max_out D) complex doubles, the taps [S][T], the workspace [S][max_out]
        assert in_use >= 2 * (5120 + 16 * 1088 * D) * 16 + S * 5121 * 16 + S * 16 * 1088 * 8, in_use
        after = free_hbm()
        assert abs(after - first) < 64 << 20, (c, first, after)

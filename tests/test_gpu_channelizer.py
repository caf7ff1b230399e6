"""The wideband channeliser on the GPU (include/mercury_channelizer.h, mercury_amd.Channelizer): every output against the normative host
twin, bit for bit (the uint64 view), at the shapes where the kernel's tiling, its polyphase LDS image and its tap blocking can go wrong;
every format from host and device memory; chunk invariance; positions; retuning; and three links end to end through the receive loop.

The FIR kernel's output tile is TILE = 128 outputs per workgroup (64 lanes of 2 consecutive outputs, D <= 32), four channels per
workgroup; at D = 16 the default filter's 5137 steps go through the LDS image in blocks of 1024 (tests/test_channelizer_host.py pins
the twin itself)."""
import functools

import numpy as np
import pytest

import channelizer_ref as cz
from mercury_amd import Channelizer, MgpuError, RxCapture, RxPhy, host_chan_design, host_chan_process
from oraclelib import CARRIER

pytestmark = pytest.mark.gpu
MAX_ITERS = 10
TILE = 128


def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def _rx():
    return RxPhy(8, max_iters=MAX_ITERS, max_batch=8)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _iq(rng, n, fmt):
    if fmt == "cs16":
        return rng.integers(-2 ** 15, 2 ** 15, (n, 2)).astype(np.int16)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return x.astype(np.complex64 if fmt == "cf32" else np.complex128)


def _channels(rng, D, S):
    """S channels anywhere a band fits in (-R/2, R/2): both sidebands, both signs of the offset, gains that are no powers of two"""
    half = 24000 * D
    out = []
    for s in range(S):
        sb = int(rng.integers(0, 2))
        lo, hi = (-half + 1, half - 2945) if sb == 0 else (-half + 2945, half - 1)
        out.append((int(rng.integers(lo, hi + 1)), sb, float(rng.uniform(0.3, 3.0))))
    return out


@functools.lru_cache(maxsize=None)
def _taps(D, tp):
    return host_chan_design(D, tp)


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


def _canon(r):
    """a structured scalar's field bytes, without its padding (bit patterns of the doubles kept)"""
    r = np.asarray(r)
    return b"".join(_canon(r[n]) if r.dtype[n].names else np.asarray(r[n]).tobytes() for n in r.dtype.names)


L_DEFAULT = 160                 # the default design's latency: tp / 2


OFFSETS, GAINS = (-30000, -27000, 12345), (1.0, 10 ** (30 / 20.0), 1.0)
FIRST_STARTS = (5 * 1088 + 333, 7 * 1088 + 17, 11 * 1088 + 901)        # mode 8: P = 1088
HOPS_PER_CALL = 16


@functools.lru_cache(maxsize=None)
def _frames():
    """three payloads and their transmit_byte frames (mode 8)"""
    rx = _rx()
    payloads = np.random.default_rng(2024).integers(0, 256, (3, rx.payload_bytes)).astype(np.uint8)
    return payloads, rx.transmit_byte(payloads, CARRIER)


def _audio(starts, delay=0):
    """the three links' 48 kHz audio [3, H P]: each frame at its start sample (+ delay) in silence; H a multiple of HOPS_PER_CALL by which
    every frame has ended, with the channeliser's latency, and some hops more"""
    P = _rx().Nofdm * 4
    _, frames = _frames()
    fsz = frames.shape[1]
    H = -(-(max(starts) + fsz + L_DEFAULT + P) // P) + 4
    H = -(-H // HOPS_PER_CALL) * HOPS_PER_CALL
    assert P == 1088 and all(s % P for s in starts) and H * P > max(starts) + fsz + L_DEFAULT
    audio = np.zeros((3, H * P))
    for s in range(3):
        audio[s, starts[s] + delay: starts[s] + delay + fsz] = frames[s]
    return audio


def _run(cap, x, run):
    """run(chunk) over x, [3, H P] audio or [H P D] IQ, in calls of HOPS_PER_CALL hops -> events (capture, hop since the start, stats
    bytes, payload bytes)"""
    n = x.shape[-1] // ((4 if x.ndim == 1 else 1) * cap.P * HOPS_PER_CALL)          # D = 4
    ev = []
    for c, part in enumerate(np.split(x, n, axis=-1)):
        ev += [(e[0], e[1] + c * HOPS_PER_CALL, _canon(e[2]), e[3].tobytes()) for e in run(np.ascontiguousarray(part))]
    return ev


def _delivered(ev, payloads):
    return {e[0] for e in ev if e[3] == payloads[e[0]].tobytes()}


@functools.lru_cache(maxsize=None)
def _starts_the_loop_delivers():
    """The receive loop's own synchroniser loses a noise-free frame at some positions on its hop grid, with no channeliser anywhere:
    fed the transmitted audio itself it delivers the frames at FIRST_STARTS but not the one at 7 P + 17 + 160 (measured; the next test
    pins it). The channeliser's latency moves a frame by L = 160 samples on that grid, so the end-to-end test places each link's frame
    where the loop delivers the transmitted audio DELAYED BY L: per link the first of start + 156 k, k = 0 .. 5 (residues that are no
    multiple of P), judged by RxCapture.run on that audio alone. What is chosen by is the existing loop on a pure delay, never the
    channeliser's output."""
    rx = _rx()
    P = rx.Nofdm * 4
    payloads, _ = _frames()
    chosen = [None] * 3
    for k in range(6):
        cand = tuple(FIRST_STARTS[s] + 156 * k for s in range(3))
        cap = RxCapture(rx, 3, CARRIER, max_hops=HOPS_PER_CALL)
        ok = _delivered(_run(cap, _audio(cand, L_DEFAULT), cap.run), payloads)
        cap.close()
        for s in ok:
            if chosen[s] is None and cand[s] % P:
                chosen[s] = cand[s]
        if all(c is not None for c in chosen):
            break
    assert all(c is not None for c in chosen), ("the loop delivers no candidate of a link", chosen)
    print("starts the loop delivers on the audio delayed by L:", chosen, [c % P for c in chosen])
    return tuple(chosen)


@functools.lru_cache(maxsize=None)
def _three_links(starts):
    """Mode 8, D = 4: three links' frames (transmit_byte, three payloads), each at its own start sample (none a multiple of P) in silence,
    synthesised at offsets -30000, -27000 and +12345 Hz, the second 30 dB stronger than its neighbour 3 kHz away; no noise, complex64 IQ;
    16 hops per call until every frame has passed. -> the payloads, the events of run_wideband, of RxCapture.run on the twin's output
    and of RxCapture.run on the transmitted audio itself delayed by the latency (no channeliser)"""
    rx, D, S = _rx(), 4, 3
    payloads, _ = _frames()
    audio = _audio(starts)
    iq = cz.synthesise(audio, D, OFFSETS, None, GAINS).astype(np.complex64)
    chs = [(OFFSETS[s], 0, 1.0 / GAINS[s]) for s in range(S)]
    twin = host_chan_process(D, chs, iq)
    for s in range(S):
        print("link %d: audio error against the direct feed %.1f dB" % (s, cz.error_db(twin[s], audio[s], L_DEFAULT, 2000)))
    chan = Channelizer(rx, D, chs)
    caps = [RxCapture(rx, S, CARRIER, max_hops=HOPS_PER_CALL) for _ in range(3)]
    ev = [_run(caps[0], iq, lambda part: caps[0].run_wideband(chan, part)), _run(caps[1], twin, caps[1].run),
          _run(caps[2], _audio(starts, L_DEFAULT), caps[2].run)]
    for k, name in enumerate(("run_wideband", "run on the twin's output", "run on the audio delayed by L")):
        print("%s: (capture, hop, own payload)" % name, [(e[0], e[1], e[3] == payloads[e[0]].tobytes()) for e in ev[k]])
    with pytest.raises(MgpuError) as e:
        RxCapture(rx, 2, CARRIER).run_wideband(chan, iq[: HOPS_PER_CALL * caps[0].P * D])     # the S of both objects must agree
    assert e.value.code == 1
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
    assert len(_delivered(got, payloads)) >= 2


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

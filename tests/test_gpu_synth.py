"""The wideband synthesiser on the GPU (include/ext/mercury_synth.h, mercury_amd.Synthesizer): every IQ sample against the normative host
twin, bit for bit, at the shapes where the kernel's tiling, its phase groups and its channel rounds can go wrong; every format from host
and device memory; chunk invariance; positions; retuning; three links end to end through the channeliser and the receive loop; memory.

The kernel's tile is TILE = 64 audio positions per workgroup (one per lane) and a group of 4 phases (D = 1: 1, D = 2: 2), so D = 3 and
D = 33 leave a group partly used and D = 64 has 16 groups; ROUND = 4 channels are in flight per workgroup, so S = 5 and 9 take two and
three rounds, the last with one channel."""
import numpy as np
import pytest

from band_links import ThreeLinks, rx as _rx, taps as _taps, torch as _torch
from mercury_amd import Channelizer, MgpuError, RxCapture, Synthesizer, host_synth_process
from oraclelib import CARRIER

pytestmark = pytest.mark.gpu
TILE = 64
ROUND = 4
POSITION = 2 ** 40 + 7


def _channels(rng, D, S):
    """S channels anywhere a band fits in (-R/2, R/2): USB and LSB mixed, a negative offset, gains that are no powers of two, and from
    S = 2 on one channel with gain 0"""
    half = 24000 * D
    out = []
    for s in range(S):
        sb = (s + 1) % 2 if s < 2 else int(rng.integers(0, 2))
        lo, hi = (-half + 1, half - 2945) if sb == 0 else (-half + 2945, half - 1)
        off = int(rng.integers(lo, 0)) if s == 0 else int(rng.integers(lo, hi + 1))
        out.append((off, sb, 0.0 if s == 1 else float(rng.uniform(0.3, 3.0))))
    return out


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _check_tile_edges(D, tp, Ss, n_ins, seed):
    rx, h = _rx(), _taps(D, tp)
    rng = np.random.default_rng(seed)
    for S in Ss:
        chs = _channels(rng, D, S)
        sy = Synthesizer(rx, D, chs, taps=h)
        assert sy.latency == tp // 2 and sy.tile == TILE
        for n_in in n_ins:
            audio = rng.standard_normal((S, n_in))
            sy.seek(0)
            got = sy.process(audio)
            want = host_synth_process(D, chs, audio, taps=h)
            assert got.shape == (n_in * D,) and np.abs(want).max() > 0
            assert _same(got, want), (S, n_in, np.abs(got - want).max())
        sy.close()


@pytest.mark.parametrize("tp", [2, 320])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 16])
def test_outputs_equal_the_twin_at_the_tile_edges(D, tp):
    """S in {1, 2, 5, 9} (a round not full, and two and three rounds with one channel in the last) x n_in in {1, TILE - 1, TILE, TILE + 1}
    (a lone position, a tile not full, full, and a second one with one position): tp = 2 is the shortest filter there is, tp = 320
    the default. D = 1 and 2 run the one- and two-phase forms, D = 3 a group of four with one phase unused, D = 16 four groups."""
    Ss = (1, 2, ROUND + 1, 2 * ROUND + 1) if D == 4 else (1, 2, ROUND + 1)
    _check_tile_edges(D, tp, Ss, (1, TILE - 1, TILE, TILE + 1), 1000 * D + tp)


@pytest.mark.parametrize("D,tp", [(33, 2), (33, 8), (64, 2), (64, 8)])
def test_outputs_equal_the_twin_above_d32(D, tp):
    """D = 33: nine phase groups, the last with one phase; D = 64: sixteen"""
    _check_tile_edges(D, tp, (1, ROUND + 1), (1, TILE - 1, TILE, TILE + 1), 3000 * D + tp)


def test_outputs_equal_the_twin_at_d64_and_the_default_filter():
    """D = 64, tp = 320 (20481 taps), one tile: the 64 phases are split over sixteen workgroups, never a sum"""
    _check_tile_edges(64, 320, (5,), (TILE,), 64320)


@pytest.mark.parametrize("D,tp", [(4, 320), (16, 320), (3, 2)])
def test_chunking_does_not_change_an_output(D, tp):
    """one call of N samples equals the same stream cut into chunks of 1, 7, tp - 1, tp + 1 and max_in samples, in turn (the first three
    shorter than the history of tp); a bad n_in is refused and changes nothing"""
    rx, h = _rx(), _taps(D, tp)
    rng = np.random.default_rng(77 + D)
    S, max_in = 3, max(2 * TILE + 9, tp + 1)
    chs = _channels(rng, D, S)
    cuts = [1, 7, tp - 1, tp + 1, max_in]
    N = 2 * sum(cuts) + 5
    audio = rng.standard_normal((S, N))
    want = host_synth_process(D, chs, audio, position=POSITION, taps=h)
    whole = Synthesizer(rx, D, chs, taps=h, max_in=N)
    whole.seek(POSITION)
    assert _same(whole.process(audio), want)
    whole.close()
    sy = Synthesizer(rx, D, chs, taps=h, max_in=max_in)
    assert sy.max_in == max_in
    sy.seek(POSITION)
    parts, at, i = [], 0, 0
    while at < N:
        n = min(cuts[i % len(cuts)], N - at)
        parts.append(sy.process(audio[:, at: at + n]))
        at, i = at + n, i + 1
    assert _same(np.concatenate(parts), want)
    assert sy.status().position == POSITION + N
    sy.seek(POSITION)
    first = sy.process(audio[:, :7])
    for bad in (audio[:, 7:7], audio[:, 7: 7 + sy.max_in + 1]):
        with pytest.raises(MgpuError) as e:
            sy.process(bad)
        assert e.value.code == 1
    assert sy.status().position == POSITION + 7
    second = sy.process(audio[:, 7:20])
    assert _same(np.concatenate([first, second]), want[: 20 * D])
    sy.close()


def _scaled(rng, S, n):
    """audio whose IQ is mostly inside CS16's range and clamps now and then (the twin: 65 of the 2640 components of the test below)"""
    return rng.standard_normal((S, n)) * 0.3


@pytest.mark.parametrize("fmt", ["cs16", "cf32", "cf64"])
def test_every_format_from_host_and_device_memory(fmt):
    """CF64, CF32 and CS16 through process() from host memory and from a device tensor whose rows are further apart than n_in, and
    through process_dev (device in and out) on a stream of the caller's and on the context's; the CS16 clamp count equals the twin's"""
    torch = _torch()
    rx, D, S, n_in = _rx(), 4, 3, 2 * TILE + 37
    h = _taps(D, 8)
    rng = np.random.default_rng(40 + len(fmt) + ord(fmt[2]))
    chs = [(-30000, 0, 1.0), (-27000, 1, 2.5), (12345, 1, 0.7)]
    audio = _scaled(rng, S, n_in)
    want, clamped = host_synth_process(D, chs, audio, fmt=fmt, taps=h, want_clamped=True)
    assert (clamped > 0) == (fmt == "cs16")
    sy = Synthesizer(rx, D, chs, taps=h)
    wide = torch.zeros((S, n_in + 11), dtype=torch.float64, device="cuda")
    wide[:, :n_in] = torch.from_numpy(audio).cuda()
    d_audio = wide[:, :n_in]                                            # row stride n_in + 11
    torch.cuda.synchronize()                                            # the library works on its own stream
    assert _same(sy.process(audio, fmt=fmt), want)
    assert sy.status().clamped == clamped
    sy.seek(0)
    assert _same(sy.process(d_audio, fmt=fmt), want)
    assert sy.status().clamped == clamped
    sy.seek(0)
    d_out = torch.from_numpy(np.zeros_like(want)).cuda()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    sy.process(d_audio, fmt=fmt, out=d_out, stream=stream.cuda_stream)
    stream.synchronize()
    assert _same(d_out.cpu().numpy(), want)
    d_out.zero_()
    torch.cuda.synchronize()
    sy.process(d_audio, fmt=fmt, out=d_out)                             # the context's stream; the stream goes on: the count adds up
    twice, clamped2 = host_synth_process(D, chs, np.concatenate([audio, audio], axis=1), fmt=fmt, taps=h, want_clamped=True)
    assert sy.status().clamped == clamped2
    assert _same(d_out.cpu().numpy(), twice[n_in * D:])
    sy.seek(0)
    assert sy.status().clamped == 0 and sy.status().position == 0
    with pytest.raises(MgpuError):
        sy.process(d_audio, fmt="cf64" if fmt != "cf64" else "cf32", out=d_out)          # the tensor is not the format asked for
    sy.close()


def test_position_and_retune():
    """after seek(2^40 + 7) the output is the twin's at that position (the history is zeros again); after retune of one channel the
    stream goes on as the twin's with the new plan on the same audio: the retuned channel is a fresh synthesiser's with the same history,
    and the other channels' contribution does not move"""
    rx, D = _rx(), 4
    h = _taps(D, 320)
    rng = np.random.default_rng(9)
    chs = [(-30000, 0, 1.0), (-27000, 0, 0.7), (12345, 1, 1.3)]
    new = (55555, 1, 0.9)
    n1, n2 = 300, 500
    audio = rng.standard_normal((3, n1 + n2))
    sy = Synthesizer(rx, D, chs, taps=h)
    sy.process(audio[:, :50])                                           # a history to forget
    sy.seek(POSITION)
    a1 = sy.process(audio[:, :n1])
    sy.retune(1, new)
    a2 = sy.process(audio[:, n1:])
    old = host_synth_process(D, chs, audio, position=POSITION, taps=h)
    assert _same(a1, old[: n1 * D])
    assert not _same(a1, host_synth_process(D, chs, audio[:, :n1], taps=h))             # the position matters
    chs2 = [chs[0], new, chs[2]]
    assert _same(a2, host_synth_process(D, chs2, audio, position=POSITION, taps=h)[n1 * D:])
    # the other channels alone: what they add is the same under either plan
    others = [chs[0], (chs[1][0], chs[1][1], 0.0), chs[2]]
    alone = Synthesizer(rx, D, others, taps=h)
    alone.seek(POSITION)
    alone.process(audio[:, :n1])
    alone.retune(1, (new[0], new[1], 0.0))
    assert _same(alone.process(audio[:, n1:]), host_synth_process(D, others, audio, position=POSITION, taps=h)[n1 * D:])
    with pytest.raises(MgpuError) as e:
        sy.retune(1, (96000, 0, 1.0))                                   # the band leaves (-R/2, R/2)
    assert e.value.code == 1
    with pytest.raises(MgpuError):
        sy.retune(3, new)
    sy.close(), alone.close()


TP_DEFAULT = 320                # synthesiser -> channeliser with the default design: a delay of tp samples
OFFSETS, SIDEBANDS, GAINS = (-30000, -27000, 12345), (0, 0, 1), (1.0, 10 ** (30 / 20.0), 1.0)


HOPS_PER_CALL = 16
LINKS = ThreeLinks(seed=2024, tail=TP_DEFAULT // 2, hops_per_call=HOPS_PER_CALL)     # the frames and the hops of tests/test_gpu_channelizer.py


def test_three_links_end_to_end_through_the_channeliser_and_the_receive_loop():
    """Mode 8, D = 4: three frames from transmit_byte_dev, left on the device, each at its start sample in silence, through Synthesizer ->
    Channelizer -> RxCapture.run_wideband in calls of 16 hops, complex64 IQ, no noise. The second link is 30 dB stronger than its neighbour
    3 kHz away and the third is LSB. Every link's payload arrives on its own capture and on no other, and the events (capture, hop,
    payload) are those of captures fed the transmitted audio itself delayed by tp samples."""
    torch = _torch()
    rx, D, S = _rx(), 4, 3
    starts = LINKS.starts_the_loop_delivers((TP_DEFAULT,))             # where the loop delivers the audio delayed by tp
    payloads, frames = LINKS.frames()
    fsz = frames.shape[1]
    direct = LINKS.audio(starts, TP_DEFAULT)
    n = direct.shape[1]
    d_payloads = torch.from_numpy(payloads).cuda()
    d_audio = torch.zeros((S, n), dtype=torch.float64, device="cuda")
    d_frames = torch.zeros((S, fsz), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                                            # the library works on its own stream
    rx.transmit_byte_dev(d_payloads.data_ptr(), rx.payload_bytes, S, d_frames.data_ptr(), CARRIER)
    rx.lib.mgpu_synchronize(rx.h, None)
    assert np.array_equal(d_frames.cpu().numpy(), frames)
    for s in range(S):
        d_audio[s, starts[s]: starts[s] + fsz] = d_frames[s]
    torch.cuda.synchronize()
    plan = [(OFFSETS[s], SIDEBANDS[s], GAINS[s]) for s in range(S)]
    sy = Synthesizer(rx, D, plan)
    ch = Channelizer(rx, D, [(o, sb, 1.0 / g) for o, sb, g in plan])
    caps = [RxCapture(rx, S, CARRIER, max_hops=HOPS_PER_CALL) for _ in range(2)]
    step = HOPS_PER_CALL * caps[0].P
    d_iq = torch.zeros(step * D, dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    got = []
    for c in range(n // step):
        sy.process(d_audio[:, c * step: (c + 1) * step], fmt="cf32", out=d_iq)          # the context's stream, as run_wideband's
        got += [(e[0], e[1] + c * HOPS_PER_CALL, e[3].tobytes()) for e in caps[0].run_wideband(ch, d_iq)]
    want = [(e[0], e[1], e[3]) for e in LINKS.run_in_calls(direct, caps[1].run)]
    print("through the band: (capture, hop, own payload)", [(e[0], e[1], e[2] == payloads[e[0]].tobytes()) for e in got])
    print("the audio delayed by tp:                     ", [(e[0], e[1], e[2] == payloads[e[0]].tobytes()) for e in want])
    assert got == want
    for s in range(S):
        assert any(e[0] == s and e[2] == payloads[s].tobytes() for e in got), "link %d was not delivered" % s
        assert not any(e[0] != s and e[2] == payloads[s].tobytes() for e in got), "link %d arrived on another capture" % s
    sy.close(), ch.close()
    for c in caps:
        c.close()


def test_create_use_destroy_gives_the_memory_back():
    """create / process / retune / destroy cycles (history, tables, staging, the output workspace) leave the device's free memory
    where it was"""
    import gc
    torch = _torch()

    def free_hbm():
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info()[0]

    rx, D, S, n_in = _rx(), 16, 64, 2 * 1088
    rng = np.random.default_rng(6)
    chs = _channels(rng, D, S)
    audio = rng.standard_normal((S, n_in))

    def cycle():
        sy = Synthesizer(rx, D, chs)
        sy.process(audio, fmt="cs16")
        sy.retune(5, chs[6])
        sy.process(audio[:, :100])
        return sy

    cycle().close()
    first = free_hbm()
    for c in range(4):
        sy = cycle()
        in_use = first - free_hbm()
        sy.close()
        # the output workspace of max_in D CF64 samples and the staged audio [S][n_in]
        assert in_use >= 16 * 1088 * D * 16 + S * n_in * 8, in_use
        after = free_hbm()
        assert abs(after - first) < 64 << 20, (c, first, after)

"""The rational resampler on the GPU (include/ext/mercury_resampler.h, mercury_amd.Resampler): every output against the normative host
twin, bit for bit (the uint64 view), at the shapes where the kernel's tiling can go wrong; every format from host and device memory; cut
invariance with calls that produce nothing; a far position; non-finite samples; three links end to end through the receive loop at
44 100 and 8 000 Hz; the refusals of run_resampled; device memory.

The kernel computes Resampler.tile consecutive outputs of one stream per workgroup (mgpu_resamp_status.tile, 128) from one LDS image of
their input span; tests/test_resampler_host.py pins the twin itself."""
import numpy as np
import pytest

import resampler_ref as rr
from band_links import ThreeLinks, bits as _bits, events as _events, last_error, other_rx, rx as _rx, torch as _torch
from mercury_amd import MgpuError, Resampler, RxCapture, host_resamp_count, host_resamp_design, host_resamp_process
from oraclelib import CARRIER

pytestmark = pytest.mark.gpu


def _signal(rng, S, n, C, fmt="f64"):
    if C == 2:
        if fmt == "cs16":
            return rng.integers(-2 ** 15, 2 ** 15, (S, n, 2)).astype(np.int16)
        x = rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n))
        return x.astype(np.complex64 if fmt == "cf32" else np.complex128)
    if fmt == "i16":
        return rng.integers(-2 ** 15, 2 ** 15, (S, n)).astype(np.int16)
    if fmt == "i32":
        return rng.integers(-2 ** 31, 2 ** 31, (S, n)).astype(np.int32)
    return rng.standard_normal((S, n)).astype(np.float32 if fmt == "f32" else np.float64)


def _call_for(fin, fout, n_out):
    """(m0, n_in): the start position below M and the input count whose call gives n_out outputs, or where no call does (a call's count
    moves in steps of floor or ceil of L / M) the least count above it"""
    L, M = rr.ratio(fin, fout)
    near = n_out * M // L
    calls = [(m0, n_in) for m0 in range(M) for n_in in range(max(1, near - 2), near + 4) if rr.count(L, M, m0, n_in) >= n_out]
    return min(calls, key=lambda c: (rr.count(L, M, *c), c))


EDGE_CASES = [(44100, 48000, 1), (12000, 48000, 1), (8000, 48000, 1), (96000, 48000, 1), (11025, 48000, 1), (48000, 48000, 1),
              (2048000, 1536000, 2)]


@pytest.mark.parametrize("tp", [2, None])
@pytest.mark.parametrize("fin,fout,C", EDGE_CASES, ids=["%d-%d" % c[:2] for c in EDGE_CASES])
def test_outputs_equal_the_twin_at_the_tile_edges(fin, fout, C, tp):
    """S = 3, n_out one less than a tile, a tile, one more, and three tiles and five: tp = 2 is the shortest filter there is, None the
    default. The counts are exact wherever a call can give them, else the least count above (_call_for)."""
    rx = _rx()
    h = host_resamp_design(fin, fout, tp=tp)
    rng = np.random.default_rng(fin % 7919 + (tp or 0))
    rs = Resampler(rx, fin, fout, S=3, components=C, taps=h)
    tile, L, M = rs.tile, rs.L, rs.M
    assert tile == rs.info().tile >= 64 and rs.delay == rs.tp * L / (2.0 * M)
    for target in (tile - 1, tile, tile + 1, 3 * tile + 5):
        m0, n_in = _call_for(fin, fout, target)
        n_out = rr.count(L, M, m0, n_in)
        assert target <= n_out < target + -(-L // M), (n_out, target)
        x = _signal(rng, 3, n_in, C)
        rs.seek(m0)
        got = rs.process(x)
        want = host_resamp_process(fin, fout, x, position=m0, components=C, taps=h)
        assert got.shape == want.shape == (3, n_out)
        assert np.abs(want).max() > 0
        assert np.array_equal(_bits(got), _bits(want)), (target, np.abs(got - want).max())
    rs.close()


FORMATS = [(1, "i16"), (1, "i32"), (1, "f32"), (1, "f64"), (2, "cs16"), (2, "cf32"), (2, "cf64")]


@pytest.mark.parametrize("C,fmt", FORMATS, ids=[f for _, f in FORMATS])
def test_every_format_from_host_and_device_memory(C, fmt):
    """each sample format through process() from host memory and from a device tensor, and through process_dev (device in and out, on a
    stream of the caller's and on the context's, into rows longer than the outputs)"""
    torch = _torch()
    rx, S = _rx(), 3
    fin, fout = (44100, 48000) if C == 1 else (2048000, 1536000)
    rng = np.random.default_rng(40 + len(fmt) + ord(fmt[1]))
    rs = Resampler(rx, fin, fout, S=S, components=C)
    x = _signal(rng, S, 2 * rs.tile + 37, C, fmt)
    want = host_resamp_process(fin, fout, x, components=C)
    n_out = want.shape[1]
    d_x = torch.from_numpy(x).cuda()
    assert np.array_equal(_bits(rs.process(x)), _bits(want))
    rs.seek(0)
    assert np.array_equal(_bits(rs.process(d_x)), _bits(want))
    stride = n_out + 3
    d_out = torch.zeros((S, stride * C), dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    for st in (stream, None):
        rs.seek(0)
        d_out.zero_()
        if st is not None:
            st.wait_stream(torch.cuda.current_stream())
        assert rs.process(d_x, out=d_out, stream=None if st is None else st.cuda_stream) == n_out
        if st is not None:
            st.synchronize()
        else:
            rx.lib.mgpu_synchronize(rx.h, None)
        got = d_out.cpu().numpy()
        assert np.array_equal(_bits(got[:, : n_out * C]), _bits(np.ascontiguousarray(want).view(np.float64)))
        assert not got[:, n_out * C:].any()
    rs.close()


@pytest.mark.parametrize("fin,fout", [(44100, 48000), (192000, 48000), (11025, 48000)])
def test_cutting_does_not_change_an_output(fin, fout):
    """one max_in call, then the same stream in random cuts and in runs of 1-sample calls (at 1/4 three of four return nothing): the
    concatenation equals the whole and the twin, and every call's count is host_resamp_count's"""
    rx, S = _rx(), 2
    rs = Resampler(rx, fin, fout, S=S)
    rng = np.random.default_rng(fin + 1)
    n = rs.max_in
    x = _signal(rng, S, n, 1, "f32")
    whole = rs.process(x)
    assert whole.shape[1] == host_resamp_count(fin, fout, 0, n)
    assert np.array_equal(_bits(whole), _bits(host_resamp_process(fin, fout, x)))
    rs.seek(0)
    cuts, at = [], 0
    while at < n:
        run = [1] * 9 if len(cuts) % 5 == 2 else [int(rng.integers(1, 4 * rs.tp)) if len(cuts) % 2 else int(rng.integers(1, n // 6))]
        for c in run:
            c = min(c, n - at)
            if c:
                cuts.append(c)
                at += c
    parts, at, empty = [], 0, 0
    for c in cuts:
        part = rs.process(x[:, at: at + c])
        assert part.shape[1] == host_resamp_count(fin, fout, at, c)
        empty += part.shape[1] == 0
        parts.append(part)
        at += c
    assert np.array_equal(_bits(np.concatenate(parts, axis=1)), _bits(whole))
    assert empty > 0 or fin < fout
    # a refused call changes nothing: the next cut continues the stream
    rs.seek(0)
    first = rs.process(x[:, :777])
    with pytest.raises(MgpuError) as e:
        rs.process(np.zeros((S, n + 1), np.float32))                  # more than max_in
    assert e.value.code == 1
    second = rs.process(x[:, 777: 2000])
    assert np.array_equal(_bits(np.concatenate([first, second], axis=1)), _bits(whole[:, : first.shape[1] + second.shape[1]]))
    rs.close()


def test_a_far_position_equals_the_twin_there():
    """after seek(2^40 + 12345) the outputs are the twin's at that position (another phase sequence than at 0, zeros for a history)"""
    rx, fin, fout = _rx(), 44100, 48000
    pos = 2 ** 40 + 12345
    rng = np.random.default_rng(12)
    x = _signal(rng, 2, 1000, 1)
    rs = Resampler(rx, fin, fout, S=2)
    rs.process(x[:, :300])                                            # a history to forget
    rs.seek(pos)
    a, b = rs.process(x[:, :411]), rs.process(x[:, 411:])
    want = host_resamp_process(fin, fout, x, position=pos)
    st = rs.info()
    assert st.m0 == pos + 1000 and st.n0 == -(-(pos + 1000) * 160 // 147)
    assert np.array_equal(_bits(np.concatenate([a, b], axis=1)), _bits(want))
    assert not np.array_equal(_bits(want[:, :900]), _bits(host_resamp_process(fin, fout, x)[:, :900]))       # the position matters
    rs.close()


def test_non_finite_samples_go_through_the_same_chain():
    """one Inf and one NaN in the input: the twin's NaN outputs are NaN here (payload bits not compared), all others equal to the bit"""
    rx, fin, fout = _rx(), 44100, 48000
    rng = np.random.default_rng(13)
    x = _signal(rng, 2, 600, 1)
    x[0, 200], x[1, 333] = np.inf, np.nan
    rs = Resampler(rx, fin, fout, S=2)
    got, want = rs.process(x), host_resamp_process(fin, fout, x)
    nan = np.isnan(want)
    assert nan.any() and not nan.all() and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])
    rs.close()


DELAYS = {44100: 32 * 160 / (2.0 * 147), 8000: 32 * 6 / 2.0}          # 17.41 and 96 output samples
HOPS_PER_CALL = 15              # H P samples are whole numbers of samples at 44 100 and 8 000 Hz
LINKS = ThreeLinks(seed=2025, tail=96, hops_per_call=HOPS_PER_CALL)    # the tail: the longest delay


def _starts_the_loop_delivers():
    """The resampler moves a frame by its delay on the loop's hop grid (band_links.ThreeLinks.starts_the_loop_delivers): the starts at
    which the loop delivers the transmitted 48 kHz audio delayed by 17, by 18 (floor and ceil of 17.41, the delay at 44 100 Hz) and by 96
    samples (the delay at 8 000 Hz)"""
    return LINKS.starts_the_loop_delivers(tuple(sorted({int(np.floor(d)) for d in DELAYS.values()} | {int(np.ceil(d)) for d in DELAYS.values()})))


@pytest.mark.parametrize("fin", [44100, 8000])
def test_three_links_end_to_end_through_the_receive_loop(fin):
    """Mode 8, S = 3: three transmit_byte frames in silence at start samples that are no multiple of P, made at rate fin by the test's FFT
    method, float32, fed to run_resampled in calls of unequal n_in. (a) The events, with hops accumulated over the calls, and payloads are
    exactly those of RxCapture.run on the twin's whole output cut into the same hops; (b) no capture reports a CRC-good payload that is
    not its link's; (c) every link is delivered (the starts are those of _starts_the_loop_delivers)."""
    rx = _rx()
    payloads, _ = LINKS.frames()
    audio = LINKS.audio(_starts_the_loop_delivers())
    x = rr.fft_resample(audio, 48000, fin).astype(np.float32)
    n = x.shape[1]
    twin = host_resamp_process(fin, 48000, x)
    assert twin.shape == audio.shape
    d = DELAYS[fin]
    for s in range(3):
        print("link %d: audio error against the 48 kHz audio delayed by %.2f: %.1f dB" % (s, d, rr.error_db(twin[s], rr.fft_delay(audio[s], d))))
    rs = Resampler(rx, fin, 48000, S=3)
    assert rs.delay == d
    cuts = [rs.max_in * 3 // 16 + 1, rs.max_in // 2 + 3, 1, rs.max_in * 5 // 16 + 2, rs.max_in - 7]
    caps = [RxCapture(rx, 3, CARRIER, max_hops=HOPS_PER_CALL) for _ in range(2)]
    got, hops, at, i = [], [], 0, 0
    while at < n:
        c = min(cuts[i % len(cuts)], n - at)
        ev, H = caps[0].run_resampled(rs, np.ascontiguousarray(x[:, at: at + c]))
        got += _events(ev, sum(hops))
        hops.append(H)
        at, i = at + c, i + 1
    P = caps[0].P
    assert sum(hops) == twin.shape[1] // P and rs.info().fifo == twin.shape[1] % P
    want = LINKS.run_in_calls(twin, caps[1].run, hops)
    print("run_resampled: (capture, hop, own payload)", [(e[0], e[1], e[3] == payloads[e[0]].tobytes()) for e in got])
    rs.close()
    for c in caps:
        c.close()
    assert got == want
    for e in got:
        crc = np.frombuffer(e[2], np.int32, 4)[1]               # RECEIVE_STATS_DTYPE: iterations_done, crc, ...
        assert not crc or e[3] == payloads[e[0]].tobytes(), "capture %d reports a payload that is not its link's" % e[0]
    for s in range(3):
        assert any(e[0] == s and e[3] == payloads[s].tobytes() for e in got), "link %d was not delivered" % s


def test_run_resampled_refuses_what_does_not_fit_the_loop():
    """another S, C = 2, fout != 48000 or a capture of another context gives MGPU_ERR_ARG, and so does a format that is no capture format;
    every refusal leaves its words as the resampler's context's last error, and the resampler where it was"""
    rx = _rx()
    cap = RxCapture(rx, 3, CARRIER)
    x = np.zeros((3, 500), np.float32)
    does_not_pair = "mgpu_capture_run_resampled: one context, the same S, components = 1 and fout = 48000"
    for kw in (dict(S=2), dict(S=3, components=2), dict(S=3, fout=44100)):
        kw = dict(dict(fout=48000), **kw)
        rs = Resampler(rx, 48000 if kw["fout"] != 48000 else 44100, **kw)
        with pytest.raises(MgpuError) as e:
            cap.run_resampled(rs, x)
        assert e.value.code == 1 and last_error(rx) == does_not_pair
        rs.close()
    rs = Resampler(rx, 44100, S=3)
    elsewhere = RxCapture(other_rx(), 3, CARRIER)                      # a capture on a second context of the same device
    with pytest.raises(MgpuError) as e:
        elsewhere.run_resampled(rs, x)
    assert e.value.code == 1 and last_error(rx) == does_not_pair
    elsewhere.close()
    n, hops = np.zeros(1, np.int32), np.zeros(1, np.int32)
    assert rx.lib.mgpu_capture_run_resampled(cap.h, rs.h, x.ctypes.data, 7, 500, None, None, 0, n.ctypes.data, hops.ctypes.data) == 1
    assert last_error(rx) == "the format does not fit the components"
    assert rs.info().m0 == 0 and rs.info().fifo == 0
    ev, H = cap.run_resampled(rs, x)                                   # 500 inputs: 545 outputs, no hop yet
    assert (ev, H) == ([], 0) and rs.info().fifo == 545
    rs.close(), cap.close()


def test_create_use_destroy_gives_the_memory_back():
    """create / process / run_resampled / destroy cycles (history, table, staging, output, FIFO and hop buffers) leave the device's free
    memory where it was"""
    import gc
    torch = _torch()

    def free_hbm():
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info()[0]

    rx, S = _rx(), 64
    x = _signal(np.random.default_rng(6), S, 3000, 1, "i16")

    def cycle():
        rs = Resampler(rx, 44100, S=S)
        cap = RxCapture(rx, S, CARRIER)
        rs.process(x)
        rs.seek(0)
        cap.run_resampled(rs, x)
        return rs, cap

    for o in cycle():
        o.close()                                         # the context's receive_byte workspace is sized on first use
    first = free_hbm()
    for c in range(4):
        rs, cap = cycle()
        in_use = first - free_hbm()
        rs.close(), cap.close()
        assert in_use >= S * rs.max_out * 8, in_use        # process()'s output rows alone
        after = free_hbm()
        assert abs(after - first) < 64 << 20, (c, first, after)

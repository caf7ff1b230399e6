"""The streaming form of the Watterson HF channel (mgpu_hf_stream_*, mercury_amd.HfStream).

Yardstick: the whole-signal kernel (mgpu_hf_channel_apply_dev), which tests/test_gpu_hf_channel.py ties to the numpy composition of the
host definitions. Chunking must change no bit, and the stream must equal that kernel's output delayed by the latency."""
import numpy as np
import pytest

from mercury_amd import HfChannel, HfStream, MgpuError, RxPhy, hf_channel_preset, host_hf_stream_noise

pytestmark = pytest.mark.gpu
SEED = 0x48465354
S, HOP = 3, 1088
N = 40 * HOP

CHANNELS = {
    "good": lambda: hf_channel_preset("good"),
    "poor": lambda: hf_channel_preset("poor"),
    "flutter": lambda: hf_channel_preset("flutter"),
    "four_paths": lambda: HfChannel(paths=((0.0, 0.0, 0.3, 0.0), (1.7, -3.0, 1.0, 0.4), (4.2, -6.0, 0.0, -1.5), (10.0, -9.0, 2.0, 0.0)),
                                    freq_offset_hz=3.7),
}
MIXED = [64, 64 * 37, HOP, 64, 64 * 3, 5 * HOP, 64 * 37, 64]


def _chunkings():
    mixed = list(MIXED)
    mixed.append(N - sum(mixed))
    assert mixed[-1] > 0 and mixed[-1] % 64 == 0
    return {"one": [N], "hops": [HOP] * 40, "mixed": mixed}


def _torch():
    import torch
    return torch


def _whole(rx, x, ch, t0):
    torch = _torch()
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.empty_like(d_in)
    s = torch.cuda.current_stream()
    rx.hf_channel_apply_dev(d_in.data_ptr(), d_out.data_ptr(), x.shape[0], x.shape[1], ch, SEED, 0, realisation0=5, t0=t0, stream=s.cuda_stream)
    s.synchronize()
    return d_out.cpu().numpy()


def _streamed(rx, x, ch, pieces, seek=None, device=False):
    st = HfStream(rx, x.shape[0], ch, SEED, realisation0=5)
    if seek is not None:
        st.seek(seek)
    out, at = [], 0
    for n in pieces:
        c = np.ascontiguousarray(x[:, at: at + n])
        if device:
            s = _torch().cuda.current_stream()
            y = st.apply(_torch().from_numpy(c).cuda(), stream=s.cuda_stream)
            s.synchronize()
            out.append(y.cpu().numpy())
        else:
            out.append(st.apply(c))
        at += n
    L = st.latency
    st.close()
    return np.concatenate(out, axis=1), L


@pytest.mark.parametrize("name", list(CHANNELS))
def test_chunking_changes_no_bit(name):
    rx = RxPhy(8, max_iters=10, max_batch=8)
    ch = CHANNELS[name]()
    x = np.random.default_rng(len(name)).standard_normal((S, N))
    for seek in (None, 2 ** 32 + 64 * 5):
        outs = {}
        for k, (cname, pieces) in enumerate(_chunkings().items()):
            outs[cname], L = _streamed(rx, x, ch, pieces, seek, device=(k == 1))
        assert L == 256
        for cname in ("hops", "mixed"):
            assert np.array_equal(outs[cname].view(np.uint64), outs["one"].view(np.uint64)), (name, seek, cname)
        o = outs["one"]
        want = _whole(rx, x, ch, 0 if seek is None else seek)
        assert np.array_equal(o[:, L:].view(np.uint64), want[:, : N - L].view(np.uint64)), (name, seek)
        assert not o[:, :L].any()
        assert np.abs(o).max() > 0.1
    rx.close()


def test_identity_channel_is_a_delay_and_the_noise_is_the_host_twins():
    rx = RxPhy(8, max_iters=10, max_batch=8)
    x = np.random.default_rng(2).standard_normal((S, N))
    o, L = _streamed(rx, x, "awgn", _chunkings()["mixed"])
    assert np.array_equal(o[:, L:].view(np.uint64), x[:, : N - L].view(np.uint64)) and not o[:, :L].any()
    amp = np.array([0.25, 1.0, 3.0])
    for ch, pos in (("awgn", 0), ("awgn", 2 ** 32 - 64 * 7), ("moderate", 2 ** 32 - 64 * 7)):
        st = HfStream(rx, S, ch, SEED, realisation0=5)
        st.seek(pos)
        quiet = HfStream(rx, S, ch, SEED, realisation0=5)
        quiet.seek(pos)
        got = np.concatenate([st.apply(x[:, :HOP], amp), st.apply(x[:, HOP: 2 * HOP]), st.apply(x[:, 2 * HOP: 4 * HOP], amp)], axis=1)
        clean = quiet.apply(x[:, : 4 * HOP])
        noise = np.stack([amp[s] * host_hf_stream_noise(SEED, s, pos, 4 * HOP) for s in range(S)])
        noise[:, HOP: 2 * HOP] = 0                                           # noise_amp = NULL adds nothing
        assert np.array_equal(got[:, HOP: 2 * HOP].view(np.uint64), clean[:, HOP: 2 * HOP].view(np.uint64))
        # device against host Box-Muller: the bound of test_txgen_matches_cpu_generator_and_round_trips
        assert np.abs(got - clean - noise).max() <= 1e-9 * np.abs(noise).max(), (ch, pos)
        assert np.abs(noise).max() > 3
        st.close(), quiet.close()
    rx.close()


def test_bad_chunks_are_refused_and_leave_the_state_alone():
    rx = RxPhy(8, max_iters=10, max_batch=8)
    x = np.random.default_rng(3).standard_normal((S, 6 * HOP))
    want, _ = _streamed(rx, x, "moderate", [6 * HOP])
    st = HfStream(rx, S, "moderate", SEED, realisation0=5)
    got = [st.apply(x[:, : 2 * HOP])]
    for n in (100, 63, 0):
        with pytest.raises(MgpuError):
            st.apply(np.zeros((S, n)))
    buf = np.ascontiguousarray(x[:, 2 * HOP: 3 * HOP])
    with pytest.raises(MgpuError):
        st.apply(buf, out=buf)                                                # in == out
    with pytest.raises(MgpuError):
        st.seek(100)
    assert rx.lib.mgpu_hf_stream_apply(st.h, None, 64, None, None) != 0
    assert rx.lib.mgpu_hf_stream_apply(st.h, buf.ctypes.data, -64, None, np.empty_like(buf).ctypes.data) != 0       # n <= 0
    got.append(st.apply(x[:, 2 * HOP:]))
    assert np.array_equal(np.concatenate(got, axis=1).view(np.uint64), want.view(np.uint64))
    st.close()
    with pytest.raises(MgpuError):
        HfStream(rx, S, HfChannel(paths=((11.0, 0.0, 0.0, 0.0),)), SEED)       # the checks are mgpu_hf_channel_apply's
    with pytest.raises(MgpuError):
        HfStream(rx, 0, "good", SEED)
    rx.close()

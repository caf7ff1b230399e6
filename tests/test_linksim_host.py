"""Host-only parts of the link simulator and the streaming HF channel (include/mercury_linksim.h, include/mercury_channel.h): the frame
schedule, the payloads and the noise draws a caller needs to rebuild what a simulator sent. No GPU."""
import ctypes as C

import numpy as np
import pytest

from mercury_amd import (HF_STREAM_SYMBOLS, LINKSIM_SYMBOLS, MgpuError, host_hf_stream_noise, host_linksim_frame_start, host_linksim_payload,
                         linksim_config, load_library)
from mercury_amd.physical_layer import NO_FILTER_MESSAGE, LinkSimConfig

FRAME, P = 30464, 1088            # mode 8: (Nsymb + preamble_nSymb) * Nofdm * 4 and Nofdm * 4


def test_symbols_are_exported_and_the_config_layout_is_the_headers():
    lib = load_library()
    for name in HF_STREAM_SYMBOLS + LINKSIM_SYMBOLS:
        assert hasattr(lib, name), name
    assert C.sizeof(LinkSimConfig) == 248      # 4 ints, uint64, mgpu_hf_channel (144), mgpu_receive_config (24), mgpu_transmit_config (56)


@pytest.mark.parametrize("gap", [0, 8])
def test_frame_start_schedule(gap):
    """offsets in [0, slot), equal for equal (seed, link), not all equal across 16 links, starts one slot apart"""
    k = linksim_config(16, 1450.0, seed=11, gap_hops=gap)
    slot = FRAME + gap * P
    offs = [host_linksim_frame_start(k, FRAME, P, s, 0) for s in range(16)]
    assert all(0 <= o < slot for o in offs) and len(set(offs)) > 1
    assert offs == [host_linksim_frame_start(linksim_config(16, 1450.0, seed=11, gap_hops=gap), FRAME, P, s, 0) for s in range(16)]
    assert offs != [host_linksim_frame_start(linksim_config(16, 1450.0, seed=12, gap_hops=gap), FRAME, P, s, 0) for s in range(16)]
    # a link's offset does not depend on how many links there are
    assert offs[:4] == [host_linksim_frame_start(linksim_config(4, 1450.0, seed=11, gap_hops=gap), FRAME, P, s, 0) for s in range(4)]
    for s in (0, 7, 15):
        starts = [host_linksim_frame_start(k, FRAME, P, s, j) for j in range(5)]
        assert list(np.diff(starts)) == [slot] * 4 and starts[0] == offs[s]


def test_frame_start_refuses_bad_configurations():
    good = linksim_config(16, 1450.0, seed=1)
    assert host_linksim_frame_start(good, FRAME, P, 0, 0) >= 0
    for change in (dict(struct_size=244), dict(S=0), dict(gap_hops=-1)):
        k = linksim_config(16, 1450.0, seed=1)
        for name, v in change.items():
            setattr(k, name, v)
        with pytest.raises(MgpuError):
            host_linksim_frame_start(k, FRAME, P, 0, 0)
    with pytest.raises(MgpuError):
        host_linksim_frame_start(linksim_config(16, 1450.0, seed=1, message_location=NO_FILTER_MESSAGE), FRAME, P, 0, 0)
    with pytest.raises(MgpuError):
        host_linksim_frame_start(good, FRAME, P, 16, 0)            # no such link


def test_payload_is_keyed_by_seed_link_and_frame():
    a = host_linksim_payload(5, 3, 7, 100)
    assert np.array_equal(a, host_linksim_payload(5, 3, 7, 100))
    assert np.array_equal(a[:37], host_linksim_payload(5, 3, 7, 37))          # a shorter payload is a prefix: asked in pieces = in one
    for other in ((6, 3, 7), (5, 4, 7), (5, 3, 8), (5, 3, 7 + 2 ** 32)):
        assert not np.array_equal(a, host_linksim_payload(*other, 100)), other
    many = np.concatenate([host_linksim_payload(5, 0, j, 64) for j in range(512)])
    counts = np.bincount(many, minlength=256)
    # 32768 uniform bytes: every value's count within 6 sigma of n / 256 (sigma = sqrt(n p (1 - p)) = 11.3)
    assert np.abs(counts - many.size / 256).max() < 6 * np.sqrt(many.size * (1 / 256) * (255 / 256))


def test_stream_noise_ranges_counter_and_moments():
    """a range in two pieces equals the range in one; positions p and p + 2^32 differ (64-bit counter); mean and variance of 2^20 draws
    within 5 standard errors of 0 and 1 (5 / sqrt(N), 5 sqrt(2 / N): the standard errors of a unit normal's mean and variance)"""
    seed, N = 0x4C494E4B, 1 << 20
    for p in (0, 12345, 2 ** 32 - 100, 2 ** 40 + 64):
        whole = host_hf_stream_noise(seed, 2, p, 1000)
        parts = np.concatenate([host_hf_stream_noise(seed, 2, p, 333), host_hf_stream_noise(seed, 2, p + 333, 667)])
        assert np.array_equal(whole.view(np.uint64), parts.view(np.uint64)), p
    a, b = host_hf_stream_noise(seed, 2, 4096, 256), host_hf_stream_noise(seed, 2, 4096 + 2 ** 32, 256)
    assert not np.any(a == b)
    assert not np.any(a == host_hf_stream_noise(seed, 3, 4096, 256)) and not np.any(a == host_hf_stream_noise(seed + 1, 2, 4096, 256))
    g = host_hf_stream_noise(seed, 0, 2 ** 33, N)
    assert abs(g.mean()) <= 5 / np.sqrt(N), g.mean()
    assert abs(g.var() - 1) <= 5 * np.sqrt(2 / N), g.var()

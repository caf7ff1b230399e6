"""What the GPU tests of the block-in, block-out IQ stages (WidebandBlanker, IqCorrector) share: comparing (out, reports) pairs byte for
byte, feeding a stream in calls, reading reports back from a device tensor, and the memory check. A plain module beside band_links: no
test lives here and no test file imports another."""
import gc

import numpy as np

from band_links import torch as _torch


def same(got, want):
    """two (out, reports) pairs are equal in shape, type and every byte"""
    return (got[0].shape == want[0].shape and got[0].dtype == want[0].dtype and got[0].tobytes() == want[0].tobytes()
            and got[1].shape == want[1].shape and got[1].tobytes() == want[1].tobytes())


def device_reports(d_reports, n, dtype):
    """the first n reports of a uint8 device tensor as a structured array"""
    return d_reports.cpu().numpy().reshape(-1)[: n * dtype.itemsize].view(dtype)


def join(parts):
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def in_calls(stage, x, blocks):
    """x fed in calls of the given block counts -> (out, reports) of all calls"""
    parts, at = [], 0
    for m in blocks:
        o, r = stage.process_raw(x[at * stage.B: (at + m) * stage.B])
        assert len(o) == m * stage.B and len(r) == m
        parts.append((o, r))
        at += m
    assert at * stage.B == len(x)
    return join(parts)


def memory_comes_back(make, x):
    """50 make() / process / close cycles on x, 64 blocks of 4096 CF64 samples, leave the device's free memory where it was"""
    torch = _torch()

    def free_hbm():
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info()[0]

    def cycle():
        stage = make()
        stage.process_raw(x)
        return stage

    cycle().close()
    first = free_hbm()
    stage = cycle()
    in_use = first - free_hbm()
    stage.close()
    assert in_use >= 2 * 64 * 4096 * 16, in_use                         # the staging area and the output of 64 blocks
    for _ in range(50):
        cycle().close()
    after = free_hbm()
    assert abs(after - first) < 64 << 20, (first, after)

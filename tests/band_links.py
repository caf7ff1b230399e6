"""What the tests of the stream stages (channeliser, synthesiser, resampler) and of the receive loop share: the small generators, and three
links' frames in silence run through RxCapture in calls of some hops. A plain module: no test lives here and no test file imports another."""
import ctypes as C
import functools

import numpy as np
import pytest

from mercury_amd import MgpuError, RxCapture, RxPhy, host_chan_design
from oraclelib import CARRIER

MAX_ITERS = 10
FIRST_STARTS = (5 * 1088 + 333, 7 * 1088 + 17, 11 * 1088 + 901)        # mode 8: P = 1088


def torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def rx():
    return RxPhy(8, max_iters=MAX_ITERS, max_batch=8)


@functools.lru_cache(maxsize=None)
def other_rx():
    """a second context of the same mode on the same device"""
    return RxPhy(8, max_iters=MAX_ITERS, max_batch=8)


def last_error(ctx):
    return ctx.lib.mgpu_last_error(ctx.h).decode()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def iq(rng, n, fmt):
    if fmt == "cs16":
        return rng.integers(-2 ** 15, 2 ** 15, (n, 2)).astype(np.int16)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return x.astype(np.complex64 if fmt == "cf32" else np.complex128)


def channels(rng, D, S):
    """S channels anywhere a band fits in (-R/2, R/2): both sidebands, both signs of the offset, gains that are no powers of two"""
    half = 24000 * D
    out = []
    for s in range(S):
        sb = int(rng.integers(0, 2))
        lo, hi = (-half + 1, half - 2945) if sb == 0 else (-half + 2945, half - 1)
        out.append((int(rng.integers(lo, hi + 1)), sb, float(rng.uniform(0.3, 3.0))))
    return out


@functools.lru_cache(maxsize=None)
def taps(D, tp):
    return host_chan_design(D, tp)


def refused(fn):
    with pytest.raises(MgpuError) as e:
        fn()
    assert e.value.code == 1


def create_without_a_context(create, *args):
    """create(no context, *args, &handle) -> its status; the handle, set beforehand, comes back null whatever the status"""
    out = C.c_void_p(1)
    rc = create(None, *args, C.byref(out))
    assert not out.value
    return rc


def canon(r):
    """a structured scalar's field bytes, without its padding (bit patterns of the doubles kept)"""
    r = np.asarray(r)
    return b"".join(canon(r[n]) if r.dtype[n].names else np.asarray(r[n]).tobytes() for n in r.dtype.names)


def events(ev, hop0=0):
    """a run's events as (capture, hop + hop0, stats bytes, payload bytes)"""
    return [(e[0], e[1] + hop0, canon(e[2]), e[3].tobytes()) for e in ev]


class ThreeLinks:
    """Mode 8: three payloads (drawn from `seed`) and their transmit_byte frames, each in silence at its own start sample, as 48 kHz
    audio that the receive loop takes in calls of hops_per_call hops. tail: the samples the audio goes on behind the last frame's end,
    for what a stage in front of the loop delays it by."""

    def __init__(self, seed, tail, hops_per_call):
        self.seed, self.tail, self.hops_per_call = seed, tail, hops_per_call

    @functools.lru_cache(maxsize=None)
    def frames(self):
        payloads = np.random.default_rng(self.seed).integers(0, 256, (3, rx().payload_bytes)).astype(np.uint8)
        return payloads, rx().transmit_byte(payloads, CARRIER)

    def audio(self, starts, delay=0):
        """the three links' 48 kHz audio [3, H P]: each frame at its start sample (+ delay) in silence; H a multiple of hops_per_call by
        which every frame has ended, with the tail, and some hops more"""
        P = rx().Nofdm * 4
        _, frames = self.frames()
        fsz = frames.shape[1]
        H = -(-(max(starts) + fsz + self.tail + P) // P) + 4
        H = -(-H // self.hops_per_call) * self.hops_per_call
        assert P == 1088 and all(s % P for s in starts) and H * P > max(starts) + fsz + self.tail
        audio = np.zeros((3, H * P))
        for s in range(3):
            audio[s, starts[s] + delay: starts[s] + delay + fsz] = frames[s]
        return audio

    def run_in_calls(self, x, run, hops=None, D=1):
        """run(chunk) over x, [3, H P] audio or [H P D] IQ, cut along its last axis into calls of the given hop counts (None: hops_per_call
        each) -> events (capture, hop since the start, stats bytes, payload bytes)"""
        per_hop = rx().Nofdm * 4 * D
        if hops is None:
            hops = [self.hops_per_call] * (x.shape[-1] // (per_hop * self.hops_per_call))
        at, out = 0, []
        for H in hops:
            if H:
                out += events(run(np.ascontiguousarray(x[..., at * per_hop: (at + H) * per_hop])), at)
                at += H
        return out

    def delivered(self, ev):
        """the links whose own payload is among the events of their capture"""
        payloads, _ = self.frames()
        return {e[0] for e in ev if e[3] == payloads[e[0]].tobytes()}

    @functools.lru_cache(maxsize=None)
    def starts_the_loop_delivers(self, delays):
        """The receive loop's own synchroniser loses a noise-free frame at some positions on its hop grid, with no stage in front of it:
        fed the transmitted audio itself it delivers the frames at FIRST_STARTS but not the one at 7 P + 17 + 160 (measured;
        tests/test_gpu_channelizer.py pins it). A stage's delay moves a frame on that grid, so an end-to-end test places each link's frame
        where the loop delivers the transmitted audio DELAYED BY every one of `delays` samples: per link the first of start + 156 k,
        k = 0 .. 5 (residues that are no multiple of P), judged by RxCapture.run on that audio alone. What is chosen by is the existing
        loop on a pure delay, never a stage's output."""
        P = rx().Nofdm * 4
        chosen = [None] * 3
        for k in range(6):
            cand = tuple(FIRST_STARTS[s] + 156 * k for s in range(3))
            ok = {0, 1, 2}
            for d in delays:
                cap = RxCapture(rx(), 3, CARRIER, max_hops=self.hops_per_call)
                ok &= self.delivered(self.run_in_calls(self.audio(cand, d), cap.run))
                cap.close()
            for s in ok:
                if chosen[s] is None and cand[s] % P:
                    chosen[s] = cand[s]
            if all(c is not None for c in chosen):
                break
        assert all(c is not None for c in chosen), ("the loop delivers no candidate of a link", chosen)
        print("starts the loop delivers on the audio delayed by", list(delays), ":", chosen, [c % P for c in chosen])
        return tuple(chosen)

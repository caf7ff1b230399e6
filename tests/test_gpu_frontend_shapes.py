"""GPU tests of the front-end's and the estimator ladder's forms that no shipped geometry and no other test selects.

A. The 1024-thread front-end kernels (MERCURY_FE_THREADS=1024; no geometry defaults to them, tests/test_estimator_ladder_host.py) against the
   512-thread ones byte for byte and against the CPU oracle with test_all_stages_match_oracle's assertions.
B. The rectangular kernel's estimate against its host twin, bit for bit, over the window shapes: every width (the width selects the estimator's
   path and the masks of the branch-free row loop) times the heights that clip differently, with a NaN frame for the fallback out of that loop.
C. A ladder is the composition of its rungs: against CPU oracles, one per square window, and against one-rung ladders for rectangular windows.
D. More frames than mgpu_ladder_select_kernel takes in one pass (1024), in one piece and through the chunked host path (frame0 > 0).

Every comparison is bit-exact or byte-exact."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import SEED
from oraclelib import FLAGS_RECEIVE_BYTE, Oracle, noise_amp_for
from test_gpu_parity import _variants, stages_match_oracle

pytestmark = pytest.mark.gpu

DY5 = dict(Dy=5, Nsymb=20)          # mode 8 on the reference's LOW_DENSITY pilot lattice: the estimator's general (non-lattice) path
FE_THREADS = "MERCURY_FE_THREADS"   # read by mgpu_create with getenv: per context


def _rx(cfg, threads=None, monkeypatch=None, **kw):
    from mercury_amd import RxPhy
    if monkeypatch is not None:
        if threads:
            monkeypatch.setenv(FE_THREADS, str(threads))
        else:
            monkeypatch.delenv(FE_THREADS, raising=False)
    return RxPhy(cfg, **kw)


def _lds_fe(rx):
    """dynamic LDS bytes of the context's front-end workgroup"""
    return rx.lib.mgpu_debug_occupancy(rx.h, 1)


def _carve(rx, threads):
    return rx.lib.mgpu_frontend_lds_bytes(rx.Nsymb * rx.Nc, rx.nPilots, rx.nBits, threads)


# ---- A: 1024 threads ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,explicit", [(0, None), (8, None), (11, None), (13, None), (16, None), (8, DY5)], ids=["0", "8", "11", "13", "16", "8-dy5"])
def test_the_1024_thread_front_end_equals_the_512_thread_one_and_the_oracle(cfg, explicit, monkeypatch):
    """Three generator frames at 10 dB through channel 1, a clean one and one of noise only, in both variants of the span the oracle has (the
    zero-forcing mode in the one it has). 16 wavefronts share the FFT work areas, the carve is another one and 15 wavefronts take the
    data cells from the LDS queue: every tap, payload and stats must not care."""
    orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
    made = [orc.gen_frame(SEED, f, noise_amp_for(10.0), 1) for f in range(3)] + [orc.gen_frame(SEED, 3, 0.0)]
    rng = np.random.default_rng(3)
    noise = rng.standard_normal(orc.frame_samples) + 1j * rng.standard_normal(orc.frame_samples)
    bb = np.stack([b for b, _ in made] + [noise])
    payloads = [p for _, p in made] + [None]
    snrs = [10.0, 10.0, 10.0, np.inf, -np.inf]          # what stages_match_oracle wants to know: the clean frame must decode, the noise is never asked to
    for agc, vs, flags in _variants(cfg):
        kw = dict(max_iters=50, agc=agc, variance_source=vs, max_batch=5, explicit=explicit)
        rx512, rx1024 = _rx(cfg, 512, monkeypatch, **kw), _rx(cfg, 1024, monkeypatch, **kw)
        assert _lds_fe(rx512) == _carve(rx512, 512) and _lds_fe(rx1024) == _carve(rx1024, 1024) != _carve(rx1024, 512)      # the variable was read
        a, b = rx512.receive(bb, taps=True), rx1024.receive(bb, taps=True)
        assert sorted(a) == sorted(b)
        for key in a:
            if key != "cycles":
                assert a[key].tobytes() == b[key].tobytes(), (cfg, flags, key)
        assert a["stats"]["message_decoded"][3] == 1 and a["stats"]["message_decoded"][4] == 0
        stages_match_oracle(rx1024, orc, bb, payloads, snrs, flags)
        plain = rx1024.receive(bb)                      # no taps: the pipelined host path
        assert plain["payload"].tobytes() == b["payload"].tobytes() and plain["stats"].tobytes() == b["stats"].tobytes(), (cfg, flags)
        for f in (0, 4):                                # one frame: the captured graph
            one = rx1024.receive(bb[f:f + 1])
            assert one["payload"].tobytes() == b["payload"][f].tobytes() and one["stats"].tobytes() == b["stats"][f].tobytes(), (cfg, flags, f)
        rx512.close(), rx1024.close()


def test_a_workgroup_size_the_kernels_are_not_built_for_is_refused(monkeypatch):
    from mercury_amd import MgpuError
    from mercury_amd.physical_layer import Config, DEC_SPA, load_library
    monkeypatch.setenv(FE_THREADS, "768")
    with pytest.raises(MgpuError) as e:
        _rx(8, max_batch=2)
    assert "MERCURY_FE_THREADS" in str(e.value)
    lib, h = load_library(), C.c_void_p()
    assert lib.mgpu_create(C.byref(Config(8, 50, DEC_SPA, 1, 1, 0, 2, 0.0, 0, 0)), C.byref(h)) != 0 and not h.value       # no context is left behind
    monkeypatch.delenv(FE_THREADS)
    rx = _rx(8, max_batch=2)                            # and the next create is an ordinary one
    assert _lds_fe(rx) == _carve(rx, 512)
    rx.close()


# ---- the two-path construction of B, C and D ---------------------------------------------------------------------------------------
DELAYS = (0, 6, 12, 24, 40, 60)     # samples between the two paths (12 = 1 ms); 0: a single path


def _two_path_frames(orc, n, esn0_db, delays=DELAYS):
    """n clean generator frames (seed 5) through two equal-power static paths delays[f % len] samples apart - delay 0: one path, not scaled -,
    the phases from default_rng(7) (drawn for every frame), then noise from the same generator. -> (baseband [n, samples], sent payloads)"""
    rng = np.random.default_rng(7)
    amp = noise_amp_for(esn0_db)
    bb, sent = [], []
    for f in range(n):
        x, pl = orc.gen_frame(5, f, 0.0, 0)
        ph = np.exp(1j * rng.uniform(0, 2 * np.pi, 2))
        d = delays[f % len(delays)]
        y = ph[0] * x
        if d:
            y[d:] += ph[1] * x[:-d]
            y /= np.sqrt(2.0)
        y += amp * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
        bb.append(y)
        sent.append(pl.astype(np.uint8))
    return np.stack(bb), np.stack(sent)


# ---- B: every window shape against the host twin -----------------------------------------------------------------------------------
WIDTHS = tuple(range(1, 22, 2))
HEIGHTS = (1, 3, 5, 11, 21)         # one row (k0 == k1), clipped at one end or the other, the default


def _twin_H(rx, cfg, explicit, grid, w, h, pilots):
    """What taps["H"] holds at the pilot cells for the w x h window: the host twin on the tapped grid, after restore_channel_amplitude (the
    device's own atan / sincos through the stage entry point) in the PSK modes. The other cells are 1 and are not compared.
    -> (that, the twin's estimate before the restoration: get_angle takes no branch on a NaN and so makes 1 + 0j of it, as the reference's does)"""
    from mercury_amd import host_ls_estimate
    want = np.ones(grid.shape, np.complex128)
    for f in range(grid.shape[0]):
        want[f, pilots] = host_ls_estimate(cfg, grid[f], w, h, explicit=explicit)
    est = want[:, pilots]
    if rx.amp_restore:
        rx._ck(rx.lib.mgpu_restore_channel_amplitude(rx.h, want.ctypes.data_as(C.c_void_p), grid.shape[0]))
    return want[:, pilots], est


def _same(a, b):
    """bit for bit where finite, NaN where NaN, in both parts"""
    return np.array_equal(a.real, b.real, equal_nan=True) and np.array_equal(a.imag, b.imag, equal_nan=True)


def _window_sweep(cfg, explicit, threads, windows, monkeypatch):
    """Three frames per call: the noisy two-path frame (delay 12, 20 dB), a clean one, and one with a single NaN sample in the middle of
    symbol 3. With the AGC the NaN reaches the whole grid; the second context runs without it, the NaN stays in row 3, and the row loop's
    fallback (exact) differs from its masked form (0.0 * NaN) wherever a seven-wide read runs from a row above into row 3's pilots."""
    orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
    bb = np.stack([_two_path_frames(orc, 1, 20.0, delays=(12,))[0][0], orc.gen_frame(5, 1, 0.0)[0], orc.gen_frame(5, 2, noise_amp_for(10.0))[0]])
    bb[2, 3 * orc.Nofdm + orc.Ngi + orc.Nfft // 2] = complex(np.nan, np.nan)
    pilots = np.flatnonzero(orc.frame_types() != 0)
    rx = _rx(cfg, threads, monkeypatch, max_batch=3, explicit=explicit)
    raw = _rx(cfg, threads, monkeypatch, max_batch=1, agc=0, variance_source=0, explicit=explicit)
    assert _lds_fe(rx) == _lds_fe(raw) == _carve(rx, threads or 512)
    square, raw_square = rx.receive(bb, taps=True), raw.receive(bb[2:], taps=True)
    assert np.isfinite(square["grid"][:2]).all() and np.isnan(square["grid"][2]).all()
    nan_rows = np.isnan(raw_square["grid"][0].reshape(orc.Nsymb, orc.Nc))
    assert nan_rows[3].all() and nan_rows.sum() == orc.Nc
    for w, h in windows:
        rx.set_estimator_ladder([(w, h)])
        raw.set_estimator_ladder([(w, h)])
        assert rx.estimator_ladder == [(w, h)]
        out, raw_out = rx.receive(bb, taps=True), raw.receive(bb[2:], taps=True)
        assert _same(out["grid"], square["grid"]) and _same(raw_out["grid"], raw_square["grid"]), (w, h)
        (want, _), (raw_want, raw_est) = _twin_H(rx, cfg, explicit, out["grid"], w, h, pilots), _twin_H(raw, cfg, explicit, raw_out["grid"], w, h, pilots)
        got, raw_got = out["H"][:, pilots], raw_out["H"][:, pilots]
        assert np.array_equal(got[:2], want[:2]), (w, h, np.abs(got[:2] - want[:2]).max())
        assert _same(got[2], want[2]), (w, h)
        assert _same(raw_got, raw_want), (w, h, np.flatnonzero(np.isnan(raw_got[0].real) != np.isnan(raw_want[0].real))[:8])
        assert np.isnan(raw_est.real).any() and (h > 5 or np.isfinite(raw_est).any()), (w, h)         # (a low window: the NaN stays near row 3)
        assert out["stats"]["message_decoded"][2] == 0, (w, h)
        if (w, h) == (21, 21):          # the control: rung 0 is the context's own window and runs the default kernel
            assert out["H"].tobytes() == square["H"].tobytes() and raw_out["H"].tobytes() == raw_square["H"].tobytes()
        else:                           # the window really was applied (every other shape, the row loop's widths 17 to 21 included)
            assert not np.array_equal(out["H"][0], square["H"][0]), (w, h)
    rx.close(), raw.close()


@pytest.mark.parametrize("cfg,explicit,threads", [(0, None, 512), (0, None, 1024), (8, None, 512), (8, None, 1024), (11, None, None), (8, DY5, None)],
                         ids=["0-512", "0-1024", "8-512", "8-1024", "11", "8-dy5"])
def test_every_width_of_the_rectangular_window_equals_the_host_twin(cfg, explicit, threads, monkeypatch):
    _window_sweep(cfg, explicit, threads, [(w, h) for w in WIDTHS for h in HEIGHTS], monkeypatch)


def test_all_121_windows_on_the_smallest_frame_equal_the_host_twin(monkeypatch):
    """mode 13: 12 symbols, so every window from height 13 on is the whole frame high, every tall one is clipped at both ends, and the 16QAM
    estimate is used as it is (no amplitude restoration)"""
    _window_sweep(13, None, None, [(w, h) for w in WIDTHS for h in WIDTHS], monkeypatch)


# ---- C: a ladder is the composition of its rungs -----------------------------------------------------------------------------------
N24 = 24
WINDOWS = (21, 9, 5, 1)
SQUARE = [(w, w) for w in WINDOWS]
LADDERS = (SQUARE, [(21, 21), (17, 5), (5, 21), (3, 3)], [(19, 3), (5, 21)])
ESN0 = {8: 20.0, 11: 22.0, 13: 25.0}
# frames by the first window whose CPU oracle decodes them (21, 9, 5, 1, none), measured on the oracle with this construction where "decodes" is
# a correct payload in at most 50 iterations. By the library's message_decoded (CRC good) mode 8 has 17, 3, 4: frame 17's payload is right with
# the 21-window although the decoder ran out of iterations. The table is only asked for its non-empty classes.
CLASSES = {11: (6, 4, 3, 6, 5), 13: (4, 6, 2, 0, 12), 8: (16, 4, 4, 0, 0)}


@functools.lru_cache(maxsize=None)
def _prototypes(cfg):
    """The 24 frames of a mode in CLASSES and what the CPU oracle makes of each with the four square windows. first[f]: index of the first
    window that decodes frame f (CRC good, not all zeros: the library's message_decoded), -1 for none."""
    orcs = [Oracle(cfg, 50, explicit=dict(ls_window=w)) for w in WINDOWS]
    bb, sent = _two_path_frames(orcs[0], N24, ESN0[cfg])
    refs = [[o.rx(bb[f], FLAGS_RECEIVE_BYTE) for f in range(N24)] for o in orcs]
    ok = np.array([[r["crc"] == 0 and r["all_zeros"] == 0 for r in row] for row in refs])
    first = np.where(ok.any(axis=0), ok.argmax(axis=0), -1)
    counts = tuple(int((first == r).sum()) for r in (0, 1, 2, 3, -1))
    # a condition on the input: every class the table has for this mode is there
    assert all(n > 0 for n, m in zip(counts, CLASSES[cfg]) if m > 0), (cfg, counts, CLASSES[cfg])
    nb = orcs[0].payload_bytes
    for f in np.flatnonzero(first >= 0):        # and no decode is a false one
        assert np.array_equal(refs[first[f]][f]["bytes"][:nb].astype(np.uint8), sent[f]), (cfg, f)
    return dict(bb=bb, sent=sent, refs=refs, first=first, counts=counts, nb=nb)


def _run(rx, ladder, bb, want_llr=True):
    F = bb.shape[0]
    rx.set_estimator_ladder(ladder)
    out = rx.receive(bb, want_llr=want_llr)
    out["rungs"] = rx.last_rungs(F)
    out["counters"] = rx.ladder_counters()
    return out


@pytest.mark.parametrize("cfg", [8, 11, 13])
def test_the_square_ladder_equals_the_oracle_of_the_first_window_that_decodes(cfg):
    """Retry rungs (frame list, compact rows, merge) against the CPU oracle in three modes and three window sizes; a frame no window decodes
    keeps the 21-window's failing record."""
    t = _prototypes(cfg)
    rx = _rx(cfg, max_batch=N24)
    out = _run(rx, SQUARE, t["bb"])
    rx.close()
    for f in range(N24):
        r = int(t["first"][f])
        ref = t["refs"][max(r, 0)][f]
        st = out["stats"][f]
        assert out["rungs"][f] == r, (f, out["rungs"][f], r)
        assert np.array_equal(out["payload"][f], ref["bytes"].astype(np.uint8)), (f, r)
        assert st["iterations_done"] == ref["iterations"] and st["crc"] == ref["crc"], (f, r, st, ref["iterations"], ref["crc"])
        assert np.float32(st["variance"]) == np.float32(ref["variance_f"]), (f, r)
        assert st["message_decoded"] == (1 if r >= 0 else 0), (f, r)
        if r >= 0:
            assert np.array_equal(out["payload"][f][: t["nb"]], t["sent"][f]), f
    by, frames = out["counters"]
    assert frames == N24 and tuple(by) == t["counts"][:4] and by.sum() == N24 - t["counts"][4]


def _composition(rx, bb, want_retries):
    """Every ladder of LADDERS on bb against its rungs run alone: frame f's payload, stats and LLR bytes are those of the first rung whose
    one-rung run decodes it, rung 0's when none does; the rungs and the counters say the same."""
    F = bb.shape[0]
    alone = {}
    for ladder in LADDERS:
        for win in ladder:
            if win not in alone:
                alone[win] = _run(rx, [win], bb)
                ok = alone[win]["stats"]["message_decoded"] != 0
                assert np.array_equal(alone[win]["rungs"], np.where(ok, 0, -1)), win
    for ladder in LADDERS:
        out = _run(rx, ladder, bb)
        ok = np.array([alone[win]["stats"]["message_decoded"] != 0 for win in ladder])
        first = np.where(ok.any(axis=0), ok.argmax(axis=0), -1)
        print("ladder", ladder, "frames by rung", [int((first == r).sum()) for r in range(len(ladder))], "none", int((first < 0).sum()))
        # a condition on the input, known from the CPU oracle for square windows: the 21-window leaves frames to retry, and the square ladder decodes
        # some of them. What the rectangular rungs make of them is printed above.
        if want_retries and ladder[0] == (21, 21):
            assert (~ok[0]).any() and (ladder != SQUARE or (first > 0).any()), (ladder, first)
        assert np.array_equal(out["rungs"], first), (ladder, out["rungs"], first)
        for f in range(F):
            src = alone[ladder[max(int(first[f]), 0)]]
            for key in ("payload", "stats", "llr_ldpc"):
                assert out[key][f].tobytes() == src[key][f].tobytes(), (ladder, f, int(first[f]), key)
        by, frames = out["counters"]
        assert frames == F and list(by) == [int((first == r).sum()) for r in range(4)], (ladder, by)


@pytest.mark.parametrize("cfg", [8, 11, 13])
def test_a_ladder_is_the_composition_of_its_rungs(cfg):
    """On the inputs whose populations the oracle gave above. Mode 8 decodes every frame by the 5-window, modes 11 and 13 leave frames to
    the last rung and to none."""
    rx = _rx(cfg, max_batch=N24)
    _composition(rx, _prototypes(cfg)["bb"], True)
    rx.close()


@pytest.mark.parametrize("cfg,explicit,threads,esn0", [(0, None, 1024, -31.0), (8, DY5, None, 20.0)], ids=["0-1024", "8-dy5"])
def test_a_ladder_is_the_composition_of_its_rungs_at_1024_threads_and_off_the_lattice(cfg, explicit, threads, esn0, monkeypatch):
    """The same construction with the delay set (0, 6, 12, 24, 40, 60) on the long BPSK frame at 1024 threads and on the Dy 5 geometry (the
    estimator's general path). Noise: on the CPU oracle's square windows mode 0's frames spread over the classes at -31 dB on this scale
    (21: 11, 9: 5, 5: 2, none: 6; at -26 dB and above the 21-window decodes nearly all, at -34 dB nearly none), the Dy 5 geometry's at mode 8's 20 dB
    (21: 20, 9: 1, 5: 3). So the 21-window leaves frames to retry and the square ladder decodes some of them, which is what is asked of
    the input; the populations of the rectangular rungs are what the one-rung runs give."""
    orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
    bb, _ = _two_path_frames(orc, N24, esn0)
    rx = _rx(cfg, threads, monkeypatch, max_batch=N24, explicit=explicit)
    assert _lds_fe(rx) == _carve(rx, threads or 512)
    _composition(rx, bb, True)
    rx.close()


# ---- D: more than 1024 frames, and the chunked host path ----------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1105, 1024])
def test_more_frames_than_one_pass_of_the_select_kernel(F):
    """Mode 13's 24 prototypes (half of them decoded by no window) tiled to F frames, frame i a copy of prototype (7 i + i // 24) % 24: failing
    frames on both sides of frame 1024, so the list of the second pass has to go behind the first's. Every frame's record equals its
    prototype's in one piece (LLRs asked for) and through the chunked host path (chunks of 512 frames: frame0 = 512 and 1024)."""
    t = _prototypes(13)
    rx = _rx(13, max_batch=F)
    proto = _run(rx, SQUARE, t["bb"])
    assert np.array_equal(proto["rungs"], t["first"])           # (what the square-ladder test holds to the oracle)
    rx.ladder_counters(reset=True)
    idx = (7 * np.arange(F) + np.arange(F) // N24) % N24
    assert (proto["rungs"][idx[:1024]] < 0).any() and (proto["rungs"][idx[1024:]] < 0).any() == (F > 1024)
    bb = t["bb"][idx]
    recount = [int((proto["rungs"][idx] == r).sum()) for r in range(4)]
    for want_llr in (True, False):
        out = rx.receive(bb, want_llr=want_llr)
        if not want_llr:
            hp = rx.host_path_last()
            chunk, nchunks = hp["chunk_frames"], hp["n_chunks"]
            assert nchunks > 1 and chunk * (nchunks - 1) < F <= chunk * nchunks, (chunk, nchunks)
        for key in ("payload", "stats") + (("llr_ldpc",) if want_llr else ()):
            same = [out[key][i].tobytes() == proto[key][idx[i]].tobytes() for i in range(F)]
            assert all(same), (F, want_llr, key, np.flatnonzero(~np.array(same))[:8])
        assert np.array_equal(rx.last_rungs(F), proto["rungs"][idx]), (F, want_llr)
        by, frames = rx.ladder_counters(reset=True)
        assert frames == F and list(by) == recount, (F, want_llr, by, recount)
    rx.close()

"""CPU tests of the host twin of the impulse blanker (include/mercury_blanker.h: mgpu_host_blank): against a numpy restatement of the rule
byte for byte on impulse frames and on the rule's edges, silent on noise-only and on faded noise-only frames, and on impulse frames the
oracle alone loses and decodes once the samples went through the twin."""
import ctypes as C

import numpy as np
import pytest

from blanker_ref import DEFAULT, DY5, MFSK, POINTS, block_len, cap_frames, decoded, hand_made, impulse_frames, np_blank
from oraclelib import Oracle

CASES = [(13, None), (8, None), (0, None), (MFSK, None), (8, DY5)]


def _same(cfg, explicit, frame, L, **prm):
    from mercury_amd import host_blank
    got, rep = host_blank(cfg, frame, explicit=explicit, **prm)
    want, marked, blanked = np_blank(frame, L, **{**DEFAULT, **prm})
    assert (rep["marked"], rep["blanked"]) == (marked, blanked), (rep, marked, blanked)
    assert got.tobytes() == want.tobytes()
    return got, rep


@pytest.mark.parametrize("cfg,explicit", CASES)
def test_twin_equals_the_numpy_restatement_on_impulse_frames(cfg, explicit):
    esn0, db, width = POINTS[cfg]
    t = impulse_frames(cfg, explicit, esn0, db, width, frames=4)
    orc, L = t["orc"], block_len(t["orc"])
    assert t["bb"].shape[1] == orc.frame_samples and L == 272
    total = 0
    for f in range(4):
        for prm in ({}, dict(guard=0), dict(guard=16), dict(threshold=12.0, max_share=0.5)):
            got, rep = _same(cfg, explicit, t["bb"][f], L, **prm)
            if not prm:
                total += rep["blanked"]
                assert rep["blanked"] == rep["marked"] > 0 and int((got == 0).sum()) >= rep["blanked"]
    print("mode %d %s: %d samples zeroed in 4 frames of %d" % (cfg, explicit, total, orc.frame_samples))


@pytest.mark.parametrize("cfg,explicit", CASES)
def test_twin_equals_the_numpy_restatement_on_the_rules_edges(cfg, explicit):
    from mercury_amd import host_blank, load_library
    orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
    L = block_len(orc)
    for name, frame in hand_made(orc).items():
        for prm in ({}, dict(guard=0), dict(guard=16)):
            got, rep = _same(cfg, explicit, frame, L, **prm)
        print("mode %d %s, %s: marked %d, blanked %d" % (cfg, explicit, name, rep["marked"], rep["blanked"]))
        if name in ("a NaN sample", "an inf sample", "impulses on the first and last sample", "impulses on both sides of a block border"):
            assert rep["blanked"] > 0, name
        if name == "a block of zeros":
            assert rep["marked"] == 0, name
    if not explicit:                                                      # in place: out may be in
        frame = hand_made(orc)["a NaN sample"]
        want, work = host_blank(cfg, frame)[0], frame.copy()
        lib = load_library()
        assert lib.mgpu_host_blank(int(cfg), None, None, work.ctypes.data_as(C.c_void_p), work.ctypes.data_as(C.c_void_p), None) == 0
        assert work.tobytes() == want.tobytes()


def test_a_frame_at_the_cap_is_blanked_and_one_above_it_is_returned():
    from mercury_amd import host_blank
    orc = Oracle(8, 50)
    at, over, cap = cap_frames(orc)
    got, rep = _same(8, None, at, block_len(orc), guard=0)
    assert rep == {"marked": cap, "blanked": cap} and int((got == 0).sum()) == cap
    got, rep = _same(8, None, over, block_len(orc), guard=0)
    assert rep == {"marked": cap + 1, "blanked": 0} and got.tobytes() == over.tobytes()
    assert host_blank(8, over, guard=0, max_share=0.126)[1]["blanked"] == cap + 1


@pytest.mark.parametrize("cfg,esn0", [(8, 6.0), (13, 14.0), (11, 10.0), (0, 6.0)])
def test_noise_only_frames_pass_untouched(cfg, esn0):
    t = impulse_frames(cfg, None, esn0, None, frames=16)
    for f in range(16):
        got, rep = _same(cfg, None, t["bb"][f], block_len(t["orc"]))
        assert rep["marked"] == 0 and got.tobytes() == t["bb"][f].tobytes(), (f, rep)


@pytest.mark.parametrize("fd", [1.0, 5.0])
@pytest.mark.parametrize("cfg,esn0", [(8, 12.0), (0, 6.0)])
def test_faded_noise_only_frames_pass_untouched(cfg, esn0, fd):
    """A Rayleigh-like gain of 1 Hz and 5 Hz Doppler (blanker_ref.fading_gain) on 16 noise-only frames at the Es/N0 of the mode's row in
    profiles/blanker.md: mode 8 at 12 dB, mode 0 at 6 dB. One level per symbol-length block follows the fade: nothing is marked. Not
    asserted here and recorded there: at 5 Hz mode 0's long frames are not entirely free of marks - frames 16 .. 31 of the 6 dB point hold
    one frame with 9 marked samples, and at 12 dB 2 of the first 16 frames have 11 and 9 (a sample or two of 13,056 above 24 medians
    where the gain climbs out of a null inside a block); no frame stops decoding for it. At 1 Hz there are none, and at threshold 12 every
    one of these points loses hundreds of samples."""
    t = impulse_frames(cfg, None, esn0, None, frames=16, fd=fd)
    for f in range(16):
        got, rep = _same(cfg, None, t["bb"][f], block_len(t["orc"]))
        assert rep["marked"] == 0 and got.tobytes() == t["bb"][f].tobytes(), (f, rep)


@pytest.mark.parametrize("cfg", [13, 11])
def test_impulse_frames_the_oracle_loses_decode_once_blanked(cfg):
    """25 dB one-sample impulses every 100 samples, mode 13 at 14 dB and mode 11 at 10 dB, 16 frames: the oracle alone decodes at most 2,
    on the twin's output at least 14, with the sent bits. Measured: 0 and 16 for both modes (profiles/blanker.md)."""
    from mercury_amd import host_blank
    esn0, db, width = POINTS[cfg]
    t = impulse_frames(cfg, None, esn0, db, width, frames=16)
    orc = t["orc"]
    plain = sum(decoded(orc, orc.rx(t["bb"][f]), t["bits"][f]) for f in range(16))
    fixed, zeroed = 0, 0
    for f in range(16):
        got, rep = host_blank(cfg, t["bb"][f])
        zeroed = max(zeroed, rep["blanked"])
        fixed += decoded(orc, orc.rx(got), t["bits"][f])
    print("mode %d at %.0f dB, %.0f dB impulses every 100 samples: the oracle alone decodes %d of 16, on blanked samples %d; at most %d samples "
          "zeroed per frame (cap %d)" % (cfg, esn0, db, plain, fixed, zeroed, orc.frame_samples // 8))
    assert plain <= 2 and fixed >= 14, (plain, fixed)


def test_library_exports_what_mercury_blanker_h_declares():
    import os
    import re
    from mercury_amd import BLANKER_DEFAULT, BLANKER_MODES, BLANKER_SYMBOLS, BlankerParams, load_library
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mercury_blanker.h")).read()
    for name, value in BLANKER_MODES.items():
        assert int(re.search(r"#define MGPU_BLANK_%s (\d+)" % name.upper(), text).group(1)) == value
    for word in ("NOT one of the reference's configurations", "mgpu_pool_", "mercury_stages.h", "captured graph", "max_batch * frame_samples * 16",
                 "synchroniser", "48 kHz", "no clipping mode", "no impulse source"):
        assert word in text, word                                         # the rule's limits are said where a caller reads them
    assert re.search(r"#define MGPU_BLANKER_PARAMS_DEFAULT \{24\.0, 4, 0\.125\}", text)
    assert BLANKER_DEFAULT == {"threshold": 24.0, "guard": 4, "max_share": 0.125} and C.sizeof(BlankerParams) == 24
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mgpu_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(BLANKER_SYMBOLS)
    lib = load_library()
    for name in declared:
        assert hasattr(lib, name), name


def test_refusals():
    from mercury_amd import MgpuError, host_blank
    frame = np.ones(Oracle(8, 50).frame_samples, np.complex128)
    for kw in (dict(threshold=1.5), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(guard=-1), dict(guard=17),
               dict(max_share=0.0), dict(max_share=0.6), dict(max_share=float("nan"))):
        with pytest.raises(MgpuError) as e:
            host_blank(8, frame, **kw)
        assert e.value.code == 1, kw                                      # MGPU_ERR_ARG
    with pytest.raises(MgpuError):
        host_blank(55, frame)                                             # no such mode
    with pytest.raises(MgpuError):
        host_blank(8, frame[:-1])
    assert host_blank(8, frame)[1] == {"marked": 0, "blanked": 0}

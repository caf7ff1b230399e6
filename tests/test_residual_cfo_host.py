"""CPU tests of the host twin of the pilot-aided residual carrier-offset correction (include/mercury_cfo.h: mgpu_host_cfo_pilots): against a
numpy restatement of the rule on the CPU oracle's cell grid, on grids the rule must pass through, for its accuracy on noisy frames, and on
offset frames the oracle alone loses and decodes once the samples are turned back by the twin's step."""
import numpy as np
import pytest

from oraclelib import Oracle
from residual_cfo_ref import (CASES, decode_fixture, decoded, derotate_samples, np_cfo_pilots, offset_frame, offsets_for, step_to_hz)


@pytest.mark.parametrize("cfg,explicit", CASES)
def test_twin_equals_the_numpy_restatement(cfg, explicit):
    from mercury_amd import host_cfo_pilots
    orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
    dy = (explicit or {}).get("Dy", 3)
    for k, f_hz in enumerate(offsets_for(explicit)):
        grid = orc.rx(offset_frame(orc, k, f_hz, 10.0)[0])["grid"]
        got, step = host_cfo_pilots(cfg, grid, explicit=explicit)
        want, want_step = np_cfo_pilots(orc, grid, dy)
        print("mode %d Dy %d: %+.1f Hz measured as %+.4f" % (cfg, dy, f_hz, step_to_hz(step)))
        assert step == want_step, (f_hz, step, want_step)
        assert got.tobytes() == want.tobytes(), (f_hz, np.abs(got - want).max())
        assert got[: orc.Nc].tobytes() == grid[: orc.Nc].tobytes()             # symbol 0 is the reference: sincos(-0.0) = (-0.0, 1.0)
        if f_hz != 0:
            assert got.tobytes() != grid.tobytes()
        assert abs(step_to_hz(step) - f_hz) < 0.5                              # (a plausibility check of the fixture; the accuracy test is below)


@pytest.mark.parametrize("cfg,explicit", CASES)
def test_grids_without_a_measurement_pass_through(cfg, explicit):
    from mercury_amd import host_cfo_pilots
    orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
    G = orc.Nsymb * orc.Nc
    zero = np.zeros(G, np.complex128)
    got, step = host_cfo_pilots(cfg, zero, explicit=explicit)
    assert step == 0.0 and got.tobytes() == zero.tobytes()
    grid = orc.rx(offset_frame(orc, 0, 2.0, 10.0)[0])["grid"].copy()
    pilots = np.flatnonzero(orc.frame_types() != 0)
    grid[pilots[len(pilots) // 2]] = complex(np.nan, 1.0)
    got, step = host_cfo_pilots(cfg, grid, explicit=explicit)
    assert step == 0.0 and got.tobytes() == grid.tobytes()
    want, want_step = np_cfo_pilots(orc, grid, (explicit or {}).get("Dy", 3))
    assert want_step == 0.0 and want.tobytes() == grid.tobytes()


@pytest.mark.parametrize("f_hz", [0.0, 2.0, 4.0])
def test_the_step_is_accurate_on_noisy_frames(f_hz):
    """Mode 8 at 2 dB, seed 77, frames 0 - 15: |step 12000 / (2 pi 272) - f| <= 0.15 Hz for every frame. Measured: 0.033 - 0.037 Hz rms,
    0.059 - 0.093 Hz at most; the bound is about 4 sigma."""
    from mercury_amd import host_cfo_pilots
    t = decode_fixture(f_hz)
    err = np.array([step_to_hz(host_cfo_pilots(8, ref["grid"])[1]) - f_hz for ref in t["ref"]])
    print("f = %.0f Hz: error rms %.4f Hz, largest %.4f Hz" % (f_hz, np.sqrt(np.mean(err * err)), np.abs(err).max()))
    assert (np.abs(err) <= 0.15).all(), err


def test_offset_frames_the_oracle_loses_decode_once_turned_back():
    """Mode 8 at 2 dB, 2 Hz: the oracle (21 x 21 window) decodes 0 of 16; with symbol s of the samples multiplied by the twin's
    exp(-j step s) at least 15. Measured: 0 and 16."""
    from mercury_amd import host_cfo_pilots
    t = decode_fixture(2.0)
    orc = t["orc"]
    plain = sum(decoded(orc, t["ref"][f], t["payload"][f]) for f in range(16))
    fixed = 0
    for f in range(16):
        _, step = host_cfo_pilots(8, t["ref"][f]["grid"])
        fixed += decoded(orc, orc.rx(derotate_samples(orc, t["bb"][f], step)), t["payload"][f])
    print("mode 8, 2 dB, 2 Hz: the oracle alone decodes %d of 16, turned back %d" % (plain, fixed))
    assert plain == 0 and fixed >= 15, (plain, fixed)


def test_library_exports_what_mercury_cfo_h_declares():
    import os
    import re
    from mercury_amd import CFO_MODES, CFO_SYMBOLS, load_library
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mercury_cfo.h")).read()
    for name, value in CFO_MODES.items():
        assert int(re.search(r"#define MGPU_CFO_%s (\d+)" % name.upper(), text).group(1)) == value
    for word in ("NOT one of the reference's configurations", "mgpu_pool_", "mercury_stages.h", "captured graph", "7.35 Hz", "4.4 Hz", "freq_offset"):
        assert word in text, word                                         # the rule's limits are said where a caller reads them
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mgpu_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(CFO_SYMBOLS)
    lib = load_library()
    for name in declared:
        assert hasattr(lib, name), name


def test_refusals():
    from mercury_amd import MgpuError, host_cfo_pilots
    with pytest.raises(MgpuError) as e:
        host_cfo_pilots(100, np.zeros(1200, np.complex128))
    assert e.value.code == 4                                         # MGPU_ERR_UNSUPPORTED: the MFSK modes have no pilots
    with pytest.raises(MgpuError):
        host_cfo_pilots(8, np.ones(7, np.complex128))

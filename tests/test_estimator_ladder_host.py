"""CPU tests of the rectangular LS estimate's host twin (include/mercury_estimator.h: mgpu_host_ls_estimate) - the same sums the
front-end kernel forms for one rung of an estimator ladder - against the CPU oracle (square windows: bit for bit) and against a numpy
restatement of the reference's estimator written here (rectangular windows, which the oracle cannot be configured for)."""
import ctypes as C

import numpy as np
import pytest

from oraclelib import Oracle, noise_amp_for

DY5 = dict(Dy=5, Nsymb=20)          # mode 8 on the reference's LOW_DENSITY pilot lattice: 20 symbols hold the codeword
CASES = [(0, None), (8, None), (11, None), (8, DY5)]


def _grid(cfg, explicit, window=21, frame=0):
    """(oracle, its result for one noisy two-path frame of the generator): the grid after the AGC is the estimator's input"""
    x = dict(explicit or {})
    x["ls_window"] = window
    orc = Oracle(cfg, 50, explicit=x)
    bb, _ = orc.gen_frame(5, frame, noise_amp_for(10.0), 1)
    return orc, orc.rx(bb)


@pytest.mark.parametrize("cfg,explicit", CASES)
@pytest.mark.parametrize("w", [1, 5, 9, 21])
def test_square_windows_equal_the_oracle_bit_for_bit(cfg, explicit, w):
    from mercury_amd import host_ls_estimate
    orc, ref = _grid(cfg, explicit, w)
    pilots = np.flatnonzero(orc.frame_types() != 0)
    want = (ref["H_noamp"] if orc.amp_restore else ref["H"])[pilots]
    got = host_ls_estimate(cfg, ref["grid"], w, w, explicit=explicit)
    assert got.size == orc.nPilots
    assert np.array_equal(got, want), (cfg, w, np.abs(got - want).max())


def _numpy_ls(orc, grid, width, height):
    """LS_channel_estimator (ofdm.cc:1315-1451) for a width x height window: per pilot the window's pilots in row-major order, x' = x / sum(x x)
    (the sum accumulated in that order, then ONE reciprocal), H = sum x' y in the same order. The reference forms x / sum as a complex
    division; the reciprocal's rounding is the only difference to it."""
    Nc, Ns = orc.Nc, orc.Nsymb
    types = orc.frame_types().reshape(Ns, Nc)
    vals = np.zeros((Ns, Nc))
    vals[types != 0] = orc.pilot_seq().real
    g = grid.reshape(Ns, Nc)
    out = []
    for i in range(Ns):
        for j in range(Nc):
            if not types[i, j]:
                continue
            k0, k1 = max(i - height // 2, 0), min(i + height // 2, Ns - 1)
            l0, l1 = max(j - width // 2, 0), min(j + width // 2, Nc - 1)
            cells = [(k, l) for k in range(k0, k1 + 1) for l in range(l0, l1 + 1) if types[k, l]]
            s = 0.0
            for k, l in cells:
                s += vals[k, l] * vals[k, l]
            inv = 1.0 / s
            h = 0j
            for k, l in cells:
                h += (vals[k, l] * inv) * g[k, l]
            out.append(h)
    return np.array(out)


@pytest.mark.parametrize("cfg,explicit", CASES)
@pytest.mark.parametrize("width,height", [(5, 21), (21, 5), (3, 11), (1, 21)])
def test_rectangular_windows_equal_a_numpy_restatement(cfg, explicit, width, height):
    """Tolerance 1e-12 max|H|: a window holds at most 150 terms whose products and sums round at 2.2e-16 each, an order of magnitude
    below the bound."""
    from mercury_amd import host_ls_estimate
    orc, ref = _grid(cfg, explicit)
    want = _numpy_ls(orc, ref["grid"], width, height)
    got = host_ls_estimate(cfg, ref["grid"], width, height, explicit=explicit)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), np.abs(got - want).max()
    if width != height:
        square = host_ls_estimate(cfg, ref["grid"], width, width, explicit=explicit)
        assert not np.array_equal(got, square)          # the height is really a parameter of its own


def test_an_even_side_is_incremented_like_the_reference_does():
    from mercury_amd import host_ls_estimate
    orc, ref = _grid(8, None)
    assert np.array_equal(host_ls_estimate(8, ref["grid"], 4, 20), host_ls_estimate(8, ref["grid"], 5, 21))


def test_argument_validation():
    from mercury_amd import load_library
    from mercury_amd.physical_layer import ExplicitParams
    lib = load_library()
    fn = lib.mgpu_host_ls_estimate
    grid = np.zeros(48 * 50, np.complex128)
    out = np.zeros(48 * 50, np.complex128)
    g, o = grid.ctypes.data, out.ctypes.data
    assert fn(8, None, 5, 21, g, o) == 0
    for w, h in ((23, 21), (22, 21), (0, 21), (-1, 21), (21, 0), (21, 23), (5, 22)):
        assert fn(8, None, w, h, g, o) == 1, (w, h)                    # MGPU_ERR_ARG
    assert fn(8, None, 5, 21, None, o) == 1 and fn(8, None, 5, 21, g, None) == 1
    assert fn(17, None, 5, 21, g, o) == 1                              # no such mode
    for cfg in (15, 16, 100, 101, 102):                                # zero-forcing and MFSK modes have no LS window
        assert fn(cfg, None, 5, 21, g, o) == 4, cfg                    # MGPU_ERR_UNSUPPORTED
    from mercury_amd import physical_layer
    assert fn(physical_layer.cfg_explicit(32, 8, 1, 0), None, 5, 21, g, o) == 4
    bad = ExplicitParams(0.0, 0, 0, 0, 0, 0, 64, 0, 0, 0, 0)           # Nc the kernels are not built for
    assert fn(8, C.byref(bad), 5, 21, g, o) == 4
    bad = ExplicitParams(0.0, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0)
    assert fn(8, C.byref(bad), 5, 21, g, o) == 1


def _geometries():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    frames = [(cfg, x) for cfg, x in mg.EXPLICIT_CASES if "Nsymb" in x or "Dy" in x]
    assert len(frames) == 6
    return [(cfg, None) for cfg in range(17)] + frames


def test_the_front_end_carve_fits_a_compute_unit_at_either_workgroup_size():
    """MERCURY_FE_THREADS=1024 cannot fail at launch on any mode or on the golden explicit geometries: the 1024-thread carve
    fits the 160 KB of a compute unit, as the 512-thread one does. mgpu_create takes 1024 threads by itself when the 512-thread carve is more
    than half of that (create.hip): the list of such geometries is part of the assertion - today there is none, so the 1024-thread
    kernels run under the variable only (tests/test_gpu_frontend_shapes.py)."""
    from mercury_amd import load_library
    fn = load_library().mgpu_frontend_lds_bytes
    lds_cu = 160 * 1024
    carve, by_default_1024 = {}, []
    for cfg, x in _geometries():
        orc = Oracle(cfg, 50, explicit=dict(x or {}))
        G = orc.Nsymb * orc.Nc
        b512, b1024 = fn(G, orc.nPilots, orc.nBits, 512), fn(G, orc.nPilots, orc.nBits, 1024)
        assert 16 * G + 16 * orc.nPilots < b512 <= lds_cu and b512 <= b1024 <= lds_cu, (cfg, x, b512, b1024)
        carve[(cfg, tuple(sorted((x or {}).items())))] = (b512, b1024)
        if b512 > lds_cu // 2:
            by_default_1024.append((cfg, x))
    assert by_default_1024 == []
    dy5 = (("Dy", 5), ("Nsymb", 20))
    assert [carve[k] for k in ((0, ()), (8, ()), (11, ()), (13, ()), (8, dy5))] == [(73632, 106400), (49920, 86784), (47616, 80384), (44416, 77184), (50816, 83584)]


def test_parse_ladder():
    from mercury_amd import parse_ladder
    assert parse_ladder("21x21,5x21") == [(21, 21), (5, 21)]
    assert parse_ladder("") == [] and parse_ladder(None) == []


def test_the_library_exports_the_header():
    import os
    import re
    from mercury_amd import ESTIMATOR_SYMBOLS, load_library
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mercury_estimator.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mgpu_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(ESTIMATOR_SYMBOLS)
    lib = load_library()
    for name in declared:
        assert hasattr(lib, name), name

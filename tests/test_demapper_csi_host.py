"""CPU tests of the channel-aware demapper's host twin (include/mercury_demapper.h: mgpu_host_demap_csi): against a numpy restatement of
the rule on the CPU oracle's stage outputs, against the plain demapper where the channel is flat, and on a two-path channel where the
plain demapper loses the frames and the weighted one decodes them."""
import numpy as np
import pytest

from conftest import SEED
from demapper_csi_ref import CASES, full_estimate, llr_src, llr_tol, np_demap_csi, same_bits, sym_src, two_path, two_path_twin
from oraclelib import Oracle, noise_amp_for


def _frames(cfg, explicit):
    orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
    return orc, [orc.rx(orc.gen_frame(SEED, f, noise_amp_for(10.0))[0]) for f in range(4)]


@pytest.mark.parametrize("cfg,explicit", CASES)
def test_the_restated_gathers_are_the_oracles(cfg, explicit):
    orc, refs = _frames(cfg, explicit)
    for ref in refs:
        assert np.array_equal(ref["syms"], ref["eq"][sym_src(orc)])
        assert np.array_equal(ref["llr_ldpc"][: orc.N], ref["llr_demod"][llr_src(orc)], equal_nan=True)


@pytest.mark.parametrize("cfg,explicit", CASES)
def test_twin_equals_the_numpy_restatement(cfg, explicit):
    from mercury_amd import host_demap_csi
    orc, refs = _frames(cfg, explicit)
    for f, ref in enumerate(refs):
        H = full_estimate(orc, ref)
        got, sigma2 = host_demap_csi(cfg, ref["grid"], H, explicit=explicit)
        want, want_sigma2 = np_demap_csi(orc, ref["grid"], H)
        assert got.shape == (orc.nBits,)
        assert sigma2 == want_sigma2, (f, sigma2, want_sigma2)
        assert got.dtype == want.dtype and same_bits(got, want), (cfg, f, np.nanmax(np.abs(got - want)))      # bit for bit, NaN where NaN
        if orc.amp_restore:                      # the weights matter: |h| is not 1 before restore_channel_amplitude
            assert not (np.abs(got - ref["llr_demod"]) <= llr_tol(ref["llr_demod"])).all()


@pytest.mark.parametrize("cfg,explicit", CASES)
def test_unit_channel_gives_the_plain_llrs_rescaled(cfg, explicit):
    """h = 1 on every cell and the oracle's equalised grid as the received one: the same distances, so the twin's LLRs are the plain
    llr_demod times variance_f / sigma2."""
    from mercury_amd import host_demap_csi
    orc, refs = _frames(cfg, explicit)
    for f, ref in enumerate(refs):
        got, sigma2 = host_demap_csi(cfg, ref["eq"], np.ones_like(ref["eq"]), explicit=explicit)
        want = ref["llr_demod"].astype(np.float64) * (np.float64(ref["variance_f"]) / sigma2)
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= llr_tol(want)).all(), (cfg, f, err.max())


@pytest.mark.parametrize("cfg,esn0,plain_most,csi_least", [(13, 15.0, 2, 30), (11, 8.0, 6, 24)])
def test_two_path_frames_the_plain_demapper_loses_decode_with_the_weights(cfg, esn0, plain_most, csi_least):
    """Measured with the numpy restatement: mode 13 at 15 dB 0 and 32 of 32 frames, mode 11 at 8 dB 2 and 28."""
    t = two_path(cfg, esn0)
    twin = two_path_twin(cfg, esn0)
    plain = int(t["plain_ok"].sum())
    csi = sum(int(np.array_equal(bits, t["bits"][f])) for f, (_, bits, _) in enumerate(twin))
    print("mode %d at %.0f dB: the oracle alone decodes %d of 32, the twin's LLRs %d" % (cfg, esn0, plain, csi))
    assert plain <= plain_most and csi >= csi_least, (plain, csi)


def test_library_exports_what_mercury_demapper_h_declares():
    import os
    import re
    from mercury_amd import DEMAPPER_SYMBOLS, DEMAPPERS, load_library
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mercury_demapper.h")).read()
    for name, value in DEMAPPERS.items():
        assert int(re.search(r"#define MGPU_DEMAP_%s (\d+)" % name.upper(), text).group(1)) == value
    for word in ("NOT one of the reference's configurations", "mgpu_pool_", "mercury_stages.h", "captured graph", "MGPU_ERR_TABLES"):
        assert word in text, word                                         # the rule's limits are said where a caller reads them
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mgpu_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(DEMAPPER_SYMBOLS)
    lib = load_library()
    for name in declared:
        assert hasattr(lib, name), name


def test_the_csi_carve_fits_every_mode_and_keeps_two_workgroups_in_the_bpsk_modes():
    """the carve the new kernels ask for (two more arrays in the work area) against a compute unit's 160 KB, at either workgroup size"""
    from mercury_amd import load_library
    lib = load_library()
    for cfg, explicit in [(c, None) for c in range(17)] + [(8, dict(Dy=5, Nsymb=20))]:
        orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
        G = orc.Nsymb * orc.Nc
        for threads in (512, 1024):
            plain = lib.mgpu_frontend_lds_bytes(G, orc.nPilots, orc.nBits, threads)
            csi = lib.mgpu_frontend_csi_lds_bytes(G, orc.nPilots, orc.nBits, threads)
            need = 16 * G + 16 * orc.nPilots + 16 * (orc.nPilots + 8) + 8 * orc.nPilots + 4 * orc.nData       # grid, Hp, two term arrays, the third, |h|^2
            assert plain <= csi <= 160 * 1024 and csi >= need, (cfg, threads, plain, csi, need)
            assert lib.mgpu_frontend_lds_workgroups(csi) >= (2 if threads == 512 else 1), (cfg, threads, csi)
            if G < 2400:                                                     # outside the BPSK modes the FFT work areas already cover the two arrays
                assert lib.mgpu_frontend_lds_workgroups(csi) == lib.mgpu_frontend_lds_workgroups(plain), (cfg, threads)


def test_refusals():
    from mercury_amd import MgpuError, host_demap_csi
    g = np.zeros(1200, np.complex128)
    with pytest.raises(MgpuError) as e:
        host_demap_csi(100, g, g + 1)
    assert e.value.code == 4                                         # MGPU_ERR_UNSUPPORTED: the MFSK modes have no channel estimate
    with pytest.raises(MgpuError):
        host_demap_csi(8, g, np.ones(7, np.complex128))

"""CPU tests of the front-end's form table (csrc/ls_rect.h, csrc/frontend.hip): which bit sets are forms, that each form has a kernel of
its own at either workgroup size, that a form's LDS carve is the plain, the CSI or the noise-map one by its CSI and NMAP bits alone - and
of the yardstick tests/test_gpu_frontend_form_order.py measures the kernels with, against the CPU oracle."""

import numpy as np
import pytest

import frontend_forms_ref as R
from frontend_forms_ref import CFO, CSI, NMAP, RECT, VALID_FORMS, WIENER
from oraclelib import FLAGS_RECEIVE_BYTE, Oracle

GEOMETRIES = [(c, None) for c in range(17)] + [(8, dict(Dy=5, Nsymb=20))]          # every OFDM mode and the low-density geometry


def _lib():
    from mercury_amd import load_library
    return load_library()


def test_thirteen_bit_sets_are_forms():
    assert len(VALID_FORMS) == 13 and len(set(VALID_FORMS)) == 13
    assert VALID_FORMS[0] == 0 and all(f & RECT for f in VALID_FORMS[1:])
    assert sum(1 for f in VALID_FORMS if not f & NMAP) == 9 and all(f & CSI for f in VALID_FORMS if f & NMAP)


@pytest.mark.parametrize("cfg,explicit", GEOMETRIES)
def test_a_forms_carve_follows_its_csi_and_nmap_bits_alone(cfg, explicit):
    lib = _lib()
    orc = Oracle(cfg, 50, explicit=dict(explicit or {}))
    G = orc.Nsymb * orc.Nc
    for threads in (512, 1024):
        geo = (G, orc.nPilots, orc.nBits, threads)
        plain, csi, nmap = lib.mgpu_frontend_lds_bytes(*geo), lib.mgpu_frontend_csi_lds_bytes(*geo), lib.mgpu_frontend_nmap_lds_bytes(*geo)
        assert 0 < plain <= csi <= nmap, (cfg, threads, plain, csi, nmap)
        for form in VALID_FORMS:
            want = nmap if form & NMAP else csi if form & CSI else plain
            assert lib.mgpu_frontend_form_lds_bytes(*geo, form) == want, (cfg, threads, form)
            for bit in (CFO, WIENER):                                        # (RECT: the plain form against the rectangular one)
                if form & RECT and form | bit in VALID_FORMS:
                    assert lib.mgpu_frontend_form_lds_bytes(*geo, form | bit) == want, (cfg, threads, form, bit)
        assert lib.mgpu_frontend_form_lds_bytes(*geo, RECT) == lib.mgpu_frontend_form_lds_bytes(*geo, 0)
        for form in range(32):
            if form not in VALID_FORMS:
                assert lib.mgpu_frontend_form_lds_bytes(*geo, form) == 0, (cfg, threads, form)


def test_the_carves_of_modes_0_and_8_in_bytes():
    """the figures csrc/frontend.hip and DESIGN.md 3.9 / 3.12 state, so that the comparison above does not stand on the old exports alone
    (they are the new function under other bit sets): (plain, CSI, noise map) at 512 and at 1024 threads"""
    lib = _lib()
    for cfg, want in ((0, {512: (73632, 79392, 80736), 1024: (106400, 106400, 106400)}), (8, {512: (49920,) * 3, 1024: (86784,) * 3})):
        orc = Oracle(cfg, 50)
        for threads, bytes_ in want.items():
            got = tuple(lib.mgpu_frontend_form_lds_bytes(orc.Nsymb * orc.Nc, orc.nPilots, orc.nBits, threads, form)
                        for form in (RECT | WIENER | CFO, RECT | CSI | CFO, RECT | CSI | NMAP | WIENER))
            assert got == bytes_, (cfg, threads, got)


def test_every_form_has_a_kernel_of_its_own_and_no_other_bit_set_has_one():
    lib = _lib()
    invalid = [f for f in range(32) if f not in VALID_FORMS]
    assert len(invalid) == 19
    for form in invalid + [32, 33, 1 << 31]:
        for threads in (512, 1024):
            assert lib.mgpu_frontend_form_kernel(threads, form) is None, (threads, form)      # (ctypes: a null pointer is None)
    kernels = [lib.mgpu_frontend_form_kernel(threads, form) for threads in (512, 1024) for form in VALID_FORMS]
    assert all(kernels) and len(set(kernels)) == 26, kernels
    for form in VALID_FORMS:
        for threads in (0, 64, 256, 2048):
            assert lib.mgpu_frontend_form_kernel(threads, form) is None, (threads, form)


@pytest.mark.parametrize("cfg", [0, 8])
def test_the_plain_tail_restatement_equals_the_oracle(cfg):
    """frontend_forms_ref.plain_tail - what every form reports as variance and SNR variance, and the plain demapper's LLRs - on the oracle's
    own grid and full estimate against the oracle's own outputs, bit for bit: the GPU test's yardstick for them is held to the reference."""
    orc = R.D.oracle(cfg)
    for frame in R.frames(cfg):
        ref = orc.rx(frame, FLAGS_RECEIVE_BYTE)
        t = R.plain_tail(orc, ref["grid"], ref["H_noamp"] if orc.amp_restore else ref["H"])
        assert np.float64(t["variance"]).tobytes() == np.float64(ref["variance"]).tobytes(), (t["variance"], ref["variance"])
        assert np.float32(t["variance"]).tobytes() == np.float32(ref["variance_f"]).tobytes()
        assert R.same_bits(t["llr_demod"], ref["llr_demod"])
        assert R.same_bits(t["llr_ldpc"], ref["llr_ldpc"][: orc.N])
        assert abs(t["snr_db"] - ref["snr_db"]) <= 2e-5 * max(1.0, abs(ref["snr_db"])), (t["snr_db"], ref["snr_db"])

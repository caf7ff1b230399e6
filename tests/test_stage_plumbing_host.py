"""CPU tests of the plumbing the optional stages share: the host twins' geometry cache (mercury_amd/csrc/geometry_cache.hpp) through every
twin family and under the sanitizers, the one parser behind parse_demapper / parse_blanker / parse_excisor, the binding's checked
call, and what the wideband IQ stages' twins raise where they refuse a call. The parsers' results and every error text are literals
recorded from the binding as it was before these pieces were shared."""
import os
import subprocess

import numpy as np
import pytest

import mercury_amd as M
from mercury_amd import MgpuError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = 50

# ---- 1. the cache's key: geometry A, then B, then A ---------------------------------------------------------------------------------
# The modes with the shortest frames: 16 (9 symbols, zero-forcing) for the twins that take it, 13 (12 symbols) for those that need the LS
# estimator. A is 8 symbols at Dy = 3 with the reference's pilot seed and boost, spelt out; B differs from A in exactly one field. Both modes
# take 8 and 9 symbols at Dy = 3 and 8 symbols at Dy = 5.
A = {"Dy": 3, "Nsymb": 8, "pilot_seed": 0, "pilot_boost": 1.33}
B_FIELDS = {"Dy": 5, "Nsymb": 9, "pilot_seed": 7, "pilot_boost": 2.0}
NOFDM = 272


def _grid(explicit, seed):
    rng = np.random.default_rng(seed)
    n = explicit["Nsymb"] * NC
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def _ls(cfg, ex):
    return (M.host_ls_estimate(cfg, _grid(ex, 1), 5, 3, explicit=ex),)


def _wiener(cfg, ex):
    return (M.host_wiener_estimate(cfg, _grid(ex, 2), explicit=ex),)


def _csi(cfg, ex):
    return M.host_demap_csi(cfg, _grid(ex, 3), _grid(ex, 4) + 2.0, explicit=ex)


def _nmap(cfg, ex):
    return M.host_demap_nmap(cfg, _grid(ex, 5), _grid(ex, 6) + 2.0, explicit=ex)


def _cfo(cfg, ex):
    return M.host_cfo_pilots(cfg, _grid(ex, 7), explicit=ex)


def _blank(cfg, ex):
    rng = np.random.default_rng(8)
    n = ex["Nsymb"] * NOFDM
    frame = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    frame[::97] *= 40.0                                                    # impulses: the blanker has something to do
    out, rep = M.host_blank(cfg, frame, explicit=ex)
    return out, np.array([rep["marked"], rep["blanked"]])


# twin family -> (mode, call, the fields its output depends on). The pilots' places follow Dy and Nsymb, their signs the seed, their
# amplitude the boost: the LS and Wiener weights and the demappers' sigma2 read all of them. The carrier-offset twin reads the pilots' places
# and signs, not their amplitude. The blanker reads the frame's length alone.
FAMILIES = {
    "host_ls_estimate": (13, _ls, {"Dy", "Nsymb", "pilot_seed", "pilot_boost"}),
    "host_wiener_estimate": (13, _wiener, {"Dy", "Nsymb", "pilot_seed", "pilot_boost"}),
    "host_demap_csi": (16, _csi, {"Dy", "Nsymb", "pilot_seed", "pilot_boost"}),
    "host_demap_nmap": (13, _nmap, {"Dy", "Nsymb", "pilot_seed", "pilot_boost"}),
    "host_cfo_pilots": (16, _cfo, {"Dy", "Nsymb", "pilot_seed"}),
    "host_blank": (16, _blank, {"Nsymb"}),
}


def _bytes(result):
    return [(np.asarray(v).shape, np.asarray(v).tobytes()) for v in result]


@pytest.mark.parametrize("field", sorted(B_FIELDS))
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_twin_cache_is_keyed_by_every_explicit_field(family, field):
    cfg, call, depends = FAMILIES[family]
    b = dict(A, **{field: B_FIELDS[field]})
    first, second, third = _bytes(call(cfg, A)), _bytes(call(cfg, b)), _bytes(call(cfg, A))
    assert third == first, "%s: A after B (%s) is not A" % (family, field)
    if field in depends:
        assert second != first, "%s: %s = %r gave A's result" % (family, field, B_FIELDS[field])


# ---- 2. the cache template under the sanitizers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitizers", ["address,undefined", "thread"])
def test_geometry_cache_is_clean_under_the_sanitizers(tmp_path, sanitizers):
    """tests/cpp/geometry_cache_sanitize.cpp, mercury_amd/csrc/tables.cpp and the LDPC table blob built as one stand-alone program and run on
    the CPU: the slot's rule on one thread, then four threads that alternate two geometries"""
    from mercury_amd import build as b
    blob_c, blob_o, exe = str(tmp_path / "ldpc_blob.c"), str(tmp_path / "ldpc_blob.o"), str(tmp_path / "geometry_cache_sanitize")
    b._write_blob_c(blob_c)
    subprocess.run(["gcc", "-O1", "-c", blob_c, "-o", blob_o], check=True)
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=" + sanitizers, "-fno-sanitize-recover=all", "-ffp-contract=off", "-pthread",
                    "-I", os.path.join(ROOT, "mercury_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "geometry_cache_sanitize.cpp"),
                    os.path.join(ROOT, "mercury_amd", "csrc", "tables.cpp"), blob_o, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "geometry cache: clean" in out.stdout


# ---- 3. the three parsers ------------------------------------------------------------------------------------------------------------------
PARSED = [
    ("parse_demapper", "nmap", ("nmap", {"dead_band": 2.0, "smooth": 1})),
    ("parse_demapper", "maxlog", ("maxlog", None)),
    ("parse_demapper", "csi", ("csi", None)),
    ("parse_demapper", "nmap:", ("nmap", {"dead_band": 2.0, "smooth": 1})),
    ("parse_demapper", "nmap:band=3.5,smooth=2", ("nmap", {"dead_band": 3.5, "smooth": 2})),
    ("parse_blanker", "median", ("median", {"threshold": 24.0, "guard": 4, "max_share": 0.125})),
    ("parse_blanker", "off", ("off", None)),
    ("parse_blanker", "median:", ("median", {"threshold": 24.0, "guard": 4, "max_share": 0.125})),
    ("parse_blanker", "median:thr=30,guard=2,share=0.25", ("median", {"threshold": 30.0, "guard": 2, "max_share": 0.25})),
    ("parse_excisor", "welch", ("welch", {"threshold": 12.0, "guard": 1, "max_bins": 16})),
    ("parse_excisor", "off", ("off", None)),
    ("parse_excisor", "welch:", ("welch", {"threshold": 12.0, "guard": 1, "max_bins": 16})),
    ("parse_excisor", "welch:thr=9.5,guard=2,bins=8", ("welch", {"threshold": 9.5, "guard": 2, "max_bins": 8})),
]
REFUSED = [
    ("parse_demapper", "nmap:foo=1", "demapper nmap: band=B and smooth=W are what it takes, not 'foo=1'"),            # an unknown key
    ("parse_demapper", "csi:band=2", "demapper: one of maxlog, csi, nmap, nmap with :band=B,smooth=W"),               # a mode that takes none
    ("parse_demapper", "bogus", "demapper: one of maxlog, csi, nmap, nmap with :band=B,smooth=W"),                    # an unknown mode
    ("parse_blanker", "median:foo=1", "blanker median: thr=T, guard=G and share=S are what it takes, not 'foo=1'"),
    ("parse_blanker", "off:thr=2", "blanker: off, or median with :thr=T,guard=G,share=S"),
    ("parse_blanker", "bogus", "blanker: off, or median with :thr=T,guard=G,share=S"),
    ("parse_excisor", "welch:foo=1", "excisor welch: thr=T, guard=G and bins=B are what it takes, not 'foo=1'"),
    ("parse_excisor", "off:thr=2", "excisor: off, or welch with :thr=T,guard=G,bins=B"),
    ("parse_excisor", "bogus", "excisor: off, or welch with :thr=T,guard=G,bins=B"),
]


@pytest.mark.parametrize("parser,text,want", PARSED)
def test_parsers_return_what_they_returned(parser, text, want):
    got = getattr(M, parser)(text)
    assert got == want
    assert got[1] is None or [type(v) for v in got[1].values()] == [type(v) for v in want[1].values()]


@pytest.mark.parametrize("parser,text,message", REFUSED)
def test_parsers_refuse_in_the_same_words(parser, text, message):
    with pytest.raises(ValueError) as e:
        getattr(M, parser)(text)
    assert str(e.value) == message


def test_parsers_leave_the_defaults_alone():
    for parser, text, defaults in (("parse_demapper", "nmap:band=9", M.physical_layer.NMAP_DEFAULT), ("parse_blanker", "median:thr=99", M.physical_layer.BLANKER_DEFAULT),
                                   ("parse_excisor", "welch:thr=99", M.physical_layer.EXCISOR_DEFAULT)):
        before = dict(defaults)
        getattr(M, parser)(text)
        assert defaults == before, parser


# ---- 4. what a refused host call raises ---------------------------------------------------------------------------------------------------
MFSK = 100
Z = np.zeros(10, np.complex128)


def _mode8_frame():
    info = M.physical_layer.Info()
    assert M.load_library().mgpu_host_mode_info(8, 0, M.physical_layer.C.byref(info)) == 0
    return np.zeros(info.frame_samples, np.complex128)


CALLS = [
    ("wiener_select on MFSK", lambda: M.host_wiener_select(MFSK, Z, [({}, None)]), "mgpu_host_wiener_select failed (4)", 4),
    ("wiener_bank_thresholds on MFSK", lambda: M.host_wiener_bank_thresholds(MFSK, [({}, None)]), "mgpu_host_wiener_bank_thresholds failed (4)", 4),
    ("wiener_estimate on MFSK", lambda: M.host_wiener_estimate(MFSK, Z), "mgpu_host_wiener_estimate failed (4)", 4),
    ("wiener_estimate, design out of range", lambda: M.host_wiener_estimate(8, Z, design={"snr_db": 99.0}), "mgpu_host_wiener_estimate failed (1)", 1),
    ("wiener_tables on MFSK", lambda: M.host_wiener_tables(MFSK), "mgpu_host_wiener_tables failed (4)", 4),
    # host_ls_estimate has always raised without a code
    ("ls_estimate on MFSK", lambda: M.host_ls_estimate(MFSK, Z, 5, 5), "mgpu_host_ls_estimate failed (4)", None),
    ("ls_estimate, window of 0", lambda: M.host_ls_estimate(8, Z, 0, 5), "mgpu_host_ls_estimate failed (1)", None),
    ("demap_csi on MFSK", lambda: M.host_demap_csi(MFSK, Z, Z), "mgpu_host_demap_csi failed (4)", 4),
    ("demap_csi, Nc = 49", lambda: M.host_demap_csi(8, Z, Z, explicit={"Nc": 49}), "mgpu_host_demap_csi failed (4)", 4),
    ("demap_nmap on MFSK", lambda: M.host_demap_nmap(MFSK, Z, Z), "mgpu_host_demap_nmap failed (4)", 4),
    ("demap_nmap, dead_band below 1", lambda: M.host_demap_nmap(8, Z, Z, dead_band=0.5), "mgpu_host_demap_nmap failed (1)", 1),
    ("cfo_pilots on MFSK", lambda: M.host_cfo_pilots(MFSK, Z), "mgpu_host_cfo_pilots failed (4)", 4),
    ("cfo_pilots, wrong-sized grid", lambda: M.host_cfo_pilots(8, Z), "host_cfo_pilots: the grid must have one entry per cell (1200)", None),
    ("blank, threshold below 2", lambda: M.host_blank(8, _mode8_frame(), threshold=1.0), "mgpu_host_blank failed (1)", 1),
    ("blank, Nc = 49", lambda: M.host_blank(8, _mode8_frame(), explicit={"Nc": 49}), "mgpu_host_blank failed (4)", 4),
    ("blank, wrong-sized frame", lambda: M.host_blank(8, Z), "host_blank: the frame must have frame_samples (6528) samples", 1),
    ("excise, threshold below 2", lambda: M.host_excise(np.zeros(100), 1500.0, threshold=1.0), "mgpu_host_excise failed (1)", 1),
    ("excise, carrier NaN", lambda: M.host_excise(np.zeros(100), float("nan")), "mgpu_host_excise failed (1)", 1),
    ("llr_combine, rows no multiple of D", lambda: M.host_llr_combine(np.zeros((3, 1600), np.float32), D=2), "mgpu_host_llr_combine refused the groups (1)", 1),
]


@pytest.mark.parametrize("what,call,message,code", CALLS, ids=[c[0] for c in CALLS])
def test_refused_host_calls_raise_what_they_raised(what, call, message, code):
    with pytest.raises(MgpuError) as e:
        call()
    assert str(e.value) == message
    assert e.value.code == code


# ---- 5. what a refused twin call of the wideband IQ stages raises ---------------------------------------------------------------------------
# The smallest shapes: the blanker at B = 64, the corrector at B = 256, the scanner at N = 256 (H = 128) and two blocks per line, the tuner
# at D = 1 and four symbols. Every text and code below was recorded from the binding and the library of the commit before the stages'
# call checks and the two block twins' Python halves were shared.
WB, QC, SC = np.zeros(128, np.complex64), np.zeros(512, np.complex64), np.zeros(512, np.complex64)
TU = np.zeros(M.tune_samples(1, 4), np.complex128)
T6 = np.zeros(6)


def _wb(x=WB, D=4, **kw):
    return M.host_wblank_process(x, D, block=64, **kw)


def _qc(x=QC, D=4, **kw):
    return M.host_iqc_process(x, D, block=256, **kw)


def _sc(x=SC, D=4, **kw):
    return M.host_scan_process(x, D, log2n=8, blocks_per_line=2, **kw)


def _tu(x=TU, D=1, **kw):
    return M.host_tune_process(x, D, [(0, 0, 1.0)], symbols=4, search=2, taps=M.host_chan_design(1, 8), **kw)


def _twin_calls(name, twin, x, block, grid, **kw):
    """the refusals every twin with a position has, for an input x of two grid steps: (what, call)"""
    assert len(x) == 2 * grid
    return [(name + ", unknown format number", lambda: twin(fmt=7, **kw)),
            (name + ", n_in no multiple of the block", lambda: twin(x[: block + 1], **kw)),
            (name + ", position off the block grid", lambda: twin(position=grid // 2, **kw)),
            (name + ", position past 2^62", lambda: twin(position=2 ** 62 + grid, **kw)),
            (name + ", the call ends past 2^62", lambda: twin(position=2 ** 62 - grid, **kw)),            # len(x) = 2 grid
            (name + ", D = 0", lambda: twin(D=0, **kw)),
            (name + ", D = 65", lambda: twin(D=65, **kw)),
            (name + ", wrong struct_size", lambda: twin(struct_size=20, **kw))]


TWIN_CALLS = (_twin_calls("wblank", _wb, WB, 64, 64) + _twin_calls("iqc", _qc, QC, 256, 256)
              + _twin_calls("iqc with state", _qc, QC, 256, 256, state=T6) + _twin_calls("scan", _sc, SC, 128, 256)
              + [("tune, unknown format number", lambda: _tu(fmt=7)), ("tune, n_in one too many", lambda: _tu(np.zeros(len(TU) + 1, np.complex128))),
                 ("tune, D = 0", lambda: _tu(D=0)), ("tune, D = 65", lambda: _tu(D=65)), ("tune, wrong struct_size", lambda: _tu(struct_size=20))])
TWIN_RAISES = {"wblank": "mgpu_host_wblank_process: bad argument", "iqc": "mgpu_host_iqc_process: bad argument",
               "iqc with state": "mgpu_host_iqc_continue: bad argument", "scan": "mgpu_host_scan_process: bad argument",
               "tune": "mgpu_host_tune_process: bad argument"}
STATE_CALLS = [("state of 5", np.zeros(5)), ("state of float32", np.zeros(6, np.float32)), ("state a list", [0.0] * 6),
               ("state not contiguous", np.zeros(12)[::2])]


def test_the_twins_take_the_smallest_good_calls():
    """what the refusals below change one argument of"""
    assert len(_wb()[1]) == 2 and len(_qc()[1]) == 2 and len(_qc(state=T6.copy())[1]) == 2 and len(_sc()[0]) == 2 and len(_tu()) == 1


@pytest.mark.parametrize("what,call", TWIN_CALLS, ids=[c[0] for c in TWIN_CALLS])
def test_refused_twin_calls_raise_what_they_raised(what, call):
    with pytest.raises(MgpuError) as e:
        call()
    assert str(e.value) == TWIN_RAISES[what.split(",")[0]]
    assert e.value.code == 1


@pytest.mark.parametrize("what,state", STATE_CALLS, ids=[c[0] for c in STATE_CALLS])
def test_a_wrong_shaped_state_raises_what_it_raised(what, state):
    with pytest.raises(MgpuError) as e:
        _qc(state=state)
    assert str(e.value) == "state: a contiguous float64 array of 6"
    assert e.value.code == 1

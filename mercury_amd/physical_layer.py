"""ctypes binding of the C-ABI in include/*.h; the functions' prototypes and the loader are in abi.py.

This is only a thin binding: every computation happens in the HIP library
(``mercury_amd/libmercury_gpu.so``). There is NO CPU fallback — if the library is missing or no
GPU is visible, constructing :class:`RxPhy` raises.

Naming follows the reference's physical layer (source/physical_layer/telecom_system.cc): a
*frame* is one LDPC codeword worth of OFDM symbols for one ``CONFIG_n`` (0..16) or ``ROBUST_n``
(100..102, MFSK) mode, ``receive`` runs
the span of ``receive_byte`` after synchronisation (telecom_system.cc:1132-1345) on a batch of
frames, ``ldpc_decode`` is ``cl_ldpc::decode`` (ldpc.h:90) on a batch of LLR vectors.
"""
import ctypes as C
import math

import numpy as np

from .abi import LIB_PATH, load_library, names  # noqa: F401  (LIB_PATH and load_library are part of this module's surface)

DEC_GBF, DEC_SPA, DEC_MINSUM, DEC_SPA_FAST = 0, 1, 2, 3
EST_ZF, EST_LS = 0, 1


def _checked(fn, *args, what="failed"):
    """fn(*args) of the library; a status other than 0 raises MgpuError("<the function's name> <what> (<status>)") with the status as its code"""
    rc = fn(*args)
    if rc != 0:
        raise MgpuError("%s %s (%d)" % (fn.__name__, what, rc), rc)


def _twin(fn, *args, code=None):
    """fn(*args) of a host twin, which has no context to leave a reason in: a status other than 0 raises
    MgpuError("<the function's name>: bad argument") with `code` as its code"""
    if fn(*args) != 0:
        raise MgpuError("%s: bad argument" % fn.__name__, code)


def _explicit_struct(explicit):
    if not explicit:
        return None
    seeds = any(k in explicit for k in ("pilot_seed", "scrambler_seed", "preamble_seed"))
    return ExplicitParams(float(explicit.get("pilot_boost", 0.0)), int(explicit.get("ls_window", 0)), 1 if seeds else 0,
                          int(explicit.get("pilot_seed", 0)), int(explicit.get("scrambler_seed", 0)), int(explicit.get("preamble_seed", 1)),
                          int(explicit.get("Nc", 0)), int(explicit.get("Nfft", 0)), int(explicit.get("Dx", 0)), int(explicit.get("Dy", 0)),
                          int(explicit.get("Nsymb", 0)))


def _explicit_ref(explicit):
    """`explicit` (a dict as RxPhy takes it, or None) as the mgpu_explicit_params pointer the library takes"""
    xp = _explicit_struct(explicit)
    return C.byref(xp) if xp is not None else None


def _written(call, *probes):
    """how many entries of each output a twin writes for the geometry at hand: call(NaN-filled arrays of the given (size, dtype)) once,
    count what is no NaN any more"""
    arrays = [np.full(n, np.nan, dtype) for n, dtype in probes]
    call(*arrays)
    return [int(np.count_nonzero(~np.isnan(a.real))) for a in arrays]


def _parse_spec(text, what, modes, mode, defaults, keys, usage, takes):
    """"NAME" or "MODE:key=value,..." (the tools' --demapper, --blanker, --excisor) -> (name, None), or (mode, the defaults with what is
    given) for the one mode that takes parameters. keys: {key: (field of defaults, its type)}"""
    name, _, rest = str(text).partition(":")
    if name not in modes or (rest and name != mode):
        raise ValueError("%s: %s" % (what, usage))
    if name != mode:
        return name, None
    prm = dict(defaults)
    for item in filter(None, rest.split(",")):
        key, _, value = item.partition("=")
        if key not in keys:
            raise ValueError("%s %s: %s what it takes, not %r" % (what, mode, takes, item))
        field, kind = keys[key]
        prm[field] = kind(value)
    return name, prm


def _params(struct, defaults, given):
    """a parameter struct of the library from the values given, in the order of its fields; None: the field's default"""
    return struct(*[kind(defaults[field] if value is None else value) for (field, kind), value in zip(struct._fields_, given)])


class _Handle:
    """what owns one handle of the library, self.h, made by self.lib: close() releases it once with the function named by _destroy, and so
    does the collection of the object"""
    _destroy = None

    def _release(self):
        getattr(self.lib, self._destroy)(self.h)

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self._release()
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Config(C.Structure):
    _fields_ = [("cfg", C.c_int), ("max_iters", C.c_int), ("decoder", C.c_int), ("agc", C.c_int),
                ("variance_source", C.c_int), ("device", C.c_int), ("max_batch", C.c_int),
                ("minsum_alpha", C.c_float), ("mfsk_ctrl_mode", C.c_int), ("test_puncture_nBits", C.c_int)]


INFO_FIELDS = ("cfg M bits_per_symbol K P N Nsymb Nc Nfft Ngi Nofdm nData nBits nPilots nVirtual nReal "
               "bit_blk tf_blk preamble_nsymb estimator amp_restore ls_window Cwidth Vwidth E "
               "payload_bytes payload_stride frame_samples mfsk_M mfsk_nStreams active_nsymb active_nbits").split()


class ExplicitParams(C.Structure):    # mgpu_explicit_params
    _fields_ = [("pilot_boost", C.c_float), ("ls_window", C.c_int), ("seeds_set", C.c_int), ("pilot_seed", C.c_uint),
                ("scrambler_seed", C.c_uint), ("preamble_seed", C.c_uint), ("Nc", C.c_int), ("Nfft", C.c_int), ("Dx", C.c_int), ("Dy", C.c_int), ("Nsymb", C.c_int)]


class Info(C.Structure):
    _fields_ = [(n, C.c_int) for n in INFO_FIELDS]


class Taps(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in "grid H eq syms llr_demod llr_ldpc variance agc_gain cycles".split()]


class ReceiveConfig(C.Structure):
    _fields_ = [("carrier_hz", C.c_double), ("time_sync_trials_max", C.c_int), ("use_last_good_time_sync", C.c_int),
                ("use_last_good_freq_offset", C.c_int), ("coarse_freq_sync_enabled", C.c_int)]


class TransmitConfig(C.Structure):     # include/mercury_tx.h
    _fields_ = [("carrier_hz", C.c_double), ("carrier_amplitude", C.c_double), ("output_power_watt", C.c_double),
                ("preamble_papr_cut", C.c_double), ("data_papr_cut", C.c_double), ("start_sample", C.c_uint64),
                ("message_location", C.c_int), ("phase_continuous", C.c_int)]


FIRST_MESSAGE, MIDDLE_MESSAGE, FLUSH_MESSAGE = 0, 1, 2
SINGLE_MESSAGE, NO_FILTER_MESSAGE, BATCH_MESSAGE = 3, 4, 16

LINK_STATE_DTYPE = np.dtype([("delay_of_last_decoded_message", "<i4"), ("freq_offset_of_last_decoded_message", "<f8"),
                             ("mfsk_search_start", "<i4"), ("fixed_delay_plus_one", "<i4")], align=True)
RECEIVE_STATS_DTYPE = np.dtype([("iterations_done", "<i4"), ("crc", "<i4"), ("all_zeros", "<i4"), ("message_decoded", "<i4"),
                                ("snr_db", "<f8"), ("delay", "<i4"), ("sync_trials", "<i4"), ("freq_offset", "<f8"),
                                ("coarse_metric", "<f8"), ("frame_overflow_symbols", "<i4"), ("mean_H", "<f8"),
                                ("signal_strength_dbm", "<f8")], align=True)

STATS_DTYPE = np.dtype([("iterations_done", "<i4"), ("crc", "<i4"), ("all_zeros", "<i4"),
                        ("message_decoded", "<i4"), ("variance", "<f4"), ("snr_db", "<f4")])

EXPORTED_SYMBOLS = names("mercury_gpu.h", "mercury_shm.h", "mercury_rxloop.h", "mercury_stages.h", "mercury_tx.h", "mercury_pool.h")


# ---- rectangular LS windows and the estimator ladder (include/mercury_estimator.h) -------------------------------
ESTIMATOR_SYMBOLS = names("mercury_estimator.h")
LADDER_MAX = 4
RUNG_LS, RUNG_WIENER = 0, 1
WIENER_DESIGN_DEFAULT = dict(tau_min_us=-333.33, tau_max_us=2333.33, doppler_hz=0.5, snr_db=0.0)


class LsWindow(C.Structure):      # mgpu_ls_window
    _fields_ = [("width", C.c_int), ("height", C.c_int)]


class WienerDesign(C.Structure):  # mgpu_wiener_design
    _fields_ = [("tau_min_us", C.c_double), ("tau_max_us", C.c_double), ("doppler_hz", C.c_double), ("snr_db", C.c_double)]


class EstimatorRung(C.Structure):  # mgpu_estimator_rung
    _fields_ = [("kind", C.c_int), ("window", LsWindow), ("design", WienerDesign)]


def _wiener_design(design):
    d = dict(WIENER_DESIGN_DEFAULT)
    for k, v in (design or {}).items():
        if k not in d:
            raise MgpuError("a Wiener design has %s, not %r" % (sorted(d), k))
        d[k] = float(v)
    return WienerDesign(d["tau_min_us"], d["tau_max_us"], d["doppler_hz"], d["snr_db"])


def parse_ladder(text):
    """'21x21,5x21' -> [(21, 21), (5, 21)] (width = carriers, height = symbols); '' or None -> []. A Wiener rung (include/mercury_estimator.h:
    MGPU_RUNG_WIENER) is 'wiener' or 'wiener:tau=-333/2333,fd=0.5,snr=5' (delay bounds in us, Doppler in Hz, design SNR in dB; what is left
    out keeps its default) -> ("wiener", {the fields given, named as mgpu_wiener_design's}). A Wiener rung that chooses its design per
    frame (include/mercury_wiener_bank.h) is 'bank:tau=-333/333|-333/1000|-333/2333,fd=0.5,snr=5' with an optional 'rho=0.9|0.6': the
    intervals in ascending width, one fd / snr for every design -> ("bank", {tau: [(min, max), ...], doppler_hz, snr_db, rho: [...]})."""
    if not text:
        return []
    rungs = []
    for item in text.split(","):
        item = item.strip().lower()
        if rungs and isinstance(rungs[-1][1], dict) and "=" in item and "x" not in item.split("=")[0] and not item.startswith(("wiener", "bank")):
            key, value = item.split("=", 1)          # a further field of the Wiener rung before it: the fields are comma-separated too
        elif item.startswith("bank"):
            if not item.startswith("bank:") or "=" not in item:
                raise MgpuError("a bank rung is 'bank:tau=MIN/MAX|MIN/MAX|...,fd=HZ,snr=DB,rho=R|R', not %r" % item)
            rungs.append(("bank", {}))
            key, value = item[len("bank:"):].split("=", 1)
        elif item.startswith("wiener"):
            rungs.append(("wiener", {}))
            if item == "wiener":
                continue
            if not item.startswith("wiener:") or "=" not in item:
                raise MgpuError("a Wiener rung is 'wiener' or 'wiener:tau=MIN/MAX,fd=HZ,snr=DB', not %r" % item)
            key, value = item[len("wiener:"):].split("=", 1)
        else:
            rungs.append(tuple(int(v) for v in item.split("x")))
            continue
        d = rungs[-1][1]
        if rungs[-1][0] == "bank" and key in ("tau", "rho"):
            if key == "tau":
                d["tau"] = [tuple(float(v) for v in iv.split("/")) for iv in value.split("|")]
                if any(len(iv) != 2 for iv in d["tau"]):
                    raise MgpuError("a bank's intervals are MIN/MAX, separated by '|', not %r" % value)
            else:
                d["rho"] = [float(v) for v in value.split("|")]
        elif key == "tau":
            lo, hi = value.split("/")
            d["tau_min_us"], d["tau_max_us"] = float(lo), float(hi)
        elif key in ("fd", "snr"):
            d["doppler_hz" if key == "fd" else "snr_db"] = float(value)
        else:
            raise MgpuError("a Wiener rung's fields are tau, fd and snr, not %r" % key)
    for kind, d in [r for r in rungs if isinstance(r[1], dict) and r[0] == "bank"]:
        if not d.get("tau"):
            raise MgpuError("a bank rung needs tau=MIN/MAX|MIN/MAX|...")
        if "rho" in d and len(d["rho"]) != len(d["tau"]) - 1:
            raise MgpuError("a bank of %d designs takes %d rho values" % (len(d["tau"]), len(d["tau"]) - 1))
    return rungs


def _is_wiener(rung):
    return rung == "wiener" or (isinstance(rung, (tuple, list)) and len(rung) == 2 and rung[0] == "wiener")


# ---- a Wiener rung's bank of designs (include/mercury_wiener_bank.h) ---------------------------------------------
WIENER_BANK_SYMBOLS = names("mercury_wiener_bank.h")
WIENER_BANK_MAX = 4


class WienerBankEntry(C.Structure):  # mgpu_wiener_bank_entry
    _fields_ = [("design", WienerDesign), ("rho_min", C.c_double)]


def _is_bank(rung):
    return isinstance(rung, (tuple, list)) and len(rung) == 2 and rung[0] == "bank"


def bank_entries(spec):
    """a ("bank", {...}) rung's dict as parse_ladder gives it (tau: [(min, max), ...] in us, doppler_hz, snr_db for every design, rho:
    the thresholds of all but the last) -> [(design dict, rho_min or None), ...] as RxPhy.set_wiener_bank takes them"""
    common = {k: spec[k] for k in ("doppler_hz", "snr_db") if k in spec}
    rho = list(spec.get("rho", [])) + [None] * len(spec["tau"])
    return [(dict(common, tau_min_us=lo, tau_max_us=hi), rho[i]) for i, (lo, hi) in enumerate(spec["tau"])]


def _bank_array(entries):
    entries = list(entries or [])
    arr = (WienerBankEntry * max(len(entries), 1))()
    for i, e in enumerate(entries):
        design, rho = e if isinstance(e, (tuple, list)) else (e, None)
        arr[i] = WienerBankEntry(_wiener_design(design), float("nan") if rho is None else float(rho))
    return arr, len(entries)


def host_wiener_select(cfg, grid, entries, explicit=None):
    """mgpu_host_wiener_select: the design a bank's rung chooses for one frame grid (complex128 [Nsymb * Nc], after the AGC); no GPU.
    entries: [(design dict, rho_min or None: the default), ...], the last one the fallback.
    -> dict(design, corr: float64 [4] R1r R1i R2r R2i, n1, n2)"""
    lib = load_library()
    g = np.ascontiguousarray(grid, np.complex128).ravel()
    arr, n = _bank_array(entries)
    design, n1, n2, corr = C.c_int(), C.c_int(), C.c_int(), np.zeros(4, np.float64)
    _checked(lib.mgpu_host_wiener_select, int(cfg), _explicit_ref(explicit), arr, n, C.sizeof(WienerBankEntry), _ptr(g), C.byref(design),
             _ptr(corr), C.byref(n1), C.byref(n2))
    return dict(design=design.value, corr=corr, n1=n1.value, n2=n2.value)


def host_wiener_bank_thresholds(cfg, entries, explicit=None):
    """mgpu_host_wiener_bank_thresholds: (rho_min as applied: float64 [n - 1], the pilot spacing s) of a bank on the mode's geometry; no GPU"""
    lib = load_library()
    arr, n = _bank_array(entries)
    rho, s = np.zeros(max(n - 1, 1), np.float64), C.c_int()
    _checked(lib.mgpu_host_wiener_bank_thresholds, int(cfg), _explicit_ref(explicit), arr, n, C.sizeof(WienerBankEntry), _ptr(rho), C.byref(s))
    return rho[: max(n - 1, 0)], s.value


def wiener_sounding(corr, n1, n2, s):
    """(rho, delay_us) from the four sums of mgpu_get_wiener_choice / mgpu_host_wiener_select (corr [..., 4]): rho = (|R2| / n2) / (|R1| / n1),
    the centroid delay = -arg R1 * 256 / (2 pi s) / 0.012 us"""
    corr = np.asarray(corr, np.float64)
    r1, r2 = corr[..., 0] + 1j * corr[..., 1], corr[..., 2] + 1j * corr[..., 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = (np.abs(r2) / n2) / (np.abs(r1) / n1)
    return rho, -np.angle(r1) * 256.0 / (2.0 * np.pi * s) / 0.012


def host_wiener_estimate(cfg, grid, design=None, explicit=None):
    """mgpu_host_wiener_estimate: the separable Wiener estimate at the pilot cells (row-major pilot order, complex128 [nPilots]) of one frame
    grid (complex128 [Nsymb * Nc], after the AGC); no GPU. design: dict with any of tau_min_us, tau_max_us, doppler_hz, snr_db (None: the
    defaults). explicit: as RxPhy's."""
    lib = load_library()
    g = np.ascontiguousarray(grid, np.complex128).ravel()
    ref = _explicit_ref(explicit)
    d = _wiener_design(design)
    # nPilots of the (possibly explicit) geometry: the entries a call on an all-zero grid writes
    nP, = _written(lambda count: _checked(lib.mgpu_host_wiener_estimate, int(cfg), ref, C.byref(d), _ptr(np.zeros_like(g)), _ptr(count)),
                   (g.size, np.complex128))
    out = np.zeros(nP, np.complex128)
    _checked(lib.mgpu_host_wiener_estimate, int(cfg), ref, C.byref(d), _ptr(g), _ptr(out))
    return out


def host_wiener_tables(cfg, design=None, explicit=None):
    """mgpu_host_wiener_tables: (time classes, frequency classes) of a design, each a list of (members: int32 [n] - the pilot rows a carrier
    has / the pilot carriers a symbol has -, matrix [n, n]: float64 / complex128, as the kernel reads it); no GPU."""
    lib = load_library()
    ref = _explicit_ref(explicit)
    d = _wiener_design(design)
    out = []
    for which in (0, 1):
        count = C.c_int()
        _checked(lib.mgpu_host_wiener_tables, int(cfg), ref, C.byref(d), which, 0, C.byref(count), None, None, None)
        classes = []
        for cls in range(count.value):
            n = C.c_int()
            lib.mgpu_host_wiener_tables(int(cfg), ref, C.byref(d), which, cls, None, C.byref(n), None, None)
            members = np.zeros(n.value, np.int32)
            matrix = np.zeros((n.value, n.value), np.complex128 if which else np.float64)
            _checked(lib.mgpu_host_wiener_tables, int(cfg), ref, C.byref(d), which, cls, None, None, _ptr(members), _ptr(matrix))
            classes.append((members, matrix))
        out.append(classes)
    return tuple(out)


def host_ls_estimate(cfg, grid, width, height, explicit=None):
    """mgpu_host_ls_estimate: the LS estimate at the pilot cells (row-major pilot order, complex128 [nPilots]) of one frame grid
    (complex128 [Nsymb * Nc], after the AGC) for a width x height window; no GPU. explicit: as RxPhy's."""
    lib = load_library()
    g = np.ascontiguousarray(grid, np.complex128).ravel()
    ref = _explicit_ref(explicit)

    def probe(count):
        rc = lib.mgpu_host_ls_estimate(cfg, ref, int(width), int(height), _ptr(np.zeros_like(g)), _ptr(count))
        if rc != 0:
            raise MgpuError("mgpu_host_ls_estimate failed (%d)" % rc)
    # nPilots of the (possibly explicit) geometry: the entries a call on an all-zero grid writes
    out = np.zeros(_written(probe, (g.size, np.complex128))[0], np.complex128)
    if lib.mgpu_host_ls_estimate(cfg, ref, int(width), int(height), _ptr(g), _ptr(out)) != 0:
        raise MgpuError("mgpu_host_ls_estimate failed")
    return out


# ---- the channel-aware demapper (include/mercury_demapper.h) --------------------------------------------------------
DEMAPPER_SYMBOLS = names("mercury_demapper.h")
DEMAPPERS = {"maxlog": 0, "csi": 1, "nmap": 2}
NMAP_DEFAULT = {"dead_band": 2.0, "smooth": 1}


class DemapperParams(C.Structure):
    """mgpu_demapper_params (include/mercury_demapper.h)"""
    _fields_ = [("dead_band", C.c_double), ("smooth", C.c_int)]


def parse_demapper(text):
    """"maxlog", "csi", "nmap" or "nmap:band=2,smooth=1" (the tools' --demapper) -> (name, {dead_band, smooth} or None)"""
    return _parse_spec(text, "demapper", DEMAPPERS, "nmap", NMAP_DEFAULT, {"band": ("dead_band", float), "smooth": ("smooth", int)},
                       "one of %s, nmap with :band=B,smooth=W" % ", ".join(DEMAPPERS), "band=B and smooth=W are")


def host_demap_csi(cfg, grid, H, explicit=None):
    """mgpu_host_demap_csi, no GPU: one frame's cell grid (after the AGC) and channel estimate at every cell (complex128 [Nsymb * Nc] each)
    -> (the demodulated LLRs in the demapper's order: float32 [nBits], sigma2). explicit: as RxPhy's."""
    lib = load_library()
    g = np.ascontiguousarray(grid, np.complex128).ravel()
    h = np.ascontiguousarray(H, np.complex128).ravel()
    if g.size != h.size:
        raise MgpuError("host_demap_csi: grid and H must have one entry per cell")
    ref = _explicit_ref(explicit)
    # nBits of the (possibly explicit) geometry: the entries a call on an all-zero grid with H = 1 writes
    nbits, = _written(lambda count: _checked(lib.mgpu_host_demap_csi, int(cfg), ref, _ptr(np.zeros_like(g)), _ptr(np.ones_like(g)), _ptr(count), None),
                      (g.size * 5, np.float32))
    llr = np.zeros(nbits, np.float32)
    sigma2 = C.c_double()
    _checked(lib.mgpu_host_demap_csi, int(cfg), ref, _ptr(g), _ptr(h), _ptr(llr), C.byref(sigma2))
    return llr, float(sigma2.value)


def host_demap_nmap(cfg, grid, H, dead_band=2.0, smooth=1, explicit=None):
    """mgpu_host_demap_nmap, no GPU: as host_demap_csi with the noise map -> (llr_demod float32 [nBits], sigma2,
    fc float64 [Nc], fs float64 [Nsymb]); the factors are those after the dead band."""
    lib = load_library()
    g = np.ascontiguousarray(grid, np.complex128).ravel()
    h = np.ascontiguousarray(H, np.complex128).ravel()
    if g.size != h.size:
        raise MgpuError("host_demap_nmap: grid and H must have one entry per cell")
    ref = _explicit_ref(explicit)
    prm = DemapperParams(float(dead_band), int(smooth))
    # nBits and Nsymb of the (possibly explicit) geometry: the entries a call on an all-zero grid with H = 1 writes
    nbits, nsymb = _written(lambda count, rows: _checked(lib.mgpu_host_demap_nmap, int(cfg), ref, _ptr(np.zeros_like(g)), _ptr(np.ones_like(g)),
                                                         C.byref(prm), C.sizeof(prm), _ptr(count), None, None, _ptr(rows)),
                            (g.size * 5, np.float32), (g.size, np.float64))
    llr, fs = np.zeros(nbits, np.float32), np.zeros(nsymb, np.float64)
    fc = np.zeros(g.size // fs.size, np.float64)
    sigma2 = C.c_double()
    _checked(lib.mgpu_host_demap_nmap, int(cfg), ref, _ptr(g), _ptr(h), C.byref(prm), C.sizeof(prm), _ptr(llr), C.byref(sigma2), _ptr(fc), _ptr(fs))
    return llr, float(sigma2.value), fc, fs


# ---- pilot-aided residual carrier-offset correction (include/mercury_cfo.h) ----------------------------------------
CFO_SYMBOLS = names("mercury_cfo.h")
CFO_MODES = {"off": 0, "pilots": 1}
_CFO_CELLS = {}


def host_cfo_pilots(cfg, grid, explicit=None):
    """mgpu_host_cfo_pilots, no GPU: one frame's cell grid (complex128 [Nsymb * Nc], after the AGC) -> (the grid with symbol s turned back
    by s steps: complex128 [Nsymb * Nc], the step in radians per symbol). explicit: as RxPhy's."""
    lib = load_library()
    g = np.ascontiguousarray(grid, np.complex128).ravel()
    ref = _explicit_ref(explicit)
    # the cells of the (possibly explicit) geometry: the entries a call on an all-zero grid writes (at most 255 symbols of 50 carriers);
    # asked once per geometry
    key = (int(cfg), tuple(sorted((explicit or {}).items())))
    if key not in _CFO_CELLS:
        _CFO_CELLS[key], = _written(lambda count: _checked(lib.mgpu_host_cfo_pilots, int(cfg), ref, _ptr(np.zeros_like(count)), _ptr(count), None),
                                    (255 * 50, np.complex128))
    cells = _CFO_CELLS[key]
    if g.size != cells:
        raise MgpuError("host_cfo_pilots: the grid must have one entry per cell (%d)" % cells)
    out = np.zeros_like(g)
    step = C.c_double()
    _checked(lib.mgpu_host_cfo_pilots, int(cfg), ref, _ptr(g), _ptr(out), C.byref(step))
    return out, float(step.value)


# ---- the impulse blanker (include/mercury_blanker.h) -----------------------------------------------------------------
BLANKER_SYMBOLS = names("mercury_blanker.h")
BLANKER_MODES = {"off": 0, "median": 1}
BLANKER_DEFAULT = {"threshold": 24.0, "guard": 4, "max_share": 0.125}
BLANKER_REPORT_DTYPE = np.dtype([("marked", "<i4"), ("blanked", "<i4")])


class BlankerParams(C.Structure):
    """mgpu_blanker_params (include/mercury_blanker.h)"""
    _fields_ = [("threshold", C.c_double), ("guard", C.c_int), ("max_share", C.c_double)]


def _blanker_params(threshold=None, guard=None, max_share=None):
    return _params(BlankerParams, BLANKER_DEFAULT, (threshold, guard, max_share))


def parse_blanker(text):
    """"off", "median" or "median:thr=24,guard=4,share=0.125" (the tools' --blanker) -> (name, {threshold, guard, max_share} or None)"""
    return _parse_spec(text, "blanker", BLANKER_MODES, "median", BLANKER_DEFAULT,
                       {"thr": ("threshold", float), "guard": ("guard", int), "share": ("max_share", float)},
                       "off, or median with :thr=T,guard=G,share=S", "thr=T, guard=G and share=S are")


def host_blank(cfg, frame, explicit=None, **params):
    """mgpu_host_blank, no GPU: one frame's baseband samples (complex128 [frame_samples]) -> (the blanked frame, {"marked", "blanked"}).
    params: threshold, guard, max_share (the defaults where left out). explicit: as RxPhy's."""
    lib = load_library()
    x = np.ascontiguousarray(frame, np.complex128).ravel()
    # frame_samples of the (possibly explicit) geometry: an explicit Nsymb symbols of the mode's length, else the mode's own
    info = Info()
    if lib.mgpu_host_mode_info(int(cfg), 0, C.byref(info)) != 0:
        raise MgpuError("host_blank: cfg %r is no mode" % (cfg,), 1)
    n = int((explicit or {}).get("Nsymb", 0)) * info.Nofdm or info.frame_samples
    if x.size != n:
        raise MgpuError("host_blank: the frame must have frame_samples (%d) samples" % n, 1)
    prm = _blanker_params(**params)
    out, rep = np.zeros_like(x), np.zeros(1, BLANKER_REPORT_DTYPE)
    _checked(lib.mgpu_host_blank, int(cfg), _explicit_ref(explicit), C.byref(prm), _ptr(x), _ptr(out), _ptr(rep))
    return out, {"marked": int(rep["marked"][0]), "blanked": int(rep["blanked"][0])}


# ---- the carrier excisor (include/ext/mercury_excisor.h) --------------------------------------------------------------
EXCISOR_SYMBOLS = names("ext/mercury_excisor.h")
EXCISOR_MODES = {"off": 0, "welch": 1}
EXCISOR_DEFAULT = {"threshold": 12.0, "guard": 1, "max_bins": 16}
EXCISOR_REPORT_DTYPE = np.dtype([("exceeding", "<u8"), ("mask", "<u8"), ("band_lo", "<i4"), ("excised", "<i4"), ("nonfinite", "<i4"),
                                 ("level", "<f8")], align=True)


class ExcisorParams(C.Structure):
    """mgpu_excisor_params (include/ext/mercury_excisor.h)"""
    _fields_ = [("threshold", C.c_double), ("guard", C.c_int), ("max_bins", C.c_int)]


def _excisor_params(threshold=None, guard=None, max_bins=None):
    return _params(ExcisorParams, EXCISOR_DEFAULT, (threshold, guard, max_bins))


def parse_excisor(text):
    """"off", "welch" or "welch:thr=12,guard=1,bins=16" (the tools' --excisor) -> (name, {threshold, guard, max_bins} or None)"""
    return _parse_spec(text, "excisor", EXCISOR_MODES, "welch", EXCISOR_DEFAULT,
                       {"thr": ("threshold", float), "guard": ("guard", int), "bins": ("max_bins", int)},
                       "off, or welch with :thr=T,guard=G,bins=B", "thr=T, guard=G and bins=B are")


def host_excise(window, carrier_hz, **params):
    """mgpu_host_excise, no GPU: one window of real samples at 48 kHz (float64 [n], n >= 1) -> (the cleaned window, its report as a dict of
    EXCISOR_REPORT_DTYPE's fields). params: threshold, guard, max_bins (the defaults where left out)."""
    lib = load_library()
    x = np.ascontiguousarray(window, np.float64).ravel()
    prm = _excisor_params(**params)
    out, rep = np.zeros_like(x), np.zeros(1, EXCISOR_REPORT_DTYPE)
    _checked(lib.mgpu_host_excise, C.byref(prm), float(carrier_hz), _ptr(x), int(x.size), _ptr(out), _ptr(rep))
    return out, {name: rep[name][0].item() for name in EXCISOR_REPORT_DTYPE.names}


# ---- diversity combining (include/mercury_diversity.h) ------------------------------------------------------------
DIVERSITY_SYMBOLS = names("mercury_diversity.h")
DIVERSITY_MAX = 8


def _csr(groups):
    """[[member, ...], ...] -> (first int32 [G + 1], member int32 [sum]); an empty group stays empty (the library refuses it)"""
    first = np.zeros(len(groups) + 1, np.int32)
    first[1:] = np.cumsum([len(g) for g in groups])
    member = np.array([m for g in groups for m in g] + [0], np.int32)       # one spare entry: never a zero-length buffer
    return first, member


def _group_args(F, D, groups):
    """the (D, first, member, G, rows out) of a combine call: uniform groups of D, or `groups` as a list of member lists"""
    if (D is None) == (groups is None):
        raise MgpuError("give either D (uniform groups) or groups (lists of member rows)")
    if groups is None:
        D = int(D)
        return D, None, None, 0, (F // D if D > 0 else 0)
    first, member = _csr(groups)
    return 0, first, member, len(groups), len(groups)


def host_llr_combine(llr, D=None, groups=None):
    """mgpu_host_llr_combine, no GPU: float32 [F, 1600] -> the groups' LLR rows added in member order, float32 [G, 1600]. D: uniform groups
    of D consecutive rows; groups: [[row, ...], ...], 1..DIVERSITY_MAX rows each."""
    lib = load_library()
    l = np.ascontiguousarray(llr, np.float32).reshape(-1, 1600)
    D, first, member, G, rows = _group_args(l.shape[0], D, groups)
    out = np.zeros((rows, 1600), np.float32)
    _checked(lib.mgpu_host_llr_combine, _ptr(l), l.shape[0], D, _ptr(first), _ptr(member), G, _ptr(out), what="refused the groups")
    return out


# ---- Watterson HF fading channel (include/mercury_channel.h) ----------------------------------------------------
HF_MAX_PATHS, HF_SINUSOIDS = 4, 32
HF_PRESETS = {"awgn": 0, "good": 1, "moderate": 2, "poor": 3, "flutter": 4}
HF_CHANNEL_SYMBOLS = names("mercury_channel.h")
# the streaming form in the same header (HfStream below)
HF_STREAM_SYMBOLS = [n for n in HF_CHANNEL_SYMBOLS if "_hf_stream_" in n]


class HfChannel(C.Structure):
    """mgpu_hf_channel: up to four paths (delay, relative gain, Gaussian Doppler spread = 2 sigma, Doppler shift) and a frequency offset."""
    _fields_ = [("struct_size", C.c_int), ("n_paths", C.c_int), ("delay_ms", C.c_double * HF_MAX_PATHS), ("gain_db", C.c_double * HF_MAX_PATHS),
                ("spread_hz", C.c_double * HF_MAX_PATHS), ("shift_hz", C.c_double * HF_MAX_PATHS), ("freq_offset_hz", C.c_double)]

    def __init__(self, paths=((0.0, 0.0, 0.0, 0.0),), freq_offset_hz=0.0):
        """paths: (delay_ms, gain_db, spread_hz, shift_hz) per path."""
        super().__init__()
        self.struct_size = C.sizeof(HfChannel)
        self.n_paths = len(paths)
        for k, (d, g, sp, sh) in enumerate(paths[:HF_MAX_PATHS]):
            self.delay_ms[k], self.gain_db[k], self.spread_hz[k], self.shift_hz[k] = d, g, sp, sh
        self.freq_offset_hz = freq_offset_hz

    def paths(self):
        return [(self.delay_ms[k], self.gain_db[k], self.spread_hz[k], self.shift_hz[k]) for k in range(self.n_paths)]


def hf_channel_preset(name):
    """MGPU_HF_AWGN / GOOD / MODERATE / POOR / FLUTTER by name ('awgn', 'good', 'moderate', 'poor', 'flutter') or number."""
    which = HF_PRESETS.get(name, -1) if isinstance(name, str) else int(name)
    ch = HfChannel()
    if load_library().mgpu_hf_channel_preset(which, C.byref(ch)) != 0:
        raise MgpuError("unknown HF channel preset %r" % (name,))
    return ch


def _hf(ch):
    return hf_channel_preset(ch) if isinstance(ch, (str, int)) else ch


def host_hilbert_taps():
    """The real-input model's Hilbert FIR (odd length, antisymmetric, centred), as the library designs it."""
    taps, n = np.zeros(512, np.float64), C.c_int()
    if load_library().mgpu_host_hilbert_taps(_ptr(taps), C.byref(n)) != 0:
        raise MgpuError("mgpu_host_hilbert_taps failed")
    return taps[: n.value].copy()


def host_hf_channel_draws(ch, seed, realisation, path):
    """(freq_hz[32], phase[32]) of one path of one realisation (a static path: one entry, NaN elsewhere)."""
    f, ph = np.zeros(HF_SINUSOIDS), np.zeros(HF_SINUSOIDS)
    if load_library().mgpu_host_hf_channel_draws(C.byref(_hf(ch)), seed, realisation, path, _ptr(f), _ptr(ph)) != 0:
        raise MgpuError("mgpu_host_hf_channel_draws: bad channel or path")
    return f, ph


def host_hf_channel_taps(ch, fs, seed, realisation, n, t0=0):
    """g_k(t_i), i < n, t_i = (t0 + i) / fs: complex128 [n_paths, n], normalised, without the frequency offset (host-only reference)."""
    ch = _hf(ch)
    g = np.zeros((max(ch.n_paths, 1), n), np.complex128)
    if load_library().mgpu_host_hf_channel_taps(C.byref(ch), fs, seed, realisation, t0, n, _ptr(g)) != 0:
        raise MgpuError("mgpu_host_hf_channel_taps: bad channel or argument")
    return g


def cfg_explicit(M, rate16, preamble_nsymb, estimator):
    """MGPU_CFG_EXPLICIT (include/mercury_gpu.h): cfg id of an explicit (constellation, LDPC rate, preamble, estimator) combination."""
    mods, rates = {2: 0, 4: 1, 8: 2, 16: 3, 32: 4}, {1: 0, 2: 1, 3: 2, 4: 3, 5: 4, 6: 5, 8: 6, 14: 7}
    if M not in mods or rate16 not in rates or not 1 <= preamble_nsymb <= 8 or estimator not in (0, 1):
        return -1
    return 1000 + (((mods[M] * 8 + rates[rate16]) * 8 + (preamble_nsymb - 1)) * 2 + estimator)


class MgpuError(RuntimeError):
    def __init__(self, message, code=None):
        super().__init__(message)
        self.code = code         # the library's status (MGPU_ERR_*) where one was returned


class DeviceProps(C.Structure):    # mgpu_device_props
    _fields_ = [("compute_units", C.c_int), ("clock_khz", C.c_int), ("memory_clock_khz", C.c_int), ("lds_bytes_per_cu", C.c_int),
                ("wavefront_size", C.c_int), ("numa_node", C.c_int), ("hbm_bytes", C.c_ulonglong),
                ("name", C.c_char * 64), ("gcn_arch", C.c_char * 32), ("pci_bus_id", C.c_char * 32)]


def device_props(device=0):
    """mgpu_device_props_get: compute units, clocks, LDS per compute unit, PCI address and NUMA node of a device, as a dict."""
    lib = load_library()
    p = DeviceProps()
    rc = lib.mgpu_device_props_get(device, C.byref(p))
    if rc != 0:
        raise MgpuError("mgpu_device_props_get(%d) failed (%d): no such device" % (device, rc))
    return {n: (getattr(p, n).decode() if isinstance(getattr(p, n), bytes) else getattr(p, n)) for n, _ in DeviceProps._fields_}


def pinned_empty(shape, dtype, device=None):
    """numpy array over page-locked host memory from mgpu_alloc_host — or, with ``device``, from mgpu_alloc_host_near (pages on that
    GPU's NUMA node). Keep the array alive while it is in use; the memory is released when the returned array's base object is collected."""
    lib = load_library()
    dt = np.dtype(dtype)
    n = int(np.prod(shape))
    ptr = lib.mgpu_alloc_host(n * dt.itemsize) if device is None else lib.mgpu_alloc_host_near(int(device), n * dt.itemsize)
    if not ptr:
        raise MgpuError("mgpu_alloc_host failed")

    class _Owner:
        def __del__(self):
            lib.mgpu_free_host(ptr)

    buf = (C.c_char * (n * dt.itemsize)).from_address(ptr)
    buf._owner = _Owner()
    return np.frombuffer(buf, dtype=dt).reshape(shape)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class RxPhy(_Handle):
    """One GPU receive context for one Mercury mode (``load_configuration(cfg)`` equivalent)."""
    _destroy = "mgpu_destroy"

    def __init__(self, cfg, max_iters=50, decoder=DEC_SPA, agc=1, variance_source=1, device=0,
                 max_batch=4096, minsum_alpha=0.0, mfsk_ctrl_mode=False, test_puncture_nbits=0, explicit=None):
        """explicit: dict with any of pilot_boost, ls_window, pilot_seed, scrambler_seed, preamble_seed, Dy, Nsymb (and Nc, Nfft, Dx, which
        must be the reference's) -> mgpu_create_explicit (include/mercury_gpu.h); the seeds override the reference's 0 / 0 / 1 together."""
        self.lib = load_library()
        self.h = C.c_void_p()
        c = Config(cfg, max_iters, decoder, agc, variance_source, device, max_batch, minsum_alpha, 1 if mfsk_ctrl_mode else 0, test_puncture_nbits)
        if explicit:
            rc = self.lib.mgpu_create_explicit(C.byref(c), _explicit_ref(explicit), C.byref(self.h))
        else:
            rc = self.lib.mgpu_create(C.byref(c), C.byref(self.h))
        if rc != 0:
            raise MgpuError("mgpu_create failed (%d): %s" % (rc, self.lib.mgpu_last_error(None).decode()))
        self.config = c
        self._mode = (int(cfg), dict(explicit) if explicit else None)      # for the host twins that need the geometry
        self.max_iters = max_iters
        self.max_batch = max_batch
        i = Info()
        self._ck(self.lib.mgpu_get_info(self.h, C.byref(i)))
        self.info = i
        for n in INFO_FIELDS:
            setattr(self, n, getattr(i, n))

    def _ck(self, rc):
        if rc != 0:
            raise MgpuError("mgpu error %d: %s" % (rc, self.lib.mgpu_last_error(self.h).decode()), rc)

    # ---- estimator ladder (include/mercury_estimator.h) ----------------------------------------
    def set_estimator_ladder(self, rungs):
        """rungs: [(width, height), ...] in cells (carriers x symbols), at most LADDER_MAX; [] or None: no ladder. Frames whose CRC fails are
        re-estimated and decoded again with the next rung, on the device, in every receive entry point of this context. A rung may also be
        "wiener" or ("wiener", {design fields}) as parse_ladder gives it: the separable Wiener estimator (MGPU_RUNG_WIENER), or
        ("bank", {...}): a Wiener rung carrying the bank's last design, plus set_wiener_bank with all of them."""
        rungs = list(rungs or [])
        banks = {i: bank_entries(r[1]) for i, r in enumerate(rungs) if _is_bank(r)}
        if banks:       # a bank rung is a Wiener rung carrying the bank's last design, plus the bank
            self.set_estimator_ladder([("wiener", dict(banks[i][-1][0])) if i in banks else r for i, r in enumerate(rungs)])
            for i, entries in banks.items():
                self.set_wiener_bank(i, entries)
            return
        if any(_is_wiener(r) for r in rungs):
            arr = (EstimatorRung * len(rungs))()
            for i, r in enumerate(rungs):
                if _is_wiener(r):
                    arr[i] = EstimatorRung(RUNG_WIENER, LsWindow(0, 0), _wiener_design(None if r == "wiener" else r[1]))
                else:
                    arr[i] = EstimatorRung(RUNG_LS, LsWindow(int(r[0]), int(r[1])), WienerDesign())
            self._ck(self.lib.mgpu_set_estimator_ladder_ex(self.h, arr, len(rungs), C.sizeof(EstimatorRung)))
            return
        arr = (LsWindow * max(len(rungs), 1))(*[LsWindow(int(w), int(h)) for w, h in rungs])
        self._ck(self.lib.mgpu_set_estimator_ladder(self.h, arr if rungs else None, len(rungs)))

    @property
    def estimator_ladder(self):
        """the rungs as they are applied (odd sides): [(width, height), ...]"""
        arr, n = (LsWindow * LADDER_MAX)(), C.c_int()
        self._ck(self.lib.mgpu_get_estimator_ladder(self.h, arr, C.byref(n)))
        return [(arr[r].width, arr[r].height) for r in range(n.value)]

    @property
    def estimator_ladder_ex(self):
        """the rungs with their kind: (width, height) for an LS rung, ("wiener", {design}) for a Wiener rung"""
        arr, n = (EstimatorRung * LADDER_MAX)(), C.c_int()
        self._ck(self.lib.mgpu_get_estimator_ladder_ex(self.h, arr, C.byref(n), C.sizeof(EstimatorRung)))
        return [("wiener", {k: getattr(arr[r].design, k) for k in WIENER_DESIGN_DEFAULT}) if arr[r].kind == RUNG_WIENER
                else (arr[r].window.width, arr[r].window.height) for r in range(n.value)]

    # ---- a Wiener rung's bank of designs (include/mercury_wiener_bank.h) --------------------------
    def set_wiener_bank(self, rung, entries):
        """Rung `rung` of the ladder in force (a Wiener rung) chooses per frame among entries = [(design dict, rho_min or None: the
        default), ...] (a bare design dict is (design, None)); the last entry is the fallback. [] or None removes the bank."""
        arr, n = _bank_array(entries)
        self._ck(self.lib.mgpu_set_wiener_bank(self.h, int(rung), arr if n else None, n, C.sizeof(WienerBankEntry)))

    def wiener_bank(self, rung):
        """the bank of a rung with the thresholds as applied: [(design dict, rho_min), ...] (None for a NaN: the fallback's is reported as
        it was given); [] where it has none"""
        arr, n = (WienerBankEntry * WIENER_BANK_MAX)(), C.c_int()
        self._ck(self.lib.mgpu_get_wiener_bank(self.h, int(rung), arr, C.byref(n), C.sizeof(WienerBankEntry)))
        return [({k: getattr(arr[d].design, k) for k in WIENER_DESIGN_DEFAULT}, None if np.isnan(arr[d].rho_min) else arr[d].rho_min) for d in range(n.value)]

    def wiener_choice(self, first=0, count=None):
        """rung 0's choice for rows first .. first + count - 1 (default: to max_batch) of the last receive call:
        dict(design int32 [count], corr float64 [count, 4], n1, n2, rho, delay_us) - rho and delay_us computed here from corr"""
        count = self.max_batch - int(first) if count is None else int(count)
        design, corr, n1, n2 = np.zeros(count, np.int32), np.zeros((count, 4), np.float64), C.c_int(), C.c_int()
        self._ck(self.lib.mgpu_get_wiener_choice(self.h, int(first), count, _ptr(design), _ptr(corr), C.byref(n1), C.byref(n2)))
        _, s = host_wiener_bank_thresholds(self._mode[0], self.wiener_bank(0), explicit=self._mode[1])
        rho, delay = wiener_sounding(corr, n1.value, n2.value, s)
        return dict(design=design, corr=corr, n1=n1.value, n2=n2.value, rho=rho, delay_us=delay)

    def last_rungs(self, F):
        """winning rung of each of the first F frames of the last receive call, -1 where no rung decoded: int32 [F]"""
        out = np.zeros(F, np.int32)
        self._ck(self.lib.mgpu_estimator_rungs_last(self.h, _ptr(out), F))
        return out

    def ladder_counters(self, reset=False):
        """(frames decoded by each rung: int64 [LADDER_MAX], frames seen) since the ladder was set or the last reset"""
        by, n = np.zeros(LADDER_MAX, np.int64), C.c_longlong()
        self._ck(self.lib.mgpu_estimator_ladder_counters(self.h, _ptr(by), C.byref(n), 1 if reset else 0))
        return by, int(n.value)

    # ---- the channel-aware demapper (include/mercury_demapper.h) -------------------------------
    def set_demapper(self, name, dead_band=None, smooth=None):
        """"maxlog": the reference's demapper (one variance per frame; the default). "csi": max-log LLRs weighted by |H|^2 per cell, in
        every receive entry point of this context. "nmap": those divided by a noise factor per carrier and per symbol measured at the
        pilots (dead_band, default 2.0: factors within [1 / dead_band, dead_band] are 1; smooth, default 1: carriers on either side that
        share a carrier's mean). name may also be the tools' form, "nmap:band=2,smooth=1" (parse_demapper)."""
        try:
            name, spec = parse_demapper(name)
        except ValueError:
            raise MgpuError("demapper must be one of %s" % sorted(DEMAPPERS))
        if spec and spec != NMAP_DEFAULT:
            dead_band = spec["dead_band"] if dead_band is None else dead_band
            smooth = spec["smooth"] if smooth is None else smooth
        if dead_band is None and smooth is None:
            self._ck(self.lib.mgpu_set_demapper(self.h, DEMAPPERS[name]))
            return
        prm = DemapperParams(float(NMAP_DEFAULT["dead_band"] if dead_band is None else dead_band), int(NMAP_DEFAULT["smooth"] if smooth is None else smooth))
        self._ck(self.lib.mgpu_set_demapper_ex(self.h, DEMAPPERS[name], C.byref(prm), C.sizeof(prm)))

    @property
    def demapper_ex(self):
        """(name, {dead_band, smooth}): the demapper and the noise map's parameters as last set (the defaults before)"""
        v, prm = C.c_int(), DemapperParams()
        self._ck(self.lib.mgpu_get_demapper_ex(self.h, C.byref(v), C.byref(prm), C.sizeof(prm)))
        return {n: k for k, n in DEMAPPERS.items()}[v.value], {"dead_band": prm.dead_band, "smooth": prm.smooth}

    def noise_map(self, first=0, count=None):
        """(fc float64 [count, Nc], fs float64 [count, Nsymb]): the noise factors, after the dead band, of rows first .. first + count - 1
        (default: to max_batch) of the last call that ran with the "nmap" demapper; rung 0's under an estimator ladder."""
        count = self.max_batch - int(first) if count is None else int(count)
        fc, fs = np.zeros((count, self.Nc), np.float64), np.zeros((count, self.Nsymb), np.float64)
        self._ck(self.lib.mgpu_get_noise_map(self.h, int(first), count, _ptr(fc), _ptr(fs)))
        return fc, fs

    @property
    def demapper(self):
        v = C.c_int()
        self._ck(self.lib.mgpu_get_demapper(self.h, C.byref(v)))
        return {n: k for k, n in DEMAPPERS.items()}[v.value]

    # ---- pilot-aided residual carrier-offset correction (include/mercury_cfo.h) -----------------
    def set_cfo(self, name):
        """"off": the reference's front-end (the default). "pilots": every frame's grid is turned back by the per-symbol phase step its
        own pilots measure, between the AGC and the channel estimate, in every receive entry point of this context."""
        if name not in CFO_MODES:
            raise MgpuError("cfo must be one of %s" % sorted(CFO_MODES))
        self._ck(self.lib.mgpu_set_cfo(self.h, CFO_MODES[name]))

    @property
    def cfo(self):
        v = C.c_int()
        self._ck(self.lib.mgpu_get_cfo(self.h, C.byref(v)))
        return {n: k for k, n in CFO_MODES.items()}[v.value]

    def cfo_steps(self, F):
        """the steps (radians per symbol; Hz = step * 12000 / (2 pi Nofdm)) of rows 0 .. F-1 of the last span that ran with the mode on"""
        out = np.zeros(int(F), np.float64)
        self._ck(self.lib.mgpu_get_cfo_steps(self.h, int(F), _ptr(out)))
        return out

    # ---- the impulse blanker (include/mercury_blanker.h) -------------------------------------------
    def set_blanker(self, name, threshold=None, guard=None, max_share=None):
        """"off": the samples go to the front-end as they are (the default). "median": every frame passes through the median-gated blanker
        first, in every receive entry point of this context (threshold, default 24 block medians; guard, default 4 samples; max_share,
        default 0.125 of the frame). name may also be the tools' form, "median:thr=24,guard=4,share=0.125" (parse_blanker)."""
        try:
            name, spec = parse_blanker(name)
        except ValueError:
            raise MgpuError("blanker must be one of %s" % sorted(BLANKER_MODES))
        spec = spec or BLANKER_DEFAULT
        prm = _blanker_params(spec["threshold"] if threshold is None else threshold, spec["guard"] if guard is None else guard,
                              spec["max_share"] if max_share is None else max_share)
        self._ck(self.lib.mgpu_set_blanker(self.h, BLANKER_MODES[name], C.byref(prm), C.sizeof(prm)))

    @property
    def blanker(self):
        """(name, {threshold, guard, max_share}): the mode and the parameters as last set (the defaults before)"""
        v, prm = C.c_int(), BlankerParams()
        self._ck(self.lib.mgpu_get_blanker(self.h, C.byref(v), C.byref(prm), C.sizeof(prm)))
        return {n: k for k, n in BLANKER_MODES.items()}[v.value], {"threshold": prm.threshold, "guard": prm.guard, "max_share": prm.max_share}

    def blanker_report(self, first=0, count=None):
        """{marked, blanked} (BLANKER_REPORT_DTYPE [count]) of rows first .. first + count - 1 (default: to max_batch) of the last call that
        ran with the blanker on"""
        count = self.max_batch - int(first) if count is None else int(count)
        out = np.zeros(count, BLANKER_REPORT_DTYPE)
        self._ck(self.lib.mgpu_get_blanker_report(self.h, int(first), count, _ptr(out)))
        return out

    def blank(self, baseband, frame_stride=None):
        """mgpu_blank_dev, the stage on its own: baseband complex128 [F, frame_samples] (or [F, frame_stride] with a frame_stride larger than
        the frame, of which each row's first frame_samples are the frame) -> (blanked complex128 [F, frame_samples], report [F]); with the
        parameters last set, whether or not the mode is on."""
        width = self.frame_samples if frame_stride is None else int(frame_stride)
        bb = np.ascontiguousarray(baseband, np.complex128).reshape(-1, width)
        F = bb.shape[0]
        out, rep = np.zeros((F, self.frame_samples), np.complex128), np.zeros(F, BLANKER_REPORT_DTYPE)
        if F:       # (the copies take the context's stream for None; mgpu_blank_dev takes the null stream)
            self._staged([bb], [out, rep], "mgpu_device_malloc failed", lambda d_bb, d_out, d_rep: self._ck(self.lib.mgpu_blank_dev(
                self.h, d_bb, F, 0 if frame_stride is None else width, d_out, d_rep, self.lib.mgpu_context_stream(self.h))))
        return out, rep

    # ---- the carrier excisor (include/ext/mercury_excisor.h) ----------------------------------------
    def set_excisor(self, name, threshold=None, guard=None, max_bins=None):
        """"off": receive_byte reads the capture windows as they are (the default). "welch": every capture window that enters receive_byte
        on this context is cleaned of narrowband carriers first (threshold, default 12 band medians; guard, default 1 bin; max_bins, default
        16). name may also be the tools' form, "welch:thr=12,guard=1,bins=16" (parse_excisor)."""
        try:
            name, spec = parse_excisor(name)
        except ValueError:
            raise MgpuError("excisor must be one of %s" % sorted(EXCISOR_MODES))
        spec = spec or EXCISOR_DEFAULT
        prm = _excisor_params(spec["threshold"] if threshold is None else threshold, spec["guard"] if guard is None else guard,
                              spec["max_bins"] if max_bins is None else max_bins)
        self._ck(self.lib.mgpu_set_excisor(self.h, EXCISOR_MODES[name], C.byref(prm), C.sizeof(prm)))

    def excisor(self):
        """(name, {threshold, guard, max_bins}): the mode and the parameters as last set (the defaults before)"""
        v, prm = C.c_int(), ExcisorParams()
        self._ck(self.lib.mgpu_get_excisor(self.h, C.byref(v), C.byref(prm), C.sizeof(prm)))
        return {n: k for k, n in EXCISOR_MODES.items()}[v.value], {"threshold": prm.threshold, "guard": prm.guard, "max_bins": prm.max_bins}

    def excisor_report(self, first=0, count=None):
        """EXCISOR_REPORT_DTYPE [count]: the reports of rows first .. first + count - 1 (default: to max_batch) of the last receive_byte call
        that ran with the excisor on, by the window's row"""
        count = self.max_batch - int(first) if count is None else int(count)
        out = np.zeros(count, EXCISOR_REPORT_DTYPE)
        self._ck(self.lib.mgpu_get_excisor_report(self.h, int(first), count, _ptr(out)))
        return out

    def excise(self, windows, carrier_hz):
        """mgpu_excise_dev, the stage on its own: windows float64 [W, n] (any n >= 1) -> (cleaned float64 [W, n], report [W]); with the
        parameters last set, whether or not the mode is on."""
        x = np.ascontiguousarray(windows, np.float64)
        x = x.reshape(1, -1) if x.ndim == 1 else x
        W, n = x.shape
        out, rep = np.zeros((W, n), np.float64), np.zeros(W, EXCISOR_REPORT_DTYPE)
        if W:
            self._staged([x], [out, rep], "mgpu_device_malloc failed", lambda d_x, d_out, d_rep: self._ck(self.lib.mgpu_excise_dev(
                self.h, d_x, W, n, float(carrier_hz), d_out, d_rep, self.lib.mgpu_context_stream(self.h))))
        return out, rep

    def _staged(self, inputs, outputs, error, run):
        """run(device pointers of inputs + outputs) between the inputs' copy to the device and the outputs' copy back, all on the
        context's stream; the device buffers are freed whatever happens"""
        lib = self.lib
        bufs = [lib.mgpu_device_malloc(self.h, max(a.nbytes, 16)) for a in inputs + outputs]
        try:
            if not all(bufs):
                raise MgpuError(error)
            for a, d in zip(inputs, bufs):
                self._ck(lib.mgpu_copy_to_device(self.h, d, _ptr(a), a.nbytes, None))
            run(*bufs)
            for a, d in zip(outputs, bufs[len(inputs):]):
                self._ck(lib.mgpu_copy_to_host(self.h, _ptr(a), d, a.nbytes, None))
        finally:
            for d in bufs:
                lib.mgpu_device_free(self.h, d)

    # ---- host-buffer entry points -------------------------------------------------------------
    def receive(self, baseband, taps=False, want_llr=False):
        """baseband: complex128 [F, Nsymb*Nofdm]. Returns dict(payload, stats[, taps...])."""
        bb = np.ascontiguousarray(baseband, np.complex128).reshape(-1, self.frame_samples)
        F = bb.shape[0]
        payload = np.zeros((F, self.payload_stride), np.uint8)
        stats = np.zeros(F, STATS_DTYPE)
        out = {"payload": payload, "stats": stats}
        if taps:
            G = self.Nsymb * self.Nc
            t = dict(grid=np.zeros((F, G), np.complex128), H=np.zeros((F, G), np.complex128),
                     eq=np.zeros((F, G), np.complex128), syms=np.zeros((F, self.nData), np.complex128),
                     llr_demod=np.zeros((F, self.nBits), np.float32), llr_ldpc=np.zeros((F, 1600), np.float32),
                     variance=np.zeros(F, np.float64), agc_gain=np.zeros(F, np.float64), cycles=np.zeros(16, np.int64))
            if self.mfsk_M:      # no channel estimate / equalised grid on the MFSK path
                for k in ("H", "eq", "syms"):
                    del t[k]
            ts = Taps(**{k: v.ctypes.data for k, v in t.items()})
            self._ck(self.lib.mgpu_rx_batch_taps(self.h, _ptr(bb), F, _ptr(payload), _ptr(stats), C.byref(ts)))
            out.update(t)
        else:
            llr = np.zeros((F, 1600), np.float32) if want_llr else None
            self._ck(self.lib.mgpu_rx_batch(self.h, _ptr(bb), F, _ptr(payload), _ptr(stats), _ptr(llr)))
            if want_llr:
                out["llr_ldpc"] = llr
        return out

    # ---- diversity combining (include/mercury_diversity.h) -------------------------------------
    def receive_div(self, baseband, D, want_llr=False):
        """receive() for F = G * D frames of which each D consecutive ones are branches of one transmitted frame: every branch through the
        front-end, one decode per group on the sum of its branches' LLRs, the group's payload and decode result in every member row (with the
        branch's own variance and SNR). want_llr: the BRANCH LLRs, float32 [F, 1600]. D = 1 is receive()."""
        bb = np.ascontiguousarray(baseband, np.complex128).reshape(-1, self.frame_samples)
        F = bb.shape[0]
        payload = np.zeros((F, self.payload_stride), np.uint8)
        stats = np.zeros(F, STATS_DTYPE)
        llr = np.zeros((F, 1600), np.float32) if want_llr else None
        self._ck(self.lib.mgpu_rx_batch_div(self.h, _ptr(bb), F, int(D), _ptr(payload), _ptr(stats), _ptr(llr)))
        out = {"payload": payload, "stats": stats}
        if want_llr:
            out["llr_ldpc"] = llr
        return out

    def receive_div_dev(self, d_baseband, F, D, d_payload, d_stats, d_llr=None, stream=None):
        self._ck(self.lib.mgpu_rx_batch_div_dev(self.h, d_baseband, F, int(D), d_payload, d_stats, d_llr, stream))

    def llr_combine_dev(self, d_llr, F, d_out, D=None, groups=None, stream=None):
        """mgpu_llr_combine_dev on device pointers: the sums of uniform groups of D rows, or of `groups` ([[row, ...], ...]), into d_out."""
        D, first, member, G, _ = _group_args(F, D, groups)
        self._ck(self.lib.mgpu_llr_combine_dev(self.h, d_llr, F, D, _ptr(first), _ptr(member), G, d_out, stream))

    def llr_combine(self, llr, D=None, groups=None):
        """host_llr_combine() on the GPU: float32 [F, 1600] -> float32 [G, 1600]."""
        l = np.ascontiguousarray(llr, np.float32).reshape(-1, 1600)
        F = l.shape[0]
        rows = _group_args(F, D, groups)[4]
        out = np.zeros((rows, 1600), np.float32)
        self._staged([l], [out], "device allocation failed", lambda d_in, d_out: self.llr_combine_dev(d_in, F, d_out, D=D, groups=groups))
        return out

    def ldpc_decode(self, llr):
        """llr: float32 [F,1600] -> (bits uint8 [F,K], iterations int32 [F])  (cl_ldpc::decode)."""
        l = np.ascontiguousarray(llr, np.float32).reshape(-1, 1600)
        F = l.shape[0]
        bits = np.zeros((F, self.K), np.uint8)
        iters = np.zeros(F, np.int32)
        self._ck(self.lib.mgpu_ldpc_batch(self.h, _ptr(l), F, _ptr(bits), _ptr(iters)))
        return bits, iters

    # ---- device-buffer entry points (raw device pointers, e.g. torch tensor.data_ptr()) --------
    def ldpc_encode(self, bits):
        """cl_ldpc::encode: uint8 [F, K] (one byte per bit) -> uint8 [F, N]."""
        b = np.ascontiguousarray(bits, np.uint8)
        b = b.reshape(1, -1) if b.ndim == 1 else b
        if b.shape[1] != self.K:
            raise MgpuError("a data word is K = %d bits" % self.K)
        out = np.zeros((b.shape[0], self.N), np.uint8)
        self._ck(self.lib.mgpu_ldpc_encode_batch(self.h, _ptr(b), b.shape[0], _ptr(out)))
        return out

    def receive_dev(self, d_baseband, F, d_payload, d_stats, d_llr=None, stream=None):
        self._ck(self.lib.mgpu_rx_batch_dev(self.h, d_baseband, F, d_payload, d_stats, d_llr, stream))

    def frontend_dev(self, d_baseband, F, d_llr, d_variance=None, stream=None):
        self._ck(self.lib.mgpu_frontend_dev(self.h, d_baseband, F, d_llr, d_variance, stream))

    def ldpc_decode_dev(self, d_llr, F, d_bits=None, d_iters=None, d_payload=None, d_stats=None, d_variance=None, stream=None):
        self._ck(self.lib.mgpu_ldpc_batch_dev(self.h, d_llr, F, d_bits, d_iters, d_payload, d_stats, d_variance, stream))

    def txgen_dev(self, seed, frame0, F, noise_amp, d_baseband, d_payload=None, channel=0, stream=None):
        self._ck(self.lib.mgpu_txgen_dev(self.h, seed, frame0, F, noise_amp, channel, d_baseband, d_payload, stream))

    def baseband_test_esn0(self, esn0_db, frames_per_point, seed=1, frame0=0, channel=0, hf_channel=None, diversity=None):
        """cl_telecom_system::baseband_test_EsN0 per Es/N0 point (BER_PLOT_baseband): list of dicts with cl_error_rate's counters.
        hf_channel (HfChannel or preset name): the Watterson channel on each frame (mgpu_baseband_test_esn0_hf; `channel` must then be 0).
        diversity = D: D branches per payload, each with its own channel realisation and noise, decoded from their summed LLRs
        (mgpu_baseband_test_esn0_div); frames_per_point then counts payloads, and no hf_channel means AWGN."""
        pts = np.ascontiguousarray(np.atleast_1d(esn0_db), np.float64)
        out = (ErrorRate * pts.size)()
        if diversity is not None:
            if channel != 0:
                raise MgpuError("diversity runs on the HF channel loop: channel must be 0")
            ch = _hf("awgn" if hf_channel is None else hf_channel)
            self._ck(self.lib.mgpu_baseband_test_esn0_div(self.h, _ptr(pts), pts.size, frames_per_point, seed, frame0, C.byref(ch), int(diversity), out))
        elif hf_channel is None:
            self._ck(self.lib.mgpu_baseband_test_esn0(self.h, _ptr(pts), pts.size, frames_per_point, seed, frame0, channel, out))
        else:
            if channel != 0:
                raise MgpuError("hf_channel replaces the generator's static echo: channel must be 0")
            self._ck(self.lib.mgpu_baseband_test_esn0_hf(self.h, _ptr(pts), pts.size, frames_per_point, seed, frame0, C.byref(_hf(hf_channel)), out))
        return [{n: getattr(r, n) for n, _ in ErrorRate._fields_} for r in out]

    def hf_channel_apply(self, x, ch, seed, realisation0=0, fs=None, t0=0):
        """x: float64 [W, n] (real audio, fs default 48 kHz) or complex128 [W, n] (baseband, fs default 12 kHz) through the Watterson
        channel `ch` (HfChannel or preset name); signal w is realisation realisation0 + w. Returns an array shaped and typed like x."""
        cplx = np.iscomplexobj(x)
        a = np.ascontiguousarray(x, np.complex128 if cplx else np.float64)
        a2 = a.reshape(1, -1) if a.ndim == 1 else a
        out = np.empty_like(a2)
        fs = (12000.0 if cplx else 48000.0) if fs is None else fs
        self._ck(self.lib.mgpu_hf_channel_apply(self.h, C.byref(_hf(ch)), _ptr(a2), int(cplx), fs, a2.shape[0], a2.shape[1], seed, realisation0, t0,
                                                _ptr(out)))
        return out.reshape(a.shape)

    def hf_channel_apply_dev(self, d_in, d_out, W, n, ch, seed, complex_input, realisation0=0, fs=None, t0=0, stream=None):
        """Device-buffer form (raw pointers, e.g. tensor.data_ptr()); enqueued on `stream` (None: the context's stream), asynchronous."""
        fs = (12000.0 if complex_input else 48000.0) if fs is None else fs
        self._ck(self.lib.mgpu_hf_channel_apply_dev(self.h, C.byref(_hf(ch)), d_in, int(complex_input), fs, W, n, seed, realisation0, t0, d_out,
                                                    stream))

    def debug_mfsk_sync(self, energy, size, search_start, variant):
        """Test hook: cl_ofdm::time_sync_mfsk's search on slot energies [W, nslots, Nc]; variant 0 host, 1 device kernel -> delay [W]."""
        e = np.ascontiguousarray(energy, np.float64)
        W, nslots = e.shape[0], e.shape[1]
        ss = None if search_start is None else np.ascontiguousarray(search_start, np.int32)
        d = np.zeros(W, np.int32)
        self._ck(self.lib.mgpu_debug_mfsk_sync(self.h, _ptr(e), W, nslots, size, _ptr(ss), variant, _ptr(d)))
        return d

    def debug_p2b_variant(self, variant):
        """Test hook (process-wide): -1 = sliding-tap passband_to_baseband kernels where they apply, 0 = generic kernel. Returns the old value."""
        return int(self.lib.mgpu_debug_p2b_variant(variant))

    def debug_span_energy(self, z, wv, off, length, variant):
        """Test hook: (sum, count) of |z|^2 over `length` samples from off[j] in window wv[j] (clipped at the window end), sample order."""
        z = np.ascontiguousarray(z, np.complex128)
        wv = np.ascontiguousarray(wv, np.int32)
        off = np.ascontiguousarray(off, np.int32)
        s = np.zeros(wv.size, np.float64)
        c = np.zeros(wv.size, np.int32)
        self._ck(self.lib.mgpu_debug_span_energy(self.h, _ptr(z), z.shape[0], z.shape[1], _ptr(wv), _ptr(off), wv.size, length, variant, _ptr(s), _ptr(c)))
        return s, c

    def passband_test_esn0(self, esn0_db, frames_per_point, carrier_hz, seed=1, frame0=0, want_windows=False, output_power_watt=0.1, hf_channel=None):
        """cl_telecom_system::passband_test_EsN0 per Es/N0 point (PLOT_PASSBAND): list of cl_error_rate dicts [, windows, sent].
        hf_channel (HfChannel or preset name): the Watterson channel in front of the noise (mgpu_passband_test_esn0_hf)."""
        pts = np.ascontiguousarray(np.atleast_1d(esn0_db), np.float64)
        out = (ErrorRate * pts.size)()
        win = sent = None
        if want_windows:
            win = np.zeros((pts.size * frames_per_point, self.receive_buffer_samples()), np.float64)
            sent = np.zeros((pts.size * frames_per_point, self.payload_stride), np.uint8)
        if hf_channel is None:
            self._ck(self.lib.mgpu_passband_test_esn0(self.h, _ptr(pts), pts.size, frames_per_point, seed, frame0, carrier_hz, output_power_watt, out,
                                                      _ptr(win) if want_windows else None, _ptr(sent) if want_windows else None))
        else:
            self._ck(self.lib.mgpu_passband_test_esn0_hf(self.h, _ptr(pts), pts.size, frames_per_point, seed, frame0, carrier_hz, output_power_watt,
                                                         C.byref(_hf(hf_channel)), out, _ptr(win) if want_windows else None,
                                                         _ptr(sent) if want_windows else None))
        res = [{n: getattr(r, n) for n, _ in ErrorRate._fields_} for r in out]
        return (res, win, sent) if want_windows else res

    # ---- synchroniser building blocks -------------------------------------------
    def passband_to_baseband(self, passband, carrier_hz, which=0, start=None, count=None, decimation=1):
        """passband: float64 [W, in_size]; carrier_hz scalar or [W]. -> complex128 [W, count]."""
        x = np.ascontiguousarray(passband, np.float64)
        x = x.reshape(1, -1) if x.ndim == 1 else x
        W, n = x.shape
        fc = np.ascontiguousarray(np.broadcast_to(np.asarray(carrier_hz, np.float64), (W,)))
        st = None if start is None else np.ascontiguousarray(np.broadcast_to(np.asarray(start, np.int32), (W,)))
        if count is None:
            count = (n + decimation - 1) // decimation
        out = np.zeros((W, count), np.complex128)
        self._ck(self.lib.mgpu_passband_to_baseband(self.h, _ptr(x), W, n, _ptr(fc), which, _ptr(st), count, decimation, _ptr(out)))
        return out

    def time_sync_preamble(self, baseband_interp, step, location_to_return=0, nTrials_max=1):
        z = np.ascontiguousarray(baseband_interp, np.complex128)
        z = z.reshape(1, -1) if z.ndim == 1 else z
        W, size = z.shape
        delay = np.zeros(W, np.int32)
        corr = np.zeros(W, np.float64)
        self._ck(self.lib.mgpu_time_sync_preamble(self.h, _ptr(z), W, size, step, location_to_return, nTrials_max, _ptr(delay), _ptr(corr)))
        return delay, corr

    def debug_tsync_metric(self, baseband_interp, step, variant=-1, start=None, sub_size=None):
        """Test hook: the Schmidl-Cox metric of every candidate, [W][ncand]; variant 0 = staged kernel, 1 = streaming kernel;
        start / sub_size: per-window sub-range to search."""
        z = np.ascontiguousarray(baseband_interp, np.complex128)
        z = z.reshape(1, -1) if z.ndim == 1 else z
        W, size = z.shape
        L = self.preamble_nsymb * self.Nofdm * 4
        ncand = (size - L + step - 1) // step
        vals = np.zeros((W, ncand), np.float64)
        st = None if start is None else np.ascontiguousarray(start, np.int32)
        sz = None if sub_size is None else np.ascontiguousarray(sub_size, np.int32)
        self._ck(self.lib.mgpu_debug_tsync_metric(self.h, _ptr(z), W, size, step, variant,
                                                  _ptr(st) if st is not None else None, _ptr(sz) if sz is not None else None, _ptr(vals)))
        return vals

    def freq_sync(self, baseband):
        z = np.ascontiguousarray(baseband, np.complex128)
        z = z.reshape(1, -1) if z.ndim == 1 else z
        W, stride = z.shape
        out = np.zeros(W, np.float64)
        self._ck(self.lib.mgpu_freq_sync(self.h, _ptr(z), W, stride, _ptr(out)))
        return out

    def time_sync_mfsk(self, baseband_interp, search_start_symb=0):
        """cl_ofdm::time_sync_mfsk on W windows of interpolated baseband -> delay [W] (MFSK modes only)."""
        z = np.ascontiguousarray(baseband_interp, np.complex128)
        z = z.reshape(1, -1) if z.ndim == 1 else z
        W, size = z.shape
        delay = np.zeros(W, np.int32)
        self._ck(self.lib.mgpu_time_sync_mfsk(self.h, _ptr(z), W, size, search_start_symb, _ptr(delay)))
        return delay

    def detect_ack_pattern(self, baseband_interp, pattern=1):
        """cl_ofdm::detect_ack_pattern (pattern 1 = ACK, 2 = BREAK) -> (metric [W], matched [W])."""
        z = np.ascontiguousarray(baseband_interp, np.complex128)
        z = z.reshape(1, -1) if z.ndim == 1 else z
        W, size = z.shape
        metric = np.zeros(W, np.float64)
        matched = np.zeros(W, np.int32)
        self._ck(self.lib.mgpu_detect_ack_pattern(self.h, _ptr(z), W, size, pattern, _ptr(metric), _ptr(matched)))
        return metric, matched

    def detect_ack_pattern_from_passband(self, passband, carrier_hz, pattern=1):
        """detect_ack_pattern_from_passband / detect_break_pattern_from_passband (telecom_system.cc:1628-1710)."""
        x = np.ascontiguousarray(passband, np.float64)
        x = x.reshape(1, -1) if x.ndim == 1 else x
        W, size = x.shape
        metric = np.zeros(W, np.float64)
        matched = np.zeros(W, np.int32)
        self._ck(self.lib.mgpu_detect_ack_pattern_from_passband(self.h, _ptr(x), W, size, carrier_hz, pattern, _ptr(metric), _ptr(matched)))
        return metric, matched

    # ---- the whole of receive_byte on capture windows (include/mercury_rxloop.h) -------------
    def receive_buffer_samples(self):
        return int(self.lib.mgpu_receive_buffer_nsymb(self.h)) * self.Nofdm * 4

    def receive_byte(self, passband, carrier_hz, trials_max=2, use_last_good_time_sync=1, use_last_good_freq_offset=1, state=None,
                     coarse_freq_sync=0):
        """passband: [W, buffer samples] float64 - or the audio device's own samples, int32 (x / INT_MAX), int16 (x / 32768) or float32, which
        are widened on the device as the reference's capture thread widens them (audioio.c:893-936): same results, half / a quarter of the bytes
        over PCIe. Returns dict(payload [W, stride], stats [W] (RECEIVE_STATS_DTYPE), state)."""
        fmt = {np.dtype(np.int32): 1, np.dtype(np.int16): 2, np.dtype(np.float32): 3}.get(np.asarray(passband).dtype, 0)
        x = np.ascontiguousarray(passband, np.asarray(passband).dtype if fmt else np.float64)
        x = x.reshape(1, -1) if x.ndim == 1 else x
        W, n = x.shape
        if n != self.receive_buffer_samples():
            raise MgpuError("a capture window is %d samples" % self.receive_buffer_samples())
        cfg = ReceiveConfig(carrier_hz, trials_max, use_last_good_time_sync, use_last_good_freq_offset, coarse_freq_sync)
        st = np.zeros(W, LINK_STATE_DTYPE) if state is None else np.ascontiguousarray(state, LINK_STATE_DTYPE)
        if state is None:
            st["delay_of_last_decoded_message"] = -1
        payload = np.zeros((W, self.payload_stride), np.uint8)
        stats = np.zeros(W, RECEIVE_STATS_DTYPE)
        if fmt:
            self._ck(self.lib.mgpu_receive_byte_batch_samples(self.h, _ptr(x), fmt, W, C.byref(cfg), _ptr(st), _ptr(payload), _ptr(stats)))
        else:
            self._ck(self.lib.mgpu_receive_byte_batch(self.h, _ptr(x), W, C.byref(cfg), _ptr(st), _ptr(payload), _ptr(stats)))
        return {"payload": payload, "stats": stats, "state": st}

    def transmit_frame_samples(self):
        return int(self.lib.mgpu_transmit_frame_samples(self.h))

    def transmit_config(self, carrier_hz, message_location=SINGLE_MESSAGE, start_sample=0, phase_continuous=0, carrier_amplitude=None,
                        output_power_watt=0.1, preamble_papr_cut=7.0, data_papr_cut=10.0):
        """The reference's defaults (telecom_system.cc:69, physical_config.cc:88,115-116) around the given carrier."""
        amp = float(np.sqrt(2.0)) if carrier_amplitude is None else carrier_amplitude
        return TransmitConfig(carrier_hz, amp, output_power_watt, preamble_papr_cut, data_papr_cut, start_sample, message_location,
                              phase_continuous)

    def transmit_buffer(self, buffer=None):
        """passband_data_tx_buffer of the FIRST / MIDDLE / FLUSH_MESSAGE calls: read it (buffer=None) or replace it."""
        n = 3 * self.transmit_frame_samples()
        if buffer is None:
            out = np.zeros(n)
            self._ck(self.lib.mgpu_transmit_buffer(self.h, _ptr(out), 0))
            return out
        b = np.ascontiguousarray(buffer, np.float64)
        if b.size != n:
            raise MgpuError("the transmit buffer is 3 frames = %d samples" % n)
        self._ck(self.lib.mgpu_transmit_buffer(self.h, _ptr(b), 1))
        return b

    def pre_equalization_channel(self, carrier_hz):
        """cl_telecom_system::get_pre_equalization_channel for this mode and carrier (host computation): complex128 [Nc]."""
        out = np.zeros(self.Nc, np.complex128)
        self._ck(self.lib.mgpu_context_pre_equalization_channel(self.h, carrier_hz, _ptr(out)))
        return out

    def set_pre_equalization_channel(self, channel):
        """Install (complex128 [Nc]) or remove (None) the table transmit_bit multiplies the carrier grids with."""
        if channel is None:
            self._ck(self.lib.mgpu_set_pre_equalization_channel(self.h, None))
        else:
            ch = np.ascontiguousarray(channel, np.complex128)
            assert ch.size == self.Nc
            self._ck(self.lib.mgpu_set_pre_equalization_channel(self.h, _ptr(ch)))

    def transmit_byte(self, payload, carrier_hz, nbytes=None, **kw):
        """cl_telecom_system::transmit_byte for F messages: payload uint8 [F, >= payload_bytes] -> float64 [F, total_frame_size]."""
        pl = np.ascontiguousarray(payload, np.uint8)
        pl = pl.reshape(1, -1) if pl.ndim == 1 else pl
        F, stride = pl.shape
        cfg = self.transmit_config(carrier_hz, **kw)
        nb = None if nbytes is None else np.ascontiguousarray(nbytes, np.int32)
        out = np.zeros((F, self.transmit_frame_samples()), np.float64)
        self._ck(self.lib.mgpu_transmit_byte_batch(self.h, _ptr(pl), stride, None if nb is None else _ptr(nb), F, C.byref(cfg),
                                                   _ptr(out)))
        return out

    def transmit_bit(self, bits, carrier_hz, **kw):
        """cl_telecom_system::transmit_bit for F frames: uint8 [F, nReal] data bits -> float64 [F, total_frame_size]."""
        b = np.ascontiguousarray(bits, np.uint8).reshape(-1, self.nReal)
        cfg = self.transmit_config(carrier_hz, **kw)
        out = np.zeros((b.shape[0], self.transmit_frame_samples()), np.float64)
        self._ck(self.lib.mgpu_transmit_bit_batch(self.h, _ptr(b), b.shape[0], C.byref(cfg), _ptr(out)))
        return out

    def transmit_byte_dev(self, d_payload, payload_stride, F, d_passband, carrier_hz, d_nbytes=None, stream=None, **kw):
        cfg = self.transmit_config(carrier_hz, **kw)
        self._ck(self.lib.mgpu_transmit_byte_batch_dev(self.h, d_payload, payload_stride, d_nbytes, F, C.byref(cfg), d_passband, stream))

    def generate_ack_pattern_passband(self, pattern=1, carrier_hz=None, **kw):
        """cl_telecom_system::generate_ack_pattern_passband (pattern 1) / generate_break_pattern_passband (2) -> float64 [16*Nofdm*4]."""
        cfg = self.transmit_config(carrier_hz, **kw)
        out = np.zeros(16 * self.Nofdm * 4, np.float64)
        self._ck(self.lib.mgpu_generate_ack_pattern_passband(self.h, pattern, C.byref(cfg), _ptr(out)))
        return out

    def symbol_mod(self, carriers):
        """cl_ofdm::symbol_mod: complex128 [n, Nc] -> [n, Nofdm]."""
        x = np.ascontiguousarray(carriers, np.complex128).reshape(-1, self.Nc)
        out = np.zeros((x.shape[0], self.Nofdm), np.complex128)
        self._ck(self.lib.mgpu_symbol_mod(self.h, _ptr(x), x.shape[0], _ptr(out)))
        return out

    def measure_signal_only(self, passband, carrier_hz):
        """cl_telecom_system::measure_signal_only: float64 [W, buffer samples] -> signal strength in dBm per window."""
        x = np.ascontiguousarray(passband, np.float64)
        x = x.reshape(1, -1) if x.ndim == 1 else x
        if x.shape[1] != self.receive_buffer_samples():
            raise MgpuError("a capture window is %d samples" % self.receive_buffer_samples())
        out = np.zeros(x.shape[0], np.float64)
        self._ck(self.lib.mgpu_measure_signal_only(self.h, _ptr(x), x.shape[0], carrier_hz, _ptr(out)))
        return out

    def receive_byte_dev(self, d_passband, W, carrier_hz, trials_max=2, use_last_good_time_sync=1, use_last_good_freq_offset=1, state=None,
                         coarse_freq_sync=0):
        """receive_byte on W capture windows that already lie in device memory (d_passband: raw pointer); host results as above."""
        cfg = ReceiveConfig(carrier_hz, trials_max, use_last_good_time_sync, use_last_good_freq_offset, coarse_freq_sync)
        st = np.zeros(W, LINK_STATE_DTYPE) if state is None else np.ascontiguousarray(state, LINK_STATE_DTYPE)
        if state is None:
            st["delay_of_last_decoded_message"] = -1
        payload = np.zeros((W, self.payload_stride), np.uint8)
        stats = np.zeros(W, RECEIVE_STATS_DTYPE)
        self._ck(self.lib.mgpu_receive_byte_batch(self.h, d_passband, W, C.byref(cfg), _ptr(st), _ptr(payload), _ptr(stats)))
        return {"payload": payload, "stats": stats, "state": st}

    def receive_byte_samples_dev(self, d_capture, sample_format, W, carrier_hz, trials_max=2, use_last_good_time_sync=1, use_last_good_freq_offset=1,
                                 state=None, coarse_freq_sync=0):
        """receive_byte on W capture windows of INT32 (1) / INT16 (2) / FLOAT32 (3) samples in device memory (raw pointer)."""
        cfg = ReceiveConfig(carrier_hz, trials_max, use_last_good_time_sync, use_last_good_freq_offset, coarse_freq_sync)
        st = np.zeros(W, LINK_STATE_DTYPE) if state is None else np.ascontiguousarray(state, LINK_STATE_DTYPE)
        if state is None:
            st["delay_of_last_decoded_message"] = -1
        payload = np.zeros((W, self.payload_stride), np.uint8)
        stats = np.zeros(W, RECEIVE_STATS_DTYPE)
        self._ck(self.lib.mgpu_receive_byte_batch_samples(self.h, d_capture, sample_format, W, C.byref(cfg), _ptr(st),
                                                          _ptr(payload), _ptr(stats)))
        return {"payload": payload, "stats": stats, "state": st}

    def last_sync_kernel_ms(self):
        ms = C.c_float(0)
        self._ck(self.lib.mgpu_last_sync_kernel_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def debug_glibc_trig(self, x):
        """Device atan / sin / cos (csrc/glibc_trig.h) of a float64 array."""
        xin = np.ascontiguousarray(x, np.float64)
        a, s, c = np.zeros_like(xin), np.zeros_like(xin), np.zeros_like(xin)
        self._ck(self.lib.mgpu_debug_glibc_trig(self.h, _ptr(xin), xin.size, _ptr(a), _ptr(s), _ptr(c)))
        return a, s, c

    def debug_spa_math(self, x):
        """Device tanh / atanh (csrc/spa_math.h) of a float64 array -> (tanh, atanh[0 where |x|>=1])."""
        xin = np.ascontiguousarray(x, np.float64).ravel()
        t = np.zeros_like(xin)
        a = np.zeros_like(xin)
        self._ck(self.lib.mgpu_debug_spa_math(self.h, _ptr(xin), xin.size, _ptr(t), _ptr(a)))
        return t, a

    def enable_timing(self, on=True):
        self._ck(self.lib.mgpu_enable_timing(self.h, 1 if on else 0))

    def host_path_last(self):
        """Profile of the last chunked mgpu_rx_batch call: dict(chunk_frames, n_chunks, fill_ms, drain_ms, total_ms)."""
        a, b = C.c_int(), C.c_int()
        f, d, t = C.c_float(), C.c_float(), C.c_float()
        self._ck(self.lib.mgpu_host_path_last(self.h, C.byref(a), C.byref(b), C.byref(f), C.byref(d), C.byref(t)))
        return {"chunk_frames": a.value, "n_chunks": b.value, "fill_ms": f.value, "drain_ms": d.value, "total_ms": t.value}

    def decoder_hard_frames(self):
        """Frames the fp64 decoder has decided without iterating since this context was created (every |LLR| >= 200 and an odd parity check)."""
        n = C.c_longlong(0)
        self._ck(self.lib.mgpu_decoder_hard_frames(self.h, C.byref(n)))
        return int(n.value)

    def kernel_ms_avg(self):
        """(front-end ms, decoder ms, launches) averaged over the launches since enable_timing()."""
        ms = (C.c_float * 2)()
        n = C.c_int(0)
        self._ck(self.lib.mgpu_kernel_ms_avg(self.h, ms, C.byref(n)))
        return float(ms[0]), float(ms[1]), int(n.value)


# ---- multi-GPU pool (include/mercury_pool.h) ------------------------------------------------------------------------------
POOL_MAX_DEVICES = 16


class ErrorRate(C.Structure):
    """mgpu_error_rate: cl_error_rate's counters for one Es/N0 point."""
    _fields_ = [("esn0_db", C.c_double), ("Frames_total", C.c_longlong), ("Error_frames_total", C.c_longlong), ("Bits_total", C.c_longlong),
                ("Error_bits_total", C.c_longlong), ("BER", C.c_double), ("FER", C.c_double), ("avg_iterations", C.c_double),
                ("crc_ok_frames", C.c_longlong)]


class PoolCounters(C.Structure):
    _fields_ = [("n_devices", C.c_int), ("frames", C.c_longlong), ("decoded", C.c_longlong), ("ldpc_iterations", C.c_longlong),
                ("wall_ms", C.c_double), ("device_frames", C.c_int * POOL_MAX_DEVICES), ("device_ms", C.c_double * POOL_MAX_DEVICES)]


def pool_shard(F, G, g):
    """Frames of device g of G: (first, count) — mgpu_pool_shard, callable without a GPU."""
    lib = load_library()
    a, n = C.c_int(), C.c_int()
    lib.mgpu_pool_shard(F, G, g, C.byref(a), C.byref(n))
    return a.value, n.value


class RxPool(_Handle):
    """One context + one host worker thread per device; a call is split into contiguous frame ranges (mgpu_pool_*)."""
    _destroy = "mgpu_pool_destroy"

    def __init__(self, cfg, devices, max_iters=50, decoder=DEC_SPA, agc=1, variance_source=1, max_batch=4096, minsum_alpha=0.0,
                 mfsk_ctrl_mode=False):
        self.lib = load_library()
        self.h = C.c_void_p()
        c = Config(cfg, max_iters, decoder, agc, variance_source, 0, max_batch, minsum_alpha, 1 if mfsk_ctrl_mode else 0)
        devs = (C.c_int * len(devices))(*devices)
        rc = self.lib.mgpu_pool_create(C.byref(c), devs, len(devices), C.byref(self.h))
        if rc != 0:
            raise MgpuError("mgpu_pool_create failed (%d): %s" % (rc, self.lib.mgpu_pool_last_error(None).decode()))
        self.n_devices = len(devices)
        i = Info()
        self._ctx0 = self._ctx(0)
        if self.lib.mgpu_get_info(self._ctx0, C.byref(i)) != 0:
            raise MgpuError("mgpu_get_info failed")
        for n in INFO_FIELDS:
            setattr(self, n, getattr(i, n))

    def _ctx(self, g):
        return self.lib.mgpu_pool_context(self.h, g)

    def numa_nodes(self):
        """NUMA node of every context's device (mgpu_pool_device_numa_node; -1: the platform names none)."""
        return [int(self.lib.mgpu_pool_device_numa_node(self.h, g)) for g in range(self.n_devices)]

    def _ck(self, rc):
        if rc != 0:
            raise MgpuError("mgpu pool error %d: %s" % (rc, self.lib.mgpu_pool_last_error(self.h).decode()))

    def counters(self):
        c = PoolCounters()
        self._ck(self.lib.mgpu_pool_last_counters(self.h, C.byref(c)))
        return {"n_devices": c.n_devices, "frames": c.frames, "decoded": c.decoded, "ldpc_iterations": c.ldpc_iterations, "wall_ms": c.wall_ms,
                "device_frames": list(c.device_frames)[: c.n_devices], "device_ms": list(c.device_ms)[: c.n_devices]}

    def receive(self, baseband):
        bb = np.ascontiguousarray(baseband, np.complex128).reshape(-1, self.frame_samples)
        F = bb.shape[0]
        payload = np.zeros((F, self.payload_stride), np.uint8)
        stats = np.zeros(F, STATS_DTYPE)
        self._ck(self.lib.mgpu_pool_rx_batch(self.h, _ptr(bb), F, _ptr(payload), _ptr(stats)))
        return {"payload": payload, "stats": stats}

    def ldpc_decode(self, llr):
        l = np.ascontiguousarray(llr, np.float32).reshape(-1, 1600)
        F = l.shape[0]
        bits = np.zeros((F, self.K), np.uint8)
        iters = np.zeros(F, np.int32)
        self._ck(self.lib.mgpu_pool_ldpc_batch(self.h, _ptr(l), F, _ptr(bits), _ptr(iters)))
        return bits, iters

    # ---- device-resident shards: one pointer and one count per pool device (mercury_pool.h) ----
    @staticmethod
    def _ptrs(ptrs, n):
        if ptrs is None:
            return None
        assert len(ptrs) == n
        return (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in ptrs])

    def shard(self, F):
        """The split the host-buffer calls use: [(first, count)] per device."""
        out = []
        for g in range(self.n_devices):
            a, b = C.c_int(), C.c_int()
            self.lib.mgpu_pool_shard(F, self.n_devices, g, C.byref(a), C.byref(b))
            out.append((a.value, b.value))
        return out

    def device_malloc(self, g, nbytes):
        p = self.lib.mgpu_device_malloc(self._ctx(g), nbytes)
        if not p:
            raise MgpuError("mgpu_device_malloc(%d bytes) failed on pool device %d" % (nbytes, g))
        return p

    def device_free(self, g, ptr):
        self.lib.mgpu_device_free(self._ctx(g), ptr)

    def copy_to_host(self, g, dst, d_src):
        """dst: a numpy array; blocking copy from pool device g."""
        rc = self.lib.mgpu_copy_to_host(self._ctx(g), _ptr(dst), d_src, dst.nbytes, None)
        if rc != 0:
            raise MgpuError("mgpu_copy_to_host failed (%d)" % rc)
        return dst

    def copy_to_device(self, g, d_dst, src):
        src = np.ascontiguousarray(src)
        rc = self.lib.mgpu_copy_to_device(self._ctx(g), d_dst, _ptr(src), src.nbytes, None)
        if rc != 0:
            raise MgpuError("mgpu_copy_to_device failed (%d)" % rc)

    def txgen_dev(self, seed, frame0, counts, noise_amp, d_bb, d_payload=None, channel=0):
        n = self.n_devices
        cnt = (C.c_int * n)(*counts)
        self._ck(self.lib.mgpu_pool_txgen_dev(self.h, seed, frame0, cnt, noise_amp, channel,
                                              self._ptrs(d_bb, n), self._ptrs(d_payload, n)))

    def receive_dev(self, d_bb, counts, d_payload, d_stats):
        n = self.n_devices
        cnt = (C.c_int * n)(*counts)
        self._ck(self.lib.mgpu_pool_rx_batch_dev(self.h, self._ptrs(d_bb, n), cnt, self._ptrs(d_payload, n), self._ptrs(d_stats, n)))

    def ldpc_decode_dev(self, d_llr, counts, d_bits, d_iters):
        n = self.n_devices
        cnt = (C.c_int * n)(*counts)
        self._ck(self.lib.mgpu_pool_ldpc_batch_dev(self.h, self._ptrs(d_llr, n), cnt, self._ptrs(d_bits, n), self._ptrs(d_iters, n)))

    def enable_timing(self, on=True):
        for g in range(self.n_devices):
            self.lib.mgpu_enable_timing(self._ctx(g), 1 if on else 0)

    def decoder_hard_frames(self):
        """Frames the pool's fp64 decoders have decided without iterating since the pool was created (sum over its devices)."""
        total = 0
        for g in range(self.n_devices):
            n = C.c_longlong(0)
            self.lib.mgpu_decoder_hard_frames(self._ctx(g), C.byref(n))
            total += int(n.value)
        return total

    def kernel_ms(self, g):
        """(front-end ms, decoder ms, launches) averaged since enable_timing on pool device g."""
        ms = (C.c_float * 2)()
        n = C.c_int()
        self.lib.mgpu_kernel_ms_avg(self._ctx(g), ms, C.byref(n))
        return float(ms[0]), float(ms[1]), n.value

    def receive_buffer_samples(self):
        return int(self.lib.mgpu_receive_buffer_nsymb(self._ctx0)) * self.Nofdm * 4

    def receive_byte(self, passband, carrier_hz, trials_max=2, use_last_good_time_sync=1, use_last_good_freq_offset=1, state=None,
                     coarse_freq_sync=0, W=None):
        """passband: float64 [W, buffer samples] in host memory, or (with W given) a raw device pointer when every context of the pool
        sits on the device that holds the windows (contexts time-sharing one GPU)."""
        if W is None:
            x = np.ascontiguousarray(passband, np.float64)
            x = x.reshape(1, -1) if x.ndim == 1 else x
            W, src = x.shape[0], _ptr(x)
        else:
            src = passband
        cfg = ReceiveConfig(carrier_hz, trials_max, use_last_good_time_sync, use_last_good_freq_offset, coarse_freq_sync)
        st = np.zeros(W, LINK_STATE_DTYPE) if state is None else np.ascontiguousarray(state, LINK_STATE_DTYPE)
        if state is None:
            st["delay_of_last_decoded_message"] = -1
        payload = np.zeros((W, self.payload_stride), np.uint8)
        stats = np.zeros(W, RECEIVE_STATS_DTYPE)
        self._ck(self.lib.mgpu_pool_receive_byte_batch(self.h, src, W, C.byref(cfg), _ptr(st), _ptr(payload), _ptr(stats)))
        return {"payload": payload, "stats": stats, "state": st}


# ---- the receive loop over continuous captures (include/mercury_capture.h) ------------------------------------------------------------
CAPTURE_SYMBOLS = names("mercury_capture.h")
CAPTURE_HELD_DTYPE = np.dtype([("iterations_done", "<i4"), ("message_decoded", "<i4"), ("crc", "<i4"), ("all_zeros", "<i4"), ("delay", "<i4"),
                               ("sync_trials", "<i4"), ("frame_overflow_symbols", "<i4"), ("snr_db", "<f8"), ("freq_offset", "<f8"),
                               ("coarse_metric", "<f8"), ("signal_strength_dbm", "<f8")], align=True)
CAPTURE_STATE_DTYPE = np.dtype([("frames_to_read", "<i4"), ("n_under", "<i4"), ("data_ready", "<i4"), ("mfsk_search_raw", "<i4"),
                                ("link", LINK_STATE_DTYPE), ("held", CAPTURE_HELD_DTYPE)], align=True)
CAPTURE_EVENT_DTYPE = np.dtype([("capture", "<i4"), ("hop", "<i4"), ("stats", RECEIVE_STATS_DTYPE)], align=True)
SAMPLE_FORMATS = {np.dtype(np.float64): 0, np.dtype(np.int32): 1, np.dtype(np.int16): 2, np.dtype(np.float32): 3}


class CaptureGeometry(C.Structure):     # mgpu_capture_geometry
    _fields_ = [("buffer_nsymb", C.c_int), ("nsymb", C.c_int), ("preamble_nsymb", C.c_int), ("symbol_period", C.c_int), ("mfsk", C.c_int)]


def _sample_format(dtype):
    fmt = SAMPLE_FORMATS.get(np.dtype(dtype))
    if fmt is None:
        raise MgpuError("capture samples are float64, int32, int16 or float32, not %s" % np.dtype(dtype))
    return fmt


def host_capture_init_state(geometry):
    """the state a capture starts with (mgpu_host_capture_init_state)"""
    st = np.zeros((), CAPTURE_STATE_DTYPE)
    if load_library().mgpu_host_capture_init_state(C.byref(geometry), _ptr(st)) != 0:
        raise MgpuError("mgpu_host_capture_init_state: bad geometry")
    return st


def host_capture_prep(geometry, window, samples, state):
    """one hop of capture prep (audioio.c:1035-1057) on a host window, in place: window float64 [buffer samples], samples [P] of a sample
    format, state a CAPTURE_STATE_DTYPE scalar array (updated)"""
    x = np.ascontiguousarray(samples)
    assert window.dtype == np.float64 and window.flags.c_contiguous and window.size == geometry.buffer_nsymb * geometry.symbol_period
    assert x.size == geometry.symbol_period and state.dtype == CAPTURE_STATE_DTYPE
    _twin(load_library().mgpu_host_capture_prep, C.byref(geometry), _ptr(window), _ptr(x), _sample_format(x.dtype), _ptr(state))


def host_capture_process(geometry, state, stats=None, link=None):
    """the process step's bookkeeping (telecom_system.cc:2304-2377) given receive_byte's result on the window (stats: RECEIVE_STATS_DTYPE
    scalar, link: LINK_STATE_DTYPE scalar as receive_byte left it; only read when the step runs receive_byte). Returns whether it did."""
    r = None if stats is None else np.ascontiguousarray(stats, RECEIVE_STATS_DTYPE)
    ls = None if link is None else np.ascontiguousarray(link, LINK_STATE_DTYPE)
    rc = load_library().mgpu_host_capture_process(C.byref(geometry), _ptr(state), _ptr(r), _ptr(ls))
    if rc < 0:
        raise MgpuError("mgpu_host_capture_process: bad argument (%d)" % rc)
    return bool(rc)


def _event_buffers(rows, payload_stride):
    """the arrays a run writes its events and their payloads into, `rows` of each"""
    return np.zeros(rows, CAPTURE_EVENT_DTYPE), np.zeros((rows, payload_stride), np.uint8)


def _event_list(ev, pl, n, m, payload_bytes):
    """the first min(n, m) events as (capture, hop, stats, payload bytes)"""
    return [(int(ev[i]["capture"]), int(ev[i]["hop"]), ev[i]["stats"].copy(), pl[i, :payload_bytes].copy()) for i in range(min(n, m))]


def _real_samples(samples):
    """-> (pointer, MGPU_SAMPLES_* format, count, keep-alive): real samples in a capture format, a numpy array or a contiguous torch
    tensor (read in place)"""
    if hasattr(samples, "data_ptr"):                       # a device tensor
        import torch
        fmt = {torch.float64: 0, torch.int32: 1, torch.int16: 2, torch.float32: 3}.get(samples.dtype)
        if fmt is None or not samples.is_contiguous():
            raise MgpuError("device samples: a contiguous float64 / int32 / int16 / float32 tensor")
        return samples.data_ptr(), fmt, samples.numel(), samples
    x = np.ascontiguousarray(samples)
    return _ptr(x), _sample_format(x.dtype), x.size, x


class RxCapture(_Handle):
    """S continuous captures on one RxPhy context: the reference's capture-prep thread and RX_SHM_process_main, batched on the GPU
    (include/mercury_capture.h). Samples go in as [S, H * P] arrays of float64 / int32 / int16 / float32 (numpy, or torch tensors on the
    context's device, read in place)."""
    _destroy = "mgpu_capture_destroy"

    def __init__(self, rx, S, carrier_hz, trials_max=2, use_last_good_time_sync=1, use_last_good_freq_offset=1, coarse_freq_sync=0,
                 initial_windows=None, max_hops=0, ladder=None):
        """ladder: rungs as RxPhy.set_estimator_ladder takes them, set on the context `rx` (RxPhy.set_estimator_ladder) before the capture is made; None: as it is"""
        self.rx, self.lib, self.S = rx, rx.lib, S
        if ladder is not None:
            rx.set_estimator_ladder(ladder)
        self.h = C.c_void_p()
        cfg = ReceiveConfig(carrier_hz, trials_max, use_last_good_time_sync, use_last_good_freq_offset, coarse_freq_sync)
        init = None
        if initial_windows is not None:
            init = np.ascontiguousarray(initial_windows, np.float64).reshape(S, -1)
        rx._ck(self.lib.mgpu_capture_create(rx.h, S, C.byref(cfg), _ptr(init), max_hops, C.byref(self.h)))
        self._read_geometry()

    def _read_geometry(self):
        self.geometry = CaptureGeometry()
        self.rx._ck(self.lib.mgpu_capture_geometry_get(self.h, C.byref(self.geometry)))
        self.P = self.geometry.symbol_period
        self.window_samples = self.geometry.buffer_nsymb * self.P
        self.payload_stride = self.rx.payload_stride

    def _samples(self, samples):
        """-> (pointer, format, H, keep-alive)"""
        ptr, fmt, n, keep = _real_samples(samples)
        if n % (self.S * self.P):
            raise MgpuError("samples must be [S, H * P] with P = %d" % self.P)
        return ptr, fmt, n // (self.S * self.P), keep

    def feed(self, samples):
        ptr, fmt, H, _keep = self._samples(samples)
        self.rx._ck(self.lib.mgpu_capture_feed(self.h, ptr, fmt, H))

    def process(self):
        """-> dict(ran [S] bool, stats [S] RECEIVE_STATS_DTYPE, payload [S, stride]); stats / payload are zero where ran is False"""
        ran = np.zeros(self.S, np.int32)
        stats = np.zeros(self.S, RECEIVE_STATS_DTYPE)
        payload = np.zeros((self.S, self.payload_stride), np.uint8)
        self.rx._ck(self.lib.mgpu_capture_process(self.h, _ptr(ran), _ptr(stats), _ptr(payload)))
        return {"ran": ran.astype(bool), "stats": stats, "payload": payload}

    def run(self, samples, max_events=None):
        """H rounds of feed(1) + process() -> list of (capture, hop, stats, payload bytes) for the decoded frames, in order of hop, then capture"""
        ptr, fmt, H, _keep = self._samples(samples)
        m = self.S * H if max_events is None else max_events
        ev, pl = _event_buffers(m, self.payload_stride)
        n = C.c_int()
        self.rx._ck(self.lib.mgpu_capture_run(self.h, ptr, fmt, H, _ptr(ev), _ptr(pl), m, C.byref(n)))
        return _event_list(ev, pl, n.value, m, self.rx.payload_bytes)

    def run_wideband(self, chan, iq, max_events=None):
        """run() on wideband IQ through the Channelizer `chan` (mgpu_capture_run_wideband): H * P * D complex samples -> the decoded
        frames as run() lists them"""
        ptr, fmt, n_in, _keep = _iq(iq)
        if n_in == 0 or n_in % (self.P * chan.D):
            raise MgpuError("IQ samples must be H * P * D with P = %d, D = %d" % (self.P, chan.D))
        H = n_in // (self.P * chan.D)
        m = self.S * H if max_events is None else max_events
        ev, pl = _event_buffers(max(m, 1), self.payload_stride)
        n = C.c_int()
        self.rx._ck(self.lib.mgpu_capture_run_wideband(self.h, chan.h, ptr, fmt, H, _ptr(ev), _ptr(pl), m, C.byref(n)))
        return _event_list(ev, pl, n.value, m, self.rx.payload_bytes)

    def run_resampled(self, rs, samples, max_events=None):
        """run() on audio at the Resampler `rs`'s input rate (mgpu_capture_run_resampled): [S, n_in] samples, any n_in up to rs.max_in ->
        (the decoded frames as run() lists them, hops numbered from the call's first, and how many hops the call ran)"""
        ptr, fmt, n_in, _keep = _resamp_input(samples, self.S, 1)
        m = self.S * (rs.max_out // self.P + 1) if max_events is None else max_events
        ev, pl = _event_buffers(max(m, 1), self.payload_stride)
        n, hops = C.c_int(), C.c_int()
        self.rx._ck(self.lib.mgpu_capture_run_resampled(self.h, rs.h, ptr, fmt, n_in, _ptr(ev), _ptr(pl), m, C.byref(n), C.byref(hops)))
        return _event_list(ev, pl, n.value, m, self.rx.payload_bytes), hops.value

    def state(self, s):
        st = np.zeros((), CAPTURE_STATE_DTYPE)
        self.rx._ck(self.lib.mgpu_capture_get_state(self.h, s, _ptr(st)))
        return st

    def set_state(self, s, st):
        st = np.ascontiguousarray(st, CAPTURE_STATE_DTYPE)
        self.rx._ck(self.lib.mgpu_capture_set_state(self.h, s, _ptr(st)))

    def window(self, s):
        out = np.zeros(self.window_samples)
        self.rx._ck(self.lib.mgpu_capture_window(self.h, s, _ptr(out)))
        return out


# ---- streaming HF channel (include/mercury_channel.h) ----------------------------------------------------------------
def host_hf_stream_noise(seed, signal, position, n):
    """g(seed, signal, position + i), i < n: the streaming channel's unit noise (host-only twin, no GPU)."""
    out = np.zeros(n)
    lib = load_library()
    _twin(lib.mgpu_host_hf_stream_noise, seed, signal, position, n, _ptr(out))
    return out


class HfStream(_Handle):
    """The Watterson channel on S real signals that are fed in chunks (mgpu_hf_stream_*): apply() takes float64 [S, n] (numpy, or a torch
    tensor on the context's device, then `out` must be one too), n a multiple of 64, and returns the next n output samples of every
    signal, delayed by `latency` samples."""
    _destroy = "mgpu_hf_stream_destroy"

    def __init__(self, rx, S, ch, seed, realisation0=0, fs=48000.0):
        self.rx, self.lib, self.S = rx, rx.lib, S
        self.h = C.c_void_p()
        lib = self.lib
        rx._ck(lib.mgpu_hf_stream_create(rx.h, C.byref(_hf(ch)), fs, S, seed, realisation0, C.byref(self.h)))
        self.latency = int(lib.mgpu_hf_stream_latency(self.h))

    def seek(self, position):
        self.rx._ck(self.lib.mgpu_hf_stream_seek(self.h, position))

    def apply(self, x, noise_amp=None, out=None, stream=None):
        na = None if noise_amp is None else np.ascontiguousarray(noise_amp, np.float64).reshape(self.S)
        if hasattr(x, "data_ptr"):                         # device tensors, asynchronous on `stream` (None: the context's stream)
            import torch
            if x.dtype != torch.float64 or not x.is_contiguous() or x.numel() % self.S:
                raise MgpuError("device samples: a contiguous float64 tensor [S, n]")
            out = torch.empty_like(x) if out is None else out
            self.rx._ck(self.lib.mgpu_hf_stream_apply_dev(self.h, x.data_ptr(), x.numel() // self.S, _ptr(na), out.data_ptr(), stream))
            return out
        a = np.ascontiguousarray(x, np.float64).reshape(self.S, -1)
        out = np.empty_like(a) if out is None else out
        self.rx._ck(self.lib.mgpu_hf_stream_apply(self.h, _ptr(a), a.shape[1], _ptr(na), _ptr(out)))
        return out


# ---- link simulator (include/mercury_linksim.h) --------------------------------------------------------------------------------------
LINKSIM_SYMBOLS = names("mercury_linksim.h")
LINKSIM_COUNTERS_DTYPE = np.dtype([("hops", "<i8"), ("frames_sent", "<i8"), ("delivered", "<i8"), ("duplicates", "<i8"), ("false_decodes", "<i8"),
                                   ("iterations_sum", "<i8"), ("snr_db_sum", "<f8")], align=True)


class LinkSimConfig(C.Structure):       # mgpu_linksim_config
    _fields_ = [("struct_size", C.c_int), ("S", C.c_int), ("gap_hops", C.c_int), ("max_hops", C.c_int), ("seed", C.c_uint64),
                ("channel", HfChannel), ("rx", ReceiveConfig), ("tx", TransmitConfig)]


def linksim_config(S, carrier_hz, seed, channel="awgn", gap_hops=0, max_hops=0, output_power_watt=0.1, trials_max=2, use_last_good_time_sync=1,
                   use_last_good_freq_offset=1, coarse_freq_sync=0, message_location=SINGLE_MESSAGE, start_sample=0):
    """An mgpu_linksim_config with the reference's transmit and receive defaults around the given carrier."""
    k = LinkSimConfig()
    k.struct_size, k.S, k.gap_hops, k.max_hops, k.seed = C.sizeof(LinkSimConfig), S, gap_hops, max_hops, seed
    k.channel = _hf(channel)
    k.rx = ReceiveConfig(carrier_hz, trials_max, use_last_good_time_sync, use_last_good_freq_offset, coarse_freq_sync)
    k.tx = TransmitConfig(carrier_hz, float(np.sqrt(2.0)), output_power_watt, 7.0, 10.0, start_sample, message_location, 0)
    return k


def host_linksim_frame_start(config, frame_samples, symbol_period, link, frame):
    """transmit position of frame `frame` of link `link` (host only)"""
    out = C.c_longlong()
    lib = load_library()
    _twin(lib.mgpu_host_linksim_frame_start, C.byref(config), frame_samples, symbol_period, link, frame, C.byref(out))
    return out.value


def host_linksim_payload(seed, link, frame, nbytes):
    """the payload link `link` sends in its frame `frame`: uint8 [nbytes] (host only)"""
    out = np.zeros(nbytes, np.uint8)
    lib = load_library()
    _twin(lib.mgpu_host_linksim_payload, seed, link, frame, nbytes, _ptr(out))
    return out


class _BorrowedCapture(RxCapture):
    """the capture inside a LinkSim: state() and window() of RxCapture on a handle the simulator owns"""

    def __init__(self, rx, handle, S):
        self.rx, self.lib, self.S, self.h = rx, rx.lib, S, handle
        self._read_geometry()

    def close(self):
        self.h = C.c_void_p()


class LinkSim(_Handle):
    """S simplex links (transmitter -> streaming HF channel -> noise -> the capture receive loop) on one RxPhy context
    (include/mercury_linksim.h). config: linksim_config(...); esn0_db: None (no noise), a number or [S]."""

    def __init__(self, rx, config, esn0_db=None, ladder=None):
        """ladder: rungs as RxPhy.set_estimator_ladder takes them, set on the context `rx` (RxPhy.set_estimator_ladder) before the simulator is made; None: as it is"""
        self.rx, self.lib, self.S, self.config = rx, rx.lib, config.S, config
        if ladder is not None:
            rx.set_estimator_ladder(ladder)
        self.h = C.c_void_p()
        lib = self.lib
        es = None if esn0_db is None else np.ascontiguousarray(np.broadcast_to(np.asarray(esn0_db, np.float64), (self.S,)))
        self.esn0_db = es
        rx._ck(lib.mgpu_linksim_create(rx.h, C.byref(config), _ptr(es), C.byref(self.h)))
        cap = C.c_void_p()
        rx._ck(lib.mgpu_linksim_capture(self.h, C.byref(cap)))
        self.capture = _BorrowedCapture(rx, cap, self.S)
        self.P = self.capture.P
        self.frame_samples = rx.transmit_frame_samples()
        self.slot = self.frame_samples + config.gap_hops * self.P
        self.payload_stride = rx.payload_stride

    def _release(self):
        self.capture.close()
        self.lib.mgpu_linksim_destroy(self.h)

    def run(self, H, want_samples=False, max_events=None):
        """H more hops for every link -> list of (link, hop since the start, stats, payload bytes) for the decoded frames; with
        want_samples also the audio the captures were fed, float64 [S, H * P]"""
        m = self.S * H if max_events is None else max_events
        ev, pl = _event_buffers(max(m, 1), self.payload_stride)
        n = C.c_int()
        audio = np.zeros((self.S, H * self.P)) if want_samples else None
        self.rx._ck(self.lib.mgpu_linksim_run(self.h, H, _ptr(ev), _ptr(pl), m, C.byref(n), _ptr(audio)))
        events = _event_list(ev, pl, n.value, m, self.rx.payload_bytes)
        return (events, audio) if want_samples else events

    def counters(self):
        out = np.zeros(self.S, LINKSIM_COUNTERS_DTYPE)
        self.rx._ck(self.lib.mgpu_linksim_counters_get(self.h, _ptr(out)))
        return out

    def noise_amp(self):
        """the streaming channel's noise amplitude per link (zeros without noise)"""
        out = np.zeros(self.S)
        self.rx._ck(self.lib.mgpu_linksim_noise_amp(self.h, _ptr(out)))
        return out

    def frame_start(self, link, frame):
        return host_linksim_frame_start(self.config, self.frame_samples, self.P, link, frame)

    def payload(self, link, frame):
        return host_linksim_payload(self.config.seed, link, frame, self.rx.payload_bytes)


# ---- wideband channeliser (include/mercury_channelizer.h) ---------------------------------------------------------------
CHANNELIZER_SYMBOLS = names("mercury_channelizer.h")
IQ_CS16, IQ_CF32, IQ_CF64 = 0, 1, 2
CHAN_DEFAULT_TP, CHAN_PHASOR_LEN = 320, 48000


class ChanChannel(C.Structure):         # mgpu_chan_channel
    _fields_ = [("offset_hz", C.c_int), ("sideband", C.c_int), ("gain", C.c_double)]


class ChanConfig(C.Structure):          # mgpu_chan_config
    _fields_ = [("struct_size", C.c_int), ("D", C.c_int), ("S", C.c_int), ("audio_centre_hz", C.c_int), ("ntaps", C.c_int),
                ("taps", C.c_void_p), ("max_out", C.c_int)]


def chan_channels(channels):
    """[(offset_hz, sideband, gain), ...] (sideband 0 / "usb" or 1 / "lsb"; gain optional, 1.0) -> an array of mgpu_chan_channel"""
    rows = []
    for ch in channels:
        ch = tuple(ch) if isinstance(ch, (tuple, list)) else (ch,)
        off = ch[0]
        sb = ch[1] if len(ch) > 1 else 0
        sb = {"usb": 0, "lsb": 1}.get(sb.lower(), -1) if isinstance(sb, str) else int(sb)
        rows.append(ChanChannel(int(off), sb, float(ch[2]) if len(ch) > 2 else 1.0))
    return (ChanChannel * len(rows))(*rows)


def _taps_arg(taps):
    """a prototype given as taps -> (float64 array or None: the keep-alive, its count, its address as a configuration's `taps` takes it)"""
    h = None if taps is None else np.ascontiguousarray(taps, np.float64).ravel()
    return h, 0 if h is None else h.size, None if h is None else h.ctypes.data


def chan_config(D, S, taps=None, audio_centre_hz=1472, max_out=0):
    """-> (mgpu_chan_config, keep-alive of its taps)"""
    h, ntaps, address = _taps_arg(taps)
    return ChanConfig(C.sizeof(ChanConfig), int(D), int(S), int(audio_centre_hz), ntaps, address, int(max_out)), h


def _plan_tables(D, keep, want_phasor):
    """what a channel plan's table twins write: T, the prototype's length (keep: a configuration's own taps, or None: the default
    design), and the phasor table's array (None: not wanted)"""
    T = keep.size if keep is not None else CHAN_DEFAULT_TP * max(int(D), 0) + 1
    return T, np.zeros(CHAN_PHASOR_LEN, np.complex128) if want_phasor else None


def _iq(iq):
    """-> (pointer, MGPU_IQ_* format, complex samples, keep-alive): complex64, complex128, or int16 with a last axis of 2;
    a numpy array or a torch tensor (read in place)"""
    if hasattr(iq, "data_ptr"):
        import torch
        fmt = {torch.complex64: IQ_CF32, torch.complex128: IQ_CF64, torch.int16: IQ_CS16}.get(iq.dtype)
        if fmt is None or not iq.is_contiguous() or (fmt == IQ_CS16 and (iq.dim() < 1 or iq.shape[-1] != 2)):
            raise MgpuError("device IQ: a contiguous complex64 / complex128 tensor, or int16 with a last axis of 2")
        n = iq.numel() // (2 if fmt == IQ_CS16 else 1)
        return iq.data_ptr(), fmt, n, iq
    x = np.ascontiguousarray(iq)
    fmt = {np.dtype(np.complex64): IQ_CF32, np.dtype(np.complex128): IQ_CF64, np.dtype(np.int16): IQ_CS16}.get(x.dtype)
    if fmt is None or (fmt == IQ_CS16 and (x.ndim < 1 or x.shape[-1] != 2)):
        raise MgpuError("IQ samples are complex64, complex128, or int16 with a last axis of 2, not %s %s" % (x.dtype, x.shape))
    return _ptr(x), fmt, x.size // (2 if fmt == IQ_CS16 else 1), x


def host_chan_design(D, tp=None, cutoff_hz=1500.0, atten_db=60.0):
    """the prototype low-pass (mgpu_host_chan_design; tp None: the default design's 320): float64 [tp * D + 1]"""
    tp = CHAN_DEFAULT_TP if tp is None else int(tp)
    taps = np.zeros(max(tp, 0) * max(int(D), 0) + 1)
    n = C.c_int()
    _twin(load_library().mgpu_host_chan_design, int(D), tp, cutoff_hz, atten_db, _ptr(taps), C.byref(n), code=1)
    return taps[: n.value]


def host_chan_tables(D, channel, taps=None, audio_centre_hz=1472, want_phasor=False):
    """one channel's tap row g, complex128 [T] (and the phasor table W, complex128 [48000]) as the device reads them"""
    k, keep = chan_config(D, 1, taps, audio_centre_hz)
    T, W = _plan_tables(D, keep, want_phasor)
    g = np.zeros(T, np.complex128)
    _twin(load_library().mgpu_host_chan_tables, C.byref(k), chan_channels([channel]), _ptr(g), _ptr(W), code=1)
    return (g, W) if want_phasor else g


def host_chan_process(D, channels, iq, position=0, taps=None, audio_centre_hz=1472, struct_size=None):
    """the twin (mgpu_host_chan_process): a fresh channeliser seeked to `position` and fed `iq` whole -> float64 [S, n_in // D]"""
    chs = chan_channels(channels)
    k, _keep = chan_config(D, len(chs), taps, audio_centre_hz)
    if struct_size is not None:
        k.struct_size = struct_size
    ptr, fmt, n_in, _x = _iq(iq)
    out = np.zeros((len(chs), max(n_in // max(int(D), 1), 1)))
    _twin(load_library().mgpu_host_chan_process, C.byref(k), chs, ptr, fmt, n_in, int(position), _ptr(out), code=1)
    return out


class Channelizer(_Handle):
    """One wideband IQ stream at 48000 * D into S 48 kHz sideband audio streams on an RxPhy context (include/mercury_channelizer.h).
    channels: [(offset_hz, sideband, gain), ...] as chan_channels takes them. process() takes complex64 / complex128 / int16 [..., 2]
    samples (numpy, or a torch tensor on the context's device), a multiple of D of them, and returns float64 [S, n_in // D]."""
    _destroy = "mgpu_chan_destroy"

    def __init__(self, rx, D, channels, taps=None, audio_centre_hz=1472, max_out=0):
        self.rx, self.lib, self.D = rx, rx.lib, int(D)
        self._chs = chan_channels(channels)
        self.S = len(self._chs)
        self.config, self._taps = chan_config(D, self.S, taps, audio_centre_hz, max_out)
        self.h = C.c_void_p()
        rx._ck(self.lib.mgpu_chan_create(rx.h, C.byref(self.config), self._chs, C.byref(self.h)))
        self.latency = int(self.lib.mgpu_chan_latency(self.h))

    def seek(self, position):
        self.rx._ck(self.lib.mgpu_chan_seek(self.h, int(position)))

    def retune(self, s, channel):
        self.rx._ck(self.lib.mgpu_chan_retune(self.h, int(s), chan_channels([channel])))

    def process(self, iq, out=None, stream=None):
        """out None: a new numpy array (blocking call). out a float64 torch tensor [S, n_in // D] on the device, with `iq` one too:
        mgpu_chan_process_dev, asynchronous on `stream` (None: the context's stream)."""
        ptr, fmt, n_in, _keep = _iq(iq)
        if out is not None and hasattr(out, "data_ptr"):
            import torch
            if not hasattr(iq, "data_ptr") or out.dtype != torch.float64 or not out.is_contiguous() or out.numel() * self.D != self.S * n_in:
                raise MgpuError("device output: device input and a contiguous float64 tensor [S, n_in // D]")
            self.rx._ck(self.lib.mgpu_chan_process_dev(self.h, ptr, fmt, n_in, out.data_ptr(), stream))
            return out
        if out is None:
            out = np.zeros((self.S, max(n_in // self.D, 1)))
        if out.dtype != np.float64 or not out.flags.c_contiguous or out.size < self.S * (n_in // self.D):      # a bad n_in: the library refuses it
            raise MgpuError("out: a contiguous float64 array [S, n_in // D]")
        self.rx._ck(self.lib.mgpu_chan_process(self.h, ptr, fmt, n_in, _ptr(out)))
        return out


# ---- rational resampler (include/ext/mercury_resampler.h) ----------------------------------------------------------------
RESAMPLER_SYMBOLS = names("ext/mercury_resampler.h")


class ResampConfig(C.Structure):        # mgpu_resamp_config
    _fields_ = [("struct_size", C.c_int), ("fin", C.c_int), ("fout", C.c_int), ("S", C.c_int), ("components", C.c_int), ("tp", C.c_int),
                ("ntaps", C.c_int), ("taps", C.c_void_p), ("max_in", C.c_int)]


class ResampStatus(C.Structure):        # mgpu_resamp_status
    _fields_ = [("L", C.c_int), ("M", C.c_int), ("tp", C.c_int), ("S", C.c_int), ("components", C.c_int), ("max_in", C.c_int),
                ("max_out", C.c_int), ("tile", C.c_int), ("fifo", C.c_int), ("pad", C.c_int), ("delay", C.c_double), ("m0", C.c_uint64),
                ("n0", C.c_uint64)]


def resamp_ratio(fin, fout):
    """(L, M) = (fout / g, fin / g), g = gcd(fin, fout)"""
    g = math.gcd(int(fin), int(fout))
    return int(fout) // g, int(fin) // g


def resamp_config(fin, fout=48000, S=1, components=1, tp=None, taps=None, max_in=None):
    """-> (mgpu_resamp_config, keep-alive of its taps). With taps and no tp, tp is (len(taps) - 1) / L."""
    h, ntaps, address = _taps_arg(taps)
    if h is not None and tp is None and fin > 0 and fout > 0:
        tp = (h.size - 1) // resamp_ratio(fin, fout)[0]
    return ResampConfig(C.sizeof(ResampConfig), int(fin), int(fout), int(S), int(components), int(tp or 0), ntaps, address, int(max_in or 0)), h


def _resamp_input(x, S, components):
    """-> (pointer, format, samples per stream, keep-alive): [S, n_in] real samples in a capture format (components 1) or IQ as
    Channelizer.process takes it (components 2); a numpy array or a torch tensor (read in place)"""
    ptr, fmt, n, keep = _iq(x) if components == 2 else _real_samples(x)
    if n % S:
        raise MgpuError("samples must be [S, n_in] with S = %d" % S)
    return ptr, fmt, n // S, keep


def host_resamp_design(fin, fout=48000, tp=None, cutoff_hz=None, atten_db=None):
    """the prototype low-pass (mgpu_host_resamp_design; None: the default of each parameter): float64 [tp * L + 1]"""
    lib = load_library()
    n = C.c_int()
    args = (int(fin), int(fout), int(tp or 0), float(cutoff_hz or 0.0), float(atten_db or 0.0))
    _twin(lib.mgpu_host_resamp_design, *args, None, C.byref(n), code=1)
    taps = np.zeros(n.value)
    _twin(lib.mgpu_host_resamp_design, *args, _ptr(taps), C.byref(n), code=1)
    return taps


def host_resamp_count(fin, fout, m0, n_in):
    """outputs of a call of n_in inputs at input position m0 (mgpu_host_resamp_count)"""
    n = C.c_int()
    _twin(load_library().mgpu_host_resamp_count, int(fin), int(fout), int(m0), int(n_in), C.byref(n), code=1)
    return n.value


def _resamp_result(out, n, components):
    out = out[:, : n * components]
    return out if components == 1 else np.ascontiguousarray(out).view(np.complex128)


def host_resamp_process(fin, fout, x, position=0, components=1, tp=None, taps=None, S=None, struct_size=None, fmt=None):
    """the twin (mgpu_host_resamp_process): a fresh resampler seeked to input position `position` and fed x ([S, n_in], or [n_in] for
    one stream) whole -> float64 [S, n_out] (components 1) or complex128 [S, n_out] (components 2)"""
    if S is None:
        a = x if hasattr(x, "shape") else np.asarray(x)
        lead = a.ndim - (1 if components == 2 and a.dtype == np.int16 else 0)
        S = a.shape[0] if lead >= 2 else 1
    k, _keep = resamp_config(fin, fout, S, components, tp, taps)
    if struct_size is not None:
        k.struct_size = struct_size
    ptr, f, n_in, _x = _resamp_input(x, S, 2 if components == 2 else 1)
    try:
        cap = host_resamp_count(fin, fout, position, n_in)
    except MgpuError:
        cap = 0
    out = np.zeros((S, max(cap, 1) * max(int(components), 1)))
    n = C.c_int()
    _twin(load_library().mgpu_host_resamp_process, C.byref(k), ptr, f if fmt is None else fmt, n_in, int(position), _ptr(out), max(cap, 1),
          C.byref(n), code=1)
    return _resamp_result(out, n.value, components)


class Resampler(_Handle):
    """S streams at fin into S streams at fout on an RxPhy context (include/ext/mercury_resampler.h). process() takes [S, n_in] samples,
    real in a capture format (components 1) or IQ as Channelizer.process takes it (components 2), numpy or a torch tensor on the
    context's device, cut anywhere, and returns float64 / complex128 [S, n_out]."""
    _destroy = "mgpu_resamp_destroy"

    def __init__(self, rx, fin, fout=48000, S=1, components=1, tp=None, taps=None, max_in=None):
        self.rx, self.lib, self.fin, self.fout, self.S, self.components = rx, rx.lib, int(fin), int(fout), int(S), int(components)
        self.config, self._taps = resamp_config(fin, fout, S, components, tp, taps, max_in)
        self.h = C.c_void_p()
        rx._ck(self.lib.mgpu_resamp_create(rx.h, C.byref(self.config), C.byref(self.h)))
        st = self.info()
        self.L, self.M, self.tp, self.max_in, self.max_out, self.tile, self.delay = st.L, st.M, st.tp, st.max_in, st.max_out, st.tile, st.delay

    def info(self):
        st = ResampStatus()
        self.rx._ck(self.lib.mgpu_resamp_info(self.h, C.byref(st)))
        return st

    def seek(self, position):
        self.rx._ck(self.lib.mgpu_resamp_seek(self.h, int(position)))

    def process(self, x, out=None, stream=None, fmt=None):
        """out None: a new numpy array [S, n_out] (blocking call). out a float64 torch tensor [S, stride * components] on the device, with
        x one too: mgpu_resamp_process_dev, asynchronous on `stream` (None: the context's stream); returns n_out."""
        ptr, f, n_in, _keep = _resamp_input(x, self.S, self.components)
        f = f if fmt is None else fmt
        n = C.c_int()
        if out is not None and hasattr(out, "data_ptr"):
            import torch
            if not hasattr(x, "data_ptr") or out.dtype != torch.float64 or not out.is_contiguous() or out.numel() % (self.S * self.components):
                raise MgpuError("device output: device input and a contiguous float64 tensor [S, stride * components]")
            stride = out.numel() // (self.S * self.components)
            self.rx._ck(self.lib.mgpu_resamp_process_dev(self.h, ptr, f, n_in, out.data_ptr(), stride, C.byref(n), stream))
            return n.value
        stride = max(self.max_out, 1)
        host = np.zeros((self.S, stride * self.components))
        self.rx._ck(self.lib.mgpu_resamp_process(self.h, ptr, f, n_in, _ptr(host), stride, C.byref(n)))
        return _resamp_result(host, n.value, self.components)


# ---- wideband synthesiser (include/ext/mercury_synth.h) -----------------------------------------------------------------
SYNTH_SYMBOLS = names("ext/mercury_synth.h")
_IQ_FORMATS = {"cs16": IQ_CS16, "cf32": IQ_CF32, "cf64": IQ_CF64}


class SynthConfig(C.Structure):         # mgpu_synth_config
    _fields_ = [("struct_size", C.c_int), ("D", C.c_int), ("S", C.c_int), ("audio_centre_hz", C.c_int), ("ntaps", C.c_int),
                ("taps", C.c_void_p), ("max_in", C.c_int)]


class SynthState(C.Structure):          # mgpu_synth_state
    _fields_ = [("position", C.c_uint64), ("clamped", C.c_uint64), ("D", C.c_int), ("S", C.c_int), ("tp", C.c_int), ("max_in", C.c_int),
                ("tile", C.c_int), ("phases", C.c_int)]


def synth_config(D, S, taps=None, audio_centre_hz=1472, max_in=0):
    """-> (mgpu_synth_config, keep-alive of its taps)"""
    h, ntaps, address = _taps_arg(taps)
    return SynthConfig(C.sizeof(SynthConfig), int(D), int(S), int(audio_centre_hz), ntaps, address, int(max_in)), h


def _iq_format(fmt):
    f = _IQ_FORMATS.get(fmt.lower()) if isinstance(fmt, str) else fmt
    if f not in (IQ_CS16, IQ_CF32, IQ_CF64):
        raise MgpuError("IQ format: 'cs16', 'cf32' or 'cf64', not %r" % (fmt,))
    return f


def _iq_empty(fmt, n):
    """a numpy array for n IQ samples of MGPU_IQ_* fmt: int16 [n, 2], complex64 [n] or complex128 [n]"""
    return np.zeros((n, 2), np.int16) if fmt == IQ_CS16 else np.zeros(n, np.complex64 if fmt == IQ_CF32 else np.complex128)


def _iq_format_number(fmt):
    """'cs16', 'cf32', 'cf64' or an MGPU_IQ_* number as a configuration takes it (an unknown name is -1 and an unknown number stays: both are
    the library's to refuse)"""
    return _IQ_FORMATS.get(fmt.lower(), -1) if isinstance(fmt, str) else int(fmt)


def _iq_like(x, fmt, n):
    """a numpy array for n IQ samples of MGPU_IQ_* fmt, shaped as the numpy input x where that holds n samples"""
    out = _iq_empty(fmt, max(n, 1))
    return out.reshape(x.shape) if isinstance(x, np.ndarray) and x.size == out.size and n else out


def _device_tensor(t, dtype, numel, exact=False):
    """t is a contiguous torch tensor of `dtype` with at least (exact: just) `numel` elements"""
    return hasattr(t, "data_ptr") and t.dtype == dtype and t.is_contiguous() and (t.numel() == numel if exact else t.numel() >= numel)


def _host_block_process(stage, make_config, block_of, report_dtype, iq, D, position, struct_size, fmt, config, state=None):
    """the twin mgpu_host_<stage>_process of a block stage: a fresh stage (make_config(D, the input's format, **config), whose block is
    block_of(it)) seeked to `position` and fed `iq` whole -> (out, as the input; reports [n_in / B]). state: a float64 array [6] that
    the twin's _continue form reads and leaves"""
    ptr, f, n_in, x = _iq(iq)
    k = make_config(D, f if fmt is None else fmt, **config)
    if struct_size is not None:
        k.struct_size = struct_size
    out = _iq_like(x, f, n_in)
    reports = np.zeros(max(n_in // block_of(k), 1), report_dtype)
    n = C.c_int()
    ahead = ()
    if state is not None:
        if not (isinstance(state, np.ndarray) and state.dtype == np.float64 and state.size == 6 and state.flags.c_contiguous):
            raise MgpuError("state: a contiguous float64 array of 6", 1)
        ahead = (_ptr(state),)
    twin = getattr(load_library(), "mgpu_host_%s_%s" % (stage, "process" if state is None else "continue"))
    _twin(twin, C.byref(k), *ahead, ptr, n_in, int(position), _ptr(out), _ptr(reports), C.byref(n), code=1)
    return out, reports[: n.value]


class _BlockStage(_Handle):
    """What WidebandBlanker and IqCorrector are alike in: a stage mgpu_<_prefix> that takes blocks of B IQ samples of one format and gives as
    many samples back, with one report (_REPORT_DTYPE, decoded by _decode) per block. _make_config: the configuration maker, _State: the
    status struct, _noun: what the stage is called where a call's format is not the stage's."""
    _prefix = _make_config = _State = _REPORT_DTYPE = _decode = _noun = None

    def _fn(self, name):
        return getattr(self.lib, "mgpu_%s_%s" % (self._prefix, name))

    def _create(self, rx, D, fmt, config):
        """the handle; -> its status"""
        self.rx, self.lib, self.D = rx, rx.lib, int(D)
        self.config = type(self)._make_config(D, fmt, **config)
        self.h = C.c_void_p()
        rx._ck(self._fn("create")(rx.h, C.byref(self.config), C.byref(self.h)))
        st = self.status()
        self.format, self.B, self.max_in = st.format, st.block, st.max_in
        return st

    def status(self):
        """the stage's state struct (the class names its fields)"""
        st = self._State()
        self.rx._ck(self._fn("status")(self.h, C.byref(st)))
        return st

    def seek(self, position):
        self.rx._ck(self._fn("seek")(self.h, int(position)))

    def process_raw(self, iq, out=None, reports=None, stream=None):
        """-> (out, as the input; reports _REPORT_DTYPE [n_in / B]) as numpy arrays (a blocking call). With out a torch tensor of the
        input's dtype and size on the device, and `iq` one too: mgpu_<stage>_process_dev, asynchronous on `stream` (None: the context's
        stream), the reports into `reports`, a uint8 torch tensor [>= n_in / B, the report's bytes] on the device or None; returns
        n_in / B."""
        ptr, fmt, n_in, x = _iq(iq)
        if fmt != self.format:
            raise MgpuError("the %s was made for IQ format %d, not %d" % (self._noun, self.format, fmt))
        n = C.c_int()
        row = self._REPORT_DTYPE.itemsize
        if out is not None and hasattr(out, "data_ptr"):
            import torch
            if not (hasattr(iq, "data_ptr") and _device_tensor(out, iq.dtype, iq.numel(), exact=True)
                    and (reports is None or _device_tensor(reports, torch.uint8, n_in // self.B * row))):
                raise MgpuError("device output: device input, a contiguous tensor like it and a contiguous uint8 tensor [n_in / B, %d] or None" % row)
            self.rx._ck(self._fn("process_dev")(self.h, ptr, n_in, out.data_ptr(), reports.data_ptr() if reports is not None else None,
                                                C.byref(n), stream))
            return n.value
        host = _iq_like(x, fmt, n_in)
        rep = np.zeros(max(n_in // self.B, 1), self._REPORT_DTYPE)
        self.rx._ck(self._fn("process")(self.h, ptr, n_in, _ptr(host), _ptr(rep), C.byref(n)))
        return host, rep[: n.value]

    def process(self, iq):
        """-> (out, [one dict per block of the call, as the stage's *_reports function makes them])"""
        out, reports = self.process_raw(iq)
        return out, type(self)._decode(reports)


def _synth_audio(audio, S):
    """-> (pointer, row stride in samples, samples per channel, keep-alive): float64 audio [S, n_in] (or [n_in] for one channel), a numpy
    array or a torch tensor (read in place; its rows may be further apart than n_in)"""
    if hasattr(audio, "data_ptr"):
        import torch
        a = audio.reshape(1, -1) if audio.dim() == 1 else audio
        if a.dtype != torch.float64 or a.dim() != 2 or a.shape[0] != S or a.stride(1) != 1 or (S > 1 and a.stride(0) < a.shape[1]):
            raise MgpuError("device audio: a float64 tensor [S, n_in] with contiguous rows, S = %d" % S)
        return a.data_ptr(), (a.stride(0) if S > 1 else a.shape[1]), a.shape[1], a
    a = np.ascontiguousarray(audio, np.float64)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    if a.ndim != 2 or a.shape[0] != S:
        raise MgpuError("audio must be [S, n_in] with S = %d" % S)
    return _ptr(a), a.shape[1], a.shape[1], a


def host_synth_tables(D, channel, taps=None, audio_centre_hz=1472, want_phasor=False):
    """one channel's tables as the device reads them: (q complex128 [T], the tap table of its sideband; P complex128 [D]; G) and, with
    want_phasor, W complex128 [48000]"""
    k, keep = synth_config(D, 1, taps, audio_centre_hz)
    T, W = _plan_tables(D, keep, want_phasor)
    q, P, G = np.zeros(T, np.complex128), np.zeros(max(int(D), 1), np.complex128), C.c_double()
    _twin(load_library().mgpu_host_synth_tables, C.byref(k), chan_channels([channel]), _ptr(q), _ptr(P), C.byref(G), _ptr(W), code=1)
    return (q, P, G.value, W) if want_phasor else (q, P, G.value)


def host_synth_process(D, channels, audio, position=0, fmt="cf64", taps=None, audio_centre_hz=1472, struct_size=None, want_clamped=False):
    """the twin (mgpu_host_synth_process): a fresh synthesiser seeked to `position` and fed audio [S, n_in] whole -> n_in * D IQ samples
    (complex128, complex64 or int16 [.., 2]); with want_clamped also the CS16 components clamped"""
    chs = chan_channels(channels)
    k, _keep = synth_config(D, len(chs), taps, audio_centre_hz)
    if struct_size is not None:
        k.struct_size = struct_size
    f = _iq_format(fmt)
    ptr, stride, n_in, _a = _synth_audio(audio, len(chs))
    out = _iq_empty(f, max(n_in * max(int(D), 1), 1))
    clamped = C.c_uint64()
    _twin(load_library().mgpu_host_synth_process, C.byref(k), chs, ptr, stride, n_in, int(position), f, _ptr(out), C.byref(clamped), code=1)
    return (out, clamped.value) if want_clamped else out


class Synthesizer(_Handle):
    """S 48 kHz transmit audio streams into one wideband IQ stream at 48000 * D on an RxPhy context (include/ext/mercury_synth.h), the
    mirror of Channelizer. channels: [(offset_hz, sideband, gain), ...] as chan_channels takes them. process() takes float64 audio
    [S, n_in] (numpy, or a torch tensor on the context's device such as the one transmit_byte_dev leaves there) and returns n_in * D IQ
    samples."""
    _destroy = "mgpu_synth_destroy"

    def __init__(self, rx, D, channels, taps=None, audio_centre_hz=1472, max_in=0):
        self.rx, self.lib, self.D = rx, rx.lib, int(D)
        self._chs = chan_channels(channels)
        self.S = len(self._chs)
        self.config, self._taps = synth_config(D, self.S, taps, audio_centre_hz, max_in)
        self.h = C.c_void_p()
        rx._ck(self.lib.mgpu_synth_create(rx.h, C.byref(self.config), self._chs, C.byref(self.h)))
        self.latency = int(self.lib.mgpu_synth_latency(self.h))
        st = self.status()
        self.tp, self.max_in, self.tile, self.phases = st.tp, st.max_in, st.tile, st.phases

    def status(self):
        """mgpu_synth_state: position, clamped (CS16 components since the last seek), D, S, tp, max_in, tile, phases. Waits for the device."""
        st = SynthState()
        self.rx._ck(self.lib.mgpu_synth_status(self.h, C.byref(st)))
        return st

    def seek(self, position):
        self.rx._ck(self.lib.mgpu_synth_seek(self.h, int(position)))

    def retune(self, s, channel):
        self.rx._ck(self.lib.mgpu_synth_retune(self.h, int(s), chan_channels([channel])))

    def process(self, audio, fmt="cf64", out=None, stream=None):
        """out None: a new numpy array of n_in * D IQ samples in fmt ('cf64' complex128, 'cf32' complex64, 'cs16' int16 [.., 2]); a
        blocking call. out a torch tensor on the device (complex128 / complex64 [n_in * D] or int16 [n_in * D, 2], matching fmt), with
        `audio` one too: mgpu_synth_process_dev, asynchronous on `stream` (None: the context's stream)."""
        f = _iq_format(fmt)
        ptr, stride, n_in, _keep = _synth_audio(audio, self.S)
        if out is not None and hasattr(out, "data_ptr"):
            optr, ofmt, n_out, _o = _iq(out)
            if not hasattr(audio, "data_ptr") or ofmt != f or n_out != n_in * self.D:
                raise MgpuError("device output: device input and a contiguous tensor of n_in * D IQ samples in the format asked for")
            self.rx._ck(self.lib.mgpu_synth_process_dev(self.h, ptr, stride, n_in, f, optr, stream))
            return out
        if out is None:
            out = _iq_empty(f, max(n_in * self.D, 1))
        optr, ofmt, n_out, _o = _iq(out)
        if ofmt != f or n_out < n_in * self.D or not out.flags.c_contiguous:
            raise MgpuError("out: a contiguous array of n_in * D IQ samples in the format asked for")
        self.rx._ck(self.lib.mgpu_synth_process(self.h, ptr, stride, n_in, f, optr))
        return out


# ---- band scanner (include/ext/mercury_scanner.h) --------------------------------------------------------------------------
SCANNER_SYMBOLS = names("ext/mercury_scanner.h")
SCAN_MAX_RUNS = 32
SCAN_DEFAULT_THRESHOLD = 5.0            # MGPU_SCAN_DEFAULT_THRESHOLD: measured (profiles/scanner.md)
SCAN_RUN_DTYPE = np.dtype([("first", np.int32), ("count", np.int32), ("peak", np.int32), ("pad", np.int32), ("power", np.float64)])
SCAN_REPORT_DTYPE = np.dtype([("first_block", np.uint64), ("level", np.float64), ("n_runs", np.int32), ("reported", np.int32),
                              ("nonfinite", np.int32), ("pad", np.int32), ("runs", SCAN_RUN_DTYPE, (SCAN_MAX_RUNS,))])       # mgpu_scan_report


class ScanConfig(C.Structure):          # mgpu_scan_config
    _fields_ = [("struct_size", C.c_int), ("D", C.c_int), ("log2n", C.c_int), ("blocks_per_line", C.c_int), ("threshold", C.c_double),
                ("edge_bins", C.c_int), ("dc_bins", C.c_int), ("gap", C.c_int), ("min_bins", C.c_int), ("max_runs", C.c_int), ("max_in", C.c_int)]


class ScanState(C.Structure):           # mgpu_scan_state
    _fields_ = [("position", C.c_uint64), ("blocks", C.c_uint64), ("lines", C.c_uint64), ("D", C.c_int), ("log2n", C.c_int),
                ("blocks_per_line", C.c_int), ("max_in", C.c_int)]


def scan_config(D, log2n=12, blocks_per_line=16, threshold=SCAN_DEFAULT_THRESHOLD, edge_bins=None, dc_bins=2, gap=2, min_bins=2,
                max_runs=SCAN_MAX_RUNS, max_in=0):
    """-> mgpu_scan_config; edge_bins None: N / 32"""
    if edge_bins is None:
        edge_bins = (1 << int(log2n)) // 32 if 0 <= int(log2n) < 31 else 0
    return ScanConfig(C.sizeof(ScanConfig), int(D), int(log2n), int(blocks_per_line), float(threshold), int(edge_bins), int(dc_bins), int(gap),
                      int(min_bins), int(max_runs), int(max_in))


def scan_reports(reports):
    """a SCAN_REPORT_DTYPE array -> [{first_block, level, n_runs, reported, nonfinite, runs: [{first, count, peak, power}]}]"""
    return [{"first_block": int(r["first_block"]), "level": float(r["level"]), "n_runs": int(r["n_runs"]), "reported": int(r["reported"]),
             "nonfinite": int(r["nonfinite"]),
             "runs": [{"first": int(q["first"]), "count": int(q["count"]), "peak": int(q["peak"]), "power": float(q["power"])}
                      for q in r["runs"][: int(r["reported"])]]} for r in reports]


def _scan_lines_host(config, position, n_in):
    """the lines a fresh scanner at `position` completes from n_in samples; 1 where the arguments are refused (room for nothing)"""
    H = (1 << config.log2n) // 2 if 8 <= config.log2n <= 12 else 0
    A = config.blocks_per_line
    if H == 0 or A < 1 or n_in < H or n_in % H or position < 0 or position % (H * A):
        return 1
    return (position // H + n_in // H) // A - position // H // A


def host_scan_process(iq, D, position=0, struct_size=None, fmt=None, **config):
    """the twin (mgpu_host_scan_process): a fresh scanner (scan_config(D, **config)) seeked to `position` and fed `iq` whole ->
    (lines float64 [n, N], reports SCAN_REPORT_DTYPE [n])"""
    k = scan_config(D, **config)
    if struct_size is not None:
        k.struct_size = struct_size
    ptr, f, n_in, _x = _iq(iq)
    room = max(_scan_lines_host(k, int(position), n_in), 1)
    lines = np.zeros((room, 1 << min(max(k.log2n, 0), 12)))
    reports = np.zeros(room, SCAN_REPORT_DTYPE)
    n = C.c_int()
    _twin(load_library().mgpu_host_scan_process, C.byref(k), ptr, f if fmt is None else fmt, n_in, int(position), _ptr(lines), _ptr(reports),
          C.byref(n), code=1)
    return lines[: n.value], reports[: n.value]


def host_scan_plan(run, D, log2n=12, sideband=0, audio_centre_hz=1472):
    """one run ({first, count, ..}) as a channel tuple (offset_hz, sideband, 1.0) (mgpu_host_scan_plan)"""
    k = scan_config(D, log2n=log2n)
    r = np.zeros(1, SCAN_RUN_DTYPE)
    r["first"], r["count"] = int(run["first"]), int(run["count"])
    ch = ChanChannel()
    _twin(load_library().mgpu_host_scan_plan, C.byref(k), _ptr(r), int(sideband), int(audio_centre_hz), C.byref(ch), code=1)
    return ch.offset_hz, ch.sideband, ch.gain


class BandScanner(_Handle):
    """One wideband IQ stream at 48000 * D into spectrum lines of N = 2^log2n bins, one per blocks_per_line blocks of N / 2 samples, and per
    line a report of the occupied runs, on an RxPhy context (include/ext/mercury_scanner.h). The other arguments are scan_config's.
    process() takes complex64 / complex128 / int16 [..., 2] samples (numpy, or a torch tensor on the context's device), a multiple of
    N / 2 of them."""
    _destroy = "mgpu_scan_destroy"

    def __init__(self, rx, D, **config):
        self.rx, self.lib, self.D = rx, rx.lib, int(D)
        self.config = scan_config(D, **config)
        self.h = C.c_void_p()
        rx._ck(self.lib.mgpu_scan_create(rx.h, C.byref(self.config), C.byref(self.h)))
        self.log2n, self.N, self.H, self.A = self.config.log2n, 1 << self.config.log2n, (1 << self.config.log2n) // 2, self.config.blocks_per_line
        self.max_in = self.status().max_in

    def status(self):
        """mgpu_scan_state: position, blocks, lines, D, log2n, blocks_per_line, max_in"""
        st = ScanState()
        self.rx._ck(self.lib.mgpu_scan_status(self.h, C.byref(st)))
        return st

    def seek(self, position):
        self.rx._ck(self.lib.mgpu_scan_seek(self.h, int(position)))

    def lines(self, n_in):
        """the lines the next call of n_in samples completes; < 0: that n_in is refused"""
        return int(self.lib.mgpu_scan_lines(self.h, int(n_in)))

    def process_raw(self, iq, lines=None, reports=None, stream=None):
        """-> (lines float64 [n, N], reports SCAN_REPORT_DTYPE [n]) as numpy arrays (a blocking call). With lines a float64 torch tensor
        [>= n, N] and reports a uint8 torch tensor [>= n, 800] on the device, and `iq` one too: mgpu_scan_process_dev, asynchronous on
        `stream` (None: the context's stream); returns n."""
        ptr, fmt, n_in, _keep = _iq(iq)
        room = max(self.lines(n_in), 0)
        n = C.c_int()
        if lines is not None and hasattr(lines, "data_ptr"):
            import torch
            if not (hasattr(iq, "data_ptr") and _device_tensor(lines, torch.float64, room * self.N)
                    and _device_tensor(reports, torch.uint8, room * SCAN_REPORT_DTYPE.itemsize)):
                raise MgpuError("device output: device input, a contiguous float64 tensor [n, N] and a contiguous uint8 tensor [n, %d]"
                                % SCAN_REPORT_DTYPE.itemsize)
            self.rx._ck(self.lib.mgpu_scan_process_dev(self.h, ptr, fmt, n_in, lines.data_ptr(), reports.data_ptr(), C.byref(n), stream))
            return n.value
        out, rep = np.zeros((max(room, 1), self.N)), np.zeros(max(room, 1), SCAN_REPORT_DTYPE)
        self.rx._ck(self.lib.mgpu_scan_process(self.h, ptr, fmt, n_in, _ptr(out), _ptr(rep), C.byref(n)))
        return out[: n.value], rep[: n.value]

    def process(self, iq):
        """-> (lines float64 [n, N], [one dict per line, as scan_reports makes them])"""
        lines, reports = self.process_raw(iq)
        return lines, scan_reports(reports)

    def bin_hz(self, f):
        """the frequency of bin f (fractions allowed) relative to the stream's centre"""
        return (f - self.N / 2) * 48000.0 * self.D / self.N

    def plan(self, report, sideband=0, min_hz=1800, max_hz=3200, audio_centre_hz=1472):
        """the channels [(offset_hz, sideband, 1.0), ...] of the report's runs whose width count * R / N lies in [min_hz, max_hz], what a
        Mercury signal's 2.4 kHz may look like; a run whose band would leave (-R/2, R/2) is left out"""
        out = []
        for run in report["runs"]:
            if not min_hz <= run["count"] * 48000.0 * self.D / self.N <= max_hz:
                continue
            try:
                out.append(host_scan_plan(run, self.D, self.log2n, sideband, audio_centre_hz))
            except MgpuError:
                pass
        return out


# ---- carrier tuner (include/ext/mercury_tuner.h) ---------------------------------------------------------------------------
TUNER_SYMBOLS = names("ext/mercury_tuner.h")
TUNE_DEFAULT_MIN_METRIC = 0.44          # MGPU_TUNE_DEFAULT_MIN_METRIC: measured (profiles/tuner.md)
TUNE_DEFAULT_CARRIER_HZ = 1471.875
TUNE_REPORT_DTYPE = np.dtype([("metric", np.float64), ("frac_hz", np.float64), ("delta_hz", np.float64), ("contrast", np.float64),
                              ("phase", np.int32), ("shift", np.int32), ("offset_hz", np.int32), ("valid", np.int32),
                              ("nonfinite", np.int32), ("pad", np.int32)])              # mgpu_tune_report


class TuneConfig(C.Structure):          # mgpu_tune_config
    _fields_ = [("struct_size", C.c_int), ("D", C.c_int), ("S", C.c_int), ("audio_centre_hz", C.c_int), ("ntaps", C.c_int),
                ("symbols", C.c_int), ("taps", C.c_void_p), ("carrier_hz", C.c_double), ("min_metric", C.c_double), ("search", C.c_int),
                ("pad", C.c_int)]


def tune_config(D, S, symbols=32, search=8, taps=None, audio_centre_hz=1472, carrier_hz=TUNE_DEFAULT_CARRIER_HZ,
                min_metric=TUNE_DEFAULT_MIN_METRIC):
    """-> (mgpu_tune_config, keep-alive of its taps)"""
    h, ntaps, address = _taps_arg(taps)
    return TuneConfig(C.sizeof(TuneConfig), int(D), int(S), int(audio_centre_hz), ntaps, int(symbols), address, float(carrier_hz),
                      float(min_metric), int(search), 0), h


def tune_samples(D, symbols=32):
    """n_in of one call: 4 D 272 (symbols + 1)"""
    return 4 * int(D) * 272 * (int(symbols) + 1)


def tune_reports(reports):
    """a TUNE_REPORT_DTYPE array -> [{metric, phase, frac_hz, shift, delta_hz, contrast, offset_hz, valid, nonfinite}]"""
    return [{"metric": float(r["metric"]), "phase": int(r["phase"]), "frac_hz": float(r["frac_hz"]), "shift": int(r["shift"]),
             "delta_hz": float(r["delta_hz"]), "contrast": float(r["contrast"]), "offset_hz": int(r["offset_hz"]), "valid": int(r["valid"]),
             "nonfinite": int(r["nonfinite"])} for r in reports]


def host_tune_process(iq, D, channels, struct_size=None, fmt=None, want_arrays=False, **config):
    """the twin (mgpu_host_tune_process) on one block of tune_samples(D, symbols) IQ samples -> reports TUNE_REPORT_DTYPE [S]; with
    want_arrays also G complex128 [S, 272], E float64 [S, 272], Q float64 [S, 256]"""
    chs = chan_channels(channels)
    k, _keep = tune_config(D, len(chs), **config)
    if struct_size is not None:
        k.struct_size = struct_size
    ptr, f, n_in, _x = _iq(iq)
    S = max(len(chs), 1)
    reports = np.zeros(S, TUNE_REPORT_DTYPE)
    G, E, Q = np.zeros((S, 272), np.complex128), np.zeros((S, 272)), np.zeros((S, 256))
    _twin(load_library().mgpu_host_tune_process, C.byref(k), chs, ptr, f if fmt is None else fmt, n_in, _ptr(reports), _ptr(G), _ptr(E),
          _ptr(Q), code=1)
    return (reports, G, E, Q) if want_arrays else reports


def host_tune_plan(reports, channels):
    """the refined plan [(offset_hz, sideband, gain), ...] (mgpu_host_tune_plan): a report's offset where it is valid, the channel's own
    where not; sideband and gain are kept. reports: a TUNE_REPORT_DTYPE array or the dicts tune_reports makes"""
    chs = chan_channels(channels)
    if len(reports) != len(chs):
        raise MgpuError("one report per channel")
    out = []
    for r, ch in zip(reports, chs):
        rep = np.zeros(1, TUNE_REPORT_DTYPE)
        rep["offset_hz"], rep["valid"] = int(r["offset_hz"]), int(r["valid"])
        refined = ChanChannel()
        _twin(load_library().mgpu_host_tune_plan, _ptr(rep), C.byref(ch), C.byref(refined), code=1)
        out.append((refined.offset_hz, refined.sideband, refined.gain))
    return out


class Tuner(_Handle):
    """The channels of a plan (as chan_channels takes them) onto their stations to the hertz, on an RxPhy context
    (include/ext/mercury_tuner.h). process() takes one block of exactly `samples` IQ samples, complex64 / complex128 / int16 [..., 2]
    (numpy, or a torch tensor on the context's device), and returns one dict per channel; plan() turns them into the refined plan. A
    call is one measurement and stands alone."""
    _destroy = "mgpu_tune_destroy"

    def __init__(self, rx, D, channels, symbols=32, search=8, taps=None, audio_centre_hz=1472, carrier_hz=TUNE_DEFAULT_CARRIER_HZ,
                 min_metric=TUNE_DEFAULT_MIN_METRIC):
        self.rx, self.lib, self.D = rx, rx.lib, int(D)
        self._chs = chan_channels(channels)
        self.S = len(self._chs)
        self.config, self._taps = tune_config(D, self.S, symbols, search, taps, audio_centre_hz, carrier_hz, min_metric)
        self.h = C.c_void_p()
        rx._ck(self.lib.mgpu_tune_create(rx.h, C.byref(self.config), self._chs, C.byref(self.h)))
        self.samples = int(self.lib.mgpu_tune_samples(self.h))

    @property
    def channels(self):
        """the plan being refined"""
        return [(ch.offset_hz, ch.sideband, ch.gain) for ch in self._chs]

    def retune(self, s, channel):
        ch = chan_channels([channel])
        self.rx._ck(self.lib.mgpu_tune_retune(self.h, int(s), ch))
        self._chs[int(s)] = ch[0]

    def process_raw(self, iq):
        """-> reports TUNE_REPORT_DTYPE [S] (a blocking call)"""
        ptr, fmt, n_in, _keep = _iq(iq)
        reports = np.zeros(self.S, TUNE_REPORT_DTYPE)
        self.rx._ck(self.lib.mgpu_tune_process(self.h, ptr, fmt, n_in, _ptr(reports)))
        return reports

    def process(self, iq):
        """-> [one dict per channel, as tune_reports makes them]"""
        return tune_reports(self.process_raw(iq))

    def arrays(self):
        """the last call's G complex128 [S, 272], E float64 [S, 272], Q float64 [S, 256]"""
        G, E, Q = np.zeros((self.S, 272), np.complex128), np.zeros((self.S, 272)), np.zeros((self.S, 256))
        self.rx._ck(self.lib.mgpu_tune_arrays(self.h, _ptr(G), _ptr(E), _ptr(Q)))
        return G, E, Q

    def plan(self, reports):
        """the refined plan [(offset_hz, sideband, gain), ...]: what Channelizer takes"""
        return host_tune_plan(reports, self.channels)


# ---- wideband impulse blanker (include/ext/mercury_wideband_blanker.h) --------------------------------------------------
WBLANK_SYMBOLS = names("ext/mercury_wideband_blanker.h")
WBLANK_DEFAULT_THRESHOLD = 38.0         # MGPU_WBLANK_DEFAULT_THRESHOLD: measured (profiles/wideband_blanker.md)
WBLANK_DEFAULT_GUARD = 4
WBLANK_DEFAULT_MAX_SHARE = 0.125
WBLANK_REPORT_DTYPE = np.dtype([("block", np.int64), ("level", np.float64), ("exceeding", np.int32), ("blanked", np.int32),
                                ("capped", np.int32), ("pad", np.int32)])                # mgpu_wblank_report


class WblankConfig(C.Structure):        # mgpu_wblank_config
    _fields_ = [("struct_size", C.c_int), ("D", C.c_int), ("format", C.c_int), ("block", C.c_int), ("threshold", C.c_double),
                ("max_share", C.c_double), ("guard", C.c_int), ("max_in", C.c_int)]


class WblankState(C.Structure):         # mgpu_wblank_state
    _fields_ = [("position", C.c_uint64), ("blocks", C.c_uint64), ("D", C.c_int), ("block", C.c_int), ("cap", C.c_int), ("max_in", C.c_int),
                ("format", C.c_int), ("delay", C.c_int)]


def wblank_config(D, fmt="cf64", block=0, threshold=WBLANK_DEFAULT_THRESHOLD, guard=WBLANK_DEFAULT_GUARD,
                  max_share=WBLANK_DEFAULT_MAX_SHARE, max_in=0):
    """-> mgpu_wblank_config; fmt 'cs16', 'cf32', 'cf64' or an MGPU_IQ_* number (an unknown number is the library's to refuse)"""
    return WblankConfig(C.sizeof(WblankConfig), int(D), _iq_format_number(fmt), int(block), float(threshold), float(max_share), int(guard), int(max_in))


def wblank_block(D, block=0):
    """B: `block`, or the default of D, the least multiple of 64 D that is >= 256"""
    return int(block) or -(-256 // (64 * int(D))) * 64 * int(D)


def wblank_reports(reports):
    """a WBLANK_REPORT_DTYPE array -> [{block, level, exceeding, blanked, capped}]"""
    return [{"block": int(r["block"]), "level": float(r["level"]), "exceeding": int(r["exceeding"]), "blanked": int(r["blanked"]),
             "capped": int(r["capped"])} for r in reports]


def host_wblank_process(iq, D, position=0, struct_size=None, fmt=None, **config):
    """the twin (mgpu_host_wblank_process): a fresh stage (wblank_config(D, the input's format, **config)) seeked to `position` and fed
    `iq` whole -> (out, as the input; reports WBLANK_REPORT_DTYPE [n_in / B])"""
    return _host_block_process("wblank", wblank_config, lambda k: max(wblank_block(D, k.block), 1) if 1 <= int(D) <= 64 else 1,
                               WBLANK_REPORT_DTYPE, iq, D, position, struct_size, fmt, config)


class WidebandBlanker(_BlockStage):
    """One wideband IQ stream at 48000 * D out again in its own format fmt ('cs16', 'cf32', 'cf64'), one block of B samples late, with
    its clicks replaced by zero, on an RxPhy context (include/ext/mercury_wideband_blanker.h). The other arguments are wblank_config's.
    process() takes complex64 / complex128 / int16 [..., 2] samples of that format (numpy, or a torch tensor on the context's device), a
    multiple of B of them, and gives one report per emitted block (32 bytes each on the device). status() is mgpu_wblank_state:
    position, blocks, D, block, cap, max_in, format, delay."""
    _destroy, _prefix, _make_config, _State, _noun = "mgpu_wblank_destroy", "wblank", wblank_config, WblankState, "blanker"
    _REPORT_DTYPE, _decode = WBLANK_REPORT_DTYPE, wblank_reports

    def __init__(self, rx, D, fmt="cf64", **config):
        st = self._create(rx, D, fmt, config)
        self.cap, self.delay = st.cap, st.delay


# ---- IQ corrector (include/ext/mercury_iq_corrector.h) -------------------------------------------------------------------
IQC_SYMBOLS = names("ext/mercury_iq_corrector.h")
IQC_DEFAULT_MEMORY = 1024               # MGPU_IQC_DEFAULT_MEMORY
IQC_DEFAULT_BLOCK = 4096                # block = 0
IQC_SKIPPED, IQC_NO_BALANCE = 1, 2      # MGPU_IQC_SKIPPED, MGPU_IQC_NO_BALANCE
IQC_REPORT_DTYPE = np.dtype([("block", np.int64), ("dc_re", np.float64), ("dc_im", np.float64), ("skew", np.float64), ("gain", np.float64),
                             ("flags", np.int32), ("clamped", np.int32)])                 # mgpu_iqc_report


class IqcConfig(C.Structure):           # mgpu_iqc_config
    _fields_ = [("struct_size", C.c_int), ("D", C.c_int), ("format", C.c_int), ("block", C.c_int), ("memory", C.c_int), ("dc", C.c_int),
                ("balance", C.c_int), ("fixed", C.c_int), ("fixed_dc_re", C.c_double), ("fixed_dc_im", C.c_double), ("fixed_skew", C.c_double),
                ("fixed_gain", C.c_double), ("max_in", C.c_int), ("pad", C.c_int)]


class IqcState(C.Structure):            # mgpu_iqc_state
    _fields_ = [("position", C.c_uint64), ("blocks", C.c_uint64), ("D", C.c_int), ("block", C.c_int), ("max_in", C.c_int), ("format", C.c_int),
                ("lambda_", C.c_double), ("T", C.c_double * 6), ("dc_re", C.c_double), ("dc_im", C.c_double), ("skew", C.c_double),
                ("gain", C.c_double), ("flags", C.c_int), ("pad", C.c_int)]


def iqc_config(D, fmt="cf32", block=0, memory=IQC_DEFAULT_MEMORY, dc=1, balance=1, fixed=0, fixed_dc_re=0.0, fixed_dc_im=0.0, fixed_skew=0.0,
               fixed_gain=1.0, max_in=0):
    """-> mgpu_iqc_config; fmt 'cs16', 'cf32', 'cf64' or an MGPU_IQ_* number (an unknown number is the library's to refuse)"""
    return IqcConfig(C.sizeof(IqcConfig), int(D), _iq_format_number(fmt), int(block), int(memory), int(dc), int(balance), int(fixed), float(fixed_dc_re),
                     float(fixed_dc_im), float(fixed_skew), float(fixed_gain), int(max_in), 0)


def iqc_reports(reports):
    """an IQC_REPORT_DTYPE array -> [{block, dc_re, dc_im, skew, gain, skipped, no_balance, clamped}]"""
    return [{"block": int(r["block"]), "dc_re": float(r["dc_re"]), "dc_im": float(r["dc_im"]), "skew": float(r["skew"]),
             "gain": float(r["gain"]), "skipped": bool(r["flags"] & IQC_SKIPPED), "no_balance": bool(r["flags"] & IQC_NO_BALANCE),
             "clamped": int(r["clamped"])} for r in reports]


def iqc_image_db(skew, gain):
    """The image ratio, in dB (station over image), of the uncorrected front end that the coefficients describe: Q' = g (Q cos(phi) +
    I sin(phi)) with g sin(phi) = skew and g cos(phi) = 1 / gain. A station at +f comes out as K1 e^{+} + K2 e^{-} with
    K1 = (1 + g e^{-j phi}) / 2 and K2 = (1 - g e^{+j phi}) / 2; the ratio is |K1|^2 / |K2|^2 =
    ((1 + c)^2 + s^2) / ((1 - c)^2 + s^2), c = 1 / gain, s = skew. A perfect front end (skew 0, gain 1) gives +inf."""
    c, s = 1.0 / float(gain), float(skew)
    image = (1.0 - c) ** 2 + s ** 2
    return float("inf") if image == 0.0 else 10.0 * float(np.log10(((1.0 + c) ** 2 + s ** 2) / image))


def host_iqc_process(iq, D, position=0, struct_size=None, fmt=None, state=None, **config):
    """the twin (mgpu_host_iqc_process): a fresh stage (iqc_config(D, the input's format, **config)) seeked to `position` and fed `iq`
    whole -> (out, as the input; reports IQC_REPORT_DTYPE [n_in / B]). state: a float64 array [6], T before the first block, which
    becomes T after the last (mgpu_host_iqc_continue)."""
    return _host_block_process("iqc", iqc_config, lambda k: k.block if k.block > 0 else IQC_DEFAULT_BLOCK, IQC_REPORT_DTYPE, iq, D, position,
                               struct_size, fmt, config, state)


class IqCorrector(_BlockStage):
    """One wideband IQ stream at 48000 * D out again in its own format fmt ('cs16', 'cf32', 'cf64'), with no delay, less its DC offset and
    its IQ imbalance, on an RxPhy context (include/ext/mercury_iq_corrector.h). The other arguments are iqc_config's. process() takes
    complex64 / complex128 / int16 [..., 2] samples of that format (numpy, or a torch tensor on the context's device), a multiple of B of
    them, and gives one report per block (48 bytes each on the device). status() is mgpu_iqc_state: position, blocks, D, block, max_in,
    format, lambda_, T [6], dc_re, dc_im, skew, gain, flags (it waits for the handle's earlier calls)."""
    _destroy, _prefix, _make_config, _State, _noun = "mgpu_iqc_destroy", "iqc", iqc_config, IqcState, "corrector"
    _REPORT_DTYPE, _decode = IQC_REPORT_DTYPE, iqc_reports

    def __init__(self, rx, D, fmt="cf32", **config):
        self.lambda_ = self._create(rx, D, fmt, config).lambda_

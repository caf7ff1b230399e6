"""What the context-reuse tests share (tests/test_context_reuse_host.py, tests/test_gpu_context_reuse.py): the inputs, the probes, the
disturbances and the table of what a probe may leave out. A plain module: no test lives here, and nothing here loads the library when it
is imported.

The rule the GPU test holds the library to needs no tolerance: a context that has done something else before gives the bytes a fresh
context gives. A probe is a function probe(rx, cfg) -> {field: bytes} that makes a few small calls on fixed inputs and returns everything
they write; a disturbance is a function disturb(rx, cfg) that uses the context hard in one direction and, where it changed an option,
puts it back through the public setters and checks through the getters that the defaults are back."""
import functools

import numpy as np

from conftest import OPERATING_ESN0, SEED
from oraclelib import CARRIER, NO_FILTER_MESSAGE, SINGLE_MESSAGE, Oracle, noise_amp_for

MODES = (0, 8, 16, 100)
MAX_ITERS, MAX_BATCH = 50, 16
GOOD_FRAMES, GOOD_DB, LOST_FRAME, LOST_DB = (7000, 7001), 4.0, 7000, -12.0
WINDOW_DELAY, WINDOW_NOISE = 9321, 0.01

# What a probe may leave out: only what a header documents as cumulative or timed. Each row: (what, where it would show, the header's
# sentence). No probe drops a field for any other reason.
EXCEPTIONS = (
    ("kernel and host-path timings",
     "taps['cycles'] of receive(taps=True); kernel_ms_avg, last_sync_kernel_ms, host_path_last (no probe calls them)",
     "include/mercury_gpu.h: 'cycles [16] shader-clock stamps at the front-end's phase boundaries for a frame from the middle of the "
     "batch (profiling aid)'; 'mgpu_kernel_ms_avg returns the average launch duration in ms over the launches since then'; "
     "'duration (ms, HIP events on the launch stream) of the kernel of the most recent synchroniser call'; 'Profile of the most recent "
     "mgpu_rx_batch call ... from device events'"),
    ("ladder_counters",
     "estimator-ladder counters (no probe runs with a ladder; a disturbance that sets one removes it, and a ladder set anew starts at zero)",
     "include/mercury_estimator.h: 'frames decoded by each rung and frames seen since the ladder was set (or the last reset)'"),
    ("pool counters",
     "RxPool.counters (the pool is outside these tests: it forwards none of the optional stages)",
     "include/mercury_pool.h: the counters of the last pool call, with wall_ms and device_ms"),
    ("decoder_hard_frames",
     "the count of frames decided without iterating (no probe calls it)",
     "include/mercury_gpu.h: 'Frames the fp64 decoder of this context has decided WITHOUT iterating, since the context was created'"),
)
DROPPED_FIELDS = {"span_host": ("cycles",)}       # the one field a probe's call writes and the probe leaves out: the first row above

# the non-default settings disturbance b) switches on, and the sensitivity test leaves on; tests/test_context_reuse_host.py checks with
# the host twins that the blanker and the excisor act on the probes' inputs with them
LADDER_ON = [(9, 5), ("bank", dict(tau=[(-333.33, 333.33), (-333.33, 2333.33)], snr_db=5.0))]
NMAP_ON = dict(dead_band=1.5, smooth=2)
BLANKER_ON = dict(threshold=5.0, guard=2, max_share=0.25)
EXCISOR_ON = dict(threshold=2.0, guard=0, max_bins=32)
EXCISOR_SEEN_ON = 100       # the mode on whose frame window these settings remove bins (mode 8's clean windows pass at any threshold)
NMAP_OFF = {"dead_band": 2.0, "smooth": 1}
BLANKER_OFF = {"threshold": 24.0, "guard": 4, "max_share": 0.125}
EXCISOR_OFF = {"threshold": 12.0, "guard": 1, "max_bins": 16}


# ---- 1. inputs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle(cfg):
    return Oracle(cfg, MAX_ITERS)


@functools.lru_cache(maxsize=None)
def frames(cfg):
    """{"good": [(frame, payload), (frame, payload)], "lost": (frame, payload)}"""
    orc = oracle(cfg)
    op = OPERATING_ESN0[cfg]
    return {"good": [orc.gen_frame(SEED, f, noise_amp_for(op + GOOD_DB)) for f in GOOD_FRAMES],
            "lost": orc.gen_frame(SEED, LOST_FRAME, noise_amp_for(op + LOST_DB))}


@functools.lru_cache(maxsize=None)
def span_frames(cfg):
    """[good, lost, good]: complex128 [3, frame_samples]"""
    fr = frames(cfg)
    return np.stack([fr["good"][0][0], fr["lost"][0], fr["good"][1][0]])


@functools.lru_cache(maxsize=None)
def poison_frames(cfg):
    """the good frame at 1e150, with a NaN at sample 100, with +Inf at sample 200, and all zeros: complex128 [4, frame_samples]"""
    good = frames(cfg)["good"][0][0]
    out = [good * 1e150, good.copy(), good.copy(), np.zeros_like(good)]
    out[1][100] = np.nan
    out[2][200] = np.inf
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def full_batch(cfg):
    """MAX_BATCH frames: [good, lost, good], then the poison frames over and over"""
    p = poison_frames(cfg)
    return np.concatenate([span_frames(cfg)] + [p[(i % 4): (i % 4) + 1] for i in range(MAX_BATCH - 3)])


def window(orc, delay, noise, seed, carrier=CARRIER, frame_idx=1):
    """one capture window as tests/test_sync_blocks.py builds it: noise, and from `delay` on the frame of payload frame_idx (None: noise only)"""
    win = np.random.default_rng(seed).standard_normal(orc.buffer_samples()) * noise
    if delay is None:
        return win, None
    payload = orc.gen_payload(SEED, frame_idx)
    pb = orc.tx_passband(orc.payload_to_bits(payload), carrier=carrier)
    win[delay: delay + pb.size] += pb
    return win, payload


@functools.lru_cache(maxsize=None)
def windows(cfg):
    """(float64 [2, buffer samples]: a frame at WINDOW_DELAY in noise, and noise only; the frame's payload)"""
    orc = oracle(cfg)
    with_frame, payload = window(orc, WINDOW_DELAY, WINDOW_NOISE, SEED & 0xFFFF)
    noise_only, _ = window(orc, None, WINDOW_NOISE, (SEED & 0xFFFF) + 1)
    return np.stack([with_frame, noise_only]), payload


@functools.lru_cache(maxsize=None)
def windows_int16(cfg):
    wins, _ = windows(cfg)
    return np.round(wins * (20000.0 / np.abs(wins).max())).astype(np.int16)


@functools.lru_cache(maxsize=None)
def more_windows(cfg, n, carrier):
    """n windows for a disturbance: frames at other delays on another carrier, the last one noise only"""
    orc = oracle(cfg)
    return np.stack([window(orc, None if i == n - 1 else 5000 + 3331 * i, 0.02, 100 + i, carrier=carrier, frame_idx=10 + i)[0] for i in range(n)])


@functools.lru_cache(maxsize=None)
def tx_payloads(cfg):
    return np.random.default_rng(SEED + 1).integers(0, 256, (2, oracle(cfg).payload_bytes)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pattern_windows(cfg):
    """interpolated baseband [2, 24 symbols] with the ACK pattern (for detect_ack_pattern) and [2, 24 symbols] with the mode's MFSK
    preamble (for time_sync_mfsk), each at its own symbol slot in noise (tests/test_sync_blocks.py:_pattern_windows)"""
    orc = oracle(cfg)
    rng = np.random.default_rng(SEED + 2)
    out = []
    for which in (1, 0):
        pat = np.repeat(orc.mfsk_pattern(which) / 16.0, 4)
        bufs = []
        for w in range(2):
            buf = (0.05, 1.0)[w] * (rng.standard_normal(24 * 1088) + 1j * rng.standard_normal(24 * 1088))
            buf[(3 + 2 * w) * 1088: (3 + 2 * w) * 1088 + pat.size] += pat
            bufs.append(buf)
        out.append(np.stack(bufs))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def hf_audio():
    return np.random.default_rng(SEED + 3).standard_normal((3, 4096))


# ---- 2. probes ---------------------------------------------------------------------------------------------------------------------------
def fields(prefix, value):
    """{name: bytes} of what a call returned: an array as its bytes, a structured array field by field (the bytes between an aligned
    record's fields belong to nobody), a dict / tuple / list entry by entry, a number as its float64 or int64"""
    if isinstance(value, dict):
        out = {}
        for k, v in value.items():
            out.update(fields("%s.%s" % (prefix, k), v))
        return out
    if isinstance(value, (tuple, list)):
        out = {}
        for i, v in enumerate(value):
            out.update(fields("%s[%d]" % (prefix, i), v))
        return out
    a = np.asarray(value)
    if a.dtype.names:
        out = {}
        for n in a.dtype.names:
            out.update(fields("%s.%s" % (prefix, n), np.ascontiguousarray(a[n])))
        return out
    assert a.dtype != object, (prefix, type(value))
    return {prefix: np.ascontiguousarray(a).tobytes()}


def probe_span_host(rx, cfg):
    out = rx.receive(span_frames(cfg), taps=True, want_llr=True)
    assert set(DROPPED_FIELDS["span_host"]) <= set(out)
    return fields("receive", {k: v for k, v in out.items() if k not in DROPPED_FIELDS["span_host"]})


def probe_span_one(rx, cfg):
    return fields("receive1", rx.receive(span_frames(cfg)[:1], taps=False))


def probe_span_dev(rx, cfg):
    import torch
    F = 3
    bb = torch.from_numpy(span_frames(cfg).view(np.float64).reshape(F, rx.frame_samples, 2)).cuda()
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    llr, var = [z((F, 1600), torch.float32) for _ in range(2)], z((F,), torch.float32)
    bits, iters = z((F, rx.K), torch.uint8), z((F,), torch.int32)
    pay, st = [z((F, rx.payload_stride), torch.uint8) for _ in range(2)], [z((F, 6), torch.int32) for _ in range(2)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    rx.frontend_dev(bb.data_ptr(), F, llr[0].data_ptr(), var.data_ptr(), stream=s.cuda_stream)
    rx.ldpc_decode_dev(llr[0].data_ptr(), F, d_bits=bits.data_ptr(), d_iters=iters.data_ptr(), d_payload=pay[0].data_ptr(), d_stats=st[0].data_ptr(),
                       d_variance=var.data_ptr(), stream=s.cuda_stream)
    rx.receive_dev(bb.data_ptr(), F, pay[1].data_ptr(), st[1].data_ptr(), llr[1].data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    host = lambda t: t.cpu().numpy()
    return fields("dev", dict(frontend_llr=host(llr[0]), frontend_variance=host(var), decode_bits=host(bits), decode_iters=host(iters),
                              decode_payload=host(pay[0]), decode_stats=host(st[0]), fused_payload=host(pay[1]), fused_stats=host(st[1]),
                              fused_llr=host(llr[1])))


def probe_span_div(rx, cfg):
    return fields("receive_div", rx.receive_div(span_frames(cfg)[[0, 2]], 2, want_llr=True))


def probe_sync(rx, cfg):
    wins, _ = windows(cfg)
    sym, size = rx.Nofdm * 4, wins.shape[1]
    count = (rx.preamble_nsymb + rx.Nsymb) * rx.Nofdm
    out = {}
    bbi = rx.passband_to_baseband(wins, CARRIER, which=0)
    out["p2b_shared_sync_filter"] = bbi
    out["p2b_shared_data_filter"] = rx.passband_to_baseband(wins, CARRIER, which=1)
    out["p2b_per_window"] = rx.passband_to_baseband(wins, np.array([CARRIER + 3.7, CARRIER - 11.0]), which=0)
    cut = rx.passband_to_baseband(wins, CARRIER, which=1, start=np.array([4001, 17], np.int32), count=count, decimation=4)
    out["p2b_cut"] = cut
    coarse = rx.time_sync_preamble(bbi, 100)
    out["time_sync_coarse"] = coarse
    seg = (rx.preamble_nsymb + 4) * sym
    bases = [min((max(1, int(d) // sym) - 1) * sym, size - seg) for d in coarse[0]]
    out["time_sync_fine"] = rx.time_sync_preamble(np.stack([bbi[w, b: b + seg] for w, b in enumerate(bases)]), 1, 0, 2)
    out["freq_sync"] = rx.freq_sync(cut[:, 16:])
    return fields("sync", out)


def probe_rxbyte(rx, cfg):
    wins, _ = windows(cfg)
    return fields("receive_byte", dict(float64=rx.receive_byte(wins, CARRIER, state=None), int16=rx.receive_byte(windows_int16(cfg), CARRIER, state=None)))


def probe_tx(rx, cfg):
    pls = tx_payloads(cfg)
    return fields("transmit_byte", dict(single=rx.transmit_byte(pls, CARRIER, message_location=SINGLE_MESSAGE, start_sample=0),
                                        no_filter=rx.transmit_byte(pls, CARRIER, message_location=NO_FILTER_MESSAGE, start_sample=0)))


def probe_patterns(rx, cfg):
    ack, pre = pattern_windows(cfg)
    return fields("patterns", dict(detect_ack=rx.detect_ack_pattern(ack, 1), detect_break=rx.detect_ack_pattern(ack, 2),
                                   time_sync_mfsk=rx.time_sync_mfsk(pre), generate_ack=rx.generate_ack_pattern_passband(1, CARRIER),
                                   generate_break=rx.generate_ack_pattern_passband(2, CARRIER)))


def probe_selfsim(rx, cfg):
    base = rx.baseband_test_esn0([OPERATING_ESN0[cfg] + 1.0], 32, seed=5)
    res, win, sent = rx.passband_test_esn0([30.0], 2, CARRIER, seed=11, want_windows=True)
    return fields("selfsim", dict(baseband=base, passband=res, windows=win, sent=sent))


def probe_stages(rx, cfg):
    wins, _ = windows(cfg)
    rx.set_blanker("median")
    try:
        blanked = rx.blank(span_frames(cfg))
    finally:
        rx.set_blanker("off")
    rx.set_excisor("welch")
    try:
        excised = rx.excise(wins, CARRIER)
    finally:
        rx.set_excisor("off")
    return fields("stages", dict(blank=blanked, excise=excised))


def probe_hf(rx, cfg):
    return fields("hf", dict(poor=rx.hf_channel_apply(hf_audio(), "poor", SEED)))


def probe_extras(rx, cfg):
    """beyond the issue's table: the entry points with workspaces of their own that no other probe reaches"""
    wins, _ = windows(cfg)
    rng = np.random.default_rng(SEED + 4)
    enc = rx.ldpc_encode(rng.integers(0, 2, (3, rx.K)).astype(np.uint8))
    llr = np.where(enc == 1, -4.0, 4.0).astype(np.float32)
    llr[:, rng.choice(1600, 12, replace=False)] *= -0.25
    llr[2] = rng.standard_normal(1600).astype(np.float32)                   # a word that does not decode
    bits = rng.integers(0, 2, (2, rx.nReal)).astype(np.uint8)
    return fields("extras", dict(ldpc_encode=enc, ldpc_decode=rx.ldpc_decode(llr), measure_signal_only=rx.measure_signal_only(wins, CARRIER),
                                 ack_from_passband=rx.detect_ack_pattern_from_passband(wins[:, : 40 * 1088], CARRIER, 1),
                                 transmit_bit=rx.transmit_bit(bits, CARRIER)))


# (name, probe, the modes it runs on)
PROBES = (
    ("span_host", probe_span_host, (0, 8, 16, 100)),
    ("span_one", probe_span_one, (8, 16)),
    ("span_dev", probe_span_dev, (8,)),
    ("span_div", probe_span_div, (8,)),
    ("sync", probe_sync, (8,)),
    ("rxbyte", probe_rxbyte, (8, 100)),
    ("tx", probe_tx, (8, 100)),
    ("patterns", probe_patterns, (100,)),
    ("selfsim", probe_selfsim, (8,)),
    ("stages", probe_stages, (8,)),
    ("hf", probe_hf, (8,)),
    ("extras", probe_extras, (8, 100)),
)


def probes_of(cfg):
    return [(name, fn) for name, fn, modes in PROBES if cfg in modes]


def run_probes(rx, cfg, order=None):
    """{probe: {field: bytes}} of the mode's probes, run in table order or in `order` (a permutation of their indices)"""
    table = probes_of(cfg)
    out = {}
    with np.errstate(all="ignore"):
        for i in (range(len(table)) if order is None else order):
            name, fn = table[i]
            out[name] = fn(rx, cfg)
    return out


def differences(got, want):
    """[(probe, field)] where two run_probes results differ, missing fields included"""
    out = []
    for name in want:
        for field in sorted(set(want[name]) | set(got.get(name, {}))):
            if got.get(name, {}).get(field) != want[name].get(field):
                out.append((name, field))
    return out


# ---- 3. disturbances ---------------------------------------------------------------------------------------------------------------------
def capabilities(rx):
    """what the headers allow for the context's mode: {ladder, csi, nmap, cfo, pre_eq}"""
    ofdm = rx.mfsk_M == 0
    ls = ofdm and rx.estimator == 1
    return dict(ladder=ls, nmap=ls, csi=ofdm, cfo=ofdm, pre_eq=ofdm)


def assert_defaults(rx):
    assert rx.estimator_ladder == [], rx.estimator_ladder
    assert rx.demapper == "maxlog" and rx.demapper_ex == ("maxlog", NMAP_OFF), rx.demapper_ex
    assert rx.cfo == "off", rx.cfo
    assert rx.blanker == ("off", BLANKER_OFF), rx.blanker
    assert rx.excisor() == ("off", EXCISOR_OFF), rx.excisor()


# the switches of disturbance b): name -> (on, off). Off puts the parameters back as well: the setters read them for the "on" mode only
# (include/mercury_blanker.h, ext/mercury_excisor.h, mercury_demapper.h), so off goes through the default "on".
def _ladder_on(rx):
    rx.set_estimator_ladder(LADDER_ON)


def _ladder_off(rx):
    rx.set_estimator_ladder([])


def _demapper_on(rx):
    if capabilities(rx)["nmap"]:
        rx.set_demapper("nmap", **NMAP_ON)
    rx.set_demapper("csi")


def _demapper_off(rx):
    if capabilities(rx)["nmap"]:
        rx.set_demapper("nmap", **NMAP_OFF)
    rx.set_demapper("maxlog")


def _cfo_on(rx):
    rx.set_cfo("pilots")


def _cfo_off(rx):
    rx.set_cfo("off")


def _blanker_on(rx):
    rx.set_blanker("median", **BLANKER_ON)


def _blanker_off(rx):
    rx.set_blanker("median", **BLANKER_OFF)
    rx.set_blanker("off")


def _excisor_on(rx):
    rx.set_excisor("welch", **EXCISOR_ON)


def _excisor_off(rx):
    rx.set_excisor("welch", **EXCISOR_OFF)
    rx.set_excisor("off")


SWITCHES = {"ladder": (_ladder_on, _ladder_off, "ladder"), "demapper": (_demapper_on, _demapper_off, "csi"), "cfo": (_cfo_on, _cfo_off, "cfo"),
            "blanker": (_blanker_on, _blanker_off, None), "excisor": (_excisor_on, _excisor_off, None)}


def switches_of(rx):
    can = capabilities(rx)
    return [name for name, (_, _, needs) in SWITCHES.items() if needs is None or can[needs]]


def disturb_grow_and_poison(rx, cfg, want_output=False):
    """a) max_batch frames of which rows 3 and up are poison, then 1 / max_batch / 1 frames: graph captured, workspaces at full size, graph
    replayed"""
    bb = full_batch(cfg)
    with np.errstate(all="ignore"):
        big = rx.receive(bb, taps=True, want_llr=True)
        rx.receive(bb[:1])
        rx.receive(bb)
        rx.receive(bb[1:2])
    return big if want_output else None


def switch_orders(cfg):
    """two orders of switching on and of switching off, from a seeded permutation: [(on order, off order), (on order, off order)]"""
    rng = np.random.default_rng(SEED + 10 + cfg)
    names = sorted(SWITCHES)
    return [([names[i] for i in rng.permutation(len(names))], [names[i] for i in rng.permutation(len(names))]) for _ in range(2)]


def disturb_options(rx, cfg):
    """b) every option the mode has on, a span and a receive_byte with them, all off again; twice, in two orders"""
    wins, _ = windows(cfg)
    have = switches_of(rx)
    for on_order, off_order in switch_orders(cfg):
        note = "mode %d: on in the order %s, off in the order %s (of these the mode has %s)" % (cfg, on_order, off_order, have)
        for name in on_order:
            if name in have:
                SWITCHES[name][0](rx)
        with np.errstate(all="ignore"):
            rx.receive(span_frames(cfg), taps=True)
            rx.receive(span_frames(cfg))            # the chunked host path, and one frame: what goes round the captured graph while
            rx.receive(span_frames(cfg)[:1])        # an option is on (rx_batch.hip: mgpu_rx_batch)
            rx.receive_byte(wins, CARRIER)
            rx.receive_byte(more_windows(cfg, 5, CARRIER + 37.5), CARRIER + 37.5)      # more windows than the stages' workspaces were made for
        for name in off_order:
            if name in have:
                SWITCHES[name][1](rx)
        try:
            assert_defaults(rx)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (note, e))
    return note


def disturb_grouped(rx, cfg):
    """c) receive_div with D = 3 on 12 frames, and the combine step on scattered CSR groups of their LLRs"""
    bb = full_batch(cfg)[:12]
    with np.errstate(all="ignore"):
        out = rx.receive_div(bb, 3, want_llr=True)
        rx.llr_combine(out["llr_ldpc"], groups=[[11, 0, 5], [3], [7, 2, 9, 4, 1, 10, 8, 6], [0, 11]])


def disturb_receive_byte_elsewhere(rx, cfg):
    """d) 5 windows on another carrier with the coarse frequency search and 3 trials, then a short passband_to_baseband on a third carrier"""
    wins = more_windows(cfg, 5, CARRIER + 37.5)
    out = rx.receive_byte(wins, CARRIER + 37.5, trials_max=3, coarse_freq_sync=1)
    rx.receive_byte(wins[:3], CARRIER + 37.5, trials_max=3, coarse_freq_sync=1, state=out["state"][:3])       # with the links' memory fed back
    rx.passband_to_baseband(wins[0, :300], CARRIER - 120.0, which=0)


def disturb_transmit_elsewhere(rx, cfg):
    """e) 5 messages on another carrier far along the carrier's phase, other power and clipping, phase-continuous; a transmit under a
    pre-equalisation table"""
    rng = np.random.default_rng(SEED + 20)
    pls = rng.integers(0, 256, (5, rx.payload_bytes)).astype(np.uint8)
    rx.transmit_byte(pls, 1650.0, start_sample=2 ** 33 + 5, output_power_watt=0.25, preamble_papr_cut=5.0, data_papr_cut=6.0, phase_continuous=1)
    if capabilities(rx)["pre_eq"]:
        rx.set_pre_equalization_channel(rng.standard_normal(rx.Nc) + 1j * rng.standard_normal(rx.Nc))
        rx.transmit_byte(pls[:1], CARRIER)
        rx.set_pre_equalization_channel(None)


def disturb_selfsim(rx, cfg):
    """f) the self-simulations through the HF channel, with diversity and on another carrier"""
    rx.baseband_test_esn0([OPERATING_ESN0[cfg]], 48, hf_channel="poor", diversity=2)
    rx.passband_test_esn0([10.0], 4, CARRIER + 5, hf_channel="moderate")


def disturb_refusals(rx, cfg):
    """g) one bad-argument call of each entry-point family: each must raise MgpuError"""
    from mercury_amd import HfChannel, MgpuError
    n = rx.frame_samples
    calls = [
        ("receive beyond max_batch", lambda: rx.receive(np.zeros((MAX_BATCH + 1, n), np.complex128))),
        ("receive_div with D = 0", lambda: rx.receive_div(np.zeros((4, n), np.complex128), 0)),
        ("ldpc_decode beyond max_batch", lambda: rx.ldpc_decode(np.zeros((MAX_BATCH + 1, 1600), np.float32))),
        ("passband_to_baseband with filter 3", lambda: rx.passband_to_baseband(np.zeros(400), CARRIER, which=3)),
        ("freq_sync on 3 samples", lambda: rx.freq_sync(np.zeros((1, 3), np.complex128))),
        ("receive_byte beyond max_batch", lambda: rx.receive_byte(np.zeros((MAX_BATCH + 1, rx.receive_buffer_samples())), CARRIER)),
        ("transmit_byte with message location 9", lambda: rx.transmit_byte(np.zeros((1, rx.payload_bytes), np.uint8), CARRIER, message_location=9)),
        ("baseband_test_esn0 with diversity 9", lambda: rx.baseband_test_esn0([0.0], 4, diversity=9)),
        ("hf_channel_apply with a channel of no paths", lambda: rx.hf_channel_apply(np.zeros((1, 64)), HfChannel(paths=()), 1)),
        ("mgpu_set_demapper(7)", lambda: rx._ck(rx.lib.mgpu_set_demapper(rx.h, 7))),
        ("mgpu_set_cfo(7)", lambda: rx._ck(rx.lib.mgpu_set_cfo(rx.h, 7))),
        ("set_blanker with threshold 1", lambda: rx.set_blanker("median", threshold=1.0)),
        ("set_excisor with guard 9", lambda: rx.set_excisor("welch", guard=9)),
        ("set_estimator_ladder with five rungs", lambda: rx.set_estimator_ladder([(3, 3)] * 5)),
        ("excise with a NaN carrier", lambda: rx.excise(np.zeros((1, 16)), float("nan"))),
    ]
    for what, call in calls:
        try:
            call()
        except MgpuError:
            continue
        raise AssertionError("mode %d: %s was not refused" % (cfg, what))
    assert_defaults(rx)


def disturb_debug_and_timing(rx, cfg):
    """h) the generic passband_to_baseband kernel for one call, and a span under the kernel timers"""
    wins, _ = windows(cfg)
    rx.debug_p2b_variant(0)
    try:
        rx.passband_to_baseband(wins[:, :20000], CARRIER, which=1)
    finally:
        rx.debug_p2b_variant(-1)
    rx.enable_timing(True)
    try:
        rx.receive(span_frames(cfg))
        rx.kernel_ms_avg()
    finally:
        rx.enable_timing(False)


def disturb_stages_on_the_context(rx, cfg, between=None):
    """i) a handle of each stream stage on the context, one small call on each, a capture run of two hops, all closed (mode 8).
    between: called while the handles are still open"""
    from mercury_amd import BandScanner, Channelizer, HfStream, Resampler, RxCapture, WidebandBlanker
    rng = np.random.default_rng(SEED + 30)
    iq = (rng.standard_normal(4096) + 1j * rng.standard_normal(4096)).astype(np.complex128)
    P = rx.Nofdm * 4
    handles = [Channelizer(rx, 4, [(-30000, 0, 1.0), (12000, 1, 0.7)]), Resampler(rx, 44100, 48000, S=2), WidebandBlanker(rx, 4, "cf64", guard=7),
               BandScanner(rx, 4, log2n=8, blocks_per_line=2), HfStream(rx, 2, "moderate", SEED), RxCapture(rx, 2, CARRIER)]
    try:
        handles[0].process(iq)
        handles[1].process(rng.standard_normal((2, 1000)))
        handles[2].process_raw(iq)
        handles[3].process_raw(iq)
        handles[4].apply(rng.standard_normal((2, 640)))
        handles[5].run(0.01 * rng.standard_normal((2, 2 * P)))
        if between is not None:
            between()
    finally:
        for h in handles:
            h.close()


def disturb_probes(rx, cfg):
    """j) the mode's probes themselves, in a seeded random order"""
    order = np.random.default_rng(SEED + 40 + cfg).permutation(len(probes_of(cfg)))
    run_probes(rx, cfg, order)


# (name, disturbance, the modes it is defined for)
DISTURBANCES = (
    ("a_grow_and_poison", disturb_grow_and_poison, MODES),
    ("b_options_on_then_off", disturb_options, MODES),
    ("c_grouped_calls", disturb_grouped, MODES),
    ("d_receive_byte_elsewhere", disturb_receive_byte_elsewhere, MODES),
    ("e_transmit_elsewhere", disturb_transmit_elsewhere, MODES),
    ("f_self_simulations", disturb_selfsim, MODES),
    ("g_refusals", disturb_refusals, MODES),
    ("h_debug_and_timing", disturb_debug_and_timing, MODES),
    ("i_stages_on_the_context", disturb_stages_on_the_context, (8,)),
    ("j_the_probes", disturb_probes, MODES),
)


def disturbances_of(cfg):
    return [(name, fn) for name, fn, modes in DISTURBANCES if cfg in modes]


def pairs():
    """[(cfg, disturbance name)] of test_a_used_context_gives_a_fresh_contexts_bytes"""
    return [(cfg, name) for cfg in MODES for name, _ in disturbances_of(cfg)]

"""A used context gives a fresh context's bytes (tests/context_reuse_cases.py holds the inputs, the probes and the disturbances;
tests/test_context_reuse_host.py holds the inputs to their intended properties on the CPU).

A context lives for a whole receive session and carries what one call leaves for the next: workspaces grown on demand, the captured
one-frame graph, the receive_byte workspace, two carrier-phase caches, six option blocks with device tables of their own, the
pre-equalisation table, stream-stage handles on its stream. The per-kernel tests tie a FRESH context's output to the CPU oracle; here every
entry point's output on a context that has done something else before is held to that fresh context's output, byte for byte, with no
tolerance. What a probe leaves out is listed in context_reuse_cases.EXCEPTIONS with the header sentence that allows it. The two carrier
caches are walked through their hit, straddle and rebuild cases against the oracle itself."""
import functools

import numpy as np
import pytest

import context_reuse_cases as cases
from conftest import SEED
from oraclelib import CARRIER

pytestmark = pytest.mark.gpu


def _fresh(cfg):
    from mercury_amd import RxPhy
    return RxPhy(cfg, max_iters=cases.MAX_ITERS, max_batch=cases.MAX_BATCH)


@functools.lru_cache(maxsize=None)
def _baseline(cfg):
    """every probe of the mode on a fresh context: bytes only, the context is closed"""
    rx = _fresh(cfg)
    try:
        return cases.run_probes(rx, cfg)
    finally:
        rx.close()


def _hold(rx, cfg, what):
    diff = cases.differences(cases.run_probes(rx, cfg), _baseline(cfg))
    assert not diff, "mode %d, after %s: (probe, field) that differ from a fresh context's: %s" % (cfg, what, diff)


# ---- 1. one disturbance, then every probe ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,disturbance", cases.pairs())
def test_a_used_context_gives_a_fresh_contexts_bytes(cfg, disturbance):
    _baseline(cfg)
    rx = _fresh(cfg)
    try:
        note = dict(cases.disturbances_of(cfg))[disturbance](rx, cfg)
        _hold(rx, cfg, "%s%s" % (disturbance, " (%s)" % note if isinstance(note, str) else ""))
    finally:
        rx.close()


def test_open_stage_handles_do_not_touch_the_probes():
    """disturbance i) with the probes run while the handles are still open (they borrow the context's stream), and again behind them"""
    cfg = 8
    _baseline(cfg)
    rx = _fresh(cfg)
    try:
        cases.disturb_stages_on_the_context(rx, cfg, between=lambda: _hold(rx, cfg, "i_stages_on_the_context, its handles still open"))
        _hold(rx, cfg, "i_stages_on_the_context and the probes under its open handles")
    finally:
        rx.close()


# ---- 2. all of them on one context ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("cfg", cases.MODES)
def test_all_disturbances_in_a_row(cfg, order):
    table = cases.disturbances_of(cfg)
    perm = [int(i) for i in np.random.default_rng(SEED + 50 + 2 * cfg + order).permutation(len(table))]
    _baseline(cfg)
    rx = _fresh(cfg)
    done = []
    try:
        for i in perm:
            name, fn = table[i]
            fn(rx, cfg)
            done.append(name)
            _hold(rx, cfg, " -> ".join(done))
    finally:
        rx.close()


# ---- 3. the probes leave nothing behind either ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", cases.MODES)
def test_probes_are_idempotent(cfg):
    rx = _fresh(cfg)
    try:
        first = cases.run_probes(rx, cfg)
        second = cases.run_probes(rx, cfg)
    finally:
        rx.close()
    assert first.keys() == second.keys() and all(first[p] for p in first)
    assert not cases.differences(second, first), (cfg, cases.differences(second, first))
    assert not cases.differences(first, _baseline(cfg)), (cfg, cases.differences(first, _baseline(cfg)))


# ---- 4. the comparison sees what it should ----------------------------------------------------------------------------------------------------
def test_the_probes_see_what_they_should():
    """Without this the comparison proves nothing: an option, a table or a poison left in place changes a probe's bytes."""
    cfg = 8
    rx = _fresh(cfg)
    try:
        want = _baseline(cfg)
        with np.errstate(all="ignore"):
            for name in ("ladder", "demapper", "cfo", "blanker"):
                on, off, _ = cases.SWITCHES[name]
                on(rx)
                got = cases.probe_span_host(rx, cfg)
                assert got != want["span_host"], "a %s left on is not seen by span_host" % name
                changed = sorted(k for k in got if got[k] != want["span_host"][k])
                print("%s left on: span_host fields that change: %s" % (name, changed))
                off(rx)
                cases.assert_defaults(rx)
                assert cases.probe_span_host(rx, cfg) == want["span_host"], "span_host after the %s went off again" % name
        rng = np.random.default_rng(SEED + 60)
        rx.set_pre_equalization_channel(rng.standard_normal(rx.Nc) + 1j * rng.standard_normal(rx.Nc))
        assert cases.probe_tx(rx, cfg) != want["tx"], "a pre-equalisation table left installed is not seen by tx"
        rx.set_pre_equalization_channel(None)
        assert cases.probe_tx(rx, cfg) == want["tx"]
        # the poison of disturbance a) went through the workspaces: the rows behind the probes' rows come back non-finite
        big = cases.disturb_grow_and_poison(rx, cfg, want_output=True)
        bb = cases.full_batch(cfg)
        poisoned = [r for r in range(3, cases.MAX_BATCH) if not (np.isfinite(big["llr_ldpc"][r]).all() and np.isfinite(big["grid"][r]).all())]
        print("rows of the %d-frame call with non-finite LLR or grid values: %s" % (cases.MAX_BATCH, poisoned))
        for r in range(3, cases.MAX_BATCH):
            if not np.isfinite(bb[r]).all():
                assert r in poisoned, "row %d holds a NaN / Inf frame and came back finite" % r
        assert len(poisoned) >= (cases.MAX_BATCH - 3) // 2
        assert cases.fields("receive", {k: v[:3] for k, v in big.items() if k not in ("cycles",)}) == want["span_host"]     # rows 0..2 are span_host's
    finally:
        rx.close()
    # the excisor, on the mode on whose frame window it acts (tests/test_context_reuse_host.py)
    cfg = cases.EXCISOR_SEEN_ON
    rx = _fresh(cfg)
    try:
        on, off, _ = cases.SWITCHES["excisor"]
        on(rx)
        assert cases.probe_rxbyte(rx, cfg) != _baseline(cfg)["rxbyte"], "an excisor left on is not seen by rxbyte"
        off(rx)
        cases.assert_defaults(rx)
        assert cases.probe_rxbyte(rx, cfg) == _baseline(cfg)["rxbyte"]
    finally:
        rx.close()


# ---- 5. the two carrier-phase caches against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [8, 100])
def test_receive_mixer_table_sequence_equals_the_oracle(cfg):
    """launch.hip mixer_table: a hit when the carrier is the cached one and the cached count covers the call. Longer, shorter, another
    carrier, the first one again - every call bit for bit the oracle's, as test_gpu_passband_to_baseband demands of a fresh context."""
    orc = cases.oracle(cfg)
    wins, _ = cases.windows(cfg)
    rx = _fresh(cfg)
    try:
        for step, (carrier, n) in enumerate([(CARRIER, 300), (CARRIER, 20000), (CARRIER, 1025), (CARRIER + 1.25, 20000), (CARRIER, 20000)]):
            for which in (0, 1):
                got = rx.passband_to_baseband(wins[:, :n], carrier, which=which)
                for w in range(2):
                    want = orc.passband_to_baseband(wins[w, :n], carrier=carrier, which=which)
                    assert got[w].tobytes() == want.tobytes(), (cfg, step, carrier, n, which, w)
    finally:
        rx.close()


@pytest.mark.parametrize("cfg", [8, 100])
def test_transmit_carrier_table_sequence_equals_the_oracle(cfg):
    """tx.hip ensure_carrier_table: a hit when the request lies inside [cs_start, cs_start + cs_count), built with eightfold head-room.
    Inside the head-room, across its end, before its start, far along, phase-continuous from zero, another carrier - every message bit
    for bit Oracle.transmit_byte at its start sample."""
    orc = cases.oracle(cfg)
    pls = np.random.default_rng(SEED + 70).integers(0, 256, (3, orc.payload_bytes)).astype(np.uint8)
    used = (orc.preamble_nsymb + orc.active_nsymb) * orc.Nofdm * 4
    rx = _fresh(cfg)
    try:
        N = rx.transmit_frame_samples()
        steps = [(CARRIER, 0, 1, 0), (CARRIER, N, 1, 0), (CARRIER, 8 * N - 5, 1, 0), (CARRIER, 3, 1, 0), (CARRIER, 2 ** 33 + 5, 1, 0),
                 (CARRIER, 0, 3, 1), (CARRIER + 0.5, 0, 3, 1)]
        for step, (carrier, start, F, continuous) in enumerate(steps):
            got = rx.transmit_byte(pls[:F], carrier, start_sample=start, phase_continuous=continuous)
            assert got.shape == (F, N)
            for f in range(F):
                want = orc.transmit_byte(pls[f].astype(np.int32), carrier=carrier, start_sample=start + f * used * continuous)
                assert got[f].tobytes() == want.tobytes(), (cfg, step, carrier, start, f)
    finally:
        rx.close()


# ---- 6. two handles of one stage on one context -------------------------------------------------------------------------------------------------
def _cuts(x, sizes, axis=-1):
    out, at = [], 0
    for n in sizes:
        out.append(np.ascontiguousarray(np.take(x, range(at, at + n), axis=axis)))
        at += n
    return out


def _clicked(rng, n, fmt):
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    x[rng.integers(0, n, n // 100)] *= 300.0
    if fmt == "cs16":
        return np.round(np.clip(np.stack([x.real, x.imag], axis=-1) * 50.0, -32767, 32767)).astype(np.int16)
    return x


def _stage_pairs():
    """{stage: two (make(rx) -> handle, the chunks it is fed, call(handle, chunk)) with different configurations}"""
    from mercury_amd import BandScanner, Channelizer, HfStream, Resampler, Synthesizer, WidebandBlanker
    rng = np.random.default_rng(SEED + 80)
    iq = lambda n: rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return {
        "Channelizer": [
            (lambda rx: Channelizer(rx, 4, [(-30000, 0, 1.0), (12000, 1, 0.7)]), _cuts(iq(4 * 700), [4 * 129, 4 * 1, 4 * 320, 4 * 250]),
             lambda h, c: h.process(c)),
            (lambda rx: Channelizer(rx, 3, [(5000, 0, 2.0)]), _cuts(iq(3 * 600).astype(np.complex64), [3 * 128, 3 * 400, 3 * 72]), lambda h, c: h.process(c))],
        "Resampler": [
            (lambda rx: Resampler(rx, 44100, 48000, S=2), _cuts(rng.standard_normal((2, 3000)), [441, 1000, 37, 1522]), lambda h, c: h.process(c)),
            (lambda rx: Resampler(rx, 11025, 48000, S=1), _cuts(rng.standard_normal((1, 900)), [1, 500, 399]), lambda h, c: h.process(c))],
        "Synthesizer": [
            (lambda rx: Synthesizer(rx, 4, [(-30000, 0, 1.0), (12000, 1, 0.7)]), _cuts(rng.standard_normal((2, 1500)), [129, 1, 700, 670]),
             lambda h, c: h.process(c, "cf64")),
            (lambda rx: Synthesizer(rx, 2, [(7000, 1, 0.01)]), _cuts(rng.standard_normal((1, 1000)), [500, 372, 128]), lambda h, c: h.process(c, "cs16"))],
        "BandScanner": [
            (lambda rx: BandScanner(rx, 4, log2n=8, blocks_per_line=2), _cuts(iq(128 * 12), [128 * 3, 128 * 1, 128 * 8]), lambda h, c: h.process(c)),
            (lambda rx: BandScanner(rx, 1, log2n=9, blocks_per_line=4, threshold=3.0), _cuts(iq(256 * 12).astype(np.complex64), [256 * 5, 256 * 7]),
             lambda h, c: h.process(c))],
        "WidebandBlanker": [
            (lambda rx: WidebandBlanker(rx, 4, "cf64", guard=7), _cuts(_clicked(rng, 256 * 9, "cf64"), [256 * 3, 256 * 1, 256 * 5]), lambda h, c: h.process(c)),
            (lambda rx: WidebandBlanker(rx, 1, "cs16", guard=0, threshold=30.0), _cuts(_clicked(rng, 256 * 6, "cs16"), [256 * 2, 256 * 4], axis=0),
             lambda h, c: h.process(c))],
        "HfStream": [
            (lambda rx: HfStream(rx, 2, "moderate", SEED), _cuts(rng.standard_normal((2, 64 * 40)), [64 * 17, 64 * 1, 64 * 22]), lambda h, c: h.apply(c)),
            (lambda rx: HfStream(rx, 1, "poor", SEED + 1, realisation0=3), _cuts(rng.standard_normal((1, 64 * 30)), [64 * 10, 64 * 20]),
             lambda h, c: h.apply(c))],
    }


@pytest.mark.parametrize("stage", ["Channelizer", "Resampler", "Synthesizer", "BandScanner", "WidebandBlanker", "HfStream"])
def test_two_handles_of_one_stage_on_one_context_stay_independent(stage):
    """two handles with different configurations on ONE context, fed alternately in chunks: each gives the bytes it gives alone on a
    fresh context (test_two_handles_on_two_contexts_stay_independent covers the wideband blanker only, and across contexts)"""
    pair = _stage_pairs()[stage]
    alone = []
    for make, chunks, call in pair:
        rx = _fresh(8)
        h = make(rx)
        try:
            alone.append(cases.fields(stage, [call(h, c) for c in chunks]))
        finally:
            h.close()
            rx.close()
    rx = _fresh(8)
    handles = [make(rx) for make, _, _ in pair]
    got = [[], []]
    try:
        for i in range(max(len(chunks) for _, chunks, _ in pair)):
            for k, (_, chunks, call) in enumerate(pair):
                if i < len(chunks):
                    got[k].append(call(handles[k], chunks[i]))
    finally:
        for h in handles:
            h.close()
        rx.close()
    for k in range(2):
        together = cases.fields(stage, got[k])
        assert alone[k] and any(np.frombuffer(v, np.uint8).any() for v in alone[k].values()), (stage, k)
        differ = sorted(f for f in alone[k] if together.get(f) != alone[k][f])
        assert together.keys() == alone[k].keys() and not differ, (stage, k, differ)

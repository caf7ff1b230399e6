"""The IQ corrector on the GPU (include/ext/mercury_iq_corrector.h, mercury_amd.IqCorrector): output and reports against the normative
host twin, byte for byte, at one term per thread (B = 256), an odd count (768) and sixteen (4096); every format from host and device
memory; calls of one block and of max_in blocks; chunk invariance, seeks and refusals; a caller's stream; the fixed mode; two contexts;
a used context; three links end to end behind an impaired front end; memory.

The scan kernel takes the call's blocks 256 at a time, eight to a group: the planted stream's 10 blocks end inside a group, and the call
of 270 blocks below crosses a round's border and a word of the skipped blocks' mask."""
import numpy as np
import pytest

import iqc_ref as ref
from band_links import ThreeLinks, last_error, other_rx, rx as _rx, torch as _torch
from block_stage_cases import device_reports, in_calls as _in_calls, join as _join, memory_comes_back, same as _same
from mercury_amd import (IQC_NO_BALANCE, IQC_REPORT_DTYPE, IQC_SKIPPED, Channelizer, IqCorrector, MgpuError, RxCapture, RxPhy, Synthesizer,
                         WidebandBlanker, host_chan_process, host_iqc_process, host_wblank_process, iqc_reports)
from oraclelib import CARRIER

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("memory", [0, 2])
@pytest.mark.parametrize("B", [256, 768, 4096])
@pytest.mark.parametrize("fmt", ["cs16", "cf32", "cf64"])
def test_output_and_reports_equal_the_twin(fmt, B, memory):
    """iqc_ref.planted, the input of tests/test_iq_corrector_host.py (its NO_BALANCE start, its skipped blocks, its clamping CS16): block
    by block from host memory, and in one call of max_in = 10 B from device memory"""
    torch = _torch()
    x = ref.planted(100 + B + memory, B, fmt)
    config = dict(block=B, memory=memory)
    want = host_iqc_process(x, 4, **config)
    assert want[1]["flags"][0] == IQC_NO_BALANCE and not want[1]["flags"][9]
    assert (want[1]["clamped"].sum() > 0) if fmt == "cs16" else (want[1]["flags"] & IQC_SKIPPED).sum() == 2
    qc = IqCorrector(_rx(), 4, fmt, max_in=ref.PLANTED_BLOCKS * B, **config)
    assert (qc.B, qc.max_in, qc.lambda_) == (B, ref.PLANTED_BLOCKS * B, 1.0 if memory == 0 else 0.5)
    assert _same(_join([qc.process_raw(x[b * B: (b + 1) * B]) for b in range(ref.PLANTED_BLOCKS)]), want)
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()                                            # the library works on its own stream
    qc.seek(0)
    assert _same(qc.process_raw(d_x), want)
    st = qc.status()
    assert st.position == len(x) and st.blocks == ref.PLANTED_BLOCKS
    assert list(st.T) == ref.process(x, 4, **config)[2]                 # the six doubles, and the estimate they give
    last = want[1][-1]
    assert (st.dc_re, st.dc_im, st.skew, st.gain, st.flags) == (last["dc_re"], last["dc_im"], last["skew"], last["gain"], last["flags"])
    qc.close()


def test_a_call_that_crosses_a_round_of_the_scan():
    """270 blocks of 256 in one call: the scan's second round begins at block 256, and skipped blocks lie in every word of a round's
    mask; the default max_in"""
    B = 256
    x = np.concatenate([ref.planted(60 + i, B, "cf32") for i in range(27)])
    want = host_iqc_process(x, 4, block=B, memory=2)
    qc = IqCorrector(_rx(), 4, "cf32", block=B, memory=2)
    assert qc.max_in == 1024 * B
    assert _same(qc.process_raw(x), want)
    qc.close()


@pytest.mark.parametrize("fmt,B", [("cf32", 256), ("cs16", 768), ("cf64", 4096)])
def test_chunking_and_seeking_do_not_change_a_byte(fmt, B):
    """24 blocks at max_in = 8 B: calls of 1, 2, 1, 8 (exactly max_in), 8 and 4 blocks, block by block, and 8, 8, 7, 1 give the twin's
    bytes for the stream fed whole. A refused n_in changes nothing; a seek in mid-stream gives a fresh stage's output."""
    x = np.concatenate([ref.planted(31, B, fmt), ref.planted(32, B, fmt), ref.planted(33, B, fmt)[: 4 * B]])
    config = dict(block=B, memory=2)
    want = host_iqc_process(x, 4, **config)
    qc = IqCorrector(_rx(), 4, fmt, max_in=8 * B, **config)
    assert qc.max_in == 8 * B
    for cut in ([1, 2, 1, 8, 8, 4], [1] * 24, [8, 8, 7, 1]):
        qc.seek(0)
        assert _same(_in_calls(qc, x, cut), want), cut
    qc.seek(0)
    first = qc.process_raw(x[: 4 * B])
    state = list(qc.status().T)
    for bad in (x[:0], x[: B - 1], x[: B + 1], x[: 9 * B]):             # none, no multiple of B, more than max_in
        with pytest.raises(MgpuError) as e:
            qc.process_raw(bad)
        assert e.value.code == 1
    assert "n_in must be a positive multiple of B" in last_error(_rx())
    assert qc.status().position == 4 * B and list(qc.status().T) == state
    rest = _in_calls(qc, x[4 * B:], [8, 8, 4])
    assert _same(_join([first, rest]), want)
    # a seek in mid-stream: what follows is a fresh stage's output at that position
    qc.seek(7 * B)
    assert not any(qc.status().T)
    assert _same(_in_calls(qc, x[4 * B: 12 * B], [3, 5]), host_iqc_process(x[4 * B: 12 * B], 4, position=7 * B, **config))
    for bad in (B // 2, B + 1, 2 ** 62 + B):
        with pytest.raises(MgpuError):
            qc.seek(bad)
    position = (2 ** 62 // B - 6) * B                                   # the call ends on 2^62
    qc.seek(position)
    assert _same(_in_calls(qc, x[: 6 * B], [2, 4]), host_iqc_process(x[: 6 * B], 4, position=position, **config))
    with pytest.raises(MgpuError):
        qc.process_raw(x[:B])                                           # past 2^62
    qc.close()


def test_process_dev_on_a_callers_stream_and_on_the_contexts():
    """device in, device out: the same bytes on a stream of the caller's and on the context's, with and without reports, two calls back
    to back with no wait between them; every byte of the output and of the reports is written; an output that overlaps the input is
    refused, and so is the wrong format"""
    torch = _torch()
    B, fmt = 768, "cf32"
    x = ref.planted(41, B, fmt)
    n, m = len(x), ref.PLANTED_BLOCKS
    want = host_iqc_process(x, 4, block=B, memory=2)
    qc = IqCorrector(_rx(), 4, fmt, block=B, memory=2)
    d_x = torch.from_numpy(x).cuda()
    for stream in (torch.cuda.Stream(), None):
        for with_reports in (True, False):
            qc.seek(0)
            d_out = torch.full((n,), complex(7.0, 7.0), dtype=torch.complex64, device="cuda")
            d_reports = torch.full((m, IQC_REPORT_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            half = (m // 2) * B                                             # two calls in a row on the stream, no wait between them
            got = qc.process_raw(d_x[:half], d_out[:half], d_reports[: m // 2] if with_reports else None,
                                 stream=stream.cuda_stream if stream else None)
            got += qc.process_raw(d_x[half:], d_out[half:], d_reports[m // 2:] if with_reports else None,
                                  stream=stream.cuda_stream if stream else None)
            if stream:
                stream.synchronize()
            else:
                qc.rx.lib.mgpu_synchronize(qc.rx.h, None)
            assert got == m
            assert d_out.cpu().numpy().tobytes() == want[0].tobytes()
            if with_reports:
                assert device_reports(d_reports, m, IQC_REPORT_DTYPE).tobytes() == want[1].tobytes()
            else:
                assert (d_reports.cpu().numpy() == 0xA5).all()
    with pytest.raises(MgpuError):
        qc.process_raw(d_x[: 2 * B], d_x[B: 3 * B])
    assert "d_out must not overlap d_iq" in last_error(_rx())
    with pytest.raises(MgpuError):
        qc.process_raw(x.astype(np.complex128))                         # not the handle's format
    qc.close()


def test_the_device_output_feeds_the_blanker_and_the_bank_as_it_is():
    """corrector -> wideband blanker -> channeliser on device memory and on the context's stream, no wait in between: the twins' chain"""
    torch = _torch()
    B, plan = 256, [(12000, 0, 1.0)]
    x = ref.planted(45, B, "cf64")[2 * B: 5 * B]
    x[300] += 40.0                                                      # a click for the blanker
    corrected, _ = host_iqc_process(x, 4, block=B, memory=2)
    blanked, _ = host_wblank_process(corrected, 4, block=B)
    want = host_chan_process(4, plan, blanked)
    qc, wb, ch = IqCorrector(_rx(), 4, "cf64", block=B, memory=2), WidebandBlanker(_rx(), 4, "cf64", block=B), Channelizer(_rx(), 4, plan)
    d_x = torch.from_numpy(x).cuda()
    d_a, d_b = torch.zeros_like(d_x), torch.zeros_like(d_x)
    d_audio = torch.zeros((1, len(x) // 4), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    qc.process_raw(d_x, d_a)
    wb.process_raw(d_a, d_b)
    ch.process(d_b, d_audio)
    _rx().lib.mgpu_synchronize(_rx().h, None)
    assert d_a.cpu().numpy().tobytes() == corrected.tobytes() and d_b.cpu().numpy().tobytes() == blanked.tobytes()
    assert d_audio.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes()
    for h in (qc, wb, ch):
        h.close()


@pytest.mark.parametrize("fmt", ["cs16", "cf32", "cf64"])
def test_the_fixed_mode(fmt):
    """Fixed mode equals the twin. And on a stream whose estimate is frozen by construction (lambda = 1 and the same block twice: after
    the second every sum and N are exactly twice what they were, so no quotient moves) the tracking stage's output equals the fixed
    stage's with the four doubles of a block's report handed in by configuration."""
    B = 256
    block = ref.planted(71, B, fmt)[2 * B: 3 * B]
    x = np.concatenate([block, block])
    tracking = IqCorrector(_rx(), 4, fmt, block=B, memory=0)
    t_out, t_rep = tracking.process_raw(x)
    tracking.close()
    assert _same((t_out, t_rep), host_iqc_process(x, 4, block=B, memory=0))
    assert t_rep[0].tobytes()[8:40] == t_rep[1].tobytes()[8:40] and not t_rep["flags"].any() and t_rep["gain"][1] != 1.0
    r = t_rep[1]
    config = dict(block=B, fixed=1, fixed_dc_re=r["dc_re"], fixed_dc_im=r["dc_im"], fixed_skew=r["skew"], fixed_gain=r["gain"])
    fixed = IqCorrector(_rx(), 4, fmt, **config)
    f_out, f_rep = fixed.process_raw(x)
    assert _same((f_out, f_rep), host_iqc_process(x, 4, **config))
    assert not any(fixed.status().T) and fixed.status().gain == r["gain"]
    fixed.close()
    assert f_out[B: 2 * B].tobytes() == t_out[B: 2 * B].tobytes() and f_rep[1].tobytes() == t_rep[1].tobytes()
    assert f_out.tobytes() == t_out.tobytes()
    # the switches apply to the fixed values as well
    for switch in (dict(dc=0), dict(balance=0)):
        qc = IqCorrector(_rx(), 4, fmt, **config, **switch)
        assert _same(qc.process_raw(x), host_iqc_process(x, 4, **config, **switch))
        qc.close()


NAN = float("nan")
REFUSALS = [(dict(D=65), "D must be 1..64"), (dict(fmt=5), "unknown IQ format"), (dict(block=384), "block must be a multiple of 256, 256..4096, or 0"),
            (dict(memory=1), "memory must be 0 or 2..2^20 blocks"), (dict(dc=2), "dc, balance and fixed must be 0 or 1"),
            (dict(fixed=1, fixed_dc_re=NAN), "fixed_dc_re and fixed_dc_im must be finite"),
            (dict(fixed=1, fixed_skew=0.75), "fixed_skew must be in [-0.5, 0.5]"), (dict(fixed=1, fixed_gain=NAN), "fixed_gain must be in [0.5, 2]"),
            (dict(max_in=300), "max_in must be a multiple of B, 2^26 at most")]


def test_a_refused_configuration_leaves_its_reason_with_the_context():
    for bad, why in REFUSALS:
        config = dict(D=4, fmt="cf64")
        config.update(bad)
        with pytest.raises(MgpuError) as e:
            IqCorrector(_rx(), config.pop("D"), config.pop("fmt"), **config)
        assert e.value.code == 1 and last_error(_rx()) == "mgpu_iqc_create: " + why, bad


def test_two_handles_on_two_contexts_stay_independent():
    """one stream through a corrector of each context, their calls interleaved and cut differently: each gives the twin's bytes"""
    B = 256
    xa, xb = ref.planted(51, B, "cf64")[: 9 * B], ref.planted(52, B, "cs16")[: 9 * B]
    a, b = IqCorrector(_rx(), 4, "cf64", block=B, memory=2), IqCorrector(other_rx(), 1, "cs16", block=B, memory=0, dc=0)
    got_a, got_b = [], []
    for i in range(3):
        got_a.append(a.process_raw(xa[i * 3 * B: (i + 1) * 3 * B]))
        got_b += [b.process_raw(xb[(3 * i + j) * B: (3 * i + j + 1) * B]) for j in range(3)]
    assert _same(_join(got_a), host_iqc_process(xa, 4, block=B, memory=2))
    assert _same(_join(got_b), host_iqc_process(xb, 1, block=B, memory=0, dc=0))
    a.close(), b.close()


def test_a_used_context_gives_a_fresh_contexts_bytes():
    """a context that has received, channelised and blanked (context_reuse_cases.disturb_stages_on_the_context, and a receive_dev probe
    before): the stage on it gives the bytes of the stage on a fresh context, and receive_dev afterwards gives what it gave before"""
    import context_reuse_cases as cases
    B = 768
    x = ref.planted(81, B, "cf32")
    used = RxPhy(8, max_iters=cases.MAX_ITERS, max_batch=cases.MAX_BATCH)
    before = cases.probe_span_dev(used, 8)
    cases.disturb_stages_on_the_context(used, 8)
    qc = IqCorrector(used, 4, "cf32", block=B, memory=2)
    on_used = _in_calls(qc, x, [3, 7])
    qc.close()
    fresh = RxPhy(8, max_iters=cases.MAX_ITERS, max_batch=cases.MAX_BATCH)
    qc = IqCorrector(fresh, 4, "cf32", block=B, memory=2)
    on_fresh = _in_calls(qc, x, [3, 7])
    qc.close()
    assert _same(on_used, on_fresh) and _same(on_used, host_iqc_process(x, 4, block=B, memory=2))
    after = cases.probe_span_dev(used, 8)
    assert after == before and before == cases.probe_span_dev(fresh, 8)
    used.close(), fresh.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
TP, D = 320, 4                  # synthesiser -> channeliser delays a frame by tp audio samples; the corrector adds nothing
HOPS_PER_CALL = 16              # 16 hops of 1088 audio samples are 17 blocks of 4096 IQ samples
LINKS = ThreeLinks(seed=2027, tail=TP, hops_per_call=HOPS_PER_CALL)
# link 0's channel contains 0 Hz (USB at -1000 Hz: the DC spur lies at 1000 Hz audio, away from the OFDM centre at 1472 Hz); link 1 is the
# victim; the fourth channel, which no capture listens to, lies on the victim's mirror band: the opposite sideband at the negated offset
PLAN = ((-1000, 0, 1.0), (30000, 0, 1.0), (-60000, 1, 1.0))
MIRROR = (-30000, 1, 1.0)
LEVELS_DB = (20, 30, 40, 50)    # the interferer's ladder, above a link's rms
DC_DB = (0, 10, 20, 30)         # the DC's ladder, |dc| above a link's rms in the IQ
AUDIO_BAND = (300.0, 2643.75)


def _band_noise(n, seed):
    """real noise of unit rms confined to Mercury's audio band"""
    spec = np.fft.rfft(np.random.default_rng(seed).standard_normal(n))
    hz = np.fft.rfftfreq(n, 1.0 / 48000.0)
    spec[(hz < AUDIO_BAND[0]) | (hz > AUDIO_BAND[1])] = 0.0
    audio = np.fft.irfft(spec, n)
    return audio / np.sqrt(np.mean(audio ** 2))


def test_three_links_end_to_end_behind_an_impaired_front_end():
    """Mode 8, D = 4: three frames in silence and continuous band noise on the victim's mirror band through Synthesizer -> (impairment:
    gain 1.1, 5 degrees, a DC step at the stream's start) -> (IqCorrector, everything at its defaults) -> Channelizer ->
    RxCapture.run_wideband in calls of 16 hops. The interferer's level and the DC are each the least of their ladder at which the
    existing chain alone delivers all three links unimpaired and a strict subset with that impairment alone: chosen by code that exists
    without the stage, never by the stage's output. Then: the impaired stream through the corrector delivers exactly what the unimpaired
    stream delivers, and without the corrector a strict subset."""
    torch = _torch()
    rx = _rx()
    starts = LINKS.starts_the_loop_delivers((TP,))
    _, frames = LINKS.frames()
    audio = LINKS.audio(starts)
    n_audio = audio.shape[1]
    link_audio_rms = np.sqrt(np.mean(frames[0] ** 2))
    step = HOPS_PER_CALL * rx.Nofdm * 4
    sy = Synthesizer(rx, D, PLAN + (MIRROR,))

    def synthesised(rows):
        return np.concatenate([sy.process(np.ascontiguousarray(rows[:, c: c + step]), fmt="cf64") for c in range(0, n_audio, step)])

    iq_links = synthesised(np.concatenate([audio, np.zeros((1, n_audio))]))
    iq_mirror = synthesised(np.concatenate([np.zeros((3, n_audio)), link_audio_rms * _band_noise(n_audio, 7)[None, :]]))
    sy.close()
    on = slice((max(starts) + TP) * D, (min(starts) + frames.shape[1]) * D)
    link_rms = np.sqrt(np.mean(np.abs(iq_links[on]) ** 2) / 3.0)
    assert on.stop - on.start > 48000                                   # a stretch where all three links are on
    iq_mirror *= link_rms / np.sqrt(np.mean(np.abs(iq_mirror[on]) ** 2))       # 0 dB: a link's rms in the IQ

    def stream(level_db):
        return iq_links + 10.0 ** (level_db / 20.0) * iq_mirror

    def dc_of(dc_db):
        return tuple(link_rms * 10.0 ** (dc_db / 20.0) * np.array([0.6, -0.8]))

    last_report = []

    def delivered(x, correct=False):
        x = x.astype(np.complex64)
        ch = Channelizer(rx, D, PLAN)
        cap = RxCapture(rx, 3, CARRIER, max_hops=HOPS_PER_CALL)
        qc = IqCorrector(rx, D) if correct else None
        d_x = torch.from_numpy(x).cuda()
        d_out = torch.zeros(step * D, dtype=torch.complex64, device="cuda")
        d_reports = torch.zeros((step * D // 4096, IQC_REPORT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        events = []
        for c in range(0, x.size, step * D):
            part = d_x[c: c + step * D]
            if qc:
                qc.process_raw(part, d_out, d_reports)                  # the context's stream, as run_wideband's
                part = d_out
            events += [(e[0], e[1], None, e[3].tobytes()) for e in cap.run_wideband(ch, part)]
        if qc:
            last_report[:] = iqc_reports(device_reports(d_reports, step * D // 4096, IQC_REPORT_DTYPE))[-1:]
        for h in (ch, cap, qc):
            if h:
                h.close()
        return LINKS.delivered(events)

    level = dc_db = clean = None
    for level_db in LEVELS_DB:
        clean = delivered(stream(level_db))
        if clean == {0, 1, 2} and delivered(ref.impair(stream(level_db), dc=(0.0, 0.0))) < clean:
            level = level_db
            break
    assert level is not None, "no rung of the interferer's ladder gives both outcomes with the existing chain"
    for db in DC_DB:
        if delivered(ref.impair(stream(level), gain=1.0, phase_deg=0.0, dc=dc_of(db))) < clean:
            dc_db = db
            break
    assert dc_db is not None, "no rung of the DC's ladder loses a link with the existing chain"
    impaired = ref.impair(stream(level), dc=dc_of(dc_db))
    plain = delivered(impaired)
    corrected = delivered(impaired, correct=True)
    print("delivered links: unimpaired", sorted(clean), "impaired", sorted(plain), "impaired and corrected", sorted(corrected),
          "; interferer", level, "dB and DC", dc_db, "dB above a link; planted DC", dc_of(dc_db), "; last report", last_report)
    assert clean == {0, 1, 2}
    assert corrected == clean
    assert plain < clean


def test_create_use_destroy_gives_the_memory_back():
    """50 create / process / destroy cycles (the state, the sums, the estimates, staging, the output buffers) leave the device's free
    memory where it was"""
    memory_comes_back(lambda: IqCorrector(_rx(), 64, "cf64"), ref.to_format(ref.white(64 * 4096, 6), "cf64"))

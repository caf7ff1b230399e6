"""GPU tests of every form of the Watterson HF channel kernel (csrc/hfchannel.hip: real, complex, fused passband, fused baseband, streaming)
against the definition, at the shapes where the one body they share can go wrong.

Yardstick: tests/hf_channel_ref.py, the closed form of DESIGN.md §6.1 with time and phase in 80-bit extended precision, and its derived
per-sample budget phase_bound (tests/test_hf_channel_ref_host.py holds the library's host twin to the same). The two fused forms have no
sample output to compare everywhere, so: the passband form's windows against the AWGN entry's windows sent through the reference, and
its counters against the CPU oracle's receive_byte on those very windows; the baseband form and the diversity loop by recounting on
the CPU oracle (or receive_div) what the reference composition of the same frames, realisations and noise gives. Every test prints its
measured error / budget; profiles/hf_channel.md records them."""
import numpy as np
import pytest

import oraclelib
from hf_channel_ref import analytic, channel_longdouble, phase_bound, worst_ratio
from oraclelib import CARRIER, FLAGS_BASEBAND_TEST, FLAGS_RECEIVE_BYTE, Oracle, noise_amp_for
from test_gpu_hf_stream import CHANNELS as STREAM_CHANNELS

pytestmark = pytest.mark.gpu
SEED = 0x48464652
BIG_T0 = 2 ** 32 + 320


def _rx(cfg=8, **kw):
    from mercury_amd import RxPhy
    return RxPhy(cfg, **kw)


@pytest.fixture(scope="module")
def rx8():
    rx = _rx(8, max_batch=8)
    yield rx
    rx.close()


def _channels():
    from mercury_amd import HfChannel
    return {
        "static_shifted": HfChannel(((0.0, 0.0, 0.0, 2.5),)),                       # ns = 1, not the identity
        "minus_20_db": HfChannel(((0.0, -20.0, 0.0, 0.0),)),                        # normalised amplitude 0.1 / sqrt(0.01): 1 or an ulp off
        "fading_static_fading": HfChannel(((0.0, 0.0, 0.7, 0.25), (1.5, -3.0, 0.0, 1.5), (3.0, -6.0, 2.0, -0.5)), freq_offset_hz=2.0),
        "four_paths": STREAM_CHANNELS["four_paths"](),                              # 10 ms: 80 samples at 8 kHz, 480 at 48 kHz
    }


def _signal(rng, W, n, cplx):
    return rng.standard_normal((W, n)) + 1j * rng.standard_normal((W, n)) if cplx else rng.standard_normal((W, n))


# ---- a. the apply forms over a channel table --------------------------------------------------------------------------------------
NS = [1, 63, 214, 431, 1023, 1024, 1025, 2049]       # below the 10 ms halo (8 kHz: 80, 48 kHz: 480) and the Hilbert half (215); tile edges


@pytest.mark.parametrize("name", ["static_shifted", "minus_20_db", "fading_static_fading", "four_paths"])
@pytest.mark.parametrize("form,fs", [("real", 48000.0), ("real", 8000.0), ("complex", 12000.0)])
def test_apply_forms_match_the_definition(rx8, form, fs, name):
    ch = _channels()[name]
    rng = np.random.default_rng(len(name) + int(fs))
    worst = 0.0
    for n in NS:
        x = _signal(rng, 3, n, form == "complex")
        for t0 in (0, -700):
            got = rx8.hf_channel_apply(x, ch, seed=SEED, realisation0=40, fs=fs, t0=t0)
            assert got.shape == x.shape and got.dtype == x.dtype
            ratio = worst_ratio(got, x, ch, SEED, 40, fs, t0)
            assert ratio <= 1.0, (form, fs, name, n, t0, ratio)
            worst = max(worst, ratio)
            if name != "minus_20_db" and n > 1:                                     # (a static path's phase at t = 0 is 0)
                assert not np.array_equal(got, x)                                   # none of these is the copy path
    print("hf_forms apply %s %g Hz %s: worst error / budget %.2e" % (form, fs, name, worst))


def test_one_path_at_minus_20_db_gives_the_input_back(rx8):
    """one static path at -20 dB normalises to an amplitude within an ulp of 1 (exactly 1 with this libm: then it is the copy path): the input
    back to a few ulp either way, far inside the budget the table test holds it to"""
    ch = _channels()["minus_20_db"]
    x = _signal(np.random.default_rng(3), 3, 1025, True)
    got = rx8.hf_channel_apply(x, ch, seed=SEED, fs=12000.0)
    assert np.max(np.abs(got - x)) <= 4 * 2.0 ** -53 * np.max(np.abs(x))


# ---- b. stream positions beyond 2^32 samples ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,fs", [("real", 48000.0), ("complex", 12000.0)])
def test_apply_at_a_position_beyond_2_to_32_matches_the_definition(rx8, form, fs):
    from mercury_amd import hf_channel_preset
    ch = hf_channel_preset("flutter")
    x = _signal(np.random.default_rng(11), 3, 2049, form == "complex")
    got = rx8.hf_channel_apply(x, ch, seed=SEED, realisation0=7, fs=fs, t0=BIG_T0)
    ref = channel_longdouble(x, ch, SEED, 7, fs, BIG_T0)
    ratio = worst_ratio(got, x, ch, SEED, 7, fs, BIG_T0, ref=ref)
    rms = np.sqrt(np.mean(np.abs(ref) ** 2))
    print("hf_forms apply %s flutter t0 = 2^32 + 320: error / budget %.2e, error / (1e-10 x RMS) %.1f"
          % (form, ratio, np.max(np.abs(got - ref)) / (1e-10 * rms)))
    assert ratio <= 1.0, ratio


def _stream(rx, x, ch, fs, pieces, seek=None, realisation0=0):
    from mercury_amd import HfStream
    st = HfStream(rx, x.shape[0], ch, SEED, realisation0=realisation0, fs=fs)
    if seek is not None:
        st.seek(seek)
    out, at = [], 0
    for n in pieces:
        out.append(st.apply(np.ascontiguousarray(x[:, at: at + n])))
        at += n
    L = st.latency
    st.close()
    return np.concatenate(out, axis=1), L


def _stream_ratio(o, L, x, ch, fs, t0, realisation0):
    """the stream's output against the definition on everything fed, delayed by the latency"""
    N = x.shape[1]
    assert not o[:, :L].any()
    ref = channel_longdouble(x, ch, SEED, realisation0, fs, t0)
    worst = 0.0
    for w in range(x.shape[0]):
        b = phase_bound(ch, fs, SEED, realisation0 + w, N, t0, analytic(x[w]), np.sqrt(np.mean(ref[w] ** 2)))
        worst = max(worst, float(np.max(np.abs(o[w, L:] - ref[w, : N - L]) / b[: N - L])))
    return worst


def test_stream_after_a_seek_beyond_2_to_32_matches_the_definition(rx8):
    from mercury_amd import hf_channel_preset
    ch = hf_channel_preset("flutter")
    x = _signal(np.random.default_rng(12), 3, 2304, False)
    o, L = _stream(rx8, x, ch, 48000.0, [1088, 1216], seek=BIG_T0, realisation0=7)
    ratio = _stream_ratio(o, L, x, ch, 48000.0, BIG_T0, 7)
    print("hf_forms stream flutter after seek(2^32 + 320): error / budget %.2e" % ratio)
    assert ratio <= 1.0, ratio


# ---- c. the LDS carve's upper edge: 10 ms at 96 and 192 kHz ------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [96000.0, 192000.0])
def test_real_signal_and_stream_above_48_khz_with_a_10_ms_path(rx8, fs):
    """46,448 + 24 d_max bytes of LDS: 69,488 at 96 kHz and 92,528 at 192 kHz, past the default limit of a launch"""
    ch = _channels()["four_paths"]
    x = _signal(np.random.default_rng(int(fs)), 2, 3000, False)
    got = rx8.hf_channel_apply(x, ch, seed=SEED, realisation0=3, fs=fs, t0=-700)
    ratio = worst_ratio(got, x, ch, SEED, 3, fs, -700)
    xs = _signal(np.random.default_rng(int(fs) + 1), 2, 3008, False)
    o, L = _stream(rx8, xs, ch, fs, [1472, 1536], realisation0=3)
    sratio = _stream_ratio(o, L, xs, ch, fs, 0, 3)
    print("hf_forms %g Hz, 10 ms: real error / budget %.2e, two-chunk stream %.2e" % (fs, ratio, sratio))
    assert ratio <= 1.0 and sratio <= 1.0, (ratio, sratio)


def test_complex_signal_at_192_khz_with_a_10_ms_path(rx8):
    """the complex form's largest carve: 65,536 bytes exactly"""
    ch = _channels()["four_paths"]
    x = _signal(np.random.default_rng(5), 2, 3000, True)
    got = rx8.hf_channel_apply(x, ch, seed=SEED, realisation0=3, fs=192000.0, t0=-700)
    ratio = worst_ratio(got, x, ch, SEED, 3, 192000.0, -700)
    print("hf_forms 192000 Hz, 10 ms: complex error / budget %.2e" % ratio)
    assert ratio <= 1.0, ratio


# ---- d. more signals than one launch takes -----------------------------------------------------------------------------------------
def test_signals_behind_the_first_launch_are_their_own_realisations(rx8):
    from mercury_amd import hf_channel_preset
    W, n, r0 = 65537, 64, 9
    ch = hf_channel_preset("moderate")
    rng = np.random.default_rng(6)
    x = rng.standard_normal((W, n)) + 1j * rng.standard_normal((W, n))
    got = rx8.hf_channel_apply(x, ch, seed=SEED, realisation0=r0, fs=12000.0)
    for w in (0, 65534, 65535, 65536):
        one = rx8.hf_channel_apply(x[w: w + 1], ch, seed=SEED, realisation0=r0 + w, fs=12000.0)
        assert np.array_equal(one[0].view(np.uint64), got[w].view(np.uint64)), w
    last = W - 1
    ratio = worst_ratio(got[last:], x[last:], ch, SEED, r0 + last, 12000.0)
    print("hf_forms W = 65537: row 65536 error / budget %.2e" % ratio)
    assert ratio <= 1.0, ratio


# ---- e. the fused passband form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,points,nf", [(8, [30.0, 12.0], 6), (100, [-5.0, -13.0], 4)])
def test_passband_form_windows_and_counts(cfg, points, nf):
    """mgpu_hf_passband_kernel's windows are the AWGN entry's noise-free windows (that entry at +300 dB: tests/test_receive_byte.py ties it to
    the oracle) through the definition, plus the AWGN entry's own noise at the point; and its counters are the oracle's receive_byte on
    those very windows."""
    from mercury_amd import hf_channel_preset
    seed, frame0 = 11, 5
    ch = hf_channel_preset("moderate")
    orc = Oracle(cfg)
    rx = _rx(cfg, max_batch=8)
    kw = dict(seed=seed, frame0=frame0, want_windows=True, output_power_watt=1.0)
    res, wins, sent = rx.passband_test_esn0(points, nf, CARRIER, hf_channel="moderate", **kw)
    _, pre, sent0 = rx.passband_test_esn0([300.0] * len(points), nf, CARRIER, **kw)
    _, noisy, _ = rx.passband_test_esn0(points, nf, CARRIER, **kw)
    rx.close()
    assert np.array_equal(sent, sent0)
    noise = noisy - pre
    assert np.max(np.abs(noise)) > 1e-3 * np.max(np.abs(pre))
    worst = 0.0
    for w in range(len(points) * nf):
        ref = channel_longdouble(pre[w: w + 1], ch, seed, frame0 + w, 48000.0)[0]
        b = phase_bound(ch, 48000.0, seed, frame0 + w, pre.shape[1], 0, analytic(pre[w]), np.sqrt(np.mean(ref ** 2)))
        worst = max(worst, float(np.max(np.abs(wins[w] - (ref + noise[w])) / b)))
    print("hf_forms passband cfg %d moderate: worst error / budget %.2e" % (cfg, worst))
    assert worst <= 1.0, worst
    assert not np.array_equal(wins, noisy)
    nb = orc.payload_bytes
    delay = ((orc.preamble_nsymb + 2) * orc.Nofdm + (100 if orc.Nfft == 1024 else 50)) * 4
    for p, pt in enumerate(points):
        be = fe = ok = 0
        for f in range(nf):
            w = p * nf + f
            state = oraclelib.LinkState(-1, 0.0, 0, delay + 1 if cfg >= 100 else 0)
            r = orc.receive_byte(wins[w], carrier=CARRIER, state=state)
            e = int(np.unpackbits(r["payload"] ^ sent[w][:nb]).sum())
            be += e; fe += e != 0; ok += int(r["message_decoded"])
        got = res[p]
        print("hf_forms passband cfg %d moderate %g dB: decoded %d of %d" % (cfg, pt, ok, nf))
        assert got["Frames_total"] == nf and got["Bits_total"] == nf * nb * 8
        assert (got["Error_bits_total"], got["Error_frames_total"], got["crc_ok_frames"]) == (be, fe, ok), (cfg, pt, got, be, fe, ok)
        if cfg == 8:
            assert 0 < got["crc_ok_frames"] < nf, got                      # some decode and some do not: the counts say something


# ---- f, g. the fused baseband form and the diversity loop, by recount ------------------------------------------------------------------
def _sent_bits(pl, nreal):
    """payload, its CRC16 (Modbus RTU) and the spare bits as sent, as tests/test_gpu_parity.py builds them"""
    crc = 0xffff
    for byte in pl.astype(np.uint8).tolist():
        crc ^= byte
        for _ in range(8):
            crc = (crc >> 1) ^ 0xA001 if crc & 1 else crc >> 1
    full = np.concatenate([pl.astype(np.uint8), np.array([crc & 0xff, crc >> 8], np.uint8), np.zeros(2, np.uint8)])
    return np.unpackbits(full, bitorder="little")[:nreal]


def _through_channel(orc, clean, ch, seed, index, esn0):
    """a clean frame through realisation `index` of the channel at 12 kHz, then the generator's own noise of frame `index`"""
    y = channel_longdouble(clean[None], ch, seed, index, 12000.0)[0]
    return orc.channel(y, seed, index, noise_amp_for(esn0))


@pytest.mark.parametrize("cfg,name,points,want_failed", [(8, "poor", [4.0, 10.0, 20.0], [28, 19, 22]), (0, "moderate", [-6.0, 0.0, 8.0], [18, 10, 12]),
                                                          (16, "good", [20.0, 30.0], [32, 19])])
def test_baseband_form_counts_match_a_recount_on_the_oracle(cfg, name, points, want_failed):
    """32 frames a point in batches of 20 and 12. The receiver is the context's default (AGC, variance from the equalised pilots: the oracle's
    receive_byte flags) except in the zero-forcing mode 16, which runs the way the reference's own loop does (tests/test_gpu_parity.py's
    _variants). want_failed: the frames of 32 the CPU recount below fails per point, so that a change of the reference shows."""
    from mercury_amd import hf_channel_preset
    ch = hf_channel_preset(name)
    orc = Oracle(cfg, 50)
    agc, vs, flags = (0, 0, FLAGS_BASEBAND_TEST) if cfg == 16 else (1, 1, FLAGS_RECEIVE_BYTE)
    rx = _rx(cfg, max_batch=20, agc=agc, variance_source=vs)
    n, seed, frame0 = 32, 77, 1000
    res = rx.baseband_test_esn0(points, n, seed=seed, frame0=frame0, hf_channel=ch)
    nreal = rx.nReal
    rx.close()
    failed = []
    for p, esn0 in enumerate(points):
        be = fe = it = 0
        for k in range(n):
            f = frame0 + p * n + k
            clean, pl = orc.gen_frame(seed, f, 0.0)
            ref = orc.rx(_through_channel(orc, clean, ch, seed, f, esn0), flags)
            e = int((_sent_bits(pl, nreal) != np.unpackbits(ref["bytes"].astype(np.uint8), bitorder="little")[:nreal]).sum())
            be += e
            fe += e != 0
            it += ref["iterations"]
        r = res[p]
        failed.append(fe)
        assert (r["Error_bits_total"], r["Error_frames_total"], r["Frames_total"], r["Bits_total"]) == (be, fe, n, n * nreal), (cfg, name, esn0, r, be, fe)
        assert abs(r["avg_iterations"] * n - it) < 1e-6, (cfg, name, esn0, r, it)
    print("hf_forms baseband cfg %d %s: failed of %d per point %s" % (cfg, name, n, failed))
    assert failed == want_failed and any(0 < fe < n for fe in failed), failed      # points where some frames decode and some do not


def test_diversity_loop_counts_match_a_recount_through_receive_div():
    """mgpu_baseband_test_esn0_div's indices: row r of a batch is the clean frame of group first + r // 2 through realisation 2 first + r with
    the noise of frame 2 first + r (tests/test_gpu_diversity.py pins receive_div itself)."""
    from mercury_amd import hf_channel_preset
    ch = hf_channel_preset("poor")
    cfg, D, G, seed, frame0, points = 8, 2, 12, 77, 1000, [6.0, 14.0]
    orc = Oracle(cfg, 50)
    rx = _rx(cfg, max_batch=16)
    res = rx.baseband_test_esn0(points, G, seed=seed, frame0=frame0, hf_channel=ch, diversity=D)
    nreal = rx.nReal
    failed = []
    for p, esn0 in enumerate(points):
        be = fe = it = ok = 0
        for done in range(0, G, 16 // D):                                  # the loop's batches: 8 groups, then 4
            groups = min(16 // D, G - done)
            first = frame0 + p * G + done
            rows = [_through_channel(orc, orc.gen_frame(seed, first + r // D, 0.0)[0], ch, seed, D * first + r, esn0) for r in range(groups * D)]
            out = rx.receive_div(np.stack(rows), D)
            for g in range(groups):
                sent = _sent_bits(orc.gen_payload(seed, first + g), nreal)
                e = int((sent != np.unpackbits(out["payload"][g * D], bitorder="little")[:nreal]).sum())
                be += e
                fe += e != 0
                it += int(out["stats"]["iterations_done"][g * D])
                ok += int(out["stats"]["message_decoded"][g * D] != 0)
        r = res[p]
        failed.append(fe)
        assert (r["Error_bits_total"], r["Error_frames_total"], r["crc_ok_frames"], r["Frames_total"]) == (be, fe, ok, G), (esn0, r, be, fe, ok)
        assert abs(r["avg_iterations"] * G - it) < 1e-6, (esn0, r, it)
    rx.close()
    print("hf_forms diversity cfg 8 poor D = 2: failed of %d per point %s" % (G, failed))

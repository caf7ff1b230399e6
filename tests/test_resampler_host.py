"""CPU tests of the rational resampler's host side (include/ext/mercury_resampler.h): the twin against an independent numpy model of the
rule, the default design's symmetry, gain and frequency response, the fidelity of a resampled band-limited signal, the call counts over
arbitrary cuts, every refusal, and one frame end to end through the CPU oracle's receive_byte. Figures: profiles/resampler.md."""
import ctypes as C
import functools

import numpy as np
import pytest

import resampler_ref as rr
from band_links import create_without_a_context
from mercury_amd import MgpuError, host_resamp_count, host_resamp_design, host_resamp_process, load_library, resamp_config

TABLED_IDS = ["%d-%d" % (fin, fout) for fin, fout, _, _ in rr.TABLED]


@functools.lru_cache(maxsize=None)
def _design(fin, fout):
    return host_resamp_design(fin, fout)


@pytest.mark.parametrize("fin,fout,L,M", rr.TABLED, ids=TABLED_IDS)
def test_twin_equals_the_model_for_every_tabled_ratio(fin, fout, L, M):
    """short random input, the default design and tp = 2, from the stream's start and from a seek: every output within
    (tp + 2) 2^-53 sum |h| |x| of the model's unfused products and sums, and as many outputs as the rule counts"""
    assert rr.ratio(fin, fout) == (L, M)
    rng = np.random.default_rng(fin % 9973 + L)
    for h in (_design(fin, fout), host_resamp_design(fin, fout, tp=2)):
        tp = (h.size - 1) // L
        for m0 in (0, 12345):
            x = rng.standard_normal(2 * tp + 40 + 2 * M // L)
            want, bound = rr.model(h, L, M, x, m0)
            got = host_resamp_process(fin, fout, x, position=m0, taps=h)
            assert got.shape == (1, want.size) and want.size == rr.count(L, M, m0, x.size) > 0
            assert np.all(np.abs(got[0] - want) <= (tp + 2) * 2.0 ** -53 * bound), (tp, m0)


def test_twin_filters_every_stream_and_component_alike_in_every_format():
    """S = 2 streams: int16, int32, float32 and float64 audio equal the twin on the widened doubles; IQ (C = 2) equals the real twin on I
    and on Q, for CS16, CF32 and CF64"""
    rng = np.random.default_rng(3)
    fin, fout = 44100, 48000
    i16 = rng.integers(-2 ** 15, 2 ** 15, (2, 300)).astype(np.int16)
    i32 = rng.integers(-2 ** 31, 2 ** 31, (2, 300)).astype(np.int32)
    f32 = rng.standard_normal((2, 300)).astype(np.float32)
    for x, wide in ((i16, i16 / 32768.0), (i32, i32 / 2147483647.0), (f32, f32.astype(np.float64))):
        got = host_resamp_process(fin, fout, x)
        for s in range(2):
            assert np.array_equal(got[s], host_resamp_process(fin, fout, wide[s])[0])
    cs16 = rng.integers(-2 ** 15, 2 ** 15, (2, 200, 2)).astype(np.int16)
    z = cs16[..., 0] / 32768.0 + 1j * (cs16[..., 1] / 32768.0)
    for x in (cs16, z.astype(np.complex128), z.astype(np.complex64)):
        got = host_resamp_process(2048000, 1536000, x, components=2)
        zz = z if x.dtype != np.complex64 else x.astype(np.complex128)
        for s in range(2):
            assert np.array_equal(got[s].real, host_resamp_process(2048000, 1536000, np.ascontiguousarray(zz[s].real))[0])
            assert np.array_equal(got[s].imag, host_resamp_process(2048000, 1536000, np.ascontiguousarray(zz[s].imag))[0])


@pytest.mark.parametrize("fin,fout,L,M", rr.TABLED, ids=TABLED_IDS)
def test_default_design(fin, fout, L, M):
    """symmetric to the bit, sum h = L to a few ulp, the default tp (rr.default_tp: 32 max(1, ceil(M / L)); 110 at 1/1); the response read from an FFT of the taps: pass-band
    deviation (up to cutoff - width / 2) and stop-band level (from cutoff + width / 2, width the Kaiser formula's transition) each within
    2 dB of delta = 10^(-60 / 20). Measured: pass-band -58.2 .. -60.2 dB, stop-band -58.5 .. -60.5 dB (profiles/resampler.md).

    At 1/1 the default tp is 110, not 32 (rr.default_tp): with 33 taps the stop-band would start at 24318 Hz, above the design rate's
    Nyquist frequency, the two band edges would lie closer than one transition width around 24 kHz, and the pass-band deviation was
    -57.42 dB. The design was lengthened; the bound and the bands are as they were."""
    h = _design(fin, fout)
    tp = rr.default_tp(L, M)
    assert h.size == tp * L + 1
    assert np.array_equal(h.view(np.uint64), h[::-1].copy().view(np.uint64))
    assert abs(h.sum() - L) <= 8 * np.finfo(float).eps * L
    f, H = rr.response(h, L, fin)
    cutoff, width = 0.45 * min(fin, fout), rr.kaiser_transition_hz(fin, tp)
    limit = 10 ** (-60 / 20.0) * 10 ** (2 / 20.0)
    passband = np.abs(H[f <= cutoff - width / 2] - 1).max()
    stop = H[f >= cutoff + width / 2]
    print("%d -> %d: pass-band deviation %.2f dB" % (fin, fout, 20 * np.log10(passband)))
    print("%d -> %d: stop-band level %.2f dB" % (fin, fout, 20 * np.log10(stop.max())))
    assert passband <= limit and stop.max() <= limit


@pytest.mark.parametrize("fin,fout,L,M", rr.TABLED, ids=TABLED_IDS)
def test_a_band_limited_signal_keeps_its_shape(fin, fout, L, M):
    """0.2 s of seven tones in 300 .. 2700 Hz at fin through the twin against the same tones synthesised at fout and delayed by the
    (fractional) delay: at most -50 dB, past the filter's filling. Measured: -69.6 .. -98.8 dB (profiles/resampler.md)."""
    tp = rr.default_tp(L, M)
    got = host_resamp_process(fin, fout, rr.tones(fin, fin // 5))[0]
    delay = tp * L / (2.0 * M)
    want = rr.tones(fout, got.size, delay=delay)
    skip = int(np.ceil(2 * delay)) + 1
    err = rr.error_db(got[skip:], want[skip:])
    print("%d -> %d: error %.1f dB" % (fin, fout, err))
    assert err <= -50.0


@pytest.mark.parametrize("fin,fout", [(44100, 48000), (96000, 48000), (192000, 48000), (250000, 240000), (11025, 48000)])
def test_counts_over_arbitrary_cuts_sum_to_the_whole(fin, fout):
    """host_resamp_count over random cuts and over runs of 1-sample calls (at 1/2 and 1/4 most of them produce nothing) sums to the count
    of the whole, from 0 and from 2^40 + 12345; each count is the rule's in Python integers"""
    L, M = rr.ratio(fin, fout)
    rng = np.random.default_rng(fin)
    for m0 in (0, 2 ** 40 + 12345):
        total = 5000
        cuts = [1] * 40 + list(rng.integers(1, 300, 30))
        cuts.append(total - sum(cuts))
        at, n, zeros = m0, 0, 0
        for c in cuts:
            k = host_resamp_count(fin, fout, at, int(c))
            assert k == rr.count(L, M, at, int(c))
            zeros += k == 0
            at, n = at + int(c), n + k
        assert n == host_resamp_count(fin, fout, m0, total) == rr.count(L, M, m0, total)
        if M >= 2 * L:
            assert zeros >= 20
    assert host_resamp_count(192000, 48000, 1, 1) == 0 and host_resamp_count(192000, 48000, 0, 1) == 1


def _create(k):
    """mgpu_resamp_create without a context: 1 for a refused configuration, 2 for a valid one, and a null handle"""
    return create_without_a_context(load_library().mgpu_resamp_create, C.byref(k))


def test_every_refusal_comes_before_any_device_work():
    """without a context a valid configuration gives MGPU_ERR_DEVICE and each refusal of the rule MGPU_ERR_ARG, from create and from the
    twin alike"""
    good = dict(fin=44100, fout=48000, S=1, components=1)
    assert _create(resamp_config(**good)[0]) == 2
    h = host_resamp_design(44100, 48000, tp=4)
    assert _create(resamp_config(taps=h, **good)[0]) == 2
    bad = [dict(good, fin=48000, fout=48001),              # L = 48001 > 640
           dict(good, fin=44101),                          # M = 44101 > 640
           dict(good, fin=17 * 48000),                     # M = 17 > 16 L
           dict(good, fin=0), dict(good, fout=-1),
           dict(good, tp=3), dict(good, tp=514), dict(good, tp=-2),
           dict(good, components=0), dict(good, components=3),
           dict(good, S=0),
           dict(good, taps=h, tp=2),                       # ntaps != tp L + 1
           dict(good, taps=h[:-1], tp=4),
           dict(good, taps=np.where(np.arange(h.size) == 5, np.nan, h), tp=4),
           dict(good, max_in=-1), dict(good, max_in=2 ** 30)]
    x = np.zeros(64)
    for kw in bad:
        k, _keep = resamp_config(**kw)
        assert _create(k) == 1, kw
        if "max_in" not in kw:
            n = C.c_int()
            out = np.zeros(4096)
            assert load_library().mgpu_host_resamp_process(C.byref(k), x.ctypes.data, 0, 64, 0, out.ctypes.data, 4096, C.byref(n)) == 1, kw
    k, _keep = resamp_config(**good)
    k.struct_size -= 4
    assert _create(k) == 1
    # a format that does not fit C: C = 1 takes MGPU_SAMPLES_* (0..3), C = 2 MGPU_IQ_* (0..2)
    for comps, fmt in ((1, 4), (1, -1), (2, 3), (2, -1)):
        with pytest.raises(MgpuError):
            host_resamp_process(44100, 48000, np.zeros((1, 64)) if comps == 1 else np.zeros((1, 64), np.complex128), components=comps, fmt=fmt)
    with pytest.raises(MgpuError):
        host_resamp_process(44100, 48000, np.zeros(16), position=2 ** 52)        # the position leaves 2^52
    for args in ((48000, 48001), (44101, 48000), (17 * 48000, 48000)):
        with pytest.raises(MgpuError):
            host_resamp_design(*args)
        with pytest.raises(MgpuError):
            host_resamp_count(args[0], args[1], 0, 10)
    for kw in (dict(tp=3), dict(tp=514), dict(cutoff_hz=-1.0), dict(cutoff_hz=44100 * 160), dict(atten_db=300.0)):
        with pytest.raises(MgpuError):
            host_resamp_design(44100, 48000, **kw)


def test_a_frame_resampled_to_44100_and_back_decodes_on_the_cpu_oracle():
    """A mode-8 transmit_byte frame in silence goes 48000 -> 44100 by the test's FFT method and 44100 -> 48000 by the twin; the CPU
    oracle's receive_byte decodes the sent payload from it. The frame is placed at the first of a few starts at which the oracle decodes
    the original audio delayed by floor and by ceil of the resampler's delay (17.41 samples): chosen with the existing code alone."""
    import oraclelib
    orc = oraclelib.Oracle(8, 50)
    payload = np.random.default_rng(44).integers(0, 256, orc.payload_bytes).astype(np.uint8)
    frame = orc.transmit_byte(payload)
    n = orc.buffer_samples()
    assert n % 160 == 0
    delay = 32 * 160 / (2.0 * 147)

    def window(start):
        w = np.zeros(n)
        w[start: start + frame.size] = frame
        return w

    def decodes(w):
        r = orc.receive_byte(w)
        return bool(r["message_decoded"]) and np.array_equal(r["payload"], payload)

    start = next((s for s in (2 * 1088 + 333, 3 * 1088 + 17, 1088 + 901, 4 * 1088 + 500)
                  if all(decodes(rr.delayed(window(s), d)) for d in (int(np.floor(delay)), int(np.ceil(delay))))), None)
    assert start is not None, "the oracle decodes no candidate on a pure delay"
    x44 = rr.fft_resample(window(start), 48000, 44100)
    back = host_resamp_process(44100, 48000, x44)[0]
    assert back.size == n
    err = rr.error_db(back, rr.fft_delay(window(start), delay))
    print("start %d: the round trip against the audio delayed by %.2f samples: %.1f dB" % (start, delay, err))
    assert decodes(back)


def test_host_side_is_clean_under_the_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/resampler_sanitize.cpp, mercury_amd/csrc/resamp_tables.cpp and chan_tables.cpp (the shared filter design) built as one stand-alone program with
    -fsanitize=address,undefined and run on the CPU: design, count and twin at two ratios (and a seeked third) in exactly sized buffers"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "resampler_sanitize")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "resampler_sanitize.cpp"),
                    os.path.join(root, "mercury_amd", "csrc", "resamp_tables.cpp"), os.path.join(root, "mercury_amd", "csrc", "chan_tables.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "resampler host side: clean" in out.stdout

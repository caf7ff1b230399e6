/* mercury_channelizer.h — a wideband channeliser: one SDR IQ stream into the S 48 kHz audio streams that mgpu_capture_* reads.
 *
 * mercury_capture.h takes S continuous 48 kHz captures ("radios on one sound clock"). A wideband SDR delivers one complex IQ stream around
 * a centre frequency instead, with many 3 kHz HF channels inside it. The channeliser is the piece in between: a frequency-translating FIR
 * decimator bank on the device. One IQ stream at R = 48000 * D goes in; S real upper- or lower-sideband audio streams come out in device
 * memory as [S][n_out], the layout mgpu_capture_feed / mgpu_capture_run read in place. The stream is fed in chunks and the result is bit
 * for bit the result of feeding it whole (as mgpu_hf_stream_*), and bit for bit the host twin's, mgpu_host_chan_process.
 *
 * The rule (normative; the twin implements exactly this).
 *   D = 1..64 decimation; channel s has offset_hz (dial frequency minus the stream's centre), sideband (0 USB, 1 LSB) and gain.
 *   a_c = audio_centre_hz, the centre of the audio band (1472: Mercury's audio is 300 .. 2643.75 Hz around carrier 1471.875 Hz).
 *   Prototype: a real symmetric low-pass h[0..T-1], T = tp * D + 1 with tp even, 2 <= tp <= 512; c = (T - 1) / 2; latency L = tp / 2 outputs.
 *   Refused (MGPU_ERR_ARG, before any device work): any other T; a channel whose band [offset, offset + 2 a_c] (USB) or
 *   [offset - 2 a_c, offset] (LSB) leaves (-R/2, R/2).
 *   Tables, made once on the host in double with the host's libm (the twin and the device read the same tables):
 *     sigma = +1 USB / -1 LSB, F = offset_hz + sigma * a_c;
 *     g_s[k] = h[k] * (cos phi, sin phi), phi = 2 pi q / R, q = (F * (k - c)) mod R (64-bit, floor-mod: q in [0, R));
 *     W[p] = (cos 2 pi p / 48000, sin 2 pi p / 48000), p < 48000.
 *   Input x[m]: the IQ sample widened exactly to double (CS16: / 32768.0); 0 before the stream's start or the last seek.
 *   Output n of channel s:
 *     re = im = +0.0
 *     for k = 0 .. T-1 ascending, v = x[n * D - k]:
 *         re = fma( g.re, v.re, re);  re = fma(-g.im, v.im, re)
 *         im = fma( g.re, v.im, im);  im = fma( g.im, v.re, im)
 *     p = (offset_hz * (n - L)) mod 48000                      (floor-mod, exact for negative offsets and n up to 2^62)
 *     y = gain * fma(im, W[p].im, re * W[p].re)                (= gain * Re{ z * conj(W[p]) })
 *   One accumulator per component, in this order, fused multiply-adds (on the host libm's fma(), correctly rounded on any x86-64).
 *   A call at output position n0 with n_in = N * D inputs produces outputs n0 .. n0 + N - 1 and advances the position by N; the last T - 1
 *   widened inputs stay on the device. Output n depends on n and the samples only, never on how the stream was cut.
 *
 * Errors as mercury_gpu.h. The context rules of INTEGRATION.md §2 apply: a channeliser belongs to its context, is used by one thread at a
 * time with it and is destroyed before it.
 */
#ifndef MERCURY_CHANNELIZER_H
#define MERCURY_CHANNELIZER_H

#include <stdint.h>

#include "mercury_capture.h"

#ifdef __cplusplus
extern "C" {
#endif

/* IQ formats: interleaved I, Q */
#define MGPU_IQ_CS16 0      /* int16 pairs, / 32768.0 */
#define MGPU_IQ_CF32 1      /* float pairs */
#define MGPU_IQ_CF64 2      /* double pairs */

#define MGPU_CHAN_MAX_D 64
#define MGPU_CHAN_MAX_TP 512
#define MGPU_CHAN_DEFAULT_TP 320
#define MGPU_CHAN_DEFAULT_AUDIO_CENTRE_HZ 1472
#define MGPU_CHAN_PHASOR_LEN 48000

typedef struct mgpu_chan mgpu_chan;

typedef struct mgpu_chan_channel {
    int offset_hz;      /* dial frequency minus the stream's centre frequency */
    int sideband;       /* 0 USB, 1 LSB */
    double gain;
} mgpu_chan_channel;

typedef struct mgpu_chan_config {
    int struct_size;        /* = sizeof(mgpu_chan_config), else MGPU_ERR_ARG (versioned by size, as mgpu_linksim_config) */
    int D;                  /* decimation 1..64: the input rate is 48000 * D */
    int S;                  /* channels, >= 1 */
    int audio_centre_hz;    /* a_c, 1..23999 (MGPU_CHAN_DEFAULT_AUDIO_CENTRE_HZ) */
    int ntaps;              /* T of `taps`; ignored when taps is NULL */
    const double* taps;     /* the prototype h[T]; NULL: the default design (mgpu_host_chan_default_taps) */
    int max_out;            /* outputs per channel that one call may produce; 0: 16 * 1088 */
} mgpu_chan_config;

/* channels: [S]. Without a context (no device could be opened) a valid configuration gives MGPU_ERR_DEVICE, a bad one MGPU_ERR_ARG. */
int mgpu_chan_create(mgpu_ctx* ctx, const mgpu_chan_config* config, const mgpu_chan_channel* channels, mgpu_chan** out);
int mgpu_chan_destroy(mgpu_chan* ch);
/* L in output samples; < 0 for a null handle */
int mgpu_chan_latency(mgpu_chan* ch);
/* the next output is `position`; the history becomes zeros */
int mgpu_chan_seek(mgpu_chan* ch, uint64_t position);
/* another frequency, sideband or gain for channel s from the next call on: rebuilds its tap row. Position and history are kept. */
int mgpu_chan_retune(mgpu_chan* ch, int s, const mgpu_chan_channel* channel);
/* n_in IQ samples (a positive multiple of D, at most max_out * D) in host or device memory (detected) -> out [S][n_in / D] host doubles.
 * Blocks. A bad n_in gives MGPU_ERR_ARG and changes nothing. */
int mgpu_chan_process(mgpu_chan* ch, const void* iq, int format, int n_in, double* out);
/* the same with device input and output, asynchronous on `stream` (a hipStream_t; NULL: the context's stream) */
int mgpu_chan_process_dev(mgpu_chan* ch, const void* d_iq, int format, int n_in, double* d_out, void* stream);

/* H hops for every capture from H * P * D IQ samples (host or device memory): mgpu_chan_process_dev into a workspace the channeliser
 * owns, then mgpu_capture_run on that workspace (MGPU_SAMPLES_F64, device memory). The S of both objects must agree, both must belong to
 * one context and H * P must not exceed max_out. events / payloads / max_events / n_events as mgpu_capture_run. */
int mgpu_capture_run_wideband(mgpu_capture* cap, mgpu_chan* ch, const void* iq, int format, int H, mgpu_capture_event* events,
                              uint8_t* payloads, int max_events, int* n_events);

/* Host only, no GPU needed.
 * mgpu_host_chan_design: a windowed-sinc low-pass of T = tp * D + 1 taps at rate 48000 * D, cutoff cutoff_hz, Kaiser window with
 *   beta = 0.1102 * (atten_db - 8.7), normalised to unit DC gain and symmetric to the bit. taps: [tp * D + 1]; *ntaps = T.
 * mgpu_host_chan_default_taps: tp = 320, cutoff 1500 Hz, 60 dB (<= 0.05 dB ripple to +-1200 Hz, <= -58 dB from +-1800 Hz on).
 * mgpu_host_chan_tables: g_out [T] complex (re, im) for one channel of `config` (S is not read); W_out NULL or [48000] complex.
 * mgpu_host_chan_process: the twin. A fresh channeliser seeked to `position` and fed the whole signal at once: out [S][n_in / D]. */
int mgpu_host_chan_design(int D, int tp, double cutoff_hz, double atten_db, double* taps, int* ntaps);
int mgpu_host_chan_default_taps(int D, double* taps, int* ntaps);
int mgpu_host_chan_tables(const mgpu_chan_config* config, const mgpu_chan_channel* channel, double* g_out, double* W_out);
int mgpu_host_chan_process(const mgpu_chan_config* config, const mgpu_chan_channel* channels, const void* iq, int format, int n_in,
                           uint64_t position, double* out);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_CHANNELIZER_H */

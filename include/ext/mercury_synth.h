/* mercury_synth.h — a wideband synthesiser: S transmit audio streams into one IQ stream, the mirror of mercury_channelizer.h.
 *
 * mgpu_transmit_byte_batch[_dev] produces S streams of 48 kHz passband audio. A gateway that listens to its HF channels through one
 * wideband SDR (mercury_channelizer.h) answers on them through the same SDR: the synthesiser is the piece in between, a
 * frequency-translating interpolating FIR bank on the device. S real audio streams [S][n_in] (doubles, rows in_stride apart, host or
 * device memory) go in; one complex IQ stream of n_in * D samples at R = 48000 * D comes out as CF64, CF32 or CS16 (MGPU_IQ_*). The
 * stream is fed in chunks and the result is bit for bit the result of feeding it whole, and bit for bit the host twin's,
 * mgpu_host_synth_process.
 *
 * The rule (normative; the twin implements exactly this).
 *   D = 1..64 interpolation; channel s is a mgpu_chan_channel: offset_hz (dial frequency minus the stream's centre), sideband (0 USB,
 *   1 LSB) and gain: one channel plan drives the channeliser and the synthesiser. a_c = audio_centre_hz (1472).
 *   Prototype: the channeliser's, a real symmetric low-pass h[0..T-1], T = tp * D + 1 with tp even, 2 <= tp <= 512; c = (T - 1) / 2.
 *   NULL: mgpu_host_chan_default_taps.
 *   Refused (MGPU_ERR_ARG, before any device work), as mgpu_chan_create refuses: any other T; a channel whose band [offset, offset + 2 a_c]
 *   (USB) or [offset - 2 a_c, offset] (LSB) leaves (-R/2, R/2).
 *   Tables, made once on the host in double with the host's libm (the twin and the device read the same tables):
 *     q+[k] = h[k] * (cos phi, sin phi), phi = 2 pi t / R, t = (a_c * (k - c)) mod R (64-bit, floor-mod: t in [0, R));
 *     q-[k] = (q+[k].re, -q+[k].im), the conjugate exactly. Channel s reads q+ (USB) or q- (LSB): the taps do not depend on offset_hz.
 *     P_s[r] = (cos, sin)(2 pi t / R), t = (offset_hz * r) mod R, r < D.
 *     W[p] = (cos, sin)(2 pi p / 48000), p < 48000: the channeliser's phasor table.
 *     G_s = (2.0 * D) * gain_s: 2 restores the one sideband kept of a real signal, D the interpolation loss.
 *   Input a_s[n]: audio sample n of stream s; 0 before the stream's start or the last seek.
 *   Output m = n * D + r (n the audio position, 64-bit; 0 <= r < D). For each channel s:
 *     vr = vi = +0.0
 *     for j = 0 .. J_r ascending (J_0 = tp, J_r = tp - 1 for r > 0), a = a_s[n - j], q = q[j * D + r]:
 *         vr = fma(q.re, a, vr);  vi = fma(q.im, a, vi)
 *     e = W[(offset_hz * n) mod 48000]                          (floor-mod, exact for negative offsets and n up to 2^62)
 *     E.re = fma(-e.im, P.im, e.re * P.re);   E.im = fma(e.im, P.re, e.re * P.im)        (P = P_s[r]: E = e P)
 *     z.re = G_s * fma(-vi, E.im, vr * E.re); z.im = G_s * fma(vi, E.re, vr * E.im)      (z = G v E)
 *   Every product written as a product is rounded on its own; nothing else is contracted.
 *   IQ[m].re and IQ[m].im start at +0.0 and the channels' z are added in ascending s with plain additions: one accumulator per channel,
 *   an ordered combine.
 *   Formats: CF64 as is; CF32 by round-to-nearest-even; CS16 as clamp(nearbyint(x * 32768), -32768, 32767) per component, every clamped
 *   component counted (a NaN component becomes 0 and is counted). Non-finite inputs go through the same chain with no special case.
 *   Latency: the band-pass is centred on c, so audio appears c IQ samples late, L = tp / 2 audio samples. The carrier phasor is NOT
 *   delayed: its phase at output m is offset_hz * m / R, not offset_hz * (m - c) / R. That is what makes synthesiser -> channeliser
 *   (the same D, plan and prototype) a pure delay of tp audio samples, because the channeliser removes its carrier at (n - L) D = n D - c.
 *   In the textbook form the rule is: zero-stuff a_s[n] e^(2 pi i offset n / 48000) to rate R, convolve with
 *   h[k] e^(2 pi i (offset k + sigma a_c (k - c)) / R), sigma = +1 USB / -1 LSB, scale by G_s and add the channels.
 *   Calls: the state is the position and the last tp audio samples of every channel. A call at audio position n0 with n_in samples per
 *   channel produces the outputs n0 D .. (n0 + n_in) D - 1 and advances the position by n_in. Output m depends on m and the samples
 *   only, never on how the stream was cut. Positions stay at or below 2^62.
 *
 * Errors as mercury_gpu.h. The context rules of INTEGRATION.md §2 apply: a synthesiser belongs to its context, is used by one thread at a
 * time with it and is destroyed before it.
 *
 * This header lives under include/ext/: the prototypes under include/ itself are a closed set.
 */
#ifndef MERCURY_SYNTH_H
#define MERCURY_SYNTH_H

#include <stddef.h>
#include <stdint.h>

#include "../mercury_channelizer.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgpu_synth mgpu_synth;

typedef struct mgpu_synth_config {
    int struct_size;        /* = sizeof(mgpu_synth_config), else MGPU_ERR_ARG (versioned by size, as mgpu_chan_config) */
    int D;                  /* interpolation 1..64: the output rate is 48000 * D */
    int S;                  /* channels, >= 1 */
    int audio_centre_hz;    /* a_c, 1..23999 (MGPU_CHAN_DEFAULT_AUDIO_CENTRE_HZ) */
    int ntaps;              /* T of `taps`; ignored when taps is NULL */
    const double* taps;     /* the prototype h[T]; NULL: the default design (mgpu_host_chan_default_taps) */
    int max_in;             /* audio samples per channel that one call may take; 0: 16 * 1088 */
} mgpu_synth_config;

typedef struct mgpu_synth_state {
    uint64_t position;      /* the next audio sample's position */
    uint64_t clamped;       /* CS16 components clamped since the last seek (or creation) */
    int D, S, tp, max_in;
    int tile;               /* audio positions that one workgroup of the kernel computes */
    int phases;             /* phases r of one position that one lane computes */
} mgpu_synth_state;

/* channels: [S]. Without a context (no device could be opened) a valid configuration gives MGPU_ERR_DEVICE, a bad one MGPU_ERR_ARG. */
int mgpu_synth_create(mgpu_ctx* ctx, const mgpu_synth_config* config, const mgpu_chan_channel* channels, mgpu_synth** out);
int mgpu_synth_destroy(mgpu_synth* sy);
/* L = tp / 2 in audio samples (L * D IQ samples); < 0 for a null handle */
int mgpu_synth_latency(mgpu_synth* sy);
/* the next audio sample is `position`; the history becomes zeros and the clamp count 0 */
int mgpu_synth_seek(mgpu_synth* sy, uint64_t position);
/* another frequency, sideband or gain for channel s from the next call on. Position and history are kept. */
int mgpu_synth_retune(mgpu_synth* sy, int s, const mgpu_chan_channel* channel);
/* n_in audio samples per channel (1..max_in), audio [S][in_stride] doubles (in_stride >= n_in) in host or device memory (detected) ->
 * n_in * D IQ samples in `format` (MGPU_IQ_*) to host memory. Blocks. A bad n_in gives MGPU_ERR_ARG and changes nothing. */
int mgpu_synth_process(mgpu_synth* sy, const double* audio, size_t in_stride, int n_in, int format, void* out);
/* the same with device input and output, asynchronous on `stream` (a hipStream_t; NULL: the context's stream) */
int mgpu_synth_process_dev(mgpu_synth* sy, const double* d_audio, size_t in_stride, int n_in, int format, void* d_out, void* stream);
/* waits for the device: the count includes every call issued so far */
int mgpu_synth_status(mgpu_synth* sy, mgpu_synth_state* state);

/* Host only, no GPU needed.
 * mgpu_host_synth_tables: for one channel of `config` (S is not read): q_out [T] complex (re, im), the tap table of the channel's
 *   sideband; P_out [D] complex; *G_out; W_out NULL or [48000] complex.
 * mgpu_host_synth_process: the twin. A fresh synthesiser seeked to `position` and fed the whole signal at once (max_in is not read):
 *   out n_in * D IQ samples in `format`; *clamped (NULL: not wanted) the CS16 components clamped. */
int mgpu_host_synth_tables(const mgpu_synth_config* config, const mgpu_chan_channel* channel, double* q_out, double* P_out, double* G_out,
                           double* W_out);
int mgpu_host_synth_process(const mgpu_synth_config* config, const mgpu_chan_channel* channels, const double* audio, size_t in_stride,
                            int n_in, uint64_t position, int format, void* out, uint64_t* clamped);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_SYNTH_H */

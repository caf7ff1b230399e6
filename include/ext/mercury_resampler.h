/* mercury_resampler.h — a rational resampler: audio or IQ at any integer sample rate into the rate a receive entry point takes.
 *
 * mercury_capture.h takes 48 000 Hz audio and mercury_channelizer.h IQ at exactly 48000 * D. A sound card at 44 100 Hz, a 12 kHz network
 * receiver, an 8 kHz codec or an SDR at 2.048 MS/s deliver neither. The resampler is the piece in front: a polyphase FIR interpolator /
 * decimator on the device. S streams at fin go in, in chunks of any length; S streams at fout come out, bit for bit what feeding the
 * stream whole gives, and bit for bit the host twin's, mgpu_host_resamp_process. This is NOT one of the reference's configurations: the
 * reference opens its sound card at 48 000 Hz.
 *
 * The rule (normative; the twin implements exactly this).
 *   fin, fout positive integer rates in Hz; g = gcd(fin, fout), L = fout / g, M = fin / g; S >= 1 streams of C components per sample
 *   (1: real audio, 2: interleaved I, Q). Every component of every stream is filtered alike and independently.
 *   Refused (MGPU_ERR_ARG, before any device work): L > 640, M > 640, M > 16 L, tp odd or outside 2..512, C not 1 or 2,
 *   ntaps != tp * L + 1, a format that does not fit C (C = 1: MGPU_SAMPLES_*, C = 2: MGPU_IQ_*).
 *   Prototype: a real symmetric low-pass h[0 .. tp * L] at rate fin * L, tp even; its centre is c = tp * L / 2 and the delay is exactly
 *   tp / 2 input samples.
 *   Input x[m]: sample m of a stream widened exactly to double, real formats as mercury_capture.h widens MGPU_SAMPLES_* (INT32
 *   / 2147483647.0, INT16 / 32768.0), IQ formats as mercury_channelizer.h widens MGPU_IQ_* (CS16 / 32768.0); 0 before the stream's start or
 *   the last seek.
 *   Output n (absolute, 64-bit), per stream and component:
 *     q = n * M;  b = q div L;  rho = q mod L;  acc = +0.0
 *     for j = 0 .. tp-1 ascending:   acc = fma(h[rho + j * L], x[b - j], acc)
 *     if rho == 0:                   acc = fma(h[tp * L],      x[b - tp], acc)
 *     y[n] = acc
 *   One accumulator, in this order, fused multiply-adds (on the host libm's fma(), correctly rounded on any x86-64). Non-finite inputs go
 *   through the same chain with no special case. Output n stands for input time n * M / L - tp / 2.
 *   Calls: the state is the input position m0, the output position n0 and the last tp widened inputs. A call with n_in >= 1 inputs (at
 *   most max_in) produces the outputs n0 .. n1 - 1 with n1 = ceil((m0 + n_in) * L / M), possibly none, and returns their count. Output n
 *   depends on n and the samples only, never on how the stream was cut. A seek to input position m sets m0 = m, n0 = ceil(m * L / M)
 *   and zeroes the history. Positions stay below 2^52.
 *   Default design (mgpu_host_resamp_design): a windowed sinc at rate fin * L, Kaiser window with beta = 0.1102 * (atten_db - 8.7),
 *   symmetric to the bit, normalised to sum h = L; tp = 32 * max(1, ceil(M / L)), cutoff 0.45 * min(fin, fout), 60 dB. The construction
 *   of mgpu_host_chan_design. The default tp is raised to the least even tp at which 1.5 w fits between that cutoff and fin * L / 2, with
 *   w = (60 - 7.95) * fin / (14.36 * tp) the transition width of Kaiser's design formula (half the transition and a stop-band one w
 *   wide below the design rate's Nyquist frequency). Of all accepted ratios this moves 1/1 alone: tp = 110, where 33 taps would leave
 *   no stop-band and a pass-band deviation of -57.4 dB. A tp that is given is taken as it is.
 *
 * Errors as mercury_gpu.h. The context rules of INTEGRATION.md §2 apply: a resampler belongs to its context, is used by one thread at a
 * time with it and is destroyed before it.
 *
 * This header lives under include/ext/: the prototypes under include/ itself are a closed set.
 */
#ifndef MERCURY_RESAMPLER_H
#define MERCURY_RESAMPLER_H

#include <stddef.h>
#include <stdint.h>

#include "../mercury_capture.h"
#include "../mercury_channelizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGPU_RESAMP_MAX_L 640
#define MGPU_RESAMP_MAX_M 640
#define MGPU_RESAMP_MAX_RATIO 16      /* M <= 16 L */
#define MGPU_RESAMP_MAX_TP 512
#define MGPU_RESAMP_MAX_POSITION (1ULL << 52)

typedef struct mgpu_resamp mgpu_resamp;

typedef struct mgpu_resamp_config {
    int struct_size;        /* = sizeof(mgpu_resamp_config), else MGPU_ERR_ARG (versioned by size, as mgpu_chan_config) */
    int fin, fout;          /* rates in Hz, >= 1 */
    int S;                  /* streams, >= 1 */
    int components;         /* C: 1 real, 2 interleaved I, Q */
    int tp;                 /* taps per phase, even, 2..512; 0 with taps NULL: the default design's (32 * max(1, ceil(M / L)); 110 at 1/1) */
    int ntaps;              /* tp * L + 1 of `taps`; ignored when taps is NULL */
    const double* taps;     /* the prototype h[tp * L + 1], finite; NULL: the default design at tp */
    int max_in;             /* inputs per stream that one call may take; 0: those of 16 * 1088 outputs, ceil(17408 * M / L) */
} mgpu_resamp_config;

typedef struct mgpu_resamp_status {
    int L, M, tp;
    int S, components;
    int max_in, max_out;    /* max_out: the most outputs per stream one call of max_in inputs can produce */
    int tile;               /* outputs of one stream that one workgroup of the kernel computes */
    int fifo;               /* outputs per stream waiting in the FIFO of mgpu_capture_run_resampled */
    int pad;
    double delay;           /* tp / 2 input samples in output samples: tp * L / (2 M) */
    uint64_t m0, n0;        /* the next input's and the next output's position */
} mgpu_resamp_status;

/* Without a context (no device could be opened) a valid configuration gives MGPU_ERR_DEVICE, a bad one MGPU_ERR_ARG. */
int mgpu_resamp_create(mgpu_ctx* ctx, const mgpu_resamp_config* config, mgpu_resamp** out);
int mgpu_resamp_destroy(mgpu_resamp* rs);
int mgpu_resamp_info(mgpu_resamp* rs, mgpu_resamp_status* status);
/* the next input is `position` (below 2^52); the history becomes zeros and the FIFO of mgpu_capture_run_resampled empty */
int mgpu_resamp_seek(mgpu_resamp* rs, uint64_t position);
/* n_in samples per stream (1..max_in), [S][n_in * C] in `format` in host or device memory (detected) -> *n_out outputs per stream as host
 * doubles out [S][out_stride * C]. Blocks. A bad argument (out_stride < *n_out included) gives MGPU_ERR_ARG and changes nothing. */
int mgpu_resamp_process(mgpu_resamp* rs, const void* in, int format, int n_in, double* out, size_t out_stride, int* n_out);
/* the same with device input and output, asynchronous on `stream` (a hipStream_t; NULL: the context's stream). *n_out is arithmetic
 * (mgpu_host_resamp_count) and written before the kernel is launched. */
int mgpu_resamp_process_dev(mgpu_resamp* rs, const void* d_in, int format, int n_in, double* d_out, size_t out_stride, int* n_out, void* stream);

/* The receive loop on audio at fin: n_in samples per capture ([S][n_in] in an MGPU_SAMPLES_* format, host or device memory) are resampled
 * into a device FIFO the resampler owns, and as many whole hops as the FIFO then holds, H = floor(available / P), go through
 * mgpu_capture_run; the remainder stays for the next call. Requires C = 1, fout = 48000, the S of both objects equal and both on one
 * context, else MGPU_ERR_ARG. events / payloads / max_events / n_events as mgpu_capture_run; event hop numbers count from the call's first
 * hop. *hops_run = H (0 is possible: then *n_events = 0). An error of the capture run itself leaves the resampler advanced. */
int mgpu_capture_run_resampled(mgpu_capture* cap, mgpu_resamp* rs, const void* samples, int format, int n_in, mgpu_capture_event* events,
                               uint8_t* payloads, int max_events, int* n_events, int* hops_run);

/* Host only, no GPU needed.
 * mgpu_host_resamp_design: the design above. tp 0, cutoff_hz 0 and atten_db 0 stand for the defaults; else tp even 2..512,
 *   0 < cutoff_hz < fin * L / 2, 0 < atten_db <= 200. taps: [tp * L + 1]; *ntaps = tp * L + 1 (taps may be NULL to ask for *ntaps only).
 * mgpu_host_resamp_default_taps: the design with every default.
 * mgpu_host_resamp_process: the twin. A fresh resampler seeked to input position `position` and fed the whole signal at once:
 *   in [S][n_in * C], out [S][out_stride * C], *n_out outputs per stream (max_in is not read).
 * mgpu_host_resamp_count: *n_out = ceil((m0 + n_in) * L / M) - ceil(m0 * L / M) for n_in >= 0. */
int mgpu_host_resamp_design(int fin, int fout, int tp, double cutoff_hz, double atten_db, double* taps, int* ntaps);
int mgpu_host_resamp_default_taps(int fin, int fout, double* taps, int* ntaps);
int mgpu_host_resamp_process(const mgpu_resamp_config* config, const void* in, int format, int n_in, uint64_t position, double* out,
                             size_t out_stride, int* n_out);
int mgpu_host_resamp_count(int fin, int fout, uint64_t m0, int n_in, int* n_out);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_RESAMPLER_H */

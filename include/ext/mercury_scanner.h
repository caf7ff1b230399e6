/* mercury_scanner.h — a band scanner: one wideband IQ stream into spectrum lines and, per line, the occupied stretches of the band.
 *
 * The channeliser, the synthesiser and the capture loop all take a channel plan (mgpu_chan_channel[S]) as given. The scanner is the piece
 * that looks at the wideband stream and says where the stations are: a Welch spectrum line of N bins per A blocks of the stream (a
 * spectrum or waterfall line per fraction of a second), the line's median level, and the runs of bins that stand above it, each of which
 * mgpu_host_scan_plan turns into a mgpu_chan_channel. The stream is fed in chunks and the result is bit for bit the result of feeding it
 * whole, and bit for bit the host twin's, mgpu_host_scan_process. This is NOT one of the reference's configurations.
 *
 * The rule (normative; the twin implements exactly this).
 *   Configuration: D = 1..64, the rate is R = 48000 * D and enters only the mapping to Hz; log2n = 8..12, N = 2^log2n, H = N / 2, one bin
 *   is R / N Hz; A = blocks_per_line = 1..4096; threshold finite and >= 2; edge_bins = 0..N/4; dc_bins = 0..16; gap = 0..64;
 *   min_bins = 1..N; max_runs = 1..MGPU_SCAN_MAX_RUNS; max_in a multiple of H (0: 256 * H). Anything else is refused with MGPU_ERR_ARG
 *   before any device work.
 *   Tables, made once on the host with the host's libm (the twin and the device read the same tables):
 *     tab[j] = {cos a, sin a}, a = 2.0 * M_PI * double(j) / double(N), j < N;   win[i] = sin(M_PI * double(i) / double(N)), i < N.
 *   Input x[m]: the IQ sample widened exactly to double as the channeliser does it (CS16: / 32768.0); {+0.0, +0.0} before the stream's
 *   start or the last seek.
 *   Blocks: block b (b >= 0, 64-bit) covers the samples (b - 1) * H .. (b + 1) * H - 1; v[i] = {x.re * win[i], x.im * win[i]}.
 *   Transform: the excisor's (mercury_excisor.h) at N points with complex input: a[brev(i)] = v[i]; for size = 2, 4, .. N, half = size / 2,
 *     step = N / size, per group start g and j < half: w = {tab[j * step].re, -tab[j * step].im}, lo = a[g + j], hi = a[g + j + half],
 *     t = {w.re * hi.re - w.im * hi.im, w.re * hi.im + w.im * hi.re}, a[g + j] = lo + t, a[g + j + half] = lo - t. Every product, sum and
 *     difference is rounded on its own, no contraction. The device schedules the network as it likes; the values are the butterflies'.
 *   Power: P_b[k] = re * re + im * im (three roundings). Bins are in ascending frequency: f = (k + N / 2) mod N lies at
 *     (f - N / 2) * R / N Hz.
 *   Lines: line l is L[f] = the sum of P_b[f] over b = l * A .. l * A + A - 1, from +0.0, in ascending b, with plain additions. A call at
 *     position j * H with n_in = m * H samples (m >= 1, n_in <= max_in) completes the blocks j .. j + m - 1 and emits
 *     floor((j + m) / A) - floor(j / A) lines. The stage carries the last H widened samples and the partial line between calls;
 *     mgpu_scan_seek takes a multiple of H * A only and clears both. A line depends on its blocks' samples only, never on how the stream
 *     was cut. Positions stay at or below 2^62.
 *   Level: the usable bins are those with edge_bins <= f <= N - 1 - edge_bins and |f - N / 2| > dc_bins (dc_bins = 0 excludes nothing).
 *     If a usable L[f] is not finite the line reports nonfinite = 1, level = +0.0, n_runs = 0 (where a bin is NaN, which NaN, its sign and
 *     payload, is the processor's choice and not part of the rule). Otherwise level is the usable L whose key
 *     has rank U / 2 (0-based, ascending) among the U usable ones, the key being the bit pattern without the sign, compared as an unsigned
 *     integer: a selection as in mercury_blanker.h, never an average.
 *   Occupancy: occ[f] = !(L[f] <= threshold * level) on usable bins, 0 elsewhere. Then every maximal stretch of unoccupied usable bins of
 *     length <= gap with an occupied bin directly on both sides becomes occupied. An excluded bin never does: no run spans DC or an edge.
 *   Runs: the maximal occupied stretches of length >= min_bins, in ascending f. n_runs counts them all; the first max_runs are reported,
 *     each as {first, count, peak, power}: peak the first f of the greatest L[f] of the run under `>`, power the sum of L[f] over the
 *     run from +0.0, ascending.
 *
 * The default threshold is measured, not chosen: over 2048 lines of white Gaussian noise at the default N = 4096 and A = 16 the highest
 * usable-bin-to-level ratio the twin saw was 3.3177 (profiles/scanner.md); times 1.5 is 4.98, rounded up: 5.
 *
 * Limits: the detection is static per line; nothing is tracked from line to line; the stage does not classify a signal (a run is a
 * stretch of power above the median, whatever sends it); the offset mgpu_host_scan_plan gives is good to about one bin, R / N Hz.
 * mgpu_pool_* does not forward the stage.
 *
 * Errors as mercury_gpu.h. The context rules of INTEGRATION.md §2 apply: a scanner belongs to its context, is used by one thread at a time
 * with it and is destroyed before it.
 *
 * This header lives under include/ext/: the prototypes under include/ itself are a closed set.
 */
#ifndef MERCURY_SCANNER_H
#define MERCURY_SCANNER_H

#include <stddef.h>
#include <stdint.h>

#include "../mercury_channelizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGPU_SCAN_MAX_RUNS 32
#define MGPU_SCAN_MIN_LOG2N 8
#define MGPU_SCAN_MAX_LOG2N 12
#define MGPU_SCAN_DEFAULT_LOG2N 12
#define MGPU_SCAN_DEFAULT_BLOCKS_PER_LINE 16
#define MGPU_SCAN_DEFAULT_THRESHOLD 5.0

typedef struct mgpu_scan mgpu_scan;

typedef struct mgpu_scan_config {
    int struct_size;        /* = sizeof(mgpu_scan_config), else MGPU_ERR_ARG (versioned by size, as mgpu_chan_config) */
    int D;                  /* 1..64: the rate is 48000 * D */
    int log2n;              /* 8..12: N = 2^log2n bins, H = N / 2 */
    int blocks_per_line;    /* A, 1..4096 */
    double threshold;       /* finite, >= 2 (MGPU_SCAN_DEFAULT_THRESHOLD) */
    int edge_bins;          /* 0..N/4 bins excluded at each edge of the span */
    int dc_bins;            /* 0..16 bins excluded on either side of DC, with DC; 0 excludes nothing */
    int gap;                /* 0..64: the longest unoccupied stretch that is closed */
    int min_bins;           /* 1..N: the shortest run that is kept */
    int max_runs;           /* 1..MGPU_SCAN_MAX_RUNS runs reported per line */
    int max_in;             /* IQ samples that one call may take, a multiple of H; 0: 256 * H */
} mgpu_scan_config;

typedef struct mgpu_scan_run {
    int first;              /* the run's first bin f */
    int count;              /* its bins */
    int peak;               /* the bin of its greatest L[f] */
    int pad;
    double power;           /* the sum of its L[f] */
} mgpu_scan_run;

typedef struct mgpu_scan_report {
    uint64_t first_block;   /* the line's first block, l * A */
    double level;           /* the median of the usable bins (+0.0 with nonfinite) */
    int n_runs;             /* all the runs of the line */
    int reported;           /* min(n_runs, max_runs): the entries of runs[] that are set; the others are zeros */
    int nonfinite;          /* 1: a usable bin's sum was not finite */
    int pad;
    mgpu_scan_run runs[MGPU_SCAN_MAX_RUNS];
} mgpu_scan_report;

typedef struct mgpu_scan_state {
    uint64_t position;      /* the next IQ sample's position */
    uint64_t blocks;        /* position / H: the next block */
    uint64_t lines;         /* blocks / A: the next line */
    int D, log2n, blocks_per_line, max_in;
} mgpu_scan_state;

/* Without a context (no device could be opened) a valid configuration gives MGPU_ERR_DEVICE, a bad one MGPU_ERR_ARG. */
int mgpu_scan_create(mgpu_ctx* ctx, const mgpu_scan_config* config, mgpu_scan** out);
int mgpu_scan_destroy(mgpu_scan* sc);
/* the next IQ sample is `position`, a multiple of H * A; the history and the partial line become zeros */
int mgpu_scan_seek(mgpu_scan* sc, uint64_t position);
/* the lines that the next call of n_in samples completes: pure arithmetic; < 0 for a null handle or a bad n_in */
int mgpu_scan_lines(mgpu_scan* sc, int n_in);
/* n_in IQ samples (a positive multiple of H, at most max_in) in `format` (MGPU_IQ_*) in host or device memory (detected) -> the completed
 * lines [n][N] doubles and their reports [n] in host memory, n = mgpu_scan_lines(sc, n_in) into *n_lines (NULL: not wanted). Blocks. A bad
 * n_in gives MGPU_ERR_ARG and changes nothing. */
int mgpu_scan_process(mgpu_scan* sc, const void* iq, int format, int n_in, double* lines, mgpu_scan_report* reports, int* n_lines);
/* the same with device input and output, asynchronous on `stream` (a hipStream_t; NULL: the context's stream) */
int mgpu_scan_process_dev(mgpu_scan* sc, const void* d_iq, int format, int n_in, double* d_lines, mgpu_scan_report* d_reports, int* n_lines,
                          void* stream);
int mgpu_scan_status(mgpu_scan* sc, mgpu_scan_state* state);

/* Host only, no GPU needed.
 * mgpu_host_scan_process: the twin. A fresh scanner seeked to `position` and fed the whole signal at once (max_in is checked and not read otherwise): lines
 *   [n][N], reports [n], *n_lines = n = floor((position + n_in) / (H A)) - position / (H A).
 * mgpu_host_scan_plan: one run of a report as a channel of gain 1.0 for `sideband` (0 USB, 1 LSB) and audio centre a_c:
 *   centre = ((first + (count - 1) / 2.0) - N / 2) * R / N, offset_hz = lround(centre - sigma * a_c), sigma = +1 USB / -1 LSB. Refused
 *   (MGPU_ERR_ARG) as mgpu_chan_create refuses the channel: a band that leaves (-R/2, R/2). */
int mgpu_host_scan_process(const mgpu_scan_config* config, const void* iq, int format, int n_in, uint64_t position, double* lines,
                           mgpu_scan_report* reports, int* n_lines);
int mgpu_host_scan_plan(const mgpu_scan_config* config, const mgpu_scan_run* run, int sideband, int audio_centre_hz,
                        mgpu_chan_channel* channel);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_SCANNER_H */

/* mercury_wideband_blanker.h — a wideband impulse blanker: the IQ stream at 48000 * D with its clicks replaced by zero, ahead of the bank.
 *
 * A power-line or ignition click is one or two samples long at the wideband rate. Behind the channeliser's prototype it rings over tp
 * audio samples at about 1/D-th of its height, and the per-frame blanker of mercury_blanker.h, which works on 12 kHz baseband frames,
 * cannot see it any more. This stage stands where every SDR receiver has its noise blanker: in the wide IF, ahead of the narrow filters.
 * IQ goes in as CS16, CF32 or CF64; the same stream comes out in the same format, delayed by exactly one block, with the samples the
 * rule marks replaced by zero and every other sample byte for byte. The output feeds mgpu_chan_process[_dev],
 * mgpu_capture_run_wideband, mgpu_scan_process[_dev] and mgpu_tune_process, which all detect device memory. The stream is fed in chunks
 * and the result is byte for byte the result of feeding it whole, and byte for byte the host twin's, mgpu_host_wblank_process. This is
 * NOT one of the reference's configurations.
 *
 * The rule (normative; the twin implements exactly this).
 *   Configuration: D = 1..64 (enters only the default block length and what the delay is in audio samples); format one of MGPU_IQ_*,
 *   fixed for the handle's life; block B a multiple of 64, 64..4096 (0: the least multiple of 64 * D that is >= 256: a whole number of
 *   audio samples at every D, 4096 at D = 64); threshold finite and >= 2; guard = 0..64; max_share in (0, 0.5],
 *   cap = floor(max_share * B), computed once on the host in double; max_in a multiple of B (0: 1024 * B), 2^26 at most. Anything else,
 *   NaN included, is refused with MGPU_ERR_ARG before any device work, with or without a context.
 *   Input x[i]: the IQ sample widened exactly to double as the channeliser does it (CS16: / 32768.0).
 *   Power: p[i] = re * re + im * im: each product is rounded on its own, then the sum, no contraction.
 *   Blocks: block b (64-bit) covers the samples b * B .. b * B + B - 1 of the stream.
 *   Level: med_b is the p of the block whose key has rank B / 2 (0-based, ascending), the key being the 64-bit pattern with the sign bit
 *     cleared, compared as an unsigned integer, exactly as in mercury_blanker.h: a selection, never an average.
 *   Exceed: limit = threshold * med_b, one multiplication; sample i exceeds when !(p[i] <= limit).
 *   Cap: E_b is the number of exceeding samples of the block. If E_b > cap the block is capped: none of its samples exceeds. Such a block
 *     is a station keying up, a fade edge or garbage, not a click. The decision rests on the block's own samples only.
 *   Guard: sample i is marked when any sample j with |i - j| <= guard exceeds. This runs over the stream and across block borders.
 *     Nothing exceeds before the stream's start or the last seek.
 *   Output: y[i] is x[i]'s original bytes where i is not marked, and the format's zero where it is: +0.0 pairs or integer 0 pairs. An
 *     unmarked -0.0 stays -0.0.
 *   Delay: the marks of block b need block b + 1, so the stage delays by one block: a call at position j * B with n_in = m * B samples
 *     writes n_in output samples, the blocks j - 1 .. j + m - 2 of y; out[n] = y[n - B]. The block before the start, or before the last
 *     seek, is all zero bytes. Output n depends on n and on the samples only, never on how the stream was cut into calls. Positions stay
 *     at or below 2^62. mgpu_wblank_seek takes a multiple of B and clears the held block and its flags. The last block of a stream comes
 *     out when B more samples, zeros for instance, are fed.
 *   Reports: one mgpu_wblank_report per emitted block: the input block it describes (position / B - 1 for the first block of a fresh or
 *     seeked stream, whose other fields are zero), level = med_b, exceeding = E_b before the cap, blanked = the samples of the block that
 *     became zero, guard included, and capped.
 *   NaN and zero levels need no rule of their own: a NaN sample exceeds; a block whose median is NaN exceeds everywhere, is capped and
 *   passes byte for byte; a block of silence has limit 0 and is capped, unless at most cap samples are non-zero: those are clicks in
 *   silence and go. (Which NaN a NaN power is, its sign and payload, is the processor's choice; the level of a block whose median is NaN
 *   is that NaN without its sign.)
 *
 * The default threshold is measured, not chosen: over 2^22 samples of white Gaussian CF64 noise at the default block of D = 1, 4 and 64
 * (B = 256, 256, 4096) the highest p / med_b the twin saw was 22.49, 25.05 and 20.96 (profiles/wideband_blanker.md); the greatest times
 * 1.5 is 37.58, rounded up: 38. The median of 64 samples is noisier: on the same three inputs B = 64 saw 35.46, 32.53 and 26.52. B = 64
 * needs a higher threshold (by the same recipe, 54), and the default block never goes below 256 for that reason.
 *
 * Limits: the stage delays by one block and the stream's last block needs a flush of B samples; there is no clipping mode (a marked
 * sample becomes zero, never a limited value); a click longer than cap samples passes; a capped block is not blanked at all; the level is
 * per block, so a click train denser than max_share wins; whether the blanker helps under fading is unmeasured. mgpu_pool_* does not
 * forward the stage.
 *
 * Errors as mercury_gpu.h. The context rules of INTEGRATION.md §2 apply: a blanker belongs to its context, is used by one thread at a time
 * with it and is destroyed before it.
 *
 * This header lives under include/ext/: the prototypes under include/ itself are a closed set.
 */
#ifndef MERCURY_WIDEBAND_BLANKER_H
#define MERCURY_WIDEBAND_BLANKER_H

#include <stddef.h>
#include <stdint.h>

#include "../mercury_channelizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGPU_WBLANK_MIN_BLOCK 64
#define MGPU_WBLANK_MAX_BLOCK 4096
#define MGPU_WBLANK_MAX_GUARD 64
#define MGPU_WBLANK_DEFAULT_THRESHOLD 38.0
#define MGPU_WBLANK_DEFAULT_GUARD 4
#define MGPU_WBLANK_DEFAULT_MAX_SHARE 0.125

typedef struct mgpu_wblank mgpu_wblank;

typedef struct mgpu_wblank_config {
    int struct_size;        /* = sizeof(mgpu_wblank_config), else MGPU_ERR_ARG (versioned by size, as mgpu_scan_config) */
    int D;                  /* 1..64: the rate is 48000 * D */
    int format;             /* MGPU_IQ_*: the format of the input and of the output */
    int block;              /* B: a multiple of 64, 64..4096; 0: the least multiple of 64 * D that is >= 256 */
    double threshold;       /* finite, >= 2 (MGPU_WBLANK_DEFAULT_THRESHOLD) */
    double max_share;       /* (0, 0.5] (MGPU_WBLANK_DEFAULT_MAX_SHARE): cap = floor(max_share * B) */
    int guard;              /* 0..64 (MGPU_WBLANK_DEFAULT_GUARD) */
    int max_in;             /* IQ samples that one call may take, a multiple of B; 0: 1024 * B */
} mgpu_wblank_config;

typedef struct mgpu_wblank_report {
    int64_t block;          /* the input block the report describes */
    double level;           /* med_b */
    int exceeding;          /* E_b, before the cap */
    int blanked;            /* the samples of the block that became zero, guard included */
    int capped;             /* 1: E_b > cap, none of the block's samples exceeds */
    int pad;
} mgpu_wblank_report;

typedef struct mgpu_wblank_state {
    uint64_t position;      /* the next IQ sample's position */
    uint64_t blocks;        /* position / B: the next input block */
    int D, block, cap, max_in, format;
    int delay;              /* B: out[n] = y[n - delay] */
} mgpu_wblank_state;

/* Without a context (no device could be opened) a valid configuration gives MGPU_ERR_DEVICE, a bad one MGPU_ERR_ARG. */
int mgpu_wblank_create(mgpu_ctx* ctx, const mgpu_wblank_config* config, mgpu_wblank** out);
int mgpu_wblank_destroy(mgpu_wblank* wb);
/* the next IQ sample is `position`, a multiple of B; the held block becomes zeros and nothing of it exceeds */
int mgpu_wblank_seek(mgpu_wblank* wb, uint64_t position);
int mgpu_wblank_status(mgpu_wblank* wb, mgpu_wblank_state* state);
/* n_in IQ samples (a positive multiple of B, at most max_in) in the handle's format in host or device memory (detected) -> n_in output
 * samples in the same format and n_in / B reports (NULL: not wanted) in host memory; *n_reports = n_in / B (NULL: not wanted). Blocks.
 * A bad n_in gives MGPU_ERR_ARG and changes nothing. */
int mgpu_wblank_process(mgpu_wblank* wb, const void* iq, int n_in, void* out, mgpu_wblank_report* reports, int* n_reports);
/* the same with device input and output, asynchronous on `stream` (a hipStream_t; NULL: the context's stream). d_out must not overlap
 * d_iq; d_reports may be NULL. */
int mgpu_wblank_process_dev(mgpu_wblank* wb, const void* d_iq, int n_in, void* d_out, mgpu_wblank_report* d_reports, int* n_reports,
                            void* stream);

/* Host only, no GPU needed: the twin. A fresh stage seeked to `position` and fed the whole signal at once (max_in is checked and not
 * read otherwise): out [n_in] samples in config->format, reports [n_in / B] (NULL: not wanted), *n_reports = n_in / B. */
int mgpu_host_wblank_process(const mgpu_wblank_config* config, const void* iq, int n_in, uint64_t position, void* out,
                             mgpu_wblank_report* reports, int* n_reports);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_WIDEBAND_BLANKER_H */

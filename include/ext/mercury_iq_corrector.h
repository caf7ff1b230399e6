/* mercury_iq_corrector.h — an IQ corrector: the DC offset and the IQ imbalance of a quadrature front end taken out of the wide IF.
 *
 * A sound-card quadrature mixer or a direct-conversion SDR adds a DC offset to I and to Q, gives Q a slightly different gain and an
 * angle to I that is not quite 90 degrees. The offset is a carrier at 0 Hz; the imbalance mirrors every station at +f onto -f, 20 to 30
 * dB down, spectrum reversed (gain 1.1 and 5 degrees: 23.8 dB). Behind the channeliser the image and its victim are the same audio band,
 * so this is corrected here, in the wide IF, next to the noise blanker: corrector, then mgpu_wblank_*, then the bank. IQ goes in as CS16,
 * CF32 or CF64 at 48000 * D and comes out in the same format with no delay. The output feeds mgpu_wblank_process[_dev],
 * mgpu_chan_process[_dev], mgpu_capture_run_wideband, mgpu_scan_process[_dev] and mgpu_tune_process as it is. The stream is fed in chunks
 * of whole blocks and the result is byte for byte the result of feeding it whole, and byte for byte the host twin's,
 * mgpu_host_iqc_process. This is NOT one of the reference's configurations.
 *
 * The rule (normative; the twin implements exactly this).
 *   Configuration: D = 1..64; format one of MGPU_IQ_*, fixed for the handle's life; block B a multiple of 256, 256..4096 (0: 4096);
 *   memory M in blocks, 0 or 2..2^20: lambda = 1 - 1 / M, computed once on the host in double (0: lambda = 1, which never forgets;
 *   MGPU_IQC_DEFAULT_MEMORY = 1024); dc and balance each 0 or 1; fixed 0 or 1, and with fixed = 1 the four calibrated coefficients
 *   fixed_dc_re, fixed_dc_im, fixed_skew, fixed_gain, all finite, |skew| <= MGPU_IQC_MAX_SKEW = 0.5, gain in [1 / MGPU_IQC_MAX_GAIN,
 *   MGPU_IQC_MAX_GAIN] = [0.5, 2] (with fixed = 0 they are not read); max_in a multiple of B (0: 1024 * B), 2^26 at most. Anything else,
 *   NaN included, is refused with MGPU_ERR_ARG before any device work, with or without a context.
 *   Input x[i]: widened exactly to double as the channeliser does it (CS16: / 32768.0); I = re, Q = im.
 *   Block sums: block b (64-bit) covers the samples b * B .. b * B + B - 1 of the stream. The five terms of a sample are I, Q, I * I,
 *     I * Q, Q * Q; each product is rounded on its own, nothing is contracted. For each term there are 256 partial sums: partial l adds
 *     the terms of the samples l, l + 256, l + 512, ... of the block in ascending order, starting from the first term (not from zero).
 *     The partials are folded: for s = 128, 64, 32, 16, 8, 4, 2, 1: p[l] += p[l + s] for l < s. S_b is p[0] of each of the five terms.
 *   Skipped block: a block any of whose five sums is not finite is skipped (MGPU_IQC_SKIPPED): it leaves the state as it was, with no
 *     decay. Its samples are still corrected, with the standing estimate: the one the unchanged state gives.
 *   State: T = (T_I, T_Q, T_II, T_IQ, T_QQ, N), six doubles, zero at creation and after a seek. For every block that is not skipped,
 *     in ascending b: T <- lambda * T + S_b and N <- lambda * N + B, the product rounded, then the sum; with lambda = 1 the
 *     multiplication is still performed. This recursion is the stage's entire memory: how the stream is cut into calls changes nothing.
 *   Estimate for block b, from T after block b (included or skipped), with +, -, *, / and sqrt only, each IEEE correctly rounded:
 *     N = 0: identity (dc 0, skew 0, gain 1) and MGPU_IQC_NO_BALANCE. Otherwise mI = T_I / N, mQ = T_Q / N, cII = T_II / N - mI * mI,
 *     cQQ = T_QQ / N - mQ * mQ, cIQ = T_IQ / N - mI * mQ, skew = cIQ / cII, r = cQQ / cII - skew * skew, gain = 1 / sqrt(r). The balance
 *     is valid when cII > 0, r > 0, skew and gain are finite, |skew| <= 0.5 and 0.5 <= gain <= 2; otherwise skew = 0, gain = 1 and the
 *     block's report carries MGPU_IQC_NO_BALANCE. dc = 0 sets mI = mQ = 0 in the correction (the moments still use the measured means);
 *     balance = 0 sets skew = 0 and gain = 1 (the flag still says whether the measured balance was valid). In fixed mode no sums are
 *     formed, the state stays zero, the four configured values are used for every block (dc = 0 and balance = 0 apply to them as well)
 *     and no flag is set.
 *   Correction (Gram-Schmidt: Q made orthogonal to I and given I's power): yI = I - mI; yQ = gain * ((Q - mQ) - skew * yI); every
 *     operation rounded on its own. A component that is NaN leaves as the positive quiet NaN without payload (0x7FF8000000000000):
 *     which NaN an operation on a NaN gives is the processor's choice, and the output is not.
 *   Output: CF64 as it is; CF32 rounded to nearest even; CS16 clamp(nearbyint(y * 32768), -32768, 32767) per component, the
 *     synthesiser's rule (a NaN becomes 0 and counts as clamped). Clamped components are counted per block.
 *   Reports: one mgpu_iqc_report per block: the block, the four values used, the flags and the clamped components.
 *
 * Limits: the estimate assumes a proper (circular) signal. A band of stations at their own offsets is one; a single real-valued signal
 * centred on 0 Hz is not, and is taken for imbalance. The imbalance is taken as one number for the whole band: frequency-dependent
 * imbalance is not corrected. Before the first signal the balance is identity. Behaviour under fading is unmeasured. mgpu_pool_* does not
 * forward the stage, and bench.py does not know it.
 *
 * Errors as mercury_gpu.h. The context rules of INTEGRATION.md §2 apply: a corrector belongs to its context, is used by one thread at a
 * time with it and is destroyed before it.
 *
 * This header lives under include/ext/: the prototypes under include/ itself are a closed set.
 */
#ifndef MERCURY_IQ_CORRECTOR_H
#define MERCURY_IQ_CORRECTOR_H

#include <stddef.h>
#include <stdint.h>

#include "../mercury_channelizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGPU_IQC_MIN_BLOCK 256
#define MGPU_IQC_MAX_BLOCK 4096
#define MGPU_IQC_MAX_MEMORY (1 << 20)
#define MGPU_IQC_DEFAULT_MEMORY 1024
#define MGPU_IQC_MAX_SKEW 0.5
#define MGPU_IQC_MAX_GAIN 2.0

#define MGPU_IQC_SKIPPED 1          /* a sum of the block was not finite: the state did not move */
#define MGPU_IQC_NO_BALANCE 2       /* the measured balance is not valid: skew 0, gain 1 */

typedef struct mgpu_iqc mgpu_iqc;

typedef struct mgpu_iqc_config {
    int struct_size;        /* = sizeof(mgpu_iqc_config), else MGPU_ERR_ARG (versioned by size, as mgpu_scan_config) */
    int D;                  /* 1..64: the rate is 48000 * D */
    int format;             /* MGPU_IQ_*: the format of the input and of the output */
    int block;              /* B: a multiple of 256, 256..4096; 0: 4096 */
    int memory;             /* M in blocks: 0 (lambda = 1) or 2..2^20 (MGPU_IQC_DEFAULT_MEMORY) */
    int dc;                 /* 1: remove the measured means */
    int balance;            /* 1: apply the measured skew and gain */
    int fixed;              /* 1: no estimate; the four values below for every block */
    double fixed_dc_re, fixed_dc_im, fixed_skew, fixed_gain;
    int max_in;             /* IQ samples that one call may take, a multiple of B; 0: 1024 * B */
    int pad;
} mgpu_iqc_config;

typedef struct mgpu_iqc_report {
    int64_t block;          /* the block the report describes */
    double dc_re, dc_im, skew, gain;    /* the values used on the block's samples */
    int flags;              /* MGPU_IQC_SKIPPED | MGPU_IQC_NO_BALANCE */
    int clamped;            /* CS16 components of the block that were clamped */
} mgpu_iqc_report;

typedef struct mgpu_iqc_state {
    uint64_t position;      /* the next IQ sample's position */
    uint64_t blocks;        /* position / B: the next block */
    int D, block, max_in, format;
    double lambda;
    double T[6];            /* T_I, T_Q, T_II, T_IQ, T_QQ, N */
    double dc_re, dc_im, skew, gain;    /* the estimate T gives (the fixed values in fixed mode): what a skipped block would use */
    int flags;              /* MGPU_IQC_NO_BALANCE or 0 */
    int pad;
} mgpu_iqc_state;

/* Without a context (no device could be opened) a valid configuration gives MGPU_ERR_DEVICE, a bad one MGPU_ERR_ARG. */
int mgpu_iqc_create(mgpu_ctx* ctx, const mgpu_iqc_config* config, mgpu_iqc** out);
int mgpu_iqc_destroy(mgpu_iqc* iqc);
/* the next IQ sample is `position`, a multiple of B, 2^62 at most; the state becomes zero */
int mgpu_iqc_seek(mgpu_iqc* iqc, uint64_t position);
/* waits for the handle's earlier calls */
int mgpu_iqc_status(mgpu_iqc* iqc, mgpu_iqc_state* state);
/* n_in IQ samples (a positive multiple of B, at most max_in) in the handle's format in host or device memory (detected) -> n_in output
 * samples in the same format and n_in / B reports (NULL: not wanted) in host memory; *n_reports = n_in / B (NULL: not wanted). Blocks.
 * A bad n_in gives MGPU_ERR_ARG and changes nothing. */
int mgpu_iqc_process(mgpu_iqc* iqc, const void* iq, int n_in, void* out, mgpu_iqc_report* reports, int* n_reports);
/* the same with device input and output, asynchronous on `stream` (a hipStream_t; NULL: the context's stream). d_out must not overlap
 * d_iq; d_reports may be NULL. The state stays on the device: calls follow each other on a stream without a wait. */
int mgpu_iqc_process_dev(mgpu_iqc* iqc, const void* d_iq, int n_in, void* d_out, mgpu_iqc_report* d_reports, int* n_reports, void* stream);

/* Host only, no GPU needed: the twin. A fresh stage seeked to `position` and fed the whole signal at once (max_in is checked and not
 * read otherwise): out [n_in] samples in config->format, reports [n_in / B] (NULL: not wanted), *n_reports = n_in / B. */
int mgpu_host_iqc_process(const mgpu_iqc_config* config, const void* iq, int n_in, uint64_t position, void* out, mgpu_iqc_report* reports,
                          int* n_reports);
/* the twin continued: state [6] is T before the call's first block and becomes T after its last (zeros: mgpu_host_iqc_process) */
int mgpu_host_iqc_continue(const mgpu_iqc_config* config, double* state, const void* iq, int n_in, uint64_t position, void* out,
                           mgpu_iqc_report* reports, int* n_reports);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_IQ_CORRECTOR_H */

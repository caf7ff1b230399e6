/* mercury_blanker.h — the impulse blanker: median-gated blanking of the baseband samples ahead of the front-end.
 *
 * Impulsive noise with a repetition rate - power-line hash at 100 / 120 Hz, electric fences, ignition - puts two or three impulses into
 * every OFDM symbol of 272 samples. The FFT spreads each impulse over all carriers of its symbol, so every carrier and every symbol is hit
 * alike and neither one variance per frame nor the noise map of mercury_demapper.h can tell the disturbance from the signal. The only place
 * where it is sparse is the time domain, before the FFT: a sample far above the level of its neighbourhood is replaced by zero, which costs
 * the symbol a few of its 272 samples instead of all of its carriers. This is NOT one of the reference's configurations: the reference has
 * no such stage.
 *
 * The rule (MGPU_BLANK_MEDIAN), per frame of n = frame_samples complex samples x[0 .. n-1]; mgpu_host_blank below is the normative statement:
 *   p[i]     = x.re * x.re + x.im * x.im, each product rounded on its own, then the sum, no contraction;
 *   blocks   consecutive runs of L samples from the frame's first sample, L the mode's symbol length Nfft + Ngi (272; the MFSK modes' own
 *            symbol length); a last, shorter block takes any remainder;
 *   key      of a p: its 64-bit pattern with the sign bit cleared, compared as an unsigned integer (NaN above +Inf above every finite value);
 *   med      per block of m samples: the p whose key has rank floor(m / 2) (0-based) in ascending order. A selection, never an average: it
 *            does not depend on any summation order. One level per symbol-length block follows a fading signal; one level per frame blanks
 *            the up-fades of a clean frame;
 *   limit    = threshold * med, one multiplication; sample i exceeds when !(p[i] <= limit): a NaN sample exceeds, a block whose med is NaN
 *            exceeds everywhere;
 *   marked   sample i is marked when any sample j with |i - j| <= guard exceeds; the guard runs over the frame, across block borders, and is
 *            clipped at the frame's ends;
 *   cap      = floor(max_share * n), computed once on the host in double. If the number of marked samples is at most cap, the output is the
 *            input with every marked sample replaced by {+0.0, +0.0} and blanked = marked; otherwise the output is the input byte for byte
 *            and blanked = 0: that is no impulse problem, and the frame is left to the stages that follow.
 * The per-frame report is {marked, blanked}.
 *
 * Parameters: threshold finite and >= 2, default 24 (a clean sample's power is exponentially distributed, its median ln 2 times its mean:
 * 24 medians are 16.6 means, passed with probability 6e-8; at 12 medians a faded clean frame already loses samples); guard 0 .. 16 samples,
 * default 4 (the 33-tap receive filter at 48 kHz smears a passband click over about 8 samples of 12 kHz baseband); max_share in (0, 0.5],
 * default 0.125.
 *
 * Where it holds: at the head of the fused receive span, wherever that runs - mgpu_rx_batch / _dev / _taps / _div, both self-simulations,
 * the decode phase of mgpu_receive_byte_batch and with it mgpu_capture_* and mgpu_linksim_*. Every frame passes through the blanker into a
 * workspace of the context, and everything behind it - the front-end in all its forms (mercury_demapper.h, mercury_cfo.h), the decoder, the
 * retries of an estimator ladder (mercury_estimator.h), the grouped span of mercury_diversity.h, the zero-forcing SNR - reads the blanked
 * copy; mgpu_rx_batch_taps describes the blanked frame. Accepted on every mode, OFDM, zero-forcing and MFSK alike: it runs before anything
 * mode-specific. With MGPU_BLANK_MEDIAN a one-frame mgpu_rx_batch call does not go through its captured graph; it equals the frame's row in
 * a batch. A span with the stage on takes frames whose rows lie inside max_batch, as a ladder does. The one-stage entry points
 * (mgpu_frontend_dev, mercury_stages.h) keep the plain stages: mgpu_blank_dev is there to put in front of them. mgpu_pool_* does not forward
 * the setting; set it on each mgpu_pool_context.
 * Limits: the synchroniser and the passband filter of mgpu_receive_byte_batch still see the unblanked samples (only the decode phase is
 * behind the blanker); there is no blanking at 48 kHz; there is no clipping mode (a marked sample becomes zero, never a limited value); the
 * device self-simulations have no impulse source. (Narrowband carriers are removed ahead of the synchroniser: ext/mercury_excisor.h.)
 * On the wideband path clicks are blanked in the IQ at 48000 * D, ahead of the channeliser and every filter: ext/mercury_wideband_blanker.h.
 * Off by default (MGPU_BLANK_OFF): every entry point computes what it computed before, with the same kernels.
 */
#ifndef MERCURY_BLANKER_H
#define MERCURY_BLANKER_H

#include <stddef.h>

#include "mercury_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGPU_BLANK_OFF 0      /* the reference's receiver: the samples go to the front-end as they are */
#define MGPU_BLANK_MEDIAN 1   /* the rule above */

typedef struct mgpu_blanker_params {
    double threshold;         /* finite, >= 2: a sample exceeds above threshold * its block's median power. Default 24 */
    int guard;                /* 0..16 samples on either side of an exceeding sample are marked with it. Default 4 */
    double max_share;         /* in (0, 0.5]: a frame with more than floor(max_share * n) marked samples passes unchanged. Default 0.125 */
} mgpu_blanker_params;
#define MGPU_BLANKER_PARAMS_DEFAULT {24.0, 4, 0.125}

typedef struct mgpu_blanker_report {
    int marked;               /* samples the rule marked */
    int blanked;              /* samples replaced by zero: marked, or 0 where marked was above the cap */
} mgpu_blanker_report;

/* mode: MGPU_BLANK_OFF or MGPU_BLANK_MEDIAN, on every mode of the receiver. params (read for MGPU_BLANK_MEDIAN only; NULL: the defaults);
 * params_size must be sizeof(mgpu_blanker_params). MGPU_ERR_ARG for another mode value, another params_size, or a parameter outside the
 * ranges above (NaN included). MGPU_BLANK_MEDIAN allocates the context's workspace of max_batch * frame_samples * 16 bytes (mode 0 at
 * max_batch 4096: 816 MiB) and the report array of max_batch rows; MGPU_ERR_DEVICE where that fails. MGPU_BLANK_OFF releases the workspace.
 * A refusal leaves the context as it was. Waits for the context's stream; work queued on a caller's stream must have finished.
 * mgpu_get_blanker returns the mode and the parameters last set (the defaults before). */
int mgpu_set_blanker(mgpu_ctx* ctx, int mode, const mgpu_blanker_params* params_or_null, size_t params_size);
int mgpu_get_blanker(mgpu_ctx* ctx, int* mode, mgpu_blanker_params* params, size_t params_size);

/* The reports of rows first .. first + count - 1 (first + count <= max_batch) of the last fused span that ran with MGPU_BLANK_MEDIAN, by the
 * frame's row. Rows the span did not write keep what an earlier span left there (0 after mgpu_set_blanker). Waits for the context's stream.
 * MGPU_ERR_ARG before the mode was ever set. */
int mgpu_get_blanker_report(mgpu_ctx* ctx, int first, int count, mgpu_blanker_report* report /*[count]*/);

/* The stage on its own, on device buffers: F frames of frame_samples complex128 samples, frame_stride complex samples apart in d_in (0: the
 * frame length; at least 1 otherwise), into the dense d_out [F][frame_samples], which must not overlap d_in; the reports, if wanted, into
 * d_report [F]. Works whether or not the mode is set, with the parameters last set (the defaults before). Queued on `stream` (NULL: the
 * default stream); does not wait. */
int mgpu_blank_dev(mgpu_ctx* ctx, const void* d_in_c128, int F, int frame_stride, void* d_out_c128, void* d_report_or_null, void* stream_or_null);

/* Host twin of the rule above, no GPU: one frame. cfg / p_or_null: the mode, as for mgpu_host_ls_estimate (it gives n and L). params NULL:
 * the defaults. out may be in. report may be NULL. MGPU_ERR_ARG for a cfg that is no mode or for refused parameters. */
int mgpu_host_blank(int cfg, const mgpu_explicit_params* p_or_null, const mgpu_blanker_params* params_or_null, const double* in_c128 /*[frame_samples]*/,
                    double* out_c128 /*[frame_samples]*/, mgpu_blanker_report* report);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_BLANKER_H */

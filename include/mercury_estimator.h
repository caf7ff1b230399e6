/* mercury_estimator.h — rectangular LS estimator windows and the estimator ladder.
 *
 * The reference's LS_channel_estimator (ofdm.cc:1315-1451) averages the pilots of a window of LS_window_width x LS_window_hight cells
 * around each pilot. The two are separate members (ofdm.cc:1359-1363); load_configuration sets them equal (telecom_system.cc:2802-2809:
 * 20, made odd = 21). 21 carriers are about 940 Hz: on a two-path channel whose notches are closer than that the mean removes the second
 * path, and the frame is equalised with the wrong channel (profiles/estimator_ladder.md). A window narrow in frequency and long in time
 * keeps the averaging and follows such a channel; it costs a few tenths of a dB on a flat one.
 *
 * An estimator ladder is an ordered list of up to MGPU_LADDER_MAX windows (its rungs). With a ladder set, every place that runs the fused
 * receive span (front-end + LDPC decoder) - mgpu_rx_batch / _dev / _taps, both self-simulations, the decode phase of
 * mgpu_receive_byte_batch and with it mgpu_capture_*, mgpu_linksim_* and the passband self-simulations - works like this, per frame:
 *   - rung 0 runs on all frames;
 *   - each later rung runs on exactly the frames whose message_decoded is 0 after the rungs before it: they are re-estimated, re-equalised,
 *     demapped and decoded again from the same samples, on the device;
 *   - the frame's record (payload, stats, variance, SNR variance, mean_H, optional LLRs) is that of the first rung that decodes it; a frame no
 *     rung decodes reports rung 0's record;
 *   - stage taps (mgpu_rx_batch_taps) describe rung 0;
 *   - the result depends on the frame alone, not on the batch, the frame's place in it or how a call is chunked.
 * In mgpu_receive_byte_batch the ladder runs inside one trial's decode, before the host looks at the results: a window a later rung decodes
 * counts as decoded in that trial. With a ladder set, a one-frame mgpu_rx_batch call does not go through its captured graph.
 * Off by default: with no ladder (0 rungs; accepted on every mode) every entry point computes what it computed before. This is NOT one
 * of the reference's configurations: a rectangular window is the reference's algorithm with a setting load_configuration never makes,
 * and the retry does not exist there. mgpu_pool_* does not forward the ladder; set it on each mgpu_pool_context.
 * The one-stage entry point mgpu_channel_estimator (mercury_stages.h) keeps the context's square window; it does not follow rung 0.
 *
 * A window is `width` cells in frequency (carriers) by `height` cells in time (symbols), each 1..21; an even value is incremented as
 * telecom_system.cc:2802-2809 does. The width is bounded by the front-end, which reads at most 7 pilots of a window row. Anything else is
 * refused with MGPU_ERR_ARG and the context is left as it was. Only OFDM modes with the LS estimator take a ladder: the zero-forcing
 * modes (15, 16, explicit ZF) and the MFSK modes return MGPU_ERR_UNSUPPORTED.
 */
#ifndef MERCURY_ESTIMATOR_H
#define MERCURY_ESTIMATOR_H

#include "mercury_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgpu_ls_window { int width, height; } mgpu_ls_window;   /* cells: frequency x time */
#define MGPU_LADDER_MAX 4

/* n_rungs 0 (rungs may be NULL): no ladder. Waits for the context's stream; work queued on a caller's stream must have finished. */
int mgpu_set_estimator_ladder(mgpu_ctx* ctx, const mgpu_ls_window* rungs, int n_rungs);
/* the rungs as they are applied (odd); rungs: room for MGPU_LADDER_MAX */
int mgpu_get_estimator_ladder(mgpu_ctx* ctx, mgpu_ls_window* rungs, int* n_rungs);
/* of the last fused-span call (for mgpu_receive_byte_batch: the last trial's decode, in the order of the windows it decoded): the winning
 * rung of each of its F frames, -1 where no rung decoded. Waits for the context's stream. MGPU_ERR_ARG without a ladder or when F exceeds
 * that call's frames. */
int mgpu_estimator_rungs_last(mgpu_ctx* ctx, int* rung /*[F]*/, int F);
/* frames decoded by each rung and frames seen since the ladder was set (or the last reset) */
int mgpu_estimator_ladder_counters(mgpu_ctx* ctx, long long decoded_by_rung[MGPU_LADDER_MAX], long long* frames, int reset);
/* Host twin of the front-end's LS estimate, no GPU: the estimate at the nPilots pilot cells (row-major pilot order) of one frame grid
 * (after the AGC) for the mode `cfg` (p_or_null: the explicit parameters of mgpu_create_explicit; its ls_window is not used) and a
 * width x height window. Same terms in the same order as the kernel. */
int mgpu_host_ls_estimate(int cfg, const mgpu_explicit_params* p_or_null, int width, int height, const double* grid_c128 /*[Nsymb*Nc]*/,
                          double* H_pilots_c128 /*[nPilots]*/);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_ESTIMATOR_H */

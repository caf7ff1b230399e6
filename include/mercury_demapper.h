/* mercury_demapper.h — the channel-aware demapper: max-log LLRs weighted by |H|^2 per cell.
 *
 * The reference's receiver equalises every cell to unit gain - the QAM and zero-forcing modes with the full channel estimate h, the PSK
 * modes (amp_restore) with h / |h| - and divides all LLRs of a frame by one measured variance (cl_psk::demod, psk.cc:278-326). A cell in a
 * notch of the channel has its noise multiplied by 1 / |H| and still hands the decoder LLRs as confident as a clean cell's. For
 * y = H x + n the max-log LLR is (|y - H x1|^2 - |y - H x0|^2) / sigma2 = |H|^2 / sigma2 * (|y/H - x1|^2 - |y/H - x0|^2): the same
 * distances, weighted per cell. This is NOT one of the reference's configurations: the reference has no such demapper.
 *
 * The rule (MGPU_DEMAP_CSI), per frame; mgpu_host_demap_csi below is the normative statement:
 *   g       the cell grid after the AGC, as without it;
 *   h       the LS / ZF estimate at every cell after column interpolation, from the context's window or the rung's under an estimator ladder,
 *           BEFORE restore_channel_amplitude (the PSK modes' full estimate, not its unit phasor);
 *   sigma2  = (sum over the pilots p, in pilot order, one term after the other, of |g_p - h_p x_p|^2) / nPilots in double, x_p = +-pilot_boost,
 *           a term being dr = g.re - h.re * x, di = g.im - h.im * x, dr * dr + di * di;
 *   a data cell: e = g / h (the equaliser's own complex division), wf = float(h.re * h.re + h.im * h.im);
 *   demapping as without it (squared distances to the constellation in double, narrowed to float; per bit the smaller, fminf semantics; the
 *           same bit order), but LLR = (inv * wf) * (d1 - d0) in float with inv = 1.0f / float(sigma2);
 *   de-interleaving and the shortening re-pack are unchanged.
 * A frame's reported variance, SNR variance, mean_H and snr_db stay exactly what the plain front-end reports, bit for bit (they feed
 * mgpu_receive_byte_batch's gates and the statistics), so the PSK modes still compute the restored-amplitude quantities for those. Only the
 * LLRs, and what the decoder makes of them, change. With MGPU_DEMAP_CSI the stage taps H and eq (mgpu_rx_batch_taps) show the h and e
 * defined here; in the amp_restore modes these differ from the plain taps (H is not a unit phasor). The equalised symbols kept for the
 * zero-forcing modes' SNR are the same in both (those modes have no amplitude restoration).
 *
 * Where it holds: everywhere the fused receive span runs - mgpu_rx_batch / _dev / _taps, both self-simulations, the decode phase of
 * mgpu_receive_byte_batch and with it mgpu_capture_*, mgpu_linksim_* and the passband self-simulations, every rung of an estimator ladder
 * (mercury_estimator.h), the grouped span of mercury_diversity.h (the float sum of such LLRs is maximal-ratio combining for every
 * constellation). With MGPU_DEMAP_CSI a one-frame mgpu_rx_batch call does not go through its captured graph; it equals the frame's row in
 * a batch. The one-stage entry points of mercury_stages.h keep the plain demapper. mgpu_pool_* does not forward the setting; set it on each
 * mgpu_pool_context.
 * Off by default (MGPU_DEMAP_MAXLOG): every entry point computes what it computed before.
 */
#ifndef MERCURY_DEMAPPER_H
#define MERCURY_DEMAPPER_H

#include "mercury_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGPU_DEMAP_MAXLOG 0   /* the reference's demapper: one variance per frame */
#define MGPU_DEMAP_CSI 1      /* max-log LLRs weighted by |H|^2 per cell */

/* Accepted on all OFDM modes, explicit geometries and zero-forcing included. MGPU_ERR_ARG for any other value; MGPU_ERR_UNSUPPORTED for
 * MGPU_DEMAP_CSI on the MFSK modes (no channel estimate; MGPU_DEMAP_MAXLOG is what they have and is accepted); MGPU_ERR_TABLES for a frame
 * geometry whose LDS carve with the two extra arrays does not fit a compute unit. A refusal leaves the context as it was.
 * Waits for the context's stream; work queued on a caller's stream must have finished. */
int mgpu_set_demapper(mgpu_ctx* ctx, int demapper);
int mgpu_get_demapper(mgpu_ctx* ctx, int* demapper);

/* Host twin of the rule above, no GPU: one frame's cell grid (after the AGC) and channel estimate at every cell -> the demodulated LLRs
 * in the demapper's order (what the llr_demod stage tap holds; mgpu_deinterleaver_f32's input) and sigma2. cfg / p_or_null: the mode, as
 * for mgpu_host_ls_estimate. Same terms in the same order as the kernel. MGPU_ERR_UNSUPPORTED for the MFSK modes. */
int mgpu_host_demap_csi(int cfg, const mgpu_explicit_params* p_or_null, const double* grid_c128 /*[Nsymb*Nc]*/, const double* H_c128 /*[Nsymb*Nc]*/,
                        float* llr_demod_f32 /*[nBits]*/, double* sigma2_out);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_DEMAPPER_H */

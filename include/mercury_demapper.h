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
 *
 * The noise-map demapper (MGPU_DEMAP_NMAP): the CSI rule with a noise variance per carrier and per symbol. One sigma2 per frame assumes the
 * frame's noise is white; a carrier from another station inside the channel ruins a handful of the 50 carriers for the whole frame, a static
 * crash one or two OFDM symbols on all carriers, and with one variance those cells hand the decoder LLRs as confident as clean ones while the
 * inflated sigma2 weakens every clean cell. With Dx = 1 every carrier has a pilot every Dy symbols and every symbol one every Dy carriers, so
 * the pilot residuals can be averaged per carrier and per symbol: a separable map sigma2(c, s) = sigma2 fc(c) fs(s) follows both kinds of
 * disturbance. Opt-in, and NOT one of the reference's configurations either.
 *
 * The rule, per frame; mgpu_host_demap_nmap below is the normative statement. g, h, the residual r_p = |g_p - h_p x_p|^2 of pilot p,
 * sigma2 = serial sum(r_p) / nPilots, e = g / h and wf = float(|h|^2) are MGPU_DEMAP_CSI's, bit for bit. Then, all in double:
 *   S_c     the sum of r_p over carrier c's pilots in ascending symbol order, from +0.0; n_c their count;
 *   V_c     = (S_{c-w} + ... + S_{c+w}) / (n_{c-w} + ... + n_{c+w}), w = smooth (default 1, 0..4), added in ascending carrier order from +0.0,
 *           carriers outside 0..Nc-1 left out;
 *   U_s     = (the sum of r_p over symbol s's pilots in ascending carrier order, from +0.0) / their count (a symbol's pilots are consecutive
 *           in pilot order);
 *   fc      = V_c / sigma2, fs = U_s / sigma2; a factor f becomes exactly 1.0 when it is NaN, when its count is 0, when sigma2 is 0 or not
 *           finite, or when it lies inside the dead band: !(f > band) && !(f * band < 1). band = dead_band (default 2.0; any value >= 1, +Inf
 *           included: no factor ever leaves the band then). Without the band, dividing by estimates from 8 to 24 pilots costs about 0.4 dB in
 *           white noise;
 *   a_c     = 1.0f / float(sigma2 * fc), b_s = 1.0f / float(fs);
 *   demapped symbol k comes from cell T.sym_src[k], carrier cell % Nc, symbol cell / Nc: LLR = ((a_c * b_s) * wf) * (d1 - d0) in float.
 * Distances, minima, bit order, de-interleaving and re-pack are unchanged. A frame none of whose factors leaves the band has
 * a_c = 1.0f / float(sigma2) and b_s = 1.0f: its LLRs are MGPU_DEMAP_CSI's bit for bit. What is reported (variance, SNR variance, mean_H,
 * snr_db) stays the plain front-end's, and the H and eq taps show what they show under MGPU_DEMAP_CSI.
 * It holds where MGPU_DEMAP_CSI holds, every rung of a ladder with its own h and its own map, Wiener rungs and the carrier-offset stage
 * included, with the same exclusions: mercury_stages.h keeps the plain demapper, mgpu_pool_* does not forward it, the one-frame captured
 * graph of mgpu_rx_batch is bypassed while it is on.
 */
#ifndef MERCURY_DEMAPPER_H
#define MERCURY_DEMAPPER_H

#include <stddef.h>

#include "mercury_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGPU_DEMAP_MAXLOG 0   /* the reference's demapper: one variance per frame */
#define MGPU_DEMAP_CSI 1      /* max-log LLRs weighted by |H|^2 per cell */
#define MGPU_DEMAP_NMAP 2     /* ... and divided by a noise variance per carrier and per symbol, measured at the pilots */

typedef struct mgpu_demapper_params {
    double dead_band;         /* >= 1, +Inf allowed: factors within [1 / dead_band, dead_band] are 1. Default 2.0 */
    int smooth;               /* 0..4 carriers on either side share a carrier's mean. Default 1 */
} mgpu_demapper_params;

/* Accepted on all OFDM modes, explicit geometries and zero-forcing included. MGPU_ERR_ARG for any other value; MGPU_ERR_UNSUPPORTED for
 * MGPU_DEMAP_CSI on the MFSK modes (no channel estimate; MGPU_DEMAP_MAXLOG is what they have and is accepted); MGPU_ERR_TABLES for a frame
 * geometry whose LDS carve with the two extra arrays does not fit a compute unit. A refusal leaves the context as it was.
 * Waits for the context's stream; work queued on a caller's stream must have finished. */
int mgpu_set_demapper(mgpu_ctx* ctx, int demapper);
int mgpu_get_demapper(mgpu_ctx* ctx, int* demapper);

/* The same with the noise map's parameters (read for MGPU_DEMAP_NMAP only; NULL: the defaults, which is what mgpu_set_demapper(ctx,
 * MGPU_DEMAP_NMAP) sets). params_size must be sizeof(mgpu_demapper_params). Beyond mgpu_set_demapper's refusals: MGPU_ERR_ARG for a
 * dead_band below 1 or NaN, a smooth outside 0..4 or another params_size; MGPU_ERR_UNSUPPORTED for MGPU_DEMAP_NMAP on the zero-forcing modes
 * (a ZF estimate passes through its own pilots: the residuals are rounding noise); MGPU_ERR_TABLES where the noise-map forms' LDS carve does
 * not fit. A refusal leaves the context as it was. mgpu_get_demapper_ex returns the mode and the parameters last set (the defaults before). */
int mgpu_set_demapper_ex(mgpu_ctx* ctx, int demapper, const mgpu_demapper_params* params_or_null, size_t params_size);
int mgpu_get_demapper_ex(mgpu_ctx* ctx, int* demapper, mgpu_demapper_params* params, size_t params_size);

/* The factors, after the dead band, of frames first .. first + count - 1 of the last fused-span call that ran with MGPU_DEMAP_NMAP, by the
 * frame's row (first + count <= max_batch): what lets an operator see an interferer (fc) or a static crash (fs). Under an estimator ladder
 * these are rung 0's; retries do not write. Either array may be NULL. Waits for the context's stream. MGPU_ERR_ARG before the mode was
 * ever set. */
int mgpu_get_noise_map(mgpu_ctx* ctx, int first, int count, double* fc /*[count][Nc]*/, double* fs /*[count][Nsymb]*/);

/* Host twin of the rule above, no GPU: one frame's cell grid (after the AGC) and channel estimate at every cell -> the demodulated LLRs
 * in the demapper's order (what the llr_demod stage tap holds; mgpu_deinterleaver_f32's input) and sigma2. cfg / p_or_null: the mode, as
 * for mgpu_host_ls_estimate. Same terms in the same order as the kernel. MGPU_ERR_UNSUPPORTED for the MFSK modes. */
int mgpu_host_demap_csi(int cfg, const mgpu_explicit_params* p_or_null, const double* grid_c128 /*[Nsymb*Nc]*/, const double* H_c128 /*[Nsymb*Nc]*/,
                        float* llr_demod_f32 /*[nBits]*/, double* sigma2_out);

/* Host twin of MGPU_DEMAP_NMAP, no GPU: as mgpu_host_demap_csi, with the parameters (NULL: the defaults; params_size as above) and the
 * factors after the dead band (fc_out [Nc], fs_out [Nsymb]; each may be NULL). Same terms in the same order as the kernel.
 * MGPU_ERR_UNSUPPORTED for the MFSK and the zero-forcing modes, MGPU_ERR_ARG for refused parameters. */
int mgpu_host_demap_nmap(int cfg, const mgpu_explicit_params* p_or_null, const double* grid_c128 /*[Nsymb*Nc]*/, const double* H_c128 /*[Nsymb*Nc]*/,
                         const mgpu_demapper_params* params_or_null, size_t params_size, float* llr_demod_f32 /*[nBits]*/, double* sigma2_out,
                         double* fc_out, double* fs_out);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_DEMAPPER_H */

/* mercury_cfo.h — pilot-aided residual carrier-offset correction in the front-end.
 *
 * The receiver removes the carrier offset its preamble estimator measures (cl_ofdm::carrier_sampling_frequency_sync) and nothing after
 * that. What the estimator leaves behind - its own error, 1.5 to 4 Hz on noisy windows (profiles/residual_cfo.md) - turns the cell grid by
 * a constant angle per symbol: 2 Hz is 16 degrees per symbol of 272 samples at 12 kHz. An LS window 21 symbols long averages such an
 * estimate towards zero and the frame is lost; a window 5 symbols long tolerates it at the price of its noise averaging. The frame's own
 * pilots measure the turn: same-carrier pilots Dy symbols apart differ by Dy steps. This is NOT one of the reference's configurations:
 * the reference has no such stage.
 *
 * The rule (MGPU_CFO_PILOTS), per frame, between the AGC and the channel estimate; mgpu_host_cfo_pilots below is the normative statement:
 *   g       the cell grid [Nsymb][Nc] after the AGC, as without it;
 *   z       at a pilot cell, g or -g by the pilot's sign (exact);
 *   a_c     per carrier c, over its pilots in ascending symbol order, for every consecutive pair whose symbol distance equals Dy, z1 the
 *           later one: a_c.re += z1.re * z0.re + z1.im * z0.im, a_c.im += z1.im * z0.re - z1.re * z0.im; one term after the other from +0.0,
 *           no contraction;
 *   r       = sum of a_c, serially for c = 0 .. Nc - 1 from +0.0;
 *   step    = 0, and the grid passes through byte for byte, if r.re or r.im is not finite or both are zero; otherwise
 *           get_angle(r) / Dy in radians per symbol, get_angle and its atan being the front-end's own (misc.cc:34-56; x86-64 glibc 2.35);
 *   symbol s: (sn, cs) = sincos(-step * double(s)) (the front-end's sincos; |step * s| < 50), every cell of the symbol becomes
 *           {g.re * cs - g.im * sn, g.re * sn + g.im * cs}. Symbol 0 is the reference: a constant phase is the channel estimate's business.
 * Everything behind this point sees the turned grid and is otherwise unchanged: LS / ZF estimate, interpolation, amplitude restoration,
 * equaliser, variance, SNR variance, mean_H, either demapper. The reported statistics are those of the corrected frame (mean_H feeds
 * mgpu_receive_byte_batch's gate, which an offset frame fails without the correction). The `grid` stage tap shows the turned grid.
 *
 * Range. The measured angle is Dy steps, so the rule is unambiguous for |f| < 12000 / (2 * Dy * Nofdm): 7.35 Hz at Dy = 3 (every mode's
 * default), 4.4 Hz at Dy = 5. An offset beyond that is turned by the wrong amount. f = step * 12000 / (2 pi * Nofdm).
 *
 * Where it holds: everywhere the fused receive span runs - mgpu_rx_batch / _dev / _taps, both self-simulations, the decode phase of
 * mgpu_receive_byte_batch and with it mgpu_capture_*, mgpu_linksim_* and the passband self-simulations, every rung of an estimator ladder
 * (mercury_estimator.h; a retry computes the same step again), every branch of the grouped span of mercury_diversity.h, with either
 * demapper (mercury_demapper.h). With MGPU_CFO_PILOTS a one-frame mgpu_rx_batch call does not go through its captured graph; it equals
 * the frame's row in a batch. The one-stage entry points of mercury_stages.h keep the plain stages. mgpu_pool_* does not forward the
 * setting; set it on each mgpu_pool_context. mgpu_receive_stats.freq_offset and the link state stay the preamble's measurement: the
 * residual is not fed back.
 * Off by default (MGPU_CFO_OFF): every entry point computes what it computed before.
 */
#ifndef MERCURY_CFO_H
#define MERCURY_CFO_H

#include "mercury_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGPU_CFO_OFF 0      /* the reference's front-end: no correction behind the preamble's */
#define MGPU_CFO_PILOTS 1   /* the rule above */

/* Accepted on all OFDM modes, explicit geometries and zero-forcing included. MGPU_ERR_ARG for any other value; MGPU_ERR_UNSUPPORTED for
 * MGPU_CFO_PILOTS on the MFSK modes (no pilots; MGPU_CFO_OFF is what they have and is accepted). A refusal leaves the context as it was.
 * Waits for the context's stream; work queued on a caller's stream must have finished. */
int mgpu_set_cfo(mgpu_ctx* ctx, int cfo);
int mgpu_get_cfo(mgpu_ctx* ctx, int* cfo);

/* The steps (radians per symbol) of rows 0 .. F-1 of the last fused span that ran with MGPU_CFO_PILOTS, as rung 0 measured them; F at most
 * the context's max_batch. Rows the span did not write keep what an earlier span left there (0 after mgpu_set_cfo). Waits for the
 * context's stream. */
int mgpu_get_cfo_steps(mgpu_ctx* ctx, int F, double* step);

/* Host twin of the rule above, no GPU: one frame's cell grid (after the AGC) -> the turned grid and the step. cfg / p_or_null: the mode, as
 * for mgpu_host_ls_estimate. grid_out may be grid_in. Same terms in the same order as the kernel, with the front-end's atan and sincos
 * compiled for the host. MGPU_ERR_UNSUPPORTED for the MFSK modes. */
int mgpu_host_cfo_pilots(int cfg, const mgpu_explicit_params* p_or_null, const double* grid_in_c128 /*[Nsymb*Nc]*/, double* grid_out_c128 /*[Nsymb*Nc]*/,
                         double* step_out);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_CFO_H */

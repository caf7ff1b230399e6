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
 *
 * A rung may also be the separable Wiener estimator (MGPU_RUNG_WIENER, set through mgpu_set_estimator_ladder_ex). A flat
 * window is a poor low-pass in the delay domain; this rung filters the sign-applied pilots with taps designed for a delay interval and
 * a Doppler bound instead: along time per carrier (every carrier that has pilots has one every Dy symbols), then along frequency per
 * symbol (one every Dy carriers). Everything behind the estimate at the pilots - column interpolation, amplitude restoration, equaliser,
 * both variances, mean_H, either demapper, the taps - is unchanged. A one-rung ladder means "this estimator alone". Every ladder rule
 * above holds for such a rung as written. This is NOT one of the reference's configurations: the reference has no such estimator.
 *
 * The rule (mgpu_host_wiener_estimate is normative; the kernel forms the same terms in the same order):
 *   design: tau0, tau1 = the delay bounds in baseband samples (us * 12000 / 1e6), Ts = 272 / 12000 s, s2 = 10^(-snr_db / 10) / boost^2,
 *           k(c) = carrier c's FFT bin relative to the empty DC bin: c - 25 below carrier 25, else c - 24; sinc(x) = sin(pi x) / (pi x).
 *   time:   for each distinct set of pilot rows a carrier has, Rt[a][b] = sinc(2 doppler Ts (row_a - row_b)), A = Rt (Rt + s2 I)^-1 (real).
 *   unit gain: row i of A is divided by sum_k A[i][k] Rt[k][i]; row i of B by Re sum_k B[i][k] Rf[k][i].
 *   frequency: s2b = s2 times the mean, over the frame's pilots, of the sum of squares of the pilot's row of A at unit gain; for each
 *           distinct set of pilot carriers a symbol has, d = k(c_a) - k(c_b), Rf[a][b] = sinc((tau1 - tau0) d / 256) exp(-j 2 pi d (tau0 + tau1) / 512),
 *           B = Rf (Rf + s2b I)^-1 (complex). Last, every A is multiplied by 1 / boost.
 *   per frame, on the grid after the AGC (and the carrier-offset stage where that is on), yp = the pilots times their sign:
 *           t[p] = sum_k A[row of p][k] yp[k-th pilot of p's carrier], ascending symbols, real and imaginary sums separate from +0.0;
 *           H[p] = sum_m B[row of p][m] t[m-th pilot of p's symbol], ascending carriers, hr += (b.re t.re - b.im t.im),
 *           hi += (b.re t.im + b.im t.re); every product and the difference rounded on its own. Non-finite inputs give what IEEE gives.
 */
#ifndef MERCURY_ESTIMATOR_H
#define MERCURY_ESTIMATOR_H

#include "mercury_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgpu_ls_window { int width, height; } mgpu_ls_window;   /* cells: frequency x time */
#define MGPU_LADDER_MAX 4

#define MGPU_RUNG_LS 0          /* the LS mean over `window` */
#define MGPU_RUNG_WIENER 1      /* the separable Wiener estimator designed by `design`; `window` is not used */
/* The channel a Wiener rung is designed for: delays within [tau_min_us, tau_max_us] of the frame timing, Doppler within +-doppler_hz,
 * pilots received at snr_db. The defaults (MGPU_WIENER_DESIGN_DEFAULT) cover -4 .. 28 baseband samples. tau_max_us <= tau_min_us,
 * doppler_hz < 0, snr_db outside [-20, 40] or a non-finite field is refused with MGPU_ERR_ARG. */
typedef struct mgpu_wiener_design { double tau_min_us, tau_max_us, doppler_hz, snr_db; } mgpu_wiener_design;
#define MGPU_WIENER_DESIGN_DEFAULT { -333.33, 2333.33, 0.5, 0.0 }
typedef struct mgpu_estimator_rung { int kind; mgpu_ls_window window; mgpu_wiener_design design; } mgpu_estimator_rung;

/* n_rungs 0 (rungs may be NULL): no ladder. Waits for the context's stream; work queued on a caller's stream must have finished. */
int mgpu_set_estimator_ladder(mgpu_ctx* ctx, const mgpu_ls_window* rungs, int n_rungs);
/* the rungs as they are applied (odd); rungs: room for MGPU_LADDER_MAX. A Wiener rung is reported as {0, 0}. */
int mgpu_get_estimator_ladder(mgpu_ctx* ctx, mgpu_ls_window* rungs, int* n_rungs);
/* The same with a kind per rung; mgpu_set_estimator_ladder is its all-LS case. rung_size: sizeof(mgpu_estimator_rung) as the caller was
 * compiled; anything else is refused with MGPU_ERR_ARG, like a kind that is neither of the two or a design out of range. A refusal leaves
 * the context as it was. The getter reports LS rungs with a zero design and Wiener rungs with a {0, 0} window. */
int mgpu_set_estimator_ladder_ex(mgpu_ctx* ctx, const mgpu_estimator_rung* rungs, int n_rungs, size_t rung_size);
int mgpu_get_estimator_ladder_ex(mgpu_ctx* ctx, mgpu_estimator_rung* rungs /*[MGPU_LADDER_MAX]*/, int* n_rungs, size_t rung_size);
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
/* Host twin of the Wiener estimate, no GPU, and the normative statement of the rule above: the estimate at the nPilots pilot cells of one
 * frame grid for the mode `cfg` and a design (d_or_null: the defaults). */
int mgpu_host_wiener_estimate(int cfg, const mgpu_explicit_params* p_or_null, const mgpu_wiener_design* d_or_null,
                              const double* grid_c128 /*[Nsymb*Nc]*/, double* H_pilots_c128 /*[nPilots]*/);
/* The design's class matrices, for tests. which 0: the time classes (one per distinct set of pilot rows a carrier has, in the order the
 * carriers meet them; real), 1: the frequency classes (per distinct set of pilot carriers a symbol has, in the order the symbols meet
 * them; complex). Every output may be NULL: the number of classes; for class `cls` (MGPU_ERR_ARG when there is none and one of the
 * following is asked for) its size n, its n rows / carriers, and its n x n row-major matrix (n*n doubles / n*n c128) as the kernel reads it. */
int mgpu_host_wiener_tables(int cfg, const mgpu_explicit_params* p_or_null, const mgpu_wiener_design* d_or_null, int which, int cls,
                            int* n_classes, int* n, int* members, double* matrix);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_ESTIMATOR_H */

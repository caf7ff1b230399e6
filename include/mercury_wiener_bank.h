/* mercury_wiener_bank.h — a Wiener rung that chooses its design per frame from a bank, by sounding the frame's own pilots.
 *
 * A Wiener rung of the estimator ladder (mercury_estimator.h: MGPU_RUNG_WIENER) is designed for one delay interval. A wide interval
 * follows a long channel and lets more noise through on a short one; a narrow one is the other way round. With a bank
 * set on such a rung, the rung measures every frame before it estimates: inside a symbol the signed pilots sit s bins apart, and their
 * correlation at one and at two spacings shows the channel's delay spread (the ratio of the two magnitudes) and its mean delay (the
 * angle at one spacing). Both correlations are free of the noise term, noise being independent from pilot to pilot. The first design
 * of the bank the frame fits is the one its estimate is made with. This is NOT one of the reference's configurations: the reference
 * has no such estimator and no such choice.
 *
 * The rule (mgpu_host_wiener_select is normative; the kernel forms the same terms in the same order):
 *   input   the frame grid after the AGC (and the carrier-offset stage where that is on); yp = the pilots times their sign, as the
 *           Wiener rung builds them.
 *   pairs   made from the geometry alone. k(c) is carrier c's bin relative to the empty DC bin, as in mercury_estimator.h. s = the
 *           smallest k(b) - k(a) over consecutive pilots (a, b) of a symbol (Dy for the built-in modes). A 1-pair is two consecutive
 *           pilots of a symbol with k(b) - k(a) = s; a 2-pair is two pilots of a symbol two apart in its pilot order with
 *           k(b) - k(a) = 2 s. Pairs that straddle the DC gap have another distance and are left out. n1, n2 = the pair counts per frame.
 *   sums    in double, no contraction. A pair's term is conj(yp[a]) yp[b]: re = (a.re b.re) + (a.im b.im), im = (a.re b.im) - (a.im b.re),
 *           every product and the one addition or subtraction rounded on its own. Per symbol the terms are added from +0.0 in ascending
 *           order of a, the 1-pairs and the 2-pairs apart, real and imaginary parts apart; then the symbols' partial sums are added from
 *           +0.0 in ascending symbols: R1 = (R1r, R1i), R2 = (R2r, R2i).
 *   bank    n = 1 .. MGPU_WIENER_BANK_MAX entries {design, rho_min}. W_d = (tau_max_us - tau_min_us) * 0.012 samples, strictly ascending.
 *           The LAST entry is the fallback: always eligible, its rho_min is not read. rho_min NaN = the default (m_d + m_{d+1}) / 2 with
 *           m_d = g(2 s W_d / 256) / g(s W_d / 256), g(x) = sinc(x) for x < 1 and 0 otherwise (m_d = 0 where the denominator is 0): the
 *           ratio a uniform delay profile of the design's own width would show. An explicit rho_min is finite and >= 0.
 *   entry d < n - 1 is eligible when both tests pass:
 *     spread    q2 = (R2r R2r + R2i R2i) (double(n1) double(n1)), q1 = (R1r R1r + R1i R1i) (double(n2) double(n2)); q2 >= (rho_min rho_min) q1.
 *     centroid  only where s W_d < 64 (otherwise passed): phi = -2 pi s (tau0 + tau1) / 512 with tau0, tau1 = the design's bounds in
 *               samples (us * 12000 / 1e6), u = (cos phi, sin phi), t = tan(pi s W_d / 256), all three made on the host at set time;
 *               zr = R1r u.re + R1i u.im, zi = R1i u.re - R1r u.im; zr > 0 and fabs(zi) <= t zr. It keeps a frame whose whole channel
 *               sits late - a pure delay, which the ratio cannot see - from a narrow design that does not cover it.
 *   Every comparison is written so that NaN fails: a non-finite frame gets the fallback.
 *   choice  the first eligible entry in bank order. The estimate is mgpu_host_wiener_estimate's with that entry's design, bit for bit;
 *           everything behind the estimate at the pilots is unchanged.
 *
 * A rung with a bank keeps every ladder rule of mercury_estimator.h: as rung 0 it runs on all frames, as a later rung on the frames the
 * rungs before it did not decode (and measures them again). The ladder's own getters keep reporting the rung as it was set. A one-entry
 * bank measures nothing: the rung is the plain Wiener rung of that design (mgpu_get_wiener_choice then reports design 0 and zeros).
 * mgpu_pool_* does not forward the bank; set it on each mgpu_pool_context.
 */
#ifndef MERCURY_WIENER_BANK_H
#define MERCURY_WIENER_BANK_H

#include "mercury_estimator.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGPU_WIENER_BANK_MAX 4
typedef struct mgpu_wiener_bank_entry { mgpu_wiener_design design; double rho_min; } mgpu_wiener_bank_entry;

/* Rung `rung` of the ladder in force must be of kind MGPU_RUNG_WIENER: from now on it chooses per frame among these designs instead of
 * its own. n = 0 (e may be NULL) removes the bank; setting any ladder removes every bank. entry_size: sizeof(mgpu_wiener_bank_entry) as
 * the caller was compiled. MGPU_ERR_ARG for no such rung or a rung that is not Wiener, n outside 0 .. MGPU_WIENER_BANK_MAX, widths not
 * strictly ascending, a design mgpu_set_estimator_ladder_ex would refuse, a rho_min that is negative or infinite, another entry_size. A
 * refusal leaves the context as it was. Waits for the context's stream; work queued on a caller's stream must have finished. */
int mgpu_set_wiener_bank(mgpu_ctx* ctx, int rung, const mgpu_wiener_bank_entry* e, int n, size_t entry_size);
/* the bank of a rung with the thresholds as applied (the last entry's rho_min as it was given); *n = 0 where the rung has none.
 * e: room for MGPU_WIENER_BANK_MAX. */
int mgpu_get_wiener_bank(mgpu_ctx* ctx, int rung, mgpu_wiener_bank_entry* e, int* n, size_t entry_size);
/* Of rows first .. first + count - 1 (within max_batch) of the last fused span: the design rung 0 chose and the four sums it chose
 * from; n1, n2: the geometry's pair counts. Every output may be NULL. Rung 0 only: retries do not write, as with mgpu_get_cfo_steps and
 * mgpu_get_noise_map, and rows the span did not write keep what an earlier span left (zeros after mgpu_set_wiener_bank).
 * MGPU_ERR_ARG when rung 0 has no bank. Waits for the context's stream. */
int mgpu_get_wiener_choice(mgpu_ctx* ctx, int first, int count, int* design /*[count]*/, double* corr /*[count][4]: R1r R1i R2r R2i*/, int* n1, int* n2);
/* Host twin of the choice, no GPU, and the normative statement of the rule above: one frame grid of the mode `cfg` (p_or_null as for
 * mgpu_host_wiener_estimate) and a bank -> the entry chosen, the four sums and the pair counts; design, corr, n1 and n2 may be NULL.
 * The bank is checked as mgpu_set_wiener_bank checks it (n >= 1). MGPU_ERR_UNSUPPORTED for the zero-forcing and MFSK modes. */
int mgpu_host_wiener_select(int cfg, const mgpu_explicit_params* p_or_null, const mgpu_wiener_bank_entry* e, int n, size_t entry_size,
                            const double* grid_c128 /*[Nsymb*Nc]*/, int* design, double corr[4], int* n1, int* n2);
/* the thresholds a bank would get (NaN entries replaced by their defaults), no GPU: rho_min[n - 1]; pilot_spacing: s, may be NULL */
int mgpu_host_wiener_bank_thresholds(int cfg, const mgpu_explicit_params* p_or_null, const mgpu_wiener_bank_entry* e, int n, size_t entry_size,
                                     double* rho_min /*[n-1]*/, int* pilot_spacing);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_WIENER_BANK_H */

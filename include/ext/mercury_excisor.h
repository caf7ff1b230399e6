/* mercury_excisor.h — the carrier excisor: narrowband carriers are found in a Welch spectrum of the capture window and subtracted from it,
 * ahead of the synchroniser.
 *
 * The commonest HF disturbance is a steady or keyed carrier inside the 2.4 kHz channel: a broadcast carrier, someone tuning up, RTTY, a
 * birdie. The Schmidl-Cox metric, the energy gates and Moose all correlate the capture window with itself, and a carrier is perfectly
 * self-correlated: a tone as strong as the signal keeps receive_byte from ever reaching the decoder, and the stages behind the synchroniser
 * (the noise map of mercury_demapper.h could carry such a carrier) never get to run. A carrier is sparse in frequency over the whole window:
 * the stage finds the bins of the channel that stand far above the band's median power and subtracts exactly those bins' content from the
 * 48 kHz samples. This is NOT one of the reference's configurations: the reference has no such stage.
 *
 * The rule (MGPU_EXCISE_WELCH), per window of n >= 1 real samples x[0 .. n-1] at 48 kHz; mgpu_host_excise below is the normative statement:
 *   constants N = 1024, H = 512, a band of 64 bins; one bin is 46.875 Hz, the OFDM carrier spacing. Two tables are made once on the host by
 *            the host's libm and read by twin and device alike: tab[j] = {cos(a), sin(a)}, a = 2.0 * M_PI * double(j) / 1024.0, j = 0 .. 1023,
 *            and win[i] = sin(M_PI * double(i) / 1024.0), whose square sums to 1 at 50 % overlap;
 *   band     lo = clamp(lround(carrier_hz / 46.875) - 32, 1, 448); the bins are lo .. lo + 63;
 *   blocks   B = ceil(n / H) + 1; block b starts at sample s = (b - 1) * H, so that every sample lies in exactly two blocks;
 *            v[i] = {x[s + i] * win[i], +0.0} where s + i lies inside the window, {+0.0, +0.0} elsewhere;
 *   transform radix-2 decimation in time at 1024 points: a[brev10(i)] = v[i]; for size = 2, 4, .. 1024, half = size / 2, step = 1024 / size,
 *            per group start g and j < half: w = {tab[j * step].re, -tab[j * step].im}, lo_ = a[g + j], hi = a[g + j + half],
 *            t = {w.re * hi.re - w.im * hi.im, w.re * hi.im + w.im * hi.re}, a[g + j] = lo_ + t, a[g + j + half] = lo_ - t. Every product,
 *            sum and difference is rounded on its own, no contraction. A butterfly network has no summation order to choose;
 *   spectrum P_b[k] = re * re + im * im (three roundings) of the 64 band bins; A[k] = the sum of P_b[k] over b, from +0.0, in ascending b;
 *   decision if any A[k] is not finite the window passes byte for byte: nonfinite = 1, exceeding = mask = 0, excised = 0, level = +0.0.
 *            Otherwise level is the A whose key has rank 32 (0-based, ascending) among the 64, the key being the bit pattern without the
 *            sign, compared as an unsigned integer: a selection as in mercury_blanker.h, never an average. Bin k exceeds when
 *            !(A[k] <= threshold * level). mask is the exceeding bins widened by `guard` bins on either side, clipped to the band. If mask
 *            is empty or has more than max_bins bits the output is the input byte for byte and excised = 0: more than max_bins is not a
 *            narrowband problem, and the window is left to the stages that follow;
 *   removal  per block, over the masked bins k in ascending order from +0.0: acc[i] = sum of (X_b[k].re * tab[q].re - X_b[k].im * tab[q].im),
 *            q = (k * i) & 1023; e_b[i] = acc[i] * win[i] * (1.0 / 512.0), from the left; y[n] = x[n] - (e_b0[512 + n % 512] + e_b1[n % 512])
 *            with b0 = n / 512, b1 = b0 + 1. The masked bins' content is subtracted on purpose: no inverse transform of the whole spectrum
 *            happens, and a window with an empty mask is untouched to the bit.
 * The per-window report is mgpu_excisor_report.
 *
 * Parameters: threshold finite and >= 2, default 12 (the highest bin-to-median ratio measured on clean windows of all modes, two equal
 * paths included, was 6.76: profiles/excisor.md); guard 0 .. 4 bins, default 1 (a carrier between two bin centres leaks into its
 * neighbours under the sine window); max_bins 1 .. 32, default 16.
 *
 * Where it holds: at the head of mgpu_receive_byte_batch / _samples, whatever the sample format and wherever the windows lie, and with it
 * mgpu_capture_*, mgpu_capture_run_wideband, mgpu_linksim_* and the passband self-simulations. Every window is excised into a workspace as
 * soon as it has landed on the device, and everything behind reads the cleaned window: the time-sync filter, the coarse and fine searches,
 * the gates, the signal level, the data filter, every trial's decode, the MFSK search. Accepted on every mode.
 * mgpu_measure_signal_only keeps the raw window: it reports what the antenna delivers. mgpu_pool_* does not forward the setting; set it on
 * each mgpu_pool_context.
 * Limits: the mask is static per window (a carrier keyed on and off is removed where it is on and costs the masked bins' signal where it
 * is off); the mask is not fed into the noise map; a mask of more than max_bins bits is not acted on; the device self-simulations have no
 * tone source. The masked bins' share of the signal is removed with the carrier (4 of 50 carriers: 0.35 dB): a window that close to the
 * reference's absolute energy gate falls under it.
 * Off by default (MGPU_EXCISE_OFF): nothing is launched and every entry point computes what it computed before, with the same kernels.
 *
 * This header lives under include/ext/: the prototypes under include/ itself are a closed set, and what is added to the ABI later goes here
 * (INTEGRATION.md).
 */
#ifndef MERCURY_EXCISOR_H
#define MERCURY_EXCISOR_H

#include <stddef.h>
#include <stdint.h>

#include "../mercury_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGPU_EXCISE_OFF 0     /* the reference's receiver: the synchroniser reads the capture window as it is */
#define MGPU_EXCISE_WELCH 1   /* the rule above */

typedef struct mgpu_excisor_params {
    double threshold;         /* finite, >= 2: a bin exceeds above threshold * the band's median summed power. Default 12 */
    int guard;                /* 0..4 bins on either side of an exceeding bin are masked with it. Default 1 */
    int max_bins;             /* 1..32: a window whose mask has more bits passes unchanged. Default 16 */
} mgpu_excisor_params;
#define MGPU_EXCISOR_PARAMS_DEFAULT {12.0, 1, 16}

typedef struct mgpu_excisor_report {
    uint64_t exceeding;       /* bit i: bin band_lo + i exceeds */
    uint64_t mask;            /* exceeding, widened by the guard */
    int band_lo;              /* the band's first bin */
    int excised;              /* bins removed: the mask's population, or 0 where the window passed unchanged */
    int nonfinite;            /* 1: a summed power was not finite and the window passed unchanged */
    double level;             /* the band's median summed power (+0.0 with nonfinite) */
} mgpu_excisor_report;

/* mode: MGPU_EXCISE_OFF or MGPU_EXCISE_WELCH, on every mode of the receiver. params (read for MGPU_EXCISE_WELCH only; NULL: the defaults);
 * params_size must be sizeof(mgpu_excisor_params). MGPU_ERR_ARG for another mode value, another params_size, or a parameter outside the
 * ranges above (NaN included). MGPU_EXCISE_WELCH allocates the report array of max_batch rows; the workspace of the cleaned windows (8 bytes
 * per sample of the call's windows) is made by the first mgpu_receive_byte_batch call and released by MGPU_EXCISE_OFF. A refusal leaves
 * the context as it was. Waits for the context's stream; work queued on a caller's stream must have finished.
 * mgpu_get_excisor returns the mode and the parameters last set (the defaults before). */
int mgpu_set_excisor(mgpu_ctx* ctx, int mode, const mgpu_excisor_params* params_or_null, size_t params_size);
int mgpu_get_excisor(mgpu_ctx* ctx, int* mode, mgpu_excisor_params* params, size_t params_size);

/* The reports of rows first .. first + count - 1 (first + count <= max_batch) of the last mgpu_receive_byte_batch call (or one built on it)
 * that ran with MGPU_EXCISE_WELCH, by the window's row in that call. Rows the call did not write keep what an earlier call left there (0
 * after mgpu_set_excisor). Waits for the context's stream. MGPU_ERR_ARG before the mode was ever set. */
int mgpu_get_excisor_report(mgpu_ctx* ctx, int first, int count, mgpu_excisor_report* report /*[count]*/);

/* The stage on its own, on device buffers: W dense windows of n >= 1 doubles each in d_in, into d_out [W][n], which must not overlap d_in;
 * the reports, if wanted, into d_report [W]. carrier_hz (finite, 1e9 at most in magnitude) places the band. Works whether or not the mode is set, with the parameters
 * last set (the defaults before). Queued on `stream` (NULL: the default stream); does not wait. It uses a spectrum workspace of the
 * context: calls on one context do not overlap on different streams, nor with mgpu_receive_byte_batch while the mode is on. */
int mgpu_excise_dev(mgpu_ctx* ctx, const double* d_in, int W, int n, double carrier_hz, double* d_out, void* d_report_or_null, void* stream_or_null);

/* Host twin of the rule above, no GPU: one window. params NULL: the defaults. out may be in. report may be NULL. MGPU_ERR_ARG for n < 1 or above 2^30, a
 * carrier_hz that is not finite or above 1e9 in magnitude, or refused parameters. */
int mgpu_host_excise(const mgpu_excisor_params* params_or_null, double carrier_hz, const double* in /*[n]*/, int n, double* out /*[n]*/,
                     mgpu_excisor_report* report);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_EXCISOR_H */

/* mercury_tuner.h — a carrier tuner: the channels of a found plan onto their stations to the hertz.
 *
 * The band scanner (mercury_scanner.h) finds a station to about one bin; receive_byte needs the channel planned to about a hertz. The tuner
 * is the stage that knows the signal. Mercury's OFDM geometry is the same in all 17 OFDM modes: Nfft = 256 at 12 kHz (carrier spacing
 * 46.875 Hz), Ngi = 16 (a symbol is 272 baseband samples), 50 carriers on the FFT bins -25..-1 and 1..25 around an empty DC. From one
 * block of wideband IQ the tuner measures, per planned channel, how far the station is off the plan: the angle of the cyclic-prefix
 * correlation gives the fraction of a carrier spacing, the position of the 50-carrier comb with its DC hole the whole spacings. The tuner
 * is stateless: a call is one measurement on one block and stands alone. The device's result is bit for bit the host twin's,
 * mgpu_host_tune_process. This is NOT one of the reference's configurations.
 *
 * The rule (normative; the twin implements exactly this).
 *   Configuration: D = 1..64, the rate is R = 48000 * D; S >= 1 channels, each one the channeliser accepts at (D, a_c);
 *   a_c = audio_centre_hz = 1..23999; carrier_hz finite, > 0 and < 24000 (MGPU_TUNE_DEFAULT_CARRIER_HZ); the prototype taps / ntaps as
 *   mgpu_chan_config's (NULL: the channeliser's default design); J = symbols = 4..256; K = search = 0..24; min_metric finite, > 0 and <= 1.
 *   Anything else is refused with MGPU_ERR_ARG before any device work.
 *   Input: exactly n_in = 4 * D * M IQ samples, M = 272 * (J + 1), widened as the channeliser widens them (CS16: / 32768.0), {+0.0, +0.0}
 *   before the block's start. Any other n_in is MGPU_ERR_ARG.
 *   Stage 1, the channel at 12 kHz. z_s[m], m < M, is the channeliser's accumulator pair (re, im) of channel s at output n = 4 m of a
 *     stream that starts with the block: the same tables g_s, the same chain of fused multiply-adds in ascending k
 *     (mercury_channelizer.h), the audio remix and the gain left off. The tap row is a band-pass around F = offset_hz + sigma * a_c
 *     (sigma = +1 USB / -1 LSB), not a mixer: a station planned exactly lies in z at F mod 12000 Hz. The stages below take the integer F
 *     out again, exactly: the angle it adds to a lag of 256 samples is (8 F mod 375) / 375 turns, and W turns by whole hertz.
 *   Stage 2, the cyclic prefix. With a = z[m], b = z[m + 256]:
 *       p[m] = {a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im}                       (= a * conj(b))
 *       e[m] = 0.5 * ((a.re * a.re + a.im * a.im) + (b.re * b.re + b.im * b.im))
 *     and for phi = 0..271: G[phi] = sum over j < J of ( sum over i < 16 of p[272 j + phi + i] ), per component, E[phi] likewise from
 *     e. The inner sum runs from +0.0 in ascending i, the outer from +0.0 in ascending j. Every product, sum and difference is rounded
 *     on its own, no contraction.
 *   Between the stages, on the host with the host's libm (the twin and the device path run the same code):
 *     if any G or E of the channel is not finite: the report is {nonfinite = 1, valid = 0, offset_hz the planned one, the rest zeros},
 *       and stage 3 runs with phi* = 0 and r = 0 (its Q is not read).
 *     phi* = the first phi of the greatest G.re * G.re + G.im * G.im under `>`;
 *     metric = sqrt(G.re * G.re + G.im * G.im) / E at phi*, +0.0 where that E is not > 0. It lies in [0, 1] up to rounding.
 *     raw = (-atan2(G.im, G.re) * 12000.0) / (2.0 * M_PI * 256.0);   frac_hz = raw - double((8 F) mod 375) / 8.0 (floor-mod), and
 *       frac_hz + 46.875 where that is < -23.4375: the station's distance from F modulo the carrier spacing;   r = lround(frac_hz).
 *   Stage 3, the comb. For j < J take the 256 samples z[m], m = b_j + i, b_j = 272 j + phi* + 8 (the useful part, begun in the middle of
 *     the prefix), turned to v[i] = {z.re * w.re + z.im * w.im, z.im * w.re - z.re * w.im}, w = W[(4 * (F + r) * m) mod 48000]
 *     (floor-mod; W the channeliser's phasor table), transformed by the scanner's transform at N = 256 (mercury_scanner.h: same table,
 *     same butterflies) into U_j[k]. Q[k] = the sum over j of (U.re * U.re + U.im * U.im), from +0.0 in ascending j.
 *   Host again:
 *     score(d) = the sum of Q[(c + d) mod 256] over c = -25..-1, 1..25 in this order from +0.0, for d = -K..K;
 *     shift = the first d of the greatest score under `>`; contrast = that score / the greatest score among the other d where that one
 *     is > 0, else +0.0;
 *     delta_hz = double(shift) * 46.875 + ((frac_hz - double(r)) + double(r));
 *     offset_hz' = lround((double(offset_hz) + delta_hz) - sigma * (carrier_hz - double(a_c)));
 *     if any Q is not finite the report is the nonfinite one. Otherwise valid = metric >= min_metric and the channeliser accepts
 *     {offset_hz', sideband, gain}; the report's offset_hz is offset_hz' where valid, the planned one where not.
 *
 * The default min_metric is measured, not chosen: over 1024 blocks of white Gaussian CF64 noise at the default configuration (D = 1) the
 * highest metric the twin saw was 0.2926 (profiles/tuner.md); times 1.5 is 0.4389, rounded up to two decimals: 0.44.
 *
 * Limits: OFDM modes only (an MFSK station has no cyclic prefix and comes back not valid); one measurement per call, nothing is tracked;
 * a displacement beyond the prototype's passband is decided on a truncated comb: with the default taps the decision was measured to hold
 * over the whole range of `search`, |delta| <= 24 * 46.875 = 1125 Hz (profiles/tuner.md); fading is unmeasured. mgpu_pool_* does not forward the stage.
 *
 * Errors as mercury_gpu.h. The context rules of INTEGRATION.md §2 apply: a tuner belongs to its context, is used by one thread at a
 * time with it and is destroyed before it.
 *
 * This header lives under include/ext/: the prototypes under include/ itself are a closed set.
 */
#ifndef MERCURY_TUNER_H
#define MERCURY_TUNER_H

#include <stddef.h>
#include <stdint.h>

#include "../mercury_channelizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGPU_TUNE_NFFT 256
#define MGPU_TUNE_SYMBOL 272                    /* Nfft + Ngi */
#define MGPU_TUNE_MIN_SYMBOLS 4
#define MGPU_TUNE_MAX_SYMBOLS 256
#define MGPU_TUNE_DEFAULT_SYMBOLS 32
#define MGPU_TUNE_MAX_SEARCH 24
#define MGPU_TUNE_DEFAULT_SEARCH 8
#define MGPU_TUNE_DEFAULT_CARRIER_HZ 1471.875
#define MGPU_TUNE_DEFAULT_MIN_METRIC 0.44

typedef struct mgpu_tune mgpu_tune;

typedef struct mgpu_tune_config {
    int struct_size;        /* = sizeof(mgpu_tune_config), else MGPU_ERR_ARG (versioned by size, as mgpu_scan_config) */
    int D;                  /* 1..64: the rate is 48000 * D */
    int S;                  /* channels, >= 1 */
    int audio_centre_hz;    /* a_c, 1..23999 (MGPU_CHAN_DEFAULT_AUDIO_CENTRE_HZ) */
    int ntaps;              /* T of `taps`; ignored when taps is NULL */
    int symbols;            /* J, 4..256 (MGPU_TUNE_DEFAULT_SYMBOLS) */
    const double* taps;     /* the prototype h[T] as mgpu_chan_config's; NULL: the channeliser's default design */
    double carrier_hz;      /* the audio carrier the station sends on (MGPU_TUNE_DEFAULT_CARRIER_HZ) */
    double min_metric;      /* (0, 1] (MGPU_TUNE_DEFAULT_MIN_METRIC) */
    int search;             /* K carriers, 0..24 (MGPU_TUNE_DEFAULT_SEARCH) */
    int pad;
} mgpu_tune_config;

typedef struct mgpu_tune_report {
    double metric;          /* |G| / E at phi* */
    double frac_hz;         /* the fraction of a carrier spacing, -23.4375..23.4375 */
    double delta_hz;        /* the station's centre minus the planned channel's centre F */
    double contrast;        /* the best comb score over the second best */
    int phase;              /* phi*, 0..271: where a symbol's prefix begins in the block, modulo 272 */
    int shift;              /* the comb's position, -K..K carriers */
    int offset_hz;          /* the refined offset where valid, else the planned one */
    int valid;
    int nonfinite;          /* 1: a G, E or Q was not finite */
    int pad;
} mgpu_tune_report;

/* channels: [S], the plan to refine. Without a context (no device could be opened) a valid configuration gives MGPU_ERR_DEVICE, a bad
 * one MGPU_ERR_ARG. */
int mgpu_tune_create(mgpu_ctx* ctx, const mgpu_tune_config* config, const mgpu_chan_channel* channels, mgpu_tune** out);
int mgpu_tune_destroy(mgpu_tune* tn);
/* another planned channel s from the next call on: rebuilds its tap row */
int mgpu_tune_retune(mgpu_tune* tn, int s, const mgpu_chan_channel* channel);
/* n_in = 4 * D * 272 * (J + 1); < 0 for a null handle */
int mgpu_tune_samples(mgpu_tune* tn);
/* n_in IQ samples in `format` (MGPU_IQ_*) in host or device memory (detected) -> reports [S] in host memory. Blocks. */
int mgpu_tune_process(mgpu_tune* tn, const void* iq, int format, int n_in, mgpu_tune_report* reports);
/* the last call's device results, for tests and for plotting: G [S][272] complex (re, im), E [S][272], Q [S][256], each NULL or host
 * memory. MGPU_ERR_ARG before the first call. */
int mgpu_tune_arrays(mgpu_tune* tn, double* G, double* E, double* Q);

/* Host only, no GPU needed.
 * mgpu_host_tune_process: the twin: reports [S] and, where not NULL, G [S][272] complex, E [S][272], Q [S][256].
 * mgpu_host_tune_plan: the refined channel of a report: *channel with the report's offset_hz; sideband and gain are kept (the offset
 *   too where the report is not valid, whose offset_hz is the planned one). */
int mgpu_host_tune_process(const mgpu_tune_config* config, const mgpu_chan_channel* channels, const void* iq, int format, int n_in,
                           mgpu_tune_report* reports, double* G, double* E, double* Q);
int mgpu_host_tune_plan(const mgpu_tune_report* report, const mgpu_chan_channel* channel, mgpu_chan_channel* refined);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_TUNER_H */

/* mercury_channel.h — a Watterson HF fading channel (CCIR Rec. 520 / ITU-R F.1487) for the GPU self-simulations.
 *
 * The reference can only simulate AWGN (cl_awgn, awgn.cc). This header adds the standard ionospheric channel model beside it, as a
 * batched GPU stage and as a channel option of the two BER loops (mgpu_baseband_test_esn0, mgpu_passband_test_esn0). The model is
 * defined exactly in DESIGN.md §6.1; in short, for W independent signals of n samples at sample rate fs:
 *
 *   a      = x + j (h * x)         real input (h: odd-length antisymmetric Hilbert FIR, mgpu_host_hilbert_taps; samples outside
 *                                  [0, n) are zero); a = x for complex input
 *   y_c[i] = e^{j 2 pi df t_i} sum_k g_k(t_i) a[i - d_k],   t_i = (t0 + i) / fs,  d_k = round(delay_ms_k * fs / 1000)
 *   y      = Re(y_c) for real input, y_c for complex input; the length stays n
 *   g_k(t) = 10^(gain_db_k / 20) u_k(t) / sqrt(sum_j 10^(gain_db_j / 10))          (mean power kept: Es/N0 is the mean Es/N0)
 *   u_k(t) = e^{j 2 pi shift_k t}                                                  spread_k == 0 (static path, phase 0)
 *          = N^-1/2 sum_{m<N} exp(j (2 pi f_km t + phi_km)),  N = 32,
 *            f_km = shift_k + (spread_k / 2) z,  z ~ N(0,1),  phi_km ~ U[0, 2 pi)  otherwise
 *
 * The draws (z, phi) of realisation r are keyed by (seed, r, k, m) on Philox4x32 stream 4. Over the ensemble the sum of random-frequency
 * sinusoids has exactly the Gaussian-spectrum autocorrelation E[u(t+tau) u*(t)] = e^{j 2 pi shift tau} exp(-pi^2 spread^2 tau^2 / 2):
 * "spread" is two standard deviations of the Doppler power spectrum (the F.1487 convention). Each realisation depends on (seed, r)
 * alone, never on the batch it runs in. The identity channel (one path, 0 dB, delay 0, spread 0, shift 0, freq_offset 0) returns its
 * input bit for bit.
 */
#ifndef MERCURY_CHANNEL_H
#define MERCURY_CHANNEL_H

#include <stdint.h>

#include "mercury_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGPU_HF_MAX_PATHS 4
#define MGPU_HF_SINUSOIDS 32
#define MGPU_HF_MAX_DELAY_MS 10.0

typedef struct mgpu_hf_channel {
    int struct_size;                        /* = sizeof(mgpu_hf_channel), else MGPU_ERR_ARG (the layout is versioned by its size) */
    int n_paths;                            /* 1..MGPU_HF_MAX_PATHS */
    double delay_ms[MGPU_HF_MAX_PATHS];     /* 0..10 ms */
    double gain_db[MGPU_HF_MAX_PATHS];      /* relative; the path gains are normalised to unit total power */
    double spread_hz[MGPU_HF_MAX_PATHS];    /* 2 sigma of the Gaussian Doppler spectrum, >= 0 (0: static path) */
    double shift_hz[MGPU_HF_MAX_PATHS];     /* Doppler shift of the path */
    double freq_offset_hz;                  /* whole-signal frequency offset */
} mgpu_hf_channel;

/* presets (values and source) */
#define MGPU_HF_AWGN 0       /* identity */
#define MGPU_HF_GOOD 1       /* CCIR 520 "good": 2 equal paths, 0.5 ms, 0.1 Hz */
#define MGPU_HF_MODERATE 2   /* "moderate": 2 equal paths, 1 ms, 0.5 Hz */
#define MGPU_HF_POOR 3       /* "poor": 2 equal paths, 2 ms, 1 Hz */
#define MGPU_HF_FLUTTER 4    /* "flutter": 2 equal paths, 0.5 ms, 10 Hz */

/* ---- host only (no GPU, no context): the definitions the device code is tested against ------------------------------------- */
int mgpu_hf_channel_preset(int which, mgpu_hf_channel* out);
/* the Hilbert FIR of the real-input model: taps[0..ntaps-1] (centre ntaps/2, room for 512 doubles) */
int mgpu_host_hilbert_taps(double* taps, int* ntaps);
/* the draws of path `path` of realisation `realisation`: freq_hz[m] = shift + spread/2 z_m, phase[m] = phi_m (rad), m < 32. A static
 * path (spread 0) has one sinusoid: freq_hz[0] = shift, phase[0] = 0, and NaN in the 31 other entries. freq_offset_hz is not included. */
int mgpu_host_hf_channel_draws(const mgpu_hf_channel* ch, uint64_t seed, uint64_t realisation, int path, double* freq_hz, double* phase);
/* g_k(t_i) of realisation `realisation` for i < n, t_i = (t0 + i) / fs, normalised, without freq_offset_hz: [n_paths][n] complex128 */
int mgpu_host_hf_channel_taps(const mgpu_hf_channel* ch, double fs, uint64_t seed, uint64_t realisation, long long t0, int n, double* g_c128);

/* ---- on the GPU ---------------------------------------------------------------------------------------------------------------
 * W signals of n samples ([W][n] doubles, complex_input = 0; [W][n] complex128, complex_input = 1) through the channel; signal w is
 * realisation realisation0 + w; out has the layout of in (it may not alias in). fs: 1..192000 Hz. Host buffers, blocking. */
int mgpu_hf_channel_apply(mgpu_ctx* ctx, const mgpu_hf_channel* ch, const void* in, int complex_input, double fs, int W, int n,
                          uint64_t seed, uint64_t realisation0, long long t0, void* out);
/* the same on device buffers, enqueued on `stream` (NULL: the context's stream), asynchronous */
int mgpu_hf_channel_apply_dev(mgpu_ctx* ctx, const mgpu_hf_channel* ch, const void* d_in, int complex_input, double fs, int W, int n,
                              uint64_t seed, uint64_t realisation0, long long t0, void* d_out, void* stream);

/* ---- streaming form -------------------------------------------------------------------------------------------
 * A stateful channel for S real signals that are fed in chunks, so that a long run needs memory for one chunk only and a chunk edge is
 * no discontinuity. Let x_s be everything fed to signal s, placed from the seek position on and zero before it, and y_s the output
 * defined above for real input, t0 = 0 and realisation realisation0 + s, taken on the unbounded signal (the Hilbert FIR sees the real
 * neighbours at a chunk edge). The output at absolute position T is
 *
 *   o_s[T] = y_s[T - L] + noise_amp[s] * g(seed, s, T)          (y_s[u] = 0 for u < 0),   L = mgpu_hf_stream_latency() = 256
 *
 * The Hilbert FIR reaches 215 samples ahead, so some latency is unavoidable; 256 keeps the kernel's 64-sample blocks aligned with
 * absolute time, and chunks whose edges lie on multiples of 64 give, bit for bit, the doubles one piece gives (and those
 * mgpu_hf_channel_apply gives on the whole signal). g is a standard normal draw of Philox stream 5 whose counter carries the signal index
 * and all 64 bits of T (mgpu_host_hf_stream_noise is its host twin). noise_amp == NULL adds nothing and draws nothing. The identity
 * channel returns its input delayed by L, bit for bit. A stream belongs to its context and is destroyed before it. */
typedef struct mgpu_hf_stream mgpu_hf_stream;
int mgpu_hf_stream_create(mgpu_ctx* ctx, const mgpu_hf_channel* ch, double fs, int S, uint64_t seed, uint64_t realisation0, mgpu_hf_stream** out);
int mgpu_hf_stream_destroy(mgpu_hf_stream* st);
/* position: a multiple of 64; the history becomes zeros. A new stream is at 0. */
int mgpu_hf_stream_seek(mgpu_hf_stream* st, uint64_t position);
int mgpu_hf_stream_latency(mgpu_hf_stream* st);
/* n more samples of every signal, n a positive multiple of 64 (else MGPU_ERR_ARG and nothing changes): [S][n] doubles in, [S][n] out, no
 * aliasing. noise_amp: NULL or [S] host doubles. Host buffers, blocking. */
int mgpu_hf_stream_apply(mgpu_hf_stream* st, const double* in, int n, const double* noise_amp, double* out);
/* the same on device buffers, enqueued on `stream` (NULL: the context's stream), asynchronous; d_in is read until the call's work is done */
int mgpu_hf_stream_apply_dev(mgpu_hf_stream* st, const void* d_in, int n, const double* noise_amp, void* d_out, void* stream);
/* host only: g(seed, signal, position + i) for i < n */
int mgpu_host_hf_stream_noise(uint64_t seed, int signal, uint64_t position, int n, double* out);

/* mgpu_passband_test_esn0 (mercury_rxloop.h) with the channel between the transmitter and the noise: each capture window (randomly
 * picked leading samples, the frame, zeros behind it) goes through the channel at 48 kHz, realisation = frame number, t0 = 0, and then
 * gets the same noise samples mgpu_passband_test_esn0 adds. The MFSK modes keep their sigma calibrated on the transmitted power and
 * the known frame position (mfsk_fixed_delay). With the identity channel every output equals mgpu_passband_test_esn0's bit for bit. */
int mgpu_passband_test_esn0_hf(mgpu_ctx* ctx, const double* esn0_db, int npoints, long long frames_per_point, uint64_t seed, uint64_t frame0,
                               double carrier_hz, double output_power_watt, const mgpu_hf_channel* ch, mgpu_error_rate* out,
                               double* windows_out, uint8_t* sent_out);
/* mgpu_baseband_test_esn0 (mercury_gpu.h) with the channel on the 12 kHz complex frame (realisation = frame number, t0 = 0) before the
 * same noise samples; with the identity channel the records equal mgpu_baseband_test_esn0(channel = 0)'s. */
int mgpu_baseband_test_esn0_hf(mgpu_ctx* ctx, const double* esn0_db, int npoints, long long frames_per_point, uint64_t seed, uint64_t frame0,
                               const mgpu_hf_channel* ch, mgpu_error_rate* out);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_CHANNEL_H */

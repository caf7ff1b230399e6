// Watterson HF fading channel (CCIR Rec. 520 / ITU-R F.1487) for the self-simulations: model and C-ABI in include/mercury_channel.h,
// definition and cost model in DESIGN.md §6.1 (§6.2 for the streaming form). Five kernels share one body:
//   mgpu_hf_channel_real_kernel      real signals [W][n] (analytic signal through the Hilbert FIR, Re() of the output)
//   mgpu_hf_channel_complex_kernel   complex signals [W][n]
//   mgpu_hf_passband_kernel          the capture windows of passband_test_esn0 built on the fly (mgpu_passband_channel_kernel's leading
//                                    random picks, the frame, zeros) -> channel -> the same Philox stream-3 noise sample that kernel adds
//   mgpu_hf_baseband_kernel          clean 12 kHz frames of the generator -> channel -> the generator's stream-1 noise, (x/16 + a n) 16
//   mgpu_hf_stream_kernel            real signals fed in chunks (mgpu_hf_stream_*): the input is a per-signal history tail followed by the
//                                    chunk, the output is delayed by HF_LATENCY samples and gets Philox stream-5 noise keyed by the 64-bit
//                                    absolute position
// One workgroup = one tile of HF_TILE output samples of one signal. The tile's input plus its halo (the largest path delay behind it,
// for real input also the Hilbert FIR's half length on both sides) is staged in LDS once. Tap gains are not interpolated: sinusoid m of
// path k at sample i0 + 64 b + l is A[b][m] * E[m][l & 7] * F[m][l >> 3], with the anchor A (one sincos per 64-sample block) and the
// in-block rotations E, F = e^{j 2 pi f (l & 7) / fs}, e^{j 2 pi f 8 (l >> 3) / fs} from sincos as well: no recurrence, every factor
// within a few ulp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/mercury_channel.h"
#include "ctx.hpp"
#include "philox.h"

#define HF_THREADS 256
#define HF_TILE 1024                            // output samples per workgroup
#define HF_BLK 64                               // samples per anchor block (one wave's lanes)
#define HF_NBLK (HF_TILE / HF_BLK)              // 16
#define HF_PER_THREAD (HF_TILE / HF_THREADS)    // 4: lane l of wave v handles blocks v, v + 4, v + 8, v + 12
#define HF_HILBERT_HALF 215                     // Hilbert FIR: offsets -215..215 (431 taps), non-zero at odd offsets only
#define HF_HILBERT_ODD 108
#define HF_STREAM 4u                            // Philox stream id of the channel draws (philox.h)
#define HF_NOISE_STREAM 5u                      // Philox stream id of the streaming channel's noise
#define HF_LATENCY 256                          // streaming form: output delay in samples (>= HF_HILBERT_HALF, a multiple of HF_BLK)
#define HF_MAX_FS 192000.0
#define HF_MAX_DELAY int(MGPU_HF_MAX_DELAY_MS * HF_MAX_FS / 1000.0)     // 1920 samples

namespace {

struct cd { double re, im; };

enum { HF_REAL = 0, HF_COMPLEX = 1, HF_PASSBAND = 2, HF_BASEBAND = 3, HF_STREAMING = 4 };

// everything the kernels need of a channel, resolved on the host: integer delays, normalised amplitudes (1/sqrt(N) included)
struct HfPlan {
    int P, identity, dmax, pad;
    int delay[MGPU_HF_MAX_PATHS], ns[MGPU_HF_MAX_PATHS];       // ns: 32 sinusoids (fading) or 1 (static path)
    double amp[MGPU_HF_MAX_PATHS], shift[MGPU_HF_MAX_PATHS], half_spread[MGPU_HF_MAX_PATHS];
    double foff, fs;
    long long t0;
    uint64_t seed, real0;
    double hil[HF_HILBERT_ODD];                                 // h at offsets 1, 3, ..., 215 (h(-o) = -h(o))
};

struct HfIo {
    const double* in;   // HF_REAL [W][n]; HF_COMPLEX / HF_BASEBAND [W][n] complex; HF_PASSBAND the transmitted audio [W][total]
    double* out;        // [W][n] (complex for HF_COMPLEX / HF_BASEBAND)
    int n, w0;          // samples per signal; first signal of this launch
    int total, delay;   // HF_PASSBAND: audio samples per frame, frame position in the window
    double noise;       // HF_PASSBAND: ampl (awgn.cc:68); HF_BASEBAND: noise_amp per component
    // HF_STREAMING: in is the chunk [W][n]; output sample i is the channel's output at chunk sample i - HF_LATENCY
    const double* hist;         // [W][nh] the nh samples fed before the chunk (zeros where nothing was fed)
    const double* noise_amp;    // NULL (no noise, no draws) or [W]
    int nh, fed;                // history length; samples fed since the seek before this chunk (clamped): older input is zero
    uint64_t pos;               // absolute position of the chunk's first sample
};

// ---- host: the definitions ------------------------------------------------------------------------------------------------------

double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= (x / (2.0 * k)) * (x / (2.0 * k));
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// ideal Hilbert transformer 2 / (pi n) at odd n, Kaiser window beta = 7: |1 - |H|| <= 5.2e-4 from 250 Hz to 23.75 kHz at 48 kHz
const std::vector<double>& hilbert_full() {
    static const std::vector<double> h = [] {
        const int M = HF_HILBERT_HALF;
        const double beta = 7.0, i0b = bessel_i0(beta);
        std::vector<double> t(2 * M + 1, 0.0);
        for (int n = -M; n <= M; ++n) {
            if ((n & 1) == 0) continue;
            const double r = double(n) / M;
            t[n + M] = 2.0 / (M_PI * n) * bessel_i0(beta * std::sqrt(1.0 - r * r)) / i0b;
        }
        return t;
    }();
    return h;
}

const char* channel_error(const mgpu_hf_channel* ch) {
    if (!ch) return "no channel";
    if (ch->struct_size != int(sizeof(mgpu_hf_channel))) return "mgpu_hf_channel.struct_size is not sizeof(mgpu_hf_channel)";
    if (ch->n_paths < 1 || ch->n_paths > MGPU_HF_MAX_PATHS) return "n_paths must be 1..MGPU_HF_MAX_PATHS";
    for (int k = 0; k < ch->n_paths; ++k) {
        if (!std::isfinite(ch->delay_ms[k]) || ch->delay_ms[k] < 0 || ch->delay_ms[k] > MGPU_HF_MAX_DELAY_MS) return "path delay must be 0..10 ms";
        if (!std::isfinite(ch->gain_db[k]) || std::fabs(ch->gain_db[k]) > 100.0) return "path gain must be finite, within +-100 dB";
        if (!std::isfinite(ch->spread_hz[k]) || ch->spread_hz[k] < 0) return "Doppler spread must be finite and >= 0";
        if (!std::isfinite(ch->shift_hz[k])) return "Doppler shift must be finite";
    }
    if (!std::isfinite(ch->freq_offset_hz)) return "frequency offset must be finite";
    return nullptr;
}

// normalised amplitude of path k's sinusoids (1/sqrt(N) for a fading path)
double path_amp(const mgpu_hf_channel* ch, int k) {
    double p = 0;
    for (int j = 0; j < ch->n_paths; ++j) p += std::pow(10.0, ch->gain_db[j] / 10.0);
    const double a = std::pow(10.0, ch->gain_db[k] / 20.0) / std::sqrt(p);
    return ch->spread_hz[k] > 0 ? a / std::sqrt(double(MGPU_HF_SINUSOIDS)) : a;
}

int path_delay(const mgpu_hf_channel* ch, int k, double fs) { return int(std::lround(ch->delay_ms[k] * fs / 1000.0)); }

// sinusoid m of fading path k, realisation r: (frequency without the offset, phase)
void draw(const mgpu_hf_channel* ch, uint64_t seed, uint64_t r, int k, int m, double* f, double* phi) {
    uint32_t w[4];
    philox4x32(seed, uint32_t(k * MGPU_HF_SINUSOIDS + m), HF_STREAM, uint32_t(r), uint32_t(r >> 32), w);
    *f = ch->shift_hz[k] + 0.5 * ch->spread_hz[k] * gauss_bm(w[0], w[1]);
    *phi = 2.0 * M_PI * (double(w[2]) * (1.0 / 4294967296.0));
}

HfPlan make_plan(const mgpu_hf_channel* ch, double fs, long long t0, uint64_t seed, uint64_t real0) {
    if (const char* e = channel_error(ch)) throw std::invalid_argument(e);
    need(std::isfinite(fs) && fs >= 1.0 && fs <= HF_MAX_FS, "sample rate must be 1..192000 Hz");
    HfPlan p{};
    p.P = ch->n_paths;
    for (int k = 0; k < p.P; ++k) {
        p.delay[k] = path_delay(ch, k, fs);
        p.dmax = std::max(p.dmax, p.delay[k]);
        p.ns[k] = ch->spread_hz[k] > 0 ? MGPU_HF_SINUSOIDS : 1;
        p.amp[k] = path_amp(ch, k);
        p.shift[k] = ch->shift_hz[k];
        p.half_spread[k] = 0.5 * ch->spread_hz[k];
    }
    p.foff = ch->freq_offset_hz;
    p.fs = fs;
    p.t0 = t0;
    p.seed = seed;
    p.real0 = real0;
    p.identity = p.P == 1 && p.delay[0] == 0 && p.ns[0] == 1 && p.shift[0] == 0.0 && p.foff == 0.0 && p.amp[0] == 1.0;
    const std::vector<double>& h = hilbert_full();
    for (int o = 0; o < HF_HILBERT_ODD; ++o) p.hil[o] = h[HF_HILBERT_HALF + 2 * o + 1];
    return p;
}

size_t lds_bytes(const HfPlan& p, bool real_in) {
    size_t b = size_t(HF_NBLK) * 32 * 16 + 2 * 32 * 8 * 16 + 2 * MGPU_HF_MAX_PATHS * 32 * 8;       // A, E, F, draws
    b += size_t(HF_TILE + p.dmax) * 16;                                                             // analytic signal + delay halo
    if (real_in) b += size_t(HF_TILE + p.dmax + 2 * HF_HILBERT_HALF) * 8;                          // real input + FIR halo
    return b;
}

// ---- device ----------------------------------------------------------------------------------------------------------------------

// input sample i of signal w (zero outside [0, n)); HF_PASSBAND builds mgpu_passband_channel_kernel's window before its noise
template <int MODE>
__device__ __forceinline__ cd source(const HfPlan& pl, const HfIo& io, int w, int i) {
    if (MODE == HF_STREAMING) {                 // chunk sample i - HF_LATENCY: from the history tail when it lies before the chunk
        const int j = i - HF_LATENCY;
        if (j >= io.n || j < -io.nh) return {0.0, 0.0};
        return {j < 0 ? io.hist[size_t(w) * io.nh + (io.nh + j)] : io.in[size_t(w) * io.n + j], 0.0};
    }
    if (i < 0 || i >= io.n) return {0.0, 0.0};
    if (MODE == HF_REAL) return {io.in[size_t(w) * io.n + i], 0.0};
    if (MODE == HF_COMPLEX || MODE == HF_BASEBAND) {
        const double* p = io.in + 2 * (size_t(w) * io.n + i);
        return {p[0], p[1]};
    }
    const double* a = io.in + size_t(w) * io.total;
    if (i >= io.delay + io.total) return {0.0, 0.0};
    if (i >= io.delay) return {a[i - io.delay], 0.0};
    const uint64_t fr = pl.real0 + uint64_t(w);
    uint32_t r[4];
    philox4x32(pl.seed, uint32_t(i), 3u, uint32_t(fr), uint32_t(fr >> 32), r);
    return {a[r[2] % uint32_t(io.total)], 0.0};
}

template <int MODE>
__device__ __forceinline__ void emit(const HfPlan& pl, const HfIo& io, int w, int i, cd y) {
    if (MODE == HF_REAL) { io.out[size_t(w) * io.n + i] = y.re; return; }
    if (MODE == HF_COMPLEX) { double* o = io.out + 2 * (size_t(w) * io.n + i); o[0] = y.re; o[1] = y.im; return; }
    if (MODE == HF_STREAMING) {                // noise keyed by (signal, 64-bit absolute position): no wrap at 2^32 samples
        double v = y.re;
        if (io.noise_amp) {
            const uint64_t T = io.pos + uint64_t(i);
            uint32_t q[4];
            philox4x32(pl.seed, uint32_t(T), HF_NOISE_STREAM, uint32_t(T >> 32), uint32_t(w), q);
            v += io.noise_amp[w] * gauss_bm(q[0], q[1]);
        }
        io.out[size_t(w) * io.n + i] = v;
        return;
    }
    const uint64_t fr = pl.real0 + uint64_t(w);
    uint32_t r[4];
    if (MODE == HF_PASSBAND) {                 // mgpu_passband_channel_kernel's noise: stream 3, counter (sample, frame)
        philox4x32(pl.seed, uint32_t(i), 3u, uint32_t(fr), uint32_t(fr >> 32), r);
        io.out[size_t(w) * io.n + i] = y.re + io.noise * gauss_bm(r[0], r[1]);
        return;
    }
    philox4x32(pl.seed, uint32_t(i), 1u, uint32_t(fr), uint32_t(fr >> 32), r);     // mgpu_txgen_kernel's noise: stream 1
    const double nr = io.noise * gauss_bm(r[0], r[1]), ni = io.noise * gauss_bm(r[2], r[3]);
    double* o = io.out + 2 * (size_t(w) * io.n + i);
    o[0] = (y.re / 16.0 + nr) * 16.0;
    o[1] = (y.im / 16.0 + ni) * 16.0;
}

template <int MODE>
__device__ __forceinline__ void hf_body(const HfPlan& pl, const HfIo& io) {
    constexpr bool kReal = MODE == HF_REAL || MODE == HF_PASSBAND || MODE == HF_STREAMING;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = io.w0 + int(blockIdx.y), i0 = int(blockIdx.x) * HF_TILE;

    if (pl.identity) {                          // the identity channel: the input itself, bit for bit
        for (int j = 0; j < HF_PER_THREAD; ++j) {
            const int i = i0 + j * HF_THREADS + tid;
            if (i < io.n) emit<MODE>(pl, io, w, i, source<MODE>(pl, io, w, i));
        }
        return;
    }

    cd* A = reinterpret_cast<cd*>(smem);                        // [HF_NBLK][32] anchors of the current path
    cd* E = A + HF_NBLK * 32;                                   // [32][8]  e^{j 2 pi f d / fs}, d < 8
    cd* F = E + 32 * 8;                                         // [32][8]  e^{j 2 pi f 8 d / fs}
    double* fr = reinterpret_cast<double*>(F + 32 * 8);         // [4][32] frequencies incl. the offset
    double* ph = fr + MGPU_HF_MAX_PATHS * 32;                   // [4][32] phases
    cd* ax = reinterpret_cast<cd*>(ph + MGPU_HF_MAX_PATHS * 32);    // analytic signal, index i0 - dmax + j, j < HF_TILE + dmax
    double* xr = reinterpret_cast<double*>(ax + HF_TILE + pl.dmax); // real input, index i0 - dmax - HL + j (real modes)
    const int base = i0 - pl.dmax, na = HF_TILE + pl.dmax;

    // the draws of this realisation: counter (k * 32 + m, stream 4, realisation)
    const uint64_t real = pl.real0 + uint64_t(w);
    for (int t = tid; t < pl.P * 32; t += HF_THREADS) {
        const int k = t >> 5, m = t & 31;
        if (pl.ns[k] == 1) {
            if (m == 0) { fr[t] = pl.shift[k] + pl.foff; ph[t] = 0.0; }
        } else {
            uint32_t r[4];
            philox4x32(pl.seed, uint32_t(t), HF_STREAM, uint32_t(real), uint32_t(real >> 32), r);
            fr[t] = (pl.shift[k] + pl.half_spread[k] * gauss_bm(r[0], r[1])) + pl.foff;
            ph[t] = 2.0 * M_PI * (double(r[2]) * (1.0 / 4294967296.0));
        }
    }
    if (kReal) {
        for (int j = tid; j < na + 2 * HF_HILBERT_HALF; j += HF_THREADS) xr[j] = source<MODE>(pl, io, w, base - HF_HILBERT_HALF + j).re;
        __syncthreads();
        for (int j = tid; j < na; j += HF_THREADS) {
            const int i = base + j;
            cd v = {0.0, 0.0};
            // the analytic signal exists where the signal does: [0, n), or from the seek position on for a stream
            if (MODE == HF_STREAMING ? i - HF_LATENCY + io.fed >= 0 : i >= 0 && i < io.n) {
                const double* c = xr + j + HF_HILBERT_HALF;
                double h = 0.0;
#pragma unroll
                for (int o = 0; o < HF_HILBERT_ODD; ++o) h = fma(pl.hil[o], c[-(2 * o + 1)] - c[2 * o + 1], h);
                v = {c[0], h};
            }
            ax[j] = v;
        }
    } else {
        for (int j = tid; j < na; j += HF_THREADS) ax[j] = source<MODE>(pl, io, w, base + j);
    }
    __syncthreads();

    cd y[HF_PER_THREAD];
#pragma unroll
    for (int j = 0; j < HF_PER_THREAD; ++j) y[j] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < MGPU_HF_MAX_PATHS; ++k) {
        if (k >= pl.P) break;
        const int ns = pl.ns[k];
        {   // tables of path k: thread (m, p) makes anchors 2p, 2p + 1 and the rotations E[m][p], F[m][p]
            const int m = tid & 31, p = tid >> 5;
            if (m < ns) {
                const double om = 2.0 * M_PI * fr[k * 32 + m], phi = ph[k * 32 + m];
                double s, c;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int b = 2 * p + q;
                    const double t = double(pl.t0 + i0 + HF_BLK * b) / pl.fs;
                    sincos(om * t + phi, &s, &c);
                    A[b * 32 + m] = {c, s};
                }
                sincos(om * (double(p) / pl.fs), &s, &c);
                E[m * 8 + p] = {c, s};
                sincos(om * (double(8 * p) / pl.fs), &s, &c);
                F[m * 8 + p] = {c, s};
            }
        }
        __syncthreads();
        cd acc[HF_PER_THREAD];
#pragma unroll
        for (int j = 0; j < HF_PER_THREAD; ++j) acc[j] = {0.0, 0.0};
        for (int m = 0; m < ns; ++m) {
            const cd e = E[m * 8 + (lane & 7)], f = F[m * 8 + (lane >> 3)];
            const cd r = {e.re * f.re - e.im * f.im, e.re * f.im + e.im * f.re};
#pragma unroll
            for (int j = 0; j < HF_PER_THREAD; ++j) {
                const cd a = A[(wave + 4 * j) * 32 + m];
                acc[j].re = fma(a.re, r.re, fma(-a.im, r.im, acc[j].re));
                acc[j].im = fma(a.re, r.im, fma(a.im, r.re, acc[j].im));
            }
        }
        const double amp = pl.amp[k];
        const int d = pl.delay[k];
#pragma unroll
        for (int j = 0; j < HF_PER_THREAD; ++j) {
            const cd g = {amp * acc[j].re, amp * acc[j].im};
            const cd s = ax[HF_BLK * (wave + 4 * j) + lane + pl.dmax - d];
            y[j].re += g.re * s.re - g.im * s.im;
            y[j].im += g.re * s.im + g.im * s.re;
        }
        __syncthreads();                        // the next path rewrites A, E, F
    }
#pragma unroll
    for (int j = 0; j < HF_PER_THREAD; ++j) {
        const int i = i0 + HF_BLK * (wave + 4 * j) + lane;
        if (i < io.n) emit<MODE>(pl, io, w, i, y[j]);
    }
}

}  // namespace

extern "C" __global__ __launch_bounds__(HF_THREADS) void mgpu_hf_channel_real_kernel(HfPlan pl, HfIo io) { hf_body<HF_REAL>(pl, io); }
extern "C" __global__ __launch_bounds__(HF_THREADS) void mgpu_hf_channel_complex_kernel(HfPlan pl, HfIo io) { hf_body<HF_COMPLEX>(pl, io); }
extern "C" __global__ __launch_bounds__(HF_THREADS) void mgpu_hf_passband_kernel(HfPlan pl, HfIo io) { hf_body<HF_PASSBAND>(pl, io); }
extern "C" __global__ __launch_bounds__(HF_THREADS) void mgpu_hf_baseband_kernel(HfPlan pl, HfIo io) { hf_body<HF_BASEBAND>(pl, io); }
extern "C" __global__ __launch_bounds__(HF_THREADS) void mgpu_hf_stream_kernel(HfPlan pl, HfIo io) { hf_body<HF_STREAMING>(pl, io); }

// the history of the next chunk: the last nh samples of (old history, chunk). grid: x over nh, y over signals
extern "C" __global__ __launch_bounds__(256) void mgpu_hf_stream_roll_kernel(const double* __restrict__ old_hist, const double* __restrict__ in, int nh,
                                                                             int n, double* __restrict__ new_hist) {
    const size_t w = blockIdx.y;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < nh; j += gridDim.x * blockDim.x) {
        const long long q = (long long)j + n;
        new_hist[w * nh + j] = q < nh ? old_hist[w * nh + q] : in[w * n + (q - nh)];
    }
}

namespace {

void launch(int mode, const HfPlan& pl, HfIo io, int W, hipStream_t s) {
    const bool real_in = mode == HF_REAL || mode == HF_PASSBAND || mode == HF_STREAMING;
    const size_t lds = pl.identity ? 0 : lds_bytes(pl, real_in);
    const unsigned tiles = unsigned((io.n + HF_TILE - 1) / HF_TILE);
    auto* k = mode == HF_REAL ? mgpu_hf_channel_real_kernel : mode == HF_COMPLEX ? mgpu_hf_channel_complex_kernel
            : mode == HF_PASSBAND ? mgpu_hf_passband_kernel : mode == HF_BASEBAND ? mgpu_hf_baseband_kernel : mgpu_hf_stream_kernel;
    // Above 48 kHz a 10 ms path's halo takes the real forms' carve past the default dynamic-LDS limit (69,488 B at 96 kHz, 92,528 B at
    // HF_MAX_FS; the complex forms stop at 65,536 B): raise the kernel's limit as create.hip does for the front-end, to the largest carve
    // make_plan admits, so that launches from two host threads cannot lower it under each other. Nothing at or below 48 kHz (57,968 B
    // at the most) comes here.
    constexpr size_t kDefaultLds = 64 * 1024;
    constexpr size_t kMaxLds = size_t(HF_NBLK) * 32 * 16 + 2 * 32 * 8 * 16 + 2 * MGPU_HF_MAX_PATHS * 32 * 8 + size_t(HF_TILE + HF_MAX_DELAY) * 16 +
                               size_t(HF_TILE + HF_MAX_DELAY + 2 * HF_HILBERT_HALF) * 8;       // lds_bytes() of a real form at dmax = HF_MAX_DELAY
    static_assert(kMaxLds == 92528, "the carve DESIGN.md §6.2 and include/mercury_channel.h's 192 kHz stand on");
    if (lds > kDefaultLds) {
        need(lds <= kMaxLds, "the channel's LDS carve exceeds the kernel's limit");
        HIPCK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, int(kMaxLds)));
    }
    for (int w0 = 0; w0 < W; w0 += 65535) {
        io.w0 = w0;
        hipLaunchKernelGGL(k, dim3(tiles, unsigned(std::min(W - w0, 65535))), dim3(HF_THREADS), lds, s, pl, io);
        HIPCK(hipGetLastError());
    }
}

}  // namespace

// S signals fed in chunks (include/mercury_channel.h): the plan, the absolute position and, on the device, the last `nh` input samples of
// every signal in one of two arrays (a chunk reads one and the roll kernel writes the other, so a chunk shorter than the history is safe)
struct mgpu_hf_stream {
    mgpu_ctx* c = nullptr;
    HfPlan pl{};
    int S = 0, nh = 0, cur = 0;
    uint64_t pos = 0, start = 0;          // next input sample; the seek position (input before it is zero)
    DevArray<double> hist[2];             // [S][nh] each
    DevArray<double> d_noise;             // [S]
    std::vector<double> noise;            // what d_noise holds (empty: nothing uploaded yet)
    DevBuf d_in, d_out;                   // mgpu_hf_stream_apply's device copies

    void apply(const double* d_x, int n, const double* noise_amp, double* d_y, hipStream_t s) {
        if (noise_amp && (noise.empty() || std::memcmp(noise.data(), noise_amp, size_t(S) * 8) != 0)) {
            HIPCK(hipStreamSynchronize(s));                 // no chunk in flight still reads the old amplitudes
            noise.assign(noise_amp, noise_amp + S);
            HIPCK(hipMemcpy(d_noise, noise.data(), size_t(S) * 8, hipMemcpyHostToDevice));
        }
        HfPlan p = pl;
        p.t0 = (long long)(pos) - HF_LATENCY;               // anchor time of output block b of tile i0: pos - L + i0 + 64 b
        HfIo io{d_x, d_y, n, 0, 0, 0, 0.0};
        io.hist = hist[cur];
        io.noise_amp = noise_amp ? static_cast<const double*>(d_noise) : nullptr;
        io.nh = nh;
        io.fed = int(std::min<uint64_t>(pos - start, uint64_t(1) << 24));
        io.pos = pos;
        launch(HF_STREAMING, p, io, S, s);
        for (int w0 = 0; w0 < S; w0 += 65535) {
            hipLaunchKernelGGL(mgpu_hf_stream_roll_kernel, dim3(unsigned((nh + 255) / 256), unsigned(std::min(S - w0, 65535))), dim3(256), 0, s,
                               hist[cur] + size_t(w0) * nh, d_x + size_t(w0) * n, nh, n, hist[cur ^ 1] + size_t(w0) * nh);
            HIPCK(hipGetLastError());
        }
        cur ^= 1;
        pos += uint64_t(n);
    }
};

namespace mgpu_detail {

void hf_check(const mgpu_hf_channel* ch) {
    if (const char* e = channel_error(ch)) throw std::invalid_argument(e);
}

void launch_hf_passband(const mgpu_hf_channel* ch, const double* d_audio, int total, int delay, int window, double ampl, uint64_t seed,
                        uint64_t frame0, int F, double* d_out, hipStream_t s) {
    const HfPlan pl = make_plan(ch, kSampleRate, 0, seed, frame0);
    launch(HF_PASSBAND, pl, HfIo{d_audio, d_out, window, 0, total, delay, ampl}, F, s);
}

void launch_hf_baseband(const mgpu_hf_channel* ch, const double* d_clean, int n, double noise_amp, uint64_t seed, uint64_t frame0, int F,
                        double* d_out, hipStream_t s) {
    const HfPlan pl = make_plan(ch, kSampleRate / 4, 0, seed, frame0);
    launch(HF_BASEBAND, pl, HfIo{d_clean, d_out, n, 0, 0, 0, noise_amp}, F, s);
}

}  // namespace mgpu_detail

extern "C" {

int mgpu_hf_channel_preset(int which, mgpu_hf_channel* out) {
    // CCIR Rec. 520-2 / ITU-R F.1487 (Table 1): two equal-power independently fading paths with Gaussian Doppler spectra, no shift
    static const double kDelay[5] = {0.0, 0.5, 1.0, 2.0, 0.5}, kSpread[5] = {0.0, 0.1, 0.5, 1.0, 10.0};
    if (!out || which < MGPU_HF_AWGN || which > MGPU_HF_FLUTTER) return MGPU_ERR_ARG;
    std::memset(out, 0, sizeof(*out));
    out->struct_size = int(sizeof(mgpu_hf_channel));
    out->n_paths = which == MGPU_HF_AWGN ? 1 : 2;
    if (which != MGPU_HF_AWGN) {
        out->delay_ms[1] = kDelay[which];
        out->spread_hz[0] = out->spread_hz[1] = kSpread[which];
    }
    return MGPU_OK;
}

int mgpu_host_hilbert_taps(double* taps, int* ntaps) {
    if (!taps || !ntaps) return MGPU_ERR_ARG;
    const std::vector<double>& h = hilbert_full();
    std::copy(h.begin(), h.end(), taps);
    *ntaps = int(h.size());
    return MGPU_OK;
}

int mgpu_host_hf_channel_draws(const mgpu_hf_channel* ch, uint64_t seed, uint64_t realisation, int path, double* freq_hz, double* phase) {
    if (channel_error(ch) || !freq_hz || !phase || path < 0 || path >= ch->n_paths) return MGPU_ERR_ARG;
    if (ch->spread_hz[path] == 0) {
        for (int m = 0; m < MGPU_HF_SINUSOIDS; ++m) freq_hz[m] = phase[m] = std::nan("");
        freq_hz[0] = ch->shift_hz[path];
        phase[0] = 0.0;
        return MGPU_OK;
    }
    for (int m = 0; m < MGPU_HF_SINUSOIDS; ++m) draw(ch, seed, realisation, path, m, &freq_hz[m], &phase[m]);
    return MGPU_OK;
}

int mgpu_host_hf_channel_taps(const mgpu_hf_channel* ch, double fs, uint64_t seed, uint64_t realisation, long long t0, int n, double* g_c128) {
    if (channel_error(ch) || !g_c128 || n < 0 || !std::isfinite(fs) || fs < 1.0 || fs > HF_MAX_FS) return MGPU_ERR_ARG;
    for (int k = 0; k < ch->n_paths; ++k) {
        const bool fading = ch->spread_hz[k] > 0;
        const int ns = fading ? MGPU_HF_SINUSOIDS : 1;
        double f[MGPU_HF_SINUSOIDS], phi[MGPU_HF_SINUSOIDS];
        if (fading) for (int m = 0; m < ns; ++m) draw(ch, seed, realisation, k, m, &f[m], &phi[m]);
        else { f[0] = ch->shift_hz[k]; phi[0] = 0.0; }
        const double amp = path_amp(ch, k);
        for (int i = 0; i < n; ++i) {
            const double t = double(t0 + i) / fs;
            double re = 0, im = 0;
            for (int m = 0; m < ns; ++m) {
                const double a = 2.0 * M_PI * f[m] * t + phi[m];
                re += std::cos(a);
                im += std::sin(a);
            }
            g_c128[2 * (size_t(k) * n + i)] = amp * re;
            g_c128[2 * (size_t(k) * n + i) + 1] = amp * im;
        }
    }
    return MGPU_OK;
}

int mgpu_host_hf_stream_noise(uint64_t seed, int signal, uint64_t position, int n, double* out) {
    if (!out || n < 0 || signal < 0) return MGPU_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        const uint64_t T = position + uint64_t(i);
        uint32_t q[4];
        philox4x32(seed, uint32_t(T), HF_NOISE_STREAM, uint32_t(T >> 32), uint32_t(signal), q);
        out[i] = gauss_bm(q[0], q[1]);
    }
    return MGPU_OK;
}

int mgpu_hf_stream_create(mgpu_ctx* c, const mgpu_hf_channel* ch, double fs, int S, uint64_t seed, uint64_t realisation0, mgpu_hf_stream** out) {
    if (!c || !out) return MGPU_ERR_ARG;
    *out = nullptr;
    return guard(c, [&] {
        const HfPlan pl = make_plan(ch, fs, 0, seed, realisation0);
        need(S >= 1 && S <= (1 << 22), "bad argument (S: 1..2^22)");
        std::unique_ptr<mgpu_hf_stream> k(new mgpu_hf_stream);
        k->c = c;
        k->pl = pl;
        k->S = S;
        k->nh = HF_LATENCY + pl.dmax + HF_HILBERT_HALF;
        for (auto& h : k->hist) {
            h = DevArray<double>(size_t(S) * k->nh * 8);
            HIPCK(hipMemsetAsync(h, 0, size_t(S) * k->nh * 8, c->stream));
        }
        k->d_noise = DevArray<double>(size_t(S) * 8);
        HIPCK(hipStreamSynchronize(c->stream));
        *out = k.release();
    });
}

int mgpu_hf_stream_destroy(mgpu_hf_stream* k) {
    if (!k) return MGPU_ERR_ARG;
    mgpu_ctx* c = k->c;
    return guard(c, [&] {
        HIPCK(hipDeviceSynchronize());          // chunks may be queued on a caller's stream
        delete k;
    });
}

int mgpu_hf_stream_latency(mgpu_hf_stream* k) { return k ? HF_LATENCY : MGPU_ERR_ARG; }

int mgpu_hf_stream_seek(mgpu_hf_stream* k, uint64_t position) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        need(position % HF_BLK == 0, "the seek position must be a multiple of 64");
        HIPCK(hipDeviceSynchronize());
        HIPCK(hipMemset(k->hist[k->cur], 0, size_t(k->S) * k->nh * 8));
        k->pos = k->start = position;
    });
}

int mgpu_hf_stream_apply_dev(mgpu_hf_stream* k, const void* d_in, int n, const double* noise_amp, void* d_out, void* stream) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        need(d_in && d_out && d_in != d_out, "bad argument (in and out must be given and may not alias)");
        need(n > 0 && n % HF_BLK == 0, "n must be a positive multiple of 64");
        k->apply(static_cast<const double*>(d_in), n, noise_amp, static_cast<double*>(d_out), stream_or_own(k->c, stream));
    });
}

int mgpu_hf_stream_apply(mgpu_hf_stream* k, const double* in, int n, const double* noise_amp, double* out) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        need(in && out && in != out, "bad argument (in and out must be given and may not alias)");
        need(n > 0 && n % HF_BLK == 0, "n must be a positive multiple of 64");
        const size_t bytes = size_t(k->S) * n * 8;
        hipStream_t s = k->c->stream;
        k->d_in.grow(bytes);
        k->d_out.grow(bytes);
        HIPCK(hipMemcpyAsync(k->d_in.p, in, bytes, hipMemcpyHostToDevice, s));
        k->apply(k->d_in.as<double>(), n, noise_amp, k->d_out.as<double>(), s);
        HIPCK(hipMemcpyAsync(out, k->d_out.p, bytes, hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
    });
}

int mgpu_hf_channel_apply_dev(mgpu_ctx* c, const mgpu_hf_channel* ch, const void* d_in, int complex_input, double fs, int W, int n,
                              uint64_t seed, uint64_t realisation0, long long t0, void* d_out, void* stream) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        const HfPlan pl = make_plan(ch, fs, t0, seed, realisation0);
        need(d_in && d_out && d_in != d_out && W >= 0 && n >= 0 && (complex_input == 0 || complex_input == 1), "bad argument");
        if (W == 0 || n == 0) return;
        launch(complex_input ? HF_COMPLEX : HF_REAL, pl, HfIo{static_cast<const double*>(d_in), static_cast<double*>(d_out), n, 0, 0, 0, 0.0}, W,
               stream_or_own(c, stream));
    });
}

int mgpu_hf_channel_apply(mgpu_ctx* c, const mgpu_hf_channel* ch, const void* in, int complex_input, double fs, int W, int n,
                          uint64_t seed, uint64_t realisation0, long long t0, void* out) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        const HfPlan pl = make_plan(ch, fs, t0, seed, realisation0);
        need(in && out && W >= 0 && n >= 0 && (complex_input == 0 || complex_input == 1), "bad argument");
        if (W == 0 || n == 0) return;
        const size_t bytes = size_t(W) * n * (complex_input ? 16 : 8);
        DevBuf d_in(bytes), d_out(bytes);
        hipStream_t s = c->stream;
        HIPCK(hipMemcpyAsync(d_in.p, in, bytes, hipMemcpyHostToDevice, s));
        launch(complex_input ? HF_COMPLEX : HF_REAL, pl, HfIo{d_in.as<double>(), d_out.as<double>(), n, 0, 0, 0, 0.0}, W, s);
        HIPCK(hipMemcpyAsync(out, d_out.p, bytes, hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
    });
}

}  // extern "C"

// Carrier tuner (include/ext/mercury_tuner.h): one block of wideband IQ into, per planned channel, how far its station is off the plan.
//
// Per call, on the context's stream:
//   1. mgpu_tune_mix_kernel: z [S][M], the channel at 12 kHz: the channeliser's tap chain at every fourth output. A workgroup is 16
//      consecutive outputs by up to 16 channels; the window of inputs its outputs share is widened into LDS once per block of steps.
//   2. mgpu_tune_fold_kernel, one workgroup per channel: the lag products of a symbol's 287 samples in LDS, the chains of 16 per phase,
//      and the chain over the symbols in a register per phase. G and E come back to the host (one copy), which decides phi* and r.
//   3. mgpu_tune_comb_kernel, one workgroup per channel, four symbols at a time, one per wavefront: the turn in the load, the scanner's
//      transform (scan_fft.h at log2n = 8), |U|^2 in rows of LDS, and the chain over the symbols in a register per bin. Q comes back
//      (the second copy) and the host completes the reports.
// Nothing is kept between calls but the last call's arrays, for mgpu_tune_arrays.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "scan_fft.h"
#include "stream_stage.hpp"
#include "tune_rule.hpp"

using namespace mgpu_tune_detail;

namespace {

constexpr int kTile = 16;                    // outputs of a workgroup of the mix kernel
constexpr int kTileChannels = 16;            // and its channels, four to a wavefront
constexpr int kMixThreads = kTile * kTileChannels;
constexpr int kMixLdsSamples = 4352;         // the image of a block of steps, in samples of 16 bytes: 17 columns of 4 D = 256 rows
constexpr int kMixMaxLds = kMixLdsSamples * 16;
constexpr int kFoldThreads = 320;            // >= 272 + 15 lag products of a symbol
constexpr int kCombWaves = 4;

struct MixArgs {
    const void* iq;           // the block's n_in samples in `format`
    const double2* g;         // [S][T]
    double2* z;               // [S][M]
    int format, n_in, S, M, D, T, NB, ncols, nblocks;
};

}  // namespace

// the channeliser's step (channelizer.hip chan_step), one output: the rule's four fused multiply-adds of tap g on sample v
__device__ inline void tune_step(const double2 g, const double2 v, double& re, double& im) {
    re = fma(g.x, v.x, re);
    re = fma(-g.y, v.y, re);
    im = fma(g.x, v.y, im);
    im = fma(g.y, v.x, im);
}

// Thread t: output m0 + (t & 15) of channel 16 blockIdx.y + (t >> 4). At step k the output m reads sample u = 4 D m - k: the outputs of a
// tile are Dm = 4 D samples apart, so the image is stored transposed with modulus Dm, window sample w at [w mod Dm][w div Dm], and at
// one step the 16 outputs read 16 consecutive 16-byte slots of one row (the four channels of a wavefront the same ones). The steps are
// cut into blocks of B = NB Dm: block b needs the window [U0 - (b + 1) B + 1, U0 - b B + 15 Dm], 15 Dm + B samples, U0 = 4 D m0.
// Rows are `ncols` (odd) slots long. A sample before the block's start is zeros.
extern "C" __global__ __launch_bounds__(kMixThreads) void mgpu_tune_mix_kernel(MixArgs a) {
    extern __shared__ double2 tune_lds[];
    const int o = threadIdx.x & (kTile - 1);
    const int s = int(blockIdx.y) * kTileChannels + int(threadIdx.x >> 4);
    const int m0 = int(blockIdx.x) * kTile, m = m0 + o;
    const bool live = s < a.S && m < a.M;
    const int Dm = 4 * a.D, B = a.NB * Dm, ncols = a.ncols, T = a.T;
    const int U0 = m0 * Dm;
    const int wn = Dm * (kTile - 1 + a.NB);
    const double2* __restrict__ gs = a.g + size_t(live ? s : 0) * T;
    const double2* __restrict__ img = tune_lds + o;
    double re = 0.0, im = 0.0;
    for (int b = 0; b < a.nblocks; ++b) {
        const int lo = U0 - (b + 1) * B + 1;                 // block sample of window sample 0 (negative at the block's start)
        if (b) __syncthreads();                              // the previous block's reads are done
        for (int w = threadIdx.x; w < wn; w += blockDim.x) {
            const int u = lo + w;
            const double2 v = (u >= 0 && u < a.n_in) ? mgpu_fmt::load_iq(a.iq, a.format, size_t(u)) : make_double2(0.0, 0.0);
            tune_lds[(w % Dm) * ncols + w / Dm] = v;
        }
        __syncthreads();
        if (live) {
            // step k of the block sits at t = B - 1 - (k - b B) = q Dm + row, output o at column q + o
            int k = b * B, row = Dm - 1, q = a.NB - 1;
            const int kend = min(k + B, T);
            for (; k + 4 <= kend; k += 4) {                  // four steps' LDS reads and taps in flight together
                double2 v[4], g[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    v[u] = img[row * ncols + q];
                    g[u] = gs[k + u];
                    if (--row < 0) { row = Dm - 1; --q; }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) tune_step(g[u], v[u], re, im);
            }
            for (; k < kend; ++k) {
                tune_step(gs[k], img[row * ncols + q], re, im);
                if (--row < 0) { row = Dm - 1; --q; }
            }
        }
    }
    if (live) a.z[size_t(s) * a.M + m] = make_double2(re, im);
}

// One workgroup per channel. Symbol j: thread t < 287 has the lag products of m = 272 j + t (the 15 that two symbols' phases share are
// made again for the second: the same values), thread phi < 272 adds its 16 in ascending i and then the sum onto its G and E: the rule's
// additions in the rule's order.
extern "C" __global__ __launch_bounds__(kFoldThreads) void mgpu_tune_fold_kernel(const double2* __restrict__ z, int M, int J,
                                                                                 double2* __restrict__ G, double* __restrict__ E) {
    __shared__ double pr[kSym + kGi], pi[kSym + kGi], pe[kSym + kGi];
    const int s = blockIdx.x, t = threadIdx.x;
    const double2* __restrict__ zs = z + size_t(s) * M;
    double gr = 0.0, gi = 0.0, ge = 0.0;
    for (int j = 0; j < J; ++j) {
        if (t < kSym + kGi - 1) {
            const int m = kSym * j + t;                      // m + 256 <= 272 J + 270 < M
            const double2 a = zs[m], b = zs[m + kNfft];
            pr[t] = a.x * b.x + a.y * b.y;
            pi[t] = a.y * b.x - a.x * b.y;
            pe[t] = 0.5 * ((a.x * a.x + a.y * a.y) + (b.x * b.x + b.y * b.y));
        }
        __syncthreads();
        if (t < kSym) {
            double ir = 0.0, ii = 0.0, ie = 0.0;
#pragma unroll
            for (int i = 0; i < kGi; ++i) {
                ir = ir + pr[t + i];
                ii = ii + pi[t + i];
                ie = ie + pe[t + i];
            }
            gr = gr + ir;
            gi = gi + ii;
            ge = ge + ie;
        }
        __syncthreads();
    }
    if (t < kSym) {
        G[size_t(s) * kSym + t] = make_double2(gr, gi);
        E[size_t(s) * kSym + t] = ge;
    }
}

// One workgroup of four wavefronts per channel; wavefront w transforms the symbols j = 4 i + w, one group of the network per lane
// (ScanFft<8>: 64 groups), and thread k adds the four rows of |U[k]|^2 onto its Q in ascending j.
extern "C" __global__ __launch_bounds__(64 * kCombWaves) void mgpu_tune_comb_kernel(const double2* __restrict__ z, int M, int J,
                                                                                    const Turn* __restrict__ turns,
                                                                                    const sc2* __restrict__ tab,
                                                                                    const double2* __restrict__ W, double* __restrict__ Q) {
    using F = ScanFft<kLog2>;
    __shared__ __attribute__((aligned(16))) sc2 work[kCombWaves][kNfft];
    __shared__ double power[kCombWaves][kNfft];
    const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double2* __restrict__ zs = z + size_t(s) * M;
    const Turn turn = turns[s];
    double q = 0.0;
    for (int j0 = 0; j0 < J; j0 += kCombWaves) {
        const int j = j0 + wave;
        const bool on = j < J;                               // uniform in a wavefront; every wavefront meets every barrier
        const int first = kSym * j + turn.phase + kGi / 2;   // first + 255 <= 272 J + 262 < M
        auto fetch = [&](int i) {
            const int m = first + i;
            const double2 v = zs[m];
            const double2 w = W[(unsigned long long)turn.index * unsigned(m) % unsigned(MGPU_CHAN_PHASOR_LEN)];
            return sc2{v.x * w.x + v.y * w.y, v.y * w.x - v.x * w.y};
        };
#pragma unroll
        for (int r = 0; r < F::kRounds; ++r) {
            if (on) F::round(r, lane, work[wave], tab, r == 0, fetch);
            __syncthreads();
        }
        if (on)
            for (int k = lane; k < kNfft; k += 64) {
                const sc2 u = work[wave][scan_entry(scan_brev(k, kLog2))];
                power[wave][k] = u.re * u.re + u.im * u.im;
            }
        __syncthreads();
        for (int w = 0; w < kCombWaves && j0 + w < J; ++w) q = q + power[w][t];
        __syncthreads();                                     // the rows are read before the next four symbols write them
    }
    Q[size_t(s) * kNfft + t] = q;
}

struct mgpu_tune {
    mgpu_ctx* c = nullptr;
    mgpu_tune_config cfg{};                       // taps points into h
    std::vector<double> h;                        // the prototype
    std::vector<mgpu_chan_channel> chans;
    int S = 0, D = 0, T = 0, J = 0, M = 0, n_in = 0, NB = 0, ncols = 0, nblocks = 0;
    size_t lds = 0;
    bool ran = false;                             // the arrays below hold a call's results
    DevArray<double2> d_g, d_W, d_z;              // [S][T], [48000], [S][M]
    DevArray<sc2> d_tab;                          // [256] the scanner's table at N = 256
    DevArray<double> d_GE, d_Q;                   // G [S][272] complex then E [S][272]; [S][256]
    DevArray<Turn> d_turns;                       // [S]
    DevArray<char> d_stage;                       // host input's landing area (ctx.hpp staged_on_device)
    std::vector<double> GE, Q;                    // the copies back
    std::vector<Turn> turns;

    void upload_row(int s, hipStream_t st) {
        std::vector<double> g(size_t(T) * 2);
        mgpu_chan_detail::tap_row(h, D, cfg.audio_centre_hz, chans[s], g.data());
        HIPCK(hipMemcpyAsync(d_g + size_t(s) * T, g.data(), g.size() * 8, hipMemcpyHostToDevice, st));
        HIPCK(hipStreamSynchronize(st));          // g is this call's
    }

    void run(const void* d_iq, int format, mgpu_tune_report* reports, hipStream_t st) {
        MixArgs a{};
        a.iq = d_iq; a.g = d_g; a.z = d_z; a.format = format; a.n_in = n_in; a.S = S; a.M = M; a.D = D; a.T = T; a.NB = NB; a.ncols = ncols;
        a.nblocks = nblocks;
        const int per_group = std::min(S, kTileChannels);
        const dim3 block(unsigned(64 * ((per_group + 3) / 4)));
        const unsigned gx = unsigned((M + kTile - 1) / kTile);
        for (int s0 = 0; s0 < S; s0 += 65535 * kTileChannels) {    // grid y is 16 bits wide
            MixArgs b = a;
            const int ns = std::min(S - s0, 65535 * kTileChannels);
            b.g += size_t(s0) * T; b.z += size_t(s0) * M; b.S = ns;
            hipLaunchKernelGGL(mgpu_tune_mix_kernel, dim3(gx, unsigned((ns + kTileChannels - 1) / kTileChannels)), block, lds, st, b);
            HIPCK(hipGetLastError());
        }
        double2* const d_G = reinterpret_cast<double2*>(d_GE.p);
        double* const d_E = d_GE + size_t(S) * kSym * 2;
        hipLaunchKernelGGL(mgpu_tune_fold_kernel, dim3(unsigned(S)), dim3(kFoldThreads), 0, st, static_cast<const double2*>(d_z), M, J, d_G, d_E);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(GE.data(), d_GE.p, GE.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        const double* const G = GE.data(), * const E = GE.data() + size_t(S) * kSym * 2;
        for (int s = 0; s < S; ++s) turns[s] = decide_phase(cfg, chans[s], G + size_t(s) * kSym * 2, E + size_t(s) * kSym, reports + s);
        HIPCK(hipMemcpyAsync(d_turns.p, turns.data(), size_t(S) * sizeof(Turn), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(mgpu_tune_comb_kernel, dim3(unsigned(S)), dim3(64 * kCombWaves), 0, st, static_cast<const double2*>(d_z), M, J,
                           static_cast<const Turn*>(d_turns), static_cast<const sc2*>(d_tab), static_cast<const double2*>(d_W), static_cast<double*>(d_Q));
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(Q.data(), d_Q.p, Q.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        for (int s = 0; s < S; ++s) decide_comb(cfg, chans[s], turns[s], Q.data() + size_t(s) * kNfft, reports + s);
        ran = true;
    }
};

extern "C" {

int mgpu_tune_create(mgpu_ctx* c, const mgpu_tune_config* kc, const mgpu_chan_channel* channels, mgpu_tune** out) {
    return create_stage(c, out, "mgpu_tune_create", config_error(kc, channels), [&](mgpu_tune* k) {
        const mgpu_chan_config cc = chan_config_of(*kc);
        keep_config(k, kc, mgpu_chan_detail::prototype(&cc));
        k->chans.assign(channels, channels + kc->S);
        const int S = k->S = kc->S, D = k->D = kc->D, T = k->T = int(k->h.size());
        k->J = kc->symbols;
        k->M = block_samples(*kc);
        k->n_in = input_samples(*kc);
        const int Dm = 4 * D;
        k->NB = std::max(2, std::min((T + Dm - 1) / Dm, kMixLdsSamples / Dm - kTile));
        k->ncols = (kTile - 1 + k->NB) | 1;
        k->nblocks = (T + k->NB * Dm - 1) / (k->NB * Dm);
        k->lds = size_t(Dm) * k->ncols * sizeof(double2);
        need(k->lds <= size_t(kMixMaxLds), "LDS image larger than the kernel's limit");
        HIPCK(hipFuncSetAttribute(reinterpret_cast<const void*>(mgpu_tune_mix_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMixMaxLds));
        k->d_g = DevArray<double2>(size_t(S) * T * sizeof(double2));
        k->d_z = DevArray<double2>(size_t(S) * k->M * sizeof(double2));
        k->d_GE = DevArray<double>(size_t(S) * kSym * 3 * 8);
        k->d_Q = DevArray<double>(size_t(S) * kNfft * 8);
        k->d_turns = DevArray<Turn>(size_t(S) * sizeof(Turn));
        k->d_tab = DevArray<sc2>(size_t(kNfft) * sizeof(sc2));
        k->d_W = phasor_table_on_device();
        const mgpu_scan_detail::Tables tables(kLog2);
        HIPCK(hipMemcpy(k->d_tab.p, tables.tab.data(), size_t(kNfft) * 16, hipMemcpyHostToDevice));
        k->GE.resize(size_t(S) * kSym * 3);
        k->Q.resize(size_t(S) * kNfft);
        k->turns.resize(size_t(S));
        for (int s = 0; s < S; ++s) k->upload_row(s, c->stream);
    });
}

int mgpu_tune_destroy(mgpu_tune* k) { return destroy_stage(k); }

int mgpu_tune_retune(mgpu_tune* k, int s, const mgpu_chan_channel* channel) { return retune_channel(k, s, channel); }

int mgpu_tune_samples(mgpu_tune* k) { return k ? k->n_in : -1; }

int mgpu_tune_process(mgpu_tune* k, const void* iq, int format, int n_in, mgpu_tune_report* reports) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        need(iq && reports, "null pointer");
        need_iq_format(format);
        need(n_in == k->n_in, "n_in must be 4 * D * 272 * (symbols + 1)");
        hipStream_t st = k->c->stream;
        const void* d_iq = staged_iq(k->d_stage, iq, format, n_in, st);
        k->run(d_iq, format, reports, st);
    });
}

int mgpu_tune_arrays(mgpu_tune* k, double* G, double* E, double* Q) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        need(k->ran, "no call has run yet");
        const size_t S = size_t(k->S);
        if (G) std::memcpy(G, k->GE.data(), S * kSym * 2 * 8);
        if (E) std::memcpy(E, k->GE.data() + S * kSym * 2, S * kSym * 8);
        if (Q) std::memcpy(Q, k->Q.data(), S * kNfft * 8);
    });
}

int mgpu_host_tune_process(const mgpu_tune_config* kc, const mgpu_chan_channel* channels, const void* iq, int format, int n_in,
                           mgpu_tune_report* reports, double* G, double* E, double* Q) {
    return host_try([&] { return host_process(kc, channels, iq, format, n_in, reports, G, E, Q); });
}

int mgpu_host_tune_plan(const mgpu_tune_report* report, const mgpu_chan_channel* channel, mgpu_chan_channel* refined) {
    return host_plan(report, channel, refined);
}

}  // extern "C"

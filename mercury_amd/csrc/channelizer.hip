// Wideband channeliser (include/mercury_channelizer.h): one IQ stream at 48000 * D into S real 48 kHz sideband streams [S][n_out].
//
// Per call, on one stream:
//   1. mgpu_chan_assemble_kernel writes the call's input line  cur = [ last T - 1 widened inputs | the chunk, widened ]  from the other of
//      two line buffers (its tail is the history; zeros after a seek) and the caller's IQ samples;
//   2. mgpu_chan_fir_kernel computes every output from that line (below);
// and the two buffers change roles. Nothing else is kept between calls, so how the stream is cut cannot change an output.
//
// The FIR kernel. 8 T flops per output and few bytes: it is bound by fp64 FMA issue and LDS reads. A workgroup is four wavefronts = four
// channels on ONE tile of 64 * R consecutive outputs: the x span is the same for every channel, so the four share one LDS image of it, and
// a channel's taps are uniform across its wavefront: scalar loads, SGPR operands. Lane l keeps the R consecutive outputs j0 + l R .. + R-1;
// at step i it reads the sample u = U0 + l R D - i once and uses it for output r at tap k = i - (R-1-r) D, so every accumulator sees its
// taps in ascending k (the rule's order; the tiling never reorders a sum) and one 16-byte LDS read feeds 4 R fused multiply-adds.
// Lanes read x with a stride of R D samples, the worst stride there is for D a power of two, so the image is stored polyphase-transposed
// with modulus R D: window sample w at [w mod RD][w div RD]. At one step every lane has the same row and consecutive columns: consecutive
// 16-byte slots, which ds_read_b128 serves without a bank conflict (its four 16-lane groups each cover 16 different slots). The span of a
// tile, 64 R D + T samples, does not fit LDS at D >= 16, so the steps are cut into blocks of B = NB R D and the span is streamed through:
// block b needs the window [U0 - (b+1) B + 1, U0 - b B + 63 R D], 63 R D + B samples. Rows are `ncols` (odd) slots long.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "stream_stage.hpp"

using namespace mgpu_chan_detail;

namespace {

constexpr int kWaves = 4;                    // channels per workgroup
constexpr int kThreads = 64 * kWaves;
constexpr int kLdsSamples = 3072;            // LDS image of a block, in samples of 16 bytes, where R D allows it (48 KiB: three workgroups per CU)
constexpr int kMaxLds = 72 * 1024;           // the largest image any (D, T) asks for: R D = 64 rows of 69 slots

struct ChanRow { int offm; int pad; double gain; };      // offset_hz mod 48000, gain

struct FirArgs {
    const double2* cur;       // the input line, `total` samples
    const double2* g;         // [S][T]
    const double2* W;         // [48000]
    const ChanRow* rows;      // [S]
    double* out;              // [S][out_stride]
    size_t out_stride;
    int total, S, N, D, T, NB, ncols, nblocks;
    unsigned nm;              // (n0 - L) mod 48000
};

inline int outputs_per_lane(int D) { return D <= 32 ? 2 : 1; }

}  // namespace

// cur[i] = prev[prev_keep + i] for i < hist (zeros when prev is null), else the chunk's sample i - hist widened. The formats and the divisor
// are sample_formats.h's, restated: with that header's dispatch in this loop the call measured slower (profiles/stage_plumbing.md)
template <typename T>
__device__ inline double2 chan_widen(const T* iq, size_t i, double div) { return make_double2(double(iq[2 * i]) / div, double(iq[2 * i + 1]) / div); }

extern "C" __global__ __launch_bounds__(256) void mgpu_chan_assemble_kernel(const double2* __restrict__ prev, size_t prev_keep, int hist,
                                                                            const void* __restrict__ iq, int format, int n_in,
                                                                            double2* __restrict__ cur) {
    const size_t total = size_t(hist) + size_t(n_in);
    for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += size_t(gridDim.x) * blockDim.x) {
        double2 v;
        if (i < size_t(hist)) v = prev ? prev[prev_keep + i] : make_double2(0.0, 0.0);
        else if (format == MGPU_IQ_CS16) v = chan_widen(static_cast<const int16_t*>(iq), i - hist, 32768.0);
        else if (format == MGPU_IQ_CF32) v = chan_widen(static_cast<const float*>(iq), i - hist, 1.0);
        else v = chan_widen(static_cast<const double*>(iq), i - hist, 1.0);
        cur[i] = v;
    }
}

// One step for one lane: the sample v serves output r at tap k = i - (R-1-r) D. CHECK: a step where not every output has a tap (k outside
// [0, T)); the conditions are uniform.
template <int R, bool CHECK>
__device__ inline void chan_step(int i, const double2 v, const int D, const int T, const double2* __restrict__ gs, double (&re)[R], double (&im)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int k = i - (R - 1 - r) * D;
        if (CHECK && (k < 0 || k >= T)) continue;
        const double2 g = gs[k];
        re[r] = fma(g.x, v.x, re[r]);
        re[r] = fma(-g.y, v.y, re[r]);
        im[r] = fma(g.x, v.y, im[r]);
        im[r] = fma(g.y, v.x, im[r]);
    }
}

// steps [i, iend) of one block for one lane, from image position (row, q) down
template <int R, bool CHECK>
__device__ inline void chan_steps(int i, int iend, int& row, int& q, const int RD, const int D, const int T, const int ncols,
                                  const double2* __restrict__ img, const double2* __restrict__ gs, double (&re)[R], double (&im)[R]) {
    if (!CHECK) {
        // four steps at a time: their four LDS reads and 4 R taps (64 contiguous bytes per output: one scalar load) are in flight together
        for (; i + 4 <= iend; i += 4) {
            double2 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = img[row * ncols + q];
                if (--row < 0) { row = RD - 1; --q; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) chan_step<R, false>(i + u, v[u], D, T, gs, re, im);
        }
    }
#pragma unroll 1
    for (; i < iend; ++i) {
        const double2 v = img[row * ncols + q];
        chan_step<R, CHECK>(i, v, D, T, gs, re, im);
        if (--row < 0) { row = RD - 1; --q; }
    }
}

template <int R>
__device__ inline void chan_fir(const FirArgs& a) {
    extern __shared__ double2 chan_lds[];
    const int lane = threadIdx.x & 63;
    const int s = int(blockIdx.y) * kWaves + __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
    const bool live = s < a.S;
    const int D = a.D, T = a.T, RD = R * D, B = a.NB * RD, I = T + (R - 1) * D, ncols = a.ncols;
    const int j0 = int(blockIdx.x) * 64 * R;
    const int U0 = (T - 1) + (j0 + R - 1) * D;
    const int wn = RD * (63 + a.NB);                         // window samples of a block
    const double2* __restrict__ gs = a.g + size_t(live ? s : 0) * T;
    const double2* __restrict__ img = chan_lds + lane;
    double re[R], im[R];
#pragma unroll
    for (int r = 0; r < R; ++r) re[r] = im[r] = 0.0;

    for (int b = 0; b < a.nblocks; ++b) {
        const int lo = U0 - (b + 1) * B + 1;                 // line index of window sample 0 (may be negative in the last block)
        if (b) __syncthreads();                              // the previous block's reads are done
        for (int w = threadIdx.x; w < wn; w += kThreads) {
            const int u = lo + w;
            const double2 v = (u >= 0 && u < a.total) ? a.cur[u] : make_double2(0.0, 0.0);
            chan_lds[(w % RD) * ncols + w / RD] = v;
        }
        __syncthreads();
        if (live) {
            // step i of the block sits at t = B - 1 - (i - b B) = q RD + row, lane l at column q + l
            int i = b * B, row = RD - 1, q = a.NB - 1;
            const int iend = std::min(i + B, I);
            const int head = std::min(iend, (R - 1) * D), mid = std::min(iend, T);
            if (i < head) { chan_steps<R, true>(i, head, row, q, RD, D, T, ncols, img, gs, re, im); i = head; }
            if (i < mid) { chan_steps<R, false>(i, mid, row, q, RD, D, T, ncols, img, gs, re, im); i = mid; }
            if (i < iend) chan_steps<R, true>(i, iend, row, q, RD, D, T, ncols, img, gs, re, im);
        }
    }
    if (!live) return;
    const ChanRow cr = a.rows[s];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = j0 + lane * R + r;
        if (j >= a.N) continue;
        const unsigned nmod = (a.nm + unsigned(j)) % unsigned(MGPU_CHAN_PHASOR_LEN);
        const unsigned p = (unsigned(cr.offm) * nmod) % unsigned(MGPU_CHAN_PHASOR_LEN);
        const double2 w = a.W[p];
        a.out[size_t(s) * a.out_stride + j] = cr.gain * fma(im[r], w.y, re[r] * w.x);
    }
}

extern "C" __global__ __launch_bounds__(256) void mgpu_chan_fir_r2_kernel(FirArgs a) { chan_fir<2>(a); }
extern "C" __global__ __launch_bounds__(256) void mgpu_chan_fir_r1_kernel(FirArgs a) { chan_fir<1>(a); }

struct mgpu_chan {
    mgpu_ctx* c = nullptr;
    mgpu_chan_config cfg{};                       // taps points into h
    std::vector<double> h;                        // the prototype
    std::vector<mgpu_chan_channel> chans;
    int S = 0, D = 0, T = 0, L = 0, max_out = 0, R = 1, NB = 0, ncols = 0, nblocks = 0;
    size_t lds = 0;
    uint64_t pos = 0;
    History<double2> line;                        // [T - 1 + max_out * D] the input line; the history is the last T - 1 samples of the old one,
    size_t kept = 0;                              // which start here
    DevArray<double2> d_g, d_W;                   // [S][T], [48000]
    DevArray<ChanRow> d_rows;                     // [S]
    DevArray<char> d_stage;                       // host input's landing area (ctx.hpp staged_on_device)
    DevArray<double> d_out;                       // [S][max_out]: process()'s output and the wideband capture's workspace (made on first use)

    void upload_row(int s, hipStream_t st) {
        std::vector<double> g(size_t(T) * 2);
        tap_row(h, D, cfg.audio_centre_hz, chans[s], g.data());
        const ChanRow row{int(floor_mod(chans[s].offset_hz, MGPU_CHAN_PHASOR_LEN)), 0, chans[s].gain};
        HIPCK(hipMemcpyAsync(d_g + size_t(s) * T, g.data(), g.size() * 8, hipMemcpyHostToDevice, st));
        HIPCK(hipMemcpyAsync(d_rows + s, &row, sizeof(row), hipMemcpyHostToDevice, st));
        HIPCK(hipStreamSynchronize(st));          // g and row are this call's
    }

    void check_n_in(const void* iq, int format, int n_in, const void* out) const {
        need(iq && out, "null pointer");
        need_iq_format(format);
        need(n_in >= D && n_in % D == 0, "n_in must be a positive multiple of D");
        need(n_in / D <= max_out, "more outputs than max_out in one call");
        need(pos + uint64_t(n_in / D) <= (1ULL << 62), "position beyond 2^62");
    }

    // one call on device memory: the next n_in / D outputs of every channel into d_o [S][n_in / D]
    void run(const void* d_iq, int format, int n_in, double* d_o, hipStream_t st) {
        const int N = n_in / D, hist = T - 1;
        double2* cur = line.next();
        const size_t total = size_t(hist) + size_t(n_in);
        hipLaunchKernelGGL(mgpu_chan_assemble_kernel, dim3(unsigned(std::min<size_t>((total + 255) / 256, 2048))), dim3(256), 0, st,
                           line.old(), kept, hist, d_iq, format, n_in, cur);
        HIPCK(hipGetLastError());
        FirArgs a{};
        a.cur = cur; a.g = d_g; a.W = d_W; a.rows = d_rows; a.out = d_o; a.out_stride = size_t(N);
        a.total = int(total); a.S = S; a.N = N; a.D = D; a.T = T; a.NB = NB; a.ncols = ncols; a.nblocks = nblocks;
        a.nm = unsigned(floor_mod((long long)(pos % MGPU_CHAN_PHASOR_LEN) - L, MGPU_CHAN_PHASOR_LEN));
        const unsigned gx = unsigned((N + 64 * R - 1) / (64 * R));
        for (int s0 = 0; s0 < S; s0 += 65535 * kWaves) {           // grid y is 16 bits wide
            FirArgs b = a;
            const int ns = std::min(S - s0, 65535 * kWaves);
            b.g += size_t(s0) * T; b.rows += s0; b.out += size_t(s0) * N; b.S = ns;
            const dim3 grid(gx, unsigned((ns + kWaves - 1) / kWaves));
            if (R == 2) hipLaunchKernelGGL(mgpu_chan_fir_r2_kernel, grid, dim3(kThreads), lds, st, b);
            else hipLaunchKernelGGL(mgpu_chan_fir_r1_kernel, grid, dim3(kThreads), lds, st, b);
            HIPCK(hipGetLastError());
        }
        kept = size_t(n_in);                      // the line's last T - 1 samples are the next call's history
        line.advance();
        pos += uint64_t(N);
    }

    const void* on_device(const void* iq, int format, int n_in, hipStream_t st) {
        return staged_iq(d_stage, iq, format, n_in, st);
    }
    void need_out() {
        if (!d_out.p) d_out = DevArray<double>(size_t(S) * max_out * 8);
    }
};

extern "C" {

int mgpu_chan_create(mgpu_ctx* c, const mgpu_chan_config* kc, const mgpu_chan_channel* channels, mgpu_chan** out) {
    const char* bad = config_error(kc, true);
    if (!bad) bad = plan_error(kc->D, kc->audio_centre_hz, kc->S, channels);
    return create_stage(c, out, "mgpu_chan_create", bad, [&](mgpu_chan* k) {
        keep_config(k, kc, prototype(kc));
        k->chans.assign(channels, channels + kc->S);
        const int S = k->S = kc->S, D = k->D = kc->D, T = k->T = int(k->h.size());
        k->L = (T - 1) / D / 2;
        k->max_out = kc->max_out ? kc->max_out : kDefaultMaxOut;
        need((long long)k->max_out * D <= (1LL << 30), "max_out * D must be at most 2^30");
        const int R = k->R = outputs_per_lane(D), RD = R * D, I = T + (R - 1) * D;
        k->NB = std::min((I + RD - 1) / RD, std::max(4, kLdsSamples / RD - 64));
        k->ncols = (64 + k->NB) | 1;
        k->nblocks = (I + k->NB * RD - 1) / (k->NB * RD);
        k->lds = size_t(RD) * k->ncols * sizeof(double2);
        const void* fn = R == 2 ? reinterpret_cast<const void*>(mgpu_chan_fir_r2_kernel) : reinterpret_cast<const void*>(mgpu_chan_fir_r1_kernel);
        need(k->lds <= size_t(kMaxLds), "LDS image larger than the kernel's limit");
        HIPCK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));   // the same for every channeliser
        k->line.make((size_t(T - 1) + size_t(k->max_out) * D) * sizeof(double2));
        k->d_g = DevArray<double2>(size_t(S) * T * sizeof(double2));
        k->d_rows = DevArray<ChanRow>(size_t(S) * sizeof(ChanRow));
        k->d_W = phasor_table_on_device();
        for (int s = 0; s < S; ++s) k->upload_row(s, c->stream);
    });
}

int mgpu_chan_destroy(mgpu_chan* k) { return destroy_stage(k); }

int mgpu_chan_latency(mgpu_chan* k) { return k ? k->L : -1; }

int mgpu_chan_seek(mgpu_chan* k, uint64_t position) {
    if (!k || position > (1ULL << 62)) return MGPU_ERR_ARG;
    k->pos = position;
    k->line.restart();
    return MGPU_OK;
}

int mgpu_chan_retune(mgpu_chan* k, int s, const mgpu_chan_channel* channel) { return retune_channel(k, s, channel); }

int mgpu_chan_process_dev(mgpu_chan* k, const void* d_iq, int format, int n_in, double* d_out, void* stream) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        k->check_n_in(d_iq, format, n_in, d_out);
        k->run(d_iq, format, n_in, d_out, stream_or_own(k->c, stream));
    });
}

int mgpu_chan_process(mgpu_chan* k, const void* iq, int format, int n_in, double* out) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        k->check_n_in(iq, format, n_in, out);
        hipStream_t st = k->c->stream;
        k->need_out();
        const void* d_iq = k->on_device(iq, format, n_in, st);
        k->run(d_iq, format, n_in, k->d_out, st);
        HIPCK(hipMemcpyAsync(out, k->d_out.p, size_t(k->S) * (n_in / k->D) * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
    });
}

int mgpu_capture_run_wideband(mgpu_capture* cap, mgpu_chan* k, const void* iq, int format, int H, mgpu_capture_event* events,
                              uint8_t* payloads, int max_events, int* n_events) {
    if (!cap || !k) return MGPU_ERR_ARG;
    mgpu_capture_geometry g{};
    if (!capture_pairs(cap, k->c, k->S, &g))
        return refuse(k->c, MGPU_ERR_ARG, capture_streams(cap) != k->S
                                              ? "mgpu_capture_run_wideband: the capture and the channeliser must have the same S"
                                              : "mgpu_capture_run_wideband: the capture and the channeliser must belong to one context");
    const int rc = guard(k->c, [&] {
        need(H > 0 && (long long)H * g.symbol_period <= k->max_out, "H * P must be 1..max_out");
        check_event_args(events, max_events, n_events);
        const int n_in = H * g.symbol_period * k->D;
        k->need_out();
        k->check_n_in(iq, format, n_in, k->d_out.p);
        hipStream_t st = k->c->stream;
        k->run(k->on_device(iq, format, n_in, st), format, n_in, k->d_out, st);
    });
    if (rc != MGPU_OK) return rc;
    // the capture runs on the same context's stream, behind the channeliser's kernels
    return mgpu_capture_run(cap, k->d_out.p, MGPU_SAMPLES_F64, H, events, payloads, max_events, n_events);
}

}  // extern "C"

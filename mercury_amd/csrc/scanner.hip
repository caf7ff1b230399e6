// Band scanner (include/ext/mercury_scanner.h): one IQ stream into spectrum lines [n][N] and a report of the occupied runs per line.
//
// Per call of m blocks, on one stream:
//   1. mgpu_scan_block_*_kernel, one workgroup per block: widens and windows the block's N samples in the load (the first H of the call's
//      first block are the history: the last H widened samples of the call before, zeros after a seek), runs the rule's transform in LDS
//      (scan_fft.h: N complex doubles, 64 KB at N = 4096, and nothing else) and writes P_b[f] to the workspace [m][N]. The call's last
//      block leaves its second half, widened, as the next call's history.
//   2. mgpu_scan_line_kernel, one thread per (f, line): adds the line's blocks of the call in ascending b, onto the carried partial line
//      where the line began in an earlier call, and either emits the line or leaves it as the next call's partial line.
//   3. mgpu_scan_detect_*_kernel, one workgroup per completed line: the level by radix selection over ballots, the occupancy bit mask in
//      LDS, gap closing and run extraction on the mask's words, the run sums in order.
// The history and the partial line are two buffers each that change roles (stream_stage.hpp History). Nothing else is kept between calls
// but the position, so how the stream is cut cannot change a line.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "scan_fft.h"
#include "scan_rule.hpp"
#include "stream_stage.hpp"

using namespace mgpu_scan_detail;

namespace {

struct BlockArgs {
    const void* iq;           // the call's m * H samples in `format`
    const sc2* hist_old;      // [H]: the samples before the call's first; null: zeros
    sc2* hist_new;            // [H]
    const sc2* tab;           // [N]
    const double* win;        // [N]
    double* P;                // [m][N]
    int format, m;
};

constexpr int kDetectThreads = 256;           // the detect kernel's workgroup: four wavefronts
constexpr int kFar = 1 << 20;                // no such bin within reach

}  // namespace

template <int L>
__device__ inline void scan_block(const BlockArgs& a) {
    using F = ScanFft<L>;
    constexpr int N = F::N, H = F::H, T = F::kThreads;
    __shared__ __attribute__((aligned(16))) sc2 s[N];
    const int t = threadIdx.x, b = blockIdx.x;
    const bool keeps_history = b == a.m - 1;
    // sample i of the block, windowed; every i is fetched once
    auto fetch = [&](int i) {
        const long long g = (long long)(b - 1) * H + i;
        sc2 x = {0.0, 0.0};
        if (g >= 0) {
            const double2 v = mgpu_fmt::load_iq(a.iq, a.format, size_t(g));
            x = {v.x, v.y};
        } else if (a.hist_old) x = a.hist_old[i];
        if (keeps_history && i >= H) a.hist_new[i - H] = x;
        const double w = a.win[i];
        return sc2{x.re * w, x.im * w};
    };
    if (L & 1) {
        for (int u = t; u < H; u += T) F::single(u, s, a.tab, fetch);
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < F::kRounds; ++r) {
        const bool from_samples = r == 0 && !(L & 1);
        for (int u = t; u < N / 4; u += T) F::round(r, u, s, a.tab, from_samples, fetch);
        __syncthreads();
    }
    double* const P = a.P + size_t(b) * N;
    for (int f = t; f < N; f += T) P[f] = F::power(f, s);
}

#define SCAN_BLOCK_KERNEL(L)                                                                                             \
    extern "C" __global__ __launch_bounds__(ScanFft<L>::kThreads) void mgpu_scan_block_##L##_kernel(BlockArgs a) { scan_block<L>(a); }
SCAN_BLOCK_KERNEL(8)
SCAN_BLOCK_KERNEL(9)
SCAN_BLOCK_KERNEL(10)
SCAN_BLOCK_KERNEL(11)
SCAN_BLOCK_KERNEL(12)

// grid: x over f in 256s, y over the segments of the call: segment sg is the blocks [sg A - a0, (sg + 1) A - a0) of the call, clipped to
// [0, m): segment 0 goes on the partial line of a0 blocks, a full segment is line sg of the call, a short last one the new partial line.
extern "C" __global__ __launch_bounds__(256) void mgpu_scan_line_kernel(const double* __restrict__ P, int m, int N, int a0, int A,
                                                                        const double* __restrict__ part_old, double* __restrict__ part_new,
                                                                        double* __restrict__ lines) {
    const int f = int(blockIdx.x) * 256 + int(threadIdx.x), sg = blockIdx.y;
    if (f >= N) return;
    const long long first = (long long)sg * A - a0, last = first + A;
    const int b0 = int(std::max(0ll, first)), b1 = int(std::min((long long)m, last));
    double acc = (sg == 0 && a0 > 0 && part_old) ? part_old[f] : 0.0;
    const double* const p = P + f;
    int b = b0;
    // one dependent chain in ascending b, as the rule has it; the loads are not: eight blocks' powers are fetched at a time
    for (; b + 8 <= b1; b += 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[size_t(b + j) * N];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = acc + v[j];
    }
    for (; b < b1; ++b) acc = acc + p[size_t(b) * N];
    if (last <= m) lines[size_t(sg) * N + f] = acc;
    else part_new[f] = acc;
}

// distance from bit `lane` of word w down (up) to the nearest set bit of the mask, looking one word further at most; kFar: none
__device__ inline int scan_below(const unsigned long long* m, int w, int lane, bool invert) {
    auto word = [&](int i) { return invert ? ~m[i] : m[i]; };
    const unsigned long long cur = word(w) & ((1ull << lane) - 1ull);
    if (cur) return lane - (63 - __clzll((long long)cur));
    if (w == 0) return kFar;
    const unsigned long long prev = word(w - 1);
    return prev ? lane + 1 + __clzll((long long)prev) : kFar;
}
__device__ inline int scan_above(const unsigned long long* m, int w, int W, int lane, bool invert) {
    auto word = [&](int i) { return invert ? ~m[i] : m[i]; };
    const unsigned long long cur = lane < 63 ? word(w) >> (lane + 1) : 0ull;
    if (cur) return __ffsll((long long)cur);
    if (w + 1 >= W) return kFar;
    const unsigned long long next = word(w + 1);
    return next ? (63 - lane) + __ffsll((long long)next) : kFar;
}
// the first set (clear) bit of the mask at or after f; N: none
__device__ inline int scan_next(const unsigned long long* m, int f, int N, bool clear) {
    if (f >= N) return N;
    int w = f >> 6;
    unsigned long long cur = (clear ? ~m[w] : m[w]) & (~0ull << (f & 63));
    while (!cur) {
        if (++w >= N / 64) return N;
        cur = clear ? ~m[w] : m[w];
    }
    return 64 * w + __ffsll((long long)cur) - 1;
}

// One workgroup of four wavefronts per completed line; thread t has the bins 256 i + t, i < K = N / 256, bit `lane` of mask word 4 i + wave,
// with their keys in registers. All counts are integers and every sum has the rule's order, so no order of execution changes a bit.
// The selection costs one barrier per bit: a wavefront's count of the bit goes to cnt[bit & 1][wave], and a wavefront can be at most one
// bit ahead of another, which writes the other half.
template <int L>
__device__ inline void scan_detect(const double* __restrict__ lines, const mgpu_scan_config& k, uint64_t first_block,
                                   mgpu_scan_report* __restrict__ reports) {
    constexpr int N = 1 << L, W = N / 64, K = N / kDetectThreads;
    __shared__ double v[N];
    __shared__ unsigned long long use[W], occ[W], fin[W];
    __shared__ int cnt[2][kDetectThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double* const line = lines + size_t(blockIdx.x) * N;
    unsigned long long key[K];
    bool us[K], o[K];
    bool bad = false;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int f = kDetectThreads * i + t;
        const double x = line[f];
        v[f] = x;
        us[i] = f >= k.edge_bins && f <= N - 1 - k.edge_bins && (k.dc_bins == 0 || abs(f - N / 2) > k.dc_bins);
        key[i] = static_cast<unsigned long long>(__double_as_longlong(x)) & kScanKeyMask;
        bad = bad || (us[i] && key[i] >= kScanKeyInf);
        const unsigned long long mk = __ballot(us[i]);
        if (lane == 0) use[4 * i + wave] = mk;
    }
    const int nonfinite = __syncthreads_or(bad) ? 1 : 0;            // the barrier behind v and use, too
    int n_runs = 0, my_first = 0, my_count = 0;
    double level = 0.0;
    if (!nonfinite) {                                               // uniform
        int rank = 0;
        for (int w = 0; w < W; ++w) rank += __popcll(use[w]);
        rank /= 2;
        // the selection, bit by bit from the top of the key: a bin is still in while its key agrees with the prefix above the bit
        unsigned long long prefix = 0;
        for (int bit = 62; bit >= 0; --bit) {
            int zeros = 0;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const bool in = us[i] && ((key[i] ^ prefix) >> (bit + 1)) == 0;
                zeros += __popcll(__ballot(in && !((key[i] >> bit) & 1ull)));
            }
            int* const c = cnt[bit & 1];
            if (lane == 0) c[wave] = zeros;
            __syncthreads();
            const int all = c[0] + c[1] + c[2] + c[3];
            if (rank >= all) { rank -= all; prefix |= 1ull << bit; }             // uniform: the counts are the workgroup's
        }
        level = __longlong_as_double(static_cast<long long>(prefix));
        const double limit = k.threshold * level;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            o[i] = us[i] && !(v[kDetectThreads * i + t] <= limit);                // the thread's own entry of v
            const unsigned long long mk = __ballot(o[i]);
            if (lane == 0) occ[4 * i + wave] = mk;
        }
        __syncthreads();
        // a gap: unoccupied and usable, the nearest occupied bins on both sides at most gap + 1 apart and no excluded bin between them
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const int w = 4 * i + wave;
            bool closed = false;
            if (us[i] && !o[i]) {
                const int dp = scan_below(occ, w, lane, false), dn = scan_above(occ, w, W, lane, false);
                closed = dp + dn - 1 <= k.gap && scan_below(use, w, lane, true) > dp && scan_above(use, w, W, lane, true) > dn;
            }
            const unsigned long long mk = __ballot(o[i] || closed);
            if (lane == 0) fin[w] = mk;
        }
        __syncthreads();
        // every lane of the first wavefront walks the runs; lane r keeps run r
        if (wave == 0)
            for (int f = scan_next(fin, 0, N, false); f < N;) {
                const int e = scan_next(fin, f, N, true);
                if (e - f >= k.min_bins) {
                    if (n_runs == lane) { my_first = f; my_count = e - f; }
                    ++n_runs;
                }
                f = scan_next(fin, e, N, false);
            }
    }
    if (wave != 0) return;
    mgpu_scan_report* const rep = reports + blockIdx.x;
    const int reported = min(n_runs, k.max_runs);
    if (lane < MGPU_SCAN_MAX_RUNS) {
        mgpu_scan_run run;
        memset(&run, 0, sizeof(run));
        if (lane < reported) {
            run.first = my_first;
            run.count = my_count;
            run.peak = my_first;
            double power = 0.0, top = v[my_first];
            for (int i = my_first; i < my_first + my_count; ++i) {
                const double x = v[i];
                if (x > top) { top = x; run.peak = i; }
                power = power + x;
            }
            run.power = power;
        }
        rep->runs[lane] = run;
    }
    if (lane == 0) {
        rep->first_block = first_block + uint64_t(blockIdx.x) * uint64_t(k.blocks_per_line);
        rep->level = level;
        rep->n_runs = n_runs;
        rep->reported = reported;
        rep->nonfinite = nonfinite;
        rep->pad = 0;
    }
}

#define SCAN_DETECT_KERNEL(L)                                                                                                         \
    extern "C" __global__ __launch_bounds__(kDetectThreads) void mgpu_scan_detect_##L##_kernel(const double* __restrict__ lines, mgpu_scan_config k, \
                                                                                                uint64_t first_block,                 \
                                                                                                mgpu_scan_report* __restrict__ reports) { \
        scan_detect<L>(lines, k, first_block, reports);                                                                               \
    }
SCAN_DETECT_KERNEL(8)
SCAN_DETECT_KERNEL(9)
SCAN_DETECT_KERNEL(10)
SCAN_DETECT_KERNEL(11)
SCAN_DETECT_KERNEL(12)

struct mgpu_scan {
    mgpu_ctx* c = nullptr;
    mgpu_scan_config cfg{};
    int N = 0, H = 0, A = 0, max_in = 0, max_blocks = 0, max_lines = 0;
    uint64_t pos = 0;
    History<sc2> hist;                            // [H] the last H widened samples
    History<double> part;                         // [N] the partial line
    DevArray<sc2> d_tab;                          // [N]
    DevArray<double> d_win;                       // [N]
    DevArray<double> d_P;                         // [max_blocks][N] the blocks' powers
    DevArray<char> d_stage;                       // host input's landing area (ctx.hpp staged_on_device)
    DevArray<double> d_lines;                     // process()'s output [max_lines][N], [max_lines] (made on first use)
    DevArray<mgpu_scan_report> d_reports;

    // the lines a call of n_in samples completes, or -1 where n_in is refused
    int lines_of(int n_in) const {
        if (n_in < H || n_in % H || n_in > max_in || pos + uint64_t(n_in) > kMaxPosition) return -1;
        return int(lines_completed(pos / uint64_t(H), uint64_t(n_in / H), A));
    }

    int check_in(const void* iq, int format, int n_in, const void* lines, const void* reports) const {
        need(iq != nullptr, "null pointer");
        need_iq_format(format);
        const int n = lines_of(n_in);
        need(n >= 0, "n_in must be a positive multiple of H, max_in at most, and the position stay below 2^62");
        need(n == 0 || (lines && reports), "null pointer");
        return n;
    }

    // one call on device memory: n = lines_of(n_in) lines into d_l [n][N] and d_r [n]
    void run(const void* d_iq, int format, int n_in, int n, double* d_l, mgpu_scan_report* d_r, hipStream_t st) {
        const int m = n_in / H;
        const uint64_t j = pos / uint64_t(H);
        const int a0 = int(j % uint64_t(A));
        BlockArgs a{};
        a.iq = d_iq; a.hist_old = hist.old(); a.hist_new = hist.next(); a.tab = d_tab; a.win = d_win; a.P = d_P; a.format = format; a.m = m;
        switch (cfg.log2n) {
            case 8: hipLaunchKernelGGL(mgpu_scan_block_8_kernel, dim3(m), dim3(ScanFft<8>::kThreads), 0, st, a); break;
            case 9: hipLaunchKernelGGL(mgpu_scan_block_9_kernel, dim3(m), dim3(ScanFft<9>::kThreads), 0, st, a); break;
            case 10: hipLaunchKernelGGL(mgpu_scan_block_10_kernel, dim3(m), dim3(ScanFft<10>::kThreads), 0, st, a); break;
            case 11: hipLaunchKernelGGL(mgpu_scan_block_11_kernel, dim3(m), dim3(ScanFft<11>::kThreads), 0, st, a); break;
            default: hipLaunchKernelGGL(mgpu_scan_block_12_kernel, dim3(m), dim3(ScanFft<12>::kThreads), 0, st, a); break;
        }
        HIPCK(hipGetLastError());
        const int segments = (a0 + m + A - 1) / A;
        hipLaunchKernelGGL(mgpu_scan_line_kernel, dim3(unsigned((N + 255) / 256), unsigned(segments)), dim3(256), 0, st,
                           static_cast<const double*>(d_P), m, N, a0, A, part.old(), part.next(), d_l);
        HIPCK(hipGetLastError());
        if (n > 0) {
            auto* detect = cfg.log2n == 8 ? mgpu_scan_detect_8_kernel : cfg.log2n == 9 ? mgpu_scan_detect_9_kernel
                           : cfg.log2n == 10 ? mgpu_scan_detect_10_kernel : cfg.log2n == 11 ? mgpu_scan_detect_11_kernel
                                                                                            : mgpu_scan_detect_12_kernel;
            hipLaunchKernelGGL(detect, dim3(unsigned(n)), dim3(kDetectThreads), 0, st, static_cast<const double*>(d_l), cfg,
                               (j / uint64_t(A)) * uint64_t(A), d_r);
            HIPCK(hipGetLastError());
        }
        hist.advance();
        if ((a0 + m) % A) part.advance();         // a partial line was written
        else part.restart();                      // the call ended on a line's end: the next line starts from +0.0
        pos += uint64_t(n_in);
    }
};

extern "C" {

int mgpu_scan_create(mgpu_ctx* c, const mgpu_scan_config* kc, mgpu_scan** out) {
    return create_stage(c, out, "mgpu_scan_create", config_error(kc), [&](mgpu_scan* k) {
        k->cfg = *kc;
        const int N = k->N = 1 << kc->log2n, H = k->H = N / 2;
        k->A = kc->blocks_per_line;
        k->max_in = k->cfg.max_in = kc->max_in ? kc->max_in : kDefaultBlocksIn * H;
        need(k->max_in <= kMaxIn, "max_in must be at most 2^26");
        k->max_blocks = k->max_in / H;
        k->max_lines = (k->max_blocks + k->A - 1) / k->A;
        need(k->max_blocks <= 65535 * k->A, "max_in / H must be at most 65535 blocks_per_line");      // the line kernel's grid y
        const Tables T(kc->log2n);
        k->d_tab = DevArray<sc2>(size_t(N) * sizeof(sc2));
        k->d_win = DevArray<double>(size_t(N) * 8);
        k->d_P = DevArray<double>(size_t(k->max_blocks) * N * 8);
        k->hist.make(size_t(H) * sizeof(sc2));
        k->part.make(size_t(N) * 8);
        HIPCK(hipMemcpy(k->d_tab.p, T.tab.data(), size_t(N) * 16, hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(k->d_win.p, T.win.data(), size_t(N) * 8, hipMemcpyHostToDevice));
    });
}

int mgpu_scan_destroy(mgpu_scan* k) { return destroy_stage(k); }

int mgpu_scan_seek(mgpu_scan* k, uint64_t position) {
    if (!k || position > kMaxPosition || position % (uint64_t(k->H) * uint64_t(k->A))) return MGPU_ERR_ARG;
    k->pos = position;
    k->hist.restart();
    k->part.restart();
    return MGPU_OK;
}

int mgpu_scan_lines(mgpu_scan* k, int n_in) { return k ? k->lines_of(n_in) : -1; }

int mgpu_scan_process_dev(mgpu_scan* k, const void* d_iq, int format, int n_in, double* d_lines, mgpu_scan_report* d_reports, int* n_lines,
                          void* stream) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        const int n = k->check_in(d_iq, format, n_in, d_lines, d_reports);
        k->run(d_iq, format, n_in, n, d_lines, d_reports, stream_or_own(k->c, stream));
        if (n_lines) *n_lines = n;
    });
}

int mgpu_scan_process(mgpu_scan* k, const void* iq, int format, int n_in, double* lines, mgpu_scan_report* reports, int* n_lines) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        const int n = k->check_in(iq, format, n_in, lines, reports);
        hipStream_t st = k->c->stream;
        if (!k->d_lines.p) {
            k->d_lines = DevArray<double>(size_t(k->max_lines) * k->N * 8);
            k->d_reports = DevArray<mgpu_scan_report>(size_t(k->max_lines) * sizeof(mgpu_scan_report));
        }
        const void* d_iq = staged_iq(k->d_stage, iq, format, n_in, st);
        k->run(d_iq, format, n_in, n, k->d_lines, k->d_reports, st);
        if (n > 0) {
            HIPCK(hipMemcpyAsync(lines, k->d_lines.p, size_t(n) * k->N * 8, hipMemcpyDeviceToHost, st));
            HIPCK(hipMemcpyAsync(reports, k->d_reports.p, size_t(n) * sizeof(mgpu_scan_report), hipMemcpyDeviceToHost, st));
        }
        HIPCK(hipStreamSynchronize(st));
        if (n_lines) *n_lines = n;
    });
}

int mgpu_scan_status(mgpu_scan* k, mgpu_scan_state* state) {
    if (!k || !state) return MGPU_ERR_ARG;
    *state = mgpu_scan_state{};
    state->position = k->pos;
    state->blocks = k->pos / uint64_t(k->H);
    state->lines = state->blocks / uint64_t(k->A);
    state->D = k->cfg.D; state->log2n = k->cfg.log2n; state->blocks_per_line = k->A; state->max_in = k->max_in;
    return MGPU_OK;
}

int mgpu_host_scan_process(const mgpu_scan_config* kc, const void* iq, int format, int n_in, uint64_t position, double* lines,
                           mgpu_scan_report* reports, int* n_lines) {
    return host_try([&] { return host_process(kc, iq, format, n_in, position, lines, reports, n_lines); });
}

int mgpu_host_scan_plan(const mgpu_scan_config* kc, const mgpu_scan_run* run, int sideband, int audio_centre_hz, mgpu_chan_channel* channel) {
    if (config_error(kc) || !run || !channel || (sideband != 0 && sideband != 1)) return MGPU_ERR_ARG;
    const int N = 1 << kc->log2n;
    if (run->first < 0 || run->count < 1 || run->first + run->count > N) return MGPU_ERR_ARG;
    const double R = 48000.0 * kc->D;
    const double centre = ((run->first + (run->count - 1) / 2.0) - N / 2) * R / N;
    const mgpu_chan_channel ch{int(std::lround(centre - (sideband ? -1.0 : 1.0) * audio_centre_hz)), sideband, 1.0};
    if (mgpu_chan_detail::channel_error(kc->D, audio_centre_hz, &ch)) return MGPU_ERR_ARG;
    *channel = ch;
    return MGPU_OK;
}

}  // extern "C"

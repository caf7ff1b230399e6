// Wideband impulse blanker (include/ext/mercury_wideband_blanker.h): one IQ stream at 48000 * D out again in its own format, one block
// late, with the samples the rule marks replaced by zero.
//
// Per call of m blocks, on one stream:
//   1. mgpu_wblank_analyse_*_kernel, one workgroup of four wavefronts per block of the call: loads the block's samples (one 4-, 8- or
//      16-byte load per sample, widened in the load), keeps thread t's powers 256 i + t, i < K <= 16, in registers, selects the median
//      bit by bit over ballots (integer counts only: no order of execution changes it), and writes the exceed flags, one 64-bit word per
//      64 samples and all zeros where the block is capped, and the block's {level, exceeding, capped}.
//   2. mgpu_wblank_emit_*_kernel, one workgroup per emitted block: the block before the call's first (the held block: zeros on a fresh
//      stream) and the call's blocks but the last. A sample is marked from its own flag word and the words on either side (guard <= 64);
//      the raw samples are read again and written as they are or as zeros; the block's report is written. The workgroup of the last
//      emitted block copies the call's last block, its flag words (with the last word of the block before) and its figures into the
//      history.
// The held block and its words are two buffers each that change roles (stream_stage.hpp History). Nothing else is kept between calls but
// the position, so how the stream is cut cannot change a byte.
#include <cstring>

#include "stream_stage.hpp"
#include "wblank_rule.hpp"

using namespace mgpu_wblank_detail;

namespace {

constexpr int kThreads = 256;                     // both kernels' workgroup: four wavefronts

struct BlockInfo {                                // what analyse leaves of a block for its report
    double level;
    int exceeding, capped;
};

struct AnalyseArgs {
    const void* iq;                               // the call's m * B samples
    unsigned long long* flags;                    // [m][W]
    BlockInfo* info;                              // [m]
    double threshold;
    int format, B, cap;
};

// The history's words: [0] the last flag word of the block before the held one, [1 .. W] the held block's, [W + 1] its level's bits,
// [W + 2] exceeding | capped << 32
struct EmitArgs {
    const void* iq;                               // the call's m * B samples
    void* out;                                    // [m * B]
    const void* held_old;                         // [B] the block before the call's first; null: a fresh stream
    void* held_new;                               // [B]
    const unsigned long long* words_old;          // [W + 3]; null: a fresh stream
    unsigned long long* words_new;                // [W + 3]
    const unsigned long long* flags;              // [m][W]
    const BlockInfo* info;                        // [m]
    mgpu_wblank_report* reports;                  // [m]; null: not wanted
    long long first_block;                        // the block the call's first report describes
    int B, m, guard;
};

}  // namespace

__device__ inline double wblank_power(const double2 v) { return v.x * v.x + v.y * v.y; }

// Thread t has the samples 256 i + t of the block, i < K: bit `lane` of flag word 4 i + wave. The selection costs one barrier per bit: a
// wavefront's count of the bit goes to cnt[bit & 1][wave], and a wavefront can be at most one bit ahead of another, which writes the
// other half.
template <int K>
__device__ inline void wblank_analyse(const AnalyseArgs& a) {
    __shared__ int cnt[2][kThreads / 64], exceeding[kThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, B = a.B;
    const size_t first = size_t(blockIdx.x) * size_t(B);
    double p[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int f = kThreads * i + t;
        p[i] = f < B ? wblank_power(mgpu_fmt::load_iq(a.iq, a.format, first + size_t(f))) : 0.0;
    }
    auto key = [&](int i) { return static_cast<unsigned long long>(__double_as_longlong(p[i])) & kWblankKeyMask; };
    int rank = B / 2;
    unsigned long long prefix = 0;
    for (int bit = 62; bit >= 0; --bit) {
        int zeros = 0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const bool in = kThreads * i + t < B && ((key(i) ^ prefix) >> (bit + 1)) == 0;
            zeros += __popcll(__ballot(in && !((key(i) >> bit) & 1ull)));
        }
        int* const c = cnt[bit & 1];
        if (lane == 0) c[wave] = zeros;
        __syncthreads();
        const int all = c[0] + c[1] + c[2] + c[3];
        if (rank >= all) { rank -= all; prefix |= 1ull << bit; }                 // uniform: the counts are the workgroup's
    }
    const double level = __longlong_as_double(static_cast<long long>(prefix));
    const double limit = a.threshold * level;
    int mine = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) mine += __popcll(__ballot(kThreads * i + t < B && !(p[i] <= limit)));
    if (lane == 0) exceeding[wave] = mine;
    __syncthreads();
    const int E = exceeding[0] + exceeding[1] + exceeding[2] + exceeding[3];
    const bool capped = E > a.cap;
    const int W = B / 64;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const unsigned long long word = __ballot(kThreads * i + t < B && !(p[i] <= limit));
        const int w = 4 * i + wave;
        if (lane == 0 && w < W) a.flags[size_t(blockIdx.x) * size_t(W) + size_t(w)] = capped ? 0ull : word;
    }
    if (t == 0) a.info[blockIdx.x] = BlockInfo{level, E, capped ? 1 : 0};
}

#define WBLANK_ANALYSE_KERNEL(K)                                                                                                  \
    extern "C" __global__ __launch_bounds__(kThreads) void mgpu_wblank_analyse_##K##_kernel(AnalyseArgs a) { wblank_analyse<K>(a); }
WBLANK_ANALYSE_KERNEL(1)
WBLANK_ANALYSE_KERNEL(4)
WBLANK_ANALYSE_KERNEL(16)

// bits a .. b of a word, 0 <= a <= b <= 63
__device__ inline unsigned long long wblank_bits(int a, int b) { return (~0ull >> (63 - b)) & (~0ull << a); }

// T: an integer carrier of one sample's bytes
template <typename T>
__device__ inline void wblank_emit(const EmitArgs& a) {
    __shared__ int blanked[kThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, B = a.B, W = B / 64, k = blockIdx.x, g = a.guard;
    // word i of the stream of flag words that begins with the history's W + 1
    auto word = [&](size_t i) { return i < size_t(W) + 1 ? (a.words_old ? a.words_old[i] : 0ull) : a.flags[i - size_t(W) - 1]; };
    const bool fresh = k == 0 && !a.held_old;
    const T* const src = k == 0 ? static_cast<const T*>(a.held_old) : static_cast<const T*>(a.iq) + size_t(k - 1) * size_t(B);
    T* const dst = static_cast<T*>(a.out) + size_t(k) * size_t(B);
    int mine = 0;
    for (int f = t; f < B; f += kThreads) {
        bool marked = false;
        T x{};
        if (!fresh) {
            const size_t at = 1 + size_t(k) * size_t(W) + size_t(f >> 6);
            const int lo = lane - g, hi = lane + g;                              // -64 <= lo, hi <= 127
            marked = (word(at) & wblank_bits(max(lo, 0), min(hi, 63))) != 0;
            if (lo < 0) marked = marked || (word(at - 1) & wblank_bits(64 + lo, 63)) != 0;
            if (hi > 63) marked = marked || (word(at + 1) & wblank_bits(0, hi - 64)) != 0;
            x = src[f];
        }
        dst[f] = marked ? T{} : x;
        mine += __popcll(__ballot(marked));
    }
    if (lane == 0) blanked[wave] = mine;
    __syncthreads();
    if (t == 0 && a.reports) {
        mgpu_wblank_report r;
        r.block = a.first_block + k;
        r.level = 0.0, r.exceeding = 0, r.blanked = 0, r.capped = 0, r.pad = 0;
        if (!fresh) {
            if (k == 0) {
                const unsigned long long counts = a.words_old[W + 2];
                r.level = __longlong_as_double(static_cast<long long>(a.words_old[W + 1]));
                r.exceeding = int(counts & 0xffffffffull), r.capped = int(counts >> 32);
            } else {
                const BlockInfo in = a.info[k - 1];
                r.level = in.level, r.exceeding = in.exceeding, r.capped = in.capped;
            }
            r.blanked = blanked[0] + blanked[1] + blanked[2] + blanked[3];
        }
        a.reports[k] = r;
    }
    if (k != a.m - 1) return;
    // the call's last block becomes the held one
    const T* const last = static_cast<const T*>(a.iq) + size_t(a.m - 1) * size_t(B);
    for (int f = t; f < B; f += kThreads) static_cast<T*>(a.held_new)[f] = last[f];
    for (int i = t; i < W + 1; i += kThreads) a.words_new[i] = word(size_t(a.m) * size_t(W) + size_t(i));
    if (t == 0) {
        const BlockInfo in = a.info[a.m - 1];
        a.words_new[W + 1] = static_cast<unsigned long long>(__double_as_longlong(in.level));
        a.words_new[W + 2] = static_cast<unsigned long long>(unsigned(in.exceeding)) | static_cast<unsigned long long>(unsigned(in.capped)) << 32;
    }
}

extern "C" __global__ __launch_bounds__(kThreads) void mgpu_wblank_emit_4_kernel(EmitArgs a) { wblank_emit<unsigned>(a); }
extern "C" __global__ __launch_bounds__(kThreads) void mgpu_wblank_emit_8_kernel(EmitArgs a) { wblank_emit<unsigned long long>(a); }
extern "C" __global__ __launch_bounds__(kThreads) void mgpu_wblank_emit_16_kernel(EmitArgs a) { wblank_emit<ulonglong2>(a); }

struct mgpu_wblank : BlockStage<mgpu_wblank_report> {
    mgpu_wblank_config cfg{};
    int W = 0, cap = 0;
    History<char> held;                           // [B] samples: the block that waits for its successor
    History<unsigned long long> words;            // [W + 3]: its flag words and figures (EmitArgs)
    DevArray<unsigned long long> d_flags;         // [max_blocks][W]
    DevArray<BlockInfo> d_info;                   // [max_blocks]

    // one call on device memory: m = n_in / B blocks into d_o [n_in] and d_r [m] (null: no reports)
    void run(const void* d_iq, int m, void* d_o, mgpu_wblank_report* d_r, hipStream_t st) {
        AnalyseArgs an{};
        an.iq = d_iq; an.flags = d_flags; an.info = d_info; an.threshold = cfg.threshold; an.format = cfg.format; an.B = B; an.cap = cap;
        auto* analyse = B <= kThreads ? mgpu_wblank_analyse_1_kernel : B <= 4 * kThreads ? mgpu_wblank_analyse_4_kernel
                                                                                         : mgpu_wblank_analyse_16_kernel;
        hipLaunchKernelGGL(analyse, dim3(unsigned(m)), dim3(kThreads), 0, st, an);
        HIPCK(hipGetLastError());
        EmitArgs em{};
        em.iq = d_iq; em.out = d_o; em.held_old = held.old(); em.held_new = held.next(); em.words_old = words.old();
        em.words_new = words.next(); em.flags = d_flags; em.info = d_info; em.reports = d_r;
        em.first_block = (long long)(pos / uint64_t(B)) - 1; em.B = B; em.m = m; em.guard = cfg.guard;
        auto* emit = bytes == 4 ? mgpu_wblank_emit_4_kernel : bytes == 8 ? mgpu_wblank_emit_8_kernel : mgpu_wblank_emit_16_kernel;
        hipLaunchKernelGGL(emit, dim3(unsigned(m)), dim3(kThreads), 0, st, em);
        HIPCK(hipGetLastError());
        held.advance();
        words.advance();
        pos += uint64_t(m) * uint64_t(B);
    }
};

extern "C" {

int mgpu_wblank_create(mgpu_ctx* c, const mgpu_wblank_config* kc, mgpu_wblank** out) {
    return create_stage(c, out, "mgpu_wblank_create", config_error(kc), [&](mgpu_wblank* k) {
        k->cfg = *kc;
        const int B = block_of(*kc);
        block_shape(k, B, kDefaultBlocksIn);
        k->W = B / 64;
        k->cap = cap_of(*kc);
        k->held.make(size_t(B) * k->bytes);
        k->words.make(size_t(k->W + 3) * 8);
        k->d_flags = DevArray<unsigned long long>(size_t(k->max_blocks) * size_t(k->W) * 8);
        k->d_info = DevArray<BlockInfo>(size_t(k->max_blocks) * sizeof(BlockInfo));
    });
}

int mgpu_wblank_destroy(mgpu_wblank* k) { return destroy_stage(k); }

int mgpu_wblank_seek(mgpu_wblank* k, uint64_t position) {
    return block_seek(k, position, [&] {
        k->held.restart();
        k->words.restart();
    });
}

int mgpu_wblank_status(mgpu_wblank* k, mgpu_wblank_state* state) {
    if (!k || !state) return MGPU_ERR_ARG;
    *state = mgpu_wblank_state{};
    state->position = k->pos;
    state->blocks = k->pos / uint64_t(k->B);
    state->D = k->cfg.D; state->block = k->B; state->cap = k->cap; state->max_in = k->max_in; state->format = k->cfg.format;
    state->delay = k->B;
    return MGPU_OK;
}

int mgpu_wblank_process_dev(mgpu_wblank* k, const void* d_iq, int n_in, void* d_out, mgpu_wblank_report* d_reports, int* n_reports,
                            void* stream) {
    return block_process_dev(k, d_iq, n_in, d_out, d_reports, n_reports, stream);
}

int mgpu_wblank_process(mgpu_wblank* k, const void* iq, int n_in, void* out, mgpu_wblank_report* reports, int* n_reports) {
    return block_process(k, iq, n_in, out, reports, n_reports);
}

int mgpu_host_wblank_process(const mgpu_wblank_config* kc, const void* iq, int n_in, uint64_t position, void* out,
                             mgpu_wblank_report* reports, int* n_reports) {
    return host_try([&] { return host_process(kc, iq, n_in, position, out, reports, n_reports); });
}

}  // extern "C"

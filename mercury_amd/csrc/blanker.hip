// The impulse blanker (include/mercury_blanker.h): the kernel, its launcher for the head of the fused span (launch.hip), the context's
// setting, the stage on its own and the host twin.
#include <algorithm>
#include <cstring>
#include <memory>

#include "ctx.hpp"

namespace {
constexpr int kBlankThreads = 256;      // four wavefronts per frame
constexpr int kBlankOwn = 8;            // samples of a block a lane owns at most: blocks (symbol lengths) up to 512 samples
}  // namespace

// One workgroup per frame. LDS, in 64-bit words, W = ceil(n / 64): the exceed flags of the frame, one bit per sample, with a zero word on
// either side ([W + 2]); the marked flags ([W]); the count. Bit-packed words keep mode 0's 13,056 samples in 3.2 KB, and every access is
// either a run of consecutive 8-byte words across the lanes or one word for a whole wavefront (a broadcast): no bank is asked twice.
// 1. The wavefronts take the frame's blocks in turn. A lane owns samples lane, lane + 64, ... of the block (16-byte loads, coalesced) and
//    keeps their powers in registers. The median is selected exactly, bit by bit from the top of the key: of the values still matching
//    the prefix, those with a 0 in this bit are counted by ballot and popcount, and the wanted rank says on which side the median lies. 63
//    steps of at most five ballots; integer counts, so no order of execution changes the result. Lanes beyond a short block's end own
//    nothing and never enter a ballot. Each ballot of exceeding samples is 64 consecutive flags: one lane ORs it into the two words it
//    straddles (LDS integer atomics: two wavefronts' blocks can share a word).
// 2. Behind a barrier every thread dilates words by the guard from its two neighbours, clips the last word at the frame's end, keeps the
//    marked word and adds its popcount to the count (integer atomic).
// 3. Behind a second barrier every thread knows marked <= cap; the input, cache-resident by now, is read again and written out with the
//    marked samples zeroed, or unchanged.
extern "C" __global__ __launch_bounds__(kBlankThreads) void mgpu_blanker_kernel(const double* __restrict__ in, size_t in_stride, int n, int L,
                                                                               double threshold, int guard, int cap, int F,
                                                                               double* __restrict__ out, int* __restrict__ report) {
    extern __shared__ unsigned long long blank_lds[];
    const int f = blockIdx.x, tid = threadIdx.x;
    if (f >= F) return;
    const int W = (n + 63) >> 6;
    unsigned long long* const exceed = blank_lds + 1;          // exceed[-1] and exceed[W] stay zero
    unsigned long long* const marked = blank_lds + W + 2;
    int* const count = reinterpret_cast<int*>(marked + W);
    const double2* const x = reinterpret_cast<const double2*>(in) + size_t(f) * in_stride;
    double2* const y = reinterpret_cast<double2*>(out) + size_t(f) * size_t(n);
    for (int i = tid; i < W + 2; i += kBlankThreads) blank_lds[i] = 0;
    if (tid == 0) *count = 0;
    __syncthreads();

    const int wave = tid >> 6, lane = tid & 63;
    const int nblocks = (n + L - 1) / L, own = (L + 63) >> 6;
    for (int b = wave; b < nblocks; b += kBlankThreads / 64) {
        const int base = b * L, m = min(L, n - base);
        double p[kBlankOwn];
        unsigned long long key[kBlankOwn];
        unsigned alive = 0;                                    // bit k: the lane's k-th sample exists and still matches the prefix
#pragma unroll
        for (int k = 0; k < kBlankOwn; ++k) {
            p[k] = 0;
            key[k] = 0;
            if (k < own && k * 64 + lane < m) {
                const double2 v = x[base + k * 64 + lane];
                p[k] = v.x * v.x + v.y * v.y;
                key[k] = static_cast<unsigned long long>(__double_as_longlong(p[k])) & kKeyMask;
                alive |= 1u << k;
            }
        }
        const unsigned valid = alive;
        int rank = m >> 1;
        unsigned long long prefix = 0;
        for (int bit = 62; bit >= 0; --bit) {
            int zeros = 0;
#pragma unroll
            for (int k = 0; k < kBlankOwn; ++k)
                if (k < own) zeros += __popcll(__ballot(((alive >> k) & 1u) && !((key[k] >> bit) & 1ull)));
            const bool one = rank >= zeros;                    // uniform: the ballots are the wavefront's
            if (one) { rank -= zeros; prefix |= 1ull << bit; }
#pragma unroll
            for (int k = 0; k < kBlankOwn; ++k)
                if (k < own && bool((key[k] >> bit) & 1ull) != one) alive &= ~(1u << k);
        }
        const double limit = threshold * __longlong_as_double(static_cast<long long>(prefix));
#pragma unroll
        for (int k = 0; k < kBlankOwn; ++k) {
            if (k >= own) continue;
            const unsigned long long hit = __ballot(((valid >> k) & 1u) && !(p[k] <= limit));
            if (lane == 0 && hit) {
                const int first = base + k * 64, w = first >> 6, sh = first & 63;
                atomicOr(exceed + w, hit << sh);
                if (sh && (hit >> (64 - sh))) atomicOr(exceed + w + 1, hit >> (64 - sh));      // set bits lie below n: w + 1 < W
            }
        }
    }
    __syncthreads();

    for (int w = tid; w < W; w += kBlankThreads) {
        const unsigned long long lo = exceed[w - 1], me = exceed[w], hi = exceed[w + 1];
        unsigned long long mk = me;
        for (int d = 1; d <= guard; ++d) mk |= (me << d) | (lo >> (64 - d)) | (me >> d) | (hi << (64 - d));
        if (w == W - 1 && (n & 63)) mk &= (1ull << (n & 63)) - 1;
        marked[w] = mk;
        if (mk) atomicAdd(count, __popcll(mk));
    }
    __syncthreads();

    const int total = *count;
    const bool blank = total <= cap;
    for (int i = tid; i < n; i += kBlankThreads) {
        double2 v = x[i];
        if (blank && ((marked[i >> 6] >> (i & 63)) & 1ull)) v = double2{0.0, 0.0};
        y[i] = v;
    }
    if (report && tid == 0) reinterpret_cast<int2*>(report)[f] = int2{total, blank ? total : 0};
}

namespace mgpu_detail {

// the arguments of a parameter set, or std::invalid_argument
static void blanker_check(const mgpu_blanker_params& q) {
    need(std::isfinite(q.threshold) && q.threshold >= 2.0, "blanker: threshold must be finite and at least 2");
    need(q.guard >= 0 && q.guard <= 16, "blanker: guard must be 0..16 samples");
    need(q.max_share > 0.0 && q.max_share <= 0.5, "blanker: max_share must be in (0, 0.5]");
}
static int blanker_cap(const mgpu_blanker_params& q, int n) { return int(std::floor(q.max_share * double(n))); }

void launch_blanker(mgpu_ctx* c, const double* d_in, int F, size_t in_stride, double* d_out, int* d_report, hipStream_t s) {
    const auto& t = c->tab;
    const int n = t.frame_samples, L = t.Nofdm;
    const mgpu_blanker_params& q = c->blk.params;
    need(n > 0 && L > 0 && L <= 64 * kBlankOwn, "blanker: the mode's symbol length is outside the kernel's blocks (at most 512 samples)");
    const size_t W = size_t(n + 63) / 64, lds = (2 * W + 2) * 8 + 8;
    need(lds <= size_t(64) * 1024, "blanker: frame too long for the flag arrays");
    for_frame_chunks(F, [&](int off, int m) {
        hipLaunchKernelGGL(mgpu_blanker_kernel, dim3(m), dim3(kBlankThreads), lds, s, d_in + size_t(off) * in_stride * 2, in_stride, n, L, q.threshold,
                           q.guard, blanker_cap(q, n), m, d_out + size_t(off) * size_t(n) * 2, at(d_report, size_t(off) * 2));
        HIPCK(hipGetLastError());
    });
}

SpanIo blanked_span(mgpu_ctx* c, const SpanIo& io, int F, hipStream_t s, hipEvent_t input_free) {
    const size_t n = size_t(c->tab.frame_samples);
    need(size_t(io.frame0) + size_t(F) <= size_t(c->max_batch), "impulse blanker: the call's frames must lie inside max_batch");
    double* ws = c->blk.d_ws + size_t(io.frame0) * n * 2;
    launch_blanker(c, io.bb, F, io.frame_stride > 0 ? size_t(io.frame_stride) : n, ws, c->blk.d_report + size_t(io.frame0) * 2, s);
    if (input_free) HIPCK(hipEventRecord(input_free, s));      // the blanker is the only reader of the caller's buffer
    SpanIo k = io;
    k.bb = ws;
    k.frame_stride = int(n);
    return k;
}

}  // namespace mgpu_detail

extern "C" {

int mgpu_set_blanker(mgpu_ctx* c, int mode, const mgpu_blanker_params* params, size_t params_size) {
    if (!c) return MGPU_ERR_ARG;
    if (params_size != sizeof(mgpu_blanker_params)) return refuse(c, MGPU_ERR_ARG, "blanker: params_size is not this library's sizeof(mgpu_blanker_params)");
    if (mode != MGPU_BLANK_OFF && mode != MGPU_BLANK_MEDIAN) return refuse(c, MGPU_ERR_ARG, "blanker mode must be MGPU_BLANK_OFF or MGPU_BLANK_MEDIAN");
    Blanker& B = c->blk;
    return guard(c, [&] {
        const mgpu_blanker_params q = params ? *params : mgpu_blanker_params MGPU_BLANKER_PARAMS_DEFAULT;
        if (mode == MGPU_BLANK_MEDIAN) {
            blanker_check(q);
            need(c->tab.Nofdm <= 64 * kBlankOwn, "blanker: the mode's symbol length is outside the kernel's blocks (at most 512 samples)");
        }
        HIPCK(hipStreamSynchronize(c->stream));
        const size_t rows = size_t(c->max_batch > 0 ? c->max_batch : 1);
        if (mode == MGPU_BLANK_MEDIAN) {
            DevArray<double> ws;                               // both made before either is kept: a failure leaves the context as it was
            DevArray<int> rep;
            if (!B.d_ws) ws = DevArray<double>(rows * size_t(c->tab.frame_samples) * 16);
            if (!B.d_report) rep = DevArray<int>(rows * sizeof(mgpu_blanker_report));
            if (!B.d_ws) B.d_ws = std::move(ws);
            if (!B.d_report) B.d_report = std::move(rep);
            HIPCK(hipMemset(B.d_report.p, 0, rows * sizeof(mgpu_blanker_report)));
            B.params = q;
        } else {
            B.d_ws = DevArray<double>();
        }
        B.mode = mode;
    });
}

int mgpu_get_blanker(mgpu_ctx* c, int* mode, mgpu_blanker_params* params, size_t params_size) {
    if (!c || !mode || !params || params_size != sizeof(mgpu_blanker_params)) return MGPU_ERR_ARG;
    *mode = c->blk.mode;
    *params = c->blk.params;
    return MGPU_OK;
}

int mgpu_get_blanker_report(mgpu_ctx* c, int first, int count, mgpu_blanker_report* report) {
    if (!c || first < 0 || count < 0 || (count && !report)) return MGPU_ERR_ARG;
    return guard(c, [&] {
        static_assert(sizeof(mgpu_blanker_report) == 2 * sizeof(int), "a report is two ints");
        read_rows(c, c->blk.d_report, 2, first, count, report, "MGPU_BLANK_MEDIAN was never set on this context");
    });
}

int mgpu_blank_dev(mgpu_ctx* c, const void* d_in, int F, int frame_stride, void* d_out, void* d_report, void* stream) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(d_in && d_out && F >= 0 && frame_stride >= 0, "bad argument");
        if (F == 0) return;
        launch_blanker(c, static_cast<const double*>(d_in), F, frame_stride > 0 ? size_t(frame_stride) : size_t(c->tab.frame_samples),
                       static_cast<double*>(d_out), static_cast<int*>(d_report), static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"

// What the twin needs of a mode's tables (geometry_cache.hpp)
namespace {
struct BlankGeometry { int n = 0, L = 0; };
}  // namespace

extern "C" int mgpu_host_blank(int cfg, const mgpu_explicit_params* p, const mgpu_blanker_params* params, const double* in, double* out,
                               mgpu_blanker_report* report) {
    if (!in || !out) return MGPU_ERR_ARG;
    return host_twin(p, [&](const mgpu::ExplicitParams& xp) -> int {
        const mgpu_blanker_params q = params ? *params : mgpu_blanker_params MGPU_BLANKER_PARAMS_DEFAULT;
        blanker_check(q);
        const auto geometry = cached_geometry<BlankGeometry>(cfg, xp, [](const mgpu::ModeTables& t) { return BlankGeometry{t.frame_samples, t.Nofdm}; });
        const int n = geometry->n, L = geometry->L;
        if (n <= 0 || L <= 0) return MGPU_ERR_ARG;
        const size_t frame = size_t(n), block = size_t(L);
        std::vector<double> pw(frame);
        std::vector<unsigned long long> key(block);
        std::vector<char> exceed(frame, 0);
        for (int i = 0; i < n; ++i) pw[size_t(i)] = in[2 * i] * in[2 * i] + in[2 * i + 1] * in[2 * i + 1];
        for (int base = 0; base < n; base += L) {
            const int m = std::min(L, n - base);
            for (int i = 0; i < m; ++i) {
                std::memcpy(&key[size_t(i)], &pw[size_t(base + i)], 8);
                key[size_t(i)] &= kKeyMask;
            }
            std::nth_element(key.begin(), key.begin() + m / 2, key.begin() + m);
            double med;
            std::memcpy(&med, &key[size_t(m / 2)], 8);
            const double limit = q.threshold * med;
            for (int i = 0; i < m; ++i) exceed[size_t(base + i)] = !(pw[size_t(base + i)] <= limit);
        }
        std::vector<char> mark(frame, 0);
        int marked = 0;
        for (int i = 0; i < n; ++i) {
            if (!exceed[size_t(i)]) continue;
            for (int j = std::max(0, i - q.guard); j <= std::min(n - 1, i + q.guard); ++j) mark[size_t(j)] = 1;
        }
        for (int i = 0; i < n; ++i) marked += mark[size_t(i)];
        const bool blank = marked <= blanker_cap(q, n);
        for (int i = 0; i < n; ++i) {
            const bool z = blank && mark[size_t(i)];
            const double re = in[2 * i], im = in[2 * i + 1];
            out[2 * i] = z ? 0.0 : re;
            out[2 * i + 1] = z ? 0.0 : im;
        }
        if (report) { report->marked = marked; report->blanked = blank ? marked : 0; }
        return MGPU_OK;
    });
}

// The carrier excisor (include/ext/mercury_excisor.h): the three kernels, their launcher for the head of receive_byte (rxloop.hip), the
// context's setting, the stage on its own and the host twin.
#include <algorithm>
#include <cstring>
#include <mutex>

#include "ctx.hpp"
#include "fft256.h"

namespace {
constexpr int kN = 1024, kH = 512, kBand = 64;
constexpr int kSpecRow = 3 * kBand;     // doubles of one block's record in the spectrum workspace: re[64], im[64], P[64]
constexpr unsigned long long kKeyInf = 0x7ff0000000000000ull;      // the smallest key (ctx.hpp kKeyMask) that is no finite power

// The rule's tables, made once per process by the host's libm; the device reads copies of these very values.
struct ExciseTables {
    double tab[kN][2], win[kN];
    ExciseTables() {
        for (int j = 0; j < kN; ++j) {
            const double a = 2.0 * M_PI * double(j) / 1024.0;
            tab[j][0] = std::cos(a);
            tab[j][1] = std::sin(a);
            win[j] = std::sin(M_PI * double(j) / 1024.0);
        }
    }
};
const ExciseTables& excise_tables() {
    static const ExciseTables t;
    return t;
}
int excise_band_lo(double carrier_hz) { return int(std::min(448l, std::max(1l, std::lround(carrier_hz / 46.875) - 32))); }
int excise_blocks(int n) { return (n + kH - 1) / kH + 1; }
}  // namespace

__device__ __forceinline__ int brev10(int p) { return int(__brev(unsigned(p)) >> 22); }
// Entry of position p in the work array: the low four bits (the 16-byte column of a 256-byte LDS row) are turned by p's bits 6..9. In the
// full rounds those bits are the same for every aligned run of 16 lanes (for the whole wavefront in the first two), and such a run reads
// and writes 16 consecutive positions: every row stays a permutation of itself. In the pruned stages lane c reads the row of residue (lo + c) & 63, i.e. row brev6 of it, always at the same four
// columns: bits 6..9 of those positions are the bit-reversed low four bits of the residue, different for any 16 lanes whose numbers differ
// mod 16 - the lane groups of a 16-byte read - where the plain layout has all 64 lanes on one column.
__device__ __forceinline__ int excise_entry(int p) { return (p & ~15) | ((p & 15) ^ ((p >> 6) & 15)); }

// (1) Analysis: one workgroup per (block, window). The transform is the rule's radix-2 network with the data kept in natural order, as
// fft256.h keeps them: element idx of the rule's array a lives at position p = brev10(idx), stage st (size 2^st) pairs positions
// 2^(10 - st) apart, the pair's member with that bit clear is the rule's lo_, and its twiddle index is (brev10(p) & (2^(st-1) - 1)) <<
// (10 - st). Same operands, same operations, same twiddles: the rule's bits. A thread holds four positions and runs two stages between
// LDS exchanges. Stages 1 and 2 pair positions 512 and 256 apart: thread t loads samples t, t + 256, t + 512, t + 768 of the block
// (consecutive lanes, consecutive doubles) and starts in registers, so the block never lies in LDS unwindowed. Stages 3..6 are two more
// rounds. The last four stages are pruned to the band: bin k = lo + c (below 512: lo <= 448) is the rule's chain through the 16 positions
// of row brev6(k & 63), one half-butterfly per stage - lo_ + t where k's bit 6 (7, 8) is clear, lo_ - t where it is set, 15
// multiplications for the bin instead of the 2048 butterflies of the four full stages. Wavefront q forms stage 8's value of every bin
// from the positions whose low two bits are q; after one more exchange wavefront 0 finishes stages 9 and 10 and writes re, im and P.
// Twiddles of stages 2..6 have indices that are multiples of 16: a 32-entry table in LDS, conjugated; those of the pruned stages are
// four per thread, read from the table in memory.
extern "C" __global__ __launch_bounds__(256) void mgpu_excise_analyse_kernel(const double* __restrict__ in, int n, int B, int lo,
                                                                            const double* __restrict__ tab, const double* __restrict__ win,
                                                                            double* __restrict__ spec) {
    __shared__ __attribute__((aligned(16))) c2 a[kN];
    __shared__ __attribute__((aligned(16))) c2 tw16[32];
    __shared__ __attribute__((aligned(16))) c2 s8[4][kBand];
    const int t = threadIdx.x, b = blockIdx.x;
    const size_t w = blockIdx.y;
    const double* const x = in + w * size_t(n);
    const int s = (b - 1) * kH;
    if (t < 32) tw16[t] = {tab[32 * t], -tab[32 * t + 1]};
    auto bfly_w = [](c2& lo_, c2& hi, const c2& wv) {
        const c2 tt = cmul(wv, hi);
        const c2 u = lo_;
        hi = {u.re - tt.re, u.im - tt.im};
        lo_ = {u.re + tt.re, u.im + tt.im};
    };
    auto bfly = [&](c2& lo_, c2& hi, int p0, int st) {          // stages 3..6: the twiddle's index is a multiple of 16
        const int j = brev10(p0) & ((1 << (st - 1)) - 1);
        bfly_w(lo_, hi, fft256_twiddle(tw16, j << (6 - st)));
    };
    c2 r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = t + 256 * k, g = s + i;
        double v = 0.0;
        if (g >= 0 && g < n) v = x[g] * win[i];
        r[k] = {v, 0.0};
    }
    __syncthreads();                                             // tw16
    {   // stages 1, 2: twiddle indices 0, 0, 0 and 256
        const c2 w0 = fft256_twiddle(tw16, 0), w256 = fft256_twiddle(tw16, 16);
        bfly_w(r[0], r[2], w0); bfly_w(r[1], r[3], w0);
        bfly_w(r[0], r[1], w0); bfly_w(r[2], r[3], w256);
#pragma unroll
        for (int k = 0; k < 4; ++k) a[excise_entry(t + 256 * k)] = r[k];
    }
    __syncthreads();
    {   // stages 3, 4: positions pb + 64 k
        const int pb = (t >> 6) * 256 + (t & 63);
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = a[excise_entry(pb + 64 * k)];
        bfly(r[0], r[2], pb, 3); bfly(r[1], r[3], pb + 64, 3);
        bfly(r[0], r[1], pb, 4); bfly(r[2], r[3], pb + 128, 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) a[excise_entry(pb + 64 * k)] = r[k];
    }
    __syncthreads();
    {   // stages 5, 6: positions pc + 16 k
        const int pc = (t >> 4) * 64 + (t & 15);
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = a[excise_entry(pc + 16 * k)];
        bfly(r[0], r[2], pc, 5); bfly(r[1], r[3], pc + 16, 5);
        bfly(r[0], r[1], pc, 6); bfly(r[2], r[3], pc + 32, 6);
#pragma unroll
        for (int k = 0; k < 4; ++k) a[excise_entry(pc + 16 * k)] = r[k];
    }
    __syncthreads();
    // stages 7..10 for bin kb alone. u - tt is u + (-tt) in IEEE arithmetic (signed zeros included): the half-butterfly is one written addition
    // of tt with its sign bit turned where the bin's bit is set.
    const int c = t & 63, q = t >> 6, kb = lo + c, m = kb & 63;
    auto twiddle = [&](int j) { return c2{tab[2 * j], -tab[2 * j + 1]}; };
    auto half = [](const c2& lo_, const c2& hi, const c2& wv, int minus) {
        const c2 tt = cmul(wv, hi);
        const uint32_t sign = minus ? 0x80000000u : 0u;
        auto flip = [&](double v) { return __hiloint2double(int(uint32_t(__double2hiint(v)) ^ sign), __double2loint(v)); };
        return c2{lo_.re + flip(tt.re), lo_.im + flip(tt.im)};
    };
    {
        const int row = 16 * (brev10(m) >> 4);                   // brev6(m) * 16
        const c2 w7 = twiddle(m * 8), w8 = twiddle((kb & 127) * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = a[excise_entry(row + 4 * k + q)];      // positions with bits 3, 2 = k
        const c2 s70 = half(r[0], r[2], w7, kb & 64), s71 = half(r[1], r[3], w7, kb & 64);
        s8[q][c] = half(s70, s71, w8, kb & 128);
    }
    __syncthreads();
    if (t < kBand) {
        const c2 w9 = twiddle((kb & 255) * 2), w10 = twiddle(kb);
        const c2 s90 = half(s8[0][c], s8[2][c], w9, kb & 256), s91 = half(s8[1][c], s8[3][c], w9, kb & 256);
        const c2 X = half(s90, s91, w10, 0);
        double* const rec = spec + (w * size_t(B) + size_t(b)) * kSpecRow;
        rec[c] = X.re;
        rec[kBand + c] = X.im;
        rec[2 * kBand + c] = X.re * X.re + X.im * X.im;
    }
}

// (2) Decision: one wavefront per window, lane k its bin. The median is the blanker's selection, bit by bit from the top of the key with
// one ballot per bit: integer counts, so no order of execution changes it.
extern "C" __global__ __launch_bounds__(64) void mgpu_excise_decide_kernel(const double* __restrict__ spec, int B, int lo, double threshold, int guard,
                                                                          int max_bins, mgpu_excisor_report* __restrict__ report) {
    const int lane = threadIdx.x;
    const size_t w = blockIdx.x;
    const double* const p = spec + w * size_t(B) * kSpecRow + 2 * kBand + lane;
    // The additions are one dependent chain in ascending b, as the rule has them; the loads are not: eight blocks' powers are fetched at a
    // time, so that the chain waits for memory once per eight terms (one load per term, as first written, made this kernel - 64
    // wavefronts per launch, nothing to hide a latency behind - the longest of the three).
    double A = 0.0;
    int b = 0;
    for (; b + 8 <= B; b += 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[size_t(b + j) * kSpecRow];
#pragma unroll
        for (int j = 0; j < 8; ++j) A = A + v[j];
    }
    for (; b < B; ++b) A = A + p[size_t(b) * kSpecRow];
    const unsigned long long key = static_cast<unsigned long long>(__double_as_longlong(A)) & kKeyMask;
    mgpu_excisor_report r;
    memset(&r, 0, sizeof(r));
    r.band_lo = lo;
    if (__ballot(key >= kKeyInf)) {
        r.nonfinite = 1;
    } else {
        bool alive = true;
        int rank = kBand / 2;
        unsigned long long prefix = 0;
        for (int bit = 62; bit >= 0; --bit) {
            const bool set = (key >> bit) & 1ull;
            const int zeros = __popcll(__ballot(alive && !set));
            const bool one = rank >= zeros;                      // uniform: the ballot is the wavefront's
            if (one) { rank -= zeros; prefix |= 1ull << bit; }
            if (set != one) alive = false;
        }
        r.level = __longlong_as_double(static_cast<long long>(prefix));
        const double limit = threshold * r.level;
        r.exceeding = __ballot(!(A <= limit));
        unsigned long long mk = r.exceeding;
        for (int d = 1; d <= guard; ++d) mk |= (r.exceeding << d) | (r.exceeding >> d);
        r.mask = mk;
        const int bits = __popcll(mk);
        r.excised = bits <= max_bins ? bits : 0;
    }
    if (lane == 0) report[w] = r;
}

// (3) Removal: one workgroup per (block pair, window) writes the H samples that blocks p and p + 1 share. A window that passes is copied
// without arithmetic. Otherwise the two blocks' band bins and the table go into LDS, and each thread forms its two samples' sums over the
// masked bins in ascending order. The products k * i are taken mod 1024 as the rule takes them.
extern "C" __global__ __launch_bounds__(256) void mgpu_excise_remove_kernel(const double* __restrict__ in, int n, int B, const double* __restrict__ spec,
                                                                           const mgpu_excisor_report* __restrict__ report,
                                                                           const double* __restrict__ tab, const double* __restrict__ win,
                                                                           double* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) c2 ltab[kN];
    __shared__ __attribute__((aligned(16))) c2 X[2][kBand];
    const int t = threadIdx.x, p = blockIdx.x;
    const size_t w = blockIdx.y;
    const double* const x = in + w * size_t(n);
    double* const y = out + w * size_t(n);
    const int n0 = p * kH, cnt = min(kH, n - n0);
    const unsigned long long mask = report[w].mask;
    const int lo = report[w].band_lo;
    if (report[w].excised == 0) {
        for (int i = t; i < cnt; i += 256) y[n0 + i] = x[n0 + i];
        return;
    }
    for (int j = t; j < kN; j += 256) ltab[j] = {tab[2 * j], tab[2 * j + 1]};
    if (t < 2 * kBand) {
        const int blk = t >> 6, c = t & 63;
        const double* const rec = spec + (w * size_t(B) + size_t(p + blk)) * kSpecRow;
        X[blk][c] = {rec[c], rec[kBand + c]};
    }
    __syncthreads();
    for (int i = t; i < cnt; i += 256) {
        double acc0 = 0.0, acc1 = 0.0;
        for (unsigned long long mk = mask; mk; mk &= mk - 1) {
            const int c = __ffsll(static_cast<long long>(mk)) - 1, k = lo + c;
            const c2 e0 = fft256_twiddle(ltab, (k * (kH + i)) & (kN - 1)), e1 = fft256_twiddle(ltab, (k * i) & (kN - 1));
            const c2 x0 = X[0][c], x1 = X[1][c];
            acc0 = acc0 + (x0.re * e0.re - x0.im * e0.im);
            acc1 = acc1 + (x1.re * e1.re - x1.im * e1.im);
        }
        const double e_b0 = acc0 * win[kH + i] * (1.0 / 512.0), e_b1 = acc1 * win[i] * (1.0 / 512.0);
        y[n0 + i] = x[n0 + i] - (e_b0 + e_b1);
    }
}

namespace mgpu_detail {

// the arguments of a parameter set, or std::invalid_argument
static void excisor_check(const mgpu_excisor_params& q) {
    need(std::isfinite(q.threshold) && q.threshold >= 2.0, "excisor: threshold must be finite and at least 2");
    need(q.guard >= 0 && q.guard <= 4, "excisor: guard must be 0..4 bins");
    need(q.max_bins >= 1 && q.max_bins <= 32, "excisor: max_bins must be 1..32");
}

void launch_excisor(mgpu_ctx* c, const double* d_in, int W, int n, double carrier_hz, double* d_out, mgpu_excisor_report* d_report, hipStream_t s) {
    need(W >= 0 && n >= 1 && n <= (1 << 30), "excisor: a window has 1 .. 2^30 samples");
    need(std::isfinite(carrier_hz) && std::fabs(carrier_hz) <= 1e9, "excisor: carrier_hz must be finite, 1e9 at most in magnitude");
    if (W == 0) return;
    Excisor& E = c->exc;
    const mgpu_excisor_params& q = E.params;
    const int B = excise_blocks(n), lo = excise_band_lo(carrier_hz);
    if (!E.d_tab.p) {
        const ExciseTables& T = excise_tables();
        DevArray<double> tab(sizeof(T.tab)), win(sizeof(T.win));
        HIPCK(hipMemcpy(tab.p, T.tab, sizeof(T.tab), hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(win.p, T.win, sizeof(T.win), hipMemcpyHostToDevice));
        E.d_tab = std::move(tab);
        E.d_win = std::move(win);
    }
    const int chunk = std::min(W, kExciseWindows);
    E.d_spec.grow(size_t(chunk) * size_t(B) * kSpecRow * 8);
    if (!d_report && !E.d_scratch.p) E.d_scratch = DevArray<mgpu_excisor_report>(kExciseWindows * sizeof(mgpu_excisor_report));
    const double *const d_tab = E.d_tab, *const d_win = E.d_win;
    double* const d_spec = E.d_spec;
    for (int off = 0; off < W; off += chunk) {                   // in order on one stream: a launch's spectra are read before the next one's are written
        const int m = std::min(chunk, W - off);
        const double* const in = d_in + size_t(off) * size_t(n);
        mgpu_excisor_report* const rep = d_report ? d_report + off : static_cast<mgpu_excisor_report*>(E.d_scratch);
        hipLaunchKernelGGL(mgpu_excise_analyse_kernel, dim3(B, m), dim3(256), 0, s, in, n, B, lo, d_tab, d_win, d_spec);
        HIPCK(hipGetLastError());
        hipLaunchKernelGGL(mgpu_excise_decide_kernel, dim3(m), dim3(64), 0, s, d_spec, B, lo, q.threshold, q.guard, q.max_bins, rep);
        HIPCK(hipGetLastError());
        hipLaunchKernelGGL(mgpu_excise_remove_kernel, dim3(B - 1, m), dim3(256), 0, s, in, n, B, d_spec, rep, d_tab, d_win,
                           d_out + size_t(off) * size_t(n));
        HIPCK(hipGetLastError());
    }
}

}  // namespace mgpu_detail

extern "C" {

int mgpu_set_excisor(mgpu_ctx* c, int mode, const mgpu_excisor_params* params, size_t params_size) {
    if (!c) return MGPU_ERR_ARG;
    if (params_size != sizeof(mgpu_excisor_params)) return refuse(c, MGPU_ERR_ARG, "excisor: params_size is not this library's sizeof(mgpu_excisor_params)");
    if (mode != MGPU_EXCISE_OFF && mode != MGPU_EXCISE_WELCH) return refuse(c, MGPU_ERR_ARG, "excisor mode must be MGPU_EXCISE_OFF or MGPU_EXCISE_WELCH");
    Excisor& E = c->exc;
    return guard(c, [&] {
        const mgpu_excisor_params q = params ? *params : mgpu_excisor_params MGPU_EXCISOR_PARAMS_DEFAULT;
        if (mode == MGPU_EXCISE_WELCH) excisor_check(q);
        HIPCK(hipStreamSynchronize(c->stream));
        const size_t rows = size_t(c->max_batch > 0 ? c->max_batch : 1);
        if (mode == MGPU_EXCISE_WELCH) {
            if (!E.d_report.p) E.d_report = DevArray<mgpu_excisor_report>(rows * sizeof(mgpu_excisor_report));
            HIPCK(hipMemset(E.d_report.p, 0, rows * sizeof(mgpu_excisor_report)));
            E.params = q;
        } else {
            release_excised_windows(c);
        }
        E.mode = mode;
    });
}

int mgpu_get_excisor(mgpu_ctx* c, int* mode, mgpu_excisor_params* params, size_t params_size) {
    if (!c || !mode || !params || params_size != sizeof(mgpu_excisor_params)) return MGPU_ERR_ARG;
    *mode = c->exc.mode;
    *params = c->exc.params;
    return MGPU_OK;
}

int mgpu_get_excisor_report(mgpu_ctx* c, int first, int count, mgpu_excisor_report* report) {
    if (!c || first < 0 || count < 0 || (count && !report)) return MGPU_ERR_ARG;
    return guard(c, [&] {
        read_rows(c, c->exc.d_report, 1, first, count, report, "MGPU_EXCISE_WELCH was never set on this context");
    });
}

int mgpu_excise_dev(mgpu_ctx* c, const double* d_in, int W, int n, double carrier_hz, double* d_out, void* d_report, void* stream) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(d_in && d_out && W >= 0, "bad argument");
        launch_excisor(c, d_in, W, n, carrier_hz, d_out, static_cast<mgpu_excisor_report*>(d_report), static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"

// ---- the host twin: the rule as the header states it, term by term ----
namespace {
struct h2 { double re, im; };

// the rule's transform of one windowed block, in place in a[1024]
void host_fft1024(h2* a, const ExciseTables& T) {
    for (int size = 2; size <= kN; size *= 2) {
        const int half = size / 2, step = kN / size;
        for (int g = 0; g < kN; g += size)
            for (int j = 0; j < half; ++j) {
                const h2 w = {T.tab[j * step][0], -T.tab[j * step][1]}, lo_ = a[g + j], hi = a[g + j + half];
                const h2 t = {w.re * hi.re - w.im * hi.im, w.re * hi.im + w.im * hi.re};
                a[g + j] = {lo_.re + t.re, lo_.im + t.im};
                a[g + j + half] = {lo_.re - t.re, lo_.im - t.im};
            }
    }
}
int host_brev10(int i) {
    int r = 0;
    for (int b = 0; b < 10; ++b) r |= ((i >> b) & 1) << (9 - b);
    return r;
}
}  // namespace

extern "C" int mgpu_host_excise(const mgpu_excisor_params* params, double carrier_hz, const double* in, int n, double* out, mgpu_excisor_report* report) {
    if (!in || !out || n < 1 || n > (1 << 30) || !std::isfinite(carrier_hz) || std::fabs(carrier_hz) > 1e9) return MGPU_ERR_ARG;
    return host_try([&]() -> int {
        const mgpu_excisor_params q = params ? *params : mgpu_excisor_params MGPU_EXCISOR_PARAMS_DEFAULT;
        excisor_check(q);
        const ExciseTables& T = excise_tables();
        const int B = excise_blocks(n), lo = excise_band_lo(carrier_hz);
        std::vector<h2> X(size_t(B) * kBand), a(kN);
        double A[kBand];
        for (double& v : A) v = 0.0;
        for (int b = 0; b < B; ++b) {
            const long s = long(b - 1) * kH;
            for (int i = 0; i < kN; ++i) {
                const long g = s + i;
                a[size_t(host_brev10(i))] = {g >= 0 && g < n ? in[g] * T.win[i] : 0.0, 0.0};
            }
            host_fft1024(a.data(), T);
            for (int k = 0; k < kBand; ++k) {
                const h2 v = a[size_t(lo + k)];
                X[size_t(b) * kBand + k] = v;
                A[k] = A[k] + (v.re * v.re + v.im * v.im);
            }
        }
        mgpu_excisor_report r;
        std::memset(&r, 0, sizeof(r));
        r.band_lo = lo;
        unsigned long long key[kBand];
        bool finite = true;
        for (int k = 0; k < kBand; ++k) {
            std::memcpy(&key[k], &A[k], 8);
            key[k] &= kKeyMask;
            if (key[k] >= kKeyInf) finite = false;
        }
        if (!finite) {
            r.nonfinite = 1;
        } else {
            std::nth_element(key, key + kBand / 2, key + kBand);
            std::memcpy(&r.level, &key[kBand / 2], 8);
            const double limit = q.threshold * r.level;
            for (int k = 0; k < kBand; ++k) if (!(A[k] <= limit)) r.exceeding |= 1ull << k;
            r.mask = r.exceeding;
            for (int d = 1; d <= q.guard; ++d) r.mask |= (r.exceeding << d) | (r.exceeding >> d);
            const int bits = __builtin_popcountll(r.mask);
            r.excised = bits <= q.max_bins ? bits : 0;
        }
        if (report) *report = r;
        if (r.excised == 0) {
            if (out != in) std::memmove(out, in, size_t(n) * 8);
            return MGPU_OK;
        }
        // e_b[i] of every block, then the samples: block b0 = n / 512 at 512 + n % 512, block b0 + 1 at n % 512
        std::vector<double> e(size_t(B) * kN);
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < kN; ++i) {
                double acc = 0.0;
                for (int c = 0; c < kBand; ++c) {
                    if (!((r.mask >> c) & 1ull)) continue;
                    const int k = lo + c, qi = (k * i) & (kN - 1);
                    const h2 v = X[size_t(b) * kBand + c];
                    acc = acc + (v.re * T.tab[qi][0] - v.im * T.tab[qi][1]);
                }
                e[size_t(b) * kN + i] = acc * T.win[i] * (1.0 / 512.0);
            }
        for (int i = 0; i < n; ++i) {
            const int b0 = i / kH, r0 = i % kH;
            out[i] = in[i] - (e[size_t(b0) * kN + kH + r0] + e[size_t(b0 + 1) * kN + r0]);
        }
        return MGPU_OK;
    });
}

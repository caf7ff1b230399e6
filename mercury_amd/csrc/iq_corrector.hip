// IQ corrector (include/ext/mercury_iq_corrector.h): one IQ stream at 48000 * D out again in its own format, with no delay, less its DC
// offset and with Q made orthogonal to I and given I's power.
//
// Per call of m blocks, on one stream:
//   1. mgpu_iqc_sums_kernel, one workgroup of four wavefronts per block: thread l owns partial l of the five terms (B / 256 <= 16 samples,
//      one 4-, 8- or 16-byte load per sample, widened in the load). The fold's steps s = 128 and 64 go through LDS, the rest runs in the
//      first wavefront over cross-lane moves: plain adds in the rule's order, no atomics.
//   2. mgpu_iqc_scan_kernel, one workgroup, in rounds of 256 blocks: thread j brings block j's sums into LDS, lanes 0..5 of the first
//      wavefront carry the six state values over the round in ascending order, then thread j turns the state after block j into the
//      block's estimate (iqc_rule.hpp estimate(): the divisions and the square root
//      are the device's correctly rounded ones). The final state stays on the device for the next call.
//   3. mgpu_iqc_apply_kernel, one workgroup per block: the block's estimate is uniform (scalar loads), the samples are read a second
//      time, corrected and narrowed in the store; the clamped components are counted over ballots and the report is written.
// In fixed mode only the third runs, with the configured values.
#include <cstring>

#include "iqc_rule.hpp"
#include "stream_stage.hpp"

using namespace mgpu_iqc_detail;

namespace {

constexpr int kThreads = 256;                     // the sums' and the apply kernel's workgroup: four wavefronts; one thread per partial
constexpr int kScanBlocks = 256;                  // the scan's round, and its workgroup: one block per thread
constexpr int kScanUnroll = 8;                    // blocks whose sums the scan holds in registers at a time
static_assert(kScanBlocks % 64 == 0 && 64 % kScanUnroll == 0, "a group of the scan never leaves S nor a word of the mask");
static_assert(kThreads == kPartials, "thread l owns partial l");

struct BlockEstimate {                            // what the scan leaves of a block for the apply kernel
    double dc_re, dc_im, skew, gain;
    int flags, pad;
};

struct ApplyArgs {
    const void* iq;                               // the call's m * B samples
    void* out;                                    // [m * B]
    const BlockEstimate* est;                     // [m]; null: fixed mode
    mgpu_iqc_report* reports;                     // [m]; null: not wanted
    BlockEstimate fixed;                          // fixed mode's values
    long long first_block;                        // the block the call's first report describes
    int format, B;
};

}  // namespace

// grid: the call's blocks. sums [m][5]
extern "C" __global__ __launch_bounds__(kThreads) void mgpu_iqc_sums_kernel(const void* __restrict__ iq, double* __restrict__ sums, int format,
                                                                            int B) {
    __shared__ double fold[kTerms][kThreads];
    const int t = threadIdx.x;
    const size_t first = size_t(blockIdx.x) * size_t(B);
    double p[kTerms];
    {
        const double2 v = mgpu_fmt::load_iq(iq, format, first + size_t(t));      // B >= 256: every thread has a first term
        const double I = v.x, Q = v.y;
        p[0] = I, p[1] = Q, p[2] = I * I, p[3] = I * Q, p[4] = Q * Q;
    }
    for (int f = t + kThreads; f < B; f += kThreads) {
        const double2 v = mgpu_fmt::load_iq(iq, format, first + size_t(f));
        const double I = v.x, Q = v.y;
        p[0] += I, p[1] += Q, p[2] += I * I, p[3] += I * Q, p[4] += Q * Q;
    }
#pragma unroll
    for (int k = 0; k < kTerms; ++k) fold[k][t] = p[k];
    __syncthreads();
    if (t < 128) {
#pragma unroll
        for (int k = 0; k < kTerms; ++k) {
            p[k] += fold[k][t + 128];
            if (t >= 64) fold[k][t] = p[k];
        }
    }
    __syncthreads();
    if (t >= 64) return;                                             // the first wavefront goes on alone
#pragma unroll
    for (int k = 0; k < kTerms; ++k) {
        p[k] += fold[k][t + 64];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) p[k] += __shfl_down(p[k], s);          // lane l < s adds lane l + s; the lanes above are not read again
    }
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < kTerms; ++k) sums[size_t(blockIdx.x) * kTerms + k] = p[k];
    }
}

// one workgroup of four wavefronts. sums [m][5] -> est [m]; state [6] read (fresh: zeros instead) and written
extern "C" __global__ __launch_bounds__(kScanBlocks) void mgpu_iqc_scan_kernel(const double* __restrict__ sums, BlockEstimate* __restrict__ est,
                                                                               double* state, int m, int fresh, double lambda, double B, int dc,
                                                                               int balance) {
    __shared__ double S[kScanBlocks][6];                             // a block's five sums and B; then, in place, the state after the block
    __shared__ unsigned long long skipped[kScanBlocks / 64];         // bit j & 63 of word j >> 6: block j of the round is skipped
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double mine = (fresh || t >= 6) ? 0.0 : state[t];
    for (int b0 = 0; b0 < m; b0 += kScanBlocks) {
        const int nb = min(kScanBlocks, m - b0);
        bool bad = false;
        if (t < nb) {
#pragma unroll
            for (int k = 0; k < kTerms; ++k) {
                const double s = sums[size_t(b0 + t) * kTerms + k];
                S[t][k] = s;
                bad = bad || !is_finite(s);
            }
            S[t][kTerms] = B;
        }
        const unsigned long long word = __ballot(bad);
        if (lane == 0) skipped[wave] = word;
        __syncthreads();
        if (t < 6) {
            // eight blocks' sums at a time into registers, so that only the multiply and the add are on the dependent path; a block that
            // is skipped, or lies past the call's last (its row of S is whatever LDS held), is a select and moves nothing
            for (int j0 = 0; j0 < nb; j0 += kScanUnroll) {
                const unsigned long long skip = skipped[j0 >> 6] >> (j0 & 63);      // kScanUnroll divides 64: the group lies in one word
                double s[kScanUnroll];
#pragma unroll
                for (int u = 0; u < kScanUnroll; ++u) s[u] = S[j0 + u][t];
#pragma unroll
                for (int u = 0; u < kScanUnroll; ++u) {
                    const bool take = j0 + u < nb && !((skip >> u) & 1ull);
                    const double decayed = lambda * mine;
                    const double next = decayed + s[u];
                    mine = take ? next : mine;
                    S[j0 + u][t] = mine;
                }
            }
        }
        __syncthreads();
        if (t < nb) {
            const Estimate e = estimate(S[t][0], S[t][1], S[t][2], S[t][3], S[t][4], S[t][5], dc, balance);
            BlockEstimate o;
            o.dc_re = e.dc_re, o.dc_im = e.dc_im, o.skew = e.skew, o.gain = e.gain;
            o.flags = e.flags | (((skipped[wave] >> lane) & 1ull) ? MGPU_IQC_SKIPPED : 0);
            o.pad = 0;
            est[b0 + t] = o;
        }
        __syncthreads();                                             // the next round writes S and the mask again
    }
    if (t < 6) state[t] = mine;
}

// grid: the call's blocks
extern "C" __global__ __launch_bounds__(kThreads) void mgpu_iqc_apply_kernel(ApplyArgs a) {
    __shared__ int clamped[kThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, B = a.B;
    const BlockEstimate be = a.est ? a.est[blockIdx.x] : a.fixed;    // uniform
    const Estimate e{be.dc_re, be.dc_im, be.skew, be.gain, be.flags};
    const size_t first = size_t(blockIdx.x) * size_t(B);
    int mine = 0;
    for (int f = t; f < B; f += kThreads) {                          // B is a multiple of 256: no lane is idle in a ballot
        const double2 v = mgpu_fmt::load_iq(a.iq, a.format, first + size_t(f));
        double yI, yQ;
        correct(e, v.x, v.y, &yI, &yQ);
        const unsigned c = mgpu_fmt::store_iq(a.out, a.format, first + size_t(f), yI, yQ);
        mine += __popcll(__ballot(c >= 1)) + __popcll(__ballot(c == 2));
    }
    if (!a.reports) return;
    if (lane == 0) clamped[wave] = mine;
    __syncthreads();
    if (t == 0) {
        mgpu_iqc_report r;
        r.block = a.first_block + (long long)blockIdx.x;
        r.dc_re = be.dc_re, r.dc_im = be.dc_im, r.skew = be.skew, r.gain = be.gain;
        r.flags = be.flags;
        r.clamped = clamped[0] + clamped[1] + clamped[2] + clamped[3];
        a.reports[blockIdx.x] = r;
    }
}

struct mgpu_iqc : BlockStage<mgpu_iqc_report> {
    mgpu_iqc_config cfg{};
    double lambda = 1.0;
    bool fresh = true;                            // the state is zero: d_state is not read
    DevArray<double> d_state;                     // [6]
    DevArray<double> d_sums;                      // [max_blocks][5]
    DevArray<BlockEstimate> d_est;                // [max_blocks]

    // one call on device memory: m = n_in / B blocks into d_o [n_in] and d_r [m] (null: no reports)
    void run(const void* d_iq, int m, void* d_o, mgpu_iqc_report* d_r, hipStream_t st) {
        ApplyArgs ap{};
        ap.iq = d_iq; ap.out = d_o; ap.reports = d_r; ap.first_block = (long long)(pos / uint64_t(B)); ap.format = cfg.format; ap.B = B;
        if (cfg.fixed) {
            const Estimate e = fixed_estimate(cfg);
            ap.fixed = BlockEstimate{e.dc_re, e.dc_im, e.skew, e.gain, 0, 0};
        } else {
            hipLaunchKernelGGL(mgpu_iqc_sums_kernel, dim3(unsigned(m)), dim3(kThreads), 0, st, d_iq, (double*)d_sums, cfg.format, B);
            HIPCK(hipGetLastError());
            hipLaunchKernelGGL(mgpu_iqc_scan_kernel, dim3(1), dim3(kScanBlocks), 0, st, (const double*)d_sums, (BlockEstimate*)d_est, (double*)d_state, m,
                               fresh ? 1 : 0, lambda, double(B), cfg.dc, cfg.balance);
            HIPCK(hipGetLastError());
            ap.est = d_est;
            fresh = false;
        }
        hipLaunchKernelGGL(mgpu_iqc_apply_kernel, dim3(unsigned(m)), dim3(kThreads), 0, st, ap);
        HIPCK(hipGetLastError());
        pos += uint64_t(m) * uint64_t(B);
    }
};

extern "C" {

int mgpu_iqc_create(mgpu_ctx* c, const mgpu_iqc_config* kc, mgpu_iqc** out) {
    return create_stage(c, out, "mgpu_iqc_create", config_error(kc), [&](mgpu_iqc* k) {
        k->cfg = *kc;
        block_shape(k, block_of(*kc), kDefaultBlocksIn);
        k->lambda = lambda_of(*kc);
        k->d_state = DevArray<double>(6 * sizeof(double));
        k->d_sums = DevArray<double>(size_t(k->max_blocks) * kTerms * sizeof(double));
        k->d_est = DevArray<BlockEstimate>(size_t(k->max_blocks) * sizeof(BlockEstimate));
    });
}

int mgpu_iqc_destroy(mgpu_iqc* k) { return destroy_stage(k); }

int mgpu_iqc_seek(mgpu_iqc* k, uint64_t position) {
    return block_seek(k, position, [&] { k->fresh = true; });
}

int mgpu_iqc_status(mgpu_iqc* k, mgpu_iqc_state* state) {
    if (!k || !state) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        mgpu_iqc_state s{};
        s.position = k->pos;
        s.blocks = k->pos / uint64_t(k->B);
        s.D = k->cfg.D; s.block = k->B; s.max_in = k->max_in; s.format = k->cfg.format;
        s.lambda = k->lambda;
        if (!k->fresh) {
            HIPCK(hipDeviceSynchronize());        // process_dev may have run on a caller's stream
            HIPCK(hipMemcpy(s.T, k->d_state.p, sizeof(s.T), hipMemcpyDeviceToHost));
        }
        const Estimate e = k->cfg.fixed ? fixed_estimate(k->cfg) : estimate(s.T[0], s.T[1], s.T[2], s.T[3], s.T[4], s.T[5], k->cfg.dc, k->cfg.balance);
        s.dc_re = e.dc_re, s.dc_im = e.dc_im, s.skew = e.skew, s.gain = e.gain, s.flags = e.flags;
        *state = s;
    });
}

int mgpu_iqc_process_dev(mgpu_iqc* k, const void* d_iq, int n_in, void* d_out, mgpu_iqc_report* d_reports, int* n_reports, void* stream) {
    return block_process_dev(k, d_iq, n_in, d_out, d_reports, n_reports, stream);
}

int mgpu_iqc_process(mgpu_iqc* k, const void* iq, int n_in, void* out, mgpu_iqc_report* reports, int* n_reports) {
    return block_process(k, iq, n_in, out, reports, n_reports);
}

int mgpu_host_iqc_process(const mgpu_iqc_config* kc, const void* iq, int n_in, uint64_t position, void* out, mgpu_iqc_report* reports,
                          int* n_reports) {
    return host_try([&] { return host_process(kc, nullptr, iq, n_in, position, out, reports, n_reports); });
}

int mgpu_host_iqc_continue(const mgpu_iqc_config* kc, double* state, const void* iq, int n_in, uint64_t position, void* out,
                           mgpu_iqc_report* reports, int* n_reports) {
    if (!state) return MGPU_ERR_ARG;
    return host_try([&] { return host_process(kc, state, iq, n_in, position, out, reports, n_reports); });
}

}  // extern "C"

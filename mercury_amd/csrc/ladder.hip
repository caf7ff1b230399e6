// The estimator ladder (include/mercury_estimator.h): the two small kernels around a retry, the host loop over the rungs, the setters and
// the host twin of the LS estimate. The retry itself is the rectangular front-end (frontend.hip; launched by launch.hip's front-end core)
// on a frame list and the unchanged decoder on compact buffers.
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>

#include "ctx.hpp"

// Frames with message_decoded == 0 as an ascending index list plus their number. One workgroup walks the stats 1024 frames at a time: a
// wavefront's failing lanes by ballot, a lane's place among them by the population of the lanes below it, the wavefronts' totals through
// LDS; the list comes out in frame order whatever the timing. first != 0 (the pass behind rung 0): every frame's rung starts as 0 or -1 and
// the counters take rung 0's share.
extern "C" __global__ __launch_bounds__(1024) void mgpu_ladder_select_kernel(const MgpuStatsDev* __restrict__ stats, int F, int first, int* __restrict__ rung,
                                                                            int* __restrict__ idx, int* __restrict__ count,
                                                                            unsigned long long* __restrict__ counters) {
    __shared__ int wave_total[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int f0 = 0; f0 < F; f0 += 1024) {
        const int f = f0 + tid;
        const bool failed = f < F && stats[f].message_decoded == 0;
        if (first && f < F) rung[f] = failed ? -1 : 0;
        const unsigned long long m = __ballot(failed);
        const int below = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const int n = wave_total[w]; before += w < wave ? n : 0; total += n; }
        if (failed && idx) idx[base + before + below] = f;
        base += total;
        __syncthreads();
    }
    if (tid == 0) {
        if (count) *count = base;
        if (first) { atomicAdd(counters, (unsigned long long)(F - base)); atomicAdd(counters + MGPU_LADDER_MAX, (unsigned long long)F); }
    }
}

// Row b of the compact results belongs to frame idx[b]: where the retry decoded it, its whole record replaces the frame's (LLRs, variance,
// SNR variance, mean_H where kept, payload, stats), the frame's rung becomes r and rung r's counter goes up. One workgroup per row.
extern "C" __global__ __launch_bounds__(256) void mgpu_ladder_merge_kernel(const int* __restrict__ idx, int n, int r, int N, int payload_stride,
                                                                          const float* __restrict__ c_llr, const float* __restrict__ c_var,
                                                                          const float* __restrict__ c_snrvar, const double* __restrict__ c_meanh,
                                                                          const uint8_t* __restrict__ c_payload, const MgpuStatsDev* __restrict__ c_stats,
                                                                          float* __restrict__ llr, float* __restrict__ var, float* __restrict__ snrvar,
                                                                          double* __restrict__ meanh, uint8_t* __restrict__ payload,
                                                                          MgpuStatsDev* __restrict__ stats, int* __restrict__ rung,
                                                                          unsigned long long* __restrict__ counters) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= n) return;
    const MgpuStatsDev st = c_stats[b];
    if (!st.message_decoded) return;
    const size_t f = size_t(idx[b]);
    for (int i = tid; i < N; i += 256) llr[f * N + i] = c_llr[size_t(b) * N + i];
    for (int i = tid; i < payload_stride; i += 256) payload[f * payload_stride + i] = c_payload[size_t(b) * payload_stride + i];
    if (tid == 0) {
        stats[f] = st;
        var[f] = c_var[b];
        if (snrvar) snrvar[f] = c_snrvar[b];
        if (meanh) meanh[f] = c_meanh[b];
        rung[f] = r;
        atomicAdd(counters + r, 1ull);
    }
}

namespace mgpu_detail {

void launch_ladder(mgpu_ctx* c, const SpanIo& io, int F, hipStream_t s) {
    Ladder& L = c->lad;
    if (L.n == 0 || F <= 0) return;
    const auto& t = c->tab;
    need(io.payload && io.stats && size_t(io.frame0) + size_t(F) <= size_t(c->max_batch), "estimator ladder: the call needs payload and stats arrays of at most max_batch frames");
    int* rung = L.d_rung + io.frame0;
    L.last_F = io.frame0 + F;
    // a retry's workspaces are the context's: one retry at a time, whatever streams the calls come on
    if (L.done_recorded) HIPCK(hipStreamWaitEvent(s, L.done, 0));
    SpanIo k = io;           // the same frames into the compact workspaces, row b = frame d_idx[b]
    k.llr = L.d_llr; k.var = L.d_var; k.snrvar = L.d_snrvar; k.payload = L.d_payload; k.stats = L.d_stats;
    k.mean_H = io.mean_H ? static_cast<double*>(L.d_meanh) : nullptr;
    for (int r = 1; r == 1 || r < L.n; ++r) {
        const bool retry = r < L.n;      // a one-rung ladder still marks the frames and counts them
        hipLaunchKernelGGL(mgpu_ladder_select_kernel, dim3(1), dim3(1024), 0, s, io.stats, F, r == 1 ? 1 : 0, rung, retry ? static_cast<int*>(L.d_idx) : nullptr,
                           retry ? static_cast<int*>(L.d_count) : nullptr, static_cast<unsigned long long*>(L.d_counters));
        HIPCK(hipGetLastError());
        if (!retry) break;
        int n = 0;       // the decoder's launch size: the one value per rung the host has to see
        HIPCK(hipMemcpyAsync(&n, L.d_count, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
        if (n == 0) break;
        MgpuLsRect w = L.win[r];
        w.frames = L.d_idx;
        // untimed: the kernel timings describe rung 0
        frontend_untimed(c, k, n, MgpuTapsDev{}, &w, s);
        decoder_untimed(c, k.llr, n, nullptr, nullptr, k.payload, k.stats, k.var, k.snrvar, s);
        for_frame_chunks(n, [&](int off, int m) {
            hipLaunchKernelGGL(mgpu_ladder_merge_kernel, dim3(m), dim3(256), 0, s, L.d_idx + off, m, r, t.N, t.payload_stride, k.llr + size_t(off) * t.N,
                               k.var + off, k.snrvar + off, at(k.mean_H, off), k.payload + size_t(off) * t.payload_stride,
                               k.stats + off, io.llr, io.var, io.snrvar, io.mean_H, io.payload, io.stats, rung,
                               static_cast<unsigned long long*>(L.d_counters));
            HIPCK(hipGetLastError());
        });
    }
    HIPCK(hipEventRecord(L.done, s));
    L.done_recorded = true;
}

// a window side as it is applied: 1..21, an even value incremented (telecom_system.cc:2802-2809); 0 = refused
static int window_side(int v) {
    if (v < 1 || v > 21) return 0;
    return v % 2 == 0 ? v + 1 : v;
}

}  // namespace mgpu_detail

extern "C" {

int mgpu_set_estimator_ladder(mgpu_ctx* c, const mgpu_ls_window* rungs, int n_rungs) {
    if (!c) return MGPU_ERR_ARG;
    const auto& t = c->tab;
    if (n_rungs == 0 && c->lad.n == 0) return MGPU_OK;      // nothing set, nothing to clear: fine on every mode
    if (t.mfsk_M > 0 || t.estimator != MGPU_EST_LS) {
        c->err = "an estimator ladder needs an OFDM mode with the LS estimator (the zero-forcing and MFSK modes have no window)";
        return MGPU_ERR_UNSUPPORTED;
    }
    return guard(c, [&] {
        need(n_rungs >= 0 && n_rungs <= MGPU_LADDER_MAX && (rungs || n_rungs == 0), "estimator ladder: 0..MGPU_LADDER_MAX rungs");
        mgpu_ls_window win[MGPU_LADDER_MAX]{};
        for (int r = 0; r < n_rungs; ++r) {
            win[r].width = window_side(rungs[r].width);
            win[r].height = window_side(rungs[r].height);
            need(win[r].width && win[r].height, "estimator ladder: a window is 1..21 cells wide (the front-end reads at most 7 pilots of a window row) and 1..21 high");
        }
        // everything that can fail comes before the context changes
        DevArray<double> weight[MGPU_LADDER_MAX];
        for (int r = 0; r < n_rungs; ++r) weight[r] = upload(mgpu::ls_weight_table(t.pilot_boost, win[r].width * win[r].height));
        const size_t B = size_t(c->max_batch);
        Ladder& L = c->lad;
        HIPCK(hipStreamSynchronize(c->stream));
        if (L.done_recorded) HIPCK(hipEventSynchronize(L.done));
        if (n_rungs > 0) {
            if (!L.done) HIPCK(hipEventCreateWithFlags(&L.done.h, hipEventDisableTiming));
            L.d_rung.grow(B * sizeof(int));
            L.d_counters.grow((MGPU_LADDER_MAX + 1) * sizeof(unsigned long long));
            HIPCK(hipFuncSetAttribute(reinterpret_cast<const void*>(fe_rect_kernel(c->fe_threads)), hipFuncAttributeMaxDynamicSharedMemorySize, int(c->lds_fe)));
        }
        if (n_rungs > 1) {
            L.d_idx.grow(B * sizeof(int)); L.d_count.grow(sizeof(int));
            L.d_llr.grow(B * t.N * sizeof(float)); L.d_var.grow(B * sizeof(float)); L.d_snrvar.grow(B * sizeof(float));
            L.d_meanh.grow(B * sizeof(double));
            L.d_payload.grow(B * t.payload_stride); L.d_stats.grow(B * sizeof(MgpuStatsDev));
        }
        if (n_rungs > 0) HIPCK(hipMemset(L.d_counters, 0, (MGPU_LADDER_MAX + 1) * sizeof(unsigned long long)));
        for (int r = 0; r < MGPU_LADDER_MAX; ++r) {
            L.rung[r] = r < n_rungs ? win[r] : mgpu_ls_window{0, 0};
            L.weight[r] = r < n_rungs ? std::move(weight[r]) : DevArray<double>();
            L.win[r] = MgpuLsRect{};
            if (r >= n_rungs) continue;
            const int hw_f = win[r].width / 2;
            L.win[r].weight = L.weight[r];
            L.win[r].hw_f = hw_f; L.win[r].hw_t = win[r].height / 2;
            // as create.hip does for the square window: 2 when every (clipped) window row holds >= 3 pilots of each column residue
            L.win[r].lattice = c->dev.regular_lattice ? (std::min(hw_f + 1, t.Nc) >= 9 ? 2 : 1) : 0;
        }
        L.rung0_is_default = n_rungs > 0 && win[0].width == t.lsw && win[0].height == t.lsw;
        L.n = n_rungs;
        L.last_F = 0;
    });
}

int mgpu_get_estimator_ladder(mgpu_ctx* c, mgpu_ls_window* rungs, int* n_rungs) {
    if (!c || !n_rungs || !rungs) return MGPU_ERR_ARG;
    *n_rungs = c->lad.n;
    for (int r = 0; r < c->lad.n; ++r) rungs[r] = c->lad.rung[r];
    return MGPU_OK;
}

int mgpu_estimator_rungs_last(mgpu_ctx* c, int* rung, int F) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(rung && c->lad.n > 0 && F >= 0 && F <= c->lad.last_F, "no ladder set, or more frames asked for than the last call had");
        HIPCK(hipStreamSynchronize(c->stream));
        if (c->lad.done_recorded) HIPCK(hipEventSynchronize(c->lad.done));
        if (F) HIPCK(hipMemcpy(rung, c->lad.d_rung, size_t(F) * sizeof(int), hipMemcpyDeviceToHost));
    });
}

int mgpu_estimator_ladder_counters(mgpu_ctx* c, long long decoded_by_rung[MGPU_LADDER_MAX], long long* frames, int reset) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(c->lad.n > 0, "no ladder set");
        HIPCK(hipStreamSynchronize(c->stream));
        if (c->lad.done_recorded) HIPCK(hipEventSynchronize(c->lad.done));
        unsigned long long v[MGPU_LADDER_MAX + 1];
        HIPCK(hipMemcpy(v, c->lad.d_counters, sizeof(v), hipMemcpyDeviceToHost));
        if (decoded_by_rung) for (int r = 0; r < MGPU_LADDER_MAX; ++r) decoded_by_rung[r] = (long long)v[r];
        if (frames) *frames = (long long)v[MGPU_LADDER_MAX];
        if (reset) HIPCK(hipMemset(c->lad.d_counters, 0, sizeof(v)));
    });
}

// The front-end's general path (frontend.hip: the reference's own walk over the window's cells, ofdm.cc:1315-1451) on the host. What it needs
// of the mode's tables is kept for the last geometry asked for: a sweep over windows and frames builds the tables once.
namespace {
struct TwinGeometry {
    int cfg = -1;
    mgpu::ExplicitParams xp;
    bool ls = false;                    // an OFDM mode with the LS estimator
    int Nc = 0, Nsymb = 0;
    double pilot_boost = 0;
    std::vector<uint8_t> cell_type;
    std::vector<double> pilot_val;
};
std::mutex twin_mutex;
std::shared_ptr<const TwinGeometry> twin_last;

std::shared_ptr<const TwinGeometry> twin_geometry(int cfg, const mgpu::ExplicitParams& xp) {
    std::lock_guard<std::mutex> lock(twin_mutex);
    const auto same = [&](const TwinGeometry& g) {
        return g.cfg == cfg && g.xp.pilot_boost == xp.pilot_boost && g.xp.ls_window == xp.ls_window && g.xp.pilot_seed == xp.pilot_seed &&
               g.xp.scrambler_seed == xp.scrambler_seed && g.xp.preamble_seed == xp.preamble_seed && g.xp.Nsymb == xp.Nsymb && g.xp.Dy == xp.Dy;
    };
    if (twin_last && same(*twin_last)) return twin_last;
    const mgpu::ModeTables t = mgpu::build_mode_tables(cfg, 0, mgpu_ldpc_blob, mgpu_ldpc_blob_size, xp);
    auto g = std::make_shared<TwinGeometry>();
    g->cfg = cfg; g->xp = xp;
    g->ls = t.mfsk_M == 0 && t.estimator == MGPU_EST_LS;
    g->Nc = t.Nc; g->Nsymb = t.Nsymb; g->pilot_boost = t.pilot_boost;
    g->cell_type = t.cell_type; g->pilot_val = t.pilot_val;
    twin_last = g;
    return g;
}
}  // namespace

int mgpu_host_ls_estimate(int cfg, const mgpu_explicit_params* p, int width, int height, const double* grid, double* H) {
    if (!grid || !H) return MGPU_ERR_ARG;
    const int wf = window_side(width), wt = window_side(height);
    if (!wf || !wt) return MGPU_ERR_ARG;
    mgpu::ExplicitParams xp;
    std::string err;
    int rc = MGPU_OK;
    if (!explicit_params_from(p, xp, err, &rc)) return rc;
    xp.ls_window = mgpu::ExplicitParams().ls_window;
    try {
        const std::shared_ptr<const TwinGeometry> geometry = twin_geometry(cfg, xp);
        const TwinGeometry& t = *geometry;
        if (!t.ls) return MGPU_ERR_UNSUPPORTED;
        const std::vector<double> weight = mgpu::ls_weight_table(t.pilot_boost, wf * wt);
        const int Nc = t.Nc, Ns = t.Nsymb, hf = wf / 2, ht = wt / 2;
        int pilot = 0;
        for (int c = 0; c < Ns * Nc; ++c) {
            if (!t.cell_type[c]) continue;
            const int i = c / Nc, j = c - i * Nc;
            const int k0 = std::max(i - ht, 0), k1 = std::min(i + ht, Ns - 1), l0 = std::max(j - hf, 0), l1 = std::min(j + hf, Nc - 1);
            int n = 0;
            for (int k = k0; k <= k1; ++k)
                for (int l = l0; l <= l1; ++l) n += t.cell_type[k * Nc + l] != 0;
            const double w = weight[n];
            double hr = 0, hi = 0;
            for (int k = k0; k <= k1; ++k)
                for (int l = l0; l <= l1; ++l) {
                    const int q = k * Nc + l;
                    if (!t.cell_type[q]) continue;
                    const double xw = t.pilot_val[q] < 0 ? -w : w;
                    hr += xw * grid[2 * q];
                    hi += xw * grid[2 * q + 1];
                }
            H[2 * pilot] = hr; H[2 * pilot + 1] = hi;
            ++pilot;
        }
        return MGPU_OK;
    } catch (const std::exception&) { return MGPU_ERR_ARG; }
}

}  // extern "C"

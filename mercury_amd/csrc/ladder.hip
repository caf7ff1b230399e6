// The estimator ladder (include/mercury_estimator.h): the two small kernels around a retry, the host loop over the rungs, the setters and
// the host twins of the LS and of the Wiener estimate. The retry itself is the rectangular front-end (frontend.hip; launched by launch.hip's front-end core)
// on a frame list and the unchanged decoder on compact buffers.
#include <algorithm>
#include <cmath>
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
        frontend_untimed(c, k, n, MgpuTapsDev{}, &w, s, r);
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

// The front-end's general path (frontend.hip: the reference's own walk over the window's cells, ofdm.cc:1315-1451) on the host. What it needs
// of the mode's tables is kept for the last geometry asked for (geometry_cache.hpp): a sweep over windows and frames builds the tables once.
namespace {
struct TwinGeometry {
    bool ls = false;                    // an OFDM mode with the LS estimator
    int Nc = 0, Nsymb = 0;
    double pilot_boost = 0;
    std::vector<uint8_t> cell_type;
    std::vector<double> pilot_val;
};

// fn(the mode's geometry) as a host twin (ctx.hpp host_twin); MGPU_ERR_UNSUPPORTED where the mode has no LS window. The twins of this file
// do not read ls_window: it is put back to its default, so that a sweep over it keeps the geometry.
template <typename Fn> int ls_twin(int cfg, const mgpu_explicit_params* p, Fn&& fn) {
    return host_twin(p, [&](mgpu::ExplicitParams xp) -> int {
        xp.ls_window = mgpu::ExplicitParams().ls_window;
        const auto geometry = cached_geometry<TwinGeometry>(cfg, xp, [](const mgpu::ModeTables& t) {
            return TwinGeometry{t.mfsk_M == 0 && t.estimator == MGPU_EST_LS, t.Nc, t.Nsymb, t.pilot_boost, t.cell_type, t.pilot_val};
        });
        if (!geometry->ls) return MGPU_ERR_UNSUPPORTED;
        return fn(geometry);
    });
}
}  // namespace

namespace {
// the tables of the last (geometry, design) asked for: a sweep over frames builds them once
struct TwinWiener {
    std::shared_ptr<const TwinGeometry> geometry;
    mgpu_wiener_design design{};
    mgpu::WienerTables tables;
};
std::mutex wiener_mutex;
std::shared_ptr<const TwinWiener> wiener_last;

// fn(the mode's geometry, the design's tables) as ls_twin; MGPU_ERR_ARG where the design is refused
template <typename Fn> int wiener_twin(int cfg, const mgpu_explicit_params* p, const mgpu_wiener_design* d_or_null, Fn&& fn) {
    const mgpu_wiener_design d = d_or_null ? *d_or_null : mgpu_wiener_design MGPU_WIENER_DESIGN_DEFAULT;
    const mgpu::WienerDesign design{d.tau_min_us, d.tau_max_us, d.doppler_hz, d.snr_db};
    if (!mgpu::wiener_design_ok(design)) return MGPU_ERR_ARG;
    return ls_twin(cfg, p, [&](const std::shared_ptr<const TwinGeometry>& geometry) -> int {
        std::shared_ptr<const TwinWiener> twin;
        {
            std::lock_guard<std::mutex> lock(wiener_mutex);
            if (!wiener_last || wiener_last->geometry != geometry || std::memcmp(&wiener_last->design, &d, sizeof(d)) != 0) {
                auto w = std::make_shared<TwinWiener>();
                w->geometry = geometry; w->design = d;
                w->tables = mgpu::build_wiener_tables(geometry->cell_type, geometry->Nsymb, geometry->Nc, geometry->pilot_boost, design);
                wiener_last = w;
            }
            twin = wiener_last;
        }
        return fn(*geometry, twin->tables);
    });
}
}  // namespace

extern "C" {

int mgpu_set_estimator_ladder_ex(mgpu_ctx* c, const mgpu_estimator_rung* rungs, int n_rungs, size_t rung_size) {
    if (!c) return MGPU_ERR_ARG;
    if (rung_size != sizeof(mgpu_estimator_rung)) return refuse(c, MGPU_ERR_ARG, "estimator ladder: rung_size is not this library's sizeof(mgpu_estimator_rung)");
    const auto& t = c->tab;
    if (n_rungs == 0 && c->lad.n == 0) return MGPU_OK;      // nothing set, nothing to clear: fine on every mode
    if (t.mfsk_M > 0 || t.estimator != MGPU_EST_LS) return refuse(c, MGPU_ERR_UNSUPPORTED, "an estimator ladder needs an OFDM mode with the LS estimator (the zero-forcing and MFSK modes have no window)");
    return guard(c, [&] {
        need(n_rungs >= 0 && n_rungs <= MGPU_LADDER_MAX && (rungs || n_rungs == 0), "estimator ladder: 0..MGPU_LADDER_MAX rungs");
        mgpu_ls_window win[MGPU_LADDER_MAX]{};
        for (int r = 0; r < n_rungs; ++r) {
            need(rungs[r].kind == MGPU_RUNG_LS || rungs[r].kind == MGPU_RUNG_WIENER, "estimator ladder: a rung is MGPU_RUNG_LS or MGPU_RUNG_WIENER");
            if (rungs[r].kind == MGPU_RUNG_WIENER) {
                const mgpu_wiener_design& d = rungs[r].design;
                need(mgpu::wiener_design_ok(mgpu::WienerDesign{d.tau_min_us, d.tau_max_us, d.doppler_hz, d.snr_db}),
                     "estimator ladder: a Wiener design needs tau_max > tau_min, doppler_hz >= 0 and snr_db in -20..40, all finite");
                continue;
            }
            win[r].width = window_side(rungs[r].window.width);
            win[r].height = window_side(rungs[r].window.height);
            need(win[r].width && win[r].height, "estimator ladder: a window is 1..21 cells wide (the front-end reads at most 7 pilots of a window row) and 1..21 high");
        }
        // everything that can fail comes before the context changes
        DevArray<double> weight[MGPU_LADDER_MAX], wA[MGPU_LADDER_MAX], wB[MGPU_LADDER_MAX];
        DevArray<int> woff[MGPU_LADDER_MAX];
        DevArray<uint16_t> widx[MGPU_LADDER_MAX];
        MgpuWiener wiener[MGPU_LADDER_MAX]{};
        for (int r = 0; r < n_rungs; ++r) {
            if (rungs[r].kind == MGPU_RUNG_LS) { weight[r] = upload(mgpu::ls_weight_table(t.pilot_boost, win[r].width * win[r].height)); continue; }
            const mgpu_wiener_design& d = rungs[r].design;
            const mgpu::WienerTables w = mgpu::build_wiener_tables(t.cell_type, t.Nsymb, t.Nc, t.pilot_boost, mgpu::WienerDesign{d.tau_min_us, d.tau_max_us, d.doppler_hz, d.snr_db});
            // the tables as MgpuWiener (ls_rect.h) names them
            std::vector<double> A, B;
            std::vector<int> off;
            for (const auto& m : w.A) { off.push_back(int(A.size())); A.insert(A.end(), m.begin(), m.end()); }
            const size_t b_off = off.size();
            for (const auto& m : w.B) { off.push_back(int(B.size() / 2)); for (const mgpu::Cplx& v : m) { B.push_back(v.re); B.push_back(v.im); } }
            const size_t nP = w.time_class.size();
            need(nP == size_t(t.nPilots), "estimator ladder: the Wiener tables' pilots are not the mode's");
            std::vector<uint16_t> idx(nP * 8), col_start(size_t(t.Nc), 0);
            size_t at_list = 0;
            for (int cc = 0; cc < t.Nc; ++cc) {
                col_start[size_t(cc)] = uint16_t(at_list);
                for (uint16_t p : w.col_pilots[size_t(cc)]) { idx.push_back(p); ++at_list; }
            }
            for (int cc = 0; cc < t.Nc; ++cc)
                for (uint16_t p : w.col_pilots[size_t(cc)]) {
                    uint16_t* e = &idx[size_t(p) * 8];
                    e[0] = w.time_class[p]; e[1] = w.time_row[p]; e[2] = uint16_t(w.time_members[w.time_class[p]].size()); e[3] = col_start[size_t(cc)];
                }
            for (int sy = 0; sy < t.Nsymb; ++sy)
                for (uint16_t p : w.row_pilots[size_t(sy)]) {
                    uint16_t* e = &idx[size_t(p) * 8];
                    e[4] = w.freq_class[p]; e[5] = w.freq_row[p]; e[6] = uint16_t(w.freq_members[w.freq_class[p]].size()); e[7] = w.row_pilots[size_t(sy)].front();
                    need(p == e[7] + e[5], "estimator ladder: a symbol's pilots are not consecutive in pilot order");
                }
            wA[r] = upload(A); wB[r] = upload(B); woff[r] = upload(off); widx[r] = upload(idx);
            wiener[r].A = wA[r]; wiener[r].B = wB[r];
            wiener[r].a_off = woff[r]; wiener[r].b_off = woff[r] + b_off;
            wiener[r].pilot = widx[r]; wiener[r].col_list = widx[r] + nP * 8;
            wiener[r].n_designs = 1;
        }
        const size_t B = size_t(c->max_batch);
        Ladder& L = c->lad;
        HIPCK(hipStreamSynchronize(c->stream));
        if (L.done_recorded) HIPCK(hipEventSynchronize(L.done));
        if (n_rungs > 0) {
            if (!L.done) HIPCK(hipEventCreateWithFlags(&L.done.h, hipEventDisableTiming));
            L.d_rung.grow(B * sizeof(int));
            L.d_counters.grow((MGPU_LADDER_MAX + 1) * sizeof(unsigned long long));
            frontend_raise_lds_limits(c);
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
            L.kind[r] = r < n_rungs ? rungs[r].kind : MGPU_RUNG_LS;
            L.design[r] = r < n_rungs && L.kind[r] == MGPU_RUNG_WIENER ? rungs[r].design : mgpu_wiener_design{};
            L.wiener_A[r] = std::move(wA[r]); L.wiener_B[r] = std::move(wB[r]); L.wiener_off[r] = std::move(woff[r]); L.wiener_idx[r] = std::move(widx[r]);
            L.wiener[r] = wiener[r];
            L.bank[r] = Ladder::Bank{};              // a new ladder carries no bank (include/mercury_wiener_bank.h)
            if (r >= n_rungs || L.kind[r] == MGPU_RUNG_WIENER) continue;
            const int hw_f = win[r].width / 2;
            L.win[r].weight = L.weight[r];
            L.win[r].hw_f = hw_f; L.win[r].hw_t = win[r].height / 2;
            // as create.hip does for the square window: 2 when every (clipped) window row holds >= 3 pilots of each column residue
            L.win[r].lattice = c->dev.regular_lattice ? (std::min(hw_f + 1, t.Nc) >= 9 ? 2 : 1) : 0;
        }
        L.rung0_is_default = n_rungs > 0 && L.kind[0] == MGPU_RUNG_LS && win[0].width == t.lsw && win[0].height == t.lsw;
        L.n = n_rungs;
        L.last_F = 0;
    });
}

int mgpu_set_estimator_ladder(mgpu_ctx* c, const mgpu_ls_window* rungs, int n_rungs) {      // the all-LS case
    if (!c) return MGPU_ERR_ARG;
    mgpu_estimator_rung ex[MGPU_LADDER_MAX]{};
    const bool countable = n_rungs >= 0 && n_rungs <= MGPU_LADDER_MAX && (rungs || n_rungs == 0);
    for (int r = 0; countable && r < n_rungs; ++r) { ex[r].kind = MGPU_RUNG_LS; ex[r].window = rungs[r]; }
    // a count the rungs cannot be read for is refused by the call below before it reads any
    return mgpu_set_estimator_ladder_ex(c, countable && n_rungs > 0 ? ex : nullptr, countable ? n_rungs : -1, sizeof(mgpu_estimator_rung));
}

int mgpu_get_estimator_ladder(mgpu_ctx* c, mgpu_ls_window* rungs, int* n_rungs) {
    if (!c || !n_rungs || !rungs) return MGPU_ERR_ARG;
    *n_rungs = c->lad.n;
    for (int r = 0; r < c->lad.n; ++r) rungs[r] = c->lad.rung[r];
    return MGPU_OK;
}

int mgpu_get_estimator_ladder_ex(mgpu_ctx* c, mgpu_estimator_rung* rungs, int* n_rungs, size_t rung_size) {
    if (!c || !n_rungs || !rungs || rung_size != sizeof(mgpu_estimator_rung)) return MGPU_ERR_ARG;
    *n_rungs = c->lad.n;
    for (int r = 0; r < c->lad.n; ++r) rungs[r] = mgpu_estimator_rung{c->lad.kind[r], c->lad.rung[r], c->lad.design[r]};
    return MGPU_OK;
}

// ---- a Wiener rung's bank of designs (include/mercury_wiener_bank.h) ----
namespace {
// the bank as wiener_tables.cpp takes it; throws std::invalid_argument where it is refused
mgpu::WienerBankRule bank_rule(const std::vector<uint8_t>& cell_type, int Nsymb, int Nc, const mgpu_wiener_bank_entry* e, int n, mgpu::WienerDesign* designs) {
    double rho[MGPU_WIENER_BANK_MAX]{};
    need(n >= 1 && n <= MGPU_WIENER_BANK_MAX && e, "Wiener bank: 1..MGPU_WIENER_BANK_MAX entries");
    for (int d = 0; d < n; ++d) {
        designs[d] = mgpu::WienerDesign{e[d].design.tau_min_us, e[d].design.tau_max_us, e[d].design.doppler_hz, e[d].design.snr_db};
        rho[d] = e[d].rho_min;
    }
    return mgpu::build_wiener_bank_rule(cell_type, Nsymb, Nc, designs, rho, n);
}
}  // namespace

int mgpu_set_wiener_bank(mgpu_ctx* c, int rung, const mgpu_wiener_bank_entry* e, int n, size_t entry_size) {
    if (!c) return MGPU_ERR_ARG;
    if (entry_size != sizeof(mgpu_wiener_bank_entry)) return refuse(c, MGPU_ERR_ARG, "Wiener bank: entry_size is not this library's sizeof(mgpu_wiener_bank_entry)");
    return guard(c, [&] {
        const auto& t = c->tab;
        Ladder& L = c->lad;
        need(rung >= 0 && rung < L.n && L.kind[rung] == MGPU_RUNG_WIENER, "Wiener bank: the ladder in force has no Wiener rung of that number");
        need(n >= 0 && n <= MGPU_WIENER_BANK_MAX && (e || n == 0), "Wiener bank: 0..MGPU_WIENER_BANK_MAX entries");
        // everything that can fail comes before the context changes
        Ladder::Bank nb;
        MgpuWiener w = L.wiener[rung];
        w.A = L.wiener_A[rung]; w.B = L.wiener_B[rung];
        w.n_designs = 1; w.bank = nullptr;
        if (n > 0) {
            mgpu::WienerDesign designs[MGPU_WIENER_BANK_MAX];
            const mgpu::WienerBankRule rule = bank_rule(t.cell_type, t.Nsymb, t.Nc, e, n, designs);
            need(t.nPilots >= 2 * t.Nsymb, "Wiener bank: the symbols' partial sums do not fit the pilots' area");
            std::vector<double> A, B;
            size_t a_stride = 0, b_stride = 0;
            for (int d = 0; d < n; ++d) {
                const mgpu::WienerTables wt = mgpu::build_wiener_tables(t.cell_type, t.Nsymb, t.Nc, t.pilot_boost, designs[d]);
                const size_t a0 = A.size(), b0 = B.size();
                for (const auto& m : wt.A) A.insert(A.end(), m.begin(), m.end());
                for (const auto& m : wt.B) for (const mgpu::Cplx& v : m) { B.push_back(v.re); B.push_back(v.im); }
                if (d == 0) { a_stride = A.size(); b_stride = B.size() / 2; }
                need(A.size() - a0 == a_stride && B.size() - b0 == 2 * b_stride, "Wiener bank: the designs' tables differ in shape");
            }
            std::vector<uint16_t> idx = rule.pair;
            idx.insert(idx.end(), rule.sym_first.begin(), rule.sym_first.end());
            nb.n = n; nb.n1 = rule.n1; nb.n2 = rule.n2;
            for (int d = 0; d < n; ++d) { nb.e[d] = e[d]; if (d + 1 < n) nb.e[d].rho_min = rule.rho_min[size_t(d)]; }
            nb.A = upload(A); nb.B = upload(B); nb.idx = upload(idx);
            std::vector<MgpuWienerBank> arg(1);
            arg[0].a_stride = int(a_stride); arg[0].b_stride = int(b_stride);
            arg[0].pair = nb.idx; arg[0].sym_first = nb.idx + rule.pair.size();
            arg[0].n1sq = double(rule.n1) * double(rule.n1); arg[0].n2sq = double(rule.n2) * double(rule.n2);
            for (size_t i = 0; i < sizeof(arg[0].sel) / sizeof(double); ++i) arg[0].sel[i / 4][i % 4] = i < rule.sel.size() ? rule.sel[i] : 0.0;
            nb.arg = upload(arg);
            w.A = nb.A; w.B = nb.B;
            w.n_designs = n; w.bank = nb.arg;
        }
        const size_t B = size_t(c->max_batch);
        HIPCK(hipStreamSynchronize(c->stream));
        if (L.done_recorded) HIPCK(hipEventSynchronize(L.done));
        if (n > 0 && rung == 0) {
            L.d_choice.grow(B * sizeof(int)); L.d_corr.grow(B * 4 * sizeof(double));
            HIPCK(hipMemset(L.d_choice, 0, B * sizeof(int)));
            HIPCK(hipMemset(L.d_corr, 0, B * 4 * sizeof(double)));
        }
        L.bank[rung] = std::move(nb);
        L.wiener[rung] = w;
    });
}

int mgpu_get_wiener_bank(mgpu_ctx* c, int rung, mgpu_wiener_bank_entry* e, int* n, size_t entry_size) {
    if (!c || !n || !e || entry_size != sizeof(mgpu_wiener_bank_entry)) return MGPU_ERR_ARG;
    if (rung < 0 || rung >= c->lad.n || c->lad.kind[rung] != MGPU_RUNG_WIENER) return MGPU_ERR_ARG;
    *n = c->lad.bank[rung].n;
    for (int d = 0; d < *n; ++d) e[d] = c->lad.bank[rung].e[d];
    return MGPU_OK;
}

int mgpu_get_wiener_choice(mgpu_ctx* c, int first, int count, int* design, double* corr, int* n1, int* n2) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        const Ladder& L = c->lad;
        need(L.n > 0 && L.kind[0] == MGPU_RUNG_WIENER && L.bank[0].n > 0, "rung 0 has no Wiener bank");
        need(first >= 0 && count >= 0, "bad argument (first + count must be <= max_batch)");
        read_rows(c, L.d_choice, 1, first, count, design, "rung 0 has no Wiener bank");
        read_rows(c, L.d_corr, 4, first, count, corr, "rung 0 has no Wiener bank");
        if (n1) *n1 = L.bank[0].n1;
        if (n2) *n2 = L.bank[0].n2;
    });
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

int mgpu_host_ls_estimate(int cfg, const mgpu_explicit_params* p, int width, int height, const double* grid, double* H) {
    if (!grid || !H) return MGPU_ERR_ARG;
    const int wf = window_side(width), wt = window_side(height);
    if (!wf || !wt) return MGPU_ERR_ARG;
    return ls_twin(cfg, p, [&](const std::shared_ptr<const TwinGeometry>& geometry) -> int {
        const TwinGeometry& t = *geometry;
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
    });
}

int mgpu_host_wiener_estimate(int cfg, const mgpu_explicit_params* p, const mgpu_wiener_design* d, const double* grid, double* H) {
    if (!grid || !H) return MGPU_ERR_ARG;
    return wiener_twin(cfg, p, d, [&](const TwinGeometry& t, const mgpu::WienerTables& w) -> int {
        const size_t nP = w.time_class.size();
        std::vector<double> yp(2 * nP), tp(2 * nP);
        size_t pilot = 0;
        for (int q = 0; q < t.Nsymb * t.Nc; ++q) {      // the pilots times their sign, in pilot order
            if (!t.cell_type[size_t(q)]) continue;
            const bool neg = t.pilot_val[size_t(q)] < 0;
            yp[2 * pilot] = neg ? -grid[2 * q] : grid[2 * q];
            yp[2 * pilot + 1] = neg ? -grid[2 * q + 1] : grid[2 * q + 1];
            ++pilot;
        }
        for (int cc = 0; cc < t.Nc; ++cc) {             // along time, per carrier
            const auto& list = w.col_pilots[size_t(cc)];
            const size_t n = list.size();
            for (size_t i = 0; i < n; ++i) {
                const double* a = &w.A[w.time_class[list[i]]][i * n];
                double hr = 0, hi = 0;
                for (size_t k = 0; k < n; ++k) { hr += a[k] * yp[2 * list[k]]; hi += a[k] * yp[2 * list[k] + 1]; }
                tp[2 * list[i]] = hr; tp[2 * list[i] + 1] = hi;
            }
        }
        for (int sy = 0; sy < t.Nsymb; ++sy) {          // along frequency, per symbol
            const auto& list = w.row_pilots[size_t(sy)];
            const size_t n = list.size();
            for (size_t i = 0; i < n; ++i) {
                const mgpu::Cplx* b = &w.B[w.freq_class[list[i]]][i * n];
                double hr = 0, hi = 0;
                for (size_t m = 0; m < n; ++m) {
                    const double tr = tp[2 * list[m]], ti = tp[2 * list[m] + 1];
                    hr += b[m].re * tr - b[m].im * ti;
                    hi += b[m].re * ti + b[m].im * tr;
                }
                H[2 * list[i]] = hr; H[2 * list[i] + 1] = hi;
            }
        }
        return MGPU_OK;
    });
}

int mgpu_host_wiener_select(int cfg, const mgpu_explicit_params* p, const mgpu_wiener_bank_entry* e, int n, size_t entry_size, const double* grid,
                            int* design, double corr[4], int* n1, int* n2) {
    if (!grid || !e || entry_size != sizeof(mgpu_wiener_bank_entry) || n < 1 || n > MGPU_WIENER_BANK_MAX) return MGPU_ERR_ARG;
    return ls_twin(cfg, p, [&](const std::shared_ptr<const TwinGeometry>& geometry) -> int {
        const TwinGeometry& t = *geometry;
        mgpu::WienerDesign designs[MGPU_WIENER_BANK_MAX];
        const mgpu::WienerBankRule rule = bank_rule(t.cell_type, t.Nsymb, t.Nc, e, n, designs);
        const size_t nP = rule.pair.size();
        std::vector<double> yp(2 * nP + 4, 0.0);
        size_t pilot = 0;
        for (int q = 0; q < t.Nsymb * t.Nc; ++q) {      // the pilots times their sign, in pilot order
            if (!t.cell_type[size_t(q)]) continue;
            const bool neg = t.pilot_val[size_t(q)] < 0;
            yp[2 * pilot] = neg ? -grid[2 * q] : grid[2 * q];
            yp[2 * pilot + 1] = neg ? -grid[2 * q + 1] : grid[2 * q + 1];
            ++pilot;
        }
        double R1r = 0, R1i = 0, R2r = 0, R2i = 0;
        for (int sy = 0; sy < t.Nsymb; ++sy) {          // a symbol's terms in ascending a, then the symbols in ascending order
            double r1r = 0, r1i = 0, r2r = 0, r2i = 0;
            for (size_t a = rule.sym_first[size_t(sy)]; a < rule.sym_first[size_t(sy) + 1]; ++a) {
                const double ar = yp[2 * a], ai = yp[2 * a + 1];
                if (rule.pair[a] & 1) { const double br = yp[2 * a + 2], bi = yp[2 * a + 3]; r1r += (ar * br) + (ai * bi); r1i += (ar * bi) - (ai * br); }
                if (rule.pair[a] & 2) { const double br = yp[2 * a + 4], bi = yp[2 * a + 5]; r2r += (ar * br) + (ai * bi); r2i += (ar * bi) - (ai * br); }
            }
            R1r += r1r; R1i += r1i; R2r += r2r; R2i += r2i;
        }
        const double n1sq = double(rule.n1) * double(rule.n1), n2sq = double(rule.n2) * double(rule.n2);
        const double q2 = (R2r * R2r + R2i * R2i) * n1sq, q1 = (R1r * R1r + R1i * R1i) * n2sq;
        int ch = n - 1;                                 // the fallback; the first eligible entry in bank order otherwise
        for (int d = n - 2; d >= 0; --d) {
            const double rho2 = rule.sel[size_t(4) * d], ur = rule.sel[size_t(4) * d + 1], ui = rule.sel[size_t(4) * d + 2], tn = rule.sel[size_t(4) * d + 3];
            bool ok = q2 >= rho2 * q1;                  // every comparison fails on a NaN
            if (tn >= 0) {
                const double zr = R1r * ur + R1i * ui, zi = R1i * ur - R1r * ui;
                ok = ok && zr > 0 && std::fabs(zi) <= tn * zr;
            }
            if (ok) ch = d;
        }
        if (design) *design = ch;
        if (corr) { corr[0] = R1r; corr[1] = R1i; corr[2] = R2r; corr[3] = R2i; }
        if (n1) *n1 = rule.n1;
        if (n2) *n2 = rule.n2;
        return MGPU_OK;
    });
}

int mgpu_host_wiener_bank_thresholds(int cfg, const mgpu_explicit_params* p, const mgpu_wiener_bank_entry* e, int n, size_t entry_size, double* rho_min,
                                     int* pilot_spacing) {
    if (!e || entry_size != sizeof(mgpu_wiener_bank_entry) || n < 1 || n > MGPU_WIENER_BANK_MAX) return MGPU_ERR_ARG;
    return ls_twin(cfg, p, [&](const std::shared_ptr<const TwinGeometry>& geometry) -> int {
        mgpu::WienerDesign designs[MGPU_WIENER_BANK_MAX];
        const mgpu::WienerBankRule rule = bank_rule(geometry->cell_type, geometry->Nsymb, geometry->Nc, e, n, designs);
        if (rho_min) std::copy(rule.rho_min.begin(), rule.rho_min.end(), rho_min);
        if (pilot_spacing) *pilot_spacing = rule.s;
        return MGPU_OK;
    });
}

int mgpu_host_wiener_tables(int cfg, const mgpu_explicit_params* p, const mgpu_wiener_design* d, int which, int cls, int* n_classes, int* n,
                            int* members, double* matrix) {
    if (which != 0 && which != 1) return MGPU_ERR_ARG;
    return wiener_twin(cfg, p, d, [&](const TwinGeometry&, const mgpu::WienerTables& w) -> int {
        const auto& sets = which == 0 ? w.time_members : w.freq_members;
        if (n_classes) *n_classes = int(sets.size());
        if (!n && !members && !matrix) return MGPU_OK;
        if (cls < 0 || size_t(cls) >= sets.size()) return MGPU_ERR_ARG;
        const size_t m = sets[size_t(cls)].size();
        if (n) *n = int(m);
        if (members) std::copy(sets[size_t(cls)].begin(), sets[size_t(cls)].end(), members);
        if (matrix && which == 0) std::copy(w.A[size_t(cls)].begin(), w.A[size_t(cls)].end(), matrix);
        if (matrix && which == 1)
            for (size_t i = 0; i < m * m; ++i) { matrix[2 * i] = w.B[size_t(cls)][i].re; matrix[2 * i + 1] = w.B[size_t(cls)][i].im; }
        return MGPU_OK;
    });
}

}  // extern "C"

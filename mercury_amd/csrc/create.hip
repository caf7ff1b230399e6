// The context's life and everything that needs no launch (include/mercury_gpu.h): the plan of a mode's tables and launch shapes, their
// upload, the lazily created workspaces, mgpu_create / mgpu_destroy, host allocation, and the pieces callable without a GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "ctx.hpp"
#include "numa.hpp"

thread_local std::string g_create_error;

namespace mgpu_detail {

constexpr size_t kLdsBytes = size_t(160) * 1024;     // LDS of a compute unit: every kernel's dynamic carve must fit it

struct Plan { std::vector<uint16_t> pilot_cell, crc_tab; std::vector<uint32_t> cell_lerp; std::vector<double> cons, tw; };

// The part of mgpu_create that needs no device: the scalars of dev / ldev, the launch shapes, LDS sizes and decoder instance go into the
// context, the derived tables into the plan. Everything it refuses is refused before any device work (MGPU_ERR_TABLES).
Plan ctx_plan(mgpu_ctx* c) {
    const auto& t = c->tab;
    MgpuDev& d = c->dev;
    Plan p;
    for (int i = 0; i < t.Nsymb * t.Nc; ++i) if (t.cell_type[i]) p.pilot_cell.push_back(uint16_t(i));
    for (auto& z : t.constellation) { p.cons.push_back(z.re); p.cons.push_back(z.im); }
    for (auto& z : t.twiddle) { p.tw.push_back(z.re); p.tw.push_back(z.im); }
    if (t.mfsk_M == 0) {
        // The two pilot rows a data cell (i, j) interpolates between and their pilots' indices, tabulated from the lattice itself the way
        // interpolate_linear_col walks a column (interpolator.cc:163-254): between two measured rows the nearest one above and the nearest
        // one below; above the column's first measured row the first two, below its last one the last two (extrapolation). Every column
        // needs two pilots (a column with fewer is refused: the reference's walk degenerates there). The kernel used to derive all of this
        // per cell from divisions by 50 and 3.
        const std::vector<uint16_t>& pilot_cell = p.pilot_cell;
        std::vector<int> pilot_of_cell(size_t(t.Nsymb) * t.Nc, -1);
        for (size_t q = 0; q < pilot_cell.size(); ++q) pilot_of_cell[pilot_cell[q]] = int(q);
        std::vector<uint32_t>& tab = p.cell_lerp;
        tab.assign(size_t(t.nData) * 2, 0u);
        bool ok = t.Nsymb >= 2 && t.Nsymb * t.Nc < 4096 && pilot_cell.size() < 1024 && t.Nsymb < 256;
        std::vector<std::vector<int>> col_rows(size_t(t.Nc));
        for (int i = 0; i < t.Nsymb; ++i)
            for (int j = 0; j < t.Nc; ++j) if (pilot_of_cell[size_t(i) * t.Nc + j] >= 0) col_rows[size_t(j)].push_back(i);
        for (int k = 0; k < t.nData && ok; ++k) {
            const int cell = t.data_cell[k], i = cell / t.Nc, j = cell - i * t.Nc;
            const std::vector<int>& rows = col_rows[size_t(j)];
            if (rows.size() < 2) { ok = false; break; }
            int a, b;
            if (i < rows.front()) { a = rows[0]; b = rows[1]; }
            else if (i > rows.back()) { a = rows[rows.size() - 2]; b = rows.back(); }
            else {
                const size_t hi = size_t(std::upper_bound(rows.begin(), rows.end(), i) - rows.begin());     // a data cell is never a measured row itself
                a = rows[hi - 1]; b = rows[hi];
            }
            tab[2 * size_t(k)] = uint32_t(cell) | uint32_t(pilot_of_cell[size_t(a) * t.Nc + j]) << 12 | uint32_t(pilot_of_cell[size_t(b) * t.Nc + j]) << 22;
            tab[2 * size_t(k) + 1] = uint32_t(a) | uint32_t(b) << 8 | uint32_t(i) << 16;
        }
        if (!ok) throw std::runtime_error("pilot lattice / frame geometry outside what the front-end kernel's interpolation table covers");
    }
    d.S = t.graph.S;
    d.M = t.M; d.bps = t.bps; d.K = t.K; d.P = t.P; d.N = t.N; d.E = t.graph.E;
    d.Nsymb = t.Nsymb; d.G = t.Nsymb * t.Nc; d.nData = t.nData; d.nBits = t.nBits; d.nPilots = t.nPilots;
    d.nVirtual = t.nVirtual; d.nReal = t.nReal;
    d.estimator = t.estimator; d.amp_restore = t.amp_restore; d.lsw = t.lsw;
    d.payload_bytes = t.payload_bytes; d.payload_stride = t.payload_stride; d.frame_samples = t.frame_samples;
    d.agc = c->cfg.agc; d.var_eq = c->cfg.variance_source; d.max_iters = c->cfg.max_iters;
    d.pilot_boost = t.pilot_boost;
    d.staircase = 1;
    for (int q = 0; q < t.P && d.staircase; ++q) {
        int others = 0;
        for (uint32_t e = t.graph.cptr[q]; e < t.graph.cptr[q + 1]; ++e) {
            const int v = t.graph.cvar[e];
            if (v >= t.K && v != t.K + q) { ++others; if (v != t.K + q - 1) d.staircase = 0; }
        }
        if (others != (q == 0 ? 0 : 1)) d.staircase = 0;
    }
    d.regular_lattice = 1;
    for (int r = 0; r < t.Nsymb; ++r)
        for (int q = 0; q < t.Nc; ++q)
            if ((t.cell_type[size_t(r) * t.Nc + q] != 0) != (((r - q) % 3 + 3) % 3 == 0)) d.regular_lattice = 0;
    if (t.mfsk_M == 0 && t.Nc != 50) throw std::runtime_error("the front-end kernel is specialised for 50 carriers");
    // regular_lattice == 0 (an explicit Dy other than 3: include/mercury_gpu.h mgpu_explicit_params): the estimator takes its general path - the
    // reference's own walk over the window's cells (frontend.hip) - everything else is table-driven and does not care
    if (d.regular_lattice && std::min(t.lsw / 2 + 1, t.Nc) >= 9) d.regular_lattice = 2;   // and every (clipped) window row holds >= 3 pilots of each column residue
    d.minsum_alpha = c->cfg.minsum_alpha > 0 ? c->cfg.minsum_alpha : 0.8f;
    d.mfsk_M = t.mfsk_M; d.mfsk_nbits = t.mfsk_nbits; d.mfsk_nstreams = t.mfsk_nstreams; d.mfsk_hop = t.mfsk_hop;
    d.mfsk_off0 = t.mfsk_off[0]; d.mfsk_off1 = t.mfsk_off[1];
    d.active_nsymb = t.active_nsymb; d.active_nbits = t.active_nbits; d.mfsk_amp = t.mfsk_amp;
    d.puncture_from = (c->cfg.test_puncture_nBits > 0 && c->cfg.test_puncture_nBits < t.active_nbits) ? c->cfg.test_puncture_nBits : t.active_nbits;
    LdpcDev& l = c->ldev;
    {   // the CRC as a sum of per-bit constants (crc16_modbus_rtu.cc:25-45 is linear over GF(2) up to the register's initial value)
        const int full = d.nReal / 8;
        std::vector<uint8_t> msg(size_t(full > 0 ? full : 1), 0);
        const uint16_t zero = mgpu::crc16_modbus(msg.data(), full);
        p.crc_tab.assign(size_t(full > 0 ? full : 1) * 8, 0);
        for (int b = 0; b < full; ++b)
            for (int j = 0; j < 8; ++j) {
                msg[b] = uint8_t(1u << j);
                p.crc_tab[size_t(b) * 8 + j] = uint16_t(mgpu::crc16_modbus(msg.data(), full) ^ zero);
                msg[b] = 0;
            }
        l.crc_init = zero;
    }
    l.Sg = t.graph.Sg;
    l.DM = t.graph.DM;
    l.S = d.S; l.N = d.N; l.P = d.P; l.K = d.K; l.E = d.E; l.nReal = d.nReal; l.payload_stride = d.payload_stride;
    l.max_iters = d.max_iters; l.minsum_alpha = d.minsum_alpha;
    {   // fp64 decoder, a frame's first iterations (ldpc.hip "adaptive"): from how many odd checks on - estimated from the 16 bins a judged look
        // samples - the next iteration's posteriors (the next two iterations') are looked at inside the following check pass instead of by a
        // pass of their own. Two pairs of weights: for the look at the channel's hard decisions (the first iteration removes far more errors
        // than any later one) and for the later looks; defaults from tests/tools/unsat_profile.py and profiles/r06_ab_spec*.txt. Results do
        // not depend on them. MERCURY_SPA_SPEC_WEIGHT="first:1,first:2,later:1,later:2" for experiments (0 = always, a huge value = never).
        int w[4] = {100, 230, 45, 150};
        if (const char* e = getenv("MERCURY_SPA_SPEC_WEIGHT")) {
            const int n = sscanf(e, "%d,%d,%d,%d", &w[0], &w[1], &w[2], &w[3]);
            if (n == 1) { w[1] = w[2] = w[3] = w[0]; }
            else if (n == 2) { w[2] = w[0]; w[3] = w[1]; }
            else if (n == 3) { w[3] = w[2]; }
        }
        const int nbins = d.S / 64 > 0 ? d.S / 64 : 1;
        auto sample_min = [&](int weight) {
            const long long m = (static_cast<long long>(weight) * 16 + nbins - 1) / nbins;
            return weight <= 0 ? 0 : (m > 0x7fffff ? 0x7fffff : int(m));
        };
        auto byte = [&](int weight) { const int m = sample_min(weight); return unsigned(m > 255 ? 255 : m); };      // (a wavefront's first bin holds at most 64 checks, 16 wavefronts: "never" is any value above 1024 - 255 stands for it, see ldpc.hip)
        l.spec_sample_pack = byte(w[0]) | byte(w[1]) << 8 | byte(w[2]) << 16 | byte(w[3]) << 24;
    }

    const bool mfsk = t.mfsk_M > 0;      // the MFSK front-end keeps no frame grid in LDS (csrc/mfsk.hip)
    {
        const char* e = getenv("MERCURY_FE_THREADS");
        const size_t lds512 = mfsk ? 0 : mgpu_frontend_lds_bytes(d.G, d.nPilots, d.nBits, 512);
        c->fe_threads = e ? atoi(e) : (lds512 > kLdsBytes / 2 ? 1024 : 512);
        if (c->fe_threads != 512 && c->fe_threads != 1024) throw std::invalid_argument("MERCURY_FE_THREADS must be 512 or 1024");
        c->lds_fe = mfsk ? 0 : mgpu_frontend_lds_bytes(d.G, d.nPilots, d.nBits, c->fe_threads);
    }
    c->lds_tx = mgpu_txgen_lds_bytes(mfsk ? 0 : d.G);
    switch (c->cfg.decoder) {
        case MGPU_DEC_SPA: {
            if (!t.graph.fp64_limit.empty()) throw std::runtime_error(t.graph.fp64_limit);
            c->lds_dec = mgpu_spa_lds_bytes(d.S, d.N);
            const int ne = std::max(4, (d.S + 1023) / 1024);      // rounds of 16 bins; the smallest instance runs 4 (tables sized to match)
            if (ne > 8) throw std::runtime_error("graph too large for the sum-product kernel");
            if (t.graph.maxdeg > mgpu_spa_max_degree(ne)) throw std::runtime_error("check degree exceeds the sum-product kernel's unrolled product walk");
            const DecoderKernel by_ne[5] = {mgpu_ldpc_spa_kernel_ne4, mgpu_ldpc_spa_kernel_ne5, mgpu_ldpc_spa_kernel_ne6, mgpu_ldpc_spa_kernel_ne7, mgpu_ldpc_spa_kernel_ne8};
            c->spa_kernel = by_ne[ne - 4];
            break;
        }
        case MGPU_DEC_GBF:
            c->lds_dec = mgpu_gbf_lds_bytes(d.N);
            break;
        case MGPU_DEC_MINSUM:
        case MGPU_DEC_SPA_FAST:
            if (!t.graph.fp32_limit.empty()) throw std::runtime_error(t.graph.fp32_limit);
            c->lds_dec = mgpu_spa_fast_lds_bytes(l.Sg, d.N);
            c->dec_threads = 512;            // SPA_FAST: 8 wavefronts per barrier domain, the kernel is bound by waits, not by issue (1024 threads: 1.4x slower)
            c->spa_kernel = c->cfg.decoder == MGPU_DEC_MINSUM ? mgpu_ldpc_minsum_kernel_t512 : mgpu_ldpc_spa_fast_kernel_t512;
            break;
        default: throw std::runtime_error("unknown decoder");
    }
    if (c->lds_fe > kLdsBytes) throw std::runtime_error("frame geometry too large for the front-end kernel's LDS carve");
    if (c->lds_dec > kLdsBytes) throw std::runtime_error("code too large for the decoder kernel's LDS");
    if (c->lds_tx > kLdsBytes) throw std::runtime_error("frame geometry too large for the generator kernel's LDS");
    return p;
}

// The rest of mgpu_create, on the device: the plan's and the mode's tables, the context's stream and events, the kernels' LDS limits.
void ctx_upload(mgpu_ctx* c, const Plan& p) {
    const auto& t = c->tab;
    MgpuDev& d = c->dev;
    LdpcDev& l = c->ldev;
    d.cell_type = c->keep(t.cell_type);
    d.pilot_val = c->keep(t.pilot_val);
    d.pilot_cell = c->keep(p.pilot_cell);
    d.constellation = c->keep(p.cons);
    d.twiddle = c->keep(p.tw);
    d.sym_src = c->keep(t.sym_src);
    d.llr_src = c->keep(t.llr_src);
    d.ls_weight = c->keep(t.ls_weight);
    d.scrambler = c->keep(t.scrambler);
    d.llr_dst = c->keep(t.llr_dst);
    d.bit_il = c->keep(t.bit_il);
    c->d_fir[0] = c->keep(t.fir_time_sync);
    c->d_fir[1] = c->keep(t.fir_data);
    d.tf_inv = c->keep(t.tf_inv);
    d.data_cell = c->keep(t.data_cell);
    d.cell_lerp = t.mfsk_M == 0 ? c->keep(p.cell_lerp) : nullptr;
    d.cptr = c->keep(t.graph.cptr);
    d.cvar = c->keep(t.graph.cvar);
    l.scrambler = d.scrambler;
    l.cptr = d.cptr; l.cvar = d.cvar;
    l.crc_tab = c->keep(p.crc_tab);
    l.gdesc = c->keep(t.graph.gdesc);
    l.gkpack = c->keep(t.graph.gkpack);
    l.vinfo_g = c->keep(t.graph.vinfo_g);
    l.sadr = c->keep(t.graph.sadr);
    l.bhead = c->keep(t.graph.bhead);
    l.bmask = c->keep(t.graph.bmask);
    l.vinfo2 = c->keep(t.graph.vinfo2);
    l.hard_frames = reinterpret_cast<unsigned long long*>(c->keep(std::vector<uint64_t>(64, 0)));
    HIPCK(hipStreamCreate(&c->stream.h));
    for (auto& q : c->kt.ev) for (auto& e : q) HIPCK(hipEventCreate(&e.h));
    for (auto& e : c->sync_ev) HIPCK(hipEventCreate(&e.h));
    auto lds_limit = [](auto kernel, size_t bytes) {
        HIPCK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes)));
    };
    if (t.mfsk_M == 0) lds_limit(mgpu_frontend_form_kernel(c->fe_threads, 0), c->lds_fe);     // the plain form alone: an option's setter raises the others (frontend_raise_lds_limits)
    // the context's own square LS window as the front-end's rectangular forms take it
    c->own_window = MgpuLsRect{};
    c->own_window.weight = d.ls_weight;
    c->own_window.hw_f = c->own_window.hw_t = t.lsw / 2;
    c->own_window.lattice = d.regular_lattice;
    lds_limit(mgpu_txgen_kernel, c->lds_tx);
    lds_limit(mgpu_tsync_metric_fine_kernel_r4, mgpu_tsync_fine_geometry(4).lds_bytes);
    lds_limit(mgpu_tsync_metric_fine_kernel_r8, mgpu_tsync_fine_geometry(8).lds_bytes);
    lds_limit(c->cfg.decoder == MGPU_DEC_GBF ? mgpu_ldpc_gbf_kernel : c->spa_kernel, c->lds_dec);
}

// Workspaces sized by max_batch are created on first use, so a context that only ever runs e.g. the
// decoder on caller-owned device buffers (the 10^7-codeword soak) does not pin tens of GB it never touches.
void ensure_workspaces(mgpu_ctx* c, unsigned what) {
    const auto& t = c->tab;
    const size_t B = size_t(c->max_batch);
    if ((what & WS_FRONTEND) && !c->d_variance) {
        c->d_variance.grow(B * sizeof(float));
        c->d_snrvar.grow(B * sizeof(float));
        if (t.estimator == MGPU_EST_ZF) c->d_eqdata.grow(B * t.nData * 16);
    }
    if ((what & WS_LLR) && !c->d_llr) c->d_llr.grow(B * t.N * sizeof(float));
    if ((what & WS_OUT) && !c->d_payload) {
        c->d_payload.grow(B * t.payload_stride);
        c->d_stats.grow(B * sizeof(MgpuStatsDev));
    }
    if ((what & WS_BITS) && !c->d_bits) {
        c->d_bits.grow(B * t.K);
        c->d_iters.grow(B * sizeof(int));
    }
}

// page-locked host memory on `node` (the GPU's NUMA node) when there is one: hipHostMallocNumaUser makes the runtime honour the calling
// thread's memory policy, which prefers that node while the allocation (and the page-locking first touch) runs
hipError_t host_alloc_on_node(void** p, size_t bytes, int node) {
    if (node >= 0) {
        mgpu_numa::PreferNode scope(node);
        if (scope.active() && hipHostMalloc(p, bytes, hipHostMallocNumaUser) == hipSuccess) return hipSuccess;
        (void)hipGetLastError();
    }
    return hipHostMalloc(p, bytes, hipHostMallocDefault);
}
int device_numa_node(int device) {
    char id[32] = {0};
    if (hipDeviceGetPCIBusId(id, int(sizeof(id)), device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return mgpu_host_numa_node_of_pci(id);
}

bool explicit_params_from(const mgpu_explicit_params* xp_in, mgpu::ExplicitParams& xp, std::string& err, int* rc) {
    if (xp_in) {
        // the kernels are specialised for the reference's carrier count, transform length and pilot column step: those fields only confirm them
        if ((xp_in->Nc != 0 && xp_in->Nc != 50) || (xp_in->Nfft != 0 && xp_in->Nfft != 256) || (xp_in->Dx != 0 && xp_in->Dx != 1)) {
            err = "explicit parameters: Nc / Nfft / Dx other than 50 / 256 / 1 are not supported (the kernels are specialised for them)";
            *rc = MGPU_ERR_UNSUPPORTED; return false;
        }
        if (xp_in->Dy < 0 || xp_in->Dy > 255 || xp_in->Nsymb < 0 || xp_in->Nsymb > 255) { err = "explicit parameters: Dy / Nsymb must be 0 (the reference's default) .. 255"; *rc = MGPU_ERR_ARG; return false; }
        if (xp_in->Dy != 0) xp.Dy = xp_in->Dy;
        xp.Nsymb = xp_in->Nsymb;
        if (xp_in->pilot_boost != 0.0f) xp.pilot_boost = xp_in->pilot_boost;
        if (xp_in->ls_window != 0) xp.ls_window = xp_in->ls_window;
        if (xp_in->ls_window < 0 || xp_in->ls_window > 21) { err = "explicit parameters: ls_window must be 1..21 (0 = the reference's 20)"; *rc = MGPU_ERR_ARG; return false; }
        if (!(xp.pilot_boost > 0.0f) || !(xp.pilot_boost < 1e6f)) { err = "explicit parameters: pilot_boost must be positive and finite (0 = the reference's 1.33)"; *rc = MGPU_ERR_ARG; return false; }
        if (xp_in->seeds_set) { xp.pilot_seed = xp_in->pilot_seed; xp.scrambler_seed = xp_in->scrambler_seed; xp.preamble_seed = xp_in->preamble_seed; }
    }
    return true;
}

}  // namespace mgpu_detail

extern "C" {

int mgpu_create(const mgpu_config* cfg, mgpu_ctx** out) { return mgpu_create_explicit(cfg, nullptr, out); }

extern "C" void mgpu_internal_libm_notice();     // libm_check.cpp

int mgpu_create_explicit(const mgpu_config* cfg, const mgpu_explicit_params* xp_in, mgpu_ctx** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return MGPU_ERR_ARG; }
    *out = nullptr;
    mgpu_internal_libm_notice();                 // only with MERCURY_GPU_LIBM_CHECK=1: is the host's libm the one the device restates? (once per process; stderr only if not)
    mgpu::ExplicitParams xp;
    {
        int rc = MGPU_OK;
        if (!mgpu_detail::explicit_params_from(xp_in, xp, g_create_error, &rc)) return rc;
    }
    int em, er, ep, ee;
    if (!((cfg->cfg >= 0 && cfg->cfg <= 16) || (cfg->cfg >= 100 && cfg->cfg <= 102) || mgpu::explicit_mode_row(cfg->cfg, &em, &er, &ep, &ee))) {
        g_create_error = "cfg must be 0..16 (OFDM modes), 100..102 (ROBUST MFSK modes) or an MGPU_CFG_EXPLICIT id";
        return MGPU_ERR_ARG;
    }
    if (cfg->max_iters < 1 || cfg->max_iters > 1000) { g_create_error = "max_iters out of range"; return MGPU_ERR_ARG; }
    if (cfg->decoder < 0 || cfg->decoder > MGPU_DEC_SPA_FAST) { g_create_error = "unknown decoder"; return MGPU_ERR_ARG; }
    if (cfg->max_batch < 1) { g_create_error = "max_batch must be >= 1"; return MGPU_ERR_ARG; }
    if (cfg->test_puncture_nBits < 0) { g_create_error = "test_puncture_nBits must be >= 0"; return MGPU_ERR_ARG; }
    std::unique_ptr<mgpu_ctx> c(new mgpu_ctx());
    c->cfg = *cfg;
    c->max_batch = cfg->max_batch;
    mgpu_detail::Plan plan;
    try {
        std::vector<uint8_t> file_blob;
        const uint8_t* blob = mgpu_ldpc_blob;
        size_t blob_size = mgpu_ldpc_blob_size;
        if (const char* p = std::getenv("MERCURY_LDPC_TABLES")) {
            std::ifstream f(p, std::ios::binary);
            if (!f) throw std::runtime_error(std::string("cannot open ") + p);
            file_blob.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
            blob = file_blob.data();
            blob_size = file_blob.size();
        }
        c->tab = mgpu::build_mode_tables(cfg->cfg, cfg->mfsk_ctrl_mode, blob, blob_size, xp);
        plan = mgpu_detail::ctx_plan(c.get());
    } catch (const std::exception& e) {
        g_create_error = e.what();
        return MGPU_ERR_TABLES;
    }
    try {
        int ndev = 0;
        HIPCK(hipGetDeviceCount(&ndev));
        if (ndev < 1) throw HipError("no HIP device visible (the MI355X path has no CPU fallback)");
        HIPCK(hipSetDevice(cfg->device));
        c->numa_node = mgpu_detail::device_numa_node(cfg->device);      // where the context's page-locked staging lives (-1: anywhere)
        mgpu_detail::ctx_upload(c.get(), plan);
    } catch (const std::exception& e) {
        g_create_error = e.what();
        return MGPU_ERR_DEVICE;
    }
    *out = c.release();
    return MGPU_OK;
}

void mgpu_destroy(mgpu_ctx* c) {
    if (!c) return;
    const int device = c->cfg.device;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device && hipSetDevice(device) != hipSuccess) prev = -1;   // no device: nothing was allocated
    (void)hipDeviceSynchronize();         // nothing queued on the context's streams still runs while its members are released (ctx.hpp)
    delete c;
    if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
}

void* mgpu_alloc_host(size_t bytes) {
    void* p = nullptr;
    return hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}

int mgpu_device_props_get(int device, mgpu_device_props* out) {
    if (!out) return MGPU_ERR_ARG;
    std::memset(out, 0, sizeof(*out));
    out->numa_node = -1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return MGPU_ERR_DEVICE;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) return MGPU_ERR_DEVICE;
    out->compute_units = p.multiProcessorCount;
    out->clock_khz = p.clockRate;
    out->memory_clock_khz = p.memoryClockRate;
    out->lds_bytes_per_cu = int(p.maxSharedMemoryPerMultiProcessor);
    out->wavefront_size = p.warpSize;
    out->hbm_bytes = p.totalGlobalMem;
    std::snprintf(out->name, sizeof(out->name), "%s", p.name);
    std::snprintf(out->gcn_arch, sizeof(out->gcn_arch), "%s", p.gcnArchName);
    if (hipDeviceGetPCIBusId(out->pci_bus_id, int(sizeof(out->pci_bus_id)), device) != hipSuccess) out->pci_bus_id[0] = 0;
    out->numa_node = mgpu_host_numa_node_of_pci(out->pci_bus_id);
    return MGPU_OK;
}

void* mgpu_alloc_host_near(int device, size_t bytes) {
    void* p = nullptr;
    return mgpu_detail::host_alloc_on_node(&p, bytes ? bytes : 16, mgpu_detail::device_numa_node(device)) == hipSuccess ? p : nullptr;
}
void mgpu_free_host(void* p) { if (p) (void)hipHostFree(p); }

const char* mgpu_last_error(mgpu_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

static void fill_info(const mgpu::ModeTables& t, mgpu_info* i) {
    i->cfg = t.cfg; i->M = t.M; i->bits_per_symbol = t.bps; i->K = t.K; i->P = t.P; i->N = t.N;
    i->Nsymb = t.Nsymb; i->Nc = t.Nc; i->Nfft = t.Nfft; i->Ngi = t.Ngi; i->Nofdm = t.Nofdm;
    i->nData = t.nData; i->nBits = t.nBits; i->nPilots = t.nPilots; i->nVirtual = t.nVirtual; i->nReal = t.nReal;
    i->bit_blk = t.bit_blk; i->tf_blk = t.tf_blk; i->preamble_nsymb = t.preamble;
    i->estimator = t.estimator; i->amp_restore = t.amp_restore; i->ls_window = t.lsw;
    i->Cwidth = t.graph.Cwidth; i->Vwidth = t.graph.Vwidth; i->E = t.graph.E;
    i->payload_bytes = t.payload_bytes; i->payload_stride = t.payload_stride; i->frame_samples = t.frame_samples;
    i->mfsk_M = t.mfsk_M; i->mfsk_nStreams = t.mfsk_nstreams; i->active_nsymb = t.active_nsymb; i->active_nbits = t.active_nbits;
}

int mgpu_get_info(mgpu_ctx* c, mgpu_info* i) {
    if (!c || !i) return MGPU_ERR_ARG;
    fill_info(c->tab, i);
    return MGPU_OK;
}

// load_configuration's mode row + derived sizes (telecom_system.cc:2487-3025, :1818-1826, :2910-2911) without a device: the same table builder
// mgpu_create runs, so the CPU test suite can hold it against the reference's printed values (tests/golden/survey_mode_table.json)
int mgpu_host_mode_info(int cfg, int mfsk_ctrl_mode, mgpu_info* i) {
    if (!i) return MGPU_ERR_ARG;
    try {
        const mgpu::ModeTables m = mgpu::build_mode_tables(cfg, mfsk_ctrl_mode, mgpu_ldpc_blob, mgpu_ldpc_blob_size);
        fill_info(m, i);
        return MGPU_OK;
    } catch (const std::exception& e) { g_create_error = e.what(); return MGPU_ERR_ARG; }
}

// the fp32 decoders' bank-aware placement, as modelled on the host (tables.cpp): LDS cycles per 32-lane gather group, 1.0 = conflict-free;
// out[0] the check pass's posterior reads, out[1] the variable update's message reads, out[2] bins, out[3] slots in use / slots
int mgpu_host_layout_stats(int cfg, double out[4]) {
    if (!out) return MGPU_ERR_ARG;
    try {
        const mgpu::ModeTables m = mgpu::build_mode_tables(cfg, 0, mgpu_ldpc_blob, mgpu_ldpc_blob_size);
        out[0] = m.graph.bank_model[0]; out[1] = m.graph.bank_model[1];
        out[2] = m.graph.Sg / 64; out[3] = m.graph.Sg ? double(m.graph.E) / m.graph.Sg : 0;
        return MGPU_OK;
    } catch (const std::exception& e) { g_create_error = e.what(); return MGPU_ERR_ARG; }
}

// ---- host-side pieces of the library, callable without a GPU (the CPU test suite checks them against the oracle) ----------------
int mgpu_host_select_peak(const double* cand_vals, int ncand, int step, int size, int location_to_return, int nTrials_max, int* delay,
                          double* correlation) {
    if (!cand_vals || !delay || ncand < 0 || step < 1 || size < 1 || nTrials_max < 1 || nTrials_max > size) return MGPU_ERR_ARG;
    double corr = 0;
    select_peak(cand_vals, ncand, step, size, location_to_return, nTrials_max, delay, &corr);
    if (correlation) *correlation = corr;
    return MGPU_OK;
}

int mgpu_host_fir_taps(int which, double carrier_hz, double* taps, int* ntaps) {
    if (!taps || !ntaps || which < 0 || which > 3) return MGPU_ERR_ARG;
    try {
        std::vector<double> t;
        if (which >= 2) t = mgpu::design_tx_fir(which - 2, carrier_hz);
        else {
            const mgpu::ModeTables m = mgpu::build_mode_tables(8, 0, mgpu_ldpc_blob, mgpu_ldpc_blob_size);
            t = which ? m.fir_data : m.fir_time_sync;
        }
        std::copy(t.begin(), t.end(), taps);
        *ntaps = int(t.size());
        return MGPU_OK;
    } catch (const std::exception&) { return MGPU_ERR_ARG; }
}

int mgpu_host_preamble_carriers(int cfg, double* carriers_c128, int* n_symbols) {
    if (!carriers_c128 || !n_symbols) return MGPU_ERR_ARG;
    try {
        const mgpu::ModeTables m = mgpu::build_mode_tables(cfg, 0, mgpu_ldpc_blob, mgpu_ldpc_blob_size);
        std::memcpy(carriers_c128, m.preamble_carriers.data(), m.preamble_carriers.size() * 16);
        *n_symbols = m.preamble;
        return MGPU_OK;
    } catch (const std::exception&) { return MGPU_ERR_ARG; }
}

}  // extern "C"

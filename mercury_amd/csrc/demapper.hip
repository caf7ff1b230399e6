// The channel-aware demapper (include/mercury_demapper.h): the context's setting, which selects the front-end's CSI form in launch.hip's
// front-end core, and the host twin of that form's pilot and demapping passes. The kernel is frontend.hip's.
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>

#include "ctx.hpp"
#include "fe_math.h"

extern "C" {

int mgpu_set_demapper(mgpu_ctx* c, int demapper) {
    if (!c) return MGPU_ERR_ARG;
    if (demapper != MGPU_DEMAP_MAXLOG && demapper != MGPU_DEMAP_CSI) {
        c->err = "demapper must be MGPU_DEMAP_MAXLOG or MGPU_DEMAP_CSI";
        return MGPU_ERR_ARG;
    }
    const auto& t = c->tab;
    if (t.mfsk_M > 0) {
        if (demapper == MGPU_DEMAP_MAXLOG) return MGPU_OK;
        c->err = "the channel-aware demapper needs an OFDM mode (the MFSK modes have no channel estimate)";
        return MGPU_ERR_UNSUPPORTED;
    }
    Demapper& D = c->dmp;
    const size_t lds = mgpu_frontend_csi_lds_bytes(c->dev.G, c->dev.nPilots, c->dev.nBits, c->fe_threads);
    if (demapper == MGPU_DEMAP_CSI && lds > size_t(160) * 1024) {
        c->err = "frame geometry too large for the LDS carve of the channel-aware demapper's front-end";
        return MGPU_ERR_TABLES;
    }
    return guard(c, [&] {
        HIPCK(hipStreamSynchronize(c->stream));
        if (demapper == MGPU_DEMAP_CSI && !D.d_sym_data) {
            // where the front-end keeps |h|^2 of the cell a demapped symbol comes from: the cell's de-framed position
            std::vector<int> data_of_cell(size_t(c->dev.G), -1);
            for (int i = 0; i < t.nData; ++i) data_of_cell[t.data_cell[i]] = i;
            std::vector<uint16_t> sym_data(size_t(t.nData));
            for (int k = 0; k < t.nData; ++k) {
                const int i = data_of_cell[t.sym_src[k]];
                if (i < 0) throw std::runtime_error("a demapped symbol comes from a cell that is no data cell");
                sym_data[size_t(k)] = uint16_t(i);
            }
            DevArray<uint16_t> d = upload(sym_data);
            HIPCK(hipFuncSetAttribute(reinterpret_cast<const void*>(fe_csi_kernel(c->fe_threads)), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
            D.d_sym_data = std::move(d);
            D.arg.sym_data = D.d_sym_data;
            D.lds = lds;
            // the context's own square window as the rectangular form takes it
            D.own = MgpuLsRect{};
            D.own.weight = c->dev.ls_weight;
            D.own.hw_f = D.own.hw_t = t.lsw / 2;
            D.own.lattice = c->dev.regular_lattice;
        }
        D.mode = demapper;
    });
}

int mgpu_get_demapper(mgpu_ctx* c, int* demapper) {
    if (!c || !demapper) return MGPU_ERR_ARG;
    *demapper = c->dmp.mode;
    return MGPU_OK;
}

// What the twin needs of a mode's tables, kept for the last geometry asked for (a sweep over frames builds the tables once).
namespace {
struct DemapGeometry {
    int cfg = -1;
    mgpu::ExplicitParams xp;
    bool ofdm = false;
    int G = 0, nData = 0, nPilots = 0, M = 0, bps = 0;
    double pilot_boost = 0;
    std::vector<uint16_t> pilot_cell, sym_src;
    std::vector<double> pilot_val;
    std::vector<mgpu::Cplx> constellation;
};
std::mutex demap_mutex;
std::shared_ptr<const DemapGeometry> demap_last;

std::shared_ptr<const DemapGeometry> demap_geometry(int cfg, const mgpu::ExplicitParams& xp) {
    std::lock_guard<std::mutex> lock(demap_mutex);
    const auto same = [&](const DemapGeometry& g) {
        return g.cfg == cfg && g.xp.pilot_boost == xp.pilot_boost && g.xp.ls_window == xp.ls_window && g.xp.pilot_seed == xp.pilot_seed &&
               g.xp.scrambler_seed == xp.scrambler_seed && g.xp.preamble_seed == xp.preamble_seed && g.xp.Nsymb == xp.Nsymb && g.xp.Dy == xp.Dy;
    };
    if (demap_last && same(*demap_last)) return demap_last;
    const mgpu::ModeTables t = mgpu::build_mode_tables(cfg, 0, mgpu_ldpc_blob, mgpu_ldpc_blob_size, xp);
    auto g = std::make_shared<DemapGeometry>();
    g->cfg = cfg; g->xp = xp;
    g->ofdm = t.mfsk_M == 0;
    g->G = t.Nsymb * t.Nc; g->nData = t.nData; g->nPilots = t.nPilots; g->M = t.M; g->bps = t.bps;
    g->pilot_boost = t.pilot_boost;
    for (int i = 0; i < g->G && g->ofdm; ++i) if (t.cell_type[i]) g->pilot_cell.push_back(uint16_t(i));
    g->sym_src = t.sym_src; g->pilot_val = t.pilot_val; g->constellation = t.constellation;
    demap_last = g;
    return g;
}
}  // namespace

int mgpu_host_demap_csi(int cfg, const mgpu_explicit_params* p, const double* grid, const double* H, float* llr, double* sigma2_out) {
    if (!grid || !H || !llr) return MGPU_ERR_ARG;
    mgpu::ExplicitParams xp;
    std::string err;
    int rc = MGPU_OK;
    if (!explicit_params_from(p, xp, err, &rc)) return rc;
    try {
        const std::shared_ptr<const DemapGeometry> geometry = demap_geometry(cfg, xp);
        const DemapGeometry& t = *geometry;
        if (!t.ofdm) return MGPU_ERR_UNSUPPORTED;
        const auto cell = [](const double* a, int c) { return c2{a[2 * c], a[2 * c + 1]}; };
        // sigma2: the pilots' terms in pilot order, one sum (frontend.hip: red3, serial_sum)
        double var = 0;
        for (size_t q = 0; q < t.pilot_cell.size(); ++q) {
            const int c = t.pilot_cell[q];
            const c2 g = cell(grid, c), h = cell(H, c);
            const double x = t.pilot_val[size_t(c)] < 0 ? -t.pilot_boost : t.pilot_boost;
            const double dr = g.re - h.re * x, di = g.im - h.im * x;
            var += dr * dr + di * di;
        }
        var /= double(t.nPilots);
        if (sigma2_out) *sigma2_out = var;
        const float inv = 1 / float(var);
        const int bps = t.bps;
        for (int k = 0; k < t.nData; ++k) {
            const int c = t.sym_src[size_t(k)];
            const c2 h = cell(H, c);
            const c2 s = cdiv(cell(grid, c), h);
            const float scale = inv * float(h.re * h.re + h.im * h.im);
            float d0[8], d1[8];
            for (int b = 0; b < bps; ++b) { d0[b] = INFINITY; d1[b] = INFINITY; }
            for (int j = 0; j < t.M; ++j) {
                const double dr = s.re - t.constellation[size_t(j)].re, di = s.im - t.constellation[size_t(j)].im;
                const float D = float(dr * dr + di * di);
                for (int b = 0; b < bps; ++b) {
                    if ((j >> b) & 1) d1[b] = std::fmin(d1[b], D);
                    else d0[b] = std::fmin(d0[b], D);
                }
            }
            for (int b = 0; b < bps; ++b) llr[k * bps + (bps - 1 - b)] = scale * (d1[b] - d0[b]);
        }
        return MGPU_OK;
    } catch (const std::exception&) { return MGPU_ERR_ARG; }
}

}  // extern "C"

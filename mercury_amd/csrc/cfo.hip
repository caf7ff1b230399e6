// Pilot-aided residual carrier-offset correction (include/mercury_cfo.h): the context's setting, which selects the front-end's CFO forms in
// launch.hip's front-end core, the stage's tables, and the host twin. The kernel is frontend.hip's; the twin's arithmetic is cfo_rule.cpp's.
#include <cstring>
#include <memory>

#include "ctx.hpp"

extern "C" void mgpu_internal_cfo_rule(const double* grid, double* out, int Ns, int Nc, int Dy, const int8_t* sign, const uint16_t* pair,
                                       const uint16_t* first, double* step_out);

namespace {

// Per carrier, its pilots in ascending symbol order; every consecutive pair whose symbol distance is Dy, carrier after carrier.
struct CfoChains {
    std::vector<uint16_t> pair, first;
    std::vector<int8_t> sign;           // [G] 0 data, +1 / -1 pilot
};
CfoChains cfo_chains(const mgpu::ModeTables& t) {
    CfoChains k;
    const int G = t.Nsymb * t.Nc, Dy = t.xp.Dy;
    if (G > 65535) throw std::runtime_error("frame geometry too large for the carrier-offset stage's tables");
    k.sign.resize(size_t(G));
    for (int i = 0; i < G; ++i) k.sign[size_t(i)] = t.cell_type[size_t(i)] ? (t.pilot_val[size_t(i)] < 0 ? int8_t(-1) : int8_t(1)) : int8_t(0);
    for (int c = 0; c < t.Nc; ++c) {
        k.first.push_back(uint16_t(k.pair.size() / 2));
        int last = -1;
        for (int s = 0; s < t.Nsymb; ++s) {
            if (!t.cell_type[size_t(s * t.Nc + c)]) continue;
            if (last >= 0 && s - last == Dy) { k.pair.push_back(uint16_t(last * t.Nc + c)); k.pair.push_back(uint16_t(s * t.Nc + c)); }
            last = s;
        }
    }
    k.first.push_back(uint16_t(k.pair.size() / 2));
    return k;
}

}  // namespace

extern "C" {

int mgpu_set_cfo(mgpu_ctx* c, int cfo) {
    if (!c) return MGPU_ERR_ARG;
    if (cfo != MGPU_CFO_OFF && cfo != MGPU_CFO_PILOTS) return refuse(c, MGPU_ERR_ARG, "cfo must be MGPU_CFO_OFF or MGPU_CFO_PILOTS");
    const auto& t = c->tab;
    if (t.mfsk_M > 0) {
        if (cfo == MGPU_CFO_OFF) return MGPU_OK;
        return refuse(c, MGPU_ERR_UNSUPPORTED, "the pilot-aided carrier-offset correction needs an OFDM mode (the MFSK modes have no pilots)");
    }
    Cfo& K = c->cfo;
    return guard(c, [&] {
        // the stage's scratch - Nc carrier sums at the head of the work area, a phasor per symbol from entry 64 on - lies inside the
        // four FFT work areas every carve has (frontend.hip)
        need(t.Nc <= 64 && t.Nsymb <= 4 * 256 - 64, "frame geometry outside the carrier-offset stage's scratch");
        HIPCK(hipStreamSynchronize(c->stream));
        if (cfo == MGPU_CFO_PILOTS) {
            if (!K.d_pair) {
                const CfoChains k = cfo_chains(t);
                DevArray<uint16_t> d_pair = upload(k.pair), d_first = upload(k.first);
                DevArray<double> d_step(size_t(c->max_batch > 0 ? c->max_batch : 1) * sizeof(double));
                K.d_pair = std::move(d_pair); K.d_first = std::move(d_first); K.d_step = std::move(d_step);
                K.arg = MgpuCfo{};
                K.arg.pair = K.d_pair; K.arg.first = K.d_first; K.arg.Dy = t.xp.Dy;
            }
            frontend_raise_lds_limits(c);
            HIPCK(hipMemset(K.d_step.p, 0, size_t(c->max_batch > 0 ? c->max_batch : 1) * sizeof(double)));
        }
        K.mode = cfo;
    });
}

int mgpu_get_cfo(mgpu_ctx* c, int* cfo) {
    if (!c || !cfo) return MGPU_ERR_ARG;
    *cfo = c->cfo.mode;
    return MGPU_OK;
}

int mgpu_get_cfo_steps(mgpu_ctx* c, int F, double* step) {
    if (!c || !step || F < 0) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(F <= c->max_batch, "bad argument (F must be <= max_batch)");
        read_rows(c, c->cfo.d_step, 1, 0, F, step, "no span has run with MGPU_CFO_PILOTS on this context");
    });
}

// What the twin needs of a mode's tables (geometry_cache.hpp)
namespace {
struct CfoGeometry {
    bool ofdm = false;
    int Ns = 0, Nc = 0, Dy = 0;
    CfoChains chains;
};
}  // namespace

int mgpu_host_cfo_pilots(int cfg, const mgpu_explicit_params* p, const double* grid_in, double* grid_out, double* step_out) {
    if (!grid_in || !grid_out) return MGPU_ERR_ARG;
    return host_twin(p, [&](const mgpu::ExplicitParams& xp) -> int {
        const auto geometry = cached_geometry<CfoGeometry>(cfg, xp, [](const mgpu::ModeTables& t) {
            CfoGeometry g;
            g.ofdm = t.mfsk_M == 0;
            g.Ns = t.Nsymb; g.Nc = t.Nc; g.Dy = t.xp.Dy;
            if (g.ofdm) g.chains = cfo_chains(t);
            return g;
        });
        const CfoGeometry& g = *geometry;
        if (!g.ofdm) return MGPU_ERR_UNSUPPORTED;
        mgpu_internal_cfo_rule(grid_in, grid_out, g.Ns, g.Nc, g.Dy, g.chains.sign.data(), g.chains.pair.data(), g.chains.first.data(), step_out);
        return MGPU_OK;
    });
}

}  // extern "C"

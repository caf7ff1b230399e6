// The channel-aware demapper and its noise-map form (include/mercury_demapper.h): the context's setting, which selects the front-end's CSI
// or NMAP forms in launch.hip's front-end core, the noise map's tables, and the host twins of those forms' pilot and demapping passes. The
// kernel is frontend.hip's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "ctx.hpp"
#include "fe_math.h"

namespace {

// The noise map's lists (ls_rect.h MgpuNmap): every carrier's pilots as indices into pilot order, ascending symbols, carrier after carrier;
// a carrier's first entry; a symbol's first pilot. One construction for the kernel's tables and the twin.
struct NmapLists { std::vector<uint16_t> car_list, car_first, sym_first; };
NmapLists nmap_lists(const std::vector<uint8_t>& cell_type, int Nsymb, int Nc) {
    NmapLists L;
    std::vector<int> index(size_t(Nsymb) * Nc, -1);
    int p = 0;
    for (int s = 0; s < Nsymb; ++s) {
        L.sym_first.push_back(uint16_t(p));
        for (int c = 0; c < Nc; ++c) if (cell_type[size_t(s) * Nc + c]) index[size_t(s) * Nc + c] = p++;
    }
    L.sym_first.push_back(uint16_t(p));
    if (p > 65535) throw std::runtime_error("frame geometry too large for the noise map's tables");
    for (int c = 0; c < Nc; ++c) {
        L.car_first.push_back(uint16_t(L.car_list.size()));
        for (int s = 0; s < Nsymb; ++s) if (index[size_t(s) * Nc + c] >= 0) L.car_list.push_back(uint16_t(index[size_t(s) * Nc + c]));
    }
    L.car_first.push_back(uint16_t(L.car_list.size()));
    return L;
}

const mgpu_demapper_params kNmapDefaults{2.0, 1};
bool nmap_params_ok(const mgpu_demapper_params& q) { return q.dead_band >= 1 && q.smooth >= 0 && q.smooth <= 4; }   // (NaN fails the comparison)

}  // namespace

extern "C" {

int mgpu_set_demapper_ex(mgpu_ctx* c, int demapper, const mgpu_demapper_params* params, size_t params_size) {
    if (!c) return MGPU_ERR_ARG;
    if (params_size != sizeof(mgpu_demapper_params)) return refuse(c, MGPU_ERR_ARG, "demapper: params_size is not this library's sizeof(mgpu_demapper_params)");
    if (demapper != MGPU_DEMAP_MAXLOG && demapper != MGPU_DEMAP_CSI && demapper != MGPU_DEMAP_NMAP) return refuse(c, MGPU_ERR_ARG, "demapper must be MGPU_DEMAP_MAXLOG, MGPU_DEMAP_CSI or MGPU_DEMAP_NMAP");
    const mgpu_demapper_params q = params ? *params : kNmapDefaults;
    if (demapper == MGPU_DEMAP_NMAP && !nmap_params_ok(q)) return refuse(c, MGPU_ERR_ARG, "the noise-map demapper takes a dead_band >= 1 (+Inf included) and a smooth of 0..4");
    const auto& t = c->tab;
    if (t.mfsk_M > 0) {
        if (demapper == MGPU_DEMAP_MAXLOG) return MGPU_OK;
        return refuse(c, MGPU_ERR_UNSUPPORTED, "the channel-aware demapper needs an OFDM mode (the MFSK modes have no channel estimate)");
    }
    if (demapper == MGPU_DEMAP_NMAP && t.estimator != MGPU_EST_LS) return refuse(c, MGPU_ERR_UNSUPPORTED, "the noise-map demapper needs the LS estimator (a zero-forcing estimate passes through its own pilots: no residuals)");
    Demapper& D = c->dmp;
    const size_t lds = mgpu_frontend_csi_lds_bytes(c->dev.G, c->dev.nPilots, c->dev.nBits, c->fe_threads);
    const size_t nmap_lds = mgpu_frontend_nmap_lds_bytes(c->dev.G, c->dev.nPilots, c->dev.nBits, c->fe_threads);
    if ((demapper == MGPU_DEMAP_CSI && lds > size_t(160) * 1024) || (demapper == MGPU_DEMAP_NMAP && nmap_lds > size_t(160) * 1024)) return refuse(c, MGPU_ERR_TABLES, "frame geometry too large for the LDS carve of the channel-aware demapper's front-end");
    // the noise map's sums and factors have a lane each: carriers on one wavefront, symbols on the five behind it (frontend.hip)
    if (demapper == MGPU_DEMAP_NMAP && (t.Nc != 50 || t.Nsymb > 255 || c->dev.G != t.Nsymb * t.Nc)) return refuse(c, MGPU_ERR_TABLES, "frame geometry outside the noise map's lane assignment");
    return guard(c, [&] {
        HIPCK(hipStreamSynchronize(c->stream));
        if (demapper != MGPU_DEMAP_MAXLOG && !D.d_sym_data) {
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
            D.d_sym_data = std::move(d);
            D.arg.sym_data = D.d_sym_data;
        }
        if (demapper != MGPU_DEMAP_MAXLOG) frontend_raise_lds_limits(c);
        if (demapper == MGPU_DEMAP_NMAP) {
            const size_t rows = size_t(c->max_batch > 0 ? c->max_batch : 1);
            if (!D.d_nmap_idx) {
                const NmapLists L = nmap_lists(t.cell_type, t.Nsymb, t.Nc);
                need(int(L.car_list.size()) == t.nPilots, "the noise map's pilot lists do not cover the pilots");
                std::vector<uint16_t> idx(L.car_list);
                const size_t at_car = idx.size();
                idx.insert(idx.end(), L.car_first.begin(), L.car_first.end());
                const size_t at_sym = idx.size();
                idx.insert(idx.end(), L.sym_first.begin(), L.sym_first.end());
                DevArray<uint16_t> d_idx = upload(idx);
                DevArray<double> d_fc(rows * size_t(t.Nc) * sizeof(double)), d_fs(rows * size_t(t.Nsymb) * sizeof(double));
                D.d_nmap_idx = std::move(d_idx); D.d_fc = std::move(d_fc); D.d_fs = std::move(d_fs);
                D.nmap = MgpuNmap{};
                D.nmap.car_list = D.d_nmap_idx;
                D.nmap.car_first = D.d_nmap_idx + at_car;
                D.nmap.sym_first = D.d_nmap_idx + at_sym;
            }
            HIPCK(hipMemset(D.d_fc.p, 0, rows * size_t(t.Nc) * sizeof(double)));
            HIPCK(hipMemset(D.d_fs.p, 0, rows * size_t(t.Nsymb) * sizeof(double)));
            D.nmap.band = q.dead_band;
            D.nmap.smooth = q.smooth;
            D.params = q;
        }
        D.mode = demapper;
    });
}

int mgpu_set_demapper(mgpu_ctx* c, int demapper) { return mgpu_set_demapper_ex(c, demapper, nullptr, sizeof(mgpu_demapper_params)); }

int mgpu_get_demapper(mgpu_ctx* c, int* demapper) {
    if (!c || !demapper) return MGPU_ERR_ARG;
    *demapper = c->dmp.mode;
    return MGPU_OK;
}

int mgpu_get_demapper_ex(mgpu_ctx* c, int* demapper, mgpu_demapper_params* params, size_t params_size) {
    if (!c || !demapper || !params || params_size != sizeof(mgpu_demapper_params)) return MGPU_ERR_ARG;
    *demapper = c->dmp.mode;
    *params = c->dmp.params;
    return MGPU_OK;
}

int mgpu_get_noise_map(mgpu_ctx* c, int first, int count, double* fc, double* fs) {
    if (!c || first < 0 || count < 0) return MGPU_ERR_ARG;
    return guard(c, [&] {
        read_rows(c, c->dmp.d_fc, size_t(c->tab.Nc), first, count, fc, "MGPU_DEMAP_NMAP was never set on this context");
        read_rows(c, c->dmp.d_fs, size_t(c->tab.Nsymb), first, count, fs, "MGPU_DEMAP_NMAP was never set on this context");
    });
}

}  // extern "C"

// What the twins need of a mode's tables (geometry_cache.hpp)
namespace {
struct DemapGeometry {
    bool ofdm = false;
    int G = 0, nData = 0, nPilots = 0, M = 0, bps = 0, Nsymb = 0, Nc = 0;
    bool ls = false;                                // the LS estimator (the noise map refuses zero-forcing)
    NmapLists nmap;
    double pilot_boost = 0;
    std::vector<uint16_t> pilot_cell, sym_src;
    std::vector<double> pilot_val;
    std::vector<mgpu::Cplx> constellation;
};

std::shared_ptr<const DemapGeometry> demap_geometry(int cfg, const mgpu::ExplicitParams& xp) {
    return cached_geometry<DemapGeometry>(cfg, xp, [](const mgpu::ModeTables& t) {
        DemapGeometry g;
        g.ofdm = t.mfsk_M == 0;
        g.G = t.Nsymb * t.Nc; g.nData = t.nData; g.nPilots = t.nPilots; g.M = t.M; g.bps = t.bps;
        g.pilot_boost = t.pilot_boost;
        g.Nsymb = t.Nsymb; g.Nc = t.Nc; g.ls = t.estimator == MGPU_EST_LS;
        if (g.ofdm) g.nmap = nmap_lists(t.cell_type, t.Nsymb, t.Nc);
        for (int i = 0; i < g.G && g.ofdm; ++i) if (t.cell_type[i]) g.pilot_cell.push_back(uint16_t(i));
        g.sym_src = t.sym_src; g.pilot_val = t.pilot_val; g.constellation = t.constellation;
        return g;
    });
}
}  // namespace

extern "C" {

int mgpu_host_demap_csi(int cfg, const mgpu_explicit_params* p, const double* grid, const double* H, float* llr, double* sigma2_out) {
    if (!grid || !H || !llr) return MGPU_ERR_ARG;
    return host_twin(p, [&](const mgpu::ExplicitParams& xp) -> int {
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
    });
}

int mgpu_host_demap_nmap(int cfg, const mgpu_explicit_params* p, const double* grid, const double* H, const mgpu_demapper_params* params, size_t params_size,
                         float* llr, double* sigma2_out, double* fc_out, double* fs_out) {
    if (!grid || !H || !llr || params_size != sizeof(mgpu_demapper_params)) return MGPU_ERR_ARG;
    const mgpu_demapper_params prm = params ? *params : kNmapDefaults;
    if (!nmap_params_ok(prm)) return MGPU_ERR_ARG;
    return host_twin(p, [&](const mgpu::ExplicitParams& xp) -> int {
        const std::shared_ptr<const DemapGeometry> geometry = demap_geometry(cfg, xp);
        const DemapGeometry& t = *geometry;
        if (!t.ofdm || !t.ls) return MGPU_ERR_UNSUPPORTED;
        const int Nc = t.Nc, Ns = t.Nsymb;
        const NmapLists& L = t.nmap;
        const auto cell = [](const double* a, int c) { return c2{a[2 * c], a[2 * c + 1]}; };
        // the pilots' terms in pilot order and sigma2, as mgpu_host_demap_csi (frontend.hip: red3, serial_sum)
        std::vector<double> r(t.pilot_cell.size(), 0.0);
        double var = 0;
        for (size_t q = 0; q < t.pilot_cell.size(); ++q) {
            const int c = t.pilot_cell[q];
            const c2 g = cell(grid, c), h = cell(H, c);
            const double x = t.pilot_val[size_t(c)] < 0 ? -t.pilot_boost : t.pilot_boost;
            const double dr = g.re - h.re * x, di = g.im - h.im * x;
            r[q] = dr * dr + di * di;
            var += r[q];
        }
        var /= double(t.nPilots);
        const double sigma2 = var, band = prm.dead_band;
        if (sigma2_out) *sigma2_out = sigma2;
        const bool usable = sigma2 != 0 && std::fabs(sigma2) < INFINITY;
        const auto banded = [&](double v, int n) {
            const double fr = v / sigma2;
            return (usable && n > 0 && (fr > band || fr * band < 1)) ? fr : 1.0;
        };
        // carrier sums in ascending symbols, their smoothed means, the carrier scales (frontend.hip: nm_S, nm_a)
        std::vector<double> S(size_t(Nc), 0.0);
        for (int c = 0; c < Nc; ++c) {
            double acc = 0;
            for (int q = L.car_first[size_t(c)]; q < L.car_first[size_t(c) + 1]; ++q) acc += r[L.car_list[size_t(q)]];
            S[size_t(c)] = acc;
        }
        std::vector<float> a(size_t(Nc), 0.0f), b(size_t(Ns), 0.0f);
        for (int c = 0; c < Nc; ++c) {
            const int lo = std::max(c - prm.smooth, 0), hi = std::min(c + prm.smooth, Nc - 1);
            double sum = 0;
            for (int k = lo; k <= hi; ++k) sum += S[size_t(k)];
            const int n = int(L.car_first[size_t(hi) + 1]) - int(L.car_first[size_t(lo)]);
            const double fc = banded(sum / double(n), n);
            a[size_t(c)] = 1.0f / float(sigma2 * fc);
            if (fc_out) fc_out[c] = fc;
        }
        // symbol sums in ascending carriers, their means, the symbol scales (nm_U, nm_b)
        for (int s = 0; s < Ns; ++s) {
            double acc = 0;
            for (int q = L.sym_first[size_t(s)]; q < L.sym_first[size_t(s) + 1]; ++q) acc += r[size_t(q)];
            const int n = int(L.sym_first[size_t(s) + 1]) - int(L.sym_first[size_t(s)]);
            const double fs = banded(acc / double(n), n);
            b[size_t(s)] = 1.0f / float(fs);
            if (fs_out) fs_out[s] = fs;
        }
        const int bps = t.bps;
        for (int k = 0; k < t.nData; ++k) {
            const int c = t.sym_src[size_t(k)], sy = c / Nc;
            const c2 h = cell(H, c);
            const c2 s = cdiv(cell(grid, c), h);
            const float scale = (a[size_t(c - sy * Nc)] * b[size_t(sy)]) * float(h.re * h.re + h.im * h.im);
            float d0[8], d1[8];
            for (int bb = 0; bb < bps; ++bb) { d0[bb] = INFINITY; d1[bb] = INFINITY; }
            for (int j = 0; j < t.M; ++j) {
                const double dr = s.re - t.constellation[size_t(j)].re, di = s.im - t.constellation[size_t(j)].im;
                const float D = float(dr * dr + di * di);
                for (int bb = 0; bb < bps; ++bb) {
                    if ((j >> bb) & 1) d1[bb] = std::fmin(d1[bb], D);
                    else d0[bb] = std::fmin(d0[bb], D);
                }
            }
            for (int bb = 0; bb < bps; ++bb) llr[k * bps + (bps - 1 - bb)] = scale * (d1[bb] - d0[bb]);
        }
        return MGPU_OK;
    });
}

}  // extern "C"

// Rational resampler, host side (include/ext/mercury_resampler.h): the rates' ratio, the prototype design and the normative twin.
// Everything here is plain double arithmetic with the host's libm; the device gets the prototype this file makes, so the libm's version
// cannot make the device and the twin differ. fma() stays a libm call (baseline x86-64, no contraction: mercury_amd/build.py).
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "chan_tables.hpp"
#include "resamp_tables.hpp"
#include "sample_formats.h"
#include "../../include/mercury_gpu.h"

namespace mgpu_resamp_detail {

bool ratio(int fin, int fout, Ratio* r) {
    if (fin < 1 || fout < 1) return false;
    const int g = std::gcd(fin, fout);
    r->L = fout / g;
    r->M = fin / g;
    return r->L <= MGPU_RESAMP_MAX_L && r->M <= MGPU_RESAMP_MAX_M && r->M <= MGPU_RESAMP_MAX_RATIO * r->L;
}

const char* config_error(const mgpu_resamp_config* k) {
    if (!k) return "no configuration";
    if (k->struct_size != int(sizeof(mgpu_resamp_config))) return "mgpu_resamp_config.struct_size is not sizeof(mgpu_resamp_config)";
    Ratio r;
    if (!ratio(k->fin, k->fout, &r)) return "rates must be >= 1 with L <= 640, M <= 640 and M <= 16 L";
    if (k->S < 1) return "S must be >= 1";
    if (k->components != 1 && k->components != 2) return "components must be 1 or 2";
    if (k->tp != 0 || k->taps) {
        if (k->tp < 2 || k->tp > MGPU_RESAMP_MAX_TP || (k->tp & 1)) return "tp must be even, 2..512";
    }
    if (k->taps) {
        if (k->ntaps != k->tp * r.L + 1) return "ntaps must be tp * L + 1";
        for (int i = 0; i < k->ntaps; ++i)
            if (!std::isfinite(k->taps[i])) return "taps must be finite";
    }
    // the kernel's 32-bit index arithmetic: (outputs of a call + 1) * M + L stays below 2^31
    if (k->max_in < 0 || (long long)k->max_in * r.L + 2LL * r.M + r.L >= (1LL << 31) || (long long)k->max_in * k->components > (1LL << 30))
        return "max_in * L must stay below 2^31";
    return nullptr;
}

namespace {

// the construction of mgpu_host_chan_design at rate fin * L, normalised to sum h = L
void design(int fin, const Ratio& r, int tp, double cutoff_hz, double atten_db, double* h) {
    const double R = double(fin) * r.L;
    mgpu_chan_detail::windowed_sinc(tp * r.L + 1, 2 * cutoff_hz / R, atten_db, r.L, h);
}

}  // namespace

std::vector<double> prototype(const mgpu_resamp_config* k, const Ratio& r) {
    if (k->taps) return std::vector<double>(k->taps, k->taps + k->ntaps);
    const int tp = config_tp(k, r);
    std::vector<double> h(size_t(tp) * r.L + 1);
    design(k->fin, r, tp, 0.45 * std::min(k->fin, k->fout), 60.0, h.data());
    return h;
}

}  // namespace mgpu_resamp_detail

using namespace mgpu_resamp_detail;

extern "C" {

int mgpu_host_resamp_design(int fin, int fout, int tp, double cutoff_hz, double atten_db, double* taps, int* ntaps) {
    Ratio r;
    if (!ntaps || !ratio(fin, fout, &r)) return MGPU_ERR_ARG;
    if (tp == 0) tp = default_tp(r);
    if (tp < 2 || tp > MGPU_RESAMP_MAX_TP || (tp & 1)) return MGPU_ERR_ARG;
    if (cutoff_hz == 0.0) cutoff_hz = 0.45 * std::min(fin, fout);
    if (atten_db == 0.0) atten_db = 60.0;
    if (!(cutoff_hz > 0) || !(cutoff_hz < 0.5 * double(fin) * r.L) || !(atten_db > 0) || !(atten_db <= 200)) return MGPU_ERR_ARG;
    *ntaps = tp * r.L + 1;
    if (taps) design(fin, r, tp, cutoff_hz, atten_db, taps);
    return MGPU_OK;
}

int mgpu_host_resamp_default_taps(int fin, int fout, double* taps, int* ntaps) {
    return mgpu_host_resamp_design(fin, fout, 0, 0.0, 0.0, taps, ntaps);
}

int mgpu_host_resamp_count(int fin, int fout, uint64_t m0, int n_in, int* n_out) {
    Ratio r;
    if (!n_out || !ratio(fin, fout, &r) || n_in < 0 || m0 > MGPU_RESAMP_MAX_POSITION || m0 + uint64_t(n_in) > MGPU_RESAMP_MAX_POSITION)
        return MGPU_ERR_ARG;
    const uint64_t n = out_position(m0 + uint64_t(n_in), r) - out_position(m0, r);
    if (n > uint64_t(INT32_MAX)) return MGPU_ERR_ARG;
    *n_out = int(n);
    return MGPU_OK;
}

int mgpu_host_resamp_process(const mgpu_resamp_config* k, const void* in, int format, int n_in, uint64_t position, double* out,
                             size_t out_stride, int* n_out) {
    const int e = k ? mgpu_fmt::element(k->components, format) : mgpu_fmt::kNone;
    if (config_error(k) || !in || !n_out || n_in < 1 || e == mgpu_fmt::kNone) return MGPU_ERR_ARG;
    int N = 0;
    if (mgpu_host_resamp_count(k->fin, k->fout, position, n_in, &N) != MGPU_OK || size_t(N) > out_stride || (N && !out)) return MGPU_ERR_ARG;
    Ratio r;
    ratio(k->fin, k->fout, &r);
    const std::vector<double> h = prototype(k, r);
    const int C = k->components, tp = int((h.size() - 1) / size_t(r.L));
    const long long L = r.L, M = r.M, m0 = (long long)position;
    const long long n0 = (long long)out_position(position, r);
    std::vector<double> x(size_t(n_in) * C);
    for (int s = 0; s < k->S; ++s) {
        for (size_t i = 0; i < x.size(); ++i) x[i] = mgpu_fmt::widen_at(e, in, size_t(s) * x.size() + i);
        for (int i = 0; i < N; ++i) {
            const long long q = (n0 + i) * M, b = q / L - m0, rho = q % L;      // b relative to the seek: zeros before it
            for (int comp = 0; comp < C; ++comp) {
                double acc = 0.0;
                for (int j = 0; j < tp; ++j) acc = std::fma(h[size_t(rho + j * L)], b - j >= 0 ? x[size_t(b - j) * C + comp] : 0.0, acc);
                if (rho == 0) acc = std::fma(h[size_t(tp) * L], b - tp >= 0 ? x[size_t(b - tp) * C + comp] : 0.0, acc);
                out[(size_t(s) * out_stride + size_t(i)) * C + comp] = acc;
            }
        }
    }
    *n_out = N;
    return MGPU_OK;
}

}  // extern "C"

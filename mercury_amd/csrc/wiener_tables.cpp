// Tables of the separable Wiener channel estimator (include/mercury_estimator.h: MGPU_RUNG_WIENER), in double on the host.
//
// With Dx = 1 and the pilots on diagonals every carrier that has pilots has one every Dy symbols and every symbol one every Dy carriers,
// so the pilots are filtered along time per carrier (real taps A) and then along frequency per symbol (complex taps B). The taps are the
// MMSE interpolator's for a channel whose Doppler spectrum is flat within +-doppler_hz and whose delay profile is flat within
// [tau_min, tau_max], evaluated at the pilots themselves and scaled to unit gain on that channel model.
#include <algorithm>
#include <cmath>
#include <complex>
#include <map>
#include <stdexcept>

#include "tables.hpp"

namespace mgpu {

namespace {

constexpr double kSampleRate = 12000.0, kSymbolSamples = 272.0, kNfft = 256.0;

double sinc(double x) { return x == 0.0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x); }

inline double magnitude(double v) { return std::fabs(v); }
inline double magnitude(const std::complex<double>& v) { return std::abs(v); }

// X with M X = R (n x n, row-major) by Gaussian elimination with partial pivoting; M and R are consumed
template <typename T>
std::vector<T> solve(std::vector<T> M, std::vector<T> R, int n) {
    for (int col = 0; col < n; ++col) {
        int piv = col;
        for (int r = col + 1; r < n; ++r)
            if (magnitude(M[size_t(r) * n + col]) > magnitude(M[size_t(piv) * n + col])) piv = r;
        if (!(magnitude(M[size_t(piv) * n + col]) > 0.0)) throw std::runtime_error("Wiener design: singular correlation matrix");
        if (piv != col)
            for (int k = 0; k < n; ++k) { std::swap(M[size_t(piv) * n + k], M[size_t(col) * n + k]); std::swap(R[size_t(piv) * n + k], R[size_t(col) * n + k]); }
        for (int r = col + 1; r < n; ++r) {
            const T f = M[size_t(r) * n + col] / M[size_t(col) * n + col];
            for (int k = col; k < n; ++k) M[size_t(r) * n + k] -= f * M[size_t(col) * n + k];
            for (int k = 0; k < n; ++k) R[size_t(r) * n + k] -= f * R[size_t(col) * n + k];
        }
    }
    for (int r = n - 1; r >= 0; --r)
        for (int k = 0; k < n; ++k) {
            T v = R[size_t(r) * n + k];
            for (int j = r + 1; j < n; ++j) v -= M[size_t(r) * n + j] * R[size_t(j) * n + k];
            R[size_t(r) * n + k] = v / M[size_t(r) * n + r];
        }
    return R;
}

}  // namespace

bool wiener_design_ok(const WienerDesign& d) {
    return std::isfinite(d.tau_min_us) && std::isfinite(d.tau_max_us) && std::isfinite(d.doppler_hz) && std::isfinite(d.snr_db) &&
           d.tau_max_us > d.tau_min_us && d.doppler_hz >= 0.0 && d.snr_db >= -20.0 && d.snr_db <= 40.0;
}

WienerTables build_wiener_tables(const std::vector<uint8_t>& cell_type, int Nsymb, int Nc, double pilot_boost, const WienerDesign& d) {
    if (!wiener_design_ok(d)) throw std::invalid_argument("Wiener design out of range");
    WienerTables w;
    const double tau0 = d.tau_min_us * kSampleRate / 1e6, tau1 = d.tau_max_us * kSampleRate / 1e6;     // delay bounds in baseband samples
    const double Ts = kSymbolSamples / kSampleRate;
    w.s2 = std::pow(10.0, -d.snr_db / 10.0) / (pilot_boost * pilot_boost);
    // a carrier's FFT bin relative to DC, which carries nothing (the zero padder's placement: build_mode_tables' preamble, tables.cpp)
    const auto bin = [&](int c) { return c < Nc / 2 ? c - Nc / 2 : c - Nc / 2 + 1; };

    w.col_pilots.assign(size_t(Nc), {});
    w.row_pilots.assign(size_t(Nsymb), {});
    std::vector<int> pilot_sym, pilot_car;
    for (int q = 0; q < Nsymb * Nc; ++q) {
        if (!cell_type[size_t(q)]) continue;
        const int p = int(pilot_sym.size());
        if (p > 0xffff) throw std::runtime_error("Wiener tables: more pilots than the 2-byte fields hold");
        pilot_sym.push_back(q / Nc); pilot_car.push_back(q % Nc);
        w.col_pilots[size_t(q % Nc)].push_back(uint16_t(p));
        w.row_pilots[size_t(q / Nc)].push_back(uint16_t(p));
    }
    const int nPilots = int(pilot_sym.size());
    w.time_class.assign(size_t(nPilots), 0); w.time_row.assign(size_t(nPilots), 0);
    w.freq_class.assign(size_t(nPilots), 0); w.freq_row.assign(size_t(nPilots), 0);

    // ---- time: one matrix per distinct set of pilot rows ----
    std::map<std::vector<int>, int> seen;
    std::vector<std::vector<double>> Rt;
    for (int c = 0; c < Nc; ++c) {
        const auto& list = w.col_pilots[size_t(c)];
        if (list.empty()) continue;
        std::vector<int> rows;
        for (uint16_t p : list) rows.push_back(pilot_sym[p]);
        auto it = seen.find(rows);
        if (it == seen.end()) {
            it = seen.emplace(rows, int(w.time_members.size())).first;
            const int n = int(rows.size());
            std::vector<double> R(size_t(n) * n), M;
            for (int a = 0; a < n; ++a)
                for (int b = 0; b < n; ++b) R[size_t(a) * n + b] = sinc(2.0 * d.doppler_hz * Ts * double(rows[a] - rows[b]));
            M = R;
            for (int a = 0; a < n; ++a) M[size_t(a) * n + a] += w.s2;
            const std::vector<double> X = solve(M, R, n);       // A = Rt M^-1 = (M^-1 Rt)^T: both are symmetric
            std::vector<double> A(size_t(n) * n);
            for (int a = 0; a < n; ++a)
                for (int b = 0; b < n; ++b) A[size_t(a) * n + b] = X[size_t(b) * n + a];
            for (int i = 0; i < n; ++i) {                       // unit gain: what row i makes of the model channel at its own pilot
                double g = 0;
                for (int k = 0; k < n; ++k) g += A[size_t(i) * n + k] * R[size_t(k) * n + i];
                for (int k = 0; k < n; ++k) A[size_t(i) * n + k] /= g;
            }
            w.time_members.push_back(rows);
            w.A.push_back(A);
            Rt.push_back(R);
        }
        for (size_t i = 0; i < list.size(); ++i) { w.time_class[list[i]] = uint16_t(it->second); w.time_row[list[i]] = uint16_t(i); }
    }
    // the noise the time filter leaves: s2 times the mean over the frame's pilots of their row's sum of squares (at unit gain, before 1 / boost)
    double acc = 0;
    for (int p = 0; p < nPilots; ++p) {
        const auto& A = w.A[w.time_class[size_t(p)]];
        const int n = int(w.time_members[w.time_class[size_t(p)]].size());
        double s = 0;
        for (int k = 0; k < n; ++k) { const double a = A[size_t(w.time_row[size_t(p)]) * n + k]; s += a * a; }
        acc += s;
    }
    w.s2b = nPilots > 0 ? w.s2 * (acc / double(nPilots)) : w.s2;
    const double inv_boost = 1.0 / pilot_boost;                 // the kernel adds the signed pilots as they are received: boost * h + noise
    for (auto& A : w.A)
        for (double& a : A) a *= inv_boost;

    // ---- frequency: one matrix per distinct set of pilot carriers ----
    seen.clear();
    using cd = std::complex<double>;
    for (int s = 0; s < Nsymb; ++s) {
        const auto& list = w.row_pilots[size_t(s)];
        if (list.empty()) continue;
        std::vector<int> cars;
        for (uint16_t p : list) cars.push_back(pilot_car[p]);
        auto it = seen.find(cars);
        if (it == seen.end()) {
            it = seen.emplace(cars, int(w.freq_members.size())).first;
            const int n = int(cars.size());
            std::vector<cd> R(size_t(n) * n), M;
            for (int a = 0; a < n; ++a)
                for (int b = 0; b < n; ++b) {
                    const double dk = double(bin(cars[a]) - bin(cars[b]));
                    const double mag = sinc((tau1 - tau0) * dk / kNfft), ph = -2.0 * M_PI * dk * (tau0 + tau1) / (2.0 * kNfft);
                    R[size_t(a) * n + b] = cd(mag * std::cos(ph), mag * std::sin(ph));
                }
            M = R;
            for (int a = 0; a < n; ++a) M[size_t(a) * n + a] += w.s2b;
            const std::vector<cd> X = solve(M, R, n);           // B = Rf M^-1 = (M^-1 Rf)^H: both are Hermitian
            std::vector<Cplx> B(size_t(n) * n);
            for (int i = 0; i < n; ++i) {
                cd g = 0;
                for (int k = 0; k < n; ++k) g += std::conj(X[size_t(k) * n + i]) * R[size_t(k) * n + i];
                for (int k = 0; k < n; ++k) { const cd b = std::conj(X[size_t(k) * n + i]) / g.real(); B[size_t(i) * n + k] = Cplx{b.real(), b.imag()}; }
            }
            w.freq_members.push_back(cars);
            w.B.push_back(B);
        }
        for (size_t i = 0; i < list.size(); ++i) { w.freq_class[list[i]] = uint16_t(it->second); w.freq_row[list[i]] = uint16_t(i); }
    }
    return w;
}

// The set-time half of include/mercury_wiener_bank.h's rule.
WienerBankRule build_wiener_bank_rule(const std::vector<uint8_t>& cell_type, int Nsymb, int Nc, const WienerDesign* designs, const double* rho_min, int n) {
    if (n < 1 || n > 4 || !designs || !rho_min) throw std::invalid_argument("Wiener bank: 1..MGPU_WIENER_BANK_MAX entries");
    WienerBankRule r;
    const auto bin = [&](int c) { return c < Nc / 2 ? c - Nc / 2 : c - Nc / 2 + 1; };
    std::vector<int> k;                             // per pilot: its bin
    std::vector<int> sym;                           // per pilot: its symbol
    r.sym_first.assign(size_t(Nsymb) + 1, 0);
    for (int q = 0; q < Nsymb * Nc; ++q) {
        if (!cell_type[size_t(q)]) continue;
        k.push_back(bin(q % Nc)); sym.push_back(q / Nc);
    }
    const int nP = int(k.size());
    if (nP > 0xffff) throw std::runtime_error("Wiener bank: more pilots than the 2-byte fields hold");
    for (int p = 0; p < nP; ++p) r.sym_first[size_t(sym[size_t(p)]) + 1] = uint16_t(p + 1);
    for (int sy = 1; sy <= Nsymb; ++sy) r.sym_first[size_t(sy)] = std::max(r.sym_first[size_t(sy)], r.sym_first[size_t(sy) - 1]);      // a symbol without pilots
    for (int p = 0; p + 1 < nP; ++p)
        if (sym[size_t(p)] == sym[size_t(p) + 1] && (r.s == 0 || k[size_t(p) + 1] - k[size_t(p)] < r.s)) r.s = k[size_t(p) + 1] - k[size_t(p)];
    if (r.s <= 0) throw std::invalid_argument("Wiener bank: no symbol has two pilots");
    r.pair.assign(size_t(nP), 0);
    for (int p = 0; p < nP; ++p) {
        if (p + 1 < nP && sym[size_t(p) + 1] == sym[size_t(p)] && k[size_t(p) + 1] - k[size_t(p)] == r.s) { r.pair[size_t(p)] |= 1; ++r.n1; }
        if (p + 2 < nP && sym[size_t(p) + 2] == sym[size_t(p)] && k[size_t(p) + 2] - k[size_t(p)] == 2 * r.s) { r.pair[size_t(p)] |= 2; ++r.n2; }
    }
    if (r.n1 == 0 || r.n2 == 0) throw std::invalid_argument("Wiener bank: the geometry has no pilot pairs one and two spacings apart");
    const double s = double(r.s);
    const auto g = [](double x) { return x < 1.0 ? sinc(x) : 0.0; };
    std::vector<double> W(static_cast<size_t>(n), 0.0), m(static_cast<size_t>(n), 0.0);
    for (int d = 0; d < n; ++d) {
        if (!wiener_design_ok(designs[d])) throw std::invalid_argument("Wiener bank: a design needs tau_max > tau_min, doppler_hz >= 0 and snr_db in -20..40, all finite");
        W[size_t(d)] = (designs[d].tau_max_us - designs[d].tau_min_us) * 0.012;
        if (d > 0 && !(W[size_t(d)] > W[size_t(d) - 1])) throw std::invalid_argument("Wiener bank: the designs' widths must be strictly ascending");
        const double den = g(s * W[size_t(d)] / kNfft);
        m[size_t(d)] = den > 0.0 ? g(2.0 * s * W[size_t(d)] / kNfft) / den : 0.0;
    }
    for (int d = 0; d + 1 < n; ++d) {
        double rho = rho_min[d];
        if (std::isnan(rho)) rho = (m[size_t(d)] + m[size_t(d) + 1]) / 2.0;
        if (!std::isfinite(rho) || rho < 0.0) throw std::invalid_argument("Wiener bank: rho_min must be finite and >= 0, or NaN for the default");
        const double tau0 = designs[d].tau_min_us * kSampleRate / 1e6, tau1 = designs[d].tau_max_us * kSampleRate / 1e6;
        const double phi = -2.0 * M_PI * s * (tau0 + tau1) / (2.0 * kNfft);
        const bool centroid = s * W[size_t(d)] < 64.0;
        r.rho_min.push_back(rho);
        r.sel.push_back(rho * rho);
        r.sel.push_back(std::cos(phi));
        r.sel.push_back(std::sin(phi));
        r.sel.push_back(centroid ? std::tan(M_PI * s * W[size_t(d)] / kNfft) : -1.0);
    }
    return r;
}

}  // namespace mgpu

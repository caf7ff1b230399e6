// Private to the library, host only, plain C++: the band scanner's rule (include/ext/mercury_scanner.h) term by term: the configuration
// check, the tables and the twin. scanner.hip exports it as mgpu_host_scan_*; tests/cpp/scanner_sanitize.cpp builds it on its own.
// Not part of the ABI.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/ext/mercury_scanner.h"
#include "iq_stream_rule.hpp"

namespace mgpu_scan_detail {

using namespace mgpu_iq_rule;

constexpr int kDefaultBlocksIn = 256;                           // max_in = 0: this many blocks
constexpr unsigned long long kScanKeyMask = 0x7fffffffffffffffull, kScanKeyInf = 0x7ff0000000000000ull;

// why the configuration is refused, or null
inline const char* config_error(const mgpu_scan_config* k) {
    if (!k) return "null configuration";
    if (k->struct_size != int(sizeof(mgpu_scan_config))) return "struct_size is not this library's sizeof(mgpu_scan_config)";
    if (const char* e = d_error(k->D)) return e;
    if (k->log2n < MGPU_SCAN_MIN_LOG2N || k->log2n > MGPU_SCAN_MAX_LOG2N) return "log2n must be 8..12";
    const int N = 1 << k->log2n;
    if (k->blocks_per_line < 1 || k->blocks_per_line > 4096) return "blocks_per_line must be 1..4096";
    if (!std::isfinite(k->threshold) || !(k->threshold >= 2.0)) return "threshold must be finite and at least 2";
    if (k->edge_bins < 0 || k->edge_bins > N / 4) return "edge_bins must be 0..N/4";
    if (k->dc_bins < 0 || k->dc_bins > 16) return "dc_bins must be 0..16";
    if (k->gap < 0 || k->gap > 64) return "gap must be 0..64";
    if (k->min_bins < 1 || k->min_bins > N) return "min_bins must be 1..N";
    if (k->max_runs < 1 || k->max_runs > MGPU_SCAN_MAX_RUNS) return "max_runs must be 1..32";
    if (k->max_in < 0 || k->max_in % (N / 2)) return "max_in must be a multiple of H";
    return nullptr;
}

inline bool usable(const mgpu_scan_config& k, int f) {
    const int N = 1 << k.log2n;
    return f >= k.edge_bins && f <= N - 1 - k.edge_bins && (k.dc_bins == 0 || std::abs(f - N / 2) > k.dc_bins);
}

// the lines a call of m blocks at block j completes
inline long long lines_completed(uint64_t j, uint64_t m, int A) { return (long long)((j + m) / uint64_t(A) - j / uint64_t(A)); }

struct Tables {
    std::vector<double> tab, win;                               // tab [N] complex (re, im), win [N]
    explicit Tables(int log2n) {
        const int N = 1 << log2n;
        tab.resize(size_t(N) * 2);
        win.resize(size_t(N));
        for (int j = 0; j < N; ++j) {
            const double a = 2.0 * M_PI * double(j) / double(N);
            tab[2 * size_t(j)] = std::cos(a);
            tab[2 * size_t(j) + 1] = std::sin(a);
            win[size_t(j)] = std::sin(M_PI * double(j) / double(N));
        }
    }
};

struct h2 { double re, im; };

inline int brev(int i, int bits) {
    int r = 0;
    for (int b = 0; b < bits; ++b) r |= ((i >> b) & 1) << (bits - 1 - b);
    return r;
}

// the rule's transform, in place in a[N]
inline void transform(h2* a, int N, const Tables& T) {
    for (int size = 2; size <= N; size *= 2) {
        const int half = size / 2, step = N / size;
        for (int g = 0; g < N; g += size)
            for (int j = 0; j < half; ++j) {
                const h2 w = {T.tab[2 * size_t(j * step)], -T.tab[2 * size_t(j * step) + 1]}, lo = a[g + j], hi = a[g + j + half];
                const h2 t = {w.re * hi.re - w.im * hi.im, w.re * hi.im + w.im * hi.re};
                a[g + j] = {lo.re + t.re, lo.im + t.im};
                a[g + j + half] = {lo.re - t.re, lo.im - t.im};
            }
    }
}

// level, occupancy and runs of one line L[N] into *r (first_block is the caller's)
inline void detect(const mgpu_scan_config& k, const double* L, mgpu_scan_report* r) {
    const int N = 1 << k.log2n;
    std::vector<unsigned long long> keys;
    std::vector<char> use(static_cast<size_t>(N), 0), occ(static_cast<size_t>(N), 0);
    bool finite = true;
    for (int f = 0; f < N; ++f) {
        use[size_t(f)] = usable(k, f);
        if (!use[size_t(f)]) continue;
        unsigned long long key;
        std::memcpy(&key, &L[f], 8);
        key &= kScanKeyMask;
        if (key >= kScanKeyInf) finite = false;
        keys.push_back(key);
    }
    if (!finite) {
        r->nonfinite = 1;
        return;
    }
    std::nth_element(keys.begin(), keys.begin() + keys.size() / 2, keys.end());
    std::memcpy(&r->level, &keys[keys.size() / 2], 8);
    const double limit = k.threshold * r->level;
    for (int f = 0; f < N; ++f) occ[size_t(f)] = use[size_t(f)] && !(L[f] <= limit);
    // the gaps: an unoccupied usable stretch between two occupied bins
    std::vector<char> closed = occ;
    for (int f = 0; f < N;) {
        if (!occ[size_t(f)] || f + 1 >= N || occ[size_t(f + 1)]) { ++f; continue; }
        int e = f + 1;                                          // the stretch is f + 1 .. e - 1
        while (e < N && use[size_t(e)] && !occ[size_t(e)]) ++e;
        if (e < N && occ[size_t(e)] && e - f - 1 <= k.gap)
            for (int i = f + 1; i < e; ++i) closed[size_t(i)] = 1;
        f = e;
    }
    for (int f = 0; f < N;) {
        if (!closed[size_t(f)]) { ++f; continue; }
        int e = f;
        while (e < N && closed[size_t(e)]) ++e;
        if (e - f >= k.min_bins) {
            if (r->n_runs < k.max_runs) {
                mgpu_scan_run& run = r->runs[r->n_runs];
                run.first = f;
                run.count = e - f;
                run.peak = f;
                double power = 0.0;
                for (int i = f; i < e; ++i) {
                    if (L[i] > L[run.peak]) run.peak = i;
                    power = power + L[i];
                }
                run.power = power;
            }
            ++r->n_runs;
        }
        f = e;
    }
    r->reported = std::min(r->n_runs, k.max_runs);
}

// the twin: MGPU_OK (0) or MGPU_ERR_ARG (1)
inline int host_process(const mgpu_scan_config* kc, const void* iq, int format, int n_in, uint64_t position, double* lines,
                        mgpu_scan_report* reports, int* n_lines) {
    if (config_error(kc) || !iq) return 1;
    const mgpu_scan_config& k = *kc;
    const int N = 1 << k.log2n, H = N / 2, A = k.blocks_per_line, e = mgpu_fmt::element(2, format);
    if (format_error(format) || n_in < H || n_in % H || position % (uint64_t(H) * A) || position > kMaxPosition ||
        position + uint64_t(n_in) > kMaxPosition)
        return 1;
    const uint64_t j = position / uint64_t(H);
    const int m = n_in / H;
    const long long n = lines_completed(j, uint64_t(m), A);
    if (n_lines) *n_lines = int(n);
    if (n > 0 && (!lines || !reports)) return 1;
    const Tables T(k.log2n);
    std::vector<h2> a(static_cast<size_t>(N), h2{0.0, 0.0});
    std::vector<double> acc(size_t(N), 0.0);
    long long line = 0;
    for (int b = 0; b < m; ++b) {
        for (int i = 0; i < N; ++i) {
            const long long g = (long long)(b - 1) * H + i;
            h2 x = {0.0, 0.0};
            if (g >= 0) x = {mgpu_fmt::widen_at(e, iq, 2 * size_t(g)), mgpu_fmt::widen_at(e, iq, 2 * size_t(g) + 1)};
            a[size_t(brev(i, k.log2n))] = {x.re * T.win[size_t(i)], x.im * T.win[size_t(i)]};
        }
        transform(a.data(), N, T);
        for (int f = 0; f < N; ++f) {
            const h2 v = a[size_t((f + N / 2) & (N - 1))];
            acc[size_t(f)] = acc[size_t(f)] + (v.re * v.re + v.im * v.im);
        }
        if ((j + uint64_t(b) + 1) % uint64_t(A) == 0) {
            double* L = lines + size_t(line) * N;
            std::memcpy(L, acc.data(), size_t(N) * 8);
            mgpu_scan_report* r = reports + line;
            std::memset(r, 0, sizeof(*r));
            r->first_block = j + uint64_t(b) + 1 - uint64_t(A);
            detect(k, L, r);
            std::fill(acc.begin(), acc.end(), 0.0);
            ++line;
        }
    }
    return 0;
}

}  // namespace mgpu_scan_detail

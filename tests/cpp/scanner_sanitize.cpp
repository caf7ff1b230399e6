// Stand-alone, CPU only (tests/test_scanner_host.py builds it with -fsanitize=address,undefined): the band scanner's twin
// (mercury_amd/csrc/scan_rule.hpp) over every format, odd cuts of the parameters and the decision edges, and the block kernel's schedule
// (mercury_amd/csrc/scan_fft.h, run group after group as the kernel's threads run it between barriers) against the rule's loop nest, bit
// for bit, at every N.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "check.hpp"
#include "scan_fft.h"
#include "scan_rule.hpp"

using namespace mgpu_scan_detail;

static mgpu_scan_config config(int log2n, int A) {
    mgpu_scan_config k{};
    k.struct_size = int(sizeof(k));
    k.D = 4; k.log2n = log2n; k.blocks_per_line = A; k.threshold = 4.0;
    k.edge_bins = 3; k.dc_bins = 1; k.gap = 2; k.min_bins = 2; k.max_runs = 4; k.max_in = 0;
    return k;
}

template <int L>
static void schedule_against_rule(std::mt19937_64& rng) {
    using F = ScanFft<L>;
    constexpr int N = F::N;
    const Tables T(L);
    std::normal_distribution<double> g;
    std::vector<sc2> v(N), s(N);
    std::vector<h2> a(N);
    for (int i = 0; i < N; ++i) {
        v[size_t(i)] = {g(rng), g(rng)};
        a[size_t(brev(i, L))] = {v[size_t(i)].re, v[size_t(i)].im};
    }
    transform(a.data(), N, T);
    const sc2* tab = reinterpret_cast<const sc2*>(T.tab.data());
    std::vector<int> fetched(N, 0);
    auto fetch = [&](int i) { ++fetched[size_t(i)]; return v[size_t(i)]; };
    if (L & 1)
        for (int u = 0; u < N / 2; ++u) F::single(u, s.data(), tab, fetch);
    for (int r = 0; r < F::kRounds; ++r)
        for (int u = N / 4 - 1; u >= 0; --u) F::round(r, u, s.data(), tab, r == 0 && !(L & 1), fetch);      // no order within a round
    for (int i = 0; i < N; ++i) CHECK(fetched[size_t(i)] == 1);
    int wrong = 0;
    for (int f = 0; f < N; ++f) {
        const h2 x = a[size_t((f + N / 2) & (N - 1))];
        const double want = x.re * x.re + x.im * x.im, got = F::power(f, s.data());
        wrong += std::memcmp(&want, &got, 8) != 0;
    }
    CHECK(wrong == 0);
    std::vector<char> seen(N, 0);                                // the entry map is a permutation
    for (int p = 0; p < N; ++p) seen[size_t(scan_entry(p))] = 1;
    for (int p = 0; p < N; ++p) CHECK(seen[size_t(p)]);
}

static void twin_runs(std::mt19937_64& rng) {
    std::normal_distribution<double> g;
    for (int log2n : {8, 9}) {
        const int N = 1 << log2n, H = N / 2;
        for (int A : {1, 3}) {
            mgpu_scan_config k = config(log2n, A);
            const int m = 2 * A + (A > 1), n_in = m * H;            // two lines, and a block of a third where a line has several
            std::vector<double> f64(size_t(n_in) * 2);
            std::vector<float> f32(f64.size());
            std::vector<int16_t> s16(f64.size());
            for (size_t i = 0; i < f64.size(); ++i) {
                f64[i] = g(rng);
                f32[i] = float(f64[i]);
                s16[i] = int16_t(rng() & 0xffff);
            }
            for (int j = 0; j < 40; ++j) f64[size_t(2 * j)] += 30.0 * std::cos(2.0 * M_PI * 0.2 * j);      // something above the level
            const void* in[3] = {s16.data(), f32.data(), f64.data()};
            for (int format = 0; format < 3; ++format) {
                std::vector<double> lines(size_t(2) * N);
                std::vector<mgpu_scan_report> reports(2);
                int n = -1;
                CHECK(host_process(&k, in[format], format, n_in, uint64_t(H) * A * 5, lines.data(), reports.data(), &n) == 0);
                CHECK(n == 2);
                CHECK(reports[0].first_block == uint64_t(5) * A && reports[1].first_block == uint64_t(6) * A);
                CHECK(reports[0].reported <= k.max_runs && reports[0].reported <= reports[0].n_runs);
            }
            f64[3] = std::numeric_limits<double>::quiet_NaN();
            std::vector<double> lines(size_t(2) * N);
            std::vector<mgpu_scan_report> reports(2);
            int n = -1;
            CHECK(host_process(&k, f64.data(), MGPU_IQ_CF64, n_in, 0, lines.data(), reports.data(), &n) == 0 && n == 2);
            CHECK(reports[0].nonfinite == 1 && reports[0].n_runs == 0 && reports[0].level == 0.0);
            // refusals touch nothing
            CHECK(host_process(&k, f64.data(), MGPU_IQ_CF64, n_in + 1, 0, lines.data(), reports.data(), &n) == 1);
            CHECK(host_process(&k, f64.data(), MGPU_IQ_CF64, n_in, uint64_t(H), lines.data(), reports.data(), &n) == (A == 1 ? 0 : 1));
            CHECK(host_process(&k, f64.data(), 7, n_in, 0, lines.data(), reports.data(), &n) == 1);
            k.gap = 65;
            CHECK(host_process(&k, f64.data(), MGPU_IQ_CF64, n_in, 0, lines.data(), reports.data(), &n) == 1);
        }
    }
    // the decision on a hand-made line: every gap length, runs at both edges and at DC
    mgpu_scan_config k = config(8, 1);
    k.max_runs = 32;
    std::vector<double> L(256, 1.0);
    for (int f = 0; f < 256; f += 1 + int(rng() % 4)) L[size_t(f)] = 100.0;
    mgpu_scan_report r;
    std::memset(&r, 0, sizeof(r));
    detect(k, L.data(), &r);
    CHECK(r.level == 1.0 && r.n_runs >= r.reported && r.reported >= 1);
    for (int i = 0; i < r.reported; ++i) CHECK(r.runs[i].first >= 3 && r.runs[i].first + r.runs[i].count <= 253);
}

int main() {
    std::mt19937_64 rng(20250607);
    schedule_against_rule<8>(rng);
    schedule_against_rule<9>(rng);
    schedule_against_rule<10>(rng);
    schedule_against_rule<11>(rng);
    schedule_against_rule<12>(rng);
    twin_runs(rng);
    if (failures) return 1;
    std::printf("scanner: clean\n");
    return 0;
}

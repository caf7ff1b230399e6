// Stand-alone, CPU only (tests/test_wideband_blanker_host.py builds it with -fsanitize=address,undefined): the wideband blanker's twin
// (mercury_amd/csrc/wblank_rule.hpp) in exactly sized buffers over the three formats, the smallest and the largest block, the widest
// guard, a seeked position and one that ends on 2^62, the refusals, and the properties that need no second implementation: an unmarked
// sample passes byte for byte, a marked one is zero, and the counts of the reports are those of the output.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "check.hpp"
#include "wblank_rule.hpp"

using namespace mgpu_wblank_detail;

static mgpu_wblank_config config(int format, int B, int guard) {
    mgpu_wblank_config k{};
    k.struct_size = int(sizeof(k));
    k.D = 4; k.format = format; k.block = B; k.threshold = MGPU_WBLANK_DEFAULT_THRESHOLD; k.max_share = MGPU_WBLANK_DEFAULT_MAX_SHARE;
    k.guard = guard; k.max_in = 0;
    return k;
}

static void twin_runs(std::mt19937_64& rng) {
    std::normal_distribution<double> g;
    for (int B : {64, 4096}) {
        const int m = 5, n_in = m * B;
        std::vector<double> f64(size_t(n_in) * 2);
        std::vector<float> f32(f64.size());
        std::vector<int16_t> s16(f64.size());
        for (size_t i = 0; i < f64.size(); ++i) f64[i] = g(rng);
        for (int b = 0; b < m; ++b)                                  // a click on every block's first and last sample
            for (int i : {0, B - 1}) f64[2 * (size_t(b) * B + size_t(i))] = 40.0;
        for (size_t i = 0; i < f64.size(); ++i) {
            f32[i] = float(f64[i]);
            s16[i] = int16_t(f64[i] * 512.0);
        }
        const void* in[3] = {s16.data(), f32.data(), f64.data()};
        const size_t bytes[3] = {4, 8, 16};
        for (int format = 0; format < 3; ++format)
            for (uint64_t position : {uint64_t(0), uint64_t(7) * B, (uint64_t(1) << 62) - uint64_t(n_in)}) {
                const mgpu_wblank_config k = config(format, B, 64);
                std::vector<char> out(size_t(n_in) * bytes[format], char(0x5a));
                std::vector<mgpu_wblank_report> reports(m);
                int n = -1;
                CHECK(host_process(&k, in[format], n_in, position, out.data(), reports.data(), &n) == 0);
                CHECK(n == m);
                const char* x = static_cast<const char*>(in[format]);
                const std::vector<char> zero(bytes[format], 0);
                CHECK(reports[0].block == int64_t(position / uint64_t(B)) - 1 && reports[0].blanked == 0 && reports[0].exceeding == 0);
                for (int b = 0; b < m; ++b) {
                    int zeros = 0, changed = 0;
                    for (int i = 0; i < B; ++i) {
                        const char* y = out.data() + (size_t(b) * B + size_t(i)) * bytes[format];
                        const bool is_zero = std::memcmp(y, zero.data(), bytes[format]) == 0;
                        zeros += is_zero;
                        if (b > 0 && !is_zero) changed += std::memcmp(y, x + (size_t(b - 1) * B + size_t(i)) * bytes[format], bytes[format]) != 0;
                    }
                    CHECK(changed == 0);
                    if (b == 0) CHECK(zeros == B);
                    else {
                        CHECK(reports[b].block == reports[0].block + b && reports[b].exceeding == 2 && reports[b].capped == 0);
                        CHECK(reports[b].blanked == (B == 64 ? 64 : 130) && zeros >= reports[b].blanked);
                    }
                }
                // without reports, and the refusals, which touch nothing
                CHECK(host_process(&k, in[format], n_in, position, out.data(), nullptr, nullptr) == 0);
                CHECK(host_process(&k, in[format], n_in + 1, 0, out.data(), reports.data(), &n) == 1);
                CHECK(host_process(&k, in[format], n_in, uint64_t(B) + 1, out.data(), reports.data(), &n) == 1);
                CHECK(host_process(&k, in[format], n_in, (uint64_t(1) << 62), out.data(), reports.data(), &n) == 1);
                CHECK(host_process(&k, nullptr, n_in, 0, out.data(), reports.data(), &n) == 1);
            }
    }
    // NaN, infinities and silence
    mgpu_wblank_config k = config(MGPU_IQ_CF64, 64, 2);
    std::vector<double> x(size_t(3) * 64 * 2, 0.0), out(x.size());
    x[10] = std::numeric_limits<double>::quiet_NaN();
    x[20] = -std::numeric_limits<double>::infinity();
    x[2 * 64 + 7] = 1e-300;
    std::vector<mgpu_wblank_report> reports(3);
    int n = 0;
    CHECK(host_process(&k, x.data(), 3 * 64, 0, out.data(), reports.data(), &n) == 0 && n == 3);
    CHECK(reports[1].exceeding == 2 && reports[1].blanked == 10 && reports[1].level == 0.0 && reports[2].exceeding == 0);
    for (double bad : {1.0, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()}) {
        k.threshold = bad;
        CHECK(config_error(&k) != nullptr && host_process(&k, x.data(), 64, 0, out.data(), nullptr, nullptr) == 1);
    }
    k = config(MGPU_IQ_CF64, 64, 65);
    CHECK(config_error(&k) != nullptr);
    k = config(7, 64, 4);
    CHECK(config_error(&k) != nullptr);
    k = config(MGPU_IQ_CF64, 0, 4);
    k.D = 64;
    CHECK(config_error(&k) == nullptr && block_of(k) == 4096 && cap_of(k) == 512);
}

int main() {
    std::mt19937_64 rng(20260321);
    twin_runs(rng);
    if (failures) return 1;
    std::printf("wideband blanker: clean\n");
    return 0;
}

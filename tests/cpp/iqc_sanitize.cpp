// Stand-alone, CPU only (tests/test_iq_corrector_host.py builds it with -fsanitize=address,undefined): the IQ corrector's twin
// (mercury_amd/csrc/iqc_rule.hpp) in exactly sized buffers over the three formats, the smallest and the largest block, a seeked position
// and one that ends on 2^62, a skipped block, the fixed mode, a carried state, the refusals, and the properties that need no second
// implementation: an identity estimate passes the floats as they are, and a call cut in two gives the whole call's bytes.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "check.hpp"
#include "iqc_rule.hpp"

using namespace mgpu_iqc_detail;

static mgpu_iqc_config config(int format, int B, int memory) {
    mgpu_iqc_config k{};
    k.struct_size = int(sizeof(k));
    k.D = 4; k.format = format; k.block = B; k.memory = memory; k.dc = 1; k.balance = 1; k.fixed = 0; k.fixed_gain = 1.0; k.max_in = 0;
    return k;
}

static void twin_runs(std::mt19937_64& rng) {
    std::normal_distribution<double> g;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (int B : {256, 4096}) {
        const int m = 5, n_in = m * B;
        std::vector<double> f64(size_t(n_in) * 2);
        std::vector<float> f32(f64.size());
        std::vector<int16_t> s16(f64.size());
        for (size_t i = 0; i < f64.size(); i += 2) {                 // gain 1.1, skew 0.1, DC (0.3, -0.2)
            const double I = 0.2 * g(rng), Q = 0.2 * g(rng);
            f64[i] = I + 0.3, f64[i + 1] = 1.1 * Q + 0.1 * I - 0.2;
        }
        f64[2 * (size_t(3) * B + 5)] = nan;                          // block 3 is skipped (the floats)
        for (size_t i = 0; i < f64.size(); ++i) {
            f32[i] = float(f64[i]);
            s16[i] = f64[i] != f64[i] ? int16_t(32767) : int16_t(std::max(-32768.0, std::min(32767.0, f64[i] * 24576.0)));
        }
        const void* in[3] = {s16.data(), f32.data(), f64.data()};
        const size_t bytes[3] = {4, 8, 16};
        for (int format = 0; format < 3; ++format)
            for (uint64_t position : {uint64_t(0), uint64_t(7) * B, (uint64_t(1) << 62) - uint64_t(n_in)}) {
                const mgpu_iqc_config k = config(format, B, 2);
                std::vector<char> out(size_t(n_in) * bytes[format], char(0x5a));
                std::vector<mgpu_iqc_report> reports(m);
                int n = -1;
                CHECK(host_process(&k, nullptr, in[format], n_in, position, out.data(), reports.data(), &n) == 0);
                CHECK(n == m);
                for (int b = 0; b < m; ++b) {
                    CHECK(reports[b].block == int64_t(position / uint64_t(B)) + b);
                    CHECK(reports[b].flags == (b == 3 && format != MGPU_IQ_CS16 ? MGPU_IQC_SKIPPED : 0));
                    CHECK(reports[b].gain > 0.7 && reports[b].gain < 1.1 && reports[b].skew > -0.1 && reports[b].skew < 0.3);
                    CHECK(reports[b].dc_re > 0.2 && reports[b].dc_im < -0.1);
                }
                if (format != MGPU_IQ_CS16) CHECK(std::memcmp(&reports[3].dc_re, &reports[2].dc_re, 32) == 0);
                // the call cut in two, the state carried by hand, and without reports
                std::vector<char> cut(out.size(), char(0x33));
                double T[6] = {0, 0, 0, 0, 0, 0};
                CHECK(host_process(&k, T, in[format], 2 * B, position, cut.data(), nullptr, nullptr) == 0);
                CHECK(T[5] > 0.0);
                CHECK(host_process(&k, T, static_cast<const char*>(in[format]) + size_t(2) * B * bytes[format], 3 * B, position + 2 * uint64_t(B),
                                   cut.data() + size_t(2) * B * bytes[format], nullptr, &n) == 0);
                CHECK(n == 3 && cut == out);
                // the refusals, which touch nothing
                CHECK(host_process(&k, nullptr, in[format], n_in + 1, 0, out.data(), reports.data(), &n) == 1);
                CHECK(host_process(&k, nullptr, in[format], n_in, uint64_t(B) + 1, out.data(), reports.data(), &n) == 1);
                CHECK(host_process(&k, nullptr, in[format], n_in, (uint64_t(1) << 62), out.data(), reports.data(), &n) == 1);
                CHECK(host_process(&k, nullptr, nullptr, n_in, 0, out.data(), reports.data(), &n) == 1);
                CHECK(cut == out);
                // fixed mode at identity: the floats pass as they are (but for what a NaN is)
                mgpu_iqc_config f = config(format, B, 0);
                f.fixed = 1;
                CHECK(host_process(&f, nullptr, in[format], 3 * B, position, cut.data(), reports.data(), &n) == 0 && n == 3);
                CHECK(std::memcmp(cut.data(), in[format], size_t(3) * B * bytes[format]) == 0);
                CHECK(reports[2].flags == 0 && reports[2].gain == 1.0 && reports[2].clamped == 0);
            }
    }
    // silence, pure I, an infinity, clamping
    mgpu_iqc_config k = config(MGPU_IQ_CF64, 256, 0);
    std::vector<double> x(size_t(3) * 256 * 2, 0.0), out(x.size());
    for (int i = 0; i < 256; ++i) x[2 * (256 + size_t(i))] = g(rng);
    x[2 * (512 + 9) + 1] = -inf;
    std::vector<mgpu_iqc_report> reports(3);
    int n = 0;
    CHECK(host_process(&k, nullptr, x.data(), 3 * 256, 0, out.data(), reports.data(), &n) == 0 && n == 3);
    CHECK(reports[0].flags == MGPU_IQC_NO_BALANCE && reports[1].flags == MGPU_IQC_NO_BALANCE);
    CHECK(reports[2].flags == (MGPU_IQC_NO_BALANCE | MGPU_IQC_SKIPPED) && reports[2].dc_re == reports[1].dc_re);
    k = config(MGPU_IQ_CS16, 256, 0);
    k.fixed = 1; k.fixed_gain = 2.0; k.fixed_dc_re = -0.5;
    std::vector<int16_t> s(size_t(256) * 2, int16_t(30000)), so(s.size());
    CHECK(host_process(&k, nullptr, s.data(), 256, 0, so.data(), reports.data(), &n) == 0 && reports[0].clamped == 512 && so[0] == 32767);
    // the configuration's refusals
    for (double bad : {nan, inf, -inf, 0.49, 2.01}) {
        k = config(MGPU_IQ_CF64, 256, 2);
        k.fixed = 1; k.fixed_gain = bad;
        CHECK(config_error(&k) != nullptr && host_process(&k, nullptr, x.data(), 256, 0, out.data(), nullptr, nullptr) == 1);
        k.fixed_gain = 1.0; k.fixed_skew = bad;
        CHECK((config_error(&k) != nullptr) == !(bad >= -0.5 && bad <= 0.5));
        k.fixed_skew = 0.0; k.fixed_dc_im = bad;
        CHECK((config_error(&k) != nullptr) == !is_finite(bad));
    }
    for (int block : {128, 384, 8192}) { k = config(MGPU_IQ_CF64, block, 2); CHECK(config_error(&k) != nullptr); }
    for (int memory : {1, -1, (1 << 20) + 1}) { k = config(MGPU_IQ_CF64, 256, memory); CHECK(config_error(&k) != nullptr); }
    k = config(7, 256, 2);
    CHECK(config_error(&k) != nullptr);
    k = config(MGPU_IQ_CF64, 256, 2); k.dc = 2;
    CHECK(config_error(&k) != nullptr);
    k = config(MGPU_IQ_CF64, 256, 2); k.max_in = 300;
    CHECK(config_error(&k) != nullptr);
    k = config(MGPU_IQ_CF64, 0, 0);
    CHECK(config_error(&k) == nullptr && block_of(k) == 4096 && lambda_of(k) == 1.0);
    k.memory = 1024;
    CHECK(lambda_of(k) == 1023.0 / 1024.0);
}

int main() {
    std::mt19937_64 rng(20261021);
    twin_runs(rng);
    if (failures) return 1;
    std::printf("iq corrector: clean\n");
    return 0;
}

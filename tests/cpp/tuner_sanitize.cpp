// Stand-alone, CPU only (tests/test_tuner_host.py builds it with mercury_amd/csrc/chan_tables.cpp under -fsanitize=address,undefined):
// the carrier tuner's twin (mercury_amd/csrc/tune_rule.hpp) in exactly sized buffers over every format, both sidebands, the smallest and
// an odd configuration, a NaN block and the refusals; and the comb kernel's use of the scanner's schedule (scan_fft.h at log2n = 8, read
// in the transform's own bin order) against the rule's loop nest, bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "check.hpp"
#include "scan_fft.h"
#include "tune_rule.hpp"

using namespace mgpu_tune_detail;

static mgpu_tune_config config(int D, int S, int J, int K, const std::vector<double>& taps) {
    mgpu_tune_config k{};
    k.struct_size = int(sizeof(k));
    k.D = D; k.S = S; k.audio_centre_hz = 1472; k.ntaps = int(taps.size()); k.taps = taps.data(); k.symbols = J; k.search = K;
    k.carrier_hz = MGPU_TUNE_DEFAULT_CARRIER_HZ; k.min_metric = 0.3;
    return k;
}

static void comb_schedule_against_rule(std::mt19937_64& rng) {
    using F = ScanFft<kLog2>;
    const mgpu_scan_detail::Tables T(kLog2);
    std::normal_distribution<double> g;
    std::vector<sc2> v(kNfft), s(kNfft);
    std::vector<mgpu_scan_detail::h2> a(kNfft);
    for (int i = 0; i < kNfft; ++i) {
        v[size_t(i)] = {g(rng), g(rng)};
        a[size_t(mgpu_scan_detail::brev(i, kLog2))] = {v[size_t(i)].re, v[size_t(i)].im};
    }
    mgpu_scan_detail::transform(a.data(), kNfft, T);
    const sc2* tab = reinterpret_cast<const sc2*>(T.tab.data());
    auto fetch = [&](int i) { return v[size_t(i)]; };
    for (int r = 0; r < F::kRounds; ++r)
        for (int u = 0; u < kNfft / 4; ++u) F::round(r, u, s.data(), tab, r == 0, fetch);
    int wrong = 0;
    for (int k = 0; k < kNfft; ++k) {
        const sc2 u = s[size_t(scan_entry(scan_brev(k, kLog2)))];
        wrong += std::memcmp(&u.re, &a[size_t(k)].re, 8) != 0 || std::memcmp(&u.im, &a[size_t(k)].im, 8) != 0;
    }
    CHECK(wrong == 0);
}

static void twin_runs(std::mt19937_64& rng) {
    std::normal_distribution<double> g;
    for (int D : {1, 3}) {
        std::vector<double> taps(size_t(8 * D + 1));
        mgpu_chan_detail::windowed_sinc(int(taps.size()), 2 * 1500.0 / (48000.0 * D), 60.0, 1.0, taps.data());
        for (int J : {4, 5}) {
            const int S = 3;
            mgpu_tune_config k = config(D, S, J, J == 4 ? 0 : 24, taps);
            const mgpu_chan_channel chans[3] = {{-24000 * D + 1, 0, 1.0}, {24000 * D - 1, 1, 0.5}, {-7, 0, 2.0}};     // the bands' edges
            const int n_in = input_samples(k);
            CHECK(n_in == 4 * D * 272 * (J + 1));
            std::vector<double> f64(size_t(n_in) * 2);
            std::vector<float> f32(f64.size());
            std::vector<int16_t> s16(f64.size());
            for (size_t i = 0; i < f64.size(); ++i) {
                f64[i] = g(rng);
                f32[i] = float(f64[i]);
                s16[i] = int16_t(rng() & 0xffff);
            }
            const void* in[3] = {s16.data(), f32.data(), f64.data()};
            for (int format = 0; format < 3; ++format) {
                std::vector<mgpu_tune_report> reports(size_t(S) * 1);
                std::vector<double> G(size_t(S) * kSym * 2), E(size_t(S) * kSym), Q(size_t(S) * kNfft);
                CHECK(host_process(&k, chans, in[format], format, n_in, reports.data(), G.data(), E.data(), Q.data()) == 0);
                for (int s = 0; s < S; ++s) {
                    const mgpu_tune_report& r = reports[size_t(s)];
                    CHECK(r.nonfinite == 0 && r.phase >= 0 && r.phase < kSym && r.shift >= -k.search && r.shift <= k.search);
                    CHECK(r.metric >= 0.0 && r.metric <= 1.0 + 1e-12 && r.frac_hz >= -23.4375 && r.frac_hz <= 23.4375);
                    CHECK(r.valid || r.offset_hz == chans[s].offset_hz);
                    mgpu_chan_channel out{};
                    CHECK(host_plan(&r, chans + s, &out) == 0 && out.sideband == chans[s].sideband && out.gain == chans[s].gain);
                    CHECK(out.offset_hz == r.offset_hz);
                }
                CHECK(host_process(&k, chans, in[format], format, n_in, reports.data(), nullptr, nullptr, nullptr) == 0);
            }
            // a NaN anywhere in the block reaches every channel's sums
            f64[size_t(n_in)] = std::numeric_limits<double>::quiet_NaN();
            std::vector<mgpu_tune_report> reports(size_t(S) * 1);
            CHECK(host_process(&k, chans, f64.data(), MGPU_IQ_CF64, n_in, reports.data(), nullptr, nullptr, nullptr) == 0);
            for (int s = 0; s < S; ++s)
                CHECK(reports[size_t(s)].nonfinite == 1 && reports[size_t(s)].valid == 0 && reports[size_t(s)].offset_hz == chans[s].offset_hz);
            // silence: E = 0, metric 0, not valid
            std::fill(f64.begin(), f64.end(), 0.0);
            CHECK(host_process(&k, chans, f64.data(), MGPU_IQ_CF64, n_in, reports.data(), nullptr, nullptr, nullptr) == 0);
            CHECK(reports[0].metric == 0.0 && reports[0].valid == 0 && reports[0].nonfinite == 0 && reports[0].phase == 0);
            // refusals touch nothing
            CHECK(host_process(&k, chans, f64.data(), MGPU_IQ_CF64, n_in - 1, reports.data(), nullptr, nullptr, nullptr) == 1);
            CHECK(host_process(&k, chans, f64.data(), 7, n_in, reports.data(), nullptr, nullptr, nullptr) == 1);
            const mgpu_chan_channel outside[3] = {{-24000 * D, 0, 1.0}, chans[1], chans[2]};
            CHECK(host_process(&k, outside, f64.data(), MGPU_IQ_CF64, n_in, reports.data(), nullptr, nullptr, nullptr) == 1);
            k.symbols = 3;
            CHECK(host_process(&k, chans, f64.data(), MGPU_IQ_CF64, n_in, reports.data(), nullptr, nullptr, nullptr) == 1);
        }
    }
}

int main() {
    std::mt19937_64 rng(20261021);
    comb_schedule_against_rule(rng);
    twin_runs(rng);
    if (failures) return 1;
    std::printf("tuner: clean\n");
    return 0;
}

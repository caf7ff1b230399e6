// The resampler's host side (include/ext/mercury_resampler.h) as a stand-alone program for the address and undefined-behaviour
// sanitizers: built from this file, mercury_amd/csrc/resamp_tables.cpp and chan_tables.cpp with -fsanitize=address,undefined and run on the CPU
// (tests/test_resampler_host.py). It designs, counts and resamples at two ratios, in exactly sized buffers, so that a read or write past
// an end, a signed overflow or a misaligned access in the design, the count or the twin stops it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "check.hpp"
#include "ext/mercury_resampler.h"

static int one(int fin, int fout, int components, int format, int tp, uint64_t position) {
    int ntaps = 0;
    CHECK(mgpu_host_resamp_design(fin, fout, tp, 0.0, 0.0, nullptr, &ntaps) == MGPU_OK && ntaps > 1);
    std::vector<double> taps(size_t(ntaps), 0.0);
    CHECK(mgpu_host_resamp_design(fin, fout, tp, 0.0, 0.0, taps.data(), &ntaps) == MGPU_OK && size_t(ntaps) == taps.size());
    for (int k = 0; k < ntaps; ++k) CHECK(std::memcmp(&taps[k], &taps[ntaps - 1 - k], 8) == 0);

    const int S = 2, n_in = 777;
    // the count of the whole equals the counts of its cuts, 1-sample cuts included
    int whole = 0, sum = 0;
    CHECK(mgpu_host_resamp_count(fin, fout, position, n_in, &whole) == MGPU_OK && whole > 0);
    for (int at = 0, cut = 1; at < n_in; at += cut, cut = cut % 7 + 1) {
        int n = 0;
        const int c = cut < n_in - at ? cut : n_in - at;
        CHECK(mgpu_host_resamp_count(fin, fout, position + uint64_t(at), c, &n) == MGPU_OK);
        sum += n;
    }
    CHECK(sum == whole);

    // input and output buffers of exactly the sizes the twin is told
    const size_t elems = size_t(S) * n_in * components;
    std::vector<int16_t> i16(elems);
    std::vector<float> f32(elems);
    for (size_t i = 0; i < elems; ++i) {
        i16[i] = int16_t((i * 2654435761u >> 7) & 0xffff);
        f32[i] = float(i16[i]) / 32768.0f;
    }
    const bool is16 = components == 1 ? format == MGPU_SAMPLES_INT16 : format == MGPU_IQ_CS16;
    const void* in = is16 ? static_cast<const void*>(i16.data()) : static_cast<const void*>(f32.data());
    mgpu_resamp_config k{};
    k.struct_size = int(sizeof(k));
    k.fin = fin; k.fout = fout; k.S = S; k.components = components; k.tp = tp;
    std::vector<double> out_default(size_t(S) * whole * components, -1.0), out_taps(out_default);
    int n_out = 0;
    CHECK(mgpu_host_resamp_process(&k, in, format, n_in, position, out_default.data(), size_t(whole), &n_out) == MGPU_OK && n_out == whole);
    int g = fin;
    for (int b = fout; b;) { const int t = g % b; g = b; b = t; }
    k.tp = (ntaps - 1) / (fout / g);
    k.taps = taps.data();
    k.ntaps = ntaps;
    CHECK(mgpu_host_resamp_process(&k, in, format, n_in, position, out_taps.data(), size_t(whole), &n_out) == MGPU_OK && n_out == whole);
    CHECK(std::memcmp(out_default.data(), out_taps.data(), out_taps.size() * 8) == 0);       // the default design is the design
    double peak = 0;
    for (double v : out_taps) {
        CHECK(std::isfinite(v));
        peak = std::fmax(peak, std::fabs(v));
    }
    CHECK(peak > 0);
    // a row shorter than the outputs, a bad format and a bad configuration are refused without a write
    CHECK(mgpu_host_resamp_process(&k, in, format, n_in, position, out_taps.data(), size_t(whole - 1), &n_out) == MGPU_ERR_ARG);
    CHECK(mgpu_host_resamp_process(&k, in, 9, n_in, position, out_taps.data(), size_t(whole), &n_out) == MGPU_ERR_ARG);
    k.ntaps -= 1;
    CHECK(mgpu_host_resamp_process(&k, in, format, n_in, position, out_taps.data(), size_t(whole), &n_out) == MGPU_ERR_ARG);
    std::printf("%d -> %d, C = %d: %d taps, %d inputs at %llu -> %d outputs, peak %.6f\n", fin, fout, components, ntaps, n_in,
                (unsigned long long)position, whole, peak);
    return failures;
}

int main() {
    if (one(44100, 48000, 1, MGPU_SAMPLES_INT16, 0, 0)) return 1;
    if (one(2048000, 1536000, 2, MGPU_IQ_CF32, 0, (1ULL << 40) + 12345)) return 1;
    if (one(192000, 48000, 1, MGPU_SAMPLES_F32, 2, 3)) return 1;
    std::printf("resampler host side: clean\n");
    return 0;
}

// Private to the library: what synth.hip takes from synth_tables.cpp (include/ext/mercury_synth.h). Not part of the ABI.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ext/mercury_synth.h"
#include "chan_tables.hpp"

#ifdef __HIPCC__
#define MGPU_SYNTH_FN __host__ __device__ inline
#else
#define MGPU_SYNTH_FN inline
#endif

namespace mgpu_synth_detail {

constexpr int kDefaultMaxIn = 16 * 1088;
constexpr uint64_t kMaxPosition = 1ULL << 62;

// why the configuration is refused, or null. need_s: S is read (the tables of one channel do not read it)
const char* config_error(const mgpu_synth_config* k, bool need_s);
// the prototype of a checked configuration: its own taps, or the channeliser's default design
std::vector<double> prototype(const mgpu_synth_config* k);
// q+[k] = h[k] * (cos, sin)(2 pi ((a_c (k - c)) mod R) / R), interleaved re, im; q- is its conjugate
void tap_table(const std::vector<double>& h, int D, int a_c, double* qplus);
// P[r] = (cos, sin)(2 pi ((offset_hz r) mod R) / R), r < D, interleaved
void phase_row(int D, int offset_hz, double* P);
// G = (2.0 * D) * gain
inline double channel_gain(int D, double gain) { return (2.0 * double(D)) * gain; }
// (offset_hz * n) mod 48000 for n < 2^63
inline int carrier_index(int offset_hz, uint64_t n) {
    const long long a = mgpu_chan_detail::floor_mod(offset_hz, MGPU_CHAN_PHASOR_LEN);
    return int((a * (long long)(n % MGPU_CHAN_PHASOR_LEN)) % MGPU_CHAN_PHASOR_LEN);
}
inline size_t iq_sample_bytes(int format) { return format == MGPU_IQ_CS16 ? 4 : format == MGPU_IQ_CF32 ? 8 : format == MGPU_IQ_CF64 ? 16 : 0; }

// one component as CS16: clamp(nearbyint(x * 32768), -32768, 32767); *clamped += 1 where it was clamped (a NaN becomes 0 and counts)
MGPU_SYNTH_FN int16_t to_cs16(double x, unsigned* clamped) {
    const double y = rint(x * 32768.0);
    if (y > 32767.0) { ++*clamped; return 32767; }
    if (y < -32768.0) { ++*clamped; return -32768; }
    if (y != y) { ++*clamped; return 0; }
    return int16_t(int(y));
}
// IQ sample m of `out` in `format`; returns the components clamped
MGPU_SYNTH_FN unsigned store_iq(void* out, int format, size_t m, double re, double im) {
    unsigned clamped = 0;
    if (format == MGPU_IQ_CS16) {
        int16_t* o = static_cast<int16_t*>(out) + 2 * m;
        o[0] = to_cs16(re, &clamped);
        o[1] = to_cs16(im, &clamped);
    } else if (format == MGPU_IQ_CF32) {
        float* o = static_cast<float*>(out) + 2 * m;
        o[0] = float(re);
        o[1] = float(im);
    } else {
        double* o = static_cast<double*>(out) + 2 * m;
        o[0] = re;
        o[1] = im;
    }
    return clamped;
}

}  // namespace mgpu_synth_detail

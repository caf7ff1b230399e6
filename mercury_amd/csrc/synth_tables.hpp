// Private to the library: what synth.hip takes from synth_tables.cpp (include/ext/mercury_synth.h). Not part of the ABI.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ext/mercury_synth.h"
#include "chan_tables.hpp"
#include "iq_stream_rule.hpp"

namespace mgpu_synth_detail {

constexpr int kDefaultMaxIn = 16 * 1088;
using mgpu_iq_rule::kMaxPosition;

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

}  // namespace mgpu_synth_detail

// Private to the library: what channelizer.hip takes from chan_tables.cpp (include/mercury_channelizer.h). Not part of the ABI.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/mercury_channelizer.h"

namespace mgpu_chan_detail {

constexpr int kDefaultMaxOut = 16 * 1088;

inline long long floor_mod(long long a, long long m) {
    const long long r = a % m;
    return r < 0 ? r + m : r;
}

// why the configuration is refused, or null. need_s: S is read (the tables of one channel do not read it)
const char* config_error(const mgpu_chan_config* k, bool need_s);
// why the channel is refused at decimation D around audio centre a_c, or null
const char* channel_error(int D, int a_c, const mgpu_chan_channel* ch);
// why a plan of S channels is refused, or null: "no channels", or the first refused channel's reason
const char* plan_error(int D, int a_c, int S, const mgpu_chan_channel* channels);
// the prototype of a checked configuration: its own taps, or the default design
std::vector<double> prototype(const mgpu_chan_config* k);
// A windowed-sinc low-pass of T (odd) taps: cutoff fc as a fraction of the Nyquist frequency, Kaiser window with
// beta = 0.1102 * (atten_db - 8.7), symmetric to the bit, the taps summing to `gain` (the resampler's prototype is made by it too)
void windowed_sinc(int T, double fc, double atten_db, double gain, double* h);
// g[k] = h[k] * (cos, sin)(2 pi ((F (k - c)) mod R) / R), interleaved re, im
void tap_row(const std::vector<double>& h, int D, int a_c, const mgpu_chan_channel& ch, double* g);
// W[p] = (cos, sin)(2 pi p / 48000), interleaved
void phasor_table(double* W);
// (offset_hz * (n - L)) mod 48000 for n < 2^63
inline int phasor_index(int offset_hz, uint64_t n, int L) {
    const long long a = floor_mod(offset_hz, MGPU_CHAN_PHASOR_LEN);
    const long long b = floor_mod((long long)n - L, MGPU_CHAN_PHASOR_LEN);
    return int((a * b) % MGPU_CHAN_PHASOR_LEN);
}

}  // namespace mgpu_chan_detail

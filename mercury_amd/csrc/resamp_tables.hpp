// Private to the library: what resampler.hip takes from resamp_tables.cpp (include/ext/mercury_resampler.h). Not part of the ABI.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ext/mercury_resampler.h"

namespace mgpu_resamp_detail {

struct Ratio { int L = 0, M = 0; };

// L = fout / g, M = fin / g; false where the rule refuses the pair of rates
bool ratio(int fin, int fout, Ratio* r);
// 32 * max(1, ceil(M / L)), and long enough for the default band to fit: between the default cutoff, 0.45 * min(fin, fout), and the design
// rate's Nyquist frequency, fin * L / 2, lie half the transition and a stop-band one transition wide, 1.5 w in all, with
// w = (60 - 7.95) * fin / (14.36 * tp) by Kaiser's design formula. In units of fin the room is L / 2 - 0.45 * min(1, L / M): 0.05 at 1/1
// (tp = 110), at least 0.275 at every other ratio (tp >= 20: the first term decides). A shorter filter at 1/1 has no stop-band below the
// Nyquist frequency and the ripples of its two band edges add (profiles/resampler.md).
inline int default_tp(const Ratio& r) {
    const double room = 0.5 * r.L - 0.45 * std::min(1.0, double(r.L) / r.M);
    const int fit = int(std::ceil(1.5 * (60.0 - 7.95) / (14.36 * room)));
    return std::max(32 * ((r.M + r.L - 1) / r.L), fit + (fit & 1));
}
inline int default_max_in(const Ratio& r) { return int((17408LL * r.M + r.L - 1) / r.L); }
// ceil(m * L / M) for m <= 2^52 (m * L < 2^62)
inline uint64_t out_position(uint64_t m, const Ratio& r) { return (m * uint64_t(r.L) + uint64_t(r.M) - 1) / uint64_t(r.M); }
// why the configuration is refused, or null
const char* config_error(const mgpu_resamp_config* k);
// the prototype of a checked configuration: its own taps, or the default design at its tp
std::vector<double> prototype(const mgpu_resamp_config* k, const Ratio& r);
inline int config_tp(const mgpu_resamp_config* k, const Ratio& r) { return k->tp ? k->tp : default_tp(r); }

}  // namespace mgpu_resamp_detail

// Private to the library, host only, plain C++ without libm: what the rules of the wideband IQ stages (scan_rule.hpp, wblank_rule.hpp,
// iqc_rule.hpp, synth_tables.hpp) check alike: the limits of a stream and of a call, and a configuration's D and IQ format. Not part
// of the ABI.
#pragma once
#include "sample_formats.h"

namespace mgpu_iq_rule {

constexpr uint64_t kMaxPosition = 1ULL << 62;                   // no stream goes further
constexpr int kMaxIn = 1 << 26;                                 // no call is longer

// why a configuration's D, or an IQ format, is refused, or null
inline const char* d_error(int D) { return D < 1 || D > MGPU_CHAN_MAX_D ? "D must be 1..64" : nullptr; }
inline const char* format_error(int format) { return mgpu_fmt::iq_bytes(format) ? nullptr : "unknown IQ format"; }

// a call of n_in samples at `position` on a stage of block B and max_in (0: no such limit)
inline bool call_ok(int B, int max_in, uint64_t position, int n_in) {
    return n_in >= B && n_in % B == 0 && (max_in == 0 || n_in <= max_in) && position <= kMaxPosition && position % uint64_t(B) == 0 &&
           position + uint64_t(n_in) <= kMaxPosition;
}

}  // namespace mgpu_iq_rule

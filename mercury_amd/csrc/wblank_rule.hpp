// Private to the library, host only, plain C++ without libm: the wideband impulse blanker's rule (include/ext/mercury_wideband_blanker.h)
// term by term: the configuration check, the refusals and the twin. wideband_blanker.hip exports it as mgpu_host_wblank_process;
// tests/cpp/wblank_sanitize.cpp builds it on its own. Not part of the ABI.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/ext/mercury_wideband_blanker.h"
#include "iq_stream_rule.hpp"

namespace mgpu_wblank_detail {

using namespace mgpu_iq_rule;

constexpr int kDefaultBlocksIn = 1024;                          // max_in = 0: this many blocks
constexpr unsigned long long kWblankKeyMask = 0x7fffffffffffffffull;

// B of a configuration whose D is in range
inline int block_of(const mgpu_wblank_config& k) {
    if (k.block) return k.block;
    const int step = 64 * k.D;
    return (256 + step - 1) / step * step;
}

// why the configuration is refused, or null. Every comparison is written so that a NaN fails it.
inline const char* config_error(const mgpu_wblank_config* k) {
    if (!k) return "null configuration";
    if (k->struct_size != int(sizeof(mgpu_wblank_config))) return "struct_size is not this library's sizeof(mgpu_wblank_config)";
    if (const char* e = d_error(k->D)) return e;
    if (const char* e = format_error(k->format)) return e;
    if (k->block != 0 && (k->block < MGPU_WBLANK_MIN_BLOCK || k->block > MGPU_WBLANK_MAX_BLOCK || k->block % 64))
        return "block must be a multiple of 64, 64..4096, or 0";
    if (!(k->threshold >= 2.0) || !(k->threshold <= 1.7976931348623157e308)) return "threshold must be finite and at least 2";
    if (k->guard < 0 || k->guard > MGPU_WBLANK_MAX_GUARD) return "guard must be 0..64";
    if (!(k->max_share > 0.0) || !(k->max_share <= 0.5)) return "max_share must be in (0, 0.5]";
    if (k->max_in < 0 || k->max_in > kMaxIn || k->max_in % block_of(*k)) return "max_in must be a multiple of B, 2^26 at most";
    return nullptr;
}

// cap = floor(max_share * B) in double; the product is non-negative and below 2^31, so the conversion is the floor
inline int cap_of(const mgpu_wblank_config& k) { return int(k.max_share * double(block_of(k))); }

inline unsigned long long key_of(double p) {
    unsigned long long key;
    std::memcpy(&key, &p, 8);
    return key & kWblankKeyMask;
}

// level, exceeding and capped of one block's powers p[B]; exceeds[B] is what is left of the flags after the cap
inline void analyse(const mgpu_wblank_config& k, int B, int cap, const double* p, char* exceeds, mgpu_wblank_report* r) {
    std::vector<unsigned long long> keys(static_cast<size_t>(B), 0ull);
    for (int i = 0; i < B; ++i) keys[size_t(i)] = key_of(p[i]);
    std::nth_element(keys.begin(), keys.begin() + B / 2, keys.end());
    std::memcpy(&r->level, &keys[size_t(B / 2)], 8);
    const double limit = k.threshold * r->level;
    int E = 0;
    for (int i = 0; i < B; ++i) {
        exceeds[i] = !(p[i] <= limit);
        E += exceeds[i];
    }
    r->exceeding = E;
    r->capped = E > cap;
    if (r->capped) std::memset(exceeds, 0, size_t(B));
}

// the twin: MGPU_OK (0) or MGPU_ERR_ARG (1)
inline int host_process(const mgpu_wblank_config* kc, const void* iq, int n_in, uint64_t position, void* out, mgpu_wblank_report* reports,
                        int* n_reports) {
    if (config_error(kc) || !iq || !out) return 1;
    const mgpu_wblank_config& k = *kc;
    const int B = block_of(k), cap = cap_of(k), e = mgpu_fmt::element(2, k.format), guard = k.guard;
    if (!call_ok(B, k.max_in, position, n_in)) return 1;
    const int m = n_in / B;
    const size_t bytes = mgpu_fmt::iq_bytes(k.format);
    if (n_reports) *n_reports = m;
    std::vector<char> exceeds(static_cast<size_t>(n_in), 0);
    std::vector<mgpu_wblank_report> rep(static_cast<size_t>(m));
    std::vector<double> p(static_cast<size_t>(B), 0.0);
    for (int b = 0; b < m; ++b) {
        for (int i = 0; i < B; ++i) {
            const size_t g = size_t(b) * B + size_t(i);
            const double re = mgpu_fmt::widen_at(e, iq, 2 * g), im = mgpu_fmt::widen_at(e, iq, 2 * g + 1);
            p[size_t(i)] = re * re + im * im;
        }
        std::memset(&rep[size_t(b)], 0, sizeof(mgpu_wblank_report));
        analyse(k, B, cap, p.data(), exceeds.data() + size_t(b) * B, &rep[size_t(b)]);
    }
    // the block before the first is zeros; then the blocks 0 .. m - 2 of the call, marked by the flags within the guard on either side
    char* const o = static_cast<char*>(out);
    const char* const x = static_cast<const char*>(iq);
    std::memset(o, 0, size_t(B) * bytes);
    if (reports) {
        std::memset(reports, 0, size_t(m) * sizeof(mgpu_wblank_report));
        reports[0].block = int64_t(position / uint64_t(B)) - 1;
    }
    for (int b = 0; b + 1 < m; ++b) {
        int blanked = 0;
        for (int i = 0; i < B; ++i) {
            const long long g = (long long)b * B + i;
            bool marked = false;
            for (long long j = std::max(0ll, g - guard); j <= g + guard && !marked; ++j) marked = exceeds[size_t(j)] != 0;   // g + guard < n_in
            char* const y = o + (size_t(g) + size_t(B)) * bytes;
            if (marked) std::memset(y, 0, bytes);
            else std::memcpy(y, x + size_t(g) * bytes, bytes);
            blanked += marked;
        }
        if (reports) {
            reports[b + 1] = rep[size_t(b)];
            reports[b + 1].block = int64_t(position / uint64_t(B)) + b;
            reports[b + 1].blanked = blanked;
        }
    }
    return 0;
}

}  // namespace mgpu_wblank_detail

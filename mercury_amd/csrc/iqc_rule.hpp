// Private to the library: the IQ corrector's rule (include/ext/mercury_iq_corrector.h) term by term: the configuration check, the
// refusals, the estimate (host and device: the kernels call the same function) and the twin. iq_corrector.hip exports the twin as
// mgpu_host_iqc_process; tests/cpp/iqc_sanitize.cpp builds it on its own. Every translation unit that includes it is built with
// -ffp-contract=off. Not part of the ABI.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/ext/mercury_iq_corrector.h"
#include "iq_stream_rule.hpp"

namespace mgpu_iqc_detail {

using namespace mgpu_iq_rule;

constexpr int kDefaultBlocksIn = 1024;                          // max_in = 0: this many blocks
constexpr int kPartials = 256;                                  // partial sums per term and block
constexpr int kTerms = 5;                                       // I, Q, I I, I Q, Q Q

inline int block_of(const mgpu_iqc_config& k) { return k.block ? k.block : MGPU_IQC_MAX_BLOCK; }
inline double lambda_of(const mgpu_iqc_config& k) { return k.memory ? 1.0 - 1.0 / double(k.memory) : 1.0; }

MGPU_FMT_FN bool is_finite(double x) { return x - x == 0.0; }      // false for a NaN and for either infinity

// why the configuration is refused, or null. Every comparison is written so that a NaN fails it.
inline const char* config_error(const mgpu_iqc_config* k) {
    if (!k) return "null configuration";
    if (k->struct_size != int(sizeof(mgpu_iqc_config))) return "struct_size is not this library's sizeof(mgpu_iqc_config)";
    if (const char* e = d_error(k->D)) return e;
    if (const char* e = format_error(k->format)) return e;
    if (k->block != 0 && (k->block < MGPU_IQC_MIN_BLOCK || k->block > MGPU_IQC_MAX_BLOCK || k->block % kPartials))
        return "block must be a multiple of 256, 256..4096, or 0";
    if (k->memory != 0 && (k->memory < 2 || k->memory > MGPU_IQC_MAX_MEMORY)) return "memory must be 0 or 2..2^20 blocks";
    if (k->dc < 0 || k->dc > 1 || k->balance < 0 || k->balance > 1 || k->fixed < 0 || k->fixed > 1) return "dc, balance and fixed must be 0 or 1";
    if (k->fixed) {
        if (!is_finite(k->fixed_dc_re) || !is_finite(k->fixed_dc_im)) return "fixed_dc_re and fixed_dc_im must be finite";
        if (!(k->fixed_skew >= -MGPU_IQC_MAX_SKEW) || !(k->fixed_skew <= MGPU_IQC_MAX_SKEW)) return "fixed_skew must be in [-0.5, 0.5]";
        if (!(k->fixed_gain >= 1.0 / MGPU_IQC_MAX_GAIN) || !(k->fixed_gain <= MGPU_IQC_MAX_GAIN)) return "fixed_gain must be in [0.5, 2]";
    }
    if (k->max_in < 0 || k->max_in > kMaxIn || k->max_in % block_of(*k)) return "max_in must be a multiple of B, 2^26 at most";
    return nullptr;
}

// the four values a block's samples are corrected with, and MGPU_IQC_NO_BALANCE or 0
struct Estimate {
    double dc_re, dc_im, skew, gain;
    int flags;
};

// the estimate the state (tI, tQ, tII, tIQ, tQQ, N) gives
MGPU_FMT_FN Estimate estimate(double tI, double tQ, double tII, double tIQ, double tQQ, double N, int dc, int balance) {
    Estimate e{0.0, 0.0, 0.0, 1.0, MGPU_IQC_NO_BALANCE};
    if (N == 0.0) return e;
    const double mI = tI / N, mQ = tQ / N;
    const double cII = tII / N - mI * mI, cQQ = tQQ / N - mQ * mQ, cIQ = tIQ / N - mI * mQ;
    if (dc) e.dc_re = mI, e.dc_im = mQ;
    if (!(cII > 0.0)) return e;                                 // not valid whatever the quotients would be
    const double skew = cIQ / cII, r = cQQ / cII - skew * skew;
    if (!(r > 0.0)) return e;
    const double gain = 1.0 / sqrt(r);
    if (!is_finite(skew) || !is_finite(gain) || !(fabs(skew) <= MGPU_IQC_MAX_SKEW) || !(gain >= 1.0 / MGPU_IQC_MAX_GAIN) || !(gain <= MGPU_IQC_MAX_GAIN))
        return e;
    e.flags = 0;
    if (balance) e.skew = skew, e.gain = gain;
    return e;
}

// the fixed mode's values as an estimate
inline Estimate fixed_estimate(const mgpu_iqc_config& k) {
    return Estimate{k.dc ? k.fixed_dc_re : 0.0, k.dc ? k.fixed_dc_im : 0.0, k.balance ? k.fixed_skew : 0.0, k.balance ? k.fixed_gain : 1.0, 0};
}

// one sample corrected: (I, Q) -> (yI, yQ). Which NaN an operation on a NaN gives (its sign, its payload) is the processor's choice, so a
// NaN component leaves as the one positive quiet NaN without payload.
MGPU_FMT_FN void correct(const Estimate& e, double I, double Q, double* yI, double* yQ) {
    const double a = I - e.dc_re, q = Q - e.dc_im, s = e.skew * a;
    const double y = e.gain * (q - s);
    *yI = a != a ? __builtin_nan("") : a;
    *yQ = y != y ? __builtin_nan("") : y;
}

// S [5] of the block that begins at sample `first` of iq (elements of type e)
inline void block_sums(int e, const void* iq, size_t first, int B, double* S) {
    double p[kTerms][kPartials];
    for (int i = 0; i < B; ++i) {
        const size_t g = first + size_t(i);
        const double I = mgpu_fmt::widen_at(e, iq, 2 * g), Q = mgpu_fmt::widen_at(e, iq, 2 * g + 1);
        const double term[kTerms] = {I, Q, I * I, I * Q, Q * Q};
        const int l = i % kPartials;
        for (int t = 0; t < kTerms; ++t) p[t][l] = i < kPartials ? term[t] : p[t][l] + term[t];
    }
    for (int t = 0; t < kTerms; ++t) {
        for (int s = kPartials / 2; s >= 1; s /= 2)
            for (int l = 0; l < s; ++l) p[t][l] += p[t][l + s];
        S[t] = p[t][0];
    }
}

// the twin, continued from state [6] (null: zeros), which becomes the state after the call: MGPU_OK (0) or MGPU_ERR_ARG (1)
inline int host_process(const mgpu_iqc_config* kc, double* state, const void* iq, int n_in, uint64_t position, void* out,
                        mgpu_iqc_report* reports, int* n_reports) {
    if (config_error(kc) || !iq || !out) return 1;
    const mgpu_iqc_config& k = *kc;
    const int B = block_of(k), e = mgpu_fmt::element(2, k.format);
    if (!call_ok(B, k.max_in, position, n_in)) return 1;
    const int m = n_in / B;
    const double lambda = lambda_of(k);
    double T[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (state) std::memcpy(T, state, sizeof(T));
    if (n_reports) *n_reports = m;
    for (int b = 0; b < m; ++b) {
        int flags = 0;
        Estimate est = fixed_estimate(k);
        if (!k.fixed) {
            double S[kTerms];
            block_sums(e, iq, size_t(b) * size_t(B), B, S);
            bool skipped = false;
            for (int t = 0; t < kTerms; ++t) skipped = skipped || !is_finite(S[t]);
            if (skipped) flags |= MGPU_IQC_SKIPPED;
            else {
                for (int t = 0; t < kTerms; ++t) {
                    const double decayed = lambda * T[t];
                    T[t] = decayed + S[t];
                }
                const double decayed = lambda * T[5];
                T[5] = decayed + double(B);
            }
            est = estimate(T[0], T[1], T[2], T[3], T[4], T[5], k.dc, k.balance);
        }
        unsigned clamped = 0;
        for (int i = 0; i < B; ++i) {
            const size_t g = size_t(b) * size_t(B) + size_t(i);
            double yI, yQ;
            correct(est, mgpu_fmt::widen_at(e, iq, 2 * g), mgpu_fmt::widen_at(e, iq, 2 * g + 1), &yI, &yQ);
            clamped += mgpu_fmt::store_iq(out, k.format, g, yI, yQ);
        }
        if (reports) {
            mgpu_iqc_report r;
            std::memset(&r, 0, sizeof(r));
            r.block = int64_t(position / uint64_t(B)) + b;
            r.dc_re = est.dc_re, r.dc_im = est.dc_im, r.skew = est.skew, r.gain = est.gain;
            r.flags = flags | est.flags;
            r.clamped = int(clamped);
            reports[b] = r;
        }
    }
    if (state) std::memcpy(state, T, sizeof(T));
    return 0;
}

}  // namespace mgpu_iqc_detail

// Private to the library, host only, plain C++: the carrier tuner's rule (include/ext/mercury_tuner.h) term by term: the configuration
// check, the decisions the host takes between the stages (the twin and tuner.hip's device path run the same code) and the twin.
// tuner.hip exports it as mgpu_host_tune_*; tests/cpp/tuner_sanitize.cpp builds it with chan_tables.cpp on its own. Not part of the ABI.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/ext/mercury_tuner.h"
#include "chan_tables.hpp"
#include "sample_formats.h"
#include "scan_rule.hpp"

namespace mgpu_tune_detail {

constexpr int kNfft = MGPU_TUNE_NFFT, kSym = MGPU_TUNE_SYMBOL, kGi = kSym - kNfft, kLog2 = 8, kCarriers = 25;
constexpr double kSpacing = 46.875;

inline mgpu_chan_config chan_config_of(const mgpu_tune_config& k) {
    mgpu_chan_config c{};
    c.struct_size = int(sizeof(c));
    c.D = k.D; c.S = k.S; c.audio_centre_hz = k.audio_centre_hz; c.ntaps = k.ntaps; c.taps = k.taps;
    return c;
}

// why the configuration or its plan is refused, or null
inline const char* config_error(const mgpu_tune_config* k, const mgpu_chan_channel* channels) {
    if (!k) return "null configuration";
    if (k->struct_size != int(sizeof(mgpu_tune_config))) return "struct_size is not this library's sizeof(mgpu_tune_config)";
    const mgpu_chan_config c = chan_config_of(*k);
    if (const char* bad = mgpu_chan_detail::config_error(&c, true)) return bad;
    if (k->symbols < MGPU_TUNE_MIN_SYMBOLS || k->symbols > MGPU_TUNE_MAX_SYMBOLS) return "symbols must be 4..256";
    if (k->search < 0 || k->search > MGPU_TUNE_MAX_SEARCH) return "search must be 0..24";
    if (!std::isfinite(k->carrier_hz) || !(k->carrier_hz > 0.0) || !(k->carrier_hz < 24000.0)) return "carrier_hz must lie in (0, 24000)";
    if (!std::isfinite(k->min_metric) || !(k->min_metric > 0.0) || !(k->min_metric <= 1.0)) return "min_metric must lie in (0, 1]";
    return mgpu_chan_detail::plan_error(k->D, k->audio_centre_hz, k->S, channels);
}

inline int block_samples(const mgpu_tune_config& k) { return kSym * (k.symbols + 1); }             // M
inline int input_samples(const mgpu_tune_config& k) { return 4 * k.D * block_samples(k); }        // n_in
inline long long centre_hz(const mgpu_tune_config& k, const mgpu_chan_channel& ch) {
    return (long long)ch.offset_hz + (ch.sideband ? -k.audio_centre_hz : k.audio_centre_hz);       // F
}

inline bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

inline mgpu_tune_report nonfinite_report(const mgpu_chan_channel& ch) {
    mgpu_tune_report r{};
    r.offset_hz = ch.offset_hz;
    r.nonfinite = 1;
    return r;
}

// what stage 3 reads of the decision between the stages
struct Turn {
    int phase;              // phi*
    int r;                  // lround(frac_hz)
    unsigned index;         // (4 (F + r)) mod 48000: the turn of sample m is W[(index * m) mod 48000]
};

inline Turn turn_of(long long F, int phase, int r) {
    return {phase, r, unsigned(mgpu_chan_detail::floor_mod(4 * (F + r), MGPU_CHAN_PHASOR_LEN))};
}

// Between the stages: G [272] complex and E [272] of one channel -> the report's metric, phase and frac_hz (or the nonfinite report)
inline Turn decide_phase(const mgpu_tune_config& k, const mgpu_chan_channel& ch, const double* G, const double* E, mgpu_tune_report* rep) {
    const long long F = centre_hz(k, ch);
    *rep = mgpu_tune_report{};
    rep->offset_hz = ch.offset_hz;
    if (!all_finite(G, size_t(kSym) * 2) || !all_finite(E, size_t(kSym))) {
        *rep = nonfinite_report(ch);
        return turn_of(F, 0, 0);
    }
    int best = 0;
    double top = G[0] * G[0] + G[1] * G[1];
    for (int phi = 1; phi < kSym; ++phi) {
        const double a = G[2 * phi] * G[2 * phi] + G[2 * phi + 1] * G[2 * phi + 1];
        if (a > top) { top = a; best = phi; }
    }
    rep->phase = best;
    rep->metric = E[best] > 0.0 ? std::sqrt(top) / E[best] : 0.0;
    const double raw = (-std::atan2(G[2 * best + 1], G[2 * best]) * 12000.0) / (2.0 * M_PI * 256.0);
    double frac = raw - double(mgpu_chan_detail::floor_mod(8 * F, 375)) / 8.0;
    if (frac < -kSpacing / 2) frac = frac + kSpacing;
    rep->frac_hz = frac;
    return turn_of(F, best, int(std::lround(frac)));
}

// Host again: Q [256] of one channel completes the report that decide_phase began
inline void decide_comb(const mgpu_tune_config& k, const mgpu_chan_channel& ch, const Turn& t, const double* Q, mgpu_tune_report* rep) {
    if (rep->nonfinite) return;
    if (!all_finite(Q, size_t(kNfft))) {
        *rep = nonfinite_report(ch);
        return;
    }
    const int K = k.search;
    double score[2 * MGPU_TUNE_MAX_SEARCH + 1];
    for (int d = -K; d <= K; ++d) {
        double acc = 0.0;
        for (int c = -kCarriers; c <= kCarriers; ++c)
            if (c != 0) acc = acc + Q[(c + d) & (kNfft - 1)];
        score[d + K] = acc;
    }
    int best = 0;
    for (int i = 1; i <= 2 * K; ++i)
        if (score[i] > score[best]) best = i;
    double second = 0.0;
    bool any = false;
    for (int i = 0; i <= 2 * K; ++i)
        if (i != best && (!any || score[i] > second)) { second = score[i]; any = true; }
    rep->shift = best - K;
    rep->contrast = any && second > 0.0 ? score[best] / second : 0.0;
    const double r = double(t.r);
    rep->delta_hz = double(rep->shift) * kSpacing + ((rep->frac_hz - r) + r);
    const double moved = double(ch.offset_hz) + rep->delta_hz, lead = k.carrier_hz - double(k.audio_centre_hz);
    const double refined = ch.sideband ? moved + lead : moved - lead;
    mgpu_chan_channel out = ch;
    out.offset_hz = int(std::lround(refined));
    rep->valid = rep->metric >= k.min_metric && !mgpu_chan_detail::channel_error(k.D, k.audio_centre_hz, &out);
    if (rep->valid) rep->offset_hz = out.offset_hz;
}

// the twin: MGPU_OK (0) or MGPU_ERR_ARG (1). G [S][272] complex, E [S][272], Q [S][256]: null where not wanted
inline int host_process(const mgpu_tune_config* kc, const mgpu_chan_channel* channels, const void* iq, int format, int n_in,
                        mgpu_tune_report* reports, double* G_out, double* E_out, double* Q_out) {
    if (config_error(kc, channels) || !iq || !reports) return 1;
    const mgpu_tune_config& k = *kc;
    const int e = mgpu_fmt::element(2, format);
    if (e == mgpu_fmt::kNone || n_in != input_samples(k)) return 1;
    const int D = k.D, J = k.symbols, M = block_samples(k);
    const mgpu_chan_config cc = chan_config_of(k);
    const std::vector<double> h = mgpu_chan_detail::prototype(&cc);
    const int T = int(h.size());
    std::vector<double> x(size_t(n_in) * 2), g(size_t(T) * 2), W(size_t(MGPU_CHAN_PHASOR_LEN) * 2);
    for (size_t i = 0; i < x.size(); ++i) x[i] = mgpu_fmt::widen_at(e, iq, i);
    mgpu_chan_detail::phasor_table(W.data());
    const mgpu_scan_detail::Tables tables(kLog2);
    std::vector<double> z(size_t(M) * 2), p(size_t(M - kNfft) * 3), G(size_t(kSym) * 2), E(size_t(kSym) * 1), Q(size_t(kNfft) * 1);
    std::vector<mgpu_scan_detail::h2> a(size_t(kNfft) * 1);
    for (int s = 0; s < k.S; ++s) {
        // stage 1
        mgpu_chan_detail::tap_row(h, D, k.audio_centre_hz, channels[s], g.data());
        for (int m = 0; m < M; ++m) {
            double re = 0.0, im = 0.0;
            for (int kk = 0; kk < T; ++kk) {
                const long long u = (long long)4 * m * D - kk;
                const double vr = u >= 0 ? x[2 * u] : 0.0, vi = u >= 0 ? x[2 * u + 1] : 0.0;
                const double gr = g[2 * kk], gi = g[2 * kk + 1];
                re = std::fma(gr, vr, re);
                re = std::fma(-gi, vi, re);
                im = std::fma(gr, vi, im);
                im = std::fma(gi, vr, im);
            }
            z[2 * size_t(m)] = re;
            z[2 * size_t(m) + 1] = im;
        }
        // stage 2
        for (int m = 0; m < M - kNfft; ++m) {
            const double ar = z[2 * size_t(m)], ai = z[2 * size_t(m) + 1], br = z[2 * size_t(m + kNfft)], bi = z[2 * size_t(m + kNfft) + 1];
            p[3 * size_t(m)] = ar * br + ai * bi;
            p[3 * size_t(m) + 1] = ai * br - ar * bi;
            p[3 * size_t(m) + 2] = 0.5 * ((ar * ar + ai * ai) + (br * br + bi * bi));
        }
        for (int phi = 0; phi < kSym; ++phi) {
            double acc[3] = {0.0, 0.0, 0.0};
            for (int j = 0; j < J; ++j) {
                double in[3] = {0.0, 0.0, 0.0};
                for (int i = 0; i < kGi; ++i)
                    for (int c = 0; c < 3; ++c) in[c] = in[c] + p[3 * size_t(kSym * j + phi + i) + c];
                for (int c = 0; c < 3; ++c) acc[c] = acc[c] + in[c];
            }
            G[2 * size_t(phi)] = acc[0];
            G[2 * size_t(phi) + 1] = acc[1];
            E[size_t(phi)] = acc[2];
        }
        const Turn t = decide_phase(k, channels[s], G.data(), E.data(), reports + s);
        // stage 3
        std::fill(Q.begin(), Q.end(), 0.0);
        for (int j = 0; j < J; ++j) {
            for (int i = 0; i < kNfft; ++i) {
                const int m = kSym * j + t.phase + kGi / 2 + i;
                const size_t w = size_t((unsigned long long)t.index * unsigned(m) % MGPU_CHAN_PHASOR_LEN);
                const double zr = z[2 * size_t(m)], zi = z[2 * size_t(m) + 1], wr = W[2 * w], wi = W[2 * w + 1];
                a[size_t(mgpu_scan_detail::brev(i, kLog2))] = {zr * wr + zi * wi, zi * wr - zr * wi};
            }
            mgpu_scan_detail::transform(a.data(), kNfft, tables);
            for (int b = 0; b < kNfft; ++b) Q[size_t(b)] = Q[size_t(b)] + (a[size_t(b)].re * a[size_t(b)].re + a[size_t(b)].im * a[size_t(b)].im);
        }
        decide_comb(k, channels[s], t, Q.data(), reports + s);
        if (G_out) std::memcpy(G_out + size_t(s) * kSym * 2, G.data(), G.size() * 8);
        if (E_out) std::memcpy(E_out + size_t(s) * kSym, E.data(), E.size() * 8);
        if (Q_out) std::memcpy(Q_out + size_t(s) * kNfft, Q.data(), Q.size() * 8);
    }
    return 0;
}

inline int host_plan(const mgpu_tune_report* report, const mgpu_chan_channel* channel, mgpu_chan_channel* refined) {
    if (!report || !channel || !refined) return 1;
    *refined = *channel;
    if (report->valid) refined->offset_hz = report->offset_hz;
    return 0;
}

}  // namespace mgpu_tune_detail

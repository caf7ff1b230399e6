// Wideband channeliser, host side (include/mercury_channelizer.h): the prototype design, the tables the device reads and the normative twin.
// Everything here is plain double arithmetic with the host's libm; the device gets these tables, so the libm's version cannot make the
// device and the twin differ.
#include <cmath>
#include <cstring>
#include <vector>

#include "chan_tables.hpp"
#include "sample_formats.h"
#include "../../include/mercury_gpu.h"

namespace mgpu_chan_detail {

const char* config_error(const mgpu_chan_config* k, bool need_s) {
    if (!k) return "no configuration";
    if (k->struct_size != int(sizeof(mgpu_chan_config))) return "mgpu_chan_config.struct_size is not sizeof(mgpu_chan_config)";
    if (k->D < 1 || k->D > MGPU_CHAN_MAX_D) return "D must be 1..64";
    if (need_s && k->S < 1) return "S must be >= 1";
    if (k->audio_centre_hz < 1 || k->audio_centre_hz >= MGPU_CHAN_PHASOR_LEN / 2) return "audio_centre_hz must be 1..23999";
    if (k->taps) {
        const int tp = (k->ntaps - 1) / k->D;
        if (k->ntaps < 1 || tp * k->D + 1 != k->ntaps || (tp & 1) || tp < 2 || tp > MGPU_CHAN_MAX_TP)
            return "ntaps must be tp * D + 1 with tp even, 2..512";
        for (int i = 0; i < k->ntaps; ++i)
            if (!std::isfinite(k->taps[i])) return "taps must be finite";
    }
    if (k->max_out < 0 || (long long)k->max_out * k->D > (1LL << 30)) return "max_out * D must be 0..2^30";
    return nullptr;
}

const char* channel_error(int D, int a_c, const mgpu_chan_channel* ch) {
    if (!ch) return "no channel";
    if (ch->sideband != 0 && ch->sideband != 1) return "sideband must be 0 (USB) or 1 (LSB)";
    if (!std::isfinite(ch->gain)) return "gain must be finite";
    const long long R = 48000LL * D;
    const long long lo = ch->sideband ? (long long)ch->offset_hz - 2 * a_c : ch->offset_hz;
    const long long hi = ch->sideband ? ch->offset_hz : (long long)ch->offset_hz + 2 * a_c;
    if (2 * lo <= -R || 2 * hi >= R) return "the channel's band leaves (-R/2, R/2)";
    return nullptr;
}

const char* plan_error(int D, int a_c, int S, const mgpu_chan_channel* channels) {
    const char* bad = channels ? nullptr : "no channels";
    for (int s = 0; !bad && s < S; ++s) bad = channel_error(D, a_c, channels + s);
    return bad;
}

namespace {

// modified Bessel function I0 by its power series (terms fall below 1e-17 of the sum within 40 for x <= 20)
double bessel_i0(double x) {
    double sum = 1, term = 1;
    const double q = x * x / 4;
    for (int m = 1; m < 200; ++m) {
        term *= q / (double(m) * m);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

}  // namespace

void windowed_sinc(int T, double fc, double atten_db, double gain, double* h) {
    const int c = (T - 1) / 2;
    const double beta = atten_db > 8.7 ? 0.1102 * (atten_db - 8.7) : 0.0;
    const double i0b = bessel_i0(beta);
    for (int k = 0; k <= c; ++k) {
        const double t = double(k - c), x = M_PI * fc * t, r = t / c;
        const double ideal = k == c ? fc : fc * std::sin(x) / x;
        h[k] = ideal * bessel_i0(beta * std::sqrt(1 - r * r)) / i0b;
    }
    // DC gain `gain` over the mirrored taps, each pair added once so that the two halves are equal to the bit
    double sum = h[c];
    for (int k = 0; k < c; ++k) sum += 2 * h[k];
    for (int k = 0; k <= c; ++k) h[k] = h[k] / sum * gain;
    for (int k = 0; k < c; ++k) h[T - 1 - k] = h[k];
}

namespace {

void design(int D, int tp, double cutoff_hz, double atten_db, double* h) {
    const double R = 48000.0 * D;
    windowed_sinc(tp * D + 1, 2 * cutoff_hz / R, atten_db, 1.0, h);
}

}  // namespace

std::vector<double> prototype(const mgpu_chan_config* k) {
    if (k->taps) return std::vector<double>(k->taps, k->taps + k->ntaps);
    std::vector<double> h(size_t(MGPU_CHAN_DEFAULT_TP) * k->D + 1);
    design(k->D, MGPU_CHAN_DEFAULT_TP, 1500.0, 60.0, h.data());
    return h;
}

void tap_row(const std::vector<double>& h, int D, int a_c, const mgpu_chan_channel& ch, double* g) {
    const int T = int(h.size()), c = (T - 1) / 2;
    const long long R = 48000LL * D, F = (long long)ch.offset_hz + (ch.sideband ? -a_c : a_c);
    for (int k = 0; k < T; ++k) {
        const long long q = floor_mod(F * (k - c), R);
        const double phi = 2 * M_PI * double(q) / double(R);
        g[2 * k] = h[k] * std::cos(phi);
        g[2 * k + 1] = h[k] * std::sin(phi);
    }
}

void phasor_table(double* W) {
    for (int p = 0; p < MGPU_CHAN_PHASOR_LEN; ++p) {
        const double a = 2 * M_PI * double(p) / double(MGPU_CHAN_PHASOR_LEN);
        W[2 * p] = std::cos(a);
        W[2 * p + 1] = std::sin(a);
    }
}

}  // namespace mgpu_chan_detail

using namespace mgpu_chan_detail;

extern "C" {

int mgpu_host_chan_design(int D, int tp, double cutoff_hz, double atten_db, double* taps, int* ntaps) {
    if (!taps || !ntaps || D < 1 || D > MGPU_CHAN_MAX_D || tp < 2 || tp > MGPU_CHAN_MAX_TP || (tp & 1)) return MGPU_ERR_ARG;
    if (!(cutoff_hz > 0) || !(cutoff_hz < 24000.0 * D) || !std::isfinite(atten_db) || atten_db < 0 || atten_db > 200) return MGPU_ERR_ARG;
    design(D, tp, cutoff_hz, atten_db, taps);
    *ntaps = tp * D + 1;
    return MGPU_OK;
}

int mgpu_host_chan_default_taps(int D, double* taps, int* ntaps) {
    return mgpu_host_chan_design(D, MGPU_CHAN_DEFAULT_TP, 1500.0, 60.0, taps, ntaps);
}

int mgpu_host_chan_tables(const mgpu_chan_config* k, const mgpu_chan_channel* channel, double* g_out, double* W_out) {
    if (config_error(k, false) || channel_error(k->D, k->audio_centre_hz, channel) || !g_out) return MGPU_ERR_ARG;
    tap_row(prototype(k), k->D, k->audio_centre_hz, *channel, g_out);
    if (W_out) phasor_table(W_out);
    return MGPU_OK;
}

int mgpu_host_chan_process(const mgpu_chan_config* k, const mgpu_chan_channel* channels, const void* iq, int format, int n_in,
                           uint64_t position, double* out) {
    if (config_error(k, true) || plan_error(k->D, k->audio_centre_hz, k->S, channels) || !iq || !out) return MGPU_ERR_ARG;
    const int D = k->D;
    const int e = mgpu_fmt::element(2, format);
    if (n_in < D || n_in % D || position > (1ULL << 62) || e == mgpu_fmt::kNone) return MGPU_ERR_ARG;
    std::vector<double> x(size_t(n_in) * 2);
    for (size_t i = 0; i < x.size(); ++i) x[i] = mgpu_fmt::widen_at(e, iq, i);
    const std::vector<double> h = prototype(k);
    const int T = int(h.size()), L = (T - 1) / D / 2, N = n_in / D;
    std::vector<double> g(size_t(T) * 2), W(size_t(MGPU_CHAN_PHASOR_LEN) * 2);
    phasor_table(W.data());
    for (int s = 0; s < k->S; ++s) {
        tap_row(h, D, k->audio_centre_hz, channels[s], g.data());
        for (int j = 0; j < N; ++j) {
            double re = 0.0, im = 0.0;
            for (int kk = 0; kk < T; ++kk) {
                const long long m = (long long)j * D - kk;            // relative to the seek: zeros before it
                const double vr = m >= 0 ? x[2 * m] : 0.0, vi = m >= 0 ? x[2 * m + 1] : 0.0;
                const double gr = g[2 * kk], gi = g[2 * kk + 1];
                re = std::fma(gr, vr, re);
                re = std::fma(-gi, vi, re);
                im = std::fma(gr, vi, im);
                im = std::fma(gi, vr, im);
            }
            const int p = phasor_index(channels[s].offset_hz, position + uint64_t(j), L);
            out[size_t(s) * N + j] = channels[s].gain * std::fma(im, W[2 * p + 1], re * W[2 * p]);
        }
    }
    return MGPU_OK;
}

}  // extern "C"

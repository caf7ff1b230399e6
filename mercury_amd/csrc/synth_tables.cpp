// Wideband synthesiser, host side (include/ext/mercury_synth.h): the tables the device reads and the normative twin. Everything here is
// plain double arithmetic with the host's libm; the device gets these tables, so the libm's version cannot make the device and the twin
// differ. The prototype, the channel check and the phasor table are the channeliser's (chan_tables.cpp).
#include <cmath>
#include <cstring>
#include <vector>

#include "synth_tables.hpp"
#include "../../include/mercury_gpu.h"

using mgpu_chan_detail::floor_mod;

namespace mgpu_synth_detail {

namespace {

// the channeliser's configuration with the same prototype: what chan_tables.cpp's checks and design read
mgpu_chan_config as_chan_config(const mgpu_synth_config* k) {
    mgpu_chan_config c{};
    c.struct_size = int(sizeof(mgpu_chan_config));
    c.D = k->D; c.S = k->S; c.audio_centre_hz = k->audio_centre_hz; c.ntaps = k->ntaps; c.taps = k->taps;
    c.max_out = 0;
    return c;
}

}  // namespace

const char* config_error(const mgpu_synth_config* k, bool need_s) {
    if (!k) return "no configuration";
    if (k->struct_size != int(sizeof(mgpu_synth_config))) return "mgpu_synth_config.struct_size is not sizeof(mgpu_synth_config)";
    const mgpu_chan_config c = as_chan_config(k);
    if (const char* bad = mgpu_chan_detail::config_error(&c, need_s)) return bad;      // D, S, audio_centre_hz, the taps
    if (k->max_in < 0 || (long long)k->max_in * k->D > (1LL << 30)) return "max_in * D must be 0..2^30";
    return nullptr;
}

std::vector<double> prototype(const mgpu_synth_config* k) {
    const mgpu_chan_config c = as_chan_config(k);
    return mgpu_chan_detail::prototype(&c);
}

void tap_table(const std::vector<double>& h, int D, int a_c, double* q) {
    const int T = int(h.size()), c = (T - 1) / 2;
    const long long R = 48000LL * D;
    for (int k = 0; k < T; ++k) {
        const long long t = floor_mod((long long)a_c * (k - c), R);
        const double phi = 2 * M_PI * double(t) / double(R);
        q[2 * k] = h[k] * std::cos(phi);
        q[2 * k + 1] = h[k] * std::sin(phi);
    }
}

void phase_row(int D, int offset_hz, double* P) {
    const long long R = 48000LL * D;
    for (int r = 0; r < D; ++r) {
        const long long t = floor_mod((long long)offset_hz * r, R);
        const double phi = 2 * M_PI * double(t) / double(R);
        P[2 * r] = std::cos(phi);
        P[2 * r + 1] = std::sin(phi);
    }
}

}  // namespace mgpu_synth_detail

using namespace mgpu_synth_detail;

extern "C" {

int mgpu_host_synth_tables(const mgpu_synth_config* k, const mgpu_chan_channel* channel, double* q_out, double* P_out, double* G_out,
                           double* W_out) {
    if (config_error(k, false) || mgpu_chan_detail::channel_error(k->D, k->audio_centre_hz, channel) || !q_out || !P_out || !G_out)
        return MGPU_ERR_ARG;
    const std::vector<double> h = prototype(k);
    tap_table(h, k->D, k->audio_centre_hz, q_out);
    if (channel->sideband)
        for (size_t i = 0; i < h.size(); ++i) q_out[2 * i + 1] = -q_out[2 * i + 1];
    phase_row(k->D, channel->offset_hz, P_out);
    *G_out = channel_gain(k->D, channel->gain);
    if (W_out) mgpu_chan_detail::phasor_table(W_out);
    return MGPU_OK;
}

int mgpu_host_synth_process(const mgpu_synth_config* k, const mgpu_chan_channel* channels, const double* audio, size_t in_stride, int n_in,
                            uint64_t position, int format, void* out, uint64_t* clamped) {
    if (config_error(k, true) || mgpu_chan_detail::plan_error(k->D, k->audio_centre_hz, k->S, channels) || !audio || !out) return MGPU_ERR_ARG;
    if (n_in < 1 || (long long)n_in * k->D > (1LL << 30) || in_stride < size_t(n_in) || !mgpu_fmt::iq_bytes(format)) return MGPU_ERR_ARG;
    if (position > kMaxPosition || position + uint64_t(n_in) > kMaxPosition) return MGPU_ERR_ARG;
    const int D = k->D, S = k->S;
    const std::vector<double> h = prototype(k);
    const int T = int(h.size()), tp = (T - 1) / D;
    std::vector<double> q(size_t(T) * 2), W(size_t(MGPU_CHAN_PHASOR_LEN) * 2), P(size_t(S) * D * 2);
    tap_table(h, D, k->audio_centre_hz, q.data());
    mgpu_chan_detail::phasor_table(W.data());
    for (int s = 0; s < S; ++s) phase_row(D, channels[s].offset_hz, P.data() + size_t(s) * D * 2);
    uint64_t count = 0;
    for (int n = 0; n < n_in; ++n) {
        for (int r = 0; r < D; ++r) {
            const int J = r ? tp - 1 : tp;
            double re = 0.0, im = 0.0;
            for (int s = 0; s < S; ++s) {
                const double sign = channels[s].sideband ? -1.0 : 1.0;         // q-: the conjugate exactly
                const double* a = audio + size_t(s) * in_stride;
                double vr = 0.0, vi = 0.0;
                for (int j = 0; j <= J; ++j) {
                    const size_t t = size_t(j) * D + r;
                    const double x = j <= n ? a[n - j] : 0.0;                  // relative to the seek: zeros before it
                    vr = std::fma(q[2 * t], x, vr);
                    vi = std::fma(sign * q[2 * t + 1], x, vi);
                }
                const int p = carrier_index(channels[s].offset_hz, position + uint64_t(n));
                const double er = W[2 * p], ei = W[2 * p + 1];
                const double pr = P[(size_t(s) * D + r) * 2], pi = P[(size_t(s) * D + r) * 2 + 1];
                const double Er = std::fma(-ei, pi, er * pr), Ei = std::fma(ei, pr, er * pi);
                const double G = channel_gain(D, channels[s].gain);
                re += G * std::fma(-vi, Ei, vr * Er);
                im += G * std::fma(vi, Er, vr * Ei);
            }
            count += mgpu_fmt::store_iq(out, format, size_t(n) * D + r, re, im);
        }
    }
    if (clamped) *clamped = count;
    return MGPU_OK;
}

}  // extern "C"

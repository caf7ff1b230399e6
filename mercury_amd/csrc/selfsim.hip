// The two BER self-simulations (include/mercury_gpu.h, mercury_rxloop.h, mercury_channel.h) and the noise level their audio path shares
// with the link simulator.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ctx.hpp"
#include "../../include/mercury_tx.h"

// sigma of passband_test_EsN0's AWGN in the reference's types (telecom_system.cc:236-239 for OFDM, from Es/N0 alone; :266-279 for MFSK, from
// the first frame's mean power), then awgn.cc:68's share of each component
double mgpu_detail::audio_noise_amplitude(const mgpu::ModeTables& t, double esn0_db, double mean_power) {
    const float sigma = t.mfsk_M > 0
        ? float(std::sqrt(2.0 * mean_power * (kSampleRate / 2.0) / (std::pow(10.0, double(float(esn0_db)) / 10.0) * kBandwidthHz)))
        : 1.0f / float(std::sqrt(std::pow(10.0f, float(esn0_db) / 10.0f)));
    return double(sigma / std::sqrt(2.0f));
}

extern "C" {

// hf: NULL = the generator's own channel (mgpu_baseband_test_esn0), else the HF channel between the clean frame and the same noise
static int baseband_test_esn0_impl(mgpu_ctx* c, const double* esn0_db, int npoints, long long frames_per_point, uint64_t seed, uint64_t frame0,
                                   int channel, const mgpu_hf_channel* hf, mgpu_error_rate* out) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        if (hf) hf_check(hf);
        need(esn0_db && out && npoints > 0 && frames_per_point > 0 && (channel == 0 || channel == 1), "bad argument");
        const auto& t = c->tab;
        const int B = int(std::min<long long>(frames_per_point, c->max_batch));
        ensure_workspaces(c, WS_FRONTEND | WS_LLR | WS_OUT);
        DevBuf d_bb(size_t(B) * t.frame_samples * 16), d_sent(size_t(B) * t.payload_stride), d_acc(4 * 8);
        DevBuf d_clean(hf ? size_t(B) * t.frame_samples * 16 : 0);
        hipStream_t s = c->stream;
        for (int p = 0; p < npoints; ++p) {
            const double noise_amp = std::pow(10.0, -esn0_db[p] / 20.0) / std::sqrt(2.0);      // per component, telecom_system.cc:100,147
            HIPCK(hipMemsetAsync(d_acc.p, 0, 32, s));
            for (long long done = 0; done < frames_per_point; done += B) {
                const int n = int(std::min<long long>(B, frames_per_point - done));
                const uint64_t first = frame0 + uint64_t(p) * uint64_t(frames_per_point) + uint64_t(done);
                launch_txgen(c, seed, first, n, hf ? 0.0 : noise_amp, channel, (hf ? d_clean : d_bb).as<double>(), d_sent.as<uint8_t>(), s);
                if (hf) launch_hf_baseband(hf, d_clean.as<double>(), t.frame_samples, noise_amp, seed, first, n, d_bb.as<double>(), s);
                SpanIo io = own_span(c);
                io.bb = d_bb.as<double>();
                io.zf_snr = false;           // the error counter does not read snr_db: one launch less per batch in the zero-forcing modes
                launch_span(c, io, n, MgpuTapsDev{}, s);
                hipLaunchKernelGGL(mgpu_error_count_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_sent.as<uint8_t>(), c->d_payload, c->d_stats,
                                   t.payload_stride, t.nReal, n, d_acc.as<unsigned long long>());
                HIPCK(hipGetLastError());
            }
            unsigned long long acc[4];
            HIPCK(hipMemcpyAsync(acc, d_acc.p, 32, hipMemcpyDeviceToHost, s));
            HIPCK(hipStreamSynchronize(s));
            mgpu_error_rate& r = out[p];
            r.esn0_db = esn0_db[p];
            r.Frames_total = frames_per_point; r.Error_frames_total = (long long)acc[1];
            r.Bits_total = frames_per_point * t.nReal; r.Error_bits_total = (long long)acc[0];
            r.BER = double(r.Error_bits_total) / double(r.Bits_total);
            r.FER = double(r.Error_frames_total) / double(r.Frames_total);
            r.avg_iterations = double(acc[2]) / double(frames_per_point);
            r.crc_ok_frames = (long long)acc[3];
        }
    });
}

int mgpu_baseband_test_esn0(mgpu_ctx* c, const double* esn0_db, int npoints, long long frames_per_point, uint64_t seed, uint64_t frame0, int channel,
                            mgpu_error_rate* out) {
    return baseband_test_esn0_impl(c, esn0_db, npoints, frames_per_point, seed, frame0, channel, nullptr, out);
}

int mgpu_baseband_test_esn0_hf(mgpu_ctx* c, const double* esn0_db, int npoints, long long frames_per_point, uint64_t seed, uint64_t frame0,
                               const mgpu_hf_channel* ch, mgpu_error_rate* out) {
    if (!c) return MGPU_ERR_ARG;
    if (!ch) return refuse(c, MGPU_ERR_ARG, "no channel");
    return baseband_test_esn0_impl(c, esn0_db, npoints, frames_per_point, seed, frame0, 0, ch, out);
}

// cl_telecom_system::passband_test_EsN0 (telecom_system.cc:231-330) per Es/N0 point, batched: random payloads -> transmit_byte
// (SINGLE_MESSAGE) -> apply_with_delay (AWGN on the audio, the frame `delay` samples into the capture window) -> receive_byte ->
// cl_error_rate::check over the payload bits. Everything stays on the device except the per-window results receive_byte returns.
// ch: NULL = AWGN alone (mgpu_passband_test_esn0), else the HF channel in front of the same noise (mgpu_passband_test_esn0_hf)
static int passband_test_esn0_impl(mgpu_ctx* c, const double* esn0_db, int npoints, long long frames_per_point, uint64_t seed, uint64_t frame0,
                                   double carrier_hz, double output_power_watt, const mgpu_hf_channel* ch, mgpu_error_rate* out, double* windows_out,
                                   uint8_t* sent_out) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(esn0_db && out && npoints > 0 && frames_per_point > 0 && output_power_watt > 0, "bad argument");
        const auto& t = c->tab;
        const bool mfsk = t.mfsk_M > 0;
        const int total = mgpu_transmit_frame_samples(c);
        const int window = t.Nofdm * mgpu_receive_buffer_nsymb(c) * kInterp;
        const int delay = ((t.preamble + 2) * t.Nofdm + (t.Nfft == 1024 ? 100 : 50)) * kInterp;           // :242-249, :292
        need(delay + total <= window, "the frame does not fit the capture window behind the test delay");
        const int B = int(std::min<long long>(frames_per_point, std::min(c->max_batch, 1024)));            // 1024 windows = 0.76 GB of audio
        const int stride = t.payload_stride, nbytes = t.payload_bytes;
        DevBuf d_pl(size_t(B) * stride), d_audio(size_t(B) * total * 8), d_win(size_t(B) * window * 8);
        std::vector<uint8_t> sent(size_t(B) * stride), got(size_t(B) * stride);
        std::vector<mgpu_receive_stats> st(B);
        std::vector<mgpu_link_state> ls(B);
        const mgpu_transmit_config txc = {carrier_hz, kCarrierAmplitude, output_power_watt, 7.0, 10.0, 0, MGPU_SINGLE_MESSAGE, 0};   // physical_config.cc defaults
        const mgpu_receive_config rxc = {carrier_hz, 2, 1, 1, 0};
        hipStream_t s = c->stream;
        for (int p = 0; p < npoints; ++p) {
            double ampl = mfsk ? 0.0 : audio_noise_amplitude(t, esn0_db[p], 0.0);
            bool calibrated = !mfsk;                   // :266-279 calibrates once per point, from the first frame's power
            long long be = 0, fe = 0, ok = 0;
            double iters = 0;
            for (long long done = 0; done < frames_per_point; done += B) {
                const int n = int(std::min<long long>(B, frames_per_point - done));
                const uint64_t first = frame0 + uint64_t(p) * uint64_t(frames_per_point) + uint64_t(done);
                hipLaunchKernelGGL(mgpu_gen_payload_kernel, dim3(n), dim3(256), 0, s, seed, first, n, nbytes, stride, d_pl.as<uint8_t>());
                HIPCK(hipGetLastError());
                if (mgpu_transmit_byte_batch_dev(c, d_pl.p, stride, nullptr, n, &txc, d_audio.p, s) != MGPU_OK) throw std::runtime_error(std::string(c->err));
                if (!calibrated) {
                    std::vector<double> a0(total);
                    HIPCK(hipMemcpyAsync(a0.data(), d_audio.p, size_t(total) * 8, hipMemcpyDeviceToHost, s));
                    HIPCK(hipStreamSynchronize(s));
                    double psig = 0;
                    for (int i = 0; i < total; ++i) psig += a0[i] * a0[i];
                    psig /= total;
                    ampl = audio_noise_amplitude(t, esn0_db[p], psig);
                    calibrated = true;
                }
                if (ch) {
                    launch_hf_passband(ch, d_audio.as<double>(), total, delay, window, ampl, seed, first, n, d_win.as<double>(), s);
                } else {
                    hipLaunchKernelGGL(mgpu_passband_channel_kernel, dim3((window + 255) / 256, n), dim3(256), 0, s, d_audio.as<double>(), total, delay, window,
                                       ampl, seed, first, n, d_win.as<double>());
                    HIPCK(hipGetLastError());
                }
                HIPCK(hipMemcpyAsync(sent.data(), d_pl.p, size_t(n) * stride, hipMemcpyDeviceToHost, s));
                if (windows_out) HIPCK(hipMemcpyAsync(windows_out + (size_t(p) * frames_per_point + done) * window, d_win.p, size_t(n) * window * 8, hipMemcpyDeviceToHost, s));
                HIPCK(hipStreamSynchronize(s));
                if (sent_out) std::memcpy(sent_out + (size_t(p) * frames_per_point + done) * stride, sent.data(), size_t(n) * stride);
                for (int w = 0; w < n; ++w) ls[w] = mgpu_link_state{-1, 0.0, 0, mfsk ? delay + 1 : 0};      // :293-296 mfsk_fixed_delay
                receive_byte_impl(c, d_win.as<double>(), n, &rxc, ls.data(), got.data(), st.data());
                for (int w = 0; w < n; ++w) {
                    int e = 0;
                    for (int b = 0; b < nbytes; ++b) e += __builtin_popcount(unsigned(sent[size_t(w) * stride + b] ^ got[size_t(w) * stride + b]));
                    be += e; fe += e != 0; ok += st[w].message_decoded != 0;
                    iters += st[w].iterations_done > 0 ? st[w].iterations_done : 0;
                }
            }
            mgpu_error_rate& r = out[p];
            r.esn0_db = esn0_db[p];
            r.Frames_total = frames_per_point; r.Error_frames_total = fe;
            r.Bits_total = frames_per_point * nbytes * 8; r.Error_bits_total = be;
            r.BER = double(be) / double(r.Bits_total); r.FER = double(fe) / double(frames_per_point);
            r.avg_iterations = iters / double(frames_per_point);
            r.crc_ok_frames = ok;
        }
    });
}

int mgpu_passband_test_esn0(mgpu_ctx* c, const double* esn0_db, int npoints, long long frames_per_point, uint64_t seed, uint64_t frame0,
                                       double carrier_hz, double output_power_watt, mgpu_error_rate* out, double* windows_out, uint8_t* sent_out) {
    return passband_test_esn0_impl(c, esn0_db, npoints, frames_per_point, seed, frame0, carrier_hz, output_power_watt, nullptr, out, windows_out,
                                   sent_out);
}

int mgpu_passband_test_esn0_hf(mgpu_ctx* c, const double* esn0_db, int npoints, long long frames_per_point, uint64_t seed, uint64_t frame0,
                                          double carrier_hz, double output_power_watt, const mgpu_hf_channel* ch, mgpu_error_rate* out,
                                          double* windows_out, uint8_t* sent_out) {
    if (!c) return MGPU_ERR_ARG;
    const int rc = guard(c, [&] { hf_check(ch); });     // a bad channel is refused before any device work
    if (rc != MGPU_OK) return rc;
    return passband_test_esn0_impl(c, esn0_db, npoints, frames_per_point, seed, frame0, carrier_hz, output_power_watt, ch, out, windows_out,
                                   sent_out);
}

}  // extern "C"

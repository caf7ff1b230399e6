// The synchroniser's building blocks as blocking host-buffer calls (include/mercury_gpu.h): upload, one kernel family, download; and the
// debug probes the tests hold against the oracle.
#include <vector>

#include "ctx.hpp"

namespace {
// carrier energies of every symbol slot of W windows: [W][nslots][50] on the host
// `passband_carrier_hz` >= 0: `bb` is real passband audio ([W][size] doubles) that is first mixed down and filtered with
// FIR_rx_data on the device (detect_ack_pattern_from_passband, telecom_system.cc:1628-1640); otherwise it is interpolated
// baseband ([W][size] complex).
// d_e ([W][nslots][Nc] doubles on the device) receives the energies; want_host: also returned on the host
std::vector<double> slot_energies(mgpu_ctx* c, const double* bb, int W, int size, int nslots, double passband_carrier_hz, DevBuf& d_e, bool want_host) {
    const auto& t = c->tab;
    DevBuf d_in(size_t(W) * size * 16);
    hipStream_t s = c->stream;
    if (passband_carrier_hz >= 0) {
        DevBuf d_pass(size_t(W) * size * 8), d_fc(size_t(W) * 8);
        std::vector<double> fc(W, passband_carrier_hz);
        HIPCK(hipMemcpyAsync(d_pass.p, bb, size_t(W) * size * 8, hipMemcpyHostToDevice, s));
        HIPCK(hipMemcpyAsync(d_fc.p, fc.data(), size_t(W) * 8, hipMemcpyHostToDevice, s));
        const int ntaps = int(t.fir_data.size());
        const double* cs = mixer_table(c, passband_carrier_hz, size_t(size), s);
        launch_p2b(d_pass.as<double>(), size, d_fc.as<double>(), nullptr, 0, size, 1, c->d_fir[1], ntaps, d_in.as<double>(), nullptr, cs, nullptr, 0, W, s);
        HIPCK(hipStreamSynchronize(s));          // d_pass / d_fc go out of scope here
    } else {
        HIPCK(hipMemcpyAsync(d_in.p, bb, size_t(W) * size * 16, hipMemcpyHostToDevice, s));
    }
    HIPCK(hipMemsetAsync(d_e.p, 0, size_t(W) * nslots * t.Nc * 8, s));
    HIPCK(hipEventRecord(c->sync_ev[0], s));
    hipLaunchKernelGGL(mgpu_slot_energy_kernel, dim3((nslots + 3) / 4, W), dim3(256), 0, s, d_in.as<double>(), size, nslots, kInterp,
                       c->dev.twiddle, d_e.as<double>());
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(c->sync_ev[1], s));
    std::vector<double> e;
    if (want_host) {
        e.resize(size_t(W) * nslots * t.Nc);
        HIPCK(hipMemcpyAsync(e.data(), d_e.p, e.size() * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCK(hipStreamSynchronize(s));              // d_in goes out of scope here
    return e;
}
std::vector<double> slot_energies(mgpu_ctx* c, const double* bb, int W, int size, int nslots, double passband_carrier_hz = -1.0) {
    DevBuf d_e(size_t(W) * nslots * c->tab.Nc * 8);
    return slot_energies(c, bb, W, size, nslots, passband_carrier_hz, d_e, true);
}
}  // namespace

extern "C" {

// ---- synchroniser building blocks (host-buffer, blocking) ---------------------------------------
int mgpu_passband_to_baseband(mgpu_ctx* c, const double* passband, int W, int in_size, const double* carrier_hz, int filter,
                              const int* start, int count, int decimation, double* out_c128) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(passband && carrier_hz && out_c128 && W > 0 && in_size > 0 && count > 0 && decimation >= 1 && (filter == 0 || filter == 1),
             "bad argument");
        const auto& taps = filter ? c->tab.fir_data : c->tab.fir_time_sync;
        DevBuf d_in(size_t(W) * in_size * 8), d_fc(size_t(W) * 8), d_out(size_t(W) * count * 16), d_start(size_t(W) * 4);
        Io io(c);
        io.up(d_in, passband, size_t(W) * in_size * 8);
        io.up(d_fc, carrier_hz, size_t(W) * 8);
        if (start) io.up(d_start, start, size_t(W) * 4);
        const int ntaps = int(taps.size());
        bool shared = true;                                           // one carrier for every window: the host-libm mixer table applies
        for (int w = 1; w < W; ++w) shared = shared && carrier_hz[w] == carrier_hz[0];
        const double* cs = shared ? mixer_table(c, carrier_hz[0], size_t(in_size), io.s) : nullptr;
        HIPCK(hipEventRecord(c->sync_ev[0], io.s));
        launch_p2b(d_in.as<double>(), in_size, d_fc.as<double>(), start ? d_start.as<int>() : nullptr, 0, count, decimation, c->d_fir[filter], ntaps,
                   d_out.as<double>(), nullptr, cs, nullptr, 0, W, io.s);
        HIPCK(hipEventRecord(c->sync_ev[1], io.s));
        io.down(out_c128, d_out, size_t(W) * count * 16);
    });
}

int mgpu_time_sync_preamble(mgpu_ctx* c, const double* bb, int W, int size, int step, int location_to_return, int nTrials_max,
                            int* delay, double* correlation) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        const auto& t = c->tab;
        const int sym = t.Nofdm * kInterp, L = t.preamble * sym;
        need(bb && delay && W > 0 && size > L && step >= 1 && nTrials_max >= 1 && nTrials_max <= size, "bad argument");
        const int ncand = (size - L + step - 1) / step;
        DevBuf d_in(size_t(W) * size * 16), d_vals(size_t(W) * ncand * 8);
        Io io(c);
        io.up(d_in, bb, size_t(W) * size * 16);
        HIPCK(hipEventRecord(c->sync_ev[0], io.s));
        const int ngi_i = t.Ngi * kInterp, nfft_i = t.Nfft * kInterp;
        launch_tsync_metric(d_in.as<double>(), size, nullptr, nullptr, nullptr, ncand, W, step, t.preamble, ngi_i, nfft_i, d_vals.as<double>(), io.s);
        HIPCK(hipGetLastError());
        HIPCK(hipEventRecord(c->sync_ev[1], io.s));
        std::vector<double> cand(size_t(W) * ncand);
        io.down(cand.data(), d_vals, cand.size() * 8);
        for (int w = 0; w < W; ++w) {
            double corr = 0;
            select_peak(&cand[size_t(w) * ncand], ncand, step, size, location_to_return, nTrials_max, &delay[w], &corr);
            if (correlation) correlation[w] = corr;
        }
    });
}

int mgpu_debug_select_peak(mgpu_ctx* c, const double* cand_vals, int n, int ncand_max, const int* ncand, const int* size, const int* loc, int step,
                           int nTrials_max, int* delay, double* corr) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(cand_vals && ncand && size && loc && delay && corr && n > 0 && ncand_max > 0 && step >= 1 && nTrials_max >= 1, "bad argument");
        DevBuf d_v(size_t(n) * ncand_max * 8), d_nc(size_t(n) * 4), d_sz(size_t(n) * 4), d_lc(size_t(n) * 4), d_d(size_t(n) * 4), d_c(size_t(n) * 8);
        Io io(c);
        io.up(d_v, cand_vals, size_t(n) * ncand_max * 8);
        io.up(d_nc, ncand, size_t(n) * 4);
        io.up(d_sz, size, size_t(n) * 4);
        io.up(d_lc, loc, size_t(n) * 4);
        hipLaunchKernelGGL(mgpu_select_peak_kernel, dim3(n), dim3(64), 0, io.s, d_v.as<double>(), d_nc.as<int>(), ncand_max, step, d_sz.as<int>(), d_lc.as<int>(),
                           nTrials_max, n, d_d.as<int>(), d_c.as<double>());
        HIPCK(hipGetLastError());
        io.back(delay, d_d, size_t(n) * 4);
        io.down(corr, d_c, size_t(n) * 8);
    });
}

int mgpu_debug_occupancy(mgpu_ctx* c, int which) {
    if (!c) return -1;
    int n = -1;
    guard(c, [&] {
        const auto& t = c->tab;
        if (which == 0 && t.mfsk_M == 0) HIPCK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, mgpu_frontend_form_kernel(c->fe_threads, 0), c->fe_threads, c->lds_fe));
        else if (which == 0) HIPCK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, t.mfsk_M == 32 ? mgpu_mfsk_frontend_kernel_m32 : mgpu_mfsk_frontend_kernel_m16x2, 256, 0));
        else if (which == 1) n = int(c->lds_fe);          // dynamic LDS bytes of the front-end workgroup
        else if (which == 2) n = int(c->lds_dec);         // ... of the decoder workgroup
        else if (which == 3) n = c->dec_threads;
        else n = -1;
    });
    return n;
}

int mgpu_debug_tsync_metric(mgpu_ctx* c, const double* bb, int W, int size, int step, int variant, const int* start, const int* sub_size, double* vals) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        const auto& t = c->tab;
        const int sym = t.Nofdm * kInterp, L = t.preamble * sym;
        need(bb && vals && W > 0 && size > L && step >= 1 && variant >= -1 && variant <= 2 && (!start == !sub_size), "bad argument");
        const int ncand = (size - L + step - 1) / step;
        std::vector<int> nc(W, ncand), st(W, 0), wi(W);
        for (int w = 0; w < W; ++w) {
            wi[w] = w;
            if (start) {
                need(start[w] >= 0 && sub_size[w] >= 0 && start[w] + sub_size[w] <= size, "sub-window outside the window");
                st[w] = start[w];
                nc[w] = sub_size[w] > L ? (sub_size[w] - L + step - 1) / step : 0;
            }
        }
        DevBuf d_in(size_t(W) * size * 16), d_vals(size_t(W) * ncand * 8), d_st(size_t(W) * 4), d_nc(size_t(W) * 4), d_wi(size_t(W) * 4);
        Io io(c);
        io.up(d_in, bb, size_t(W) * size * 16);
        io.up(d_st, st.data(), size_t(W) * 4);
        io.up(d_nc, nc.data(), size_t(W) * 4);
        io.up(d_wi, wi.data(), size_t(W) * 4);
        HIPCK(hipMemsetAsync(d_vals.p, 0xff, size_t(W) * ncand * 8, io.s));
        HIPCK(hipEventRecord(c->sync_ev[0], io.s));
        launch_tsync_metric(d_in.as<double>(), size, start ? d_st.as<int>() : nullptr, start ? d_wi.as<int>() : nullptr, start ? d_nc.as<int>() : nullptr, ncand, W, step,
                            t.preamble, t.Ngi * kInterp, t.Nfft * kInterp, d_vals.as<double>(), io.s, variant);
        HIPCK(hipEventRecord(c->sync_ev[1], io.s));
        io.down(vals, d_vals, size_t(W) * ncand * 8);
    });
}

int mgpu_debug_mfsk_sync(mgpu_ctx* c, const double* energy, int W, int nslots, int size, const int* search_start, int variant, int* delay) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        const auto& t = c->tab;
        need(t.mfsk_M > 0, "MFSK modes only (cfg 100..102)");
        need(energy && delay && W > 0 && nslots >= t.preamble && size > 0 && (variant == 0 || variant == 1), "bad argument");
        if (variant == 0) {
            for (int w = 0; w < W; ++w) delay[w] = mfsk_sync_from_energies(t, energy + size_t(w) * nslots * t.Nc, nslots, size, search_start ? search_start[w] : 0);
            return;
        }
        DevBuf d_e(size_t(W) * nslots * t.Nc * 8), d_ss(size_t(W) * 4), d_delay(size_t(W) * 4);
        Io io(c);
        io.up(d_e, energy, size_t(W) * nslots * t.Nc * 8);
        if (search_start) io.up(d_ss, search_start, size_t(W) * 4);
        launch_mfsk_sync(c, d_e.as<double>(), W, nslots, size, search_start ? d_ss.as<int>() : nullptr, d_delay.as<int>(), io.s);
        io.down(delay, d_delay, size_t(W) * 4);
    });
}

int mgpu_debug_span_energy(mgpu_ctx* c, const double* bb, int W, int size, const int* wv, const int* off, int n, int len, int variant, double* sum, int* cnt) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(bb && wv && off && sum && cnt && W > 0 && size > 0 && n > 0 && len > 0 && len <= 1088 && (variant == 0 || variant == 1), "bad argument");
        for (int j = 0; j < n; ++j) need(wv[j] >= 0 && wv[j] < W && off[j] >= 0, "span outside the windows");
        DevBuf d_in(size_t(W) * size * 16), d_wv(size_t(n) * 4), d_off(size_t(n) * 4), d_sum(size_t(n) * 8), d_cnt(size_t(n) * 4);
        Io io(c);
        io.up(d_in, bb, size_t(W) * size * 16);
        io.up(d_wv, wv, size_t(n) * 4);
        io.up(d_off, off, size_t(n) * 4);
        HIPCK(hipEventRecord(c->sync_ev[0], io.s));
        if (variant)
            hipLaunchKernelGGL(mgpu_span_energy_many_kernel, dim3((n + 255) / 256), dim3(256), 0, io.s, d_in.as<double>(), size, d_wv.as<int>(), d_off.as<int>(), n, len,
                               d_sum.as<double>(), d_cnt.as<int>());
        else
            hipLaunchKernelGGL(mgpu_span_energy_kernel, dim3((n + 3) / 4), dim3(256), 0, io.s, d_in.as<double>(), size, d_wv.as<int>(), d_off.as<int>(), n, len,
                               d_sum.as<double>(), d_cnt.as<int>());
        HIPCK(hipGetLastError());
        HIPCK(hipEventRecord(c->sync_ev[1], io.s));
        io.back(sum, d_sum, size_t(n) * 8);
        io.down(cnt, d_cnt, size_t(n) * 4);
    });
}

int mgpu_freq_sync(mgpu_ctx* c, const double* bb, int W, int stride, double* freq_offset_hz) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        const auto& t = c->tab;
        int pre_half = t.preamble / 2 == 0 ? 1 : t.preamble / 2;            // ofdm.cc:548-555
        need(bb && freq_offset_hz && W > 0 && stride >= pre_half * t.Nofdm, "bad argument");
        DevBuf d_in(size_t(W) * stride * 16), d_out(size_t(W) * 16);
        Io io(c);
        io.up(d_in, bb, size_t(W) * stride * 16);
        HIPCK(hipEventRecord(c->sync_ev[0], io.s));
        hipLaunchKernelGGL(mgpu_fsync_kernel, dim3(W), dim3(256), 0, io.s, d_in.as<double>(), stride, pre_half, c->dev.twiddle, d_out.as<double>());
        HIPCK(hipGetLastError());
        HIPCK(hipEventRecord(c->sync_ev[1], io.s));
        std::vector<double> mul(size_t(W) * 2);
        io.down(mul.data(), d_out, size_t(W) * 16);
        for (int w = 0; w < W; ++w) freq_offset_hz[w] = moose_hz(mul[2 * w], mul[2 * w + 1], kBandwidthHz / double(t.Nc));
    });
}

// ---- MFSK synchroniser / signalling blocks (host buffers, blocking) -----------------------------------
int mgpu_time_sync_mfsk(mgpu_ctx* c, const double* bb, int W, int size, int search_start_symb, int* delay) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        const auto& t = c->tab;
        need(t.mfsk_M > 0, "time_sync_mfsk needs an MFSK mode (cfg 100..102)");
        const int sym_period = t.Nofdm * kInterp, nslots = size / sym_period, np = t.preamble;
        need(bb && delay && W > 0 && nslots >= np, "bad argument");
        if (W == 1) {                                                // one window: 260 KB of energies, the search on the host
            const std::vector<double> E = slot_energies(c, bb, W, size, nslots);
            delay[0] = mfsk_sync_from_energies(t, E.data(), nslots, size, search_start_symb);
            return;
        }
        DevBuf d_e(size_t(W) * nslots * t.Nc * 8), d_ss(size_t(W) * 4), d_delay(size_t(W) * 4);
        slot_energies(c, bb, W, size, nslots, -1.0, d_e, false);
        const std::vector<int> ss(W, search_start_symb);
        HIPCK(hipMemcpyAsync(d_ss.p, ss.data(), size_t(W) * 4, hipMemcpyHostToDevice, c->stream));
        launch_mfsk_sync(c, d_e.as<double>(), W, nslots, size, d_ss.as<int>(), d_delay.as<int>(), c->stream);
        HIPCK(hipMemcpyAsync(delay, d_delay.p, size_t(W) * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
    });
}

static int detect_ack_impl(mgpu_ctx* c, const double* bb, int W, int size, int pattern, double passband_carrier_hz, double* metric_out,
                           int* matched_out) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        const auto& t = c->tab;
        const int sym_period = t.Nofdm * kInterp, nslots = size / sym_period;
        need(bb && metric_out && W > 0 && size > 0 && (pattern == 1 || pattern == 2) && t.Nc == 50, "bad argument");
        if (nslots < kAckNsymb) {                                      // ofdm.cc:2075
            for (int w = 0; w < W; ++w) { metric_out[w] = 0.0; if (matched_out) matched_out[w] = 0; }
            return;
        }
        const std::vector<double> E = slot_energies(c, bb, W, size, nslots, passband_carrier_hz);
        const int* tones = pattern == 2 ? kBreakTones : kAckTones;
        for (int w = 0; w < W; ++w) {                                  // ofdm.cc:2085-2178
            double best_metric = 0.0;
            int best_matched = 0;
            for (int s = 0; s <= nslots - kAckNsymb; ++s) {
                double metric = 0;
                int matched = 0;
                for (int p = 0; p < kAckNsymb; ++p) {
                    if ((s + p) * sym_period + t.Ngi * kInterp + t.Nfft * kInterp > size) break;
                    const double* e = &E[(size_t(w) * nslots + s + p) * t.Nc];
                    const int actual = (tones[p % kAckLen] + p * kAckHop) % kAckM;
                    const double e_expected = e[kAckOffset + actual];
                    double e_target = 0;
                    e_target += e_expected;
                    double peak_e = -1.0;
                    for (int q = 0; q < kAckM; ++q) if (e[kAckOffset + q] > peak_e) peak_e = e[kAckOffset + q];
                    if (!(e_expected >= peak_e)) continue;             // the expected tone must be the band's peak
                    ++matched;
                    double e_total = 0;
                    for (int k = 0; k < t.Nc; ++k) e_total += e[k];
                    if (e_total > 0) metric += e_target / e_total;
                }
                if (metric > best_metric) { best_metric = metric; best_matched = matched; }
            }
            metric_out[w] = best_metric;
            if (matched_out) matched_out[w] = best_matched;
        }
    });
}

int mgpu_detect_ack_pattern(mgpu_ctx* c, const double* bb, int W, int size, int pattern, double* metric_out, int* matched_out) {
    return detect_ack_impl(c, bb, W, size, pattern, -1.0, metric_out, matched_out);
}

int mgpu_detect_ack_pattern_from_passband(mgpu_ctx* c, const double* passband, int W, int size, double carrier_hz, int pattern,
                                          double* metric_out, int* matched_out) {
    if (!(carrier_hz >= 0)) return MGPU_ERR_ARG;
    return detect_ack_impl(c, passband, W, size, pattern, carrier_hz, metric_out, matched_out);
}

int mgpu_last_sync_kernel_ms(mgpu_ctx* c, float* ms) {
    if (!c || !ms) return MGPU_ERR_ARG;
    return guard(c, [&] {
        HIPCK(hipEventSynchronize(c->sync_ev[1]));
        HIPCK(hipEventElapsedTime(ms, c->sync_ev[0], c->sync_ev[1]));
    });
}

int mgpu_debug_spa_math(mgpu_ctx* c, const double* in, int n, double* tanh_out, double* atanh_out) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(in && tanh_out && atanh_out && n > 0, "bad argument");
        DevArray<double> d_in(size_t(n) * 8), d_t(size_t(n) * 8), d_a(size_t(n) * 8);
        HIPCK(hipMemcpy(d_in, in, size_t(n) * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(mgpu_spa_math_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, d_in, d_t, d_a, n);
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(c->stream));
        HIPCK(hipMemcpy(tanh_out, d_t, size_t(n) * 8, hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(atanh_out, d_a, size_t(n) * 8, hipMemcpyDeviceToHost));
    });
}

int mgpu_debug_glibc_trig(mgpu_ctx* c, const double* in, int n, double* atan_out, double* sin_out, double* cos_out) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(in && atan_out && sin_out && cos_out && n > 0, "bad argument");
        DevBuf d_in(size_t(n) * 8), d_a(size_t(n) * 8), d_s(size_t(n) * 8), d_c(size_t(n) * 8);
        Io io(c);
        io.up(d_in, in, size_t(n) * 8);
        hipLaunchKernelGGL(mgpu_glibc_trig_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, io.s, d_in.as<double>(), d_a.as<double>(), d_s.as<double>(),
                           d_c.as<double>(), n);
        HIPCK(hipGetLastError());
        io.back(atan_out, d_a, size_t(n) * 8);
        io.back(sin_out, d_s, size_t(n) * 8);
        io.down(cos_out, d_c, size_t(n) * 8);
    });
}

}  // extern "C"

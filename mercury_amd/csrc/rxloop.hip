// cl_telecom_system::receive_byte as a whole (telecom_system.cc:646-1503), batched over W independent capture
// windows: passband samples in, payload + receive_stats out. The DSP runs in the library's kernels
// (passband_to_baseband, Schmidl-Cox / MFSK time sync, energy gates, decimation, Moose, the RX hot path); the
// control flow — bounds / energy / metric gates, silence-skip and SKIP-H recoveries, the multi-trial retry loop with
// its k-th-best-peak and last-good fallbacks — is host logic that advances all windows of the batch in lock-step
// rounds, each round one batched kernel call per DSP step over the windows that still need it.
//
// Parity: every block is checked against the oracle / the compiled reference on its own; the orchestration is checked window for window
// against oracle/mercury_oracle.c:morc_receive_byte and against the reference's own cl_telecom_system::receive_byte
// (telecom_system.cc compiled unmodified: oracle/ref_ts_harness.cc; tests/test_receive_byte_vs_reference.py pins the oracle,
// tests/test_receive_byte.py::test_gpu_receive_byte_equals_the_reference_cl_telecom_system the GPU) — see DESIGN.md section 7.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "ctx.hpp"
#include "../../include/mercury_tx.h"

namespace {

// MERCURY_RXLOOP_TIMING=1: wall-clock per phase on stderr (the stream is synchronised at every mark)
struct PhaseTimer {
    bool on = std::getenv("MERCURY_RXLOOP_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void mark(hipStream_t s, const char* what) {
        if (!on) return;
        (void)hipStreamSynchronize(s);
        const auto n = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[rxloop] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

constexpr int kCoarseStep = 100;
constexpr int kManySpans = 4096;          // span energies: the lane-per-span kernel from this many spans per launch
constexpr int kSlice = 64, kCoarseGroup = 2;   // upload / mixer slices of windows; slices per coarse-search launch from host memory
constexpr double kEnergyGate = 0.001, kMetricGate = 0.5, kMeanHGate = 0.3, kFreqIgnore = 0.1;   // telecom_system.cc:843, :854, :1269; physical_config.cc:60

struct Win {                       // one capture window's walk through receive_byte
    int delay = 0, pream = 1, sync_trials = 0, skip_h = 0;
    double metric = 0.0, freq = 0.0, coarse_freq_offset = 0.0;
    bool in_loop = false, recovery_attempted = false, decoded = false;
};

}  // namespace

namespace mgpu_detail {

// Device workspace for W windows; allocated on the first call and kept in the context (hipMalloc / hipFree of several GB
// per call cost more than the kernels). Rebuilt when a call brings more windows, so its streams and events cover every call.
struct Workspace {
    DevBuf d_pass, d_bbi, d_frames, d_carrier, d_ia, d_ib, d_ic, d_vals, d_sum, d_cnt, d_freq, d_meanh, d_stats_k, d_payload_k, d_snr_k;
    DevBuf d_exc;                    // the carrier excisor's cleaned windows, sized like d_pass; made by the first call with the stage on
    size_t vals_per_window;
    PinnedBuf h_vals;                // page-locked landing area for the synchroniser metrics (tens of MB per call)
    // page-locked arena for the small index / result arrays of the control rounds: a copy from or to pageable memory holds the calling
    // thread for ~20-40 us each while the runtime stages it; from here the copies are queued back to back and the host moves on.
    // Bump-allocated; reset whenever the stream has been synchronised (everything queued before has completed by then).
    PinnedBuf h_pin;
    size_t pin_cap = 0, pin_off = 0;
    struct PendingDown { void* dst; const void* src; size_t bytes; };
    std::vector<PendingDown> pending;
    void* pin_take(size_t bytes) {
        const size_t need = (bytes + 63) & ~size_t(63);
        if (pin_off + need > pin_cap) return nullptr;
        void* p = static_cast<char*>(h_pin.h) + pin_off;
        pin_off += need;
        return p;
    }
    Stream side;                     // the signal-strength sum (a 92 k-term dependent chain per window) runs beside the synchroniser
    Stream copy;                     // brings the capture windows in, slice by slice, under the first kernels
    Stream search;                   // the coarse search of a group of slices, beside the mixer / filter of the next ones
    std::vector<Event> slice_ev, group_ev, we_ev;   // one per slice of windows
    Event ev_search, ev_ready, ev_done;
    Workspace(int W, int buf, int frame_n, size_t vals_per_window, int payload_stride, int numa_node)
        : d_pass(size_t(W) * buf * 8), d_bbi(size_t(W) * buf * 16), d_frames(size_t(W) * frame_n * 16), d_carrier(size_t(W) * 8),
          d_ia(size_t(W) * 128 * 4), d_ib(size_t(W) * 128 * 4), d_ic(size_t(W) * 4), d_vals(size_t(W) * vals_per_window * 8),
          d_sum(size_t(W) * 128 * 8), d_cnt(size_t(W) * 128 * 4), d_freq(size_t(W) * 16), d_meanh(size_t(W) * 8),
          d_stats_k(size_t(W) * sizeof(MgpuStatsDev)), d_payload_k(size_t(W) * payload_stride), d_snr_k(size_t(W) * 8), vals_per_window(vals_per_window) {
        HIPCK(host_alloc_on_node(&h_vals.h, size_t(W) * vals_per_window * 8, numa_node));      // control rounds' results: on the GPU's NUMA node
        pin_cap = std::max<size_t>(size_t(1) << 20, size_t(W) * 128 * 8 * 6);             // a few rounds of the largest index / result arrays
        HIPCK(host_alloc_on_node(&h_pin.h, pin_cap, numa_node));
        HIPCK(hipStreamCreate(&side.h));
        HIPCK(hipStreamCreateWithFlags(&copy.h, hipStreamNonBlocking));
        HIPCK(hipStreamCreateWithFlags(&search.h, hipStreamNonBlocking));
        const int nsl = (W + kSlice - 1) / kSlice;
        for (auto* v : {&slice_ev, &group_ev, &we_ev}) {
            v->resize(nsl);
            for (Event& e : *v) HIPCK(hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
        }
        for (Event* e : {&ev_search, &ev_ready, &ev_done}) HIPCK(hipEventCreateWithFlags(&e->h, hipEventDisableTiming));
    }
};
void Release::operator()(Workspace* p) const { delete p; }
void release_excised_windows(mgpu_ctx* c) { if (c->rxloop_ws) c->rxloop_ws->d_exc = DevBuf(); }

}  // namespace mgpu_detail

namespace {

struct Loop {
    PhaseTimer pt;
    mgpu_ctx* c;
    const mgpu::ModeTables& t;
    int W, buf, sym, pre, frame_i, frame_n, lower, upper, ngi_i, nfft_i, L, T;
    int span;                      // the search span of a fixed start: two preambles and a frame (telecom_system.cc:949-1012, :1447-1456)
    bool mfsk;
    hipStream_t s;
    mgpu_receive_config rc;
    Workspace& ws;
    std::vector<double> carrier;   // per window, as currently applied (carrier + fine offset of the running trial)
    const double* pass = nullptr;  // the capture windows on the device: the workspace copy, or the caller's buffer when it already lies in HBM
    // receive_byte's caller arrays and per-window state
    mgpu_link_state* state;
    uint8_t* payload;
    mgpu_receive_stats* stats;
    std::vector<Win> win;
    std::vector<char> live;        // still on the way to the trial loop
    std::vector<char> fixed_delay; // MFSK: delay given by the caller, no search and no signal level
    bool need_level = true;        // the whole-window signal level is wanted (not when every window comes with a known delay)
    int ncand0 = 0;                // coarse-search candidates per window
    int row0 = 0;                  // row of window 0 in the context's arrays kept by window row (the excisor's reports)

    static Workspace& workspace(mgpu_ctx* ctx, int W, int buffer_nsymb) {
        const auto& t = ctx->tab;
        if (!ctx->rxloop_ws || ctx->rxloop_ws_windows < W) {
            ctx->rxloop_ws.reset();
            const int buf = t.Nofdm * buffer_nsymb * kInterp, sym = t.Nofdm * kInterp;
            const size_t vals = size_t(std::max(buf / kCoarseStep + 2, 4 * sym + 2));       // coarse / fine candidate counts
            ctx->rxloop_ws.reset(new Workspace(W, buf, t.Nofdm * (t.Nsymb + t.preamble), vals, t.payload_stride, ctx->numa_node));
            ctx->rxloop_ws_windows = W;
        }
        return *ctx->rxloop_ws;
    }

    Loop(mgpu_ctx* ctx, int W_, const mgpu_receive_config& rc_, int buffer_nsymb, mgpu_link_state* state_ = nullptr, uint8_t* payload_ = nullptr,
         mgpu_receive_stats* stats_ = nullptr)
        : c(ctx), t(ctx->tab), W(W_), buf(t.Nofdm * buffer_nsymb * kInterp), sym(t.Nofdm * kInterp), pre(t.preamble),
          frame_i(t.Nofdm * (t.Nsymb + t.preamble) * kInterp), frame_n(t.Nofdm * (t.Nsymb + t.preamble)), lower(t.preamble),
          upper(buffer_nsymb - (t.Nsymb + t.preamble)), ngi_i(t.Ngi * kInterp), nfft_i(t.Nfft * kInterp), L(t.preamble * t.Nofdm * kInterp),
          T(rc_.time_sync_trials_max), span(t.Nofdm * (2 * t.preamble + t.Nsymb) * kInterp), mfsk(t.mfsk_M > 0), s(ctx->stream), rc(rc_),
          ws(workspace(ctx, W_, buffer_nsymb)), carrier(W_, rc_.carrier_hz), state(state_), payload(payload_), stats(stats_), win(W_), live(W_, 1),
          fixed_delay(W_, 0) {
        // a call that threw between down_async() and settle() leaves entries whose destinations were its stack vectors: never replay them
        ws.pending.clear();
        ws.pin_off = 0;
        ws.d_ia.view = ws.d_ib.view = ws.d_ic.view = ws.d_carrier.view = nullptr;
    }
    // Nothing of a call may outlive it: when the call ends - by return or by an exception unwinding it - with slots of the staging ring handed
    // out and no settle() since, the stream is drained before the ring can be reset by the next call.
    ~Loop() { if (unsettled) (void)hipStreamSynchronize(s); }

    bool in_bounds(int p) const { return p > lower && p < upper; }
    bool trials_used_up(const Win& x) const { return x.sync_trials > T || (mfsk && x.sync_trials > 0); }   // :931, :939-944

    // Host -> device for the control rounds' small index arrays (window lists, start offsets, carriers: a few KB). They are placed in the
    // page-locked staging area and the kernels read them THERE (the buffer's view): a 4 KB hipMemcpyAsync is a 5 us blit kernel plus the
    // gaps around it on the stream, and a call of 1024 windows made 400 of them (a fifth of its device time). A staging slot is reused
    // only after settle() has waited for the stream, so every kernel launched with a view has read it by then.
    // INVARIANT: a buffer with a view may only be consumed by kernels launched on stream `s` — settle() waits for `s` alone, so a kernel on
    // the side stream reading a view could still be running when its slot is handed out again. The side stream's kernels (signal level,
    // upload slices) take device buffers only; keep it that way or give them their own settle().
    // true from the first staging slot handed out / copy queued until settle() has waited for the stream: while it is set, kernels in flight may
    // still read this call's slots of the staging ring, and the call must not return.
    bool unsettled = false;
    void up(DevBuf& d, const void* h, size_t bytes) {
        d.view = nullptr;
        unsettled = true;
        if (void* p = ws.pin_take(bytes)) {
            std::memcpy(p, h, bytes);
            d.view = p;
            return;
        }
        HIPCK(hipMemcpyAsync(d.p, h, bytes, hipMemcpyHostToDevice, s));
    }
    // device -> host without waiting: the bytes are in h after the next down() / settle()
    void down_async(void* h, const void* d_src, size_t bytes) {
        unsettled = true;
        if (void* p = ws.pin_take(bytes)) {
            HIPCK(hipMemcpyAsync(p, d_src, bytes, hipMemcpyDeviceToHost, s));
            ws.pending.push_back({h, p, bytes});
        } else {
            HIPCK(hipMemcpyAsync(h, d_src, bytes, hipMemcpyDeviceToHost, s));
        }
    }
    void down_async(void* h, DevBuf& d, size_t bytes) { down_async(h, static_cast<const void*>(d.p), bytes); }
    void settle() {
        HIPCK(hipStreamSynchronize(s));
        for (const auto& q : ws.pending) std::memcpy(q.dst, q.src, q.bytes);
        ws.pending.clear();
        ws.pin_off = 0;
        unsettled = false;
    }
    void down(void* h, DevBuf& d, size_t bytes) { down_async(h, d, bytes); settle(); }

    // Windows that all mix with the call's own carrier (always so before a frequency offset has been measured) use the host-libm
    // table: the reference's own cos / sin values, and no trigonometry on the device. A window re-mixed at its measured offset
    // has a carrier of its own — never the table's, which would have to be rebuilt (3 ms of host time) for every such launch.
    const double* shared_mixer(const std::vector<int>& wins) {
        for (int w : wins) if (carrier[w] != rc.carrier_hz) return nullptr;
        return mixer_table(c, carrier[wins[0]], size_t(buf), s);
    }

    // passband_to_baseband of the whole buffer for the listed windows, overwriting their interpolated baseband
    void p2b(const std::vector<int>& wins, int filter) {
        if (wins.empty()) return;
        up(ws.d_ia, wins.data(), wins.size() * 4);
        up(ws.d_carrier, carrier.data(), size_t(W) * 8);
        const int ntaps = int((filter ? t.fir_data : t.fir_time_sync).size());
        launch_p2b(pass, buf, ws.d_carrier.as<double>(), nullptr, 0, buf, 1, c->d_fir[filter], ntaps, ws.d_bbi.as<double>(), ws.d_ia.as<int>(),
                   shared_mixer(wins), nullptr, 0, int(wins.size()), s);
    }

    // FIR_rx_data baseband of each listed window's frame at its `delay` only, decimated, straight into d_frames (row = slot[j] or j):
    // passband_to_baseband (ofdm.cc:2316-2339) followed by rational_resampler(DECIMATION) at the delay (:2267-2278) keeps every kInterp-th
    // sample of the (preamble + Nsymb) * Nofdm * kInterp the frame spans — a tenth of the capture window; each kept sample is the same 33-term sum.
    void p2b_frames(const std::vector<int>& wins, const int* slot) {
        if (wins.empty()) return;
        std::vector<int> st(W, 0);
        for (int w : wins) st[w] = win[w].delay;
        up(ws.d_ia, wins.data(), wins.size() * 4);
        up(ws.d_ib, st.data(), size_t(W) * 4);
        if (slot) up(ws.d_ic, slot, wins.size() * 4);
        up(ws.d_carrier, carrier.data(), size_t(W) * 8);
        launch_p2b(pass, buf, ws.d_carrier.as<double>(), ws.d_ib.as<int>(), 0, frame_n, kInterp, c->d_fir[1], int(t.fir_data.size()),
                   ws.d_frames.as<double>(), ws.d_ia.as<int>(), shared_mixer(wins), slot ? ws.d_ic.as<int>() : nullptr, 1, int(wins.size()), s);
    }

    // time_sync_preamble[_with_metric] on a sub-window [start, start + size) of each listed window
    void tsync(const std::vector<int>& wins, const std::vector<int>& start, const std::vector<int>& size, int step,
               const std::vector<int>& loc, int ntrials, std::vector<int>& delay, std::vector<double>& corr) {
        const int n = int(wins.size());
        delay.assign(n, 0);
        corr.assign(n, 0.0);
        if (!n) return;
        std::vector<int> nc(n);
        int ncmax = 1;
        for (int k = 0; k < n; ++k) { nc[k] = size[k] > L ? (size[k] - L + step - 1) / step : 0; ncmax = std::max(ncmax, nc[k]); }
        need(size_t(ncmax) <= ws.vals_per_window, "search window larger than the workspace");
        up(ws.d_ia, wins.data(), size_t(n) * 4);
        up(ws.d_ib, start.data(), size_t(n) * 4);
        up(ws.d_ic, nc.data(), size_t(n) * 4);
        launch_tsync_metric(ws.d_bbi.as<double>(), buf, ws.d_ib.as<int>(), ws.d_ia.as<int>(), ws.d_ic.as<int>(), ncmax, n, step, pre, ngi_i, nfft_i,
                            ws.d_vals.as<double>(), s);
        select(n, ncmax, nc, size, loc, step, ntrials, delay, corr);
    }

    // the reference's peak selection (ofdm.cc:1943-1964) over the candidate metrics of n windows lying in d_vals ([n][ncmax])
    void select(int n, int ncmax, const std::vector<int>& nc, const std::vector<int>& size, const std::vector<int>& loc, int step, int ntrials,
                std::vector<int>& delay, std::vector<double>& corr) {
        delay.assign(n, 0);
        corr.assign(n, 0.0);
        if (!n) return;
        if (n >= 32) {   // peak selection where the metrics lie; only (delay, correlation) per window come back
            up(ws.d_ic, nc.data(), size_t(n) * 4);
            up(ws.d_ia, size.data(), size_t(n) * 4);                    // wins / start are consumed: reuse their index buffers
            up(ws.d_ib, loc.data(), size_t(n) * 4);
            hipLaunchKernelGGL(mgpu_select_peak_kernel, dim3(n), dim3(64), 0, s, ws.d_vals.as<double>(), ws.d_ic.as<int>(), ncmax, step,
                               ws.d_ia.as<int>(), ws.d_ib.as<int>(), ntrials, n, ws.d_cnt.as<int>(), ws.d_sum.as<double>());
            HIPCK(hipGetLastError());
            down_async(delay.data(), ws.d_cnt, size_t(n) * 4);
            down(corr.data(), ws.d_sum, size_t(n) * 8);
        } else {         // a few windows: one lane per window would crawl through its candidates; the host is quicker
            const double* vals = static_cast<const double*>(ws.h_vals.h);
            down(ws.h_vals, ws.d_vals, size_t(n) * ncmax * 8);
            for (int k = 0; k < n; ++k) select_peak(&vals[size_t(k) * ncmax], nc[k], step, size[k], loc[k], ntrials, &delay[k], &corr[k]);
        }
    }

    // sum and count of |x|^2 over [off, off + len) (clipped at the buffer end) for every (window, offset) pair
    void energies(const std::vector<int>& wv, const std::vector<int>& off, std::vector<double>& sum, std::vector<int>& cnt, int len = 0) {
        if (len <= 0) len = sym;
        const int n = int(wv.size());
        sum.assign(n, 0.0);
        cnt.assign(n, 0);
        for (int base = 0; base < n; base += W * 128) {              // the index buffers hold W * 128 entries
            const int m = std::min(n - base, W * 128);
            up(ws.d_ia, wv.data() + base, size_t(m) * 4);
            up(ws.d_ib, off.data() + base, size_t(m) * 4);
            // a few spans: a wavefront each (short latency); thousands: a lane each (sync.hip)
            if (m >= kManySpans)
                hipLaunchKernelGGL(mgpu_span_energy_many_kernel, dim3((m + 255) / 256), dim3(256), 0, s, ws.d_bbi.as<double>(), buf, ws.d_ia.as<int>(),
                                   ws.d_ib.as<int>(), m, len, ws.d_sum.as<double>(), ws.d_cnt.as<int>());
            else
                hipLaunchKernelGGL(mgpu_span_energy_kernel, dim3((m + 3) / 4), dim3(256), 0, s, ws.d_bbi.as<double>(), buf, ws.d_ia.as<int>(),
                                   ws.d_ib.as<int>(), m, len, ws.d_sum.as<double>(), ws.d_cnt.as<int>());
            HIPCK(hipGetLastError());
            down_async(sum.data() + base, ws.d_sum, size_t(m) * 8);
            down(cnt.data() + base, ws.d_cnt, size_t(m) * 4);
        }
    }
    static double mean(double sum, int cnt) { return cnt > 0 ? sum / cnt : 0.0; }

    // measure_signal_stregth (ofdm.cc:1523-1539): the whole window's |x|^2 added in sample order, a 92 k-term dependent chain per window,
    // for windows [w0, w0 + n) of the baseband into d_freq. Device buffers only: it may run on the side stream.
    void launch_window_energy(int w0, int n, hipStream_t q) {
        hipLaunchKernelGGL(mgpu_window_energy_kernel, dim3(n), dim3(64), 0, q, ws.d_bbi.as<double>() + size_t(w0) * buf * 2, buf, buf,
                           ws.d_freq.as<double>() + w0);
        HIPCK(hipGetLastError());
    }
    // the window energies in d_freq as signal strengths in dBm (ofdm.cc:1523-1539)
    std::vector<double> window_dbm() {
        std::vector<double> sum(W);
        down(sum.data(), ws.d_freq, size_t(W) * 8);
        for (double& x : sum) x = 10.0 * std::log10((x / buf) / 0.001);
        return sum;
    }

    // The "scan forward for signal energy, re-run Schmidl-Cox from there" recovery shared by the bounds check
    // (telecom_system.cc:733-806), the silence skip (:862-925) and, with a fixed start and size, SKIP-H (:1436-1497)
    void recover(const std::vector<int>& wins, const std::vector<int>& scan_from, bool fixed_start, bool need_metric, std::vector<char>& ok) {
        const int n = int(wins.size());
        ok.assign(n, 0);
        if (!n) return;
        std::vector<int> search_start(n, -1);
        if (fixed_start) {
            for (int k = 0; k < n; ++k) if (scan_from[k] < upper) search_start[k] = scan_from[k] * sym;      // :1447-1456
        } else {
            std::vector<int> wv, off, first(n + 1, 0);
            for (int k = 0; k < n; ++k) {
                for (int q = scan_from[k]; q < upper; ++q) { wv.push_back(wins[k]); off.push_back(q * sym); }
                first[k + 1] = int(wv.size());
            }
            std::vector<double> sum;
            std::vector<int> cnt;
            energies(wv, off, sum, cnt);
            for (int k = 0; k < n; ++k)
                for (int j = first[k]; j < first[k + 1]; ++j)
                    if (mean(sum[j], cnt[j]) > kEnergyGate) { search_start[k] = off[j]; break; }
        }
        std::vector<int> sel, sw, ss, sz, loc;
        for (int k = 0; k < n; ++k) {
            if (search_start[k] < 0) continue;
            int available = buf - search_start[k];
            if (fixed_start) available = std::min(available, span);
            if (available <= pre * sym) continue;
            sel.push_back(k); sw.push_back(wins[k]); ss.push_back(search_start[k]); sz.push_back(available); loc.push_back(0);
        }
        std::vector<int> d;
        std::vector<double> corr;
        tsync(sw, ss, sz, kCoarseStep, loc, 1, d, corr);
        std::vector<int> off(sel.size());
        for (size_t j = 0; j < sel.size(); ++j) { d[j] += ss[j]; off[j] = d[j]; }
        std::vector<double> sum;
        std::vector<int> cnt;
        energies(sw, off, sum, cnt);
        for (size_t j = 0; j < sel.size(); ++j) {
            int rsym = d[j] / sym;
            if (rsym < 1) rsym = 1;
            if (mean(sum[j], cnt[j]) >= kEnergyGate && (!need_metric || corr[j] >= kMetricGate) && in_bounds(rsym)) {
                Win& x = win[wins[sel[j]]];
                x.delay = d[j]; x.metric = corr[j]; x.pream = rsym;
                ok[sel[j]] = 1;
            }
        }
    }

    // ---- receive_byte's phases, in call order ----

    // receive_stats as init() leaves it (telecom_system.cc:1968-1981) + the per-call resets (:653-655)
    void reset_outputs() {
        for (int w = 0; w < W; ++w) {
            mgpu_receive_stats& r = stats[w];
            r.iterations_done = -1; r.crc = 0; r.all_zeros = 0; r.message_decoded = 0; r.snr_db = -99.9;
            r.delay = 0; r.sync_trials = 0; r.freq_offset = 0; r.coarse_metric = 0; r.frame_overflow_symbols = 0; r.mean_H = -1.0;
            r.signal_strength_dbm = -999;
        }
        std::memset(payload, 0, size_t(W) * t.payload_stride);
    }

    // ---- upload + :676-696 coarse synchronisation on the FIR_rx_time_sync baseband, pipelined over slices of windows ----
    // The windows may lie in host memory (the reference's capture buffer; 740 KB each in mode 8, i.e. 13 ms of PCIe time per
    // 1024) or already in HBM (hipMemcpyDefault). A copy stream brings them over slice by slice; the mixer + time-sync filter
    // and the Schmidl-Cox metric of a slice run as soon as it has landed, under the copies of the following slices (a copy
    // from pageable memory holds the host thread, but the kernels of the slices before it are already queued).
    // Windows that already lie in HBM are read where they are. The coarse search (one wavefront per SIMD, issue-limited: sync.hip)
    // runs on a stream of its own, group by group, beside the mixer / filter launches of the following slices; from host memory a
    // group is kCoarseGroup slices (its search runs under the next group's copies), from HBM all of them (one launch: groups of 4
    // slices beside the filter launches measured 5 % slower).
    void coarse_sync(const double* passband) {
        const bool on_device = is_device_memory(passband);
        std::vector<int> all(W);
        for (int w = 0; w < W; ++w) all[w] = w;
        up(ws.d_ia, all.data(), size_t(W) * 4);
        up(ws.d_carrier, carrier.data(), size_t(W) * 8);
        const double* mix_cs = mixer_table(c, rc.carrier_hz, size_t(buf), s);        // every window mixes with the call's carrier here
        HIPCK(hipEventRecord(ws.ev_ready, s));
        HIPCK(hipStreamWaitEvent(ws.copy, ws.ev_ready, 0));                         // the previous call is done with d_pass
        ncand0 = buf > L ? (buf - L + kCoarseStep - 1) / kCoarseStep : 0;
        need(size_t(std::max(ncand0, 1)) <= ws.vals_per_window, "search window larger than the workspace");
        // The carrier excisor (include/ext/mercury_excisor.h), when on: each slice is cleaned into d_exc as soon as it has landed, on the main
        // stream ahead of the slice's filter, and `pass` points there from the first launch_p2b on; the raw windows are read by the excisor alone.
        const double* const raw = on_device ? passband : ws.d_pass.as<double>();
        const bool excise = c->exc.mode == MGPU_EXCISE_WELCH;
        if (excise) {
            need(size_t(row0) + size_t(W) <= size_t(c->max_batch), "carrier excisor: the call's windows must lie inside max_batch");
            ws.d_exc.grow(size_t(c->rxloop_ws_windows) * buf * 8);
        }
        pass = excise ? ws.d_exc.as<double>() : raw;
        need_level = !mfsk || !state;
        if (!need_level) for (int w = 0; w < W; ++w) if (state[w].fixed_delay_plus_one <= 0) { need_level = true; break; }
        // Windows already in HBM (OFDM): the signal-level chains (one wavefront per window, 0.6 ms of dependent additions) are launched
        // behind the coarse search instead of ahead of it: they then run beside the gates, their host round trips and the recovery search,
        // where the GPU has room; beside the coarse search — one latency-bound wavefront per SIMD — they cost it 0.37 ms. (From host memory
        // the search waits for PCIe anyway; MFSK windows have the longest chain and nothing but the whole call to hide it behind.)
        const bool defer_level = need_level && on_device && !mfsk;
        const int nsl = (W + kSlice - 1) / kSlice, group = on_device ? nsl : kCoarseGroup;
        for (int k = 0; k < nsl; ++k) {
            const int off = k * kSlice, n = std::min(kSlice, W - off);
            const int g0 = (k / group) * group * kSlice, gn = off + n - g0;
            const bool group_end = (k + 1) % group == 0 || k == nsl - 1;
            if (!on_device) {
                HIPCK(hipMemcpyAsync(ws.d_pass.as<double>() + size_t(off) * buf, passband + size_t(off) * buf, size_t(n) * buf * 8, hipMemcpyDefault, ws.copy));
                HIPCK(hipEventRecord(ws.slice_ev[k], ws.copy));
                HIPCK(hipStreamWaitEvent(s, ws.slice_ev[k], 0));
            }
            if (excise)
                launch_excisor(c, raw + size_t(off) * buf, n, buf, rc.carrier_hz, ws.d_exc.as<double>() + size_t(off) * buf,
                               c->exc.d_report + size_t(row0 + off), s);
            launch_p2b(pass, buf, ws.d_carrier.as<double>(), nullptr, 0, buf, 1, c->d_fir[0], int(t.fir_time_sync.size()), ws.d_bbi.as<double>(),
                       ws.d_ia.as<int>() + off, mix_cs, nullptr, 0, n, s);
            // :678 the signal level, on the side stream ahead of the group's coarse search so that the two share the compute units
            // (behind the search it added its full latency to the call)
            if (group_end && need_level && !defer_level) launch_level(g0, gn, ws.we_ev[k]);
            if (group_end && !mfsk && ncand0 > 0) {
                HIPCK(hipEventRecord(ws.group_ev[k], s));
                HIPCK(hipStreamWaitEvent(ws.search, ws.group_ev[k], 0));
                launch_tsync_metric(ws.d_bbi.as<double>() + size_t(g0) * buf * 2, buf, nullptr, nullptr, nullptr, ncand0, gn, kCoarseStep, pre, ngi_i,
                                    nfft_i, ws.d_vals.as<double>() + size_t(g0) * ncand0, ws.search);
            }
        }
        if (!mfsk && ncand0 > 0) {                                   // the main stream continues when the last group's search is done
            HIPCK(hipEventRecord(ws.ev_search, ws.search));
            HIPCK(hipStreamWaitEvent(s, ws.ev_search, 0));
        }
        pt.mark(s, "upload + p2b + coarse metric");
        if (defer_level) launch_level(0, W, ws.we_ev[0]);           // behind the coarse search (the event is recorded after the main stream's wait for it)
        HIPCK(hipEventRecord(ws.ev_done, ws.side));                  // signal strength: the main stream waits for it before the trial loop overwrites the baseband
        pt.mark(s, "signal strength");
    }
    // the signal level of windows [w0, w0 + n) on the side stream, once the main stream has filtered them
    void launch_level(int w0, int n, hipEvent_t ev) {
        HIPCK(hipEventRecord(ev, s));
        HIPCK(hipStreamWaitEvent(ws.side, ev, 0));
        launch_window_energy(w0, n, ws.side);
    }

    // ---- the first delay estimate: the MFSK preamble search, or the coarse Schmidl-Cox peak of the metrics already in d_vals ----
    void coarse_delays() {
        if (mfsk) {
            mfsk_delays();
        } else {
            std::vector<int> zero(W, 0), full(W, buf), d;
            std::vector<double> corr;
            select(W, ncand0, std::vector<int>(W, ncand0), full, zero, kCoarseStep, 1, d, corr);
            for (int w = 0; w < W; ++w) { win[w].delay = d[w]; win[w].metric = corr[w]; }
        }
        pt.mark(s, "coarse time sync");
        for (int w = 0; w < W; ++w) win[w].pream = std::max(1, win[w].delay / sym);
    }
    // cl_ofdm::time_sync_mfsk (ofdm.cc:2011-2061): slot energies and the preamble-tone search, both where the baseband lies; only the
    // delays come back. Windows with a known delay (:663-672 mfsk_fixed_delay, used once, no signal level) need neither.
    void mfsk_delays() {
        std::vector<int> d(W, 0);
        if (need_level) {
            const int nslots = buf / sym;
            DevBuf d_e(size_t(W) * nslots * t.Nc * 8);
            HIPCK(hipMemsetAsync(d_e.p, 0, size_t(W) * nslots * t.Nc * 8, s));
            hipLaunchKernelGGL(mgpu_slot_energy_kernel, dim3((nslots + 3) / 4, W), dim3(256), 0, s, ws.d_bbi.as<double>(), buf, nslots, kInterp,
                               c->dev.twiddle, d_e.as<double>());
            HIPCK(hipGetLastError());
            std::vector<int> ss(W, 0);
            if (state) for (int w = 0; w < W; ++w) ss[w] = state[w].mfsk_search_start;
            up(ws.d_ib, ss.data(), size_t(W) * 4);
            launch_mfsk_sync(c, d_e.as<double>(), W, nslots, buf, ws.d_ib.as<int>(), ws.d_cnt.as<int>(), s);
            down(d.data(), ws.d_cnt, size_t(W) * 4);
        }
        for (int w = 0; w < W; ++w) {
            if (state && state[w].fixed_delay_plus_one > 0) {
                win[w].delay = state[w].fixed_delay_plus_one - 1;
                state[w].fixed_delay_plus_one = 0;
                fixed_delay[w] = 1;
                continue;
            }
            win[w].delay = d[w];
        }
    }

    // ---- :702-718 MFSK frame completeness; :733-806 bounds recovery; :808-928 energy / metric gates and the silence-skip recovery ----
    void gates() {
        if (mfsk)
            for (int w = 0; w < W; ++w) {
                const int frame_end = win[w].delay + (pre + t.active_nsymb) * sym;
                if (frame_end > buf) { stats[w].frame_overflow_symbols = (frame_end - buf + sym - 1) / sym; live[w] = 0; }
            }
        if (!mfsk) {   // preamble outside the valid bounds: scan the buffer for signal, search again from there
            std::vector<int> wins, from;
            for (int w = 0; w < W; ++w) if (!in_bounds(win[w].pream)) { wins.push_back(w); from.push_back(lower + 1); }
            std::vector<char> ok;
            recover(wins, from, false, true, ok);
        }
        for (int w = 0; w < W; ++w) if (live[w] && !in_bounds(win[w].pream)) live[w] = 0;
        if (!mfsk) {
            std::vector<int> wv, off;
            for (int w = 0; w < W; ++w) if (live[w]) { wv.push_back(w); off.push_back(win[w].delay); }
            std::vector<double> sum;
            std::vector<int> cnt;
            pt.mark(s, "gates: bounds recovery");
            energies(wv, off, sum, cnt);
            pt.mark(s, "gates: energy at delay");
            std::vector<int> wins, from;
            for (size_t j = 0; j < wv.size(); ++j) {
                bool energy_ok = !(mean(sum[j], cnt[j]) < kEnergyGate);
                if (energy_ok && win[wv[j]].metric < kMetricGate) energy_ok = false;
                if (!energy_ok) { wins.push_back(wv[j]); from.push_back(win[wv[j]].pream + 1); }
            }
            if (pt.on) std::fprintf(stderr, "[rxloop] %zu of %zu windows fail the energy / metric gate\n", wins.size(), wv.size());
            std::vector<char> ok;
            recover(wins, from, false, true, ok);
            for (size_t j = 0; j < wins.size(); ++j) if (!ok[j]) live[wins[j]] = 0;
        }
        for (int w = 0; w < W; ++w) win[w].in_loop = live[w] != 0;
        pt.mark(s, "bounds / energy gates");
    }

    // the signal-strength sums must be out of the baseband before the trial loop re-filters it
    void collect_signal_strength() {
        HIPCK(hipStreamWaitEvent(s, ws.ev_done, 0));
        const std::vector<double> dbm = window_dbm();
        for (int w = 0; w < W; ++w) stats[w].signal_strength_dbm = fixed_delay[w] ? 0.0 : dbm[w];
    }

    // the windows that run another trial; one that has used up its trials leaves the loop here
    std::vector<int> active() {
        std::vector<int> act;
        for (int w = 0; w < W; ++w) {
            Win& x = win[w];
            if (!x.in_loop) continue;
            if (trials_used_up(x)) { x.in_loop = false; continue; }
            act.push_back(w);
        }
        return act;
    }

    // ---- one round of the trial loop (:931-1431) over the windows still in it ----
    void trial(const std::vector<int>& act) {
        choose_delays(act);
        fix_delays(act);
        cut_frames(act);
        decode(act);
        remix_continuing(act);
    }

    // delay for this trial: last good one on the final trial (:945-948), else the k-th best fine-search peak (:1014-1018), after the
    // coarse frequency search before trial 1 when it is enabled
    void choose_delays(const std::vector<int>& act) {
        std::vector<int> fw, cw;
        for (int w : act) {
            Win& x = win[w];
            if (mfsk) continue;
            const bool use_last_delay = x.sync_trials == T && rc.use_last_good_time_sync && state && state[w].delay_of_last_decoded_message != -1;
            if (use_last_delay) x.delay = state[w].delay_of_last_decoded_message;
            else if (x.sync_trials == 1 && rc.coarse_freq_sync_enabled) cw.push_back(w);
            else fw.push_back(w);
        }
        if (!cw.empty()) {
            coarse_freq_search(cw);
            fw.insert(fw.end(), cw.begin(), cw.end());
        }
        std::vector<int> fstart, fsize, floc, d;
        for (int w : fw) { fstart.push_back((win[w].pream - 1) * sym); fsize.push_back((pre + 4) * sym); floc.push_back(win[w].sync_trials); }
        std::vector<double> corr;
        tsync(fw, fstart, fsize, 1, floc, T, d, corr);
        for (size_t j = 0; j < fw.size(); ++j) win[fw[j]].delay = fstart[j] + d[j];
        pt.mark(s, "trial: fine time sync");
    }

    // :949-1012 coarse frequency search before trial 1: Schmidl-Cox at carrier -30 / 0 / +30 Hz; leaves the time-sync baseband at the
    // (possibly corrected) carrier
    void coarse_freq_search(const std::vector<int>& cw) {
        const double freq_search[3] = {-30.0, 0.0, 30.0};
        const int nc = int(cw.size());
        std::vector<double> best_corr(nc, 0.0), best_off(nc, 0.0), zero_corr(nc, 0.0);
        std::vector<int> best_delay(nc), zero(nc, 0), ssize(nc, span);
        for (int j = 0; j < nc; ++j) best_delay[j] = win[cw[j]].delay;
        for (int i = 0; i < 3; ++i) {
            for (int w : cw) carrier[w] = rc.carrier_hz + freq_search[i];
            p2b(cw, 0);
            std::vector<int> d;
            std::vector<double> corr;
            tsync(cw, zero, ssize, kCoarseStep, zero, 1, d, corr);
            for (int j = 0; j < nc; ++j) {
                if (std::fabs(freq_search[i]) < 0.1) zero_corr[j] = corr[j];
                if (corr[j] > best_corr[j]) { best_corr[j] = corr[j]; best_off[j] = freq_search[i]; best_delay[j] = d[j]; }
            }
        }
        for (int j = 0; j < nc; ++j) {
            Win& x = win[cw[j]];
            if (std::fabs(best_off[j]) > 1.0 && best_corr[j] > 0.5 && best_corr[j] > zero_corr[j] + 0.1) {
                x.coarse_freq_offset = best_off[j];
                x.delay = best_delay[j];
                x.pream = std::max(1, x.delay / sym);
            }
            carrier[cw[j]] = rc.carrier_hz + x.coarse_freq_offset;
        }
        p2b(cw, 0);
    }

    // :1020-1031 the delay clamped into the buffer; :1039-1071 the post-fine-sync energy fix
    void fix_delays(const std::vector<int>& act) {
        for (int w : act) {
            Win& x = win[w];
            if (x.delay < 0) x.delay = 0;
            if (x.delay > buf - frame_i) x.delay = buf - frame_i;
        }
        if (!mfsk) {
            std::vector<int> wv, off;
            for (int w : act) for (int q = 0; q <= 3; ++q) { wv.push_back(w); off.push_back(std::min(win[w].delay + q * sym, buf)); }
            std::vector<double> sum;
            std::vector<int> cnt;
            energies(wv, off, sum, cnt);
            for (size_t k = 0; k < act.size(); ++k) {
                Win& x = win[act[k]];
                if (sum[k * 4] / sym < kEnergyGate) {
                    const int orig = x.delay;
                    for (int q = 1; q <= 3; ++q) {
                        const int cand = orig + q * sym;
                        if (cand + sym > buf) break;
                        if (sum[k * 4 + q] / sym >= kEnergyGate) { x.delay = cand; break; }
                    }
                }
            }
        }
        pt.mark(s, "trial: energy fix");
    }

    // :1083-1105 FIR_rx_data baseband at the (coarse-corrected) carrier, frame cut out at `delay`, decimated; :1108-1131 fine frequency
    // offset (Moose) or the last good one on the final trial, and the frames re-cut at it where it matters
    void cut_frames(const std::vector<int>& act) {
        const int n = int(act.size());
        for (int w : act) carrier[w] = rc.carrier_hz + win[w].coarse_freq_offset;   // effective_carrier_freq, :1074
        p2b_frames(act, nullptr);
        pt.mark(s, "trial: p2b data filter + cut");
        const int pre_half = pre / 2 == 0 ? 1 : pre / 2;
        hipLaunchKernelGGL(mgpu_fsync_kernel, dim3(n), dim3(256), 0, s, ws.d_frames.as<double>() + size_t(t.Ngi) * 2, frame_n, pre_half,
                           c->dev.twiddle, ws.d_freq.as<double>());
        HIPCK(hipGetLastError());
        std::vector<double> mul(size_t(n) * 2);
        down(mul.data(), ws.d_freq, size_t(n) * 16);
        std::vector<int> rw, rslot;
        for (int k = 0; k < n; ++k) {
            Win& x = win[act[k]];
            double f = moose_hz(mul[2 * k], mul[2 * k + 1], kBandwidthHz / double(t.Nc));
            if (x.sync_trials == T && rc.use_last_good_freq_offset && state && state[act[k]].freq_offset_of_last_decoded_message != 0)
                f = state[act[k]].freq_offset_of_last_decoded_message;
            x.freq = f;
            if (!mfsk && std::fabs(f) > kFreqIgnore) { carrier[act[k]] = rc.carrier_hz + x.coarse_freq_offset + f; rw.push_back(act[k]); rslot.push_back(k); }
        }
        p2b_frames(rw, rslot.data());
        pt.mark(s, "trial: Moose + re-mix");
    }

    // :1132-1345 the hot path on the data symbols (they start `preamble` symbols into each extracted frame), then each window's result
    void decode(const std::vector<int>& act) {
        const int n = int(act.size());
        const bool zf = t.estimator == MGPU_EST_ZF;
        SpanIo io = own_span(c);
        io.bb = ws.d_frames.as<double>() + size_t(pre) * t.Nofdm * 2; io.frame_stride = frame_n;
        io.payload = ws.d_payload_k.as<uint8_t>(); io.stats = ws.d_stats_k.as<MgpuStatsDev>();
        if (!mfsk) io.mean_H = ws.d_meanh.as<double>();
        // receive_stats.SNR is a double (telecom_system.cc:1343-1396): 10 log10(1 / variance) of the float variance (LS modes), -10 log10 of
        // the re-encoded symbols' error power (ZF modes). The kernels' records carry it as a float (the mgpu_frame_stats ABI); here the
        // argument of the logarithm comes back and the host takes it with the libm the reference calls: the double equals the reference's.
        if (zf) io.zf_var = ws.d_snr_k.as<double>();
        // an estimator ladder retries inside this span, before the host looks: a window a later rung decodes counts as decoded here
        launch_span(c, io, n, MgpuTapsDev{}, s);
        std::vector<double> zf_var(zf ? n : 0, 1.0), mh(n, 1.0);
        std::vector<float> snr_var(!zf && !mfsk ? n : 0, 1.0f);
        std::vector<MgpuStatsDev> st(n);
        std::vector<uint8_t> pay(size_t(n) * t.payload_stride);
        if (zf) down_async(zf_var.data(), ws.d_snr_k, size_t(n) * 8);
        else if (!mfsk) down_async(snr_var.data(), static_cast<const void*>(c->d_snrvar), size_t(n) * 4);
        if (!mfsk) down_async(mh.data(), ws.d_meanh, size_t(n) * 8);
        down_async(st.data(), ws.d_stats_k, size_t(n) * sizeof(MgpuStatsDev));
        down(pay.data(), ws.d_payload_k, size_t(n) * t.payload_stride);
        pt.mark(s, "trial: RX path + results");
        for (int k = 0; k < n; ++k) {
            const int w = act[k];
            Win& x = win[w];
            mgpu_receive_stats& r = stats[w];
            r.delay = x.delay;
            if (!mfsk) {
                r.mean_H = mh[k];
                if (mh[k] < kMeanHGate) { ++x.skip_h; ++x.sync_trials; r.sync_trials = x.sync_trials; continue; }   // :1269-1280: no decode this trial
            }
            const MgpuStatsDev& d = st[k];
            r.iterations_done = d.iterations_done; r.crc = d.crc; r.all_zeros = d.all_zeros;
            std::memcpy(payload + size_t(w) * t.payload_stride, &pay[size_t(k) * t.payload_stride], t.payload_stride);
            if (!d.message_decoded) {                            // :1343-1360
                r.snr_db = -99.9; r.message_decoded = 0;
                ++x.sync_trials;
            } else {                                             // :1361-1430
                r.snr_db = double(d.snr_db); r.message_decoded = 1;                       // MFSK: 0.0 (:1362-1367)
                if (zf) r.snr_db = -10.0 * std::log10(zf_var[k]);                              // ofdm.cc:1622-1635
                else if (!mfsk) r.snr_db = 10.0 * std::log10(1.0 / double(snr_var[k]));        // :1369-1376
                x.decoded = true; x.in_loop = false;
                if (!mfsk) { r.freq_offset = x.freq; if (state) state[w].freq_offset_of_last_decoded_message = x.freq; }
                if (state) state[w].delay_of_last_decoded_message = x.delay;
            }
            r.sync_trials = x.sync_trials;
        }
    }

    // Windows that go on to another trial: in the reference the baseband buffer now holds the FIR_rx_data output of the whole capture
    // window (:1083-1105 wrote it) and a later trial may read it before refreshing it. p2b_frames computed only the samples the RX path
    // reads, so the full buffer is produced here for the windows that did not decode. Only for those that WILL run another trial
    // (trials_used_up() is the test at the top of the next round): nothing reads the baseband of a window that leaves the loop (the SKIP-H
    // recovery mixes afresh, :1458-1463), and the last kernel of a call is thereby always followed by a round's down() / settle().
    void remix_continuing(const std::vector<int>& act) {
        std::vector<int> again;
        for (int w : act) if (win[w].in_loop && !trials_used_up(win[w])) again.push_back(w);
        p2b(again, 1);
    }

    // ---- :1436-1497 SKIP-H recovery: every trial died on a low channel estimate -> look for a later preamble. True when a window
    // re-enters the trial loop ----
    bool skip_h_recovery() {
        std::vector<int> wins, from;
        for (int w = 0; w < W; ++w) {
            Win& x = win[w];
            if (!mfsk && live[w] && !x.decoded && x.skip_h >= T + 1 && !x.recovery_attempted) {
                x.recovery_attempted = true;
                wins.push_back(w); from.push_back(x.pream + 2);
            }
        }
        if (wins.empty()) return false;
        std::vector<int> searchable;
        for (size_t j = 0; j < wins.size(); ++j) {
            const int available = std::min(buf - from[j] * sym, span);
            if (from[j] < upper && available > pre * sym) { searchable.push_back(wins[j]); carrier[wins[j]] = rc.carrier_hz; }
        }
        p2b(searchable, 0);                                // fresh FIR_rx_time_sync baseband for the search (:1458-1463)
        std::vector<char> ok;
        recover(wins, from, true, false, ok);
        bool any = false;
        for (size_t j = 0; j < wins.size(); ++j)
            if (ok[j]) { Win& x = win[wins[j]]; x.sync_trials = 0; x.skip_h = 0; x.coarse_freq_offset = 0.0; x.in_loop = true; any = true; }
        return any;
    }

    // The call is blocking, to the last kernel: a kernel still in flight could read its window list in the staging ring after the next call
    // has reset it. Every phase ends on a settle(); should one ever not, the stream is waited for here (and by ~Loop when an exception
    // unwinds the call).
    void finish() {
        for (int w = 0; w < W; ++w) { stats[w].delay = win[w].delay; stats[w].coarse_metric = win[w].metric; stats[w].sync_trials = win[w].sync_trials; }
        if (unsettled) HIPCK(hipStreamSynchronize(s));
        unsettled = false;
    }
};

}  // namespace

extern "C" {

int mgpu_receive_buffer_nsymb(mgpu_ctx* c) {
    if (!c) return -1;
    const auto& t = c->tab;                                      // data_container.cc:133-143
    const double sym_time_ms = 1000.0 * t.Nofdm * kInterp / kSampleRate;
    const int turnaround_symb = int(std::ceil(1200.0 / sym_time_ms)) + 4;
    const int frame_symb = t.preamble + t.Nsymb;
    int min_buf = frame_symb * 2;
    if (frame_symb + turnaround_symb > min_buf) min_buf = frame_symb + turnaround_symb;
    if (min_buf < 32) min_buf = 32;
    return min_buf;
}

// cl_telecom_system::measure_signal_only (telecom_system.cc:1520-1541): time-sync filter + whole-window power, nothing else
int mgpu_measure_signal_only(mgpu_ctx* c, const double* passband, int W, double carrier_hz, double* signal_strength_dbm) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(passband && signal_strength_dbm && W > 0 && W <= c->max_batch, "bad argument (W must be 1..max_batch)");
        const mgpu_receive_config rc = {carrier_hz, 1, 0, 0, 0};
        Loop lp(c, W, rc, mgpu_receive_buffer_nsymb(c));
        std::vector<int> all(W);
        for (int w = 0; w < W; ++w) all[w] = w;
        HIPCK(hipMemcpyAsync(lp.ws.d_pass.p, passband, size_t(W) * lp.buf * 8, hipMemcpyDefault, lp.s));
        lp.pass = lp.ws.d_pass.as<double>();
        lp.p2b(all, 0);
        lp.launch_window_energy(0, W, lp.s);
        const std::vector<double> dbm = lp.window_dbm();
        std::copy(dbm.begin(), dbm.end(), signal_strength_dbm);
    });
}

}  // extern "C"

// receive_byte for W windows that lie in host or device memory, on the context's stream: the reference's receive_byte, phase by phase
void mgpu_detail::receive_byte_impl(mgpu_ctx* c, const double* passband, int W, const mgpu_receive_config* rcp, mgpu_link_state* state,
                                    uint8_t* payload, mgpu_receive_stats* stats, int row0) {
    Loop lp(c, W, *rcp, mgpu_receive_buffer_nsymb(c), state, payload, stats);
    lp.row0 = row0;
    lp.pt.mark(lp.s, "device buffers");
    ensure_workspaces(c, WS_FRONTEND | WS_LLR | WS_OUT);
    lp.reset_outputs();
    lp.coarse_sync(passband);                  // upload, :676-696 coarse metric, :678 signal level launched
    lp.coarse_delays();                        // MFSK preamble search or the coarse peak
    lp.gates();                                // :702-928
    lp.collect_signal_strength();
    for (;;) {                                 // :931-1431 one round per trial over the windows still in the loop, then :1436-1497
        const std::vector<int> act = lp.active();
        if (!act.empty()) lp.trial(act);
        else if (!lp.skip_h_recovery()) break;
    }
    lp.finish();
}

// The capture thread's widening of the audio device's samples to the doubles receive_byte works on (radio_capture_thread,
// audioio.c:893-936), on the device: INT32 / INT_MAX (:909), INT16 / 32768.0 (:907), FLOAT32 widened (:905). int -> double is exact and the
// division is the IEEE-754 correctly rounded one on both sides, so the doubles are the CPU's bit for bit; what crosses PCIe is 4 (2) bytes
// per sample instead of 8.
template <typename T>
__global__ __launch_bounds__(256) void mgpu_widen_capture_kernel(const T* __restrict__ in, size_t n, double divisor, double* __restrict__ out) {
    for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
        out[i] = mgpu_fmt::widen(in[i], divisor);
    }
}
namespace {
void launch_widen(const void* d_in, int fmt, size_t n, double* d_out, hipStream_t s) {      // compact formats only: doubles are read where they lie
    const dim3 grid(unsigned(std::min<size_t>((n + 255) / 256, 65535u * 4))), block(256);
    mgpu_fmt::with_elements(mgpu_fmt::element(1, fmt), d_in, [&](auto* in, double divisor) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(in)>>;
        if constexpr (!std::is_same_v<T, double>) hipLaunchKernelGGL(mgpu_widen_capture_kernel<T>, grid, block, 0, s, in, n, divisor, d_out);
    });
    HIPCK(hipGetLastError());
}
// The sub-batches [offset, count) a pipelined host call is cut into. Doubles are upload-bound (the synchroniser of a sub-batch is over before
// the next one has landed): equal pieces of 256, so that little is left to do behind the last byte. Compact samples (4 or 2 bytes each) land
// two to four times faster than they are processed, and every receive_byte_impl call pays its control rounds' fixed ~1.5 ms whatever its size:
// a short first piece gets the device started, then the pieces grow (1/8, 3/8, 1/2 of the call; INT16: 128 windows, then the rest) - fewer
// calls, each one's upload still hidden behind its predecessor. Measured on 1024 mode-8 windows (tools/bench_rb_sched.py,
// profiles/r06_rb_sched.txt), k windows/s, equal pieces of 256 -> these schedules: INT32 66.7 -> 72.4, INT16 71.7 -> 85.3; doubles stay at
// equal pieces (60.0; 128,384,512 gives 52.9). MERCURY_RB_SCHED=<a,b,c,...> gives the piece sizes instead (the last one repeats).
std::vector<std::pair<int, int>> pieces(int W, int fmt) {
    std::vector<int> sched;
    if (const char* e = getenv("MERCURY_RB_SCHED"))
        for (const char* q = e; *q;) { const int v = atoi(q); if (v >= 32) sched.push_back(v); while (*q && *q != ',') ++q; if (*q == ',') ++q; }
    if (sched.empty()) {
        if (fmt == MGPU_SAMPLES_F64) sched = {256};
        else if (fmt == MGPU_SAMPLES_INT16) sched = {128, std::max(256, W - 128)};     // the whole call lands in the time one piece is processed
        else { const int a = std::max(128, (W / 8 + 63) & ~63); sched = {a, 3 * a, std::max(256, W - 4 * a)}; }
    }
    std::vector<std::pair<int, int>> out;
    for (int off = 0; off < W;) {
        const int n = std::min(sched[std::min(out.size(), sched.size() - 1)], W - off);
        out.emplace_back(off, n);
        off += n;
    }
    return out;
}

// windows [off, off + n) of the host capture into the staging buffer as doubles (compact samples: copied, then widened), waited for
hipError_t upload_piece(mgpu_ctx* c, const char* src, int fmt, size_t buf, int off, int n) {
    const size_t sb = mgpu_fmt::element_bytes(mgpu_fmt::element(1, fmt));
    double* stage = c->rb_stage + size_t(off) * buf;
    void* dst = fmt == MGPU_SAMPLES_F64 ? static_cast<void*>(stage) : c->rb_compact + size_t(off) * buf * sb;
    hipError_t e = hipMemcpyAsync(dst, src + size_t(off) * buf * sb, size_t(n) * buf * sb, hipMemcpyHostToDevice, c->rb_stream);
    if (e == hipSuccess && fmt != MGPU_SAMPLES_F64) {
        try { launch_widen(dst, fmt, size_t(n) * buf, stage, c->rb_stream); }
        catch (...) { e = hipErrorLaunchFailure; }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->rb_stream);
    return e;
}

// mgpu_receive_byte_batch / _samples: fmt = the sample format of `capture`
void receive_byte_any(mgpu_ctx* c, const void* capture, int fmt, int W, const mgpu_receive_config* rcp, mgpu_link_state* state, uint8_t* payload,
                      mgpu_receive_stats* stats) {
    need(capture && rcp && payload && stats && W > 0 && W <= c->max_batch, "bad argument (W must be 1..max_batch)");
    need(mgpu_fmt::element(1, fmt) != mgpu_fmt::kNone, "unknown sample format");
    need(rcp->time_sync_trials_max >= 1 && rcp->time_sync_trials_max < 64,
         "time_sync_trials_max must be 1..63 (0 makes the reference index its peak table at -1)");
    // every argument is judged before the first copy or kernel is queued: an error return leaves nothing in flight and no state[] entry touched
    if (state && c->tab.mfsk_M == 0) for (int w = 0; w < W; ++w) need(state[w].fixed_delay_plus_one <= 0, "fixed_delay_plus_one: MFSK modes only");
    // Windows in host memory: bringing 1024 mode-8 windows over PCIe takes 13.5 ms as doubles (half that as INT32 / FLOAT32 samples, a quarter
    // as INT16) and the synchroniser + decoder another 17 ms. The windows are independent, so from 512 windows on the call is cut into
    // sub-batches (pieces()): a helper thread uploads them one after another into a staging buffer (a copy from pageable memory holds its
    // calling thread; compact samples are widened there by a kernel on the upload stream), this thread runs the whole receive_byte on each
    // sub-batch as soon as it has landed. The call then lasts the upload plus the receive_byte of the last sub-batch, so small sub-batches win
    // until the fixed cost of the control rounds takes over: 1024 windows in 19.0 ms with sub-batches of 512, 17.1 ms with 256, 19.4 ms with
    // 128 (doubles; the upload alone is 13.5 ms). MERCURY_NO_PIPELINE=1 receives the call in one piece.
    static const bool no_pipe = getenv("MERCURY_NO_PIPELINE") != nullptr;
    const bool on_device = is_device_memory(capture);
    const auto& t = c->tab;
    const size_t buf = size_t(t.Nofdm) * mgpu_receive_buffer_nsymb(c) * kInterp;
    const size_t sb = mgpu_fmt::element_bytes(mgpu_fmt::element(1, fmt));
    const char* src = static_cast<const char*>(capture);
    if (!c->rb_stream) HIPCK(hipStreamCreateWithFlags(&c->rb_stream.h, hipStreamNonBlocking));
    const int kMinSub = 256;
    if (on_device || no_pipe || W < 2 * kMinSub) {
        if (fmt == MGPU_SAMPLES_F64) { receive_byte_impl(c, static_cast<const double*>(capture), W, rcp, state, payload, stats); return; }
        // compact samples, one piece: (upload,) widen into the staging buffer, then the doubles path on device memory
        c->rb_stage.grow(size_t(W) * buf * 8);
        const void* d_in = capture;
        if (!on_device) {
            c->rb_compact.grow(size_t(W) * buf * sb);
            HIPCK(hipMemcpyAsync(c->rb_compact, capture, size_t(W) * buf * sb, hipMemcpyHostToDevice, c->rb_stream));
            d_in = c->rb_compact;
        }
        launch_widen(d_in, fmt, size_t(W) * buf, c->rb_stage, c->rb_stream);
        HIPCK(hipStreamSynchronize(c->rb_stream));
        receive_byte_impl(c, c->rb_stage, W, rcp, state, payload, stats);
        return;
    }
    const std::vector<std::pair<int, int>> ps = pieces(W, fmt);
    c->rb_stage.grow(size_t(W) * buf * 8);
    if (fmt != MGPU_SAMPLES_F64) c->rb_compact.grow(size_t(W) * buf * sb);
    std::mutex m;
    std::condition_variable cv;
    int landed = 0;
    hipError_t failed = hipSuccess;
    std::thread uploader([&] {
        hipError_t e = hipSetDevice(c->cfg.device);
        for (int j = 0; j < int(ps.size()); ++j) {
            if (e == hipSuccess) e = upload_piece(c, src, fmt, buf, ps[j].first, ps[j].second);
            {
                std::lock_guard<std::mutex> lk(m);
                failed = e;
                landed = j + 1;
            }
            cv.notify_all();
            if (e != hipSuccess) break;
        }
    });
    try {
        for (int j = 0; j < int(ps.size()); ++j) {
            const int off = ps[j].first, n = ps[j].second;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return landed > j || failed != hipSuccess; });
                if (failed != hipSuccess) break;
            }
            receive_byte_impl(c, c->rb_stage + size_t(off) * buf, n, rcp, state ? state + off : nullptr,
                              payload + size_t(off) * t.payload_stride, stats + off, off);
        }
    } catch (...) {
        uploader.join();
        throw;
    }
    uploader.join();
    if (failed != hipSuccess) throw std::runtime_error(std::string("upload of the capture windows: ") + hipGetErrorString(failed));
}
}  // namespace

extern "C" int mgpu_receive_byte_batch(mgpu_ctx* c, const double* passband, int W, const mgpu_receive_config* rcp, mgpu_link_state* state,
                                       uint8_t* payload, mgpu_receive_stats* stats) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] { receive_byte_any(c, passband, MGPU_SAMPLES_F64, W, rcp, state, payload, stats); });
}

extern "C" int mgpu_receive_byte_batch_samples(mgpu_ctx* c, const void* capture, int sample_format, int W, const mgpu_receive_config* rcp,
                                               mgpu_link_state* state, uint8_t* payload, mgpu_receive_stats* stats) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] { receive_byte_any(c, capture, sample_format, W, rcp, state, payload, stats); });
}

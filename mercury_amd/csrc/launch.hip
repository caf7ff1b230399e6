// The kernel launches the host-side translation units share (declared in ctx.hpp): the fused receive span (launch_span) and its parts -
// front-end and decoder, untimed and timed, and zero-forcing SNR; the ladder's part is in ladder.hip, the grouped span's kernels in combine.hip -, the synchroniser's
// metric / mixer / MFSK search kernels with the host halves of their searches, and the frame generator.
#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "ctx.hpp"

namespace mgpu_detail {

void frontend_untimed(mgpu_ctx* c, const SpanIo& io, int F, const MgpuTapsDev& taps, const MgpuLsRect* rect, hipStream_t s, int rung) {
    const auto& t = c->tab;
    MgpuDev dev = c->dev;                        // kernel argument; the frame stride can differ from the frame length
    if (io.frame_stride > 0) dev.frame_samples = io.frame_stride;
    const size_t stride = size_t(dev.frame_samples);
    MgpuTapsDev tp = taps;
    auto begin_chunk = [&](int off) {            // the per-frame taps have no row offset, so they allow one launch per call; mean_H has one
        if (off && wants_frame_taps(taps)) throw std::invalid_argument("stage taps are limited to one launch per call");
        tp.mean_H = at(io.mean_H, off);
    };
    if (t.mfsk_M > 0) {
        // MFSK modes: workgroups of (frame, run of symbols); keep gridDim * blockDim below 2^32
        const int per = mgpu_mfsk_syms_per_block(), chunks = (t.active_nsymb + per - 1) / per;
        if (!((t.mfsk_M == 32 && t.mfsk_nstreams == 1) || (t.mfsk_M == 16 && t.mfsk_nstreams == 2)) || t.mfsk_off[0] != 9 ||
            (t.mfsk_nstreams == 2 && t.mfsk_off[1] != 25) || t.Nc != 50)
            throw std::runtime_error("MFSK tone plan differs from the one the kernel is specialised for");
        const int max_frames = (1 << 23) / chunks;
        for (int off = 0; off < F; off += max_frames) {
            const int n = F - off < max_frames ? F - off : max_frames;
            begin_chunk(off);
            hipLaunchKernelGGL(t.mfsk_M == 32 ? mgpu_mfsk_frontend_kernel_m32 : mgpu_mfsk_frontend_kernel_m16x2, dim3(unsigned(n) * chunks), dim3(256), 0, s, dev,
                               io.bb + size_t(off) * stride * 2, n, chunks, io.llr + size_t(off) * t.N, io.var + off, at(io.snrvar, off), tp);
            HIPCK(hipGetLastError());
        }
        return;
    }
    if (!rect && c->lad.n > 0 && !c->lad.rung0_is_default) rect = &c->lad.win[0];      // rung 0 of an estimator ladder with a window of its own
    // The launch's form (ls_rect.h): one kernel and one LDS carve per call. A Wiener rung's `rect` carries the frame list alone.
    const bool wiener = rung < c->lad.n && c->lad.kind[rung] == MGPU_RUNG_WIENER;
    const bool nmap = c->dmp.mode == MGPU_DEMAP_NMAP, csi = nmap || c->dmp.mode == MGPU_DEMAP_CSI;     // the noise map is a CSI form with a map of its own
    const bool cfo = c->cfo.mode == MGPU_CFO_PILOTS;
    unsigned form = (wiener ? MGPU_FE_WIENER : 0) | (csi ? MGPU_FE_CSI : 0) | (nmap ? MGPU_FE_NMAP : 0) | (cfo ? MGPU_FE_CFO : 0);
    if (rect || form) form |= MGPU_FE_RECT;                                            // every option runs on a rectangle: the context's own window as one
    const void* kernel = mgpu_frontend_form_kernel(c->fe_threads, form);
    const size_t lds = mgpu_frontend_form_lds_bytes(dev.G, dev.nPilots, dev.nBits, c->fe_threads, form);
    if (!kernel) throw std::runtime_error("the front-end has no kernel for this combination of options");
    for_frame_chunks(F, [&](int off, int n) {
        begin_chunk(off);
        const double* bb = io.bb + size_t(off) * stride * 2;
        float *llr = io.llr + size_t(off) * t.N, *var = io.var + off, *snrvar = at(io.snrvar, off);
        MgpuFeOpt opt{};
        opt.win = rect ? *rect : c->own_window;
        const bool retry = opt.win.frames != nullptr;
        if (retry) { opt.win.frames += off; bb = io.bb; }        // a retry: workgroup b reads frame frames[b] and writes row b
        // what a first pass reports per frame goes to the frames' rows in the context's max_batch-sized arrays, as far as they reach
        const size_t row = size_t(io.frame0) + size_t(off);
        const int rows = !retry && row < size_t(c->max_batch) ? int(std::min(size_t(c->max_batch) - row, size_t(n))) : 0;
        double* eqd = retry ? nullptr : at<double>(c->d_eqdata, row * t.nData * 2);
        opt.csi = c->dmp.arg;
        opt.cfo = c->cfo.arg;
        opt.cfo.step_rows = cfo ? rows : 0;
        opt.cfo.step = opt.cfo.step_rows > 0 ? c->cfo.d_step + row : nullptr;
        opt.nm = c->dmp.nmap;
        opt.nm.rows = nmap ? rows : 0;
        opt.nm.fc = opt.nm.rows > 0 ? c->dmp.d_fc + row * size_t(t.Nc) : nullptr;
        opt.nm.fs = opt.nm.rows > 0 ? c->dmp.d_fs + row * size_t(t.Nsymb) : nullptr;
        if (wiener) opt.wn = c->lad.wiener[rung];
        opt.wn.rows = wiener && opt.wn.n_designs > 1 && rung == 0 ? rows : 0;         // a bank's choices: from rung 0 alone
        opt.wn.choice = opt.wn.rows > 0 ? c->lad.d_choice + row : nullptr;
        opt.wn.corr = opt.wn.rows > 0 ? c->lad.d_corr + row * 4 : nullptr;
        void* args[] = {&dev, &bb, &n, &llr, &var, &snrvar, &eqd, &tp, &opt, nullptr};
        if (form == (MGPU_FE_RECT | MGPU_FE_CSI)) { args[8] = &opt.win; args[9] = &opt.csi; }      // the csi pair takes its two structs themselves (frontend.hip FE_FORMS)
        HIPCK(hipLaunchKernel(kernel, dim3(n), dim3(c->fe_threads), args, lds, s));
    });
}

void frontend_raise_lds_limits(mgpu_ctx* c) {
    for (unsigned form = 0; form < MGPU_FE_FORMS; ++form) {
        const void* kernel = mgpu_frontend_form_kernel(c->fe_threads, form);
        const size_t lds = mgpu_frontend_form_lds_bytes(c->dev.G, c->dev.nPilots, c->dev.nBits, c->fe_threads, form);
        // (a carve beyond a compute unit's LDS: the option that needs it is refused where it is set)
        if (kernel && lds <= size_t(160) * 1024) HIPCK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    }
}

// The timed launchers: the only code that records into the context's event ring, one start and one stop around the untimed launches.
// A slot is a front-end and the decoder launch behind it; the decoder's stop closes it (mgpu_frontend_dev alone leaves it open).
void launch_frontend(mgpu_ctx* c, const SpanIo& io, int F, const MgpuTapsDev& taps, hipStream_t s) {
    auto& k = c->kt;
    const int slot = k.ev_count % k.kEvRing;
    if (k.timing) { HIPCK(hipEventRecord(k.ev[slot][0], s)); k.ev_fe[slot] = true; }
    frontend_untimed(c, io, F, taps, nullptr, s);
    if (k.timing) HIPCK(hipEventRecord(k.ev[slot][1], s));
}

void launch_decoder(mgpu_ctx* c, const float* d_llr, int F, uint8_t* d_bits, int* d_iters, uint8_t* d_payload,
                    MgpuStatsDev* d_stats, const float* d_var, const float* d_snrvar, hipStream_t s) {
    auto& k = c->kt;
    const int slot = k.ev_count % k.kEvRing;
    if (k.timing) HIPCK(hipEventRecord(k.ev[slot][2], s));
    decoder_untimed(c, d_llr, F, d_bits, d_iters, d_payload, d_stats, d_var, d_snrvar, s);
    if (k.timing) { HIPCK(hipEventRecord(k.ev[slot][3], s)); ++k.ev_count; k.ev_fe[k.ev_count % k.kEvRing] = false; }
}

// io.group = D: the D branches of each group share one decode (include/mercury_diversity.h). D = 1 takes the same steps, so the scatter
// is held against the plain span byte for byte. No ladder part: the entry points refuse a ladder with retries, and a one-rung ladder's
// window is the front-end's.
static void launch_group_span(mgpu_ctx* c, const SpanIo& io, int F, const MgpuTapsDev& taps, hipStream_t s, hipEvent_t input_free) {
    const int D = io.group, G = F / D;
    need(F % D == 0 && io.payload && io.stats && F <= c->max_batch, "a grouped span needs payload and stats arrays of G * D <= max_batch frames");
    Diversity& dv = c->div;
    diversity_workspaces(c);
    launch_frontend(c, io, F, taps, s);
    if (input_free) HIPCK(hipEventRecord(input_free, s));                  // the front-end is the only reader of the input
    if (dv.done_recorded) HIPCK(hipStreamWaitEvent(s, dv.done, 0));       // the compact rows are the context's: one grouped span at a time
    launch_llr_combine(io.llr, D, nullptr, nullptr, G, dv.d_llr, s);
    launch_decoder(c, dv.d_llr, G, nullptr, nullptr, dv.d_payload, dv.d_stats, nullptr, nullptr, s);
    launch_group_scatter(c, io, F, D, s);
    HIPCK(hipEventRecord(dv.done, s));
    dv.done_recorded = true;
    if (io.zf_snr) launch_zf_snr(c, io, F, s);     // per row: the group's payload against the branch's own equalised symbols
}

void launch_span(mgpu_ctx* c, const SpanIo& caller_io, int F, const MgpuTapsDev& taps, hipStream_t s, hipEvent_t input_free) {
    // The impulse blanker (include/mercury_blanker.h), when on: in front of the front-end's start event, so that the kernel timings keep
    // describing the front-end. It is the only reader of the caller's buffer (input_free is recorded right behind it); everything from here
    // on, the ladder's retries and the grouped span included, reads the blanked frames in the context's workspace.
    const bool blank = c->blk.mode == MGPU_BLANK_MEDIAN;
    const SpanIo blanked = blank ? blanked_span(c, caller_io, F, s, input_free) : SpanIo{};
    const SpanIo& io = blank ? blanked : caller_io;
    if (blank) input_free = nullptr;
    if (io.group > 0) { launch_group_span(c, io, F, taps, s, input_free); return; }
    const bool retries = c->lad.n > 1;           // an estimator ladder's retries read the input again
    launch_frontend(c, io, F, taps, s);
    if (input_free && !retries) HIPCK(hipEventRecord(input_free, s));      // the front-end is the only reader of the input
    launch_decoder(c, io.llr, F, nullptr, nullptr, io.payload, io.stats, io.var, io.snrvar, s);
    launch_ladder(c, io, F, s);
    if (input_free && retries) HIPCK(hipEventRecord(input_free, s));
    if (io.zf_snr) launch_zf_snr(c, io, F, s);
}

void select_peak(const double* cand_vals, int ncand, int step, int size, int location_to_return, int nTrials_max, int* delay, double* corr) {
    // The reference fills vals[k*step] = metric of candidate k, leaves every other entry 0, and for j = 0..nTrials_max-1
    // sets loc[j] = j and scans i = j+1..size-1 replacing (vals[j], loc[j]) by any strictly larger vals[i] — nothing is
    // swapped out, so later passes see the same maximum again. Emulated without the size-long arrays: a pass only
    // meets candidates and zeros, and a zero matters only the first time it is met while the running value is negative.
    if (location_to_return >= nTrials_max) location_to_return = nTrials_max - 1;
    const int j = location_to_return;
    auto original = [&](int i) { return (i % step == 0 && i / step < ncand) ? cand_vals[i / step] : 0.0; };
    double cur = j < size ? original(j) : 0.0;
    int loc = j;
    int p = j + 1;                                   // next index the scan visits
    for (int k = (j + step) / step; k < ncand; ++k) {               // candidates with index k*step > j
        const int ci = k * step;
        if (ci <= j) continue;
        if (p < ci && cur < 0) { cur = 0.0; loc = p; }               // a non-candidate (zero) entry comes first
        if (cand_vals[k] > cur) { cur = cand_vals[k]; loc = ci; }
        p = ci + 1;
    }
    if (p < size && cur < 0) { cur = 0.0; loc = p; }
    *delay = loc;
    *corr = cur;
}

const double* mixer_table(mgpu_ctx* c, double carrier_hz, size_t count, hipStream_t s) {
    if (c->mix_carrier == carrier_hz && c->mix_count >= count) return c->d_mix_cs;
    std::vector<double> cs(2 * count);
    const double Ts = 1.0 / kSampleRate;
    // ofdm.cc:2331-2332 evaluates cos and sin of one phase; the reference's compiler merges the pair into a single sincos() call, and glibc's
    // sincos is not bit-for-bit its cos + sin, so the same call is made here
    for (size_t i = 0; i < count; ++i) ::sincos(2 * M_PI * carrier_hz * double(int(i)) * Ts, &cs[2 * i + 1], &cs[2 * i]);
    HIPCK(hipStreamSynchronize(s));
    c->mix_count = 0;                    // no table until the new one is in place
    c->d_mix_cs.grow(cs.size() * 8);
    HIPCK(hipMemcpy(c->d_mix_cs, cs.data(), cs.size() * 8, hipMemcpyHostToDevice));
    c->mix_carrier = carrier_hz; c->mix_count = count;
    return c->d_mix_cs;
}

// The streaming coarse kernel (sync.hip: mgpu_tsync_metric_stream_kernel) when the geometry fits it and there are enough windows to give
// every SIMD a wavefront; false = use the staged kernel. MERCURY_TSYNC_STREAM=0 / 1 forces the choice (tests compare the two).
static bool tsync_stream_launch(const double* d_bb, int stride, const int* d_start, const int* d_widx, const int* d_ncand, int ncand_max, int n, int step,
                                int pre_nsymb, int ngi_i, int nfft_i, double* d_vals, hipStream_t s, int variant) {
    static const int env = [] { const char* e = getenv("MERCURY_TSYNC_STREAM"); return e ? atoi(e) : -1; }();
    const int force = variant >= 0 ? variant : env;
    if (force == 0 || (force < 0 && n < 32)) return false;                   // measured: 16 windows 0.21 vs 0.17 ms staged, 64 windows 0.26 vs 0.34 ms
    const MgpuStreamGeometry g = mgpu_tsync_stream_geometry();
    if (step != g.step || ngi_i != g.ngi || nfft_i != g.nfft || pre_nsymb != g.pre) return false;      // the kernel is built for the reference's coarse search
    const int K = g.K, ring = g.ring;
    const int sym = ngi_i + nfft_i, half = nfft_i / 2, PS = ngi_i + half, NP = pre_nsymb * PS;
    const int J = (NP + K - 1) / K;
    // the span the candidates in flight read, relative to step * (newest candidate): candidate `e` periods older is at pair rho + K*e
    int lo = 1 << 30, hi = -(1 << 30);
    for (int rho = 0; rho < K; rho += 4)
        for (int e = 0; e < J; ++e) {
            const int np = rho + K * e;
            if (np >= NP) break;
            const int l = np / PS, k = np % PS, a = l * sym + k, b = a + (k < ngi_i ? nfft_i : half);
            lo = std::min(lo, a - step * e);
            hi = std::max(hi, b + 4 - step * e);
        }
    if (hi - lo + 128 > ring) return false;
    // pieces of the candidate range per window: about one wavefront per SIMD (4 rings of 35 KB fit a CU's LDS), at least J candidates each
    int pieces = std::max(1, (1024 + n - 1) / n);               // ceil: 618 windows in two pieces each measured faster than one wavefront per window
    pieces = std::min(pieces, std::max(1, ncand_max / J));
    const int cpp = (ncand_max + pieces - 1) / pieces;
    pieces = (ncand_max + cpp - 1) / cpp;
    hipLaunchKernelGGL(mgpu_tsync_metric_stream_kernel, dim3(n, pieces), dim3(64), 0, s, d_bb, stride, d_start, d_widx, d_ncand, ncand_max, d_vals, lo, hi, cpp);
    return true;
}

void launch_tsync_metric(const double* d_bb, int stride, const int* d_start, const int* d_widx, const int* d_ncand, int ncand_max, int n, int step,
                         int pre_nsymb, int ngi_i, int nfft_i, double* d_vals, hipStream_t s, int variant) {
    if (ngi_i % 64 || (nfft_i / 2) % 64) {    // the staged kernels walk the preamble in chunks of 8 / 64 pairs
        hipLaunchKernelGGL(mgpu_tsync_metric_generic_kernel, dim3((ncand_max + 63) / 64, n), dim3(64), 0, s, d_bb, stride, d_start, d_widx, d_ncand,
                           ncand_max, step, pre_nsymb, ngi_i, nfft_i, d_vals);
    } else if (step == 1 && ngi_i == 64 * (ngi_i / 64) && (variant > 0 || (variant < 0 && n >= 32))) {
        // fine search over many windows: R adjacent candidates per lane share every sample's products (sync.hip). variant 1: R = 4, 2: R = 8;
        // -1 picks by the number of windows (ms per launch of 4352 candidates, dense / R = 4 / R = 8: 16 windows 0.18 / 0.18 / 0.29,
        // 64: 0.40 / 0.33 / 0.31, 256: 1.24 / 0.81 / 0.84, 1024: 5.13 / 2.91 / 2.71). A few windows keep the dense kernel (one candidate
        // per lane: four times the wavefronts, a quarter of the latency).
        if (variant < 0) variant = n >= 512 ? 2 : 1;
        const MgpuKernelGeometry g = mgpu_tsync_fine_geometry(variant == 2 ? 8 : 4);      // the kernels' LDS limits are raised per device in mgpu_create
        hipLaunchKernelGGL(variant == 2 ? mgpu_tsync_metric_fine_kernel_r8 : mgpu_tsync_metric_fine_kernel_r4, dim3((ncand_max + g.outputs_per_block - 1) / g.outputs_per_block, n),
                           dim3(g.threads), size_t(g.lds_bytes), s, d_bb, stride, d_start, d_widx, d_ncand, ncand_max, pre_nsymb, ngi_i, nfft_i, d_vals);
    } else if (step > 4 && tsync_stream_launch(d_bb, stride, d_start, d_widx, d_ncand, ncand_max, n, step, pre_nsymb, ngi_i, nfft_i, d_vals, s, variant)) {
        // many windows: one wavefront streams each (piece of a) window through an LDS ring, see sync.hip
    } else {
        // The coarse search re-reads every sample ~44 times (overlapping candidates) and is bound by that traffic. Launching it over
        // 64 windows at a time keeps the windows in flight (95 MB) inside the 256 MB Infinity Cache instead of streaming 1.5 GB per
        // 1024 windows from HBM: 10.4 -> 7.1 ms per 1024 windows (MERCURY_TSYNC_SLICE overrides; 0 = one launch).
        static const int slice = [] { const char* e = getenv("MERCURY_TSYNC_SLICE"); return e ? atoi(e) : 64; }();
        const int per = (slice > 0 && step > 4) ? slice : n;
        for (int off = 0; off < n; off += per) {
            const int m = std::min(per, n - off);
            const int threads = step <= 4 ? 256 : mgpu_tsync_coarse_threads();
            const int nblk = (ncand_max + threads - 1) / threads;
            // coarse kernel: windows along x, so that with a multiple of 8 windows per launch all workgroups of a window land on one XCD
            hipLaunchKernelGGL(step <= 4 ? mgpu_tsync_metric_dense_kernel : mgpu_tsync_metric_kernel, step <= 4 ? dim3(nblk, m) : dim3(m, nblk), dim3(threads), 0, s,
                               d_widx ? d_bb : d_bb + size_t(off) * stride * 2, stride, at(d_start, size_t(off)), at(d_widx, size_t(off)), at(d_ncand, size_t(off)),
                               ncand_max, step, pre_nsymb, ngi_i, nfft_i, d_vals + size_t(off) * ncand_max);
        }
    }
    HIPCK(hipGetLastError());
}

// -1: pick (sliding-tap kernels where they apply), 0: always the generic kernel, 1: as -1; test hook mgpu_debug_p2b_variant
static std::atomic<int> g_p2b_variant{-1};
extern "C" int mgpu_debug_p2b_variant(int v) { const int old = g_p2b_variant.exchange(v); return old; }

void launch_p2b(const double* passband, int in_size, const double* d_carrier, const int* d_start, int start_all, int count, int decim, const double* d_taps,
                int ntaps, double* out, const int* widx, const double* cs, const int* out_row, int row_by_launch, int nwin, hipStream_t s) {
    if (g_p2b_variant.load() != 0 && ntaps == 33 && (decim == 1 || decim == 4)) {
        const MgpuKernelGeometry g = mgpu_p2b_slide_geometry(decim);
        auto kernel = decim == 1 ? (cs ? mgpu_p2b_slide_d1_kernel : mgpu_p2b_slide_d1_sincos_kernel) : (cs ? mgpu_p2b_slide_d4_kernel : mgpu_p2b_slide_d4_sincos_kernel);
        hipLaunchKernelGGL(kernel, dim3((count + g.outputs_per_block - 1) / g.outputs_per_block, unsigned(nwin)), dim3(g.threads), size_t(g.lds_bytes), s, passband,
                           in_size, d_carrier, d_start, start_all, count, d_taps, kSampleRate, kCarrierAmplitude, out, widx, cs, out_row, row_by_launch);
    } else {
        const size_t lds = size_t(255 * decim + ntaps) * 16;
        need(lds <= 64 * 1024 && ntaps <= 64, "decimation too large for the staging buffer");
        hipLaunchKernelGGL(mgpu_p2b_kernel, dim3((count + 255) / 256, unsigned(nwin)), dim3(256), lds, s, passband, in_size, d_carrier, d_start, start_all, count, decim,
                           d_taps, ntaps, kSampleRate, kCarrierAmplitude, out, widx, cs, out_row, row_by_launch);
    }
    HIPCK(hipGetLastError());
}

static constexpr int kTones32[4] = {4, 20, 12, 28}, kTones16[4] = {2, 10, 6, 14};      // mfsk.cc:82-95

// the same search on the device, for the energies of W windows lying in d_energy ([W][nslots][Nc]); d_search_start: [W] or null
void launch_mfsk_sync(mgpu_ctx* c, const double* d_energy, int W, int nslots, int size, const int* d_search_start, int* d_delay, hipStream_t s) {
    const auto& t = c->tab;
    need(t.preamble >= 1 && t.preamble <= 4 && t.mfsk_nstreams >= 1 && t.mfsk_nstreams <= 4, "MFSK preamble / stream count outside the kernel's tables");
    MgpuMfskSync P{};
    P.np = t.preamble; P.nstreams = t.mfsk_nstreams; P.Nc = t.Nc; P.sym_period = t.Nofdm * kInterp; P.tail = t.Ngi * kInterp + t.Nfft * kInterp;
    for (int i = 0; i < 4; ++i) P.off[i] = t.mfsk_off[i];
    for (int p = 0; p < P.np; ++p) P.tones[p] = (t.mfsk_M == 32 ? kTones32 : kTones16)[p % P.np];
    hipLaunchKernelGGL(mgpu_mfsk_sync_kernel, dim3(W), dim3(256), size_t(P.np) * nslots * 8, s, d_energy, nslots, size, P, d_search_start, d_delay);
    HIPCK(hipGetLastError());
}

int mfsk_sync_from_energies(const mgpu::ModeTables& t, const double* E, int nslots, int size, int search_start_symb) {
    const int* tones = t.mfsk_M == 32 ? kTones32 : kTones16;
    const int sym_period = t.Nofdm * kInterp, np = t.preamble;
    double best_metric = -1;
    int best = 0;
    for (int s = search_start_symb > 0 ? search_start_symb : 0; s <= nslots - np; ++s) {
        double metric = 0;
        for (int p = 0; p < np; ++p) {
            if ((s + p) * sym_period + t.Ngi * kInterp + t.Nfft * kInterp > size) break;
            const double* e = &E[size_t(s + p) * t.Nc];
            double e_target = 0;
            for (int st = 0; st < t.mfsk_nstreams; ++st) e_target += e[t.mfsk_off[st] + tones[p % np]];
            double e_total = 0;
            for (int k = 0; k < t.Nc; ++k) e_total += e[k];
            if (e_total > 0) metric += e_target / e_total;
        }
        if (metric > best_metric) { best_metric = metric; best = s; }
    }
    return best * sym_period;
}

// zero-forcing modes: SNR from the re-encoded decision (telecom_system.cc:1374-1396); needs the payload and
// the de-framed equalised symbols the front-end kept.
void launch_zf_snr(mgpu_ctx* c, const SpanIo& io, int F, hipStream_t s) {
    const auto& t = c->tab;
    if (t.estimator != MGPU_EST_ZF || !io.payload || !io.stats) return;
    for_frame_chunks(F, [&](int off, int n) {
        hipLaunchKernelGGL(mgpu_zf_snr_kernel, dim3(n), dim3(256), mgpu_zfsnr_lds_bytes(t.nData), s, c->dev,
                           io.payload + size_t(off) * t.payload_stride, c->d_eqdata + (size_t(io.frame0) + off) * t.nData * 2, n, io.stats + off,
                           at(io.zf_var, off));
        HIPCK(hipGetLastError());
    });
}

void decoder_untimed(mgpu_ctx* c, const float* d_llr, int F, uint8_t* d_bits, int* d_iters, uint8_t* d_payload,
                     MgpuStatsDev* d_stats, const float* d_var, const float* d_snrvar, hipStream_t s) {
    const auto& t = c->tab;
    for_frame_chunks(F, [&](int off, int n) {
        const float* llr = d_llr + size_t(off) * t.N;
        uint8_t* bits = at(d_bits, size_t(off) * t.K);
        int* iters = at(d_iters, off);
        uint8_t* pay = at(d_payload, size_t(off) * t.payload_stride);
        MgpuStatsDev* st = at(d_stats, off);
        const float* var = at(d_var, off);
        const float* sv = at(d_snrvar, off);
        if (c->cfg.decoder == MGPU_DEC_GBF)
            hipLaunchKernelGGL(mgpu_ldpc_gbf_kernel, dim3(n), dim3(1024), c->lds_dec, s, c->ldev, llr, n, bits, iters, pay, st, var, sv);
        else   // sum-product or min-sum, the variant for this graph's round count
            hipLaunchKernelGGL(c->spa_kernel, dim3(n), dim3(c->dec_threads), c->lds_dec, s, c->ldev, llr, n, bits, iters, pay, st, var, sv);
        HIPCK(hipGetLastError());
    });
}

void launch_txgen(mgpu_ctx* c, uint64_t seed, uint64_t frame0, int F, double noise_amp, int channel, double* d_bb, uint8_t* d_payload, hipStream_t s,
                  const uint8_t* tx_payload, int tx_stride, const int* d_nbytes) {
    const auto& t = c->tab;
    for_frame_chunks(F, [&](int off, int n) {
        hipLaunchKernelGGL(mgpu_txgen_kernel, dim3(n), dim3(256), c->lds_tx, s, c->dev, seed, frame0 + uint64_t(off), n, noise_amp, channel,
                           d_bb + size_t(off) * t.frame_samples * 2, at(d_payload, size_t(off) * t.payload_stride),
                           at(tx_payload, size_t(off) * size_t(tx_stride < 0 ? -tx_stride : tx_stride)), tx_stride, at(d_nbytes, size_t(off)), 0, 0);
        HIPCK(hipGetLastError());
    });
}

}  // namespace mgpu_detail

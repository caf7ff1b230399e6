// The RX hot path's entry points (include/mercury_gpu.h): front-end and decoder on device buffers, the blocking host-buffer batch calls
// (one-frame graph, double-buffered pipeline, stage taps), device memory / copy / sync helpers and the kernel timing queries.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "ctx.hpp"

extern "C" {

int mgpu_enable_timing(mgpu_ctx* c, int on) {
    if (!c) return MGPU_ERR_ARG;
    c->kt.timing = on != 0;
    c->kt.ev_count = 0;
    for (auto& b : c->kt.ev_fe) b = false;
    return MGPU_OK;
}

int mgpu_decoder_hard_frames(mgpu_ctx* c, long long* frames) {
    if (!c || !frames) return MGPU_ERR_ARG;
    return guard(c, [&] {
        HIPCK(hipStreamSynchronize(c->stream));
        unsigned long long v[64];
        HIPCK(hipMemcpy(v, c->ldev.hard_frames, sizeof(v), hipMemcpyDeviceToHost));
        long long sum = 0;
        for (unsigned long long x : v) sum += (long long)x;
        *frames = sum;
    });
}

int mgpu_last_kernel_ms(mgpu_ctx* c, float ms[2]) {
    int n = 0;
    return mgpu_kernel_ms_avg(c, ms, &n);
}

int mgpu_kernel_ms_avg(mgpu_ctx* c, float ms[2], int* n_launches) {
    if (!c || !ms) return MGPU_ERR_ARG;
    return guard(c, [&] {
        const auto& k = c->kt;
        need(k.timing && k.ev_count > 0, "timing not enabled or nothing launched");
        const int n = k.ev_count < k.kEvRing ? k.ev_count : k.kEvRing;
        double fe = 0, dec = 0;
        int nfe = 0;
        for (int i = 0; i < n; ++i) {
            HIPCK(hipEventSynchronize(k.ev[i][3]));
            float t = 0;
            HIPCK(hipEventElapsedTime(&t, k.ev[i][2], k.ev[i][3]));
            dec += t;
            if (k.ev_fe[i]) { HIPCK(hipEventElapsedTime(&t, k.ev[i][0], k.ev[i][1])); fe += t; ++nfe; }
        }
        ms[0] = nfe ? float(fe / nfe) : 0.f;
        ms[1] = float(dec / n);
        if (n_launches) *n_launches = n;
    });
}

int mgpu_frontend_dev(mgpu_ctx* c, const void* d_bb, int F, void* d_llr, void* d_variance_f, void* stream) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(d_bb && d_llr && F >= 0 && F <= c->max_batch, "bad argument (F must be <= max_batch)");
        if (F == 0) return;
        ensure_workspaces(c, WS_FRONTEND);
        SpanIo io;
        io.bb = static_cast<const double*>(d_bb); io.llr = static_cast<float*>(d_llr);
        io.var = d_variance_f ? static_cast<float*>(d_variance_f) : c->d_variance; io.snrvar = c->d_snrvar;
        launch_frontend(c, io, F, MgpuTapsDev{}, static_cast<hipStream_t>(stream));
    });
}

int mgpu_ldpc_batch_dev(mgpu_ctx* c, const void* d_llr, int F, void* d_bits, void* d_iters, void* d_payload,
                        void* d_stats, const void* d_variance_f, void* stream) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(d_llr && F >= 0 && F <= c->max_batch, "bad argument (F must be <= max_batch)");
        if (F == 0) return;
        launch_decoder(c, static_cast<const float*>(d_llr), F, static_cast<uint8_t*>(d_bits), static_cast<int*>(d_iters),
                       static_cast<uint8_t*>(d_payload), static_cast<MgpuStatsDev*>(d_stats),
                       static_cast<const float*>(d_variance_f), nullptr, static_cast<hipStream_t>(stream));
    });
}

int mgpu_rx_batch_dev(mgpu_ctx* c, const void* d_bb, int F, void* d_payload, void* d_stats, void* d_llr_opt, void* stream) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(d_bb && d_payload && d_stats && F >= 0 && F <= c->max_batch, "bad argument (F must be <= max_batch)");
        if (F == 0) return;
        ensure_workspaces(c, WS_FRONTEND | (d_llr_opt ? 0u : unsigned(WS_LLR)));
        SpanIo io = own_span(c);
        io.bb = static_cast<const double*>(d_bb);
        if (d_llr_opt) io.llr = static_cast<float*>(d_llr_opt);
        io.payload = static_cast<uint8_t*>(d_payload); io.stats = static_cast<MgpuStatsDev*>(d_stats);
        launch_span(c, io, F, MgpuTapsDev{}, static_cast<hipStream_t>(stream));
    });
}

void* mgpu_device_malloc(mgpu_ctx* c, size_t bytes) {
    if (!c) return nullptr;
    void* p = nullptr;
    const int rc = guard(c, [&] { HIPCK(hipMalloc(&p, bytes ? bytes : 1)); });
    return rc == MGPU_OK ? p : nullptr;
}
void mgpu_device_free(mgpu_ctx* c, void* d_ptr) {
    if (c && d_ptr) (void)guard(c, [&] { HIPCK(hipFree(d_ptr)); });
}
void* mgpu_context_stream(mgpu_ctx* c) { return c ? static_cast<void*>(c->stream) : nullptr; }
int mgpu_synchronize(mgpu_ctx* c, void* stream) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] { HIPCK(hipStreamSynchronize(stream_or_own(c, stream))); });
}
static int copy_and_wait(mgpu_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, void* stream) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need((dst && src) || bytes == 0, "bad argument");
        hipStream_t s = stream_or_own(c, stream);
        if (bytes) HIPCK(hipMemcpyAsync(dst, src, bytes, kind, s));
        HIPCK(hipStreamSynchronize(s));
    });
}
int mgpu_copy_to_host(mgpu_ctx* c, void* dst, const void* d_src, size_t bytes, void* stream) {
    return copy_and_wait(c, dst, d_src, bytes, hipMemcpyDeviceToHost, stream);
}
int mgpu_copy_to_device(mgpu_ctx* c, void* d_dst, const void* src, size_t bytes, void* stream) {
    return copy_and_wait(c, d_dst, src, bytes, hipMemcpyHostToDevice, stream);
}

int mgpu_txgen_dev(mgpu_ctx* c, uint64_t seed, uint64_t frame0, int F, double noise_amp, int channel, void* d_bb,
                   void* d_payload_opt, void* stream) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(d_bb && F >= 0 && (channel == 0 || channel == 1), "bad argument");
        if (F == 0) return;
        launch_txgen(c, seed, frame0, F, noise_amp, channel, static_cast<double*>(d_bb), static_cast<uint8_t*>(d_payload_opt), static_cast<hipStream_t>(stream));
    });
}

int mgpu_rx_batch_taps(mgpu_ctx* c, const double* bb, int F, uint8_t* payload, mgpu_frame_stats* stats, const mgpu_stage_taps* taps) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(bb && F >= 0 && F <= c->max_batch, "bad argument (F must be <= max_batch)");
        if (F == 0) return;
        const auto& t = c->tab;
        const size_t in_bytes = size_t(F) * t.frame_samples * 16;
        ensure_workspaces(c, WS_FRONTEND | WS_LLR | WS_OUT);
        c->d_baseband.grow(in_bytes);
        hipStream_t s = c->stream;
        HIPCK(hipMemcpyAsync(c->d_baseband, bb, in_bytes, hipMemcpyHostToDevice, s));
        MgpuTapsDev dt{};
        const size_t G = size_t(t.Nsymb) * t.Nc;
        std::vector<DevBuf> tmp;             // the taps' device buffers, for this call
        auto dalloc = [&](size_t bytes) { tmp.emplace_back(bytes); return tmp.back().p; };
        if (taps) {
            if (taps->grid) { dt.grid = static_cast<double*>(dalloc(F * G * 16)); if (t.mfsk_M > 0) HIPCK(hipMemsetAsync(dt.grid, 0, F * G * 16, s)); }
            need(t.mfsk_M == 0 || !(taps->H || taps->eq || taps->syms), "the MFSK modes have no channel estimate / equalised grid to tap");
            if (taps->H) dt.H = static_cast<double*>(dalloc(F * G * 16));
            if (taps->eq) dt.eq = static_cast<double*>(dalloc(F * G * 16));
            if (taps->syms) dt.syms = static_cast<double*>(dalloc(size_t(F) * t.nData * 16));
            if (taps->llr_demod) dt.llr_demod = static_cast<float*>(dalloc(size_t(F) * t.nBits * 4));
            if (taps->variance) dt.variance = static_cast<double*>(dalloc(size_t(F) * 8));
            if (taps->cycles) { dt.cycles = static_cast<long long*>(dalloc(16 * 8)); HIPCK(hipMemsetAsync(dt.cycles, 0, 16 * 8, s)); }
            if (taps->agc_gain) { dt.agc_gain = static_cast<double*>(dalloc(size_t(F) * 8)); HIPCK(hipMemsetAsync(dt.agc_gain, 0, size_t(F) * 8, s)); }
        }
        SpanIo io = own_span(c);
        io.bb = c->d_baseband;
        launch_span(c, io, F, dt, s);        // the taps stay rung 0's
        if (payload) HIPCK(hipMemcpyAsync(payload, c->d_payload, size_t(F) * t.payload_stride, hipMemcpyDeviceToHost, s));
        if (stats) HIPCK(hipMemcpyAsync(stats, c->d_stats, size_t(F) * sizeof(MgpuStatsDev), hipMemcpyDeviceToHost, s));
        if (taps) {
            auto back = [&](void* h, void* d, size_t bytes) { if (h) HIPCK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s)); };
            back(taps->grid, dt.grid, F * G * 16); back(taps->H, dt.H, F * G * 16); back(taps->eq, dt.eq, F * G * 16);
            back(taps->syms, dt.syms, size_t(F) * t.nData * 16); back(taps->llr_demod, dt.llr_demod, size_t(F) * t.nBits * 4);
            back(taps->variance, dt.variance, size_t(F) * 8); back(taps->agc_gain, dt.agc_gain, size_t(F) * 8);
            back(taps->llr_ldpc, c->d_llr, size_t(F) * t.N * 4);
            back(taps->cycles, dt.cycles, 16 * 8);
        }
        HIPCK(hipStreamSynchronize(s));
    });
}

// One frame per call is how the reference's receive_byte uses this span, and at that size the call is bound by launch and
// copy submission, not by the kernels: the whole sequence (H2D, front-end, decoder, [ZF SNR], D2H x2) is captured once into
// a hipGraph over fixed page-locked staging buffers and replayed with a single launch.
static int rx_one_frame(mgpu_ctx* c, const double* bb, uint8_t* payload, mgpu_frame_stats* stats) {
    return guard(c, [&] {
        const auto& t = c->tab;
        const size_t in_bytes = size_t(t.frame_samples) * 16, out_bytes = size_t(t.payload_stride) + sizeof(MgpuStatsDev);
        hipStream_t s = c->stream;
        auto& one = c->one;
        if (!one.graph) {
            ensure_workspaces(c, WS_FRONTEND | WS_LLR | WS_OUT);
            // The graph bakes in every address it touches, so it reads from a device buffer and staging buffers of its own
            // that live as long as the context (d_baseband may be reallocated by a larger batch later; the max_batch-sized
            // workspaces never are). Nothing is published in the context until the whole graph exists.
            one.d_in.grow(in_bytes);
            if (!one.h_in) HIPCK(host_alloc_on_node(&one.h_in.h, in_bytes, c->numa_node));
            if (!one.h_out) HIPCK(host_alloc_on_node(&one.h_out.h, out_bytes, c->numa_node));
            hipGraph_t graph = nullptr;
            HIPCK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            try {
                HIPCK(hipMemcpyAsync(one.d_in, one.h_in, in_bytes, hipMemcpyHostToDevice, s));
                SpanIo io = own_span(c);
                io.bb = one.d_in;
                launch_span(c, io, 1, MgpuTapsDev{}, s);      // no ladder is set here (mgpu_rx_batch): its part returns before any HIP call
                HIPCK(hipMemcpyAsync(one.h_out, c->d_payload, t.payload_stride, hipMemcpyDeviceToHost, s));
                HIPCK(hipMemcpyAsync(static_cast<char*>(one.h_out.h) + t.payload_stride, c->d_stats, sizeof(MgpuStatsDev), hipMemcpyDeviceToHost, s));
            } catch (...) {
                (void)hipStreamEndCapture(s, &graph);
                if (graph) (void)hipGraphDestroy(graph);
                throw;
            }
            HIPCK(hipStreamEndCapture(s, &graph));
            hipGraphExec_t exec = nullptr;
            const hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            HIPCK(e);
            one.graph.h = exec;
        }
        std::memcpy(one.h_in, bb, in_bytes);
        HIPCK(hipGraphLaunch(one.graph, s));
        HIPCK(hipStreamSynchronize(s));
        if (payload) std::memcpy(payload, one.h_out, t.payload_stride);
        if (stats) std::memcpy(stats, static_cast<char*>(one.h_out.h) + t.payload_stride, sizeof(MgpuStatsDev));
    });
}

// Chunk size: a decoder launch keeps the whole chip busy only from 2 workgroups per CU upwards (512 codewords on 256 CUs; a
// smaller launch takes just as long), and a copy should carry a few MB; so chunks are multiples of that wave of workgroups
// and a batch that is not larger than one chunk goes through in one piece.
static int pipeline_chunk_frames(mgpu_ctx* c, int F, size_t frame_bytes) {
    int& wave_of_wgs = c->hp.wave_of_wgs;
    if (wave_of_wgs == 0) {              // per context: the devices of a pool need not be alike
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->cfg.device);
        wave_of_wgs = 2 * (cus > 0 ? cus : 256);
    }
    int chunk = wave_of_wgs;
    while (size_t(chunk) * frame_bytes < (size_t(8) << 20)) chunk += wave_of_wgs;
    if (const char* e = std::getenv("MERCURY_RX_CHUNK")) chunk = std::max(1, std::atoi(e));
    return std::min(chunk, F);
}

// The two pipes' streams, events and input buffers of `in_bytes`, the profile's events and the result staging, made on first use.
static void pipeline_resources(mgpu_ctx* c, size_t in_bytes, size_t out_bytes) {
    for (auto& p : c->hp.pipe) {
        if (!p.stream) HIPCK(hipStreamCreateWithFlags(&p.stream.h, hipStreamNonBlocking));
        if (!p.done) HIPCK(hipEventCreateWithFlags(&p.done.h, hipEventDisableTiming));
        if (!p.copied) HIPCK(hipEventCreateWithFlags(&p.copied.h, hipEventDisableTiming));
        if (p.d_in.capacity() < in_bytes) {
            HIPCK(hipStreamSynchronize(p.stream));
            p.d_in.grow(in_bytes);
        }
    }
    // Results come back through page-locked staging owned by the context: a device-to-host copy into the caller's pageable
    // arrays would block the host until the chunk's kernels have finished, i.e. before the next chunk's input copy could even
    // be queued, and nothing would overlap.
    if (!c->hp.h_out) HIPCK(host_alloc_on_node(&c->hp.h_out.h, out_bytes + 16, c->numa_node));
    for (auto& e : c->hp.ev) if (!e) HIPCK(hipEventCreate(&e.h));
}

// The blocking host-buffer entry point for F > 1 with no stage taps: classic double buffering. The batch goes through in
// chunks; a copy stream brings chunk i+1 (104 KB per mode-8 frame over PCIe) into the second input buffer while the kernel
// stream runs the front-end and the decoder of chunk i; the kernels stay in order on one stream (two decoder launches sharing
// the CUs only delay each other), events hand the buffers back and forth, and the small payload / stats copies ride behind each
// chunk into page-locked staging. The LLR / variance / payload / stats workspaces are the max_batch-sized ones, addressed by
// frame offset. Results are byte-identical to the one-launch path (frames are independent).
static void rx_batch_pipelined(mgpu_ctx* c, const double* bb, int F, uint8_t* payload, mgpu_frame_stats* stats) {
    const auto& t = c->tab;
    auto& hp = c->hp;
    ensure_workspaces(c, WS_FRONTEND | WS_LLR | WS_OUT);
    const size_t frame_bytes = size_t(t.frame_samples) * 16;
    const int chunk = pipeline_chunk_frames(c, F, frame_bytes);
    pipeline_resources(c, size_t(chunk) * frame_bytes, size_t(c->max_batch) * (t.payload_stride + sizeof(MgpuStatsDev)));
    uint8_t* h_payload = static_cast<uint8_t*>(hp.h_out.h);
    MgpuStatsDev* h_stats = reinterpret_cast<MgpuStatsDev*>(h_payload + ((size_t(c->max_batch) * t.payload_stride + 15) & ~size_t(15)));
    // Two ways to overlap, chosen by the kind of host memory (measured on MI355X / PCIe Gen5, tools/bench_host_path.py):
    //  * page-locked input (mgpu_alloc_host, hipHostMalloc/Register): the copy is a true asynchronous DMA. One copy stream runs
    //    ahead into the other input buffer while ONE kernel stream keeps the launches in order (two decoder launches sharing the
    //    CUs only delay each other); events hand the buffers back and forth.
    //  * pageable input: the runtime stages the copy itself and holds the calling thread until it is done, which already paces
    //    the copies one behind the other; each chunk's copy and kernels then go to the stream that owns the chunk's input
    //    buffer (two streams alternating), so a copy waits exactly for the front-end that last read its buffer.
    hipPointerAttribute_t attr{};
    const bool pinned = hipPointerGetAttributes(&attr, bb) == hipSuccess && attr.type == hipMemoryTypeHost;
    if (!pinned) (void)hipGetLastError();
    const int nchunks = (F + chunk - 1) / chunk;
    int k = 0;
    for (int off = 0; off < F; off += chunk, ++k) {
        auto& p = hp.pipe[k % hp.kPipes];                            // input buffer of this chunk
        hipStream_t cs = pinned ? hp.pipe[0].stream : p.stream, ks = pinned ? hp.pipe[1].stream : p.stream;
        const int n = std::min(chunk, F - off);
        if (pinned && k >= hp.kPipes) HIPCK(hipStreamWaitEvent(cs, p.done, 0));                 // the span of chunk k-2 has consumed it
        if (k == 0) HIPCK(hipEventRecord(hp.ev[0], cs));
        HIPCK(hipMemcpyAsync(p.d_in, reinterpret_cast<const char*>(bb) + size_t(off) * frame_bytes, size_t(n) * frame_bytes, hipMemcpyHostToDevice, cs));
        if (k == 0) HIPCK(hipEventRecord(hp.ev[1], cs));             // fill: nothing can compute before the first chunk has landed
        if (k == nchunks - 1) HIPCK(hipEventRecord(hp.ev[2], cs));   // drain: what is left when the last input byte has landed
        if (pinned) {
            HIPCK(hipEventRecord(p.copied, cs));
            HIPCK(hipStreamWaitEvent(ks, p.copied, 0));
        }
        SpanIo io = own_span(c, off);
        io.bb = p.d_in;
        launch_span(c, io, n, MgpuTapsDev{}, ks, pinned ? static_cast<hipEvent_t>(p.done) : nullptr);     // p.done: behind the input's last reader
        if (payload) HIPCK(hipMemcpyAsync(h_payload + size_t(off) * t.payload_stride, io.payload, size_t(n) * t.payload_stride, hipMemcpyDeviceToHost, ks));
        if (stats) HIPCK(hipMemcpyAsync(h_stats + off, io.stats, size_t(n) * sizeof(MgpuStatsDev), hipMemcpyDeviceToHost, ks));
        if (k == nchunks - 1) HIPCK(hipEventRecord(hp.ev[3], ks));
    }
    for (auto& p : hp.pipe) HIPCK(hipStreamSynchronize(p.stream));
    hp.chunk = chunk; hp.nchunks = nchunks;
    (void)hipEventElapsedTime(&hp.fill_ms, hp.ev[0], hp.ev[1]);
    (void)hipEventElapsedTime(&hp.drain_ms, hp.ev[2], hp.ev[3]);
    (void)hipEventElapsedTime(&hp.total_ms, hp.ev[0], hp.ev[3]);
    if (payload) std::memcpy(payload, h_payload, size_t(F) * t.payload_stride);
    if (stats) std::memcpy(stats, h_stats, size_t(F) * sizeof(MgpuStatsDev));
}

int mgpu_host_path_last(mgpu_ctx* c, int* chunk_frames, int* n_chunks, float* fill_ms, float* drain_ms, float* total_ms) {
    if (!c) return MGPU_ERR_ARG;
    if (chunk_frames) *chunk_frames = c->hp.chunk;
    if (n_chunks) *n_chunks = c->hp.nchunks;
    if (fill_ms) *fill_ms = c->hp.fill_ms;
    if (drain_ms) *drain_ms = c->hp.drain_ms;
    if (total_ms) *total_ms = c->hp.total_ms;
    return MGPU_OK;
}

int mgpu_rx_batch(mgpu_ctx* c, const double* bb, int F, uint8_t* payload, mgpu_frame_stats* stats, float* llr_opt) {
    // (an estimator ladder's retry depends on the frame's result: it does not go into the captured graph; nor does the channel-aware
    // demapper's kernel, the residual carrier-offset stage's or the impulse blanker's, so that the graph never has to be captured again)
    if (c && bb && F == 1 && !llr_opt && !c->kt.timing && c->max_batch >= 1 && c->lad.n == 0 && c->dmp.mode == MGPU_DEMAP_MAXLOG && c->cfo.mode == MGPU_CFO_OFF && c->blk.mode == MGPU_BLANK_OFF && !std::getenv("MERCURY_NO_GRAPH"))
        return rx_one_frame(c, bb, payload, stats);
    if (c && bb && F > 1 && F <= c->max_batch && !llr_opt && !c->kt.timing && !std::getenv("MERCURY_NO_PIPELINE"))
        return guard(c, [&] { rx_batch_pipelined(c, bb, F, payload, stats); });
    mgpu_stage_taps taps{};
    taps.llr_ldpc = llr_opt;
    return mgpu_rx_batch_taps(c, bb, F, payload, stats, llr_opt ? &taps : nullptr);
}

int mgpu_ldpc_batch(mgpu_ctx* c, const float* llr, int F, uint8_t* bits, int* iters) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(llr && F >= 0 && F <= c->max_batch, "bad argument (F must be <= max_batch)");
        if (F == 0) return;
        const auto& t = c->tab;
        hipStream_t s = c->stream;
        ensure_workspaces(c, WS_LLR | WS_BITS);
        HIPCK(hipMemcpyAsync(c->d_llr, llr, size_t(F) * t.N * 4, hipMemcpyHostToDevice, s));
        launch_decoder(c, c->d_llr, F, c->d_bits, c->d_iters, nullptr, nullptr, nullptr, nullptr, s);
        if (bits) HIPCK(hipMemcpyAsync(bits, c->d_bits, size_t(F) * t.K, hipMemcpyDeviceToHost, s));
        if (iters) HIPCK(hipMemcpyAsync(iters, c->d_iters, size_t(F) * 4, hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
    });
}

int mgpu_ldpc_encode_batch(mgpu_ctx* c, const uint8_t* bits, int F, uint8_t* encoded) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(bits && encoded && F >= 0, "bad argument");
        if (F == 0) return;
        const auto& t = c->tab;
        DevBuf d_in(size_t(F) * t.K), d_out(size_t(F) * t.N);
        Io io(c);
        io.up(d_in, bits, size_t(F) * t.K);
        for_frame_chunks(F, [&](int off, int n) {
            hipLaunchKernelGGL(mgpu_ldpc_encode_kernel, dim3(n), dim3(256), 0, io.s, c->dev, d_in.as<uint8_t>() + size_t(off) * t.K, n,
                               d_out.as<uint8_t>() + size_t(off) * t.N);
            HIPCK(hipGetLastError());
        });
        io.down(encoded, d_out, size_t(F) * t.N);
    });
}

}  // extern "C"

// Private to the library, host only: what the stream stages (channelizer.hip, synth.hip, resampler.hip, scanner.hip, tuner.hip,
// wideband_blanker.hip, iq_corrector.hip) do the same way: how a handle is made and destroyed, the pair of history buffers a stage carries
// from call to call, the channel plan's retune and phasor table, how a caller's IQ reaches the device, and the whole call of a stage that
// takes blocks of IQ and gives as many back (BlockStage). Not part of the ABI.
#pragma once
#include "chan_tables.hpp"
#include "ctx.hpp"
#include "iq_stream_rule.hpp"

namespace mgpu_detail {

// A stage handle K on context c into *out. bad: why the configuration is refused, or null. A bad configuration is refused before any
// device work, with or without a context (with one, "<who>: <bad>" is its last error); build(K*) then runs with c's device current, and
// the handle exists only if it returns.
template <typename K, typename Build>
int create_stage(mgpu_ctx* c, K** out, const char* who, const char* bad, Build&& build) {
    if (!out) return MGPU_ERR_ARG;
    *out = nullptr;
    if (bad) {
        if (c) c->err = std::string(who) + ": " + bad;
        return MGPU_ERR_ARG;
    }
    if (!c) return MGPU_ERR_DEVICE;               // no context: no device was opened
    return guard(c, [&] {
        std::unique_ptr<K> k(new K);
        k->c = c;
        build(k.get());
        *out = k.release();
    });
}

// The stage's own copy of its configuration: the prototype h, and *kc with its taps pointing into it
template <typename K, typename Config>
void keep_config(K* k, const Config* kc, std::vector<double> h) {
    k->h = std::move(h);
    k->cfg = *kc;
    k->cfg.taps = k->h.data();
    k->cfg.ntaps = int(k->h.size());
}

template <typename K>
int destroy_stage(K* k) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        HIPCK(hipDeviceSynchronize());            // process_dev may have run on a caller's stream
        delete k;
    });
}

// What a stage keeps of its input between calls: two device buffers that change roles. A call reads old() and writes next(), then advance().
template <typename T>
struct History {
    DevArray<T> buf[2];
    int cur = 0;                                  // the buffer the next call writes
    bool fresh = true;                            // no history: the next call reads zeros
    void make(size_t bytes) { for (auto& b : buf) b = DevArray<T>(bytes); }
    const T* old() const { return fresh ? nullptr : static_cast<const T*>(buf[cur ^ 1]); }
    T* next() const { return buf[cur]; }
    void advance() { cur ^= 1; fresh = false; }
    void restart() { fresh = true; }              // after a seek
};

// Channel s of a stage with a channel plan (S, D, cfg.audio_centre_hz, chans, upload_row) becomes *channel
template <typename K>
int retune_channel(K* k, int s, const mgpu_chan_channel* channel) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        need(s >= 0 && s < k->S, "no such channel");
        if (const char* e = mgpu_chan_detail::channel_error(k->D, k->cfg.audio_centre_hz, channel)) throw std::invalid_argument(e);
        HIPCK(hipDeviceSynchronize());            // calls that still read the row, on whatever stream
        k->chans[s] = *channel;
        k->upload_row(s, k->c->stream);
    });
}

// chan_tables.hpp's phasor table W [48000] on the device
inline DevArray<double2> phasor_table_on_device() {
    std::vector<double> W(size_t(MGPU_CHAN_PHASOR_LEN) * 2);
    mgpu_chan_detail::phasor_table(W.data());
    DevArray<double2> d(W.size() * 8);
    HIPCK(hipMemcpy(d.p, W.data(), W.size() * 8, hipMemcpyHostToDevice));
    return d;
}

// A call's IQ format is one of MGPU_IQ_*
inline void need_iq_format(int format) {
    if (const char* e = mgpu_iq_rule::format_error(format)) throw std::invalid_argument(e);
}
// A caller's n_in IQ samples in `format` where the kernels can read them (ctx.hpp staged_on_device)
inline const void* staged_iq(DevArray<char>& stage, const void* iq, int format, int n_in, hipStream_t st) {
    return staged_on_device(stage, iq, size_t(n_in) * mgpu_fmt::iq_bytes(format), st);
}

// What a stage K that takes m blocks of B IQ samples per call and gives m blocks and m reports R back keeps, beside its own: K has a
// configuration cfg (format, block, max_in) and run(d_iq, m, d_out, d_reports, stream), which launches the call and advances pos.
template <typename R>
struct BlockStage {
    mgpu_ctx* c = nullptr;
    int B = 0, max_in = 0, max_blocks = 0;
    size_t bytes = 0;                             // of one IQ sample
    uint64_t pos = 0;
    DevArray<char> d_stage;                       // host input's landing area (ctx.hpp staged_on_device)
    DevArray<char> d_out;                         // process()'s output and reports (grown to the call)
    DevArray<R> d_reports;

    // the call's blocks
    int check_in(const void* iq, int n_in, const void* out) const {
        need(iq != nullptr && out != nullptr, "null pointer");
        need(mgpu_iq_rule::call_ok(B, max_in, pos, n_in), "n_in must be a positive multiple of B, max_in at most, and the position stay below 2^62");
        return n_in / B;
    }
};

// create()'s part: a checked configuration's block B and max_in (0: default_blocks blocks) into the handle and its copy of the configuration
template <typename K>
void block_shape(K* k, int B, int default_blocks) {
    k->B = k->cfg.block = B;
    k->max_in = k->cfg.max_in = k->cfg.max_in ? k->cfg.max_in : default_blocks * B;
    k->max_blocks = k->max_in / B;
    k->bytes = mgpu_fmt::iq_bytes(k->cfg.format);
}

// seek: a position on the block grid becomes the stage's, and reset() forgets what the stage carried
template <typename K, typename Reset>
int block_seek(K* k, uint64_t position, Reset&& reset) {
    if (!k || position > mgpu_iq_rule::kMaxPosition || position % uint64_t(k->B)) return MGPU_ERR_ARG;
    k->pos = position;
    reset();
    return MGPU_OK;
}

// one call on device memory, on `stream` (null: the context's)
template <typename K, typename R>
int block_process_dev(K* k, const void* d_iq, int n_in, void* d_out, R* d_reports, int* n_reports, void* stream) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        const int m = k->check_in(d_iq, n_in, d_out);
        const char* const i0 = static_cast<const char*>(d_iq);
        const char* const o0 = static_cast<const char*>(d_out);
        const size_t len = size_t(n_in) * k->bytes;
        need(o0 + len <= i0 || i0 + len <= o0, "d_out must not overlap d_iq");
        k->run(d_iq, m, d_out, d_reports, stream_or_own(k->c, stream));
        if (n_reports) *n_reports = m;
    });
}

// one call from host (or device) memory into host memory, waited for
template <typename K, typename R>
int block_process(K* k, const void* iq, int n_in, void* out, R* reports, int* n_reports) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        const int m = k->check_in(iq, n_in, out);
        hipStream_t st = k->c->stream;
        const size_t len = size_t(n_in) * k->bytes;
        HIPCK(hipStreamSynchronize(st));          // the buffers below grow only when nothing reads them
        k->d_out.grow(len);
        k->d_reports.grow(size_t(m) * sizeof(R));
        const void* d_iq = staged_on_device(k->d_stage, iq, len, st);
        k->run(d_iq, m, k->d_out.p, k->d_reports, st);
        HIPCK(hipMemcpyAsync(out, k->d_out.p, len, hipMemcpyDeviceToHost, st));
        if (reports) HIPCK(hipMemcpyAsync(reports, k->d_reports.p, size_t(m) * sizeof(R), hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        if (n_reports) *n_reports = m;
    });
}

}  // namespace mgpu_detail

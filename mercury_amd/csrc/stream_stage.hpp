// Private to the library, host only: what the stream stages (channelizer.hip, synth.hip, resampler.hip) do the same way: how a handle is
// made and destroyed, the pair of history buffers a stage carries from call to call, and the channel plan's retune and phasor table.
// Not part of the ABI.
#pragma once
#include "chan_tables.hpp"
#include "ctx.hpp"

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

}  // namespace mgpu_detail

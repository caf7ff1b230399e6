// The reference's receive loop over continuous captures (include/mercury_capture.h): the capture-prep thread (audioio.c:999-1069) and
// RX_SHM_process_main's bookkeeping (telecom_system.cc:2266-2390) for S captures at once, with every capture's window kept on the device.
//
// Ring. Capture s's history - its initial window[0 .. sp-2] followed by every sample fed since - is a sequence h; its window is the last
// sp - 1 entries of h plus window[sp-1], which the loop never overwrites (shift_left moves sp - P samples and the new hop lands at
// sp - P - 1). h[k] lives at ring[s][k mod cap] and all captures advance together, so one counter of hops fed places every ring.
// cap = (buffer_Nsymb + max_hops) * P holds a window plus max_hops hops: run() uploads max_hops hops at once and still reads each hop's
// window. cap and P are even and a window starts at a multiple of P, so the gather moves aligned pairs of doubles and a pair never
// straddles the wrap.
//
// Per hop, the windows of the captures whose frames_to_read is 0 are gathered into one [A][sp] device array and receive_byte reads them
// there (mgpu_receive_byte_batch on device memory, unchanged). The bookkeeping around each call is the host twin's
// (mgpu_host_capture_process), so the CPU pin against the reference's loop covers what runs here.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "../../include/mercury_capture.h"
#include "../../include/mercury_gpu.hpp"

namespace {

constexpr int kDefaultHops = 16;

bool good_geometry(const mgpu_capture_geometry* g) {
    return g && g->symbol_period > 1 && g->nsymb > 0 && g->preamble_nsymb >= 0 && g->buffer_nsymb > 1;
}

// audioio.c:1047-1057 without the samples
void prep_counters(mgpu_capture_state& st) {
    if (st.data_ready == 1) st.n_under++;
    st.frames_to_read--;
    if (st.frames_to_read < 0) st.frames_to_read = 0;
    st.data_ready = 1;
}

// telecom_system.cc:2304-2377 around one receive_byte result (r, link: NULL when the step does not run it)
int process_step(const mgpu_capture_geometry& g, mgpu_capture_state& st, const mgpu_receive_stats* r, const mgpu_link_state* link) {
    if (!st.data_ready) return 0;                                        // :2278-2282
    int ran = 0;
    if (st.frames_to_read == 0) {
        ran = 1;
        // what receive_byte leaves in the receive_stats member
        mgpu::st_receive_stats q;
        const mgpu_capture_held_stats& h = st.held;
        q.iterations_done = h.iterations_done; q.message_decoded = h.message_decoded; q.crc = h.crc; q.all_zeros = h.all_zeros;
        q.delay = h.delay; q.sync_trials = h.sync_trials; q.frame_overflow_symbols = h.frame_overflow_symbols; q.SNR = h.snr_db;
        q.freq_offset = h.freq_offset; q.coarse_metric = h.coarse_metric; q.signal_stregth_dbm = h.signal_strength_dbm;
        mgpu::detail::apply_receive_byte(q, *r, *link, g.mfsk != 0);
        mgpu_capture_held_stats& o = st.held;
        o.iterations_done = q.iterations_done; o.message_decoded = q.message_decoded; o.crc = q.crc; o.all_zeros = q.all_zeros;
        o.delay = q.delay; o.sync_trials = q.sync_trials; o.frame_overflow_symbols = q.frame_overflow_symbols; o.snr_db = q.SNR;
        o.freq_offset = q.freq_offset; o.coarse_metric = q.coarse_metric; o.signal_strength_dbm = q.signal_stregth_dbm;
        st.link = *link;
        const int P = g.symbol_period, frame = g.nsymb + g.preamble_nsymb;
        if (r->message_decoded) {                                        // :2338-2351
            const int end_of_current_message = r->delay / P + frame;
            int frames_left_in_buffer = g.buffer_nsymb - end_of_current_message;
            if (frames_left_in_buffer < 0) frames_left_in_buffer = 0;
            st.frames_to_read = frame - frames_left_in_buffer - st.n_under;
            if (st.frames_to_read > frame || st.frames_to_read < 0) st.frames_to_read = frame - frames_left_in_buffer;
            st.link.delay_of_last_decoded_message += (frame - st.frames_to_read) * P;
            st.n_under = 0;
        } else if (st.link.delay_of_last_decoded_message != -1) {       // :2352-2361
            st.link.delay_of_last_decoded_message -= P;
            if (st.link.delay_of_last_decoded_message < 0) st.link.delay_of_last_decoded_message = -1;
        }
    }
    st.data_ready = 0;                                                   // :2387
    return ran;
}

void init_state(const mgpu_capture_geometry& g, mgpu_capture_state& st) {
    st = mgpu_capture_state{};
    st.frames_to_read = g.preamble_nsymb + g.nsymb;                      // data_container.cc:155-157
    st.link.delay_of_last_decoded_message = -1;                          // telecom_system.cc:38-51
    st.held.iterations_done = -1;
    st.held.snr_db = -99.9;
    st.held.signal_strength_dbm = -999;
}

}  // namespace

// ring[s][(pos0 + i) mod cap] = widen(in[s * in_stride + i]) for i < n (pos0 < cap, n <= cap); grid: x over i, y over captures
template <typename T>
__global__ __launch_bounds__(256) void mgpu_capture_feed_kernel(const T* __restrict__ in, size_t in_stride, int n, double divisor,
                                                                double* __restrict__ ring, size_t cap, size_t pos0) {
    const size_t s = blockIdx.y;
    const T* src = in + s * in_stride;
    double* dst = ring + s * cap;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        size_t p = pos0 + size_t(i);
        if (p >= cap) p -= cap;
        dst[p] = mgpu_fmt::widen(src[i], divisor);
    }
}

// out[a][j] = ring[idx[a]][(start + j) mod cap] for j < sp - 1, out[a][sp - 1] = last[idx[a]]; in pairs of doubles (sp, cap, start even,
// so a pair never straddles the wrap and both sides are 16-byte aligned). grid: x over pairs, y over the gathered windows
__global__ __launch_bounds__(256) void mgpu_capture_gather_kernel(const double* __restrict__ ring, size_t cap, size_t start,
                                                                  const double* __restrict__ last, const int* __restrict__ idx, int sp,
                                                                  double* __restrict__ out) {
    const int s = idx[blockIdx.y];
    const double2* src = reinterpret_cast<const double2*>(ring + size_t(s) * cap);
    double2* dst = reinterpret_cast<double2*>(out + size_t(blockIdx.y) * sp);
    const size_t half = cap / 2, q0 = start / 2;
    const int np = sp / 2;
    for (int m = blockIdx.x * blockDim.x + threadIdx.x; m < np; m += gridDim.x * blockDim.x) {
        size_t q = q0 + size_t(m);
        if (q >= half) q -= half;
        double2 v = src[q];
        if (m == np - 1) v.y = last[s];
        dst[m] = v;
    }
}

struct mgpu_capture {
    mgpu_ctx* c = nullptr;
    int S = 0, sp = 0, P = 0, max_hops = 0;
    size_t cap = 0;                       // ring length per capture, doubles
    long long hops = 0;                   // hops fed so far (the same for every capture)
    mgpu_receive_config rc{};
    mgpu_capture_geometry g{};
    std::vector<mgpu_capture_state> st;
    DevArray<double> ring, last;          // [S][cap], [S]
    DevArray<char> d_in;                  // one upload of compact samples: [S][max_hops * P]
    PinnedBuf h_in;                       // its page-locked staging
    size_t h_in_bytes = 0;
    DevArray<double> d_win;               // gathered windows [A][sp], A <= max_batch
    int win_cap = 0;
    DevArray<int> d_idx;                  // [max_batch] capture index of each gathered window
    PinnedBuf h_idx;
    std::vector<mgpu_link_state> links;
    std::vector<mgpu_receive_stats> rstats;
    std::vector<uint8_t> rpayload;

    size_t window_start() const { return size_t((hops * P) % (long long)cap); }
    size_t write_pos() const { return size_t((sp - 1 + hops * P) % (long long)cap); }
    hipStream_t s() const { return c->stream; }

    // hops [h0, h0 + n) of the call's samples ([S][H * P], host or device) into every ring; the counters are the caller's
    void feed_chunk(const void* samples, int fmt, int H, int h0, int n, bool dev) {
        const size_t sb = mgpu_fmt::element_bytes(mgpu_fmt::element(1, fmt)), row = size_t(n) * P, in_row = size_t(H) * P;
        const char* src = static_cast<const char*>(samples) + size_t(h0) * P * sb;
        size_t stride = in_row;
        if (!dev) {
            const size_t bytes = size_t(S) * row * sb;
            if (h_in_bytes < bytes) {
                h_in = PinnedBuf();
                HIPCK(host_alloc_on_node(&h_in.h, bytes, c->numa_node));
                h_in_bytes = bytes;
            }
            HIPCK(hipStreamSynchronize(s()));          // the previous upload from the staging area has completed
            char* stage = static_cast<char*>(h_in.h);
            if (row == in_row) std::memcpy(stage, src, bytes);
            else for (int k = 0; k < S; ++k) std::memcpy(stage + size_t(k) * row * sb, src + size_t(k) * in_row * sb, row * sb);
            d_in.grow(bytes);
            HIPCK(hipMemcpyAsync(d_in, stage, bytes, hipMemcpyHostToDevice, s()));
            src = d_in;
            stride = row;
        }
        const size_t pos0 = write_pos();
        const unsigned gx = unsigned(std::min<size_t>((row + 255) / 256, 64));
        for (int k0 = 0; k0 < S; k0 += 65535) {
            const int ns = std::min(S - k0, 65535);
            const dim3 grid(gx, unsigned(ns)), block(256);
            double* r = ring + size_t(k0) * cap;
            const char* in = src + size_t(k0) * stride * sb;
            mgpu_fmt::with_elements(mgpu_fmt::element(1, fmt), in, [&](auto* typed, double divisor) {
                using T = std::remove_cv_t<std::remove_pointer_t<decltype(typed)>>;
                hipLaunchKernelGGL(mgpu_capture_feed_kernel<T>, grid, block, 0, s(), typed, stride, int(row), divisor, r, cap, pos0);
            });
            HIPCK(hipGetLastError());
        }
    }

    // the current windows of captures idx[0 .. n) into d_win (n <= win_cap), queued on the context's stream
    void gather(const int* idx, int n) {
        std::memcpy(h_idx.h, idx, size_t(n) * sizeof(int));
        HIPCK(hipMemcpyAsync(d_idx, h_idx.h, size_t(n) * sizeof(int), hipMemcpyHostToDevice, s()));
        const unsigned gx = unsigned(std::min((sp / 2 + 255) / 256, 64));
        hipLaunchKernelGGL(mgpu_capture_gather_kernel, dim3(gx, unsigned(n)), dim3(256), 0, s(), ring, cap, window_start(), last, d_idx, sp, d_win);
        HIPCK(hipGetLastError());
    }

    // one process step for every capture; decoded frames are handed to `decoded(capture, stats, payload)`
    template <typename Fn>
    void process(int* ran, mgpu_receive_stats* stats, uint8_t* payload, Fn&& decoded) {
        const int stride = c->tab.payload_stride;
        std::vector<int> act;
        for (int k = 0; k < S; ++k)
            if (st[k].data_ready && st[k].frames_to_read == 0) act.push_back(k);
        if (ran) std::fill(ran, ran + S, 0);
        for (size_t a0 = 0; a0 < act.size(); a0 += size_t(win_cap)) {
            const int n = int(std::min(act.size() - a0, size_t(win_cap)));
            gather(act.data() + a0, n);
            for (int a = 0; a < n; ++a) {
                const mgpu_capture_state& q = st[act[a0 + a]];
                links[a] = q.link;
                links[a].mfsk_search_start = std::max(0, q.mfsk_search_raw - q.n_under);     // telecom_system.cc:683-685
            }
            if (mgpu_receive_byte_batch(c, d_win, n, &rc, links.data(), rpayload.data(), rstats.data()) != MGPU_OK)
                throw std::runtime_error("receive_byte on the gathered windows: " + c->err);
            for (int a = 0; a < n; ++a) {
                const int k = act[a0 + a];
                process_step(g, st[k], &rstats[a], &links[a]);
                if (ran) ran[k] = 1;
                if (stats) stats[k] = rstats[a];
                if (payload) std::memcpy(payload + size_t(k) * stride, &rpayload[size_t(a) * stride], size_t(stride));
                if (rstats[a].message_decoded) decoded(k, rstats[a], &rpayload[size_t(a) * stride]);
            }
        }
        for (int k = 0; k < S; ++k)
            if (st[k].data_ready) process_step(g, st[k], nullptr, nullptr);    // frames_to_read > 0: nothing but data_ready = 0
    }

    void feed(const void* samples, int fmt, int H, int h0, int n, bool dev) {
        feed_chunk(samples, fmt, H, h0, n, dev);
        for (int h = 0; h < n; ++h)
            for (auto& q : st) prep_counters(q);
        hops += n;
    }
};

int capture_streams(mgpu_capture* cap) { return cap->S; }
bool capture_pairs(mgpu_capture* cap, mgpu_ctx* c, int S, mgpu_capture_geometry* g) {
    return mgpu_capture_geometry_get(cap, g) == MGPU_OK && cap->S == S && cap->c == c;
}

namespace {
void check_feed_args(mgpu_capture* k, const void* samples, int fmt, int H) {
    need(samples != nullptr && H > 0, "bad argument (samples must be non-null, H >= 1)");
    need(mgpu_fmt::element(1, fmt) != mgpu_fmt::kNone, "unknown sample format");
    need(size_t(H) * k->P < (size_t(1) << 31) / 2, "H too large");
}
}  // namespace

extern "C" {

int mgpu_capture_create(mgpu_ctx* c, int S, const mgpu_receive_config* rcp, const double* initial_windows, int max_hops, mgpu_capture** out) {
    if (!c || !out) return MGPU_ERR_ARG;
    *out = nullptr;
    return guard(c, [&] {
        need(S > 0 && rcp && max_hops >= 0 && max_hops <= 4096, "bad argument (S >= 1, config non-null, max_hops 0..4096)");
        need(rcp->time_sync_trials_max >= 1 && rcp->time_sync_trials_max < 64, "time_sync_trials_max must be 1..63");
        std::unique_ptr<mgpu_capture> k(new mgpu_capture);
        const auto& t = c->tab;
        k->c = c;
        k->S = S;
        k->P = t.Nofdm * kInterp;
        k->g = {mgpu_receive_buffer_nsymb(c), t.Nsymb, t.preamble, k->P, t.mfsk_M > 0 ? 1 : 0};   // data_container.Nsymb, not the active one
        k->sp = k->g.buffer_nsymb * k->P;
        k->max_hops = max_hops ? max_hops : kDefaultHops;
        k->cap = size_t(k->g.buffer_nsymb + k->max_hops) * k->P;
        k->rc = *rcp;
        k->st.resize(S);
        for (auto& q : k->st) init_state(k->g, q);
        k->win_cap = std::min(S, c->max_batch);
        k->links.resize(k->win_cap);
        k->rstats.resize(k->win_cap);
        k->rpayload.resize(size_t(k->win_cap) * t.payload_stride);
        k->ring = DevArray<double>(size_t(S) * k->cap * 8);
        k->last = DevArray<double>(size_t(S) * 8);
        k->d_win = DevArray<double>(size_t(k->win_cap) * k->sp * 8);
        k->d_idx = DevArray<int>(size_t(k->win_cap) * 4);
        HIPCK(host_alloc_on_node(&k->h_idx.h, size_t(k->win_cap) * 4, c->numa_node));
        if (initial_windows) {
            HIPCK(hipMemcpy2D(k->ring, k->cap * 8, initial_windows, size_t(k->sp) * 8, size_t(k->sp - 1) * 8, size_t(S), hipMemcpyHostToDevice));
            std::vector<double> last(S);
            for (int s = 0; s < S; ++s) last[s] = initial_windows[size_t(s) * k->sp + k->sp - 1];
            HIPCK(hipMemcpy(k->last, last.data(), size_t(S) * 8, hipMemcpyHostToDevice));
        } else {
            HIPCK(hipMemset(k->ring, 0, size_t(S) * k->cap * 8));
            HIPCK(hipMemset(k->last, 0, size_t(S) * 8));
        }
        HIPCK(hipDeviceSynchronize());
        *out = k.release();
    });
}

int mgpu_capture_destroy(mgpu_capture* k) {
    if (!k) return MGPU_ERR_ARG;
    mgpu_ctx* c = k->c;
    return guard(c, [&] {
        HIPCK(hipStreamSynchronize(c->stream));
        delete k;
    });
}

int mgpu_capture_geometry_get(mgpu_capture* k, mgpu_capture_geometry* g) {
    if (!k || !g) return MGPU_ERR_ARG;
    *g = k->g;
    return MGPU_OK;
}

int mgpu_capture_feed(mgpu_capture* k, const void* samples, int fmt, int H) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        check_feed_args(k, samples, fmt, H);
        const bool dev = is_device_memory(samples);
        // only the last sp - 1 samples matter to the window: chunks of max_hops hops, each one upload and one launch
        for (int h0 = 0; h0 < H; h0 += k->max_hops) k->feed(samples, fmt, H, h0, std::min(k->max_hops, H - h0), dev);
        HIPCK(hipStreamSynchronize(k->c->stream));
    });
}

int mgpu_capture_process(mgpu_capture* k, int* ran, mgpu_receive_stats* stats, uint8_t* payload) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        k->process(ran, stats, payload, [](int, const mgpu_receive_stats&, const uint8_t*) {});
        HIPCK(hipStreamSynchronize(k->c->stream));
    });
}

int mgpu_capture_run(mgpu_capture* k, const void* samples, int fmt, int H, mgpu_capture_event* events, uint8_t* payloads, int max_events,
                     int* n_events) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        check_feed_args(k, samples, fmt, H);
        check_event_args(events, max_events, n_events);
        const bool dev = is_device_memory(samples);
        const int stride = k->c->tab.payload_stride;
        int n = 0;
        for (int h0 = 0; h0 < H; h0 += k->max_hops) {
            const int nh = std::min(k->max_hops, H - h0);
            k->feed_chunk(samples, fmt, H, h0, nh, dev);          // one upload, one launch: hop h's window is read before hop h + max_hops lands
            for (int h = 0; h < nh; ++h) {
                for (auto& q : k->st) prep_counters(q);
                k->hops++;
                k->process(nullptr, nullptr, nullptr, [&](int s, const mgpu_receive_stats& r, const uint8_t* pl) {
                    if (n < max_events) {
                        events[n].capture = s;
                        events[n].hop = h0 + h;
                        events[n].stats = r;
                        if (payloads) std::memcpy(payloads + size_t(n) * stride, pl, size_t(stride));
                    }
                    ++n;
                });
            }
        }
        HIPCK(hipStreamSynchronize(k->c->stream));
        *n_events = n;
    });
}

int mgpu_capture_get_state(mgpu_capture* k, int s, mgpu_capture_state* st) {
    if (!k || !st || s < 0 || s >= k->S) return MGPU_ERR_ARG;
    *st = k->st[s];
    return MGPU_OK;
}

int mgpu_capture_set_state(mgpu_capture* k, int s, const mgpu_capture_state* st) {
    if (!k || !st || s < 0 || s >= k->S) return MGPU_ERR_ARG;
    if (st->n_under < 0 || (st->data_ready != 0 && st->data_ready != 1)) return refuse(k->c, MGPU_ERR_ARG, "mgpu_capture_set_state: n_under must be >= 0, data_ready 0 or 1");
    if (!k->g.mfsk && st->link.fixed_delay_plus_one > 0) return refuse(k->c, MGPU_ERR_ARG, "mgpu_capture_set_state: fixed_delay_plus_one: MFSK modes only");
    k->st[s] = *st;
    return MGPU_OK;
}

int mgpu_capture_window(mgpu_capture* k, int s, double* window) {
    if (!k || !window || s < 0 || s >= k->S) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        k->gather(&s, 1);
        HIPCK(hipMemcpyAsync(window, k->d_win, size_t(k->sp) * 8, hipMemcpyDeviceToHost, k->c->stream));
        HIPCK(hipStreamSynchronize(k->c->stream));
    });
}

int mgpu_host_capture_init_state(const mgpu_capture_geometry* g, mgpu_capture_state* st) {
    if (!good_geometry(g) || !st) return MGPU_ERR_ARG;
    init_state(*g, *st);
    return MGPU_OK;
}

int mgpu_host_capture_prep(const mgpu_capture_geometry* g, double* window, const void* samples, int fmt, mgpu_capture_state* st) {
    const int e = mgpu_fmt::element(1, fmt);
    if (!good_geometry(g) || !window || !samples || !st || e == mgpu_fmt::kNone) return MGPU_ERR_ARG;
    const int P = g->symbol_period, sp = g->buffer_nsymb * P, loc = sp - P - 1;   // audioio.c:1035
    if (st->data_ready == 1) st->n_under++;                                      // :1047-1048
    for (int j = 0; j < sp - P; ++j) window[j] = window[j + P];                   // shift_left, misc.cc:26-32
    for (int i = 0; i < P; ++i) window[loc + i] = mgpu_fmt::widen_at(e, samples, size_t(i)); // :1051
    st->frames_to_read--;                                                        // :1053-1055
    if (st->frames_to_read < 0) st->frames_to_read = 0;
    st->data_ready = 1;
    return MGPU_OK;
}

int mgpu_host_capture_process(const mgpu_capture_geometry* g, mgpu_capture_state* st, const mgpu_receive_stats* r, const mgpu_link_state* link) {
    if (!good_geometry(g) || !st) return -MGPU_ERR_ARG;
    if (st->data_ready && st->frames_to_read == 0 && (!r || !link)) return -MGPU_ERR_ARG;
    return process_step(*g, *st, r, link);
}

}  // extern "C"

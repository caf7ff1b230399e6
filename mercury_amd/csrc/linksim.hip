// Link simulator (include/mercury_linksim.h): S transmitter -> streaming HF channel -> noise -> capture-receive links on one context.
//
// A run is cut into rounds of at most `round_hops` hops (max_hops, and never more than a slot, so that a round overlaps at most two frames
// of a link). Per round, all on the context's stream:
//   1. the host draws the payloads of the frames that start inside the round, uploads them, mgpu_transmit_byte_batch_dev makes their audio
//      and mgpu_linksim_place_kernel files each frame into its link's two-frame store (frame j lives in slot j & 1);
//   2. mgpu_linksim_assemble_kernel writes the round's transmit stream [S][n]: per sample the frame it falls into, or silence;
//   3. the streaming channel (mgpu_hf_stream_apply_dev) turns it into the received stream [S][n];
//   4. mgpu_capture_run on that device array runs the receive loop; its events feed the host's bookkeeping.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <set>
#include <vector>

#include "ctx.hpp"
#include "philox.h"
#include "../../include/mercury_linksim.h"

#define LS_SCHEDULE_STREAM 6u
#define LS_PAYLOAD_STREAM 7u

namespace {

constexpr int kDefaultHops = 16;

const char* config_error(const mgpu_linksim_config* k) {
    if (!k) return "no configuration";
    if (k->struct_size != int(sizeof(mgpu_linksim_config))) return "mgpu_linksim_config.struct_size is not sizeof(mgpu_linksim_config)";
    if (k->S < 1) return "S must be >= 1";
    if (k->gap_hops < 0 || k->gap_hops > (1 << 20)) return "gap_hops must be 0..2^20";
    if (k->tx.message_location != MGPU_SINGLE_MESSAGE) return "the link simulator transmits MGPU_SINGLE_MESSAGE frames only";
    return nullptr;
}

long long link_offset(uint64_t seed, int link, long long slot) {
    uint32_t r[4];
    philox4x32(seed, uint32_t(link), LS_SCHEDULE_STREAM, 0u, 0u, r);
    return (long long)(((uint64_t(r[0]) << 32) | r[1]) % uint64_t(slot));
}

// 16 bytes per draw: counter (link, stream 7, frame bits 0..31, frame bits 32..47 | block)
void payload_bytes(uint64_t seed, int link, long long frame, int nbytes, uint8_t* out) {
    for (int b = 0; b * 16 < nbytes; ++b) {
        uint32_t r[4];
        philox4x32(seed, uint32_t(link), LS_PAYLOAD_STREAM, uint32_t(uint64_t(frame)), (uint32_t(uint64_t(frame) >> 32) << 16) | uint32_t(b), r);
        for (int i = 0; i < 16 && b * 16 + i < nbytes; ++i) out[b * 16 + i] = uint8_t(r[i >> 2] >> (8 * (i & 3)));
    }
}

}  // namespace

// store[dst[f]][0 .. fsz) = audio[f][0 .. fsz): grid x over samples, y over the frames made this round
extern "C" __global__ __launch_bounds__(256) void mgpu_linksim_place_kernel(const double* __restrict__ audio, const int* __restrict__ dst, int fsz,
                                                                            double* __restrict__ store) {
    const double* a = audio + size_t(blockIdx.y) * fsz;
    double* o = store + size_t(dst[blockIdx.y]) * fsz;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < fsz; i += gridDim.x * blockDim.x) o[i] = a[i];
}

// out[s][i] = the transmit stream of link s at position pos + i, i < n <= slot: frame j = floor((pos + i - off[s]) / slot) from the link's
// store slot j & 1 where the sample lies inside the frame, zero in the gap behind it and before frame 0. A round is no longer than a slot, so
// one division per thread places its first sample and the rest wrap at most once. grid: x over samples, y over links
extern "C" __global__ __launch_bounds__(256) void mgpu_linksim_assemble_kernel(const double* __restrict__ store, const long long* __restrict__ off,
                                                                               long long pos, int n, int fsz, long long slot, int s0,
                                                                               double* __restrict__ out) {
    const int s = s0 + int(blockIdx.y);
    const long long u0 = pos - off[s];                            // > -slot
    const long long j0 = u0 >= 0 ? u0 / slot : -1;
    const long long w0 = u0 - j0 * slot;                          // in [0, slot)
    const double* f = store + size_t(s) * 2 * fsz;
    double* o = out + size_t(s) * n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        long long w = w0 + i, j = j0;
        if (w >= slot) { w -= slot; ++j; }
        o[i] = (j >= 0 && w < fsz) ? f[size_t(j & 1) * fsz + size_t(w)] : 0.0;
    }
}

struct mgpu_linksim {
    mgpu_ctx* c = nullptr;
    mgpu_linksim_config cfg{};
    int S = 0, P = 0, fsz = 0, round_hops = 0, nbytes = 0, stride = 0, L = 0, window = 0;
    long long slot = 0, hops = 0;                 // hops run so far: the next transmit position is hops * P
    bool noisy = false;
    std::vector<long long> off, next_frame;       // [S] offset_s; the next frame of the link that has no audio yet
    std::vector<double> noise_amp;                // [S]
    std::vector<mgpu_linksim_counters> cnt;       // [S]
    std::vector<std::set<long long>> delivered;   // [S] delivered frames that are still matchable
    mgpu_hf_stream* chan = nullptr;
    mgpu_capture* cap = nullptr;
    DevArray<double> d_store, d_audio, d_tx, d_rx;   // [S][2][fsz], [2 S][fsz] (grown), [S][round], [S][round]
    DevArray<long long> d_off;
    DevArray<uint8_t> d_payload;                  // [2 S][stride]
    DevArray<int> d_dst;                          // [2 S]
    PinnedBuf h_payload, h_dst;
    std::vector<mgpu_capture_event> ev;
    std::vector<uint8_t> evpl;

    ~mgpu_linksim() {
        if (cap) mgpu_capture_destroy(cap);
        if (chan) mgpu_hf_stream_destroy(chan);
    }
    hipStream_t s() const { return c->stream; }
    void ck(int rc, const char* what) {
        if (rc == MGPU_ERR_ARG) throw std::invalid_argument(std::string(what) + ": " + c->err);
        if (rc != MGPU_OK) throw std::runtime_error(std::string(what) + ": " + c->err);
    }

    // the audio of the frames that begin before transmit position `end` and have none yet, into the store
    void make_frames(long long end) {
        uint8_t* hp = static_cast<uint8_t*>(h_payload.h);
        int* hd = static_cast<int*>(h_dst.h);
        int F = 0;
        for (int k = 0; k < S; ++k)
            while (off[k] + next_frame[k] * slot < end) {            // at most two per link and round (a round is no longer than a slot)
                if (F == 2 * S) throw std::runtime_error("link simulator: more than two new frames per link in one round");
                std::memset(hp + size_t(F) * stride, 0, size_t(stride));
                payload_bytes(cfg.seed, k, next_frame[k], nbytes, hp + size_t(F) * stride);
                hd[F++] = 2 * k + int(next_frame[k] & 1);
                ++next_frame[k];
            }
        if (!F) return;
        HIPCK(hipMemcpyAsync(d_payload, hp, size_t(F) * stride, hipMemcpyHostToDevice, s()));
        HIPCK(hipMemcpyAsync(d_dst, hd, size_t(F) * sizeof(int), hipMemcpyHostToDevice, s()));
        ck(mgpu_transmit_byte_batch_dev(c, d_payload, stride, nullptr, F, &cfg.tx, d_audio, s()), "transmit_byte");
        hipLaunchKernelGGL(mgpu_linksim_place_kernel, dim3(unsigned(std::min((fsz + 255) / 256, 64)), unsigned(F)), dim3(256), 0, s(), d_audio, d_dst, fsz,
                           d_store);
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(s()));                             // the staging area is rewritten by the next round
    }

    void book(const mgpu_capture_event& e, const uint8_t* pl) {
        const int k = e.capture;
        const long long got = (e.hop + 1LL) * P - 1;                 // last sample the capture has received
        // matchable frames: e_j = off + j slot + fsz - 1 + L with e_j <= got < e_j + window
        const long long base = off[k] + fsz - 1 + L;
        long long jhi = got >= base ? (got - base) / slot : -1;
        long long jlo = got - window - base >= 0 ? (got - window - base) / slot + 1 : 0;     // first j with e_j > got - window
        auto& dl = delivered[k];
        while (!dl.empty() && *dl.begin() < jlo) dl.erase(dl.begin());
        std::vector<uint8_t> sent(static_cast<size_t>(nbytes));
        bool dup = false;
        for (long long j = jlo; j <= jhi; ++j) {
            payload_bytes(cfg.seed, k, j, nbytes, sent.data());
            if (std::memcmp(sent.data(), pl, size_t(nbytes)) != 0) continue;
            if (dl.count(j)) { dup = true; continue; }
            dl.insert(j);
            cnt[k].delivered++;
            cnt[k].iterations_sum += e.stats.iterations_done;
            cnt[k].snr_db_sum += e.stats.snr_db;
            return;
        }
        if (dup) cnt[k].duplicates++;
        else if (e.stats.crc) cnt[k].false_decodes++;
    }

    void round(int nh, mgpu_capture_event* events, uint8_t* payloads, int max_events, int& n_total, double* samples_out, int H, int h0) {
        const long long pos = hops * P;
        const int n = nh * P;
        make_frames(pos + n);
        const unsigned gx = unsigned(std::min((n + 255) / 256, 64));
        for (int k0 = 0; k0 < S; k0 += 65535) {
            hipLaunchKernelGGL(mgpu_linksim_assemble_kernel, dim3(gx, unsigned(std::min(S - k0, 65535))), dim3(256), 0, s(), d_store, d_off, pos, n, fsz,
                               slot, k0, d_tx);
            HIPCK(hipGetLastError());
        }
        ck(mgpu_hf_stream_apply_dev(chan, d_tx, n, noisy ? noise_amp.data() : nullptr, d_rx, s()), "streaming channel");
        if (samples_out)
            HIPCK(hipMemcpy2DAsync(samples_out + size_t(h0) * P, size_t(H) * P * 8, d_rx, size_t(n) * 8, size_t(n) * 8, size_t(S), hipMemcpyDeviceToHost, s()));
        int ne = 0;
        ck(mgpu_capture_run(cap, d_rx, MGPU_SAMPLES_F64, nh, ev.data(), evpl.data(), int(ev.size()), &ne), "capture run");
        for (int i = 0; i < ne; ++i) {
            mgpu_capture_event e = ev[i];
            e.hop += int(hops);
            const uint8_t* pl = &evpl[size_t(i) * stride];
            book(e, pl);
            if (n_total < max_events) {
                events[n_total] = e;
                if (payloads) std::memcpy(payloads + size_t(n_total) * stride, pl, size_t(stride));
            }
            ++n_total;
        }
        hops += nh;
        const long long fed = hops * P;
        for (int k = 0; k < S; ++k) {
            cnt[k].hops = hops;
            cnt[k].frames_sent = fed - off[k] - fsz >= 0 ? (fed - off[k] - fsz) / slot + 1 : 0;
        }
    }
};

extern "C" {

int mgpu_host_linksim_frame_start(const mgpu_linksim_config* k, int frame_samples, int symbol_period, int link, long long frame,
                                  long long* start_sample) {
    if (config_error(k) || !start_sample || frame_samples < 1 || symbol_period < 1 || link < 0 || link >= k->S || frame < 0 ||
        frame >= (1LL << 40))
        return MGPU_ERR_ARG;
    const long long slot = (long long)frame_samples + (long long)k->gap_hops * symbol_period;
    *start_sample = link_offset(k->seed, link, slot) + frame * slot;
    return MGPU_OK;
}

int mgpu_host_linksim_payload(uint64_t seed, int link, long long frame, int nbytes, uint8_t* out) {
    if (!out || link < 0 || frame < 0 || frame >= (1LL << 48) || nbytes < 0 || nbytes > 16 * 65536) return MGPU_ERR_ARG;
    payload_bytes(seed, link, frame, nbytes, out);
    return MGPU_OK;
}

int mgpu_linksim_create(mgpu_ctx* c, const mgpu_linksim_config* kc, const double* esn0_db, mgpu_linksim** out) {
    if (!c || !out) return MGPU_ERR_ARG;
    *out = nullptr;
    return guard(c, [&] {
        if (const char* e = config_error(kc)) throw std::invalid_argument(e);
        need(kc->max_hops >= 0 && kc->max_hops <= 4096, "max_hops must be 0..4096");
        need(kc->S <= 32767, "at most 32767 links per simulator");
        hf_check(&kc->channel);
        const auto& t = c->tab;
        std::unique_ptr<mgpu_linksim> k(new mgpu_linksim);
        k->c = c;
        k->cfg = *kc;
        const int S = k->S = kc->S;
        k->P = t.Nofdm * kInterp;
        k->fsz = mgpu_transmit_frame_samples(c);
        k->slot = (long long)k->fsz + (long long)kc->gap_hops * k->P;
        const int max_hops = kc->max_hops ? kc->max_hops : kDefaultHops;
        k->round_hops = int(std::min<long long>(max_hops, k->slot / k->P));
        k->nbytes = t.payload_bytes;
        k->stride = t.payload_stride;
        k->window = mgpu_receive_buffer_nsymb(c) * k->P;
        need(k->P % 64 == 0, "the symbol period must be a multiple of 64 samples");
        k->off.resize(S);
        for (int s = 0; s < S; ++s) k->off[s] = link_offset(kc->seed, s, k->slot);
        k->next_frame.assign(S, 0);
        k->cnt.assign(S, mgpu_linksim_counters{});
        k->delivered.resize(S);
        k->ck(mgpu_hf_stream_create(c, &kc->channel, kSampleRate, S, kc->seed, 0, &k->chan), "streaming channel");
        k->L = mgpu_hf_stream_latency(k->chan);
        k->ck(mgpu_capture_create(c, S, &kc->rx, nullptr, max_hops, &k->cap), "capture");
        const size_t n = size_t(k->round_hops) * k->P;
        k->d_store = DevArray<double>(size_t(S) * 2 * k->fsz * 8);
        k->d_audio = DevArray<double>(size_t(S) * 2 * k->fsz * 8);
        k->d_tx = DevArray<double>(size_t(S) * n * 8);
        k->d_rx = DevArray<double>(size_t(S) * n * 8);
        k->d_off = DevArray<long long>(size_t(S) * 8);
        k->d_payload = DevArray<uint8_t>(size_t(S) * 2 * k->stride);
        k->d_dst = DevArray<int>(size_t(S) * 2 * 4);
        HIPCK(host_alloc_on_node(&k->h_payload.h, size_t(S) * 2 * k->stride, c->numa_node));
        HIPCK(host_alloc_on_node(&k->h_dst.h, size_t(S) * 2 * 4, c->numa_node));
        HIPCK(hipMemset(k->d_store, 0, size_t(S) * 2 * k->fsz * 8));
        HIPCK(hipMemcpy(k->d_off, k->off.data(), size_t(S) * 8, hipMemcpyHostToDevice));
        k->ev.resize(size_t(S) * k->round_hops);
        k->evpl.resize(k->ev.size() * k->stride);
        k->noisy = esn0_db != nullptr;
        if (k->noisy) {
            // the noise of mgpu_passband_test_esn0 (selfsim.hip); MFSK calibrates it from the power of the first frame link 0 sends
            double psig = 0;
            if (t.mfsk_M > 0) {
                uint8_t* hp = static_cast<uint8_t*>(k->h_payload.h);
                std::memset(hp, 0, size_t(k->stride));
                payload_bytes(kc->seed, 0, 0, k->nbytes, hp);
                HIPCK(hipMemcpy(k->d_payload, hp, size_t(k->stride), hipMemcpyHostToDevice));
                k->ck(mgpu_transmit_byte_batch_dev(c, k->d_payload, k->stride, nullptr, 1, &k->cfg.tx, k->d_audio, c->stream), "transmit_byte");
                std::vector<double> a0(static_cast<size_t>(k->fsz));
                HIPCK(hipMemcpyAsync(a0.data(), k->d_audio, size_t(k->fsz) * 8, hipMemcpyDeviceToHost, c->stream));
                HIPCK(hipStreamSynchronize(c->stream));
                for (double v : a0) psig += v * v;
                psig /= k->fsz;
            }
            k->noise_amp.resize(S);
            for (int s = 0; s < S; ++s) {
                need(std::isfinite(esn0_db[s]), "esn0_db must be finite");
                k->noise_amp[s] = audio_noise_amplitude(t, esn0_db[s], psig);
            }
        }
        HIPCK(hipDeviceSynchronize());
        *out = k.release();
    });
}

int mgpu_linksim_destroy(mgpu_linksim* k) {
    if (!k) return MGPU_ERR_ARG;
    mgpu_ctx* c = k->c;
    return guard(c, [&] {
        HIPCK(hipStreamSynchronize(c->stream));
        delete k;
    });
}

int mgpu_linksim_run(mgpu_linksim* k, int H, mgpu_capture_event* events, uint8_t* payloads, int max_events, int* n_events, double* samples_out) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        need(H > 0 && n_events != nullptr && max_events >= 0 && (max_events == 0 || events), "bad argument (H >= 1, n_events, events)");
        need(k->hops + H < (1LL << 31), "the simulator's hop counter is an int in mgpu_capture_event");
        int n = 0;
        for (int h0 = 0; h0 < H; h0 += k->round_hops)
            k->round(std::min(k->round_hops, H - h0), events, payloads, max_events, n, samples_out, H, h0);
        HIPCK(hipStreamSynchronize(k->c->stream));
        *n_events = n;
    });
}

int mgpu_linksim_counters_get(mgpu_linksim* k, mgpu_linksim_counters* out) {
    if (!k || !out) return MGPU_ERR_ARG;
    std::copy(k->cnt.begin(), k->cnt.end(), out);
    return MGPU_OK;
}

int mgpu_linksim_capture(mgpu_linksim* k, mgpu_capture** cap) {
    if (!k || !cap) return MGPU_ERR_ARG;
    *cap = k->cap;
    return MGPU_OK;
}

int mgpu_linksim_noise_amp(mgpu_linksim* k, double* out) {
    if (!k || !out) return MGPU_ERR_ARG;
    for (int s = 0; s < k->S; ++s) out[s] = k->noisy ? k->noise_amp[s] : 0.0;
    return MGPU_OK;
}

}  // extern "C"

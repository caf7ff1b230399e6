// Wideband synthesiser (include/ext/mercury_synth.h): S real 48 kHz audio streams [S][n_in] into one IQ stream of n_in * D samples.
//
// One kernel per call, mgpu_synth_kernel. Nothing is kept between calls but the position and the last tp audio samples of every channel
// (two history buffers that change roles, as the resampler's), so how the stream is cut cannot change an output.
//
// 4 (tp + 1) S flops per IQ sample and few bytes: bound by fp64 FMA issue. A workgroup is four wavefronts on ONE tile of kTile = 64
// consecutive audio positions and one group of PH consecutive phases r0 .. r0 + PH - 1 (grid: x the tiles, y the phase groups; a lane's
// 2 PH accumulators are why D = 64 does not go to one lane: 16 groups of 4). Lane l owns position n0 + l. At step j it reads a_s[n - j]
// from LDS once (consecutive lanes, consecutive doubles: no bank conflict) and uses it for 2 PH fused multiply-adds, one per component and
// phase, every accumulator seeing its taps in ascending j: the rule's order. The taps of a sideband are the same for every channel and
// every lane: the table is laid out [sideband][group][j][PH], 16 PH contiguous bytes per step, read by scalar loads into SGPR operands.
// Step j = tp exists for r = 0 alone (T - 1 = tp D): one more fused multiply-add pair in group 0, not a zero tap, which would turn an
// infinite sample into a NaN where the rule has none.
//
// Channels: wavefront w takes the channels s = 4 i + w, i = 0, 1, ..: each has its own accumulators and its own z = G v E, which goes to
// LDS; wavefront p < PH keeps the running IQ totals of phase r0 + p in registers and adds the round's z in ascending s. Four channels
// are worked on at once and no sum is reordered. After the last round the totals go through LDS once more so that thread t stores
// position t / PH, phase t % PH: runs of PH consecutive IQ samples per position.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "stream_stage.hpp"
#include "synth_tables.hpp"

using namespace mgpu_synth_detail;
using mgpu_chan_detail::floor_mod;

namespace {

constexpr int kWaves = 4;                    // channels in flight per workgroup
constexpr int kThreads = 64 * kWaves;
constexpr int kTile = 64;                    // audio positions per workgroup: one per lane
constexpr int kMaxPhases = 4;                // phases per lane

struct SynthRow { int offm; int sideband; double gain; };      // offset_hz mod 48000, 0 USB / 1 LSB, G

struct SynthArgs {
    const double* in;         // [S][in_stride]
    size_t in_stride;
    const double* hist_old;   // [S][tp]: the samples n0 - tp .. n0 - 1; null: zeros
    double* hist_new;         // [S][tp]
    void* out;                // n_in * D IQ samples in `format`
    unsigned long long* clamped;
    int format, S, D, tp, n_in, groups;
    unsigned nm;              // n0 mod 48000
};

inline int phases_per_lane(int D) { return D <= 2 ? D : kMaxPhases; }

}  // namespace

// sample idx of channel s counted from the call's first one: the caller's, the history below 0 (idx >= -tp), zeros behind the chunk
__device__ inline double synth_x(const SynthArgs& a, int s, int idx) {
    if (idx < 0) return a.hist_old ? a.hist_old[size_t(s) * a.tp + size_t(a.tp + idx)] : 0.0;
    return idx < a.n_in ? a.in[size_t(s) * a.in_stride + size_t(idx)] : 0.0;
}

template <int PH>
__device__ inline void synth_tile(const SynthArgs& a, const double2* __restrict__ q, const double2* __restrict__ P,
                                  const double2* __restrict__ W, const SynthRow* __restrict__ rows) {
    __shared__ double au[kWaves][kTile + MGPU_CHAN_MAX_TP];          // au[w][i] = a_s[n0 - tp + i] of wavefront w's channel
    __shared__ double2 zx[kWaves * PH * kTile];                      // z of the round [w][p][lane]; at the end the totals [lane][p]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
    const int tp = a.tp, n0 = int(blockIdx.x) * kTile, g = int(blockIdx.y), r0 = g * PH;
    const bool keeps_history = blockIdx.x == 0 && blockIdx.y == 0;
    const unsigned nmod = (a.nm + unsigned(n0 + lane)) % unsigned(MGPU_CHAN_PHASOR_LEN);
    double tr = 0.0, ti = 0.0;                                       // wavefront p < PH: the totals of phase r0 + p

    for (int s0 = 0; s0 < a.S; s0 += kWaves) {
        const int s = s0 + wave;
        const bool live = s < a.S;
        double2 z[PH];
        if (live) {
            for (int i = lane; i < kTile + tp; i += 64) au[wave][i] = synth_x(a, s, n0 - tp + i);
            if (keeps_history)                                       // the next call's history: the last tp samples of (history, chunk)
                for (int e = lane; e < tp; e += 64) a.hist_new[size_t(s) * tp + e] = synth_x(a, s, a.n_in - tp + e);
        }
        __syncthreads();
        if (live) {
            const SynthRow row = rows[s];
            const double2* __restrict__ qs = q + (size_t(row.sideband) * a.groups + g) * size_t(tp + 1) * PH;
            const double* x = au[wave] + lane + tp;                  // x[-j] = a_s[n - j]
            double vr[PH], vi[PH];
#pragma unroll
            for (int p = 0; p < PH; ++p) vr[p] = vi[p] = 0.0;
            int j = 0;
            // four steps at a time: their LDS reads and 4 PH taps (64 PH contiguous bytes) are in flight together
            for (; j + 4 <= tp; j += 4) {
                double v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = x[-(j + u)];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int p = 0; p < PH; ++p) {
                        const double2 t = qs[(j + u) * PH + p];
                        vr[p] = fma(t.x, v[u], vr[p]);
                        vi[p] = fma(t.y, v[u], vi[p]);
                    }
            }
            for (; j < tp; ++j) {
                const double v = x[-j];
#pragma unroll
                for (int p = 0; p < PH; ++p) {
                    const double2 t = qs[j * PH + p];
                    vr[p] = fma(t.x, v, vr[p]);
                    vi[p] = fma(t.y, v, vi[p]);
                }
            }
            if (r0 == 0) {                                           // j = tp: phase 0 alone
                const double2 t = qs[tp * PH];
                const double v = x[-tp];
                vr[0] = fma(t.x, v, vr[0]);
                vi[0] = fma(t.y, v, vi[0]);
            }
            const double2 e = W[(unsigned(row.offm) * nmod) % unsigned(MGPU_CHAN_PHASOR_LEN)];
#pragma unroll
            for (int p = 0; p < PH; ++p) {
                const double2 ph = P[size_t(s) * (a.groups * PH) + r0 + p];
                const double er = fma(-e.y, ph.y, e.x * ph.x), ei = fma(e.y, ph.x, e.x * ph.y);
                z[p] = make_double2(row.gain * fma(-vi[p], ei, vr[p] * er), row.gain * fma(vi[p], er, vr[p] * ei));
            }
        }
        __syncthreads();                                             // the totals' reads of the round before are over
        if (live) {
#pragma unroll
            for (int p = 0; p < PH; ++p) zx[(wave * PH + p) * kTile + lane] = z[p];
        }
        __syncthreads();
        if (wave < PH) {
            const int nw = min(kWaves, a.S - s0);
            for (int w = 0; w < nw; ++w) {                           // ascending s
                const double2 t = zx[(w * PH + wave) * kTile + lane];
                tr += t.x;
                ti += t.y;
            }
        }
    }
    __syncthreads();
    if (wave < PH) zx[lane * PH + wave] = make_double2(tr, ti);
    __syncthreads();
    if (threadIdx.x < kTile * PH) {
        const int n = n0 + int(threadIdx.x) / PH, r = r0 + int(threadIdx.x) % PH;
        if (n < a.n_in && r < a.D) {
            const double2 t = zx[threadIdx.x];
            const unsigned c = mgpu_fmt::store_iq(a.out, a.format, size_t(n) * a.D + r, t.x, t.y);
            if (c) atomicAdd(a.clamped, (unsigned long long)c);
        }
    }
}

// grid: x over the tiles of n_in, y over the phase groups; kThreads threads. q [2][groups][tp + 1][PH], P [S][groups PH], W [48000], rows [S]
extern "C" __global__ __launch_bounds__(256) void mgpu_synth_ph4_kernel(SynthArgs a, const double2* __restrict__ q, const double2* __restrict__ P,
                                                                        const double2* __restrict__ W, const SynthRow* __restrict__ rows) {
    synth_tile<4>(a, q, P, W, rows);
}
extern "C" __global__ __launch_bounds__(256) void mgpu_synth_ph2_kernel(SynthArgs a, const double2* __restrict__ q, const double2* __restrict__ P,
                                                                        const double2* __restrict__ W, const SynthRow* __restrict__ rows) {
    synth_tile<2>(a, q, P, W, rows);
}
extern "C" __global__ __launch_bounds__(256) void mgpu_synth_ph1_kernel(SynthArgs a, const double2* __restrict__ q, const double2* __restrict__ P,
                                                                        const double2* __restrict__ W, const SynthRow* __restrict__ rows) {
    synth_tile<1>(a, q, P, W, rows);
}

struct mgpu_synth {
    mgpu_ctx* c = nullptr;
    mgpu_synth_config cfg{};                      // taps points into h
    std::vector<double> h;                        // the prototype
    std::vector<mgpu_chan_channel> chans;
    int S = 0, D = 0, tp = 0, max_in = 0, PH = 1, groups = 1;
    uint64_t pos = 0;
    bool recount = true;                          // the clamp count restarts at the next call
    History<double> hist;                         // [S][tp]
    DevArray<double2> d_q, d_P, d_W;              // [2][groups][tp + 1][PH], [S][groups PH], [48000]
    DevArray<SynthRow> d_rows;                    // [S]
    DevArray<unsigned long long> d_clamped;       // [1]
    DevArray<char> d_stage;                       // host input's landing area, [S][n_in]
    DevArray<char> d_out;                         // process()'s output, max_in * D CF64 samples (made on first use)

    void upload_row(int s, hipStream_t st) {
        std::vector<double> P(size_t(groups) * PH * 2, 0.0);
        phase_row(D, chans[s].offset_hz, P.data());
        const SynthRow row{int(floor_mod(chans[s].offset_hz, MGPU_CHAN_PHASOR_LEN)), chans[s].sideband, channel_gain(D, chans[s].gain)};
        HIPCK(hipMemcpyAsync(d_P + size_t(s) * groups * PH, P.data(), P.size() * 8, hipMemcpyHostToDevice, st));
        HIPCK(hipMemcpyAsync(d_rows + s, &row, sizeof(row), hipMemcpyHostToDevice, st));
        HIPCK(hipStreamSynchronize(st));          // P and row are this call's
    }

    void check_in(const void* audio, size_t in_stride, int n_in, int format, const void* out) const {
        need(audio && out, "null pointer");
        need_iq_format(format);
        need(n_in >= 1 && n_in <= max_in, "n_in must be 1..max_in");
        need(in_stride >= size_t(n_in), "in_stride is smaller than n_in");
        need(pos + uint64_t(n_in) <= kMaxPosition, "position beyond 2^62");
    }

    // one call on device memory: the next n_in * D IQ samples into d_o
    void run(const double* d_in, size_t in_stride, int n_in, int format, void* d_o, hipStream_t st) {
        if (recount) HIPCK(hipMemsetAsync(d_clamped.p, 0, sizeof(unsigned long long), st));
        recount = false;
        SynthArgs a{};
        a.in = d_in; a.in_stride = in_stride; a.hist_old = hist.old(); a.hist_new = hist.next();
        a.out = d_o; a.clamped = d_clamped; a.format = format; a.S = S; a.D = D; a.tp = tp; a.n_in = n_in; a.groups = groups;
        a.nm = unsigned(pos % MGPU_CHAN_PHASOR_LEN);
        const dim3 grid(unsigned((n_in + kTile - 1) / kTile), unsigned(groups));
        auto* fn = PH == 4 ? mgpu_synth_ph4_kernel : PH == 2 ? mgpu_synth_ph2_kernel : mgpu_synth_ph1_kernel;
        hipLaunchKernelGGL(fn, grid, dim3(kThreads), 0, st, a, static_cast<const double2*>(d_q), static_cast<const double2*>(d_P),
                           static_cast<const double2*>(d_W), static_cast<const SynthRow*>(d_rows));
        HIPCK(hipGetLastError());
        hist.advance();
        pos += uint64_t(n_in);
    }
};

extern "C" {

int mgpu_synth_create(mgpu_ctx* c, const mgpu_synth_config* kc, const mgpu_chan_channel* channels, mgpu_synth** out) {
    const char* bad = config_error(kc, true);
    if (!bad) bad = mgpu_chan_detail::plan_error(kc->D, kc->audio_centre_hz, kc->S, channels);
    return create_stage(c, out, "mgpu_synth_create", bad, [&](mgpu_synth* k) {
        keep_config(k, kc, prototype(kc));
        k->chans.assign(channels, channels + kc->S);
        const int S = k->S = kc->S, D = k->D = kc->D, T = int(k->h.size()), tp = k->tp = (T - 1) / D;
        k->max_in = k->cfg.max_in = kc->max_in ? kc->max_in : kDefaultMaxIn;
        need((long long)k->max_in * D <= (1LL << 30), "max_in * D must be at most 2^30");
        const int PH = k->PH = phases_per_lane(D), groups = k->groups = (D + PH - 1) / PH;
        k->hist.make(size_t(S) * tp * 8);
        // the taps as the kernel walks them: [sideband][group][j = 0 .. tp][PH]; a phase beyond D - 1, and step tp of a phase above 0, are zeros
        // that no output reads
        std::vector<double> qp(size_t(T) * 2), q(size_t(2) * groups * (tp + 1) * PH * 2, 0.0);
        tap_table(k->h, D, kc->audio_centre_hz, qp.data());
        for (int sb = 0; sb < 2; ++sb)
            for (int g = 0; g < groups; ++g)
                for (int j = 0; j <= tp; ++j)
                    for (int p = 0; p < PH; ++p) {
                        const int r = g * PH + p, t = j * D + r;
                        if (r >= D || t >= T) continue;
                        double* o = q.data() + (((size_t(sb) * groups + g) * (tp + 1) + j) * PH + p) * 2;
                        o[0] = qp[2 * size_t(t)];
                        o[1] = sb ? -qp[2 * size_t(t) + 1] : qp[2 * size_t(t) + 1];
                    }
        k->d_q = DevArray<double2>(q.size() * 8);
        k->d_P = DevArray<double2>(size_t(S) * groups * PH * sizeof(double2));
        k->d_rows = DevArray<SynthRow>(size_t(S) * sizeof(SynthRow));
        k->d_clamped = DevArray<unsigned long long>(sizeof(unsigned long long));
        k->d_W = phasor_table_on_device();
        HIPCK(hipMemcpyAsync(k->d_q, q.data(), q.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemsetAsync(k->d_clamped.p, 0, sizeof(unsigned long long), c->stream));
        for (int s = 0; s < S; ++s) k->upload_row(s, c->stream);
        HIPCK(hipStreamSynchronize(c->stream));   // q is this call's
    });
}

int mgpu_synth_destroy(mgpu_synth* k) { return destroy_stage(k); }

int mgpu_synth_latency(mgpu_synth* k) { return k ? k->tp / 2 : -1; }

int mgpu_synth_seek(mgpu_synth* k, uint64_t position) {
    if (!k || position > kMaxPosition) return MGPU_ERR_ARG;
    k->pos = position;
    k->hist.restart();
    k->recount = true;
    return MGPU_OK;
}

int mgpu_synth_retune(mgpu_synth* k, int s, const mgpu_chan_channel* channel) { return retune_channel(k, s, channel); }

int mgpu_synth_process_dev(mgpu_synth* k, const double* d_audio, size_t in_stride, int n_in, int format, void* d_out, void* stream) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        k->check_in(d_audio, in_stride, n_in, format, d_out);
        k->run(d_audio, in_stride, n_in, format, d_out, stream_or_own(k->c, stream));
    });
}

int mgpu_synth_process(mgpu_synth* k, const double* audio, size_t in_stride, int n_in, int format, void* out) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        k->check_in(audio, in_stride, n_in, format, out);
        hipStream_t st = k->c->stream;
        if (!k->d_out.p) k->d_out = DevArray<char>(size_t(k->max_in) * k->D * 16);
        const double* d_in = audio;
        if (!is_device_memory(audio)) {           // the rows' n_in samples, packed
            HIPCK(hipStreamSynchronize(st));      // the stream's earlier reads of the staging buffer are over
            k->d_stage.grow(size_t(k->S) * n_in * 8);
            HIPCK(hipMemcpy2DAsync(k->d_stage.p, size_t(n_in) * 8, audio, in_stride * 8, size_t(n_in) * 8, size_t(k->S), hipMemcpyHostToDevice, st));
            d_in = reinterpret_cast<const double*>(k->d_stage.p);
            in_stride = size_t(n_in);
        }
        k->run(d_in, in_stride, n_in, format, k->d_out.p, st);
        HIPCK(hipMemcpyAsync(out, k->d_out.p, size_t(n_in) * k->D * mgpu_fmt::iq_bytes(format), hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
    });
}

int mgpu_synth_status(mgpu_synth* k, mgpu_synth_state* state) {
    if (!k || !state) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        unsigned long long n = 0;
        if (!k->recount) {
            HIPCK(hipDeviceSynchronize());        // process_dev may have run on a caller's stream
            HIPCK(hipMemcpy(&n, k->d_clamped.p, sizeof(n), hipMemcpyDeviceToHost));
        }
        *state = mgpu_synth_state{};
        state->position = k->pos; state->clamped = n;
        state->D = k->D; state->S = k->S; state->tp = k->tp; state->max_in = k->max_in; state->tile = kTile; state->phases = k->PH;
    });
}

}  // extern "C"

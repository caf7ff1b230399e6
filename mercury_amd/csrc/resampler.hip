// Rational resampler (include/ext/mercury_resampler.h): S streams at fin into S streams at fout = fin L / M, [S][n_out * C] doubles.
//
// One kernel per call, mgpu_resamp_kernel. Nothing is kept between calls but the positions and the last tp widened inputs of every stream
// (two history buffers that change roles), so how the stream is cut cannot change an output.
//
// The call's outputs are i = 0 .. n_out - 1 (absolute n0 + i). The host does the 64-bit part once: q0 = n0 M, b0 = q0 div L, r0 = q0 mod L,
// d0 = b0 - m0. Output i then reads the inputs around d = d0 + (r0 + i M) div L, counted from the call's first input (negative: the
// history), with the phase rho = (r0 + i M) mod L, in 32-bit arithmetic ((n_out + 1) M + L < 2^31 is checked at creation).
//
// A workgroup is kTile consecutive outputs of one stream, one lane per output. Their inputs are one contiguous span
// [d(first) - tp, d(last)] of at most (kTile - 1) M / L + tp + 2 samples: the workgroup writes it to LDS once, widening on the way from
// the caller's samples or, below 0, copying the history (zeros after a seek); no assembled line exists in global memory. Each lane walks
// its phase's row of the phase-major table hp[rho][j] = h[rho + j L] (16 bytes = two taps per load; the table of the tabled ratios is at
// most 164 KB and stays in L2) and its LDS span downwards, one fused multiply-add per tap into one accumulator per component: the rule's
// order. The tap h[tp L], which only phase 0 has, is a kernel argument. The workgroups of tile 0 also write the next call's history.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "resamp_tables.hpp"
#include "stream_stage.hpp"

using namespace mgpu_resamp_detail;

namespace {

constexpr int kTile = 128;                   // outputs of one stream per workgroup = threads per workgroup

struct ResampArgs {
    const void* in;           // [S][n_in * C] elements of `kind`
    const double* hist_old;   // [S][tp * C]: the inputs m0 - tp .. m0 - 1; null: zeros
    double* hist_new;         // [S][tp * C]
    const double* hp;         // [L][tp]
    double h_last;            // h[tp L]
    double* out0;             // outputs i < split:  out0[(s * stride0 + i) * C + comp]
    double* out1;             // the others:         out1[(s * stride1 + i - split) * C + comp]
    size_t stride0, stride1;
    int split, kind, n_in, n_out, tp, L, M, d0, s0, lds_elems;      // kind: the samples' mgpu_fmt::Element
    unsigned r0;
};

}  // namespace

// element e of stream s, counted from the call's first input: the caller's samples widened, the history below 0, zeros outside both
__device__ inline double resamp_x(const ResampArgs& a, int s, int C, int e) {
    const int hist = a.tp * C, n = a.n_in * C;
    if (e < 0) return (a.hist_old && e >= -hist) ? a.hist_old[size_t(s) * hist + size_t(hist + e)] : 0.0;
    if (e >= n) return 0.0;
    return mgpu_fmt::widen_at(a.kind, a.in, size_t(s) * size_t(n) + size_t(e));
}

template <int C>
__device__ inline void resamp_tile(const ResampArgs& a) {
    extern __shared__ double resamp_lds[];
    const int s = a.s0 + int(blockIdx.y), tp = a.tp;
    if (blockIdx.x == 0)                                         // the next call's history: the last tp inputs of (history, chunk)
        for (int e = threadIdx.x; e < tp * C; e += kTile) a.hist_new[size_t(s) * (tp * C) + e] = resamp_x(a, s, C, (a.n_in - tp) * C + e);
    const int i0 = int(blockIdx.x) * kTile;
    if (i0 >= a.n_out) return;
    const int i1 = min(a.n_out, i0 + kTile) - 1;
    const int lo = a.d0 + int((a.r0 + unsigned(i0) * unsigned(a.M)) / unsigned(a.L)) - tp;
    const int hi = a.d0 + int((a.r0 + unsigned(i1) * unsigned(a.M)) / unsigned(a.L));
    const int wn = min((hi - lo + 1) * C, a.lds_elems);
    for (int w = threadIdx.x; w < wn; w += kTile) resamp_lds[w] = resamp_x(a, s, C, lo * C + w);
    __syncthreads();
    const int i = i0 + int(threadIdx.x);
    if (i > i1) return;
    const unsigned u = a.r0 + unsigned(i) * unsigned(a.M), dd = u / unsigned(a.L), rho = u - dd * unsigned(a.L);
    const int pos = a.d0 + int(dd) - lo;                          // x[b] in the image; pos - tp >= 0
    if (pos - tp < 0 || (pos + 1) * C > wn) return;              // cannot happen: the span covers every lane's taps
    const double* __restrict__ hr = a.hp + size_t(rho) * tp;
    double* o = i < a.split ? a.out0 + (size_t(s) * a.stride0 + size_t(i)) * C : a.out1 + (size_t(s) * a.stride1 + size_t(i - a.split)) * C;
    if (C == 1) {
        const double* x = resamp_lds + pos;
        double acc = 0.0;
        for (int j = 0; j < tp; j += 2) {
            const double2 h = *reinterpret_cast<const double2*>(hr + j);
            acc = fma(h.x, x[-j], acc);
            acc = fma(h.y, x[-j - 1], acc);
        }
        if (rho == 0) acc = fma(a.h_last, x[-tp], acc);
        o[0] = acc;
    } else {
        const double2* x = reinterpret_cast<const double2*>(resamp_lds) + pos;
        double re = 0.0, im = 0.0;
        for (int j = 0; j < tp; j += 2) {
            const double2 h = *reinterpret_cast<const double2*>(hr + j);
            const double2 v0 = x[-j], v1 = x[-j - 1];
            re = fma(h.x, v0.x, re);
            im = fma(h.x, v0.y, im);
            re = fma(h.y, v1.x, re);
            im = fma(h.y, v1.y, im);
        }
        if (rho == 0) {
            const double2 v = x[-tp];
            re = fma(a.h_last, v.x, re);
            im = fma(a.h_last, v.y, im);
        }
        o[0] = re;
        o[1] = im;
    }
}

// grid: x over the tiles of n_out (at least one: it writes the history), y over streams; kTile threads; lds_elems doubles of LDS
extern "C" __global__ __launch_bounds__(128) void mgpu_resamp_kernel(ResampArgs a, int components) {
    if (components == 1) resamp_tile<1>(a);
    else resamp_tile<2>(a);
}

struct mgpu_resamp {
    mgpu_ctx* c = nullptr;
    mgpu_resamp_config cfg{};                     // taps points into h
    std::vector<double> h;                        // the prototype
    Ratio r;
    int S = 0, C = 0, tp = 0, max_in = 0, max_out = 0, lds_elems = 0;
    uint64_t m0 = 0;
    History<double> hist;                         // [S][tp * C]
    DevArray<double> d_hp;                        // [L][tp]
    DevArray<char> d_stage;                       // host input's landing area (ctx.hpp staged_on_device)
    DevArray<double> d_out;                       // [S][max_out * C]: process()'s output (made on first use)
    // the FIFO of mgpu_capture_run_resampled (made on its first call): what is left after the last whole hop, fewer than P per stream
    int P = 0, fill = 0, rem_cur = 0;
    DevArray<double> d_rem[2];                    // [S][P]
    DevArray<double> d_run;                       // [S][H * P]: the hops of one call, as mgpu_capture_run reads them (grown)

    int count(int n_in) const { return int(out_position(m0 + uint64_t(n_in), r) - out_position(m0, r)); }

    void check_in(const void* in, int format, int n_in, const int* n_out) const {
        need(in && n_out, "null pointer");
        need(mgpu_fmt::element(C, format) != mgpu_fmt::kNone, "the format does not fit the components");
        need(n_in >= 1 && n_in <= max_in, "n_in must be 1..max_in");
        need(m0 + uint64_t(n_in) <= MGPU_RESAMP_MAX_POSITION, "position beyond 2^52");
    }

    // one call on device memory: the next count(n_in) outputs of every stream, output i < split to out0, the others to out1
    void run(const void* d_in, int format, int n_in, double* out0, size_t stride0, int split, double* out1, size_t stride1, hipStream_t st) {
        const uint64_t n0 = out_position(m0, r), q0 = n0 * uint64_t(r.M);
        ResampArgs a{};
        a.in = d_in; a.hist_old = hist.old(); a.hist_new = hist.next();
        a.hp = d_hp; a.h_last = h.back();
        a.out0 = out0; a.out1 = out1; a.stride0 = stride0; a.stride1 = stride1; a.split = split;
        a.kind = mgpu_fmt::element(C, format); a.n_in = n_in; a.n_out = count(n_in); a.tp = tp; a.L = r.L; a.M = r.M;
        a.d0 = int(q0 / uint64_t(r.L) - m0); a.r0 = unsigned(q0 % uint64_t(r.L)); a.lds_elems = lds_elems;
        const unsigned gx = unsigned(std::max(1, (a.n_out + kTile - 1) / kTile));
        for (int s0 = 0; s0 < S; s0 += 65535) {                    // grid y is 16 bits wide
            a.s0 = s0;
            hipLaunchKernelGGL(mgpu_resamp_kernel, dim3(gx, unsigned(std::min(S - s0, 65535))), dim3(kTile), size_t(lds_elems) * 8, st, a, C);
            HIPCK(hipGetLastError());
        }
        hist.advance();
        m0 += uint64_t(n_in);
    }

    const void* on_device(const void* in, int format, int n_in, hipStream_t st) {
        return staged_on_device(d_stage, in, size_t(S) * n_in * C * mgpu_fmt::element_bytes(mgpu_fmt::element(C, format)), st);
    }
};

extern "C" {

int mgpu_resamp_create(mgpu_ctx* c, const mgpu_resamp_config* kc, mgpu_resamp** out) {
    return create_stage(c, out, "mgpu_resamp_create", config_error(kc), [&](mgpu_resamp* k) {
        ratio(kc->fin, kc->fout, &k->r);
        keep_config(k, kc, prototype(kc, k->r));
        const int L = k->r.L, M = k->r.M, tp = k->tp = int((k->h.size() - 1) / size_t(L)), S = k->S = kc->S, C = k->C = kc->components;
        k->cfg.tp = tp;
        k->max_in = k->cfg.max_in = kc->max_in ? kc->max_in : default_max_in(k->r);
        k->max_out = int(((long long)k->max_in * L + M - 1) / M) + 1;
        k->lds_elems = (((kTile - 1) * M) / L + tp + 3) * C;      // <= (127 * 16 + 515) * 2 doubles = 40752 bytes
        k->hist.make(size_t(S) * tp * C * 8);
        std::vector<double> hp(size_t(L) * tp);
        for (int rho = 0; rho < L; ++rho)
            for (int j = 0; j < tp; ++j) hp[size_t(rho) * tp + j] = k->h[size_t(rho) + size_t(j) * L];
        k->d_hp = DevArray<double>(hp.size() * 8);
        HIPCK(hipMemcpyAsync(k->d_hp, hp.data(), hp.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));   // hp is this call's
    });
}

int mgpu_resamp_destroy(mgpu_resamp* k) { return destroy_stage(k); }

int mgpu_resamp_info(mgpu_resamp* k, mgpu_resamp_status* st) {
    if (!k || !st) return MGPU_ERR_ARG;
    *st = mgpu_resamp_status{};
    st->L = k->r.L; st->M = k->r.M; st->tp = k->tp; st->S = k->S; st->components = k->C; st->max_in = k->max_in; st->max_out = k->max_out;
    st->tile = kTile; st->fifo = k->fill;
    st->delay = double(k->tp) * k->r.L / (2.0 * k->r.M);
    st->m0 = k->m0; st->n0 = out_position(k->m0, k->r);
    return MGPU_OK;
}

int mgpu_resamp_seek(mgpu_resamp* k, uint64_t position) {
    if (!k || position > MGPU_RESAMP_MAX_POSITION) return MGPU_ERR_ARG;
    k->m0 = position;
    k->hist.restart();
    k->fill = 0;
    return MGPU_OK;
}

int mgpu_resamp_process_dev(mgpu_resamp* k, const void* d_in, int format, int n_in, double* d_out, size_t out_stride, int* n_out, void* stream) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        k->check_in(d_in, format, n_in, n_out);
        const int N = k->count(n_in);
        need(size_t(N) <= out_stride && (d_out || !N), "out_stride is smaller than the call's outputs");
        *n_out = N;
        k->run(d_in, format, n_in, d_out, out_stride, N, nullptr, 0, stream_or_own(k->c, stream));
    });
}

int mgpu_resamp_process(mgpu_resamp* k, const void* in, int format, int n_in, double* out, size_t out_stride, int* n_out) {
    if (!k) return MGPU_ERR_ARG;
    return guard(k->c, [&] {
        k->check_in(in, format, n_in, n_out);
        const int N = k->count(n_in), C = k->C;
        need(size_t(N) <= out_stride && (out || !N), "out_stride is smaller than the call's outputs");
        hipStream_t st = k->c->stream;
        if (!k->d_out.p) k->d_out = DevArray<double>(size_t(k->S) * k->max_out * C * 8);
        const void* d_in = k->on_device(in, format, n_in, st);
        k->run(d_in, format, n_in, k->d_out, size_t(N), N, nullptr, 0, st);
        if (N) HIPCK(hipMemcpy2DAsync(out, out_stride * C * 8, k->d_out.p, size_t(N) * C * 8, size_t(N) * C * 8, size_t(k->S), hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        *n_out = N;
    });
}

int mgpu_capture_run_resampled(mgpu_capture* cap, mgpu_resamp* k, const void* samples, int format, int n_in, mgpu_capture_event* events,
                               uint8_t* payloads, int max_events, int* n_events, int* hops_run) {
    if (!cap || !k) return MGPU_ERR_ARG;
    mgpu_capture_geometry g{};
    if (!capture_pairs(cap, k->c, k->S, &g) || k->C != 1 || k->cfg.fout != 48000)
        return refuse(k->c, MGPU_ERR_ARG, "mgpu_capture_run_resampled: one context, the same S, components = 1 and fout = 48000");
    int H = 0;
    const int rc = guard(k->c, [&] {
        k->check_in(samples, format, n_in, hops_run);
        check_event_args(events, max_events, n_events);
        const int P = g.symbol_period, S = k->S;
        if (k->P != P) {                                              // first call, or another capture's hop: an empty FIFO of rows of P
            need(k->fill == 0, "the FIFO holds outputs for a capture with another symbol period: seek first");
            for (auto& b : k->d_rem) b = DevArray<double>(size_t(S) * P * 8);
            k->P = P;
        }
        hipStream_t st = k->c->stream;
        const void* d_in = k->on_device(samples, format, n_in, st);
        const int N = k->count(n_in), avail = k->fill + N;
        H = avail / P;
        double* rem = k->d_rem[k->rem_cur];
        if (!H) {                                                     // not a hop yet: behind what the FIFO holds
            k->run(d_in, format, n_in, rem + k->fill, size_t(P), N, nullptr, 0, st);
            k->fill = avail;
            return;
        }
        const size_t row = size_t(H) * P;
        HIPCK(hipStreamSynchronize(st));                              // d_run may be replaced
        k->d_run.grow(size_t(S) * row * 8);
        double* run = k->d_run;
        if (k->fill)
            HIPCK(hipMemcpy2DAsync(run, row * 8, rem, size_t(P) * 8, size_t(k->fill) * 8, size_t(S), hipMemcpyDeviceToDevice, st));
        // outputs up to the last whole hop behind the FIFO's content, the rest into the other remainder buffer
        k->run(d_in, format, n_in, run + k->fill, row, int(row) - k->fill, k->d_rem[k->rem_cur ^ 1], size_t(P), st);
        k->rem_cur ^= 1;
        k->fill = avail - int(row);
    });
    if (rc != MGPU_OK) return rc;
    *hops_run = H;
    if (!H) {
        *n_events = 0;
        return MGPU_OK;
    }
    // the capture runs on the same context's stream, behind the resampler's kernel
    return mgpu_capture_run(cap, k->d_run.p, MGPU_SAMPLES_F64, H, events, payloads, max_events, n_events);
}

}  // extern "C"

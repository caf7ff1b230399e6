// Diversity combining (include/mercury_diversity.h): the kernels that sum the LLR rows of a group's branches and hand the
// group's decode back to every branch row, their launchers for the grouped span (launch.hip: launch_span with io.group), the entry points
// and the host twin, and the baseband self-simulation with D branches per payload.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ctx.hpp"

#define CB_THREADS 256
constexpr int kRow = 1600;                  // floats per LLR row (tables.cpp refuses any other N)
constexpr int kRow4 = kRow / 4;

// One workgroup per group: out[g] = the group's member rows added in member order, the first one copied. first == null: the uniform rule,
// members g*D .. g*D+D-1; else the CSR pair. Every lane fetches its piece of all member rows before it adds, so the |group| loads of a
// piece are in flight together. Whether the rows can move as float4 is one test of the two base pointers (a row is 6400 bytes, so every
// row of an aligned base is aligned); it is the same for the whole launch.
extern "C" __global__ __launch_bounds__(CB_THREADS) void mgpu_llr_combine_kernel(const float* __restrict__ llr, int D, const int* __restrict__ first,
                                                                                const int* __restrict__ member, int G, float* __restrict__ out) {
    const int g = blockIdx.x, tid = threadIdx.x;
    if (g >= G) return;
    const int base = first ? first[g] : g * D;
    const int n = first ? first[g + 1] - base : D;
    size_t row[MGPU_DIVERSITY_MAX];
#pragma unroll
    for (int k = 0; k < MGPU_DIVERSITY_MAX; ++k) row[k] = k < n ? size_t(first ? member[base + k] : base + k) * kRow : 0;
    float* o = out + size_t(g) * kRow;
    if (((reinterpret_cast<uintptr_t>(llr) | reinterpret_cast<uintptr_t>(out)) & 15) == 0) {
        for (int i = tid; i < kRow4; i += CB_THREADS) {
            float4 v[MGPU_DIVERSITY_MAX];
#pragma unroll
            for (int k = 0; k < MGPU_DIVERSITY_MAX; ++k)
                if (k < n) v[k] = reinterpret_cast<const float4*>(llr + row[k])[i];
            float4 a = v[0];
#pragma unroll
            for (int k = 1; k < MGPU_DIVERSITY_MAX; ++k)
                if (k < n) { a.x += v[k].x; a.y += v[k].y; a.z += v[k].z; a.w += v[k].w; }
            reinterpret_cast<float4*>(o)[i] = a;
        }
    } else {
        for (int i = tid; i < kRow; i += CB_THREADS) {
            float v[MGPU_DIVERSITY_MAX];
#pragma unroll
            for (int k = 0; k < MGPU_DIVERSITY_MAX; ++k)
                if (k < n) v[k] = llr[row[k] + i];
            float a = v[0];
#pragma unroll
            for (int k = 1; k < MGPU_DIVERSITY_MAX; ++k)
                if (k < n) a += v[k];
            o[i] = a;
        }
    }
}

// One workgroup per frame row f = f0 + block of group f / D: the group's payload and the decode's four integers, the branch's own variance
// and, where the group decoded, the branch's own SNR - decode_tail's expression (ldpc.hip) on the value decode_tail would have read.
extern "C" __global__ __launch_bounds__(64) void mgpu_group_scatter_kernel(int f0, int F, int D, int payload_stride, const uint8_t* __restrict__ g_payload,
                                                                          const MgpuStatsDev* __restrict__ g_stats, const float* __restrict__ var,
                                                                          const float* __restrict__ snrvar, uint8_t* __restrict__ payload,
                                                                          MgpuStatsDev* __restrict__ stats) {
    const int f = f0 + int(blockIdx.x), tid = threadIdx.x;
    if (f >= F) return;
    const int g = f / D;
    for (int i = tid; i < payload_stride; i += 64) payload[size_t(f) * payload_stride + i] = g_payload[size_t(g) * payload_stride + i];
    if (tid == 0) {
        MgpuStatsDev s = g_stats[g];
        s.variance = var[f];
        const float sv = snrvar ? snrvar[f] : s.variance;
        s.snr_db = s.message_decoded ? float(10.0 * log10(1.0 / double(sv))) : -99.9f;
        stats[f] = s;
    }
}

// Row r of out = frame r / D of in: the self-simulation's clean frame in front of each of its D channel realisations (n complex samples a frame)
extern "C" __global__ __launch_bounds__(CB_THREADS) void mgpu_replicate_frames_kernel(const double2* __restrict__ in, int n, int D, int rows,
                                                                                     double2* __restrict__ out) {
    const int r = blockIdx.x;
    if (r >= rows) return;
    const double2* src = in + size_t(r / D) * n;
    double2* dst = out + size_t(r) * n;
    for (int i = threadIdx.x; i < n; i += CB_THREADS) dst[i] = src[i];
}

namespace mgpu_detail {

// The groups of a call as the header defines them; std::invalid_argument for what it refuses. Returns the number of groups.
static int check_groups(int F, int D, const int* first, const int* member, int G) {
    need(F >= 0, "diversity: F < 0");
    if (!first && !member) {
        need(D >= 1 && D <= MGPU_DIVERSITY_MAX, "diversity: D is 1..MGPU_DIVERSITY_MAX");
        need(F % D == 0, "diversity: F is not a multiple of D");
        return F / D;
    }
    need(first && member && G >= 0, "diversity: a CSR needs both first and member");
    need(first[0] == 0, "diversity: first[0] must be 0");
    for (int g = 0; g < G; ++g) {
        const long long n = (long long)first[g + 1] - first[g];
        need(n >= 1, "diversity: first must increase (no empty group)");
        need(n <= MGPU_DIVERSITY_MAX, "diversity: a group has at most MGPU_DIVERSITY_MAX members");
    }
    for (int k = 0; k < first[G]; ++k) need(member[k] >= 0 && member[k] < F, "diversity: a member is outside [0, F)");
    return G;
}

void diversity_workspaces(mgpu_ctx* c) {
    Diversity& dv = c->div;
    const size_t B = size_t(c->max_batch);
    if (!dv.done) HIPCK(hipEventCreateWithFlags(&dv.done.h, hipEventDisableTiming));
    dv.d_llr.grow(B * kRow * sizeof(float));
    dv.d_payload.grow(B * c->tab.payload_stride);
    dv.d_stats.grow(B * sizeof(MgpuStatsDev));
}

void launch_llr_combine(const float* d_llr, int D, const int* d_first, const int* d_member, int G, float* d_out, hipStream_t s) {
    for_frame_chunks(G, [&](int off, int n) {
        hipLaunchKernelGGL(mgpu_llr_combine_kernel, dim3(n), dim3(CB_THREADS), 0, s, d_first ? d_llr : d_llr + size_t(off) * D * kRow, D, at(d_first, size_t(off)),
                           d_member, n, d_out + size_t(off) * kRow);
        HIPCK(hipGetLastError());
    });
}

void launch_group_scatter(mgpu_ctx* c, const SpanIo& io, int F, int D, hipStream_t s) {
    const Diversity& dv = c->div;
    for_frame_chunks(F, [&](int off, int n) {
        hipLaunchKernelGGL(mgpu_group_scatter_kernel, dim3(n), dim3(64), 0, s, off, F, D, c->tab.payload_stride, static_cast<const uint8_t*>(dv.d_payload),
                           static_cast<const MgpuStatsDev*>(dv.d_stats), io.var, io.snrvar, io.payload, io.stats);
        HIPCK(hipGetLastError());
    });
}

// what a grouped receive call refuses, before any device work: MGPU_OK, or the code with the context's message set
static int div_refusal(mgpu_ctx* c, int F, int D) {
    const int rc = guard(nullptr, [&] {
        try {
            (void)check_groups(F, D, nullptr, nullptr, 0);
            need(F <= c->max_batch, "diversity: F must be <= max_batch");
        } catch (const std::invalid_argument& e) { c->err = e.what(); throw; }
    });
    if (rc != MGPU_OK) return rc;
    if (c->lad.n > 1)
        return refuse(c, MGPU_ERR_UNSUPPORTED,
                      "diversity combining with an estimator ladder of more than one rung is not supported (a retry would have to re-estimate whole groups)");
    return MGPU_OK;
}

}  // namespace mgpu_detail

extern "C" {

int mgpu_host_llr_combine(const float* llr, int F, int D, const int* first, const int* member, int G, float* out) {
    if (!llr || !out) return MGPU_ERR_ARG;
    int groups = 0;
    if (guard(nullptr, [&] { groups = check_groups(F, D, first, member, G); }) != MGPU_OK) return MGPU_ERR_ARG;
    for (int g = 0; g < groups; ++g) {
        const int base = first ? first[g] : g * D, n = first ? first[g + 1] - base : D;
        float* o = out + size_t(g) * kRow;
        for (int k = 0; k < n; ++k) {
            const float* r = llr + size_t(first ? member[base + k] : base + k) * kRow;
            if (k == 0) std::memcpy(o, r, kRow * sizeof(float));
            else for (int i = 0; i < kRow; ++i) o[i] = o[i] + r[i];
        }
    }
    return MGPU_OK;
}

int mgpu_llr_combine_dev(mgpu_ctx* c, const void* d_llr, int F, int D, const int* first, const int* member, int G, void* d_out, void* stream) {
    if (!c) return MGPU_ERR_ARG;
    return guard(c, [&] {
        need(d_llr && d_out, "bad argument");
        const int groups = check_groups(F, D, first, member, G);
        need(F <= c->max_batch, "diversity: F must be <= max_batch");
        if (groups == 0) return;
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (!first) {
            launch_llr_combine(static_cast<const float*>(d_llr), D, nullptr, nullptr, groups, static_cast<float*>(d_out), s);
            return;
        }
        // the CSR's device copy is the context's: one call at a time uses it, whatever streams the calls come on
        Diversity& dv = c->div;
        if (!dv.done) HIPCK(hipEventCreateWithFlags(&dv.done.h, hipEventDisableTiming));
        const size_t nf = size_t(groups) + 1, nm = size_t(first[groups]);
        if (dv.d_csr.capacity() < (nf + nm) * sizeof(int)) {
            if (dv.done_recorded) HIPCK(hipEventSynchronize(dv.done));
            dv.d_csr.grow((nf + nm) * sizeof(int));
        }
        if (dv.done_recorded) HIPCK(hipStreamWaitEvent(s, dv.done, 0));
        int* d_first = dv.d_csr;
        HIPCK(hipMemcpyAsync(d_first, first, nf * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCK(hipMemcpyAsync(d_first + nf, member, nm * sizeof(int), hipMemcpyHostToDevice, s));
        launch_llr_combine(static_cast<const float*>(d_llr), 0, d_first, d_first + nf, groups, static_cast<float*>(d_out), s);
        HIPCK(hipEventRecord(dv.done, s));
        dv.done_recorded = true;
    });
}

int mgpu_rx_batch_div_dev(mgpu_ctx* c, const void* d_bb, int F, int D, void* d_payload, void* d_stats, void* d_llr_opt, void* stream) {
    if (!c) return MGPU_ERR_ARG;
    if (!d_bb || !d_payload || !d_stats) return refuse(c, MGPU_ERR_ARG, "bad argument");
    if (const int rc = div_refusal(c, F, D)) return rc;
    return guard(c, [&] {
        if (F == 0) return;
        ensure_workspaces(c, WS_FRONTEND | (d_llr_opt ? 0u : unsigned(WS_LLR)));
        SpanIo io = own_span(c);
        io.bb = static_cast<const double*>(d_bb);
        if (d_llr_opt) io.llr = static_cast<float*>(d_llr_opt);
        io.payload = static_cast<uint8_t*>(d_payload); io.stats = static_cast<MgpuStatsDev*>(d_stats);
        io.group = D;
        launch_span(c, io, F, MgpuTapsDev{}, static_cast<hipStream_t>(stream));
    });
}

int mgpu_rx_batch_div(mgpu_ctx* c, const double* bb, int F, int D, uint8_t* payload, mgpu_frame_stats* stats, float* llr_opt) {
    if (!c) return MGPU_ERR_ARG;
    if (!bb) return refuse(c, MGPU_ERR_ARG, "bad argument");
    if (const int rc = div_refusal(c, F, D)) return rc;
    return guard(c, [&] {
        if (F == 0) return;
        const auto& t = c->tab;
        const size_t in_bytes = size_t(F) * t.frame_samples * 16;
        ensure_workspaces(c, WS_FRONTEND | WS_LLR | WS_OUT);
        c->d_baseband.grow(in_bytes);
        hipStream_t s = c->stream;
        HIPCK(hipMemcpyAsync(c->d_baseband, bb, in_bytes, hipMemcpyHostToDevice, s));
        SpanIo io = own_span(c);
        io.bb = c->d_baseband;
        io.group = D;
        launch_span(c, io, F, MgpuTapsDev{}, s);
        if (payload) HIPCK(hipMemcpyAsync(payload, c->d_payload, size_t(F) * t.payload_stride, hipMemcpyDeviceToHost, s));
        if (stats) HIPCK(hipMemcpyAsync(stats, c->d_stats, size_t(F) * sizeof(MgpuStatsDev), hipMemcpyDeviceToHost, s));
        if (llr_opt) HIPCK(hipMemcpyAsync(llr_opt, c->d_llr, size_t(F) * kRow * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
    });
}

int mgpu_baseband_test_esn0_div(mgpu_ctx* c, const double* esn0_db, int npoints, long long groups_per_point, uint64_t seed, uint64_t frame0,
                                const mgpu_hf_channel* ch, int D, mgpu_error_rate* out) {
    if (!c) return MGPU_ERR_ARG;
    if (!ch) return refuse(c, MGPU_ERR_ARG, "no channel");
    if (const int rc = div_refusal(c, 0, D)) return rc;
    return guard(c, [&] {
        hf_check(ch);
        need(esn0_db && out && npoints > 0 && groups_per_point > 0, "bad argument");
        need(D <= c->max_batch, "diversity: a group of D frames does not fit max_batch");
        const auto& t = c->tab;
        const int B = int(std::min<long long>(groups_per_point, c->max_batch / D));      // groups per batch
        ensure_workspaces(c, WS_FRONTEND | WS_LLR | WS_OUT);
        diversity_workspaces(c);
        const size_t frame_bytes = size_t(t.frame_samples) * 16;
        DevBuf d_clean(size_t(B) * frame_bytes), d_rep(size_t(B) * D * frame_bytes), d_bb(size_t(B) * D * frame_bytes);
        DevBuf d_sent(size_t(B) * t.payload_stride), d_acc(4 * 8);
        hipStream_t s = c->stream;
        for (int p = 0; p < npoints; ++p) {
            const double noise_amp = std::pow(10.0, -esn0_db[p] / 20.0) / std::sqrt(2.0);      // per component, as mgpu_baseband_test_esn0
            HIPCK(hipMemsetAsync(d_acc.p, 0, 32, s));
            for (long long done = 0; done < groups_per_point; done += B) {
                const int n = int(std::min<long long>(B, groups_per_point - done)), rows = n * D;
                const uint64_t first = frame0 + uint64_t(p) * uint64_t(groups_per_point) + uint64_t(done);
                launch_txgen(c, seed, first, n, 0.0, 0, d_clean.as<double>(), d_sent.as<uint8_t>(), s);
                hipLaunchKernelGGL(mgpu_replicate_frames_kernel, dim3(rows), dim3(CB_THREADS), 0, s, d_clean.as<double2>(), t.frame_samples, D, rows,
                                   d_rep.as<double2>());
                HIPCK(hipGetLastError());
                launch_hf_baseband(ch, d_rep.as<double>(), t.frame_samples, noise_amp, seed, first * uint64_t(D), rows, d_bb.as<double>(), s);
                SpanIo io = own_span(c);
                io.bb = d_bb.as<double>();
                io.zf_snr = false;           // the error counter does not read snr_db
                io.group = D;
                launch_span(c, io, rows, MgpuTapsDev{}, s);
                // once per group, on the decoder's compact rows (this stream ran the span: the workspaces are still this call's)
                hipLaunchKernelGGL(mgpu_error_count_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_sent.as<uint8_t>(), static_cast<const uint8_t*>(c->div.d_payload),
                                   static_cast<const MgpuStatsDev*>(c->div.d_stats), t.payload_stride, t.nReal, n, d_acc.as<unsigned long long>());
                HIPCK(hipGetLastError());
                HIPCK(hipEventRecord(c->div.done, s));       // the counter is the workspaces' last reader
            }
            unsigned long long acc[4];
            HIPCK(hipMemcpyAsync(acc, d_acc.p, 32, hipMemcpyDeviceToHost, s));
            HIPCK(hipStreamSynchronize(s));
            mgpu_error_rate& r = out[p];
            r.esn0_db = esn0_db[p];
            r.Frames_total = groups_per_point; r.Error_frames_total = (long long)acc[1];
            r.Bits_total = groups_per_point * t.nReal; r.Error_bits_total = (long long)acc[0];
            r.BER = double(r.Error_bits_total) / double(r.Bits_total);
            r.FER = double(r.Error_frames_total) / double(r.Frames_total);
            r.avg_iterations = double(acc[2]) / double(groups_per_point);
            r.crc_ok_frames = (long long)acc[3];
        }
    });
}

}  // extern "C"

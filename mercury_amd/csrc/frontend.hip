// RX front-end for gfx950: one workgroup per OFDM frame, everything between the baseband
// samples and the LDPC input stays in LDS; HBM sees the samples once (16 B/sample, coalesced)
// and 1600 floats out.
//
// Stages and the reference code they reproduce (same operations, same order, FP64, no FMA
// contraction — this TU is built with -ffp-contract=off):
//   symbol_demod ............. ofdm.cc:862-867 (gi_remover :423-429, radix-2 DIT fft :310-340 with
//                              1/Nfft scaling :431-444, zero_depadder :401-411)
//   automatic_gain_control ... ofdm.cc:1467-1498
//   LS_/ZF_channel_estimator . ofdm.cc:1315-1451 / :1266-1313 ; matrix_multiplication misc.cc:73-91
//   interpolate_linear_col ... interpolator.cc:163-254
//   restore_channel_amplitude  ofdm.cc:1453-1466 ; get_angle/set_complex misc.cc:34-71
//   channel_equalizer ........ ofdm.cc:1637-1647 (complex divide = libgcc __divdc3, Smith)
//   measure_variance ......... ofdm.cc:1500-1521 (sequential sum, narrowed to float by the callers)
//   deframer + deinterleaver . ofdm.cc:837-852, interleaver.cc:94-109   (one gather table)
//   cl_psk::demod ............ psk.cc:278-326 (double distances narrowed to float, float LLR math)
//   deinterleaver + re-pack .. interleaver.cc:77-92, telecom_system.cc:1300-1308 (one gather table)
//
// Sequential reductions (AGC mean, variance) are kept sequential on purpose: the terms are
// produced in parallel, one lane adds them in the reference's order, so the float `variance`
// that scales every LLR is bit-identical to the CPU path.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_tables.h"
#include "fft256.h"
#include "fe_math.h"
#include "ls_rect.h"

namespace {

// restore_channel_amplitude for one cell (ofdm.cc:1453-1466, set_complex misc.cc:65-71), with the reference platform's atan and
// sincos restated (glibc_trig.h): the unit phasor is bit-identical to the CPU's. Kept out of line so that the constants of the
// three routines do not stay live (and spill) across the rest of the front-end kernel.
__device__ __attribute__((noinline)) c2 unit_phasor(c2 h) {
    const double th = get_angle(h);
    double s, c;
    gl_sincos(th, &s, &c);
    return {1 * c, 1 * s};
}

// The two evaluations of the residual carrier-offset stage (CFO below), out of line for the same reason.
__device__ __attribute__((noinline)) double cfo_angle(c2 r) { return get_angle(r); }
__device__ __attribute__((noinline)) c2 cfo_phasor(double x) {
    double s, c;
    gl_sincos(x, &s, &c);
    return {c, s};
}

}  // namespace

// device probe of glibc_trig.h for tests: atan, sin and cos of n arguments
extern "C" __global__ void mgpu_glibc_trig_probe_kernel(const double* __restrict__ in, double* __restrict__ out_atan, double* __restrict__ out_sin,
                                                        double* __restrict__ out_cos, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out_atan[i] = gl_atan(in[i]);
    double s, c;
    gl_sincos(in[i], &s, &c);
    out_sin[i] = s;
    out_cos[i] = c;
}

// Sum n doubles from LDS in index order with one lane: the additions are a dependent chain by
// construction (the reference's `+=` loop), so the only thing to hide is the LDS latency: fetch eight
// ahead while the previous eight are being added.
__device__ __forceinline__ double serial_sum(const double* red, int n) {
    double acc = 0;
    int p = 0;
    for (; p + 8 <= n; p += 8) {
        const double a0 = red[p], a1 = red[p + 1], a2 = red[p + 2], a3 = red[p + 3];
        const double a4 = red[p + 4], a5 = red[p + 5], a6 = red[p + 6], a7 = red[p + 7];
        acc += a0; acc += a1; acc += a2; acc += a3; acc += a4; acc += a5; acc += a6; acc += a7;
    }
    for (; p < n; ++p) acc += red[p];
    return acc;
}

// Workgroup size: 512 threads (three workgroups per compute unit in the QPSK and QAM modes, two in the long BPSK frames); a
// 1024-thread variant exists for configurations whose LDS carve lets only one workgroup onto a compute unit.

// LDS carve (bytes): grid 16G (the carrier grid, equalised in place at the end) | work = Hp 16 nPilots (channel estimate at the pilots,
//                    pilot order) + rsz (reduction terms / signed pilots / demapper LLRs), first the FFT work areas | aux = tw 2048
//                    during the FFTs, then type G + scal 64 (the cell types are first needed by the estimator)
// The channel estimate of a DATA cell is never stored: interpolation, amplitude restoration and the equaliser are applied to a cell
// in one go (the interpolated value is a function of two pilot estimates). That keeps the frame at one grid + one pilot-sized
// array: 40 KB in mode 8, 67 KB in the BPSK modes (92 KB with a second full grid: one workgroup per compute unit).
// The FFT runs on as many wavefronts as work areas fit next to the grid without costing a workgroup per compute unit.
struct FeCarve { int fft_waves; size_t rsz, work, total; };
// after: bytes of the work area kept behind Hp and rsz once the FFTs are done (none in the plain form)
__host__ __device__ inline FeCarve fe_carve_with(int G, int nPilots, int nBits, int FE_WAVES, size_t after) {
    FeCarve c;
    c.rsz = size_t(16) * (nPilots + 8) > size_t(4) * nBits ? size_t(16) * (nPilots + 8) : size_t(4) * nBits;   // + 8: zero pad behind the signed pilots (LS row reads)
    c.rsz = (c.rsz + 15) & ~size_t(15);
    const size_t per_wave = size_t(FFT256_STRIDE) * 16, lds_cu = size_t(160) * 1024;
    const size_t aux0 = size_t((G + 15) & ~15) + 64, aux = aux0 > 2048 ? aux0 : 2048;
    const size_t fixed = size_t(16) * G + aux, need = size_t(16) * nPilots + c.rsz + after;
    const size_t minimal = fixed + (need > 4 * per_wave ? need : 4 * per_wave);
    // LDS is handed out in blocks of 1280 bytes (measured: three workgroups of 53,504 bytes run side by side on a compute unit, three of
    // 54,016 do not — the runtime's occupancy calculator says 3 for both), so a workgroup's share is a whole number of blocks
    const size_t block = 1280;
    // ... less 256 bytes: round 4 measured three workgroups of 53,504 bytes resident and three of 53,760 (42 blocks exactly) not. The same
    // budget (bytes + 256, rounded up to blocks) counts the workgroups AND sizes the FFT work areas.
    const size_t overhead = 256;
    size_t wgs = lds_cu / ((minimal + overhead + block - 1) / block * block);  // workgroups per compute unit by LDS with the fewest FFT work areas
    const size_t cap = size_t(24 / FE_WAVES) > 0 ? size_t(24 / FE_WAVES) : 1;    // 80 registers per lane: 24 wavefronts per compute unit
    if (wgs > cap) wgs = cap;
    if (wgs < 1) wgs = 1;
    const size_t share = lds_cu / wgs / block * block;
    size_t w = share > fixed + overhead ? (share - overhead - fixed) / per_wave : 0;
    c.fft_waves = int(w < 4 ? 4 : (w > size_t(FE_WAVES) ? size_t(FE_WAVES) : w));
    c.work = need > c.fft_waves * per_wave ? need : c.fft_waves * per_wave;
    c.total = fixed + c.work;
    return c;
}
// The channel-aware demapper's form (CSI below; include/mercury_demapper.h) keeps two more arrays in the work area: the terms of its own
// noise variance, one double per pilot, and |h|^2 of every data cell as a float, in de-framed order. Both are written after the FFTs, whose
// work areas they share, so the carve grows only where Hp + rsz + these exceed the FFT areas: 5.6 KB in the BPSK modes (73.6 -> 79.4 KB, still
// two workgroups per compute unit - with a float per CELL it would be 82.6 KB and one), nothing in the others.
__host__ __device__ inline size_t fe_csi_var_bytes(int nPilots) { return (size_t(8) * nPilots + 15) & ~size_t(15); }
__host__ __device__ inline size_t fe_csi_h2_bytes(int G, int nPilots) { return (size_t(4) * (G - nPilots) + 15) & ~size_t(15); }
// The noise-map demapper's form (NMAP below; include/mercury_demapper.h MGPU_DEMAP_NMAP) is the CSI form with one more piece behind |h|^2: the
// carrier sums S_c (64 doubles), the symbol sums U_s (Nsymb doubles) and the two scales a_c (64 floats) and b_s (Nsymb floats). Everything
// before it in the work area is in use when it is written (Hp by the data cells, the three term arrays by their sums, |h|^2 being filled) and
// the LLRs take the terms' place while a_c and b_s are read, so it is a piece of its own: 1,056 bytes in mode 8, where the FFT work areas
// cover it, 1,344 more than the CSI carve in the BPSK modes (79,392 -> 80,736 bytes: still two workgroups per compute unit).
__host__ __device__ inline size_t fe_nmap_bytes(int G) { return (size_t(64) * 12 + size_t(G / 50) * 12 + 15) & ~size_t(15); }
// A form's carve (ls_rect.h: the form bits), for the host and for the kernel alike: the noise map's with NMAP, else the CSI form's with CSI,
// else the plain one. RECT and CFO keep nothing in LDS behind the FFTs, and neither do the Wiener forms (WIENER below;
// include/mercury_estimator.h MGPU_RUNG_WIENER): the time pass writes Hp, the frequency pass the signed pilots' area (16 nPilots bytes of rsz).
__host__ __device__ inline FeCarve fe_carve_form(int G, int nPilots, int nBits, int FE_WAVES, unsigned form) {
    const size_t csi = fe_csi_var_bytes(nPilots) + fe_csi_h2_bytes(G, nPilots);
    return fe_carve_with(G, nPilots, nBits, FE_WAVES, form & MGPU_FE_NMAP ? csi + fe_nmap_bytes(G) : form & MGPU_FE_CSI ? csi : 0);
}
extern "C" size_t mgpu_frontend_form_lds_bytes(int G, int nPilots, int nBits, int threads, unsigned form) {
    return mgpu_fe_form_valid(form) ? fe_carve_form(G, nPilots, nBits, threads / 64, form).total : 0;
}
// the forms' carves by their earlier names, which the host tests call
extern "C" size_t mgpu_frontend_lds_bytes(int G, int nPilots, int nBits, int threads) { return mgpu_frontend_form_lds_bytes(G, nPilots, nBits, threads, 0); }
extern "C" size_t mgpu_frontend_csi_lds_bytes(int G, int nPilots, int nBits, int threads) { return mgpu_frontend_form_lds_bytes(G, nPilots, nBits, threads, MGPU_FE_RECT | MGPU_FE_CSI); }
extern "C" size_t mgpu_frontend_wiener_lds_bytes(int G, int nPilots, int nBits, int threads, int csi) {
    return mgpu_frontend_form_lds_bytes(G, nPilots, nBits, threads, MGPU_FE_RECT | MGPU_FE_WIENER | (csi ? MGPU_FE_CSI : 0));
}
extern "C" size_t mgpu_frontend_nmap_lds_bytes(int G, int nPilots, int nBits, int threads) { return mgpu_frontend_form_lds_bytes(G, nPilots, nBits, threads, MGPU_FE_RECT | MGPU_FE_CSI | MGPU_FE_NMAP); }
// workgroups per compute unit the LDS lets a carve of `bytes` have, counted as fe_carve_with counts them (blocks of 1280 bytes, 256 of overhead)
extern "C" int mgpu_frontend_lds_workgroups(size_t bytes) { return int(size_t(160) * 1024 / ((bytes + 256 + 1279) / 1280 * 1280)); }

// RECT: the LS window has a width and a height of its own (`win`, ls_rect.h) instead of T.lsw squared, and the workgroup may take its
// frame from a list: the form the estimator ladder runs (ladder.hip). Everything else is the one body.
// CSI: the channel-aware demapper (include/mercury_demapper.h). Every cell is equalised with the full estimate h (no
// restore_channel_amplitude), the LLRs are (|h|^2 / sigma2) (d1 - d0) with sigma2 = mean |g - h x|^2 over the pilots, and the H and eq taps
// show that h and g / h. variance, SNR variance and mean_H are still the plain form's, term for term.
// CFO: pilot-aided residual carrier-offset correction (include/mercury_cfo.h) between the AGC and the estimate: the phase
// of the summed lag-Dy products of same-carrier pilots, divided by Dy, is the turn per symbol; symbol s is turned back by s times that.
// Its scratch (50 carrier sums, one phasor per symbol: at most (64 + 255) * 16 B) is the head of the work area, where the FFTs are done
// and the estimate has not begun (>= four FFT work areas, 16 KB): no carve changes.
// WIENER: the estimate at the pilots is the separable Wiener filter's (include/mercury_estimator.h MGPU_RUNG_WIENER) instead
// of the window mean; `win` only carries the frame list. Its two passes live in Hp and the signed pilots' area: no carve changes.
// NMAP (with CSI): the noise-map demapper (include/mercury_demapper.h MGPU_DEMAP_NMAP). The CSI form's pilot residuals are
// also averaged per carrier and per symbol; the LLRs of a cell are scaled by a_c b_s |h|^2 with a_c = 1 / (sigma2 fc(c)), b_s = 1 / fs(s)
// in place of |h|^2 / sigma2, fc and fs being those means over sigma2, 1 inside the dead band. Its scratch is a piece of the carve of its own.
template <int FE_THREADS, unsigned FORM>
__device__ __forceinline__ void fe_frame(const MgpuDev& T, const double* __restrict__ baseband, int F, float* __restrict__ llr_out,
                                         float* __restrict__ variance_out, float* __restrict__ snr_variance_out, double* __restrict__ eqdata_out,
                                         const MgpuTapsDev& taps, const MgpuFeOpt& opt) {
    static_assert(mgpu_fe_form_valid(FORM), "any option implies RECT, and the noise-map demapper is a form of the channel-aware one");
    constexpr bool RECT = FORM & MGPU_FE_RECT, CSI = FORM & MGPU_FE_CSI, CFO = FORM & MGPU_FE_CFO, WIENER = FORM & MGPU_FE_WIENER, NMAP = FORM & MGPU_FE_NMAP;
    [[maybe_unused]] const MgpuLsRect& win = opt.win;
    [[maybe_unused]] const MgpuCsi& csi = opt.csi;
    [[maybe_unused]] const MgpuCfo& cfo = opt.cfo;
    [[maybe_unused]] const MgpuWiener& wn = opt.wn;
    [[maybe_unused]] const MgpuNmap& nm = opt.nm;
    constexpr int FE_WAVES = FE_THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int G = T.G, Nc = 50, Ns = T.Nsymb;
    const FeCarve carve = fe_carve_form(G, T.nPilots, T.nBits, FE_WAVES, FORM);
    c2* grid = reinterpret_cast<c2*>(smem);
    c2* Hp = grid + G;                                              // channel estimate at the pilots, pilot order; Hp and red are the FFT work area first
    c2* fftb = Hp;
    double* red = reinterpret_cast<double*>(__builtin_assume_aligned(Hp + T.nPilots, 16));        // nPilots doubles
    float* llr = reinterpret_cast<float*>(red);                     // demapper output reuses the reduction area
    c2* yp = reinterpret_cast<c2*>(red);                            // pilots in row-major pilot order, multiplied by their sign
    // (every piece of the carve is a multiple of 16 bytes; said so, a c2 is one ds_read_b128 - 4 LDS-pipeline cycles - instead of a ds_read2_b64 - 8: tools/ubench/lds_mask.hip)
    c2* tw = reinterpret_cast<c2*>(__builtin_assume_aligned(reinterpret_cast<unsigned char*>(Hp) + carve.work, 16));
    int8_t* type = reinterpret_cast<int8_t*>(tw);                   // 0 data, +1 / -1 pilot with that sign; takes the twiddles' place after the FFTs
    double* scal = reinterpret_cast<double*>(type + ((G + 15) & ~15));
    // CSI: behind rsz, the terms of sigma2 in pilot order and |h|^2 per data cell in de-framed order
    [[maybe_unused]] double* red3 = reinterpret_cast<double*>(__builtin_assume_aligned(reinterpret_cast<unsigned char*>(red) + carve.rsz, 16));
    [[maybe_unused]] float* wf = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(red3) + fe_csi_var_bytes(T.nPilots));
    // NMAP: behind |h|^2, the carrier sums, the symbol sums (their means later), the carrier scales, the symbol scales
    [[maybe_unused]] double* nm_S = reinterpret_cast<double*>(__builtin_assume_aligned(reinterpret_cast<unsigned char*>(wf) + ((size_t(4) * (G - T.nPilots) + 15) & ~size_t(15)), 16));
    [[maybe_unused]] double* nm_U = nm_S + 64;
    [[maybe_unused]] float* nm_a = reinterpret_cast<float*>(nm_U + Ns);
    [[maybe_unused]] float* nm_b = nm_a + 64;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.x;
    if (f >= F) return;
    int fin = f;                                                    // the frame read; f is the row written
    if constexpr (RECT) { if (win.frames) fin = win.frames[f]; }
    const c2* bb = reinterpret_cast<const c2*>(baseband) + size_t(fin) * T.frame_samples;
    const double boost = T.pilot_boost;
    int stamp_i = 0;
#define FE_STAMP() do { if (taps.cycles && f == (F >> 1) && tid == 0) taps.cycles[stamp_i] = __builtin_readcyclecounter(); ++stamp_i; } while (0)    /* a frame from the middle of the launch: the compute unit is in its steady mix of phases */
    FE_STAMP();

    for (int i = tid; i < 128; i += FE_THREADS) tw[fft256_tw_slot(i)] = {T.twiddle[2 * i], T.twiddle[2 * i + 1]};
    __syncthreads();

    // ---- symbol_demod: one wave per symbol (fft256.h), next symbol's samples requested before the butterflies ----
    c2 n0 = {0, 0}, n1 = {0, 0}, n2 = {0, 0}, n3 = {0, 0};
    const Fft256CarrierLane fcl = fft256_carrier_lane(lane);
    const int nfw = carve.fft_waves;                                // waves that own an FFT work area
    if (wave < nfw && wave < Ns) {
        const c2* in = bb + size_t(wave) * 272 + 16;                // gi_remover
        n0 = in[lane]; n1 = in[lane + 64]; n2 = in[lane + 128]; n3 = in[lane + 192];
    }
    for (int s = wave; wave < nfw && s < Ns; s += nfw) {
        c2 r0 = n0, r1 = n1, r2 = n2, r3 = n3;
        if (s + nfw < Ns) {
            const c2* in = bb + size_t(s + nfw) * 272 + 16;
            n0 = in[lane]; n1 = in[lane + 64]; n2 = in[lane + 128]; n3 = in[lane + 192];
        }
        // 1/Nfft scale + zero_depadder: a lane ends with the one bin it keeps, if any (fft256.h: 50 of the 256 bins are carriers)
        const c2 x = wave_fft256_carriers(r0, r1, r2, r3, fftb + wave * FFT256_STRIDE, tw, lane, fcl);
        if (fcl.col >= 0) grid[s * Nc + fcl.col] = {x.re / 256.0, x.im / 256.0};
    }
    __syncthreads();
    for (int i = tid; i < G; i += FE_THREADS) type[i] = T.cell_type[i] ? (T.pilot_val[i] < 0 ? int8_t(-1) : int8_t(1)) : int8_t(0);
    __syncthreads();

    FE_STAMP();   // 1: FFT done
    // ---- automatic_gain_control ---------------------------------------------------------------
    if (T.agc) {
        for (int p = tid; p < T.nPilots; p += FE_THREADS) {
            const c2 y = grid[T.pilot_cell[p]];
            red[p] = sqrt(y.re * y.re + y.im * y.im);
        }
        __syncthreads();
        if (tid == 0) {
            double amp = serial_sum(red, T.nPilots);
            amp /= T.nPilots;
            scal[0] = boost / amp;
        }
        __syncthreads();
        const double agc = scal[0];
        for (int c = tid; c < G; c += FE_THREADS) grid[c] = {grid[c].re * agc, grid[c].im * agc};
        __syncthreads();
        if (taps.agc_gain && tid == 0) taps.agc_gain[f] = agc;
    }
    if constexpr (CFO) {
        c2* acc = Hp;                                               // [Nc] a_c
        c2* rot = Hp + 64;                                          // [Ns] {cos, sin} of -step * s
        if (tid < Nc) {                                             // one lane per carrier adds its chain (at most 15 pairs), in symbol order
            double ar = 0, ai = 0;
            for (int q = cfo.first[tid]; q < cfo.first[tid + 1]; ++q) {
                const int q0 = cfo.pair[2 * q], q1 = cfo.pair[2 * q + 1];
                c2 z0 = grid[q0], z1 = grid[q1];
                if (type[q0] < 0) z0 = {-z0.re, -z0.im};
                if (type[q1] < 0) z1 = {-z1.re, -z1.im};
                ar += z1.re * z0.re + z1.im * z0.im;
                ai += z1.im * z0.re - z1.re * z0.im;
            }
            acc[tid] = {ar, ai};
        }
        __syncthreads();
        if (tid == 0) {
            double rr = 0, ri = 0;
            for (int c = 0; c < Nc; ++c) { const c2 a = acc[c]; rr += a.re; ri += a.im; }
            const bool ok = fabs(rr) < __builtin_inf() && fabs(ri) < __builtin_inf() && !(rr == 0 && ri == 0);
            const double step = ok ? cfo_angle(c2{rr, ri}) / double(cfo.Dy) : 0.0;
            scal[5] = step;
            scal[6] = ok ? 1.0 : 0.0;
            bool first_pass = true;                                 // a retry computes the same step and does not write it out
            if constexpr (RECT) first_pass = win.frames == nullptr;
            if (first_pass && cfo.step && f < cfo.step_rows) cfo.step[f] = step;
        }
        __syncthreads();
        if (scal[6] != 0) {                                         // (the whole workgroup takes the same side)
            const double step = scal[5];
            if (tid < Ns) rot[tid] = cfo_phasor(-step * double(tid));
            __syncthreads();
            for (int c = tid; c < G; c += FE_THREADS) {
                const c2 g = grid[c], r = rot[c / Nc];
                grid[c] = {g.re * r.re - g.im * r.im, g.re * r.im + g.im * r.re};
            }
            __syncthreads();
        }
    }
    if (taps.grid) for (int c = tid; c < G; c += FE_THREADS) { taps.grid[(size_t(f) * G + c) * 2] = grid[c].re; taps.grid[(size_t(f) * G + c) * 2 + 1] = grid[c].im; }

    FE_STAMP();   // 2: AGC done (in the CFO forms: AGC and the carrier-offset stage)
    // ---- channel estimate at the pilots -------------------------------------------------------
    if constexpr (WIENER) {
        // The separable Wiener estimate: the signed pilots filtered along time per carrier (real taps, one matrix row per
        // pilot), then along frequency per symbol (complex taps); one lane per pilot in both passes, the sums in ascending symbol and
        // ascending carrier order as mgpu_host_wiener_estimate forms them. The second pass writes where the signed pilots were.
        for (int p = tid; p < T.nPilots; p += FE_THREADS) {
            const int q = T.pilot_cell[p];
            const c2 y = grid[q];
            yp[p] = type[q] < 0 ? c2{-y.re, -y.im} : y;
        }
        __syncthreads();
        const double* __restrict__ wA = wn.A;
        const double* __restrict__ wB = wn.B;
        if (wn.n_designs > 1) {                                     // (uniform) a bank: the frame chooses its design (include/mercury_wiener_bank.h)
            // One lane per symbol adds the terms conj(yp[a]) yp[b] of its symbol's 1-pairs and 2-pairs in ascending a; its four sums go to
            // Hp, which is free until the time pass. Lanes 0..3 of the first wavefront then add the symbols' sums in ascending symbols, one
            // component each, and lane 0 applies the tests: the same terms in the same order as mgpu_host_wiener_select.
            const MgpuWienerBank& bk = *wn.bank;
            double* part = reinterpret_cast<double*>(Hp);           // [Ns][4]: 32 Ns <= 16 nPilots bytes (checked where the bank is set)
            for (int s = tid; s < Ns; s += FE_THREADS) {
                double r1r = 0, r1i = 0, r2r = 0, r2i = 0;
                for (int p = bk.sym_first[s], p1 = bk.sym_first[s + 1]; p < p1; ++p) {
                    const unsigned fl = bk.pair[p];
                    const c2 a = yp[p];
                    if (fl & 1u) { const c2 b = yp[p + 1]; r1r += (a.re * b.re) + (a.im * b.im); r1i += (a.re * b.im) - (a.im * b.re); }
                    if (fl & 2u) { const c2 b = yp[p + 2]; r2r += (a.re * b.re) + (a.im * b.im); r2i += (a.re * b.im) - (a.im * b.re); }
                }
                part[4 * s] = r1r; part[4 * s + 1] = r1i; part[4 * s + 2] = r2r; part[4 * s + 3] = r2i;
            }
            __syncthreads();
            if (wave == 0) {
                double acc = 0;
                if (lane < 4) for (int s = 0; s < Ns; ++s) acc += part[4 * s + lane];
                const double R1r = __shfl(acc, 0), R1i = __shfl(acc, 1), R2r = __shfl(acc, 2), R2i = __shfl(acc, 3);
                if (lane == 0) {
                    const double q2 = (R2r * R2r + R2i * R2i) * bk.n1sq, q1 = (R1r * R1r + R1i * R1i) * bk.n2sq;
                    int ch = wn.n_designs - 1;                      // the fallback; the first eligible entry in bank order otherwise
                    for (int d = wn.n_designs - 2; d >= 0; --d) {
                        const double rho2 = bk.sel[d][0], ur = bk.sel[d][1], ui = bk.sel[d][2], t = bk.sel[d][3];
                        bool ok = q2 >= rho2 * q1;                  // every comparison fails on a NaN
                        if (t >= 0) {
                            const double zr = R1r * ur + R1i * ui, zi = R1i * ur - R1r * ui;
                            ok = ok && zr > 0 && fabs(zi) <= t * zr;
                        }
                        if (ok) ch = d;
                    }
                    scal[7] = double(ch);
                    if (wn.choice && f < wn.rows) {                 // rung 0 alone: a retry measures the same and does not write it out
                        wn.choice[f] = ch;
                        wn.corr[4 * size_t(f)] = R1r; wn.corr[4 * size_t(f) + 1] = R1i; wn.corr[4 * size_t(f) + 2] = R2r; wn.corr[4 * size_t(f) + 3] = R2i;
                    }
                }
            }
            __syncthreads();
            const int ch = __builtin_amdgcn_readfirstlane(int(scal[7]));      // the same in every lane: the table bases stay scalar
            wA += size_t(ch) * size_t(bk.a_stride);
            wB += size_t(ch) * size_t(bk.b_stride) * 2;
        }
        const uint4* __restrict__ wpilot = reinterpret_cast<const uint4*>(wn.pilot);
        for (int p = tid; p < T.nPilots; p += FE_THREADS) {
            const uint4 q = wpilot[p];
            const int n = int(q.y & 0xffffu);
            const double* __restrict__ a = wA + wn.a_off[q.x & 0xffffu] + int(q.x >> 16) * n;
            const uint16_t* __restrict__ list = wn.col_list + (q.y >> 16);
            double hr = 0, hi = 0;
            for (int k = 0; k < n; ++k) {
                const c2 v = yp[list[k]];
                hr += a[k] * v.re; hi += a[k] * v.im;
            }
            Hp[p] = {hr, hi};
        }
        __syncthreads();
        for (int p = tid; p < T.nPilots; p += FE_THREADS) {
            const uint4 q = wpilot[p];
            const int n = int(q.w & 0xffffu);
            const c2* __restrict__ b = reinterpret_cast<const c2*>(wB) + wn.b_off[q.z & 0xffffu] + int(q.z >> 16) * n;
            const c2* t = Hp + (q.w >> 16);
            double hr = 0, hi = 0;
            for (int m = 0; m < n; ++m) {
                const c2 w = b[m], v = t[m];
                hr += w.re * v.re - w.im * v.im;
                hi += w.re * v.im + w.im * v.re;
            }
            yp[p] = {hr, hi};
        }
        __syncthreads();
        for (int p = tid; p < T.nPilots; p += FE_THREADS) Hp[p] = yp[p];
    } else {
        const int hwt = RECT ? win.hw_t : T.lsw / 2, hwf = RECT ? win.hw_f : T.lsw / 2;      // half-widths in time (rows) and frequency (columns)
        const int lattice = RECT ? win.lattice : T.regular_lattice;
        const double* __restrict__ ls_weight = RECT ? win.weight : T.ls_weight;
        const bool ls_fast = T.estimator != 0 && lattice;
        int ls_rows = 0;     // 1: every window row holds >= 3 pilots and every pilot of the frame is finite -> the branch-free row loop below
        if (ls_fast) {       // x*y for the LS sums: the pilot's sign applied once ((-w)*y == w*(-y) exactly), in pilot order
            int finite = 1;
            for (int p = tid; p < T.nPilots + 8; p += FE_THREADS) {
                if (p >= T.nPilots) { yp[p] = {0.0, 0.0}; continue; }
                const int q = T.pilot_cell[p];
                const c2 y = grid[q];
                yp[p] = type[q] < 0 ? c2{-y.re, -y.im} : y;
                finite &= (fabs(y.re) < __builtin_inf()) & (fabs(y.im) < __builtin_inf());
            }
            ls_rows = __syncthreads_and(finite) && lattice == 2;
        }
        for (int p = tid; p < T.nPilots; p += FE_THREADS) {
            const int c = T.pilot_cell[p], i = c / Nc, j = c - i * Nc;
            if (T.estimator == 0) {            // ZF: Y / (x + 0i) reduces to two real divisions in __divdc3
                const double x = type[c] < 0 ? -boost : boost;
                Hp[p] = {grid[c].re / x, grid[c].im / x};
            } else {                           // LS over the (clipped) window - 21x21 unless RECT -, row-major order
                const int k0 = max(i - hwt, 0), k1 = min(i + hwt, Ns - 1), l0 = max(j - hwf, 0), l1 = min(j + hwf, Nc - 1);
                double hr = 0, hi = 0;
                if (ls_fast) {
                    // pilots of row k sit at columns == k (mod 3); rows hold 17,17,16 pilots cyclically, so the pilot
                    // index of (k, l) is 50*(k/3) + {0,17,34}[k%3] + (l - k%3)/3 and a row's window pilots are contiguous
                    // per column residue r = k % 3: first window column == r (mod 3), how many pilots, and the offset of
                    // that first pilot inside its row; computed once per pilot, then rows just cycle through r
                    int cntr[3], offr[3];
    #pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        const int first = l0 + ((r - l0) % 3 + 3) % 3;
                        cntr[r] = first <= l1 ? (l1 - first) / 3 + 1 : 0;
                        offr[r] = (r == 0 ? 0 : r == 1 ? 17 : 34) + (first - r) / 3;
                    }
                    int n = 0;
                    {
                        int r = k0 % 3;
                        for (int k = k0; k <= k1; ++k) { n += r == 0 ? cntr[0] : r == 1 ? cntr[1] : cntr[2]; r = r == 2 ? 0 : r + 1; }
                    }
                    const double w = ls_weight[n];
                    if (ls_rows) {
                        // Rows k0, k0+1, k0+2, k0+3, ... cycle through the three column residues, so a lane's (pilot count, first pilot) pair of a
                        // row depends only on the row's place in that cycle. A row's first three pilots are always inside the window; pilots
                        // four to seven are added with the weight w or +0.0: x + (+-0 * y) == x exactly for finite y, and the sums start at +0.0
                        // and can therefore never be -0.0. Same terms in the same order as the loop below, without its per-term branches.
                        const int r0 = k0 % 3;
                        int ptr[3];
                        double wq[3][4];
    #pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            const int r = r0 + q >= 3 ? r0 + q - 3 : r0 + q;
                            const int cn = r == 0 ? cntr[0] : r == 1 ? cntr[1] : cntr[2];
                            ptr[q] = 50 * ((k0 + q) / 3) + (r == 0 ? offr[0] : r == 1 ? offr[1] : offr[2]);
    #pragma unroll
                            for (int m = 0; m < 4; ++m) wq[q][m] = m + 3 < cn ? w : 0.0;
                        }
                        auto add_row = [&](int q) {
                            const c2* row = yp + ptr[q];
                            const c2 v0 = row[0], v1 = row[1], v2 = row[2], v3 = row[3], v4 = row[4], v5 = row[5], v6 = row[6];
                            hr += w * v0.re; hi += w * v0.im;
                            hr += w * v1.re; hi += w * v1.im;
                            hr += w * v2.re; hi += w * v2.im;
                            hr += wq[q][0] * v3.re; hi += wq[q][0] * v3.im;
                            hr += wq[q][1] * v4.re; hi += wq[q][1] * v4.im;
                            hr += wq[q][2] * v5.re; hi += wq[q][2] * v5.im;
                            hr += wq[q][3] * v6.re; hi += wq[q][3] * v6.im;
                            ptr[q] += 50;
                        };
                        for (int k = k0; k <= k1; k += 3) {
                            add_row(0);
                            if (k + 1 <= k1) add_row(1);
                            if (k + 2 <= k1) add_row(2);
                        }
                        Hp[p] = {hr, hi};
                        continue;
                    }
                    int km = k0 % 3, rowbase = 50 * (k0 / 3);
                    for (int k = k0; k <= k1; ++k) {
                        const int cnt = km == 0 ? cntr[0] : km == 1 ? cntr[1] : cntr[2];
                        const c2* row = yp + rowbase + (km == 0 ? offr[0] : km == 1 ? offr[1] : offr[2]);
                        if (km == 2) { km = 0; rowbase += 50; } else ++km;
                        if (cnt == 0) continue;
                        // a window row holds at most 7 pilots: fetch all seven at once (one LDS latency per row; reading past
                        // the row's end stays inside the LDS carve), add the first cnt in order
                        const c2 v0 = row[0], v1 = row[1], v2 = row[2], v3 = row[3], v4 = row[4], v5 = row[5], v6 = row[6];
                        hr += w * v0.re; hi += w * v0.im;
                        if (cnt > 1) { hr += w * v1.re; hi += w * v1.im; }
                        if (cnt > 2) { hr += w * v2.re; hi += w * v2.im; }
                        if (cnt > 3) { hr += w * v3.re; hi += w * v3.im; }
                        if (cnt > 4) { hr += w * v4.re; hi += w * v4.im; }
                        if (cnt > 5) { hr += w * v5.re; hi += w * v5.im; }
                        if (cnt > 6) { hr += w * v6.re; hi += w * v6.im; }
                    }
                } else {
                    int n = 0;
                    for (int k = k0; k <= k1; ++k)
                        for (int l = l0; l <= l1; ++l) n += type[k * Nc + l] != 0;
                    const double w = ls_weight[n];
                    for (int k = k0; k <= k1; ++k)
                        for (int l = l0; l <= l1; ++l) {
                            const int q = k * Nc + l;
                            if (!type[q]) continue;
                            const double xw = type[q] < 0 ? -w : w;
                            hr += xw * grid[q].re;
                            hi += xw * grid[q].im;
                        }
                }
                Hp[p] = {hr, hi};
            }
        }
    }
    __syncthreads();
    FE_STAMP();   // 3: estimate done
    // ---- interpolate_linear_col + restore_channel_amplitude + channel_equalizer, one cell at a time ----------------------
    if (taps.mean_H) {      // mean |H| over the MEASURED (pilot) cells in cell order, telecom_system.cc:1224-1243
        for (int p = tid; p < T.nPilots; p += FE_THREADS) { const c2 h = Hp[p]; red[p] = hypot(h.re, h.im); }
        __syncthreads();
        if (tid == 0) taps.mean_H[f] = T.nPilots > 0 ? serial_sum(red, T.nPilots) / T.nPilots : -1.0;
        __syncthreads();
    }
    FE_STAMP();   // 4: (interpolation is part of the equaliser pass below)
    // A data cell (i, j): column j has its pilots in the rows == j (mod 3) (checked on the host), so the two pilot rows it interpolates
    // between follow from (i - j) mod 3 (above the first / below the last pilot: extrapolation from the nearest two), and a pilot of
    // row r, column j has index first_pilot(r) + j / 3 in pilot order (rows hold 17, 17, 16 pilots cyclically). The cell's estimate
    // = lerp of the two pilot estimates (interpolator.cc:163-254), made a unit phasor in the PSK modes (ofdm.cc:1453-1466), divides the
    // received cell (ofdm.cc:1637-1647); the equalised value replaces the received one in the grid. Same operations per cell as the
    // reference's three passes over a full channel grid.
    const uint2* __restrict__ cell_lerp = reinterpret_cast<const uint2*>(T.cell_lerp);
    auto equalise_data = [&](int idx) {
        // the cell, the pilot rows a / b it interpolates between and their pilots' indices in its column: tabulated on the host (create.hip)
        const uint2 q = cell_lerp[idx];
        const int c = int(q.x & 0xfffu), pa = int((q.x >> 12) & 0x3ffu), pb = int(q.x >> 22);
        const int a = int(q.y & 0xffu), b = int((q.y >> 8) & 0xffu), i = int(q.y >> 16);
        c2 h = lerp(Hp[pa], double(a), Hp[pb], double(b), double(i));
        if constexpr (CSI) wf[idx] = float(h.re * h.re + h.im * h.im);
        else if (T.amp_restore) h = unit_phasor(h);
        if (taps.H) { taps.H[(size_t(f) * G + c) * 2] = h.re; taps.H[(size_t(f) * G + c) * 2 + 1] = h.im; }
        grid[c] = cdiv(grid[c], h);
    };
    // The pilot cells first, all of them in one pass: the term of the variance before amplitude restoration (PSK modes; SNR report),
    // the cell's own equalisation, and the term of the variance that scales the LLRs (from the un-equalised cell in the
    // baseband_test_EsN0 variant). Both variances are sums of nPilots terms in pilot order — dependent chains for one lane — so
    // wavefront 0 adds them while the other wavefronts equalise the data cells, handed out in runs of 64 from a counter in LDS;
    // wavefront 0 joins when its sums are done.
    double* red2 = reinterpret_cast<double*>(__builtin_assume_aligned(red + ((T.nPilots + 1) & ~1), 16));   // second term array (the signed pilots are no longer needed), on a 16-byte boundary
    int* queue = reinterpret_cast<int*>(scal + 3);
    if (tid == 0) *queue = 0;
    for (int p = tid; p < T.nPilots; p += FE_THREADS) {
        const int c = T.pilot_cell[p];
        const c2 g = grid[c];
        c2 h = Hp[p];
        [[maybe_unused]] const c2 h0 = h;
        const double x = type[c] < 0 ? -boost : boost;
        if (T.amp_restore) {                                         // measure_variance(equalized_data_without_amplitude_restoration)
            const c2 e0 = cdiv(g, h);
            const double dr = e0.re - x, di = e0.im - 0.0;
            red[p] = dr * dr + di * di;
            h = unit_phasor(h);
        }
        if constexpr (CSI) {
            if (taps.H) { taps.H[(size_t(f) * G + c) * 2] = h0.re; taps.H[(size_t(f) * G + c) * 2 + 1] = h0.im; }
            const double dr = g.re - h0.re * x, di = g.im - h0.im * x;
            red3[p] = dr * dr + di * di;
        } else {
            if (taps.H) { taps.H[(size_t(f) * G + c) * 2] = h.re; taps.H[(size_t(f) * G + c) * 2 + 1] = h.im; }
        }
        const c2 e = cdiv(g, h);
        if constexpr (CSI) grid[c] = cdiv(g, h0);
        else grid[c] = e;
        const c2 v = T.var_eq ? e : g;
        const double dr = v.re - x, di = v.im - 0.0;
        red2[p] = dr * dr + di * di;
    }
    __syncthreads();
    FE_STAMP();   // 5: pilot cells done
    if (tid == 0) {
        if (T.amp_restore) {
            double var = serial_sum(red, T.nPilots);
            var /= double(T.nPilots);
            scal[2] = var;
        }
        double var = serial_sum(red2, T.nPilots);
        var /= double(T.nPilots);
        scal[1] = var;
    }
    if constexpr (CSI) {
        if (tid == 64) {      // the third chain on a wavefront of its own
            double var = serial_sum(red3, T.nPilots);
            var /= double(T.nPilots);
            scal[4] = var;
        }
    }
    if constexpr (NMAP) {
        // the same terms once more per carrier (ascending symbols) and per symbol (ascending carriers), a lane each on wavefronts 2 and 3 to 6
        if (tid >= 128 && tid < 128 + Nc) {
            const int c = tid - 128;
            double acc = 0;
            for (int q = nm.car_first[c]; q < nm.car_first[c + 1]; ++q) acc += red3[nm.car_list[q]];
            nm_S[c] = acc;
        } else if (tid >= 192 && tid < 192 + Ns) {
            const int sy = tid - 192;
            double acc = 0;
            for (int p = nm.sym_first[sy]; p < nm.sym_first[sy + 1]; ++p) acc += red3[p];
            nm_U[sy] = acc;
        }
    }
    for (;;) {
        int base = 0;
        if (lane == 0) base = atomicAdd(queue, 64);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= T.nData) break;
        if (base + lane < T.nData) equalise_data(base + lane);
    }
    __syncthreads();
    if constexpr (NMAP) {
        // The factors (mgpu_host_demap_nmap is the normative statement): a mean over sigma2, exactly 1 when it is NaN, has no pilot, sigma2
        // is 0 or not finite, or it lies inside the dead band. A retry computes its own map and does not write it out.
        const double sigma2 = scal[4], band = nm.band;
        const bool usable = sigma2 != 0 && fabs(sigma2) < __builtin_inf();
        const bool report = win.frames == nullptr && nm.fc && f < nm.rows;
        auto banded = [&](double v, int n) {
            const double fr = v / sigma2;
            return (usable && n > 0 && (fr > band || fr * band < 1)) ? fr : 1.0;
        };
        if (tid < Nc) {
            const int lo = max(tid - nm.smooth, 0), hi = min(tid + nm.smooth, Nc - 1);
            double sum = 0;
            for (int c = lo; c <= hi; ++c) sum += nm_S[c];
            const int n = int(nm.car_first[hi + 1]) - int(nm.car_first[lo]);
            const double fc = banded(sum / double(n), n);
            nm_a[tid] = 1.0f / float(sigma2 * fc);
            if (report) nm.fc[size_t(f) * Nc + tid] = fc;
        } else if (tid >= 64 && tid < 64 + Ns) {
            const int sy = tid - 64;
            const int n = int(nm.sym_first[sy + 1]) - int(nm.sym_first[sy]);
            const double fs = banded(nm_U[sy] / double(n), n);
            nm_b[sy] = 1.0f / float(fs);
            if (report) nm.fs[size_t(f) * Ns + sy] = fs;
        }
        __syncthreads();
    }
    c2* eq = grid;
    if (taps.eq) for (int c = tid; c < G; c += FE_THREADS) { taps.eq[(size_t(f) * G + c) * 2] = eq[c].re; taps.eq[(size_t(f) * G + c) * 2 + 1] = eq[c].im; }
    if (eqdata_out)   // de-framed equalised symbols, kept for the zero-forcing modes' post-decode SNR (ofdm_deframed_data)
        for (int i = tid; i < T.nData; i += FE_THREADS) { const c2 e = eq[T.data_cell[i]]; eqdata_out[(size_t(f) * T.nData + i) * 2] = e.re; eqdata_out[(size_t(f) * T.nData + i) * 2 + 1] = e.im; }
    const float variance = float(scal[1]);
    if (tid == 0) {
        variance_out[f] = variance;
        if (snr_variance_out) snr_variance_out[f] = T.amp_restore ? float(scal[2]) : variance;
        if (taps.variance) taps.variance[f] = scal[1];
    }

    FE_STAMP();   // 6: equalise + variance done
    // ---- deframe + time/freq de-interleave + max-log demap -------------------------------------
    [[maybe_unused]] const float inv_var = CSI ? 1 / float(scal[4]) : 1 / variance;
    const int M = T.M, bps = T.bps;
    // cl_psk::demod (psk.cc:278-326): squared distance to every constellation point in double, narrowed to float; per bit the smallest
    // distance among the points with that bit set / clear; LLR = (d1 - d0) / variance in float. Specialised per constellation size so that
    // "which of the two minima does point j feed" is a compile-time fact (one v_min_f32 per point and bit) — with M at run time it is a
    // bit test, two compares and two selects per point and bit, and the 32 points of mode 16 were half of that mode's front-end time.
    // fminf keeps the running minimum when the new distance is NaN, like the reference's `if (D < d)`.
    auto demap_all = [&](auto m_tag) {
        constexpr int MM = decltype(m_tag)::value;
        constexpr int BPS = MM == 2 ? 1 : MM == 4 ? 2 : MM == 8 ? 3 : MM == 16 ? 4 : 5;
        for (int k = tid; k < T.nData; k += FE_THREADS) {
            const c2 s = eq[T.sym_src[k]];
            float scale;
            if constexpr (NMAP) { const int cell = T.sym_src[k], sy = cell / Nc; scale = (nm_a[cell - sy * Nc] * nm_b[sy]) * wf[csi.sym_data[k]]; }
            else scale = CSI ? inv_var * wf[csi.sym_data[k]] : inv_var;
            if (taps.syms) { taps.syms[(size_t(f) * T.nData + k) * 2] = s.re; taps.syms[(size_t(f) * T.nData + k) * 2 + 1] = s.im; }
            float d0[BPS], d1[BPS];
#pragma unroll
            for (int b = 0; b < BPS; ++b) { d0[b] = __builtin_inff(); d1[b] = __builtin_inff(); }
#pragma unroll
            for (int j = 0; j < MM; ++j) {
                const double dr = s.re - T.constellation[2 * j], di = s.im - T.constellation[2 * j + 1];
                const float D = float(dr * dr + di * di);
#pragma unroll
                for (int b = 0; b < BPS; ++b) {
                    if ((j >> b) & 1) d1[b] = __builtin_fminf(d1[b], D);
                    else d0[b] = __builtin_fminf(d0[b], D);
                }
            }
#pragma unroll
            for (int b = 0; b < BPS; ++b) llr[k * BPS + (BPS - 1 - b)] = scale * (d1[b] - d0[b]);
        }
    };
    if (M == 2 && bps == 1) demap_all(std::integral_constant<int, 2>());
    else if (M == 4 && bps == 2) demap_all(std::integral_constant<int, 4>());
    else if (M == 8 && bps == 3) demap_all(std::integral_constant<int, 8>());
    else if (M == 16 && bps == 4) demap_all(std::integral_constant<int, 16>());
    else if (M == 32 && bps == 5) demap_all(std::integral_constant<int, 32>());
    else
    for (int k = tid; k < T.nData; k += FE_THREADS) {
        const c2 s = eq[T.sym_src[k]];
        float scale;
        if constexpr (NMAP) { const int cell = T.sym_src[k], sy = cell / Nc; scale = (nm_a[cell - sy * Nc] * nm_b[sy]) * wf[csi.sym_data[k]]; }
        else scale = CSI ? inv_var * wf[csi.sym_data[k]] : inv_var;
        if (taps.syms) { taps.syms[(size_t(f) * T.nData + k) * 2] = s.re; taps.syms[(size_t(f) * T.nData + k) * 2 + 1] = s.im; }
        float d0[5], d1[5];
#pragma unroll
        for (int b = 0; b < 5; ++b) { d0[b] = __builtin_inff(); d1[b] = __builtin_inff(); }
        for (int j = 0; j < M; ++j) {
            const double dr = s.re - T.constellation[2 * j], di = s.im - T.constellation[2 * j + 1];
            const float D = float(dr * dr + di * di);
#pragma unroll
            for (int b = 0; b < 5; ++b) {
                if (b < bps) {
                    if ((j >> b) & 1) { if (D < d1[b]) d1[b] = D; }
                    else { if (D < d0[b]) d0[b] = D; }
                }
            }
        }
#pragma unroll
        for (int b = 0; b < 5; ++b)
            if (b < bps) llr[k * bps + (bps - 1 - b)] = scale * (d1[b] - d0[b]);
    }
    __syncthreads();
    if (taps.llr_demod) for (int i = tid; i < T.nBits; i += FE_THREADS) taps.llr_demod[size_t(f) * T.nBits + i] = llr[i];
    FE_STAMP();   // 7: demap done
    // ---- bit de-interleave + shortening re-pack -------------------------------------------------
    for (int p = tid; p < T.N; p += FE_THREADS) llr_out[size_t(f) * T.N + p] = llr[T.llr_src[p]];
    FE_STAMP();   // 8: end
#undef FE_STAMP
}

// The 13 forms, one row each: the kernel's name, the options it is built with, and how the options' arguments reach it. Every row makes
// the 512- and the 1024-thread kernel; a form reads the members of `opt` that its bits name.
//   plain ....... the context's own square window and nothing else: the default span
//   rect ........ a window of its own and an optional frame list (include/mercury_estimator.h): rung 0 of an estimator ladder when it is
//                 not the context's own window, and every later rung on the frames that rung left undecoded
//   csi, nmap ... every launch of the span while the context's demapper is MGPU_DEMAP_CSI / MGPU_DEMAP_NMAP (include/mercury_demapper.h)
//   cfo ......... every launch of the span while the context's correction is MGPU_CFO_PILOTS (include/mercury_cfo.h)
//   wiener ...... a Wiener rung of an estimator ladder, as rung 0 or as a retry (include/mercury_estimator.h MGPU_RUNG_WIENER)
// OPT: the one signature, the options' arguments in a trailing MgpuFeOpt. WIN_CSI: the csi pair alone takes its two structs as arguments of
// their own, (..., MgpuTapsDev, MgpuLsRect, MgpuCsi): with the wider argument block, whatever its layout, the compiler gives the pair two
// more spill slots at 512 threads and a vector register more at 1024 (profiles/frontend_forms.md); frontend_untimed has one `if` for it.
#define FE_FORMS(X)                                                                                                 \
    X(mgpu_frontend_kernel, 0, OPT)                                                                                 \
    X(mgpu_frontend_rect_kernel, MGPU_FE_RECT, OPT)                                                                 \
    X(mgpu_frontend_csi_kernel, MGPU_FE_RECT | MGPU_FE_CSI, WIN_CSI)                                                \
    X(mgpu_frontend_cfo_kernel, MGPU_FE_RECT | MGPU_FE_CFO, OPT)                                                    \
    X(mgpu_frontend_csi_cfo_kernel, MGPU_FE_RECT | MGPU_FE_CSI | MGPU_FE_CFO, OPT)                                  \
    X(mgpu_frontend_wiener_kernel, MGPU_FE_RECT | MGPU_FE_WIENER, OPT)                                              \
    X(mgpu_frontend_wiener_cfo_kernel, MGPU_FE_RECT | MGPU_FE_CFO | MGPU_FE_WIENER, OPT)                            \
    X(mgpu_frontend_wiener_csi_kernel, MGPU_FE_RECT | MGPU_FE_CSI | MGPU_FE_WIENER, OPT)                            \
    X(mgpu_frontend_wiener_csi_cfo_kernel, MGPU_FE_RECT | MGPU_FE_CSI | MGPU_FE_CFO | MGPU_FE_WIENER, OPT)          \
    X(mgpu_frontend_nmap_kernel, MGPU_FE_RECT | MGPU_FE_CSI | MGPU_FE_NMAP, OPT)                                    \
    X(mgpu_frontend_nmap_cfo_kernel, MGPU_FE_RECT | MGPU_FE_CSI | MGPU_FE_NMAP | MGPU_FE_CFO, OPT)                  \
    X(mgpu_frontend_wiener_nmap_kernel, MGPU_FE_RECT | MGPU_FE_CSI | MGPU_FE_NMAP | MGPU_FE_WIENER, OPT)            \
    X(mgpu_frontend_wiener_nmap_cfo_kernel, MGPU_FE_RECT | MGPU_FE_CSI | MGPU_FE_NMAP | MGPU_FE_CFO | MGPU_FE_WIENER, OPT)

#define FE_ARGS_OPT MgpuFeOpt opt
#define FE_PASS_OPT opt
#define FE_ARGS_WIN_CSI MgpuLsRect win, MgpuCsi csi
#define FE_PASS_WIN_CSI MgpuFeOpt{win, MgpuNmap{}, MgpuWiener{}, MgpuCfo{}, csi}
#define FE_KERNEL(name, form, args)                                                                                                        \
    extern "C" __global__ __launch_bounds__(512, 6) void name(                                                                             \
        MgpuDev T, const double* __restrict__ baseband, int F, float* __restrict__ llr_out, float* __restrict__ variance_out,              \
        float* __restrict__ snr_variance_out, double* __restrict__ eqdata_out, MgpuTapsDev taps, FE_ARGS_##args) {                         \
        fe_frame<512, (form)>(T, baseband, F, llr_out, variance_out, snr_variance_out, eqdata_out, taps, FE_PASS_##args);                  \
    }                                                                                                                                      \
    extern "C" __global__ __launch_bounds__(1024, 4) void name##_t1024(                                                                    \
        MgpuDev T, const double* __restrict__ baseband, int F, float* __restrict__ llr_out, float* __restrict__ variance_out,              \
        float* __restrict__ snr_variance_out, double* __restrict__ eqdata_out, MgpuTapsDev taps, FE_ARGS_##args) {                         \
        fe_frame<1024, (form)>(T, baseband, F, llr_out, variance_out, snr_variance_out, eqdata_out, taps, FE_PASS_##args);                 \
    }
FE_FORMS(FE_KERNEL)
#undef FE_KERNEL

// a form's kernel for a workgroup of `threads` (512 or 1024); null when the form is none of the 13
extern "C" const void* mgpu_frontend_form_kernel(int threads, unsigned form) {
#define FE_ROW(name, form, args) {(form), reinterpret_cast<const void*>(name), reinterpret_cast<const void*>(name##_t1024)},
    static const struct { unsigned form; const void *t512, *t1024; } table[] = {FE_FORMS(FE_ROW)};
#undef FE_ROW
    for (const auto& row : table)
        if (row.form == form) return threads == 1024 ? row.t1024 : threads == 512 ? row.t512 : nullptr;
    return nullptr;
}

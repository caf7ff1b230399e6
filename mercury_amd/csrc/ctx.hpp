// Private to the library: the context behind the opaque mgpu_ctx handle, the kernel declarations and the helpers
// that the host-side translation units share. Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include <cmath>
#include "../../include/mercury_gpu.h"
#include "../../include/mercury_rxloop.h"
#include "../../include/mercury_channel.h"
#include "../../include/mercury_estimator.h"
#include "../../include/mercury_wiener_bank.h"
#include "../../include/mercury_diversity.h"
#include "../../include/mercury_demapper.h"
#include "../../include/mercury_cfo.h"
#include "../../include/mercury_blanker.h"
#include "../../include/ext/mercury_excisor.h"
#include "device_tables.h"
#include "geometry_cache.hpp"
#include "ls_rect.h"
#include "sample_formats.h"
#include "tables.hpp"

extern "C" size_t mgpu_frontend_lds_bytes(int G, int nPilots, int nBits, int threads);
extern "C" size_t mgpu_frontend_csi_lds_bytes(int G, int nPilots, int nBits, int threads);
extern "C" size_t mgpu_frontend_nmap_lds_bytes(int G, int nPilots, int nBits, int threads);
// The OFDM front-end's kernels stay in frontend.hip; these two name them. A form is a set of MGPU_FE_* bits (ls_rect.h), and every kernel has
// the signature (MgpuDev, const double*, int, float*, float*, float*, double*, MgpuTapsDev, MgpuFeOpt) - but the form RECT | CSI, which takes
// (..., MgpuTapsDev, MgpuLsRect, MgpuCsi): frontend.hip FE_FORMS says why. A form that is none of the 13: null, 0.
extern "C" const void* mgpu_frontend_form_kernel(int threads, unsigned form);
extern "C" size_t mgpu_frontend_form_lds_bytes(int G, int nPilots, int nBits, int threads, unsigned form);
extern "C" size_t mgpu_spa_lds_bytes(int E, int N);
extern "C" size_t mgpu_gbf_lds_bytes(int N);
extern "C" size_t mgpu_spa_fast_lds_bytes(int Sg, int N);
extern "C" size_t mgpu_txgen_lds_bytes(int G);

extern "C" __global__ void mgpu_ladder_select_kernel(const MgpuStatsDev*, int, int, int*, int*, int*, unsigned long long*);
extern "C" __global__ void mgpu_ladder_merge_kernel(const int*, int, int, int, int, const float*, const float*, const float*, const double*, const uint8_t*,
                                                    const MgpuStatsDev*, float*, float*, float*, double*, uint8_t*, MgpuStatsDev*, int*, unsigned long long*);
extern "C" __global__ void mgpu_mfsk_frontend_kernel_m32(MgpuDev, const double*, int, int, float*, float*, float*, MgpuTapsDev);
extern "C" __global__ void mgpu_mfsk_frontend_kernel_m16x2(MgpuDev, const double*, int, int, float*, float*, float*, MgpuTapsDev);
extern "C" int mgpu_mfsk_syms_per_block();
extern "C" __global__ void mgpu_slot_energy_kernel(const double*, int, int, int, const double*, double*);
extern "C" __global__ void mgpu_mfsk_sync_kernel(const double*, int, int, MgpuMfskSync, const int*, int*);
extern "C" __global__ void mgpu_zf_snr_kernel(MgpuDev, const uint8_t*, const double*, int, MgpuStatsDev*, double*);
extern "C" size_t mgpu_zfsnr_lds_bytes(int nData);
extern "C" __global__ void mgpu_p2b_kernel(const double*, int, const double*, const int*, int, int, int, const double*, int, double, double, double*, const int*, const double*, const int*, int);
extern "C" __global__ void mgpu_p2b_slide_d1_kernel(const double*, int, const double*, const int*, int, int, const double*, double, double, double*, const int*, const double*, const int*, int);
extern "C" __global__ void mgpu_p2b_slide_d4_kernel(const double*, int, const double*, const int*, int, int, const double*, double, double, double*, const int*, const double*, const int*, int);
extern "C" __global__ void mgpu_p2b_slide_d1_sincos_kernel(const double*, int, const double*, const int*, int, int, const double*, double, double, double*, const int*, const double*, const int*, int);
extern "C" __global__ void mgpu_p2b_slide_d4_sincos_kernel(const double*, int, const double*, const int*, int, int, const double*, double, double, double*, const int*, const double*, const int*, int);
// launch shape of one kernel variant, and what the streaming coarse kernel is built for (sync.hip)
struct MgpuKernelGeometry { int outputs_per_block, threads, lds_bytes; };
struct MgpuStreamGeometry { int step, ngi, nfft, pre, K, ring; };
extern "C" MgpuKernelGeometry mgpu_p2b_slide_geometry(int decim);      // decimation 1 or 4
extern "C" __global__ void mgpu_tsync_metric_kernel(const double*, int, const int*, const int*, const int*, int, int, int, int, int, double*);
extern "C" __global__ void mgpu_tsync_metric_dense_kernel(const double*, int, const int*, const int*, const int*, int, int, int, int, int, double*);
extern "C" int mgpu_tsync_coarse_threads();
extern "C" __global__ void mgpu_tsync_metric_stream_kernel(const double*, int, const int*, const int*, const int*, int, double*, int, int, int);
extern "C" MgpuStreamGeometry mgpu_tsync_stream_geometry();
extern "C" __global__ void mgpu_tsync_metric_fine_kernel_r4(const double*, int, const int*, const int*, const int*, int, int, int, int, double*);
extern "C" __global__ void mgpu_tsync_metric_fine_kernel_r8(const double*, int, const int*, const int*, const int*, int, int, int, int, double*);
extern "C" MgpuKernelGeometry mgpu_tsync_fine_geometry(int R);          // R = 4 or 8 candidates per lane
extern "C" __global__ void mgpu_tsync_metric_generic_kernel(const double*, int, const int*, const int*, const int*, int, int, int, int, int, double*);
extern "C" __global__ void mgpu_fsync_kernel(const double*, int, int, const double*, double*);
extern "C" __global__ void mgpu_span_energy_kernel(const double*, int, const int*, const int*, int, int, double*, int*);
extern "C" __global__ void mgpu_span_energy_many_kernel(const double*, int, const int*, const int*, int, int, double*, int*);
extern "C" __global__ void mgpu_window_energy_kernel(const double*, int, int, double*);
extern "C" __global__ void mgpu_select_peak_kernel(const double*, const int*, int, int, const int*, const int*, int, int, int*, double*);
extern "C" __global__ void mgpu_decimate_kernel(const double*, int, const int*, const int*, const int*, int, int, double*);
#define DECL_SPA(NE) extern "C" __global__ void mgpu_ldpc_spa_kernel_ne##NE(LdpcDev, const float*, int, uint8_t*, int*, uint8_t*, MgpuStatsDev*, const float*, const float*);
extern "C" int mgpu_spa_max_degree(int ne);     // largest check degree the ne-round instance's unrolled product walk covers
DECL_SPA(4) DECL_SPA(5) DECL_SPA(6) DECL_SPA(7) DECL_SPA(8)
extern "C" __global__ void mgpu_spa_math_probe_kernel(const double*, double*, double*, int);
extern "C" __global__ void mgpu_glibc_trig_probe_kernel(const double*, double*, double*, double*, int);
using DecoderKernel = void (*)(LdpcDev, const float*, int, uint8_t*, int*, uint8_t*, MgpuStatsDev*, const float*, const float*);
extern "C" __global__ void mgpu_gen_payload_kernel(uint64_t, uint64_t, int, int, int, uint8_t*);
extern "C" __global__ void mgpu_passband_channel_kernel(const double*, int, int, int, double, uint64_t, uint64_t, int, double*);
extern "C" __global__ void mgpu_error_count_kernel(const uint8_t*, const uint8_t*, const MgpuStatsDev*, int, int, int, unsigned long long*);
extern "C" __global__ void mgpu_ldpc_gbf_kernel(LdpcDev, const float*, int, uint8_t*, int*, uint8_t*, MgpuStatsDev*, const float*, const float*);
#define DECL_MS(T) extern "C" __global__ void mgpu_ldpc_minsum_kernel_t##T(LdpcDev, const float*, int, uint8_t*, int*, uint8_t*, MgpuStatsDev*, const float*, const float*);
DECL_MS(512)
#define DECL_SF(T) extern "C" __global__ void mgpu_ldpc_spa_fast_kernel_t##T(LdpcDev, const float*, int, uint8_t*, int*, uint8_t*, MgpuStatsDev*, const float*, const float*);
DECL_SF(512)
extern "C" __global__ void mgpu_ldpc_encode_kernel(MgpuDev, const uint8_t*, int, uint8_t*);
extern "C" __global__ void mgpu_txgen_kernel(MgpuDev, uint64_t, uint64_t, int, double, int, double*, uint8_t*, const uint8_t*, int, const int*, int, int);

static_assert(sizeof(MgpuStatsDev) == sizeof(mgpu_frame_stats), "stats layout");

namespace mgpu_detail {

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
#define HIPCK(expr)                                                                              \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) throw HipError(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

hipError_t host_alloc_on_node(void** p, size_t bytes, int node);   // create.hip
int device_numa_node(int device);

// Owning handles: move-only, released by the destructor (errors ignored), so that a throw on any path frees what was made before it.
struct DevBuf {
    void* p = nullptr;
    void* view = nullptr;       // when set: page-locked host memory holding the buffer's current content, which kernels read in place
    DevBuf() = default;
    explicit DevBuf(size_t bytes) : cap(bytes ? bytes : 16) { HIPCK(hipMalloc(&p, cap)); }
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { swap(o); return *this; }
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <typename T> T* as() { return static_cast<T*>(view ? view : p); }
    size_t capacity() const { return cap; }
    // a buffer that only grows: reallocated (old one freed first, content not kept) when smaller than `bytes`
    void grow(size_t bytes) {
        if (cap >= bytes) return;
        *this = DevBuf();
        *this = DevBuf(bytes);
    }
private:
    size_t cap = 0;
    void swap(DevBuf& o) noexcept { std::swap(p, o.p); std::swap(view, o.view); std::swap(cap, o.cap); }
};
// a DevBuf that reads as a T* (the context's workspaces and tables)
template <typename T> struct DevArray : DevBuf {
    using DevBuf::DevBuf;
    operator T*() const { return static_cast<T*>(p); }
};
template <typename H, hipError_t (*Destroy)(H)> struct Handle {
    H h = nullptr;              // created in place: HIPCK(hipStreamCreate(&s.h))
    Handle() = default;
    Handle(Handle&& o) noexcept { std::swap(h, o.h); }
    Handle& operator=(Handle&& o) noexcept { std::swap(h, o.h); return *this; }
    ~Handle() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;
using GraphExec = Handle<hipGraphExec_t, hipGraphExecDestroy>;
using PinnedBuf = Handle<void*, hipHostFree>;   // page-locked host memory from host_alloc_on_node

template <typename T>
DevArray<T> upload(const std::vector<T>& v) {
    DevArray<T> d(v.size() * sizeof(T) + 16);
    HIPCK(hipMemcpy(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}

// The estimator ladder of a context (include/mercury_estimator.h; ladder.hip). n == 0: none, every entry point as without it.
struct Ladder {
    int n = 0;
    mgpu_ls_window rung[MGPU_LADDER_MAX]{};
    MgpuLsRect win[MGPU_LADDER_MAX]{};              // rung r as the rectangular front-end takes it (frames = NULL)
    DevArray<double> weight[MGPU_LADDER_MAX];       // win[r].weight
    bool rung0_is_default = false;                  // rung 0 is the context's own square window: the default kernel runs it
    int kind[MGPU_LADDER_MAX]{};                    // MGPU_RUNG_LS / MGPU_RUNG_WIENER; a Wiener rung's `rung` is {0, 0} and its `win` carries no window
    mgpu_wiener_design design[MGPU_LADDER_MAX]{};   // of the Wiener rungs
    MgpuWiener wiener[MGPU_LADDER_MAX]{};           // a Wiener rung as its front-end takes it
    DevArray<double> wiener_A[MGPU_LADDER_MAX], wiener_B[MGPU_LADDER_MAX];
    DevArray<int> wiener_off[MGPU_LADDER_MAX];      // a_off, then b_off
    DevArray<uint16_t> wiener_idx[MGPU_LADDER_MAX]; // pilot, then col_list
    // a Wiener rung's bank (include/mercury_wiener_bank.h): with n > 0 wiener[r] reads these tables instead of wiener_A / wiener_B
    struct Bank {
        int n = 0;
        mgpu_wiener_bank_entry e[MGPU_WIENER_BANK_MAX]{};   // the thresholds as applied
        DevArray<double> A, B;                      // the designs' blocks one after the other
        DevArray<MgpuWienerBank> arg;               // wiener[r].bank: strides, pair lists, the entries' test constants
        DevArray<uint16_t> idx;                     // pair, then sym_first
        int n1 = 0, n2 = 0;
    } bank[MGPU_LADDER_MAX];
    DevArray<int> d_choice;                         // [max_batch] rung 0's choice per frame of the last call, by the frame's row
    DevArray<double> d_corr;                        // [max_batch][4] the sums it chose from
    DevArray<int> d_rung;                           // [max_batch] winning rung per frame of the last call, -1 = none
    DevArray<unsigned long long> d_counters;        // [MGPU_LADDER_MAX + 1] frames decoded by rung r; frames seen
    // a retry's compact workspaces, [max_batch] each, created with the first ladder of more than one rung
    DevArray<int> d_idx, d_count;
    DevArray<float> d_llr, d_var, d_snrvar;
    DevArray<double> d_meanh;
    DevArray<uint8_t> d_payload;
    DevArray<MgpuStatsDev> d_stats;
    Event done;                                     // behind the last retry: the next one, on whatever stream, waits for the workspaces
    bool done_recorded = false;
    int last_F = 0;                                 // frames of the last fused-span call
};

// Diversity combining (include/mercury_diversity.h; combine.hip): the decoder's compact rows of a grouped span, [max_batch] each, created
// with the first grouped call, and the device copy of a stand-alone combine's CSR.
struct Diversity {
    DevArray<float> d_llr;                          // [G][N] the groups' summed LLRs
    DevArray<uint8_t> d_payload;
    DevArray<MgpuStatsDev> d_stats;
    DevArray<int> d_csr;                            // first[G + 1], member[]
    Event done;                                     // behind the last user of the above: the next one, on whatever stream, waits for it
    bool done_recorded = false;
};

// The context's demapper (include/mercury_demapper.h; demapper.hip). MGPU_DEMAP_CSI: every front-end launch of the fused span is the CSI form.
struct Demapper {
    int mode = MGPU_DEMAP_MAXLOG;
    MgpuCsi arg{};
    DevArray<uint16_t> d_sym_data;                  // arg.sym_data; made with the first MGPU_DEMAP_CSI or MGPU_DEMAP_NMAP
    // MGPU_DEMAP_NMAP: every front-end launch of the fused span is a noise-map form (a CSI form with per-carrier and per-symbol noise factors)
    mgpu_demapper_params params{2.0, 1};            // as set; the defaults until then
    MgpuNmap nmap{};                                // lists, band, smooth; fc / fs / rows are set per launch
    DevArray<uint16_t> d_nmap_idx;                  // car_list, car_first, sym_first; made with the first MGPU_DEMAP_NMAP
    DevArray<double> d_fc, d_fs;                    // [max_batch][Nc], [max_batch][Nsymb] the factors of the last call's frames, by the frame's row
};

// The context's residual carrier-offset correction (include/mercury_cfo.h; cfo.hip). MGPU_CFO_PILOTS: every front-end launch of the fused span
// is a CFO form (with or without the channel-aware demapper).
struct Cfo {
    int mode = MGPU_CFO_OFF;
    MgpuCfo arg{};                                  // pair, first, Dy; step / step_rows are set per launch
    DevArray<uint16_t> d_pair, d_first;             // made with the first MGPU_CFO_PILOTS
    DevArray<double> d_step;                        // [max_batch] radians per symbol, by the frame's row in the context's workspaces
};

// The context's impulse blanker (include/mercury_blanker.h; blanker.hip). MGPU_BLANK_MEDIAN: the fused span starts with the blanker kernel and
// everything behind it reads the blanked frames in d_ws.
struct Blanker {
    int mode = MGPU_BLANK_OFF;
    mgpu_blanker_params params = MGPU_BLANKER_PARAMS_DEFAULT;   // as set; the defaults until then
    DevArray<double> d_ws;                          // [max_batch][frame_samples] c128 the blanked frames, by the frame's row; held while the mode is on
    DevArray<int> d_report;                         // [max_batch] {marked, blanked} of the last span's frames, by the frame's row
};

// The context's carrier excisor (include/ext/mercury_excisor.h; excisor.hip). MGPU_EXCISE_WELCH: receive_byte excises every capture window
// into its workspace (rxloop.hip) before the first filter reads it.
struct Excisor {
    int mode = MGPU_EXCISE_OFF;
    mgpu_excisor_params params = MGPU_EXCISOR_PARAMS_DEFAULT;   // as set; the defaults until then
    DevArray<double> d_tab, d_win;                  // the rule's tables, [1024][2] and [1024]; made with the first launch
    DevArray<double> d_spec;                        // [windows of a launch][B][3][64] the band bins' re, im and power per block; grows
    DevArray<mgpu_excisor_report> d_report;         // [max_batch] of the last receive_byte call's windows, by the window's row
    DevArray<mgpu_excisor_report> d_scratch;        // [kExciseWindows] the reports of a stand-alone call that wants none
};
constexpr int kExciseWindows = 64;                  // windows per launch: the spectrum workspace is that many windows' (18 MB in mode 8)
// a double's bits without its sign: the blanker's and the excisor's medians are selected on these keys (non-negative doubles order as them)
constexpr unsigned long long kKeyMask = 0x7fffffffffffffffull;

// The arrays one fused-span call (launch_span) reads and writes; row 0 = the call's first frame.
struct SpanIo {
    const double* bb = nullptr;         // input frames
    int frame_stride = 0;               // complex samples between consecutive frames of bb, 0 = the mode's frame_samples
    float *llr = nullptr, *var = nullptr, *snrvar = nullptr;
    uint8_t* payload = nullptr;
    MgpuStatsDev* stats = nullptr;
    double* mean_H = nullptr;           // the front-end's mean_H tap, which the ladder also merges (receive_byte's gate), or null
    double* zf_var = nullptr;           // zero-forcing modes: the argument of the SNR's logarithm per frame, or null
    int frame0 = 0;                     // row of the call's first frame in the context's max_batch-sized workspaces (d_eqdata, the ladder's d_rung)
    bool zf_snr = true;                 // false: no zero-forcing SNR launch (the baseband self-simulation's error counter does not read snr_db)
    int group = 0;                      // D >= 1: frames g*D .. g*D+D-1 are the branches of one transmitted frame, decoded from their summed LLRs; 0: every frame alone
};

struct Workspace;   // rxloop.hip
struct TxState;     // tx.hip
struct Release { void operator()(Workspace*) const; void operator()(TxState*) const; };   // defined where each type is complete

}  // namespace mgpu_detail
using namespace mgpu_detail;

struct mgpu_ctx {
    mgpu_config cfg{};
    mgpu::ModeTables tab;
    MgpuDev dev{};
    LdpcDev ldev{};
    std::vector<DevBuf> tables;     // the constant tables dev / ldev point into (keep())
    std::string err;
    int max_batch = 0;
    int numa_node = -1;             // the device's NUMA node (sysfs), -1 when the platform names none: page-locked staging is allocated there
    // Release order: mgpu_destroy drains the device before it deletes the context, so no work queued on the streams below (or on a
    // caller's stream with these buffers) is still running when the members are released; their order does not matter then.
    Stream stream;                  // private stream for the host-buffer entry points
    // workspaces (device)
    DevArray<double> d_baseband;    // lazily sized for the host-buffer entry points
    DevArray<float> d_llr, d_variance, d_snrvar;
    DevArray<uint8_t> d_payload;
    DevArray<MgpuStatsDev> d_stats;
    DevArray<uint8_t> d_bits;
    DevArray<double> d_eqdata;      // [max_batch][nData] c128, zero-forcing modes only (post-decode SNR)
    double* d_fir[2] = {nullptr, nullptr};   // FIR_rx_time_sync, FIR_rx_data taps (in tables)
    Event sync_ev[2];               // around the most recent synchroniser kernel
    float last_sync_ms = -1.f;
    DevArray<int> d_iters;
    // single-frame fast path of mgpu_rx_batch: the copy-in / front-end / decoder / copy-out sequence as one hipGraph
    struct OneFrame {
        GraphExec graph;
        DevArray<double> d_in;      // the graph's own one-frame device buffer (never reallocated: the graph holds its address)
        PinnedBuf h_in;             // page-locked staging for one frame of samples
        PinnedBuf h_out;            // page-locked staging for its payload + stats
    } one;
    std::unique_ptr<Workspace, Release> rxloop_ws;   // device workspace of mgpu_receive_byte_batch, kept between calls (rxloop.hip)
    int rxloop_ws_windows = 0;
    DevArray<double> rb_stage;      // mgpu_receive_byte_batch from host memory: landing area of the whole call's windows (uploaded by a helper thread)
    DevArray<char> rb_compact;      // mgpu_receive_byte_batch_samples: the windows as INT32 / INT16 / FLOAT32 samples, before the widening kernel
    Stream rb_stream;
    DevArray<double> d_mix_cs;      // receive mixer: cos / sin of the carrier phase per sample index (host libm) for mix_carrier
    double mix_carrier = -1;
    size_t mix_count = 0;
    std::unique_ptr<TxState, Release> tx_state;      // transmit path: preamble baseband, filter taps, carrier table (tx.hip)
    std::vector<double> pre_eq;     // [Nc][2] installed pre_equalization_channel (empty: none); dev.pre_eq is its device copy
    DevArray<double> d_pre_eq_buf;  // device copy of pre_eq
    Ladder lad;
    Diversity div;
    Demapper dmp;
    Cfo cfo;
    Blanker blk;
    Excisor exc;
    int pre_eq_version = 0;         // bumped by mgpu_set_pre_equalization_channel: the transmit state rebuilds its preamble
    struct Pipe { Stream stream; Event done, copied; DevArray<double> d_in; };
    // the blocking host-buffer entry points' chunk pipeline (rx_batch.hip rx_batch_pipelined)
    struct HostPath {
        static constexpr int kPipes = 2;
        Pipe pipe[kPipes];              // the two chunk pipelines
        PinnedBuf h_out;                // page-locked staging for the payloads + stats of a pipelined call ([max_batch])
        Event ev[4];                    // call start, first chunk copied, last chunk copied, all done (host-path profile)
        int chunk = 0, nchunks = 0;     // the last pipelined call: frames per chunk, chunks
        float fill_ms = 0, drain_ms = 0, total_ms = 0;
        int wave_of_wgs = 0;            // decoder workgroups that fill the device once (2 per compute unit); 0 = not asked yet
    } hp;
    // kernel timing (mgpu_enable_timing): named by launch.hip's two timed launchers and rx_batch.hip's queries only
    struct KernelTimes {
        static constexpr int kEvRing = 64;
        Event ev[kEvRing][4];           // per launch: front-end start/stop, decoder start/stop
        bool timing = false;
        int ev_count = 0;               // launches recorded since timing was enabled (ring of kEvRing)
        bool ev_fe[kEvRing]{};          // whether the front-end ran in that slot
    } kt;
    size_t lds_fe = 0, lds_dec = 0, lds_tx = 0;
    MgpuLsRect own_window{};        // the context's own square LS window as the front-end's rectangular forms take it (frames = NULL)
    int fe_threads = 512;           // front-end workgroup size: 1024 when the 512-thread carve is more than half a compute unit's LDS (no mode or golden geometry today: 1024 runs under MERCURY_FE_THREADS only)
    DecoderKernel spa_kernel = nullptr;
    int dec_threads = 1024;         // workgroup size of the decoder kernel

    template <typename T>
    T* keep(const std::vector<T>& v) { tables.push_back(upload(v)); return static_cast<T*>(tables.back().p); }
};


namespace mgpu_detail {

// Workspaces sized by max_batch are created on first use (create.hip)
enum : unsigned { WS_FRONTEND = 1, WS_LLR = 2, WS_OUT = 4, WS_BITS = 8 };
void ensure_workspaces(mgpu_ctx* c, unsigned what);

// HIP caps gridDim*blockDim below 2^32 threads, so very large batches go out in chunks of frames.
constexpr int kMaxFramesPerLaunch = 1 << 21;
template <typename Fn> void for_frame_chunks(int F, Fn&& fn) {      // fn(first frame, frames) per launch
    for (int off = 0; off < F; off += kMaxFramesPerLaunch) fn(off, F - off < kMaxFramesPerLaunch ? F - off : kMaxFramesPerLaunch);
}
template <typename T> T* at(T* p, size_t off) { return p ? p + off : nullptr; }

// whether the caller wants a tap with a row per frame (a launch's kernel writes them from row 0: one launch per call then)
inline bool wants_frame_taps(const MgpuTapsDev& t) { return t.grid || t.H || t.eq || t.syms || t.llr_demod || t.variance || t.agc_gain; }

// the context's own workspaces from frame `frame0` on (the caller sets bb, and whatever array is not the context's)
inline SpanIo own_span(mgpu_ctx* c, int frame0 = 0) {
    SpanIo io;
    io.llr = c->d_llr + size_t(frame0) * c->tab.N; io.var = c->d_variance + frame0; io.snrvar = c->d_snrvar + frame0;
    io.payload = c->d_payload + size_t(frame0) * c->tab.payload_stride; io.stats = c->d_stats + frame0;
    io.frame0 = frame0;
    return io;
}

// The fused span of the production receive path, on one stream: front-end, decoder, the estimator ladder's retries, zero-forcing SNR.
// taps: the stage taps of the front-end (rung 0's; mean_H comes from io). input_free, when given, is recorded behind the last launch that
// reads io.bb: the front-end, or the ladder where a retry can read the frames again.
void launch_span(mgpu_ctx* c, const SpanIo& io, int F, const MgpuTapsDev& taps, hipStream_t s, hipEvent_t input_free = nullptr);
// The halves of the span, timed when mgpu_enable_timing is on (launch.hip). The front-end reads io.bb and writes llr, var, snrvar, mean_H.
void launch_frontend(mgpu_ctx* c, const SpanIo& io, int F, const MgpuTapsDev& taps, hipStream_t s);
void launch_decoder(mgpu_ctx* c, const float* d_llr, int F, uint8_t* d_bits, int* d_iters, uint8_t* d_payload, MgpuStatsDev* d_stats,
                    const float* d_var, const float* d_snrvar, hipStream_t s);
// The same launches without the timing events, as the ladder's retries run them: the kernel timings describe rung 0.
// rect: null = rung 0 (the ladder's first window where it is not the context's own, else the context's own); a retry's window otherwise,
// whose `frames` list names the frame each row of the compact outputs in io belongs to. rung: the ladder's rung the launch is (0 without a
// ladder). The launch's form (ls_rect.h) follows from the context: WIENER from the rung's kind, which the ladder keeps, CSI and NMAP from the
// demapper, CFO from the carrier-offset setting, RECT with any of them or a window other than the context's own.
void frontend_untimed(mgpu_ctx* c, const SpanIo& io, int F, const MgpuTapsDev& taps, const MgpuLsRect* rect, hipStream_t s, int rung = 0);
// Lets every form's kernel of the context's workgroup size use its whole LDS carve (a BPSK geometry's exceeds the default limit). The setter
// of each option calls it, so that no setter has to know the forms its option makes with the others. 13 hipFuncSetAttribute calls
// on every such call of a setter, where each setter used to make one to four on its first: idempotent, and setters are not on the receive path.
void frontend_raise_lds_limits(mgpu_ctx* c);
void decoder_untimed(mgpu_ctx* c, const float* d_llr, int F, uint8_t* d_bits, int* d_iters, uint8_t* d_payload, MgpuStatsDev* d_stats,
                     const float* d_var, const float* d_snrvar, hipStream_t s);
// The estimator ladder behind rung 0 (ladder.hip), called by launch_span alone: marks each frame's rung and, rung by rung, re-runs the
// frames still undecoded and merges the ones that decode. Nothing without a ladder. Waits for the stream once per rung (the retry's frame count).
void launch_ladder(mgpu_ctx* c, const SpanIo& io, int F, hipStream_t s);
void launch_zf_snr(mgpu_ctx* c, const SpanIo& io, int F, hipStream_t s);
// The impulse blanker (blanker.hip): F frames, in_stride complex samples apart in d_in, into the dense d_out (and their reports, if wanted),
// with the context's parameters. blanked_span: the head of a fused span with the stage on - the blanker on io.bb into the context's workspace
// rows from io.frame0, input_free (if given) recorded right behind it - and the SpanIo the rest of the span runs on.
void launch_blanker(mgpu_ctx* c, const double* d_in, int F, size_t in_stride, double* d_out, int* d_report, hipStream_t s);
SpanIo blanked_span(mgpu_ctx* c, const SpanIo& io, int F, hipStream_t s, hipEvent_t input_free);
// The carrier excisor (excisor.hip): W dense windows of n samples from d_in into d_out and their reports into d_report (null: none), with the
// context's parameters, on stream s. release_excised_windows (rxloop.hip) frees receive_byte's workspace of cleaned windows.
void launch_excisor(mgpu_ctx* c, const double* d_in, int W, int n, double carrier_hz, double* d_out, mgpu_excisor_report* d_report, hipStream_t s);
void release_excised_windows(mgpu_ctx* c);
// The grouped span's own steps (combine.hip): the context's compact rows, made on first use; the sums of G groups of member rows (uniform
// groups of D when d_first is null, else the CSR on the device) into d_out; the groups' decode back to the F rows of io.
void diversity_workspaces(mgpu_ctx* c);
void launch_llr_combine(const float* d_llr, int D, const int* d_first, const int* d_member, int G, float* d_out, hipStream_t s);
void launch_group_scatter(mgpu_ctx* c, const SpanIo& io, int F, int D, hipStream_t s);
// mgpu_explicit_params as the table builder takes them; false (and *rc, err) when they are refused (create.hip)
bool explicit_params_from(const mgpu_explicit_params* in, mgpu::ExplicitParams& xp, std::string& err, int* rc);
// F generated frames from frame0 on into d_bb (and their payloads into d_payload, if given). channel -1: the transmit path's clean frames,
// whose payloads come from tx_payload (frames tx_stride bytes apart, d_nbytes of each in use) instead of the generator
void launch_txgen(mgpu_ctx* c, uint64_t seed, uint64_t frame0, int F, double noise_amp, int channel, double* d_bb, uint8_t* d_payload, hipStream_t s,
                  const uint8_t* tx_payload = nullptr, int tx_stride = 0, const int* d_nbytes = nullptr);

// the scalar half of cl_ofdm::time_sync_mfsk (ofdm.cc:2004-2060) on the slot energies of one window ([nslots][Nc])
int mfsk_sync_from_energies(const mgpu::ModeTables& t, const double* E, int nslots, int size, int search_start_symb);
void launch_mfsk_sync(mgpu_ctx* c, const double* d_energy, int W, int nslots, int size, const int* d_search_start, int* d_delay, hipStream_t s);
// passband_to_baseband launch for nwin windows (grid y) of `count` outputs each: the sliding-tap kernels for the reference's 33-tap filters
// at decimation 1 / 4, the generic kernel otherwise (launch.hip)
void launch_p2b(const double* passband, int in_size, const double* d_carrier, const int* d_start, int start_all, int count, int decim, const double* d_taps,
                int ntaps, double* out, const int* widx, const double* cs, const int* out_row, int row_by_launch, int nwin, hipStream_t s);
// the reference's peak selection (ofdm.cc:1943-1964): overwrite-not-swap partial sort over an array of `size` entries that
// holds the metric of candidate k at index k*step and 0 elsewhere; returns the index (delay) and value of entry
// `location_to_return` after nTrials_max passes
void select_peak(const double* cand_vals, int ncand, int step, int size, int location_to_return, int nTrials_max, int* delay, double* corr);

// carrier_sampling_frequency_sync's last step (ofdm.cc:594 with get_angle, misc.cc:34-56) on the sum the Moose kernel returns
inline double moose_hz(double re, double im, double carrier_freq_width) {
    double theta = 0;
    if (re == 0) theta = M_PI / 2;
    else if (re > 0) theta = std::atan(im / re);
    else if (re < 0 && im >= 0) theta = std::atan(im / re) + M_PI;
    else if (re < 0 && im < 0) theta = std::atan(im / re) - M_PI;
    return (theta / M_PI) * carrier_freq_width;
}

// cos / sin table of the receive mixer for `carrier_hz`, at least `count` samples long (built on the host with the reference's libm call,
// cached in the context); the stream is synchronised when the table has to be rebuilt
const double* mixer_table(mgpu_ctx* c, double carrier_hz, size_t count, hipStream_t s);

// Watterson HF channel (hfchannel.hip, include/mercury_channel.h): validation (std::invalid_argument) and the fused kernels of the two
// self-simulations. Passband: the capture windows of mgpu_passband_channel_kernel through the channel at 48 kHz before the same noise;
// baseband: the generator's clean 12 kHz frames through the channel before the generator's own noise. Realisation = frame number.
void hf_check(const mgpu_hf_channel* ch);
void launch_hf_passband(const mgpu_hf_channel* ch, const double* d_audio, int total, int delay, int window, double ampl, uint64_t seed,
                        uint64_t frame0, int F, double* d_out, hipStream_t s);
void launch_hf_baseband(const mgpu_hf_channel* ch, const double* d_clean, int n, double noise_amp, uint64_t seed, uint64_t frame0, int F,
                        double* d_out, hipStream_t s);

// Schmidl-Cox metrics of n windows (sync.hip): picks the kernel for the step and the segment lengths.
// d_start / d_widx / d_ncand may be null (search from sample 0, window k = k, ncand_max candidates each).
void launch_tsync_metric(const double* d_bb, int stride, const int* d_start, const int* d_widx, const int* d_ncand, int ncand_max, int n, int step,
                         int pre_nsymb, int ngi_i, int nfft_i, double* d_vals, hipStream_t s, int variant = -1);

// Every entry point that takes a context runs with the context's device current and puts the caller's device back
// afterwards, so one host thread can hold contexts on several GPUs (lazy workspaces, per-call buffers, page-locked
// staging and launches on c->stream all land on cfg.device, whatever the thread's current device was).
struct DeviceScope {
    int prev = -1, want = -1;
    explicit DeviceScope(int device) : want(device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != want) HIPCK(hipSetDevice(want));
    }
    ~DeviceScope() { if (prev >= 0 && prev != want) (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

inline int guard(mgpu_ctx* c, const std::function<void()>& fn) {
    try {
        if (c) {
            DeviceScope on(c->cfg.device);
            fn();
        } else {
            fn();
        }
        return MGPU_OK;
    } catch (const HipError& e) {
        if (c) c->err = e.what();
        return MGPU_ERR_DEVICE;
    } catch (const std::invalid_argument& e) {
        if (c) c->err = e.what();
        return MGPU_ERR_ARG;
    } catch (const std::exception& e) {
        if (c) c->err = e.what();
        return MGPU_ERR_DEVICE;
    }
}
inline void need(bool ok, const char* what) { if (!ok) throw std::invalid_argument(what); }
// a refusal before any device work: the message where mgpu_last_error finds it, and the code to return
inline int refuse(mgpu_ctx* c, int code, const char* message) { c->err = message; return code; }
// the stream a *_dev entry point works on: the caller's, or the context's own where it names none
inline hipStream_t stream_or_own(mgpu_ctx* c, void* stream) { return stream ? static_cast<hipStream_t>(stream) : c->stream.h; }
// the event arguments of mgpu_capture_run and of the entry points that end in it
inline void check_event_args(const void* events, int max_events, const int* n_events) {
    need(n_events != nullptr && max_events >= 0 && (max_events == 0 || events), "bad argument (n_events, events)");
}
// Rows [first, first + count) of an array the last call left on the device, one row of `per_row` elements per frame (or window) of
// max_batch, into dst (null: not wanted). never_set: the message where the array was never made.
template <typename T>
void read_rows(mgpu_ctx* c, const DevArray<T>& d, size_t per_row, int first, int count, void* dst, const char* never_set) {
    need(size_t(first) + size_t(count) <= size_t(c->max_batch), "bad argument (first + count must be <= max_batch)");
    need(bool(d.p), never_set);
    HIPCK(hipStreamSynchronize(c->stream));
    if (count && dst) HIPCK(hipMemcpy(dst, d + size_t(first) * per_row, size_t(count) * per_row * sizeof(T), hipMemcpyDeviceToHost));
}
// A host twin has no context to leave a message in: fn's own code, or MGPU_ERR_ARG where it throws
template <typename Fn> int host_try(Fn&& fn) {
    try {
        return fn();
    } catch (const std::exception&) { return MGPU_ERR_ARG; }
}
// ... on a mode's geometry: fn(the caller's explicit parameters as the table builder takes them), or the code they are refused with
template <typename Fn> int host_twin(const mgpu_explicit_params* p, Fn&& fn) {
    mgpu::ExplicitParams xp;
    std::string err;
    int rc = MGPU_OK;
    if (!explicit_params_from(p, xp, err, &rc)) return rc;
    return host_try([&] { return fn(xp); });
}
// mfsk.cc:82-95, :120-126, :149-155; the universal ACK/BREAK patterns use M = 16, one stream centred in Nc = 50
// (telecom_system.cc:3006), hop step 7, 8 tones sent twice.
constexpr int kAckTones[8] = {4, 7, 5, 12, 13, 1, 9, 15}, kBreakTones[8] = {6, 14, 2, 3, 10, 8, 11, 15};
constexpr int kAckM = 16, kAckNsymb = 16, kAckLen = 8, kAckHop = 7, kAckOffset = 17;
constexpr int kInterp = 4;                       // frequency_interpolation_rate, physical_config.cc:79
constexpr double kSampleRate = 48000.0;          // telecom_system.cc:1569
constexpr double kBandwidthHz = kSampleRate * 50.0 / 256 / 4;     // physical_config.cc:81, in its order
constexpr double kCarrierAmplitude = 1.4142135623730951;   // sqrt(2.0), telecom_system.cc:69

// run `launch(d_in..., d_out)` between an upload of the inputs and a download of the outputs on the context's stream
struct Io {
    mgpu_ctx* c;
    hipStream_t s;
    explicit Io(mgpu_ctx* ctx) : c(ctx), s(ctx->stream) {}
    void up(DevBuf& d, const void* h, size_t bytes) { HIPCK(hipMemcpyAsync(d.p, h, bytes, hipMemcpyHostToDevice, s)); }
    void back(void* h, DevBuf& d, size_t bytes) { HIPCK(hipMemcpyAsync(h, d.p, bytes, hipMemcpyDeviceToHost, s)); }
    void down(void* h, DevBuf& d, size_t bytes) { back(h, d, bytes); HIPCK(hipStreamSynchronize(s)); }      // the last output: waited for
};

inline bool is_device_memory(const void* p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeDevice) return true;
    (void)hipGetLastError();
    return false;
}
// A caller's input where the kernels can read it: device memory as it is, host memory through the staging buffer (grown), once the
// stream's earlier reads of that buffer are over
inline const void* staged_on_device(DevArray<char>& stage, const void* in, size_t bytes, hipStream_t st) {
    if (is_device_memory(in)) return in;
    HIPCK(hipStreamSynchronize(st));
    stage.grow(bytes);
    HIPCK(hipMemcpyAsync(stage.p, in, bytes, hipMemcpyHostToDevice, st));
    return stage.p;
}

// receive_byte for W windows in host or device memory, on the context's stream (rxloop.hip)
// row0: the row of the call's first window in the arrays kept by window row (the excisor's reports): a piece of a pipelined call
void receive_byte_impl(mgpu_ctx* c, const double* passband, int W, const mgpu_receive_config* rcp, mgpu_link_state* state, uint8_t* payload,
                       mgpu_receive_stats* stats, int row0 = 0);
// Per-component noise amplitude of the audio-path simulations at esn0_db (selfsim.hip): OFDM from Es/N0 alone, MFSK calibrated from the mean
// power of the first transmitted frame
double audio_noise_amplitude(const mgpu::ModeTables& t, double esn0_db, double mean_power);

}  // namespace mgpu_detail

// what the feeders in front of a capture (capture.hip) hold against their own: the number of its captures,
struct mgpu_capture;
struct mgpu_capture_geometry;
int capture_streams(mgpu_capture* cap);
// and whether a stage of context c with S streams can feed the capture: its geometry (into *g) is readable, it has S captures and it was made
// on c, so that its kernels run on the stream of the stage's, behind them
bool capture_pairs(mgpu_capture* cap, mgpu_ctx* c, int S, mgpu_capture_geometry* g);

// What the front-end's opt-in forms (frontend.hip) take beyond MgpuDev (device_tables.h), which stays what the plain form and the decoder
// are built from: a struct per option, the form bits, and the one kernel argument MgpuFeOpt that carries the structs.
//
// One LS estimator window of its own width and height (include/mercury_estimator.h) as the front-end's rectangular
// instantiation takes it, and the frame list of a ladder retry (ladder.hip).
#pragma once
#include <stdint.h>

struct MgpuLsRect {
    const double* weight;   // [width*height+1] boost / sum_n(boost^2) per window population n (tables.cpp ls_weight_table)
    const int* frames;      // workgroup b reads frame frames[b] and writes row b of compact outputs; NULL: frame b
    int hw_f, hw_t;         // half-widths: frequency (columns) and time (rows)
    int lattice;            // MgpuDev::regular_lattice evaluated for this width: 2 = every clipped window row holds >= 3 pilots of each column residue
};

// What the channel-aware demapper's front-end (frontend.hip CSI; include/mercury_demapper.h) needs beyond MgpuDev, again an argument of its own.
struct MgpuCsi {
    const uint16_t* sym_data;   // [nData] de-framed position of the cell MgpuDev::sym_src[k] names: where that cell's |h|^2 is kept
};

// What the pilot-aided residual carrier-offset stage (frontend.hip CFO; include/mercury_cfo.h) needs beyond MgpuDev, again an argument of
// its own; made at mgpu_set_cfo (cfo.hip).
struct MgpuCfo {
    const uint16_t* pair;   // [pairs][2] earlier and later cell of every same-carrier pilot pair Dy symbols apart: carrier after carrier, ascending symbols
    const uint16_t* first;  // [Nc + 1] a carrier's first pair; first[Nc] = pairs
    double* step;           // row of the launch's first frame in the context's step array, or null
    int step_rows;          // rows of `step` that may be written
    int Dy;
};

// What the separable Wiener estimator (frontend.hip WIENER; include/mercury_estimator.h MGPU_RUNG_WIENER) needs beyond MgpuDev, again an
// argument of its own; made at mgpu_set_estimator_ladder_ex (ladder.hip) from wiener_tables.cpp's tables. The matrices stay in global
// memory: a few per mode, shared by every workgroup.
struct MgpuWienerBank;
struct MgpuWiener {
    const double* A;            // the time classes' matrices one after the other, each row-major n x n
    const double* B;            // the frequency classes' matrices one after the other, each row-major n x n complex (re, im)
    const int* a_off;           // [time classes] a class's first double in A
    const int* b_off;           // [frequency classes] a class's first complex in B
    const uint16_t* pilot;      // [nPilots][8] time class, row in it, its size n, first entry of the carrier's list in col_list;
                                //              frequency class, row in it, its size n, the symbol's first pilot (a symbol's pilots are consecutive)
    const uint16_t* col_list;   // every carrier's pilots in ascending symbols, carrier after carrier
    // A bank of designs (include/mercury_wiener_bank.h; made at mgpu_set_wiener_bank): the workgroup chooses one per frame. The class
    // structure depends on the geometry alone, so a_off, b_off, pilot and col_list above are the same for every design.
    int n_designs;              // 0 or 1: A and B are the one design's and nothing below is read
    int rows;                   // rows of choice / corr that may be written
    const MgpuWienerBank* bank; // in device memory: what only the choice reads stays out of the kernel's arguments
    int* choice;                // row of the launch's first frame in the context's arrays, or null (a retry, a rung behind rung 0)
    double* corr;               // [rows][4] R1r R1i R2r R2i
};
struct MgpuWienerBank {
    int a_stride, b_stride;     // from one design's block to the next: doubles in A, complex in B
    const uint16_t* pair;       // [nPilots] bit 0: pilots p and p + 1 are a 1-pair, bit 1: p and p + 2 are a 2-pair
    const uint16_t* sym_first;  // [Nsymb + 1] a symbol's first pilot in pilot order; sym_first[Nsymb] = nPilots
    double n1sq, n2sq;          // double(n1) double(n1), double(n2) double(n2)
    double sel[3][4];           // per entry but the last: rho_min^2, u.re, u.im, t (< 0: no centroid test)
};

// What the noise-map demapper's front-end (frontend.hip NMAP; include/mercury_demapper.h MGPU_DEMAP_NMAP) needs beyond MgpuDev and MgpuCsi,
// again an argument of its own; made at mgpu_set_demapper_ex (demapper.hip).
struct MgpuNmap {
    const uint16_t* car_list;   // every carrier's pilots as indices into pilot order, in ascending symbols, carrier after carrier
    const uint16_t* car_first;  // [Nc + 1] a carrier's first entry in car_list; car_first[Nc] = nPilots
    const uint16_t* sym_first;  // [Nsymb + 1] a symbol's first pilot in pilot order (its pilots are consecutive); sym_first[Nsymb] = nPilots
    double band;                // the dead band, >= 1 (+Inf: no factor ever leaves it)
    double* fc;                 // [rows][Nc] row of the launch's first frame in the context's factor arrays, or null
    double* fs;                 // [rows][Nsymb]
    int rows;                   // rows of fc / fs that may be written
    int smooth;                 // carriers on either side that share a carrier's mean, 0..4
};

// A front-end form (frontend.hip): which of the options above the one body fe_frame is built with, as a bit set. Any option implies RECT and
// NMAP implies CSI, which leaves 13 forms: the plain one, RECT with any of CSI, CFO and WIENER, RECT | CSI | NMAP with any of CFO and WIENER.
enum : unsigned { MGPU_FE_RECT = 1, MGPU_FE_CSI = 2, MGPU_FE_CFO = 4, MGPU_FE_WIENER = 8, MGPU_FE_NMAP = 16, MGPU_FE_FORMS = 32 };
constexpr bool mgpu_fe_form_valid(unsigned form) {
    return form < MGPU_FE_FORMS && (form == 0 || (form & MGPU_FE_RECT)) && (!(form & MGPU_FE_NMAP) || (form & MGPU_FE_CSI));
}

// The options' arguments, the last argument of every front-end kernel. A form reads the members its bits name and no other.
// (In this order every kernel keeps the registers, scratch and occupancy it had with arguments of its own, and all but one no more
// instructions inside loops: profiles/frontend_forms.md.)
struct MgpuFeOpt {
    MgpuLsRect win;
    MgpuNmap nm;
    MgpuWiener wn;
    MgpuCfo cfo;
    MgpuCsi csi;
};

// The band scanner's transform as scanner.hip's block kernel schedules it (include/ext/mercury_scanner.h has the rule). Host and device
// code: the kernel runs these functions one group per thread between barriers, tests/cpp/scanner_sanitize.cpp runs them group after
// group on the CPU and holds the schedule to the rule's loop nest.
//
// The data stay in natural order, as fft256.h and excisor.hip keep them: element idx of the rule's array a lives at position
// p = brev(idx), so position i starts as v[i], stage st (size 2^st) pairs positions 2^(L - st) apart, the member with that bit clear is
// the rule's lo, and the twiddle's index is (brev(p) & (2^(st-1) - 1)) << (L - st). Same operands, same operations, same twiddles: the
// rule's bits. A group is four positions q apart and runs two stages (pairs 2 q apart, then q apart) between exchanges, q = 4^r counted
// from the last round; with L odd, stage 1 runs alone first.
//
// Where a position lies in the work array (scan_entry): its low four bits, the 16-byte column of a 256-byte LDS row, are turned by its
// bits 4..7 and 8..11. Sixteen lanes of one LDS access then touch sixteen different columns in every round:
//   q >= 16  lanes take consecutive positions, the turning bits are the same for an aligned run of 16;
//   q = 4    a group is o + 4 k in a 16-block B; lanes vary o and B's bits 2, 3: column bits (o ^ B01, k ^ B23), B01 fixed;
//   q = 1    a group is 4 g + k; lanes vary g's four low bits = position bits 2..5: column bits (k ^ p45, p23 ^ p67), p67 fixed;
//   the power read, lane f -> position brev(f + N/2): the lanes' four low bits are the position's four top bits, which turn the column.
// scan_group_base is the lane-to-group map that makes the two short rounds so.
#pragma once

#ifdef __HIPCC__
#define SCAN_FN __host__ __device__ inline
#else
#define SCAN_FN inline
#endif

struct sc2 { double re, im; };

SCAN_FN int scan_entry(int p) { return p ^ (((p >> 4) ^ (p >> 8)) & 15); }

SCAN_FN int scan_brev(int p, int L) {
#ifdef __HIP_DEVICE_COMPILE__
    return int(__builtin_bitreverse32(unsigned(p)) >> (32 - L));
#else
    int r = 0;
    for (int b = 0; b < L; ++b) r |= ((p >> b) & 1) << (L - 1 - b);
    return r;
#endif
}

// lo, hi <- lo + w hi, lo - w hi with w = conj(tab[idx]): the rule's butterfly
SCAN_FN void scan_bfly(sc2& lo, sc2& hi, const sc2* __restrict__ tab, int idx) {
    const sc2 e = tab[idx];
    const sc2 w = {e.re, -e.im};
    const sc2 t = {w.re * hi.re - w.im * hi.im, w.re * hi.im + w.im * hi.re};
    const sc2 u = lo;
    hi = {u.re - t.re, u.im - t.im};
    lo = {u.re + t.re, u.im + t.im};
}

// the twiddle's index of stage st for the pair whose lo lies at position p
SCAN_FN int scan_twiddle(int p, int st, int L) { return (scan_brev(p, L) & ((1 << (st - 1)) - 1)) << (L - st); }

// the first position of group u (u < N / 4) of a round whose positions are q apart
SCAN_FN int scan_group_base(int u, int q) {
    if (q >= 16) return (u / q) * 4 * q + (u % q);
    if (q == 4) return (u & 3) | (((u >> 4) & 3) << 4) | (((u >> 2) & 3) << 6) | ((u >> 6) << 8);
    return u << 2;
}

template <int L>
struct ScanFft {
    static constexpr int N = 1 << L, H = N / 2;
    static constexpr int kThreads = N / 4 < 256 ? N / 4 : 256;
    static constexpr int kRounds = L / 2;
    static constexpr int kFirst = (L & 1) ? 2 : 1;              // the first stage that runs in a round

    // L odd: stage 1 for pair u (u < N / 2) from the windowed samples into the work array
    template <typename Fetch>
    static SCAN_FN void single(int u, sc2* __restrict__ s, const sc2* __restrict__ tab, Fetch&& fetch) {
        sc2 lo = fetch(u), hi = fetch(u + H);
        scan_bfly(lo, hi, tab, 0);
        s[scan_entry(u)] = lo;
        s[scan_entry(u + H)] = hi;
    }

    // round r (0 .. kRounds - 1) for group u: stages st = kFirst + 2 r and st + 1. from_samples: the round reads the windowed samples
    // (round 0 with L even), not the work array
    template <typename Fetch>
    static SCAN_FN void round(int r, int u, sc2* __restrict__ s, const sc2* __restrict__ tab, bool from_samples, Fetch&& fetch) {
        const int st = kFirst + 2 * r, q = 1 << (L - st - 1), p0 = scan_group_base(u, q);
        sc2 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = from_samples ? fetch(p0 + k * q) : s[scan_entry(p0 + k * q)];
        const int w0 = scan_twiddle(p0, st, L);
        scan_bfly(v[0], v[2], tab, w0);
        scan_bfly(v[1], v[3], tab, w0);
        scan_bfly(v[0], v[1], tab, scan_twiddle(p0, st + 1, L));
        scan_bfly(v[2], v[3], tab, scan_twiddle(p0 + 2 * q, st + 1, L));
#pragma unroll
        for (int k = 0; k < 4; ++k) s[scan_entry(p0 + k * q)] = v[k];
    }

    // P[f] of the finished work array
    static SCAN_FN double power(int f, const sc2* __restrict__ s) {
        const sc2 v = s[scan_entry(scan_brev((f + H) & (N - 1), L))];
        return v.re * v.re + v.im * v.im;
    }
};

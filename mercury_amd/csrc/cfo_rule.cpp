// The arithmetic of the residual carrier-offset rule (include/mercury_cfo.h) on the host: the normative statement behind
// mgpu_host_cfo_pilots (cfo.hip). A translation unit of its own because it is plain C++: glibc_trig.h compiles for the host here, so the
// twin's atan and sincos are the restatement the kernel runs (frontend.hip), whatever libm the host has. Built with -ffp-contract=off.
#include <math.h>
#include <stdint.h>

#include "glibc_trig.h"

namespace {
// get_angle (misc.cc:34-56), as fe_math.h states it for the device
double get_angle_host(double re, double im) {
    const double a = gl_atan(im / re);
    double theta = 0;
    if (re == 0) theta = M_PI / 2;
    else if (re > 0) theta = a;
    else if (re < 0 && im >= 0) theta = a + M_PI;
    else if (re < 0 && im < 0) theta = a - M_PI;
    return theta;
}
}  // namespace

// grid / out: [Ns * Nc] complex128 (out may be grid); sign: [Ns * Nc] 0 data, +1 / -1 pilot; pair / first: MgpuCfo's tables (ls_rect.h)
extern "C" void mgpu_internal_cfo_rule(const double* grid, double* out, int Ns, int Nc, int Dy, const int8_t* sign, const uint16_t* pair,
                                       const uint16_t* first, double* step_out) {
    double rr = 0, ri = 0;
    for (int c = 0; c < Nc; ++c) {
        double ar = 0, ai = 0;
        for (int q = first[c]; q < first[c + 1]; ++q) {
            const int q0 = pair[2 * q], q1 = pair[2 * q + 1];
            double z0r = grid[2 * q0], z0i = grid[2 * q0 + 1], z1r = grid[2 * q1], z1i = grid[2 * q1 + 1];
            if (sign[q0] < 0) { z0r = -z0r; z0i = -z0i; }
            if (sign[q1] < 0) { z1r = -z1r; z1i = -z1i; }
            ar += z1r * z0r + z1i * z0i;
            ai += z1i * z0r - z1r * z0i;
        }
        rr += ar;
        ri += ai;
    }
    const bool ok = fabs(rr) < INFINITY && fabs(ri) < INFINITY && !(rr == 0 && ri == 0);
    const double step = ok ? get_angle_host(rr, ri) / double(Dy) : 0.0;
    if (step_out) *step_out = step;
    for (int s = 0; s < Ns; ++s) {
        double sn = 0, cs = 1;
        if (ok) gl_sincos(-step * double(s), &sn, &cs);
        for (int c = s * Nc; c < (s + 1) * Nc; ++c) {
            const double gr = grid[2 * c], gi = grid[2 * c + 1];
            if (ok) { out[2 * c] = gr * cs - gi * sn; out[2 * c + 1] = gr * sn + gi * cs; }
            else { out[2 * c] = gr; out[2 * c + 1] = gi; }
        }
    }
}

// The sample formats the library widens to double, stated once for host and device code: the audio device's real formats (mercury_rxloop.h
// MGPU_SAMPLES_*, the capture thread's widening, audioio.c:893-936) and the SDR's IQ formats (mercury_channelizer.h MGPU_IQ_*) each name one
// of four element types. An integer element is converted to double and divided by its divisor (INT32 / INT_MAX :909, INT16 / 32768.0 :907),
// a float is converted (:905), a double is read as it lies. int -> double is exact and the division is the IEEE-754 correctly rounded one
// on the host and on the device, so both sides get the same doubles bit for bit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "../../include/mercury_channelizer.h"
#include "../../include/mercury_rxloop.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MGPU_FMT_FN __host__ __device__ inline
#else
#define MGPU_FMT_FN inline
#endif

namespace mgpu_fmt {

enum Element { kNone = -1, kF64 = 0, kI32 = 1, kI16 = 2, kF32 = 3 };

// the element type of a format: one component = MGPU_SAMPLES_*, two = MGPU_IQ_*; kNone where the format does not fit the components
MGPU_FMT_FN int element(int components, int format) {
    if (components == 1)
        return format == MGPU_SAMPLES_F64 ? kF64 : format == MGPU_SAMPLES_INT32 ? kI32 : format == MGPU_SAMPLES_INT16 ? kI16 : format == MGPU_SAMPLES_F32 ? kF32 : kNone;
    if (components == 2) return format == MGPU_IQ_CS16 ? kI16 : format == MGPU_IQ_CF32 ? kF32 : format == MGPU_IQ_CF64 ? kF64 : kNone;
    return kNone;
}
MGPU_FMT_FN size_t element_bytes(int e) { return e == kF64 ? 8 : e == kI16 ? 2 : e == kNone ? 0 : 4; }

// the one widening expression (a division by 1.0 is exact: either branch serves a float or a double)
template <typename T> MGPU_FMT_FN double widen(T x, double divisor) { return divisor == 1.0 ? double(x) : double(x) / divisor; }

// fn(the samples as their element type, that type's divisor); what is none of the four reads as doubles
template <typename Fn> MGPU_FMT_FN auto with_elements(int e, const void* samples, Fn&& fn) {
    switch (e) {
        case kI32: return fn(static_cast<const int32_t*>(samples), 2147483647.0);
        case kI16: return fn(static_cast<const int16_t*>(samples), 32768.0);
        case kF32: return fn(static_cast<const float*>(samples), 1.0);
        default: return fn(static_cast<const double*>(samples), 1.0);
    }
}
// element i of the samples, widened
MGPU_FMT_FN double widen_at(int e, const void* samples, size_t i) {
    return with_elements(e, samples, [i](auto* in, double divisor) { return widen(in[i], divisor); });
}

// The IQ formats in both directions. The bytes of one IQ sample; 0: no such format
MGPU_FMT_FN size_t iq_bytes(int format) { return format == MGPU_IQ_CS16 ? 4 : format == MGPU_IQ_CF32 ? 8 : format == MGPU_IQ_CF64 ? 16 : 0; }

#ifdef __HIPCC__
// IQ sample g of a buffer in `format`, widened: one 4-, 8- or 16-byte load. A chain on the format itself: going through element() and
// with_elements() made the channeliser's assemble kernel longer and slower (profiles/stage_plumbing.md)
__device__ inline double2 load_iq(const void* iq, int format, size_t g) {
    if (format == MGPU_IQ_CS16) {
        const short2 v = static_cast<const short2*>(iq)[g];
        return make_double2(widen(v.x, 32768.0), widen(v.y, 32768.0));
    }
    if (format == MGPU_IQ_CF32) {
        const float2 v = static_cast<const float2*>(iq)[g];
        return make_double2(widen(v.x, 1.0), widen(v.y, 1.0));
    }
    return static_cast<const double2*>(iq)[g];
}
#endif

// one component as CS16: clamp(nearbyint(x * 32768), -32768, 32767); *clamped += 1 where it was clamped (a NaN becomes 0 and counts)
MGPU_FMT_FN int16_t to_cs16(double x, unsigned* clamped) {
    const double y = rint(x * 32768.0);
    if (y > 32767.0) { ++*clamped; return 32767; }
    if (y < -32768.0) { ++*clamped; return -32768; }
    if (y != y) { ++*clamped; return 0; }
    return int16_t(int(y));
}
// IQ sample m of `out` in `format`; returns the components clamped
MGPU_FMT_FN unsigned store_iq(void* out, int format, size_t m, double re, double im) {
    unsigned clamped = 0;
    if (format == MGPU_IQ_CS16) {
        int16_t* o = static_cast<int16_t*>(out) + 2 * m;
        o[0] = to_cs16(re, &clamped);
        o[1] = to_cs16(im, &clamped);
    } else if (format == MGPU_IQ_CF32) {
        float* o = static_cast<float*>(out) + 2 * m;
        o[0] = float(re);
        o[1] = float(im);
    } else {
        double* o = static_cast<double*>(out) + 2 * m;
        o[0] = re;
        o[1] = im;
    }
    return clamped;
}

}  // namespace mgpu_fmt

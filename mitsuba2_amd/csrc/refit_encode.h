// refit_encode.h -- the box encodings of bvh.cpp's emission, restated per box for the device refit (refit.hip).  The requirement is byte
// identity with emit_bvh, not "conservative enough": every expression keeps the host's operand order (the build has -ffp-contract=off),
// the arithmetic is double where the host's is, and what the host does with nextafter / frexp / ldexp is done on the bits.  The
// functions compile for the host too, where tests/refit_driver.cpp holds them against the arrays emit_bvh wrote.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define MTS_ENC __host__ __device__ inline
#else
#define MTS_ENC inline
#endif

namespace mtsamd {

// what the emission derives from the scene box: `extent` of padded() and the quantisation grid as the device decodes it
struct RefitGrid {
    double extent;
    double glo[3], gstep[3];      // (double) of the float q_lo / q_step
};

MTS_ENC uint32_t enc_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
MTS_ENC float enc_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// std::min / std::max, operand for operand (the first wins a tie, which decides the sign of a zero): the host refit and the device use
// these in the same order, so their boxes agree to the bit
MTS_ENC float enc_min(float a, float b) { return b < a ? b : a; }
MTS_ENC float enc_max(float a, float b) { return a < b ? b : a; }

// std::nextafter(x, -INFINITY) / (x, +INFINITY)
MTS_ENC float enc_next_down(float x) {
    const uint32_t u = enc_bits(x);
    if (x != x || u == 0xff800000u) return x;
    if (x == 0.0f) return enc_float(0x80000001u);
    return enc_float(x > 0.0f ? u - 1u : u + 1u);
}
MTS_ENC float enc_next_up(float x) {
    const uint32_t u = enc_bits(x);
    if (x != x || u == 0x7f800000u) return x;
    if (x == 0.0f) return enc_float(0x00000001u);
    return enc_float(x > 0.0f ? u + 1u : u - 1u);
}

// padded() of one axis of an exact box [lo, hi]
MTS_ENC void enc_padded(float lo_f, float hi_f, double extent, float *lo, float *hi) {
    const double blo = (double) lo_f, bhi = (double) hi_f;
    const double m = fmax(fmax(fabs(blo), fabs(bhi)), bhi - blo);
    const double pad = 1e-5 * m + 1e-7 * extent + 1e-30;
    *lo = enc_next_down((float) (blo - pad));
    *hi = enc_next_up((float) (bhi + pad));
}

MTS_ENC uint32_t enc_qlo(float v, double glo, double gstep) {
    const double q = floor(((double) v - glo) / gstep - 0.125);
    return (uint32_t) fmin(65535.0, fmax(0.0, q));
}
MTS_ENC uint32_t enc_qhi(float v, double glo, double gstep) {
    const double q = ceil(((double) v - glo) / gstep + 0.125);
    return (uint32_t) fmin(65535.0, fmax(0.0, q));
}

// fp16 with directed rounding of an integer v in [-32768, 32768]: the 11 significant bits are the top of the float's 24, the 13 below
// them decide whether the magnitude goes up
MTS_ENC uint32_t enc_half(float v, bool up) {
    const uint32_t sign = v < 0.0f ? 0x8000u : 0u;
    const uint32_t a = enc_bits(v) & 0x7fffffffu;
    if (a == 0u) return sign;
    const uint32_t mant = (a & 0x7fffffu) | 0x800000u;
    uint32_t e = a >> 23;                       // biased; frexp's exponent is e - 126
    uint32_t k = mant >> 13;                    // in [1024, 2048)
    const bool away = (v >= 0.0f) == up;
    if (away && (mant & 0x1fffu)) ++k;
    if (k >= 2048u) { k = 1024u; ++e; }
    return sign | ((e - 112u) << 10) | (k - 1024u);       // (e - 126) - 1 + 15
}

// one axis of one child box in the three BVH4 encodings (bvh.h) and the BVH2 grid word
MTS_ENC uint32_t enc_word16(uint32_t ql, uint32_t qh) { return ql | (qh << 16); }
MTS_ENC uint32_t enc_word_half(uint32_t ql, uint32_t qh) {
    return enc_half((float) ql - 32768.0f, false) | (enc_half((float) qh - 32768.0f, true) << 16);
}
MTS_ENC uint32_t enc_word_p15(uint32_t ql, uint32_t qh) {
    const uint32_t l15 = ql >> 1, h = (qh + 1u) >> 1, h15 = h < 32767u ? h : 32767u;
    return (0x8000u | l15) | ((0x8000u | h15) << 16);
}

} // namespace mtsamd

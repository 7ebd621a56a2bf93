// vertex_normals.h -- Mesh::recompute_vertex_normals (mesh.cpp:199-276) restated in fp32, one definition for the host specification
// (compute_vertex_normals, scene_build.cpp) and the device (k_normals_faces / k_normals_vertices, refit.hip).  The requirement is bit
// identity between the two, so only operations whose result IEEE fixes are used: fp32 and fp64 + - * /, explicit fmaf, a square root
// taken in double and rounded once more (exact for 24-bit operands, as triangle_area), and lm_acos (device_libm.h).  The build has
// -ffp-contract=off.
//
// Per face (vn_face): a = v1 - v0, b = v2 - v0, c = v2 - v1; n = cross(a, b) with the explicit-fma form of k_refit_check;
// length_sqr = fma(nz, nz, fma(ny, ny, nx * nx)).  The face normal is n / sqrt(length_sqr); the angle at corner j is
// lm_acos(clamp(dot(normalize(d0), normalize(d1)), -1, 1)) with d0 = v[j + 1] - v[j], d1 = v[j + 2] - v[j] (the safe_acos form of the
// reference's GPU branch, mesh.cpp:264-268) and normalize(d) = d / sqrt(fma(dz, dz, fma(dy, dy, dx * dx))).
//
// Underflow and overflow.  A face contributes only if length_sqr and the three squared edge lengths are all > 0 and finite; any other
// face is degenerate and is skipped, as the reference's scalar branch skips length_sqr <= 0.  That covers a zero-area face, a squared
// length that underflows to 0 (edges of 1e-30 and 1e10: the cross product is a positive denormal, one squared edge length is 0), an
// edge or a product that overflows (inf, or NaN from inf - inf: no comparison with a NaN holds).  A contributing face has finite
// quotients throughout: every numerator is finite and every divisor positive and finite; the dot product is clamped before lm_acos, so
// an angle lies in [0, pi].  A denormal length_sqr keeps few bits, so such a face's normal may be off unit length: it only weighs less
// or more, the vertex normal is normalised below.
//
// Per vertex: acc += n * angle (a product, then a sum, per component) over the incident corners in increasing (face, corner) order,
// the order of the reference's sequential loop, starting from +0.  A skipped face adds nothing; the device, which gathers, adds the
// zeros k_normals_faces wrote for it instead: acc + (+0) == acc bit for bit, since a sum that starts at +0 never becomes -0.  The
// length is taken in double (vn_finish): the squares of fp32 values neither underflow nor overflow there, so length != 0 exactly when
// some component is not zero, and the quotient rounded to fp32 is a unit vector to one rounding.  A vertex with length == 0 (isolated,
// only in skipped faces, or contributions that cancel exactly) gets the reference's bogus (1, 0, 0).  No output is ever non-finite.
#pragma once
#include "device_libm.h"

namespace mtsamd {

#define MTS_VN __host__ __device__ inline

// the correctly rounded fp32 square root: a double root rounded once more
MTS_VN float vn_sqrt(float x) { return (float) sqrt((double) x); }
MTS_VN float vn_length_sqr(const float d[3]) { return __builtin_fmaf(d[2], d[2], __builtin_fmaf(d[1], d[1], d[0] * d[0])); }
MTS_VN bool vn_positive_finite(float x) { return x > 0.0f && x < __builtin_inff(); }

// angle between q - p and r - p; the caller has checked their squared lengths
MTS_VN float vn_corner_angle(const float *p, const float *q, const float *r) {
    float d0[3] = { q[0] - p[0], q[1] - p[1], q[2] - p[2] }, d1[3] = { r[0] - p[0], r[1] - p[1], r[2] - p[2] };
    const float l0 = vn_sqrt(vn_length_sqr(d0)), l1 = vn_sqrt(vn_length_sqr(d1));
    for (int k = 0; k < 3; ++k) { d0[k] = d0[k] / l0; d1[k] = d1[k] / l1; }
    float c = __builtin_fmaf(d0[2], d1[2], __builtin_fmaf(d0[1], d1[1], d0[0] * d1[0]));
    c = c < -1.0f ? -1.0f : (c > 1.0f ? 1.0f : c);
    return lm_acos(c);
}

// rec[0..3): the normalised face normal, rec[3..6): the angles at its three corners.  false: the face is skipped and rec is all +0
MTS_VN bool vn_face(const float *v0, const float *v1, const float *v2, float rec[6]) {
    const float a[3] = { v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2] }, b[3] = { v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2] };
    const float c[3] = { v2[0] - v1[0], v2[1] - v1[1], v2[2] - v1[2] };
    const float n[3] = { __builtin_fmaf(a[1], b[2], -(a[2] * b[1])), __builtin_fmaf(a[2], b[0], -(a[0] * b[2])), __builtin_fmaf(a[0], b[1], -(a[1] * b[0])) };
    const float length_sqr = vn_length_sqr(n);
    if (!(vn_positive_finite(length_sqr) && vn_positive_finite(vn_length_sqr(a)) && vn_positive_finite(vn_length_sqr(b)) &&
          vn_positive_finite(vn_length_sqr(c)))) {
        for (int k = 0; k < 6; ++k) rec[k] = 0.0f;
        return false;
    }
    const float length = vn_sqrt(length_sqr);
    for (int k = 0; k < 3; ++k) rec[k] = n[k] / length;
    rec[3] = vn_corner_angle(v0, v1, v2);
    rec[4] = vn_corner_angle(v1, v2, v0);
    rec[5] = vn_corner_angle(v2, v0, v1);
    return true;
}

// one incident corner into a vertex's sum
MTS_VN void vn_accumulate(float acc[3], const float rec[6], uint32_t corner) {
    for (int k = 0; k < 3; ++k) acc[k] = acc[k] + rec[k] * rec[3 + corner];
}

MTS_VN void vn_finish(const float acc[3], float out[3]) {
    const double x = (double) acc[0], y = (double) acc[1], z = (double) acc[2];
    const double length = sqrt(x * x + y * y + z * z);
    if (length != 0.0) { out[0] = (float) (x / length); out[1] = (float) (y / length); out[2] = (float) (z / length); }
    else { out[0] = 1.0f; out[1] = 0.0f; out[2] = 0.0f; }       // "Choose some bogus value" (mesh.cpp:244)
}

} // namespace mtsamd

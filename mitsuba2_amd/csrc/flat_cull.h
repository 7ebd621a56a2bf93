// Cluster culls of the flat-scene ray queries (traverse_flat_clustered, traverse_flat_clustered_any, traverse_flat_worklist,
// device_scene.h): the encoding of a cluster record (scene_build.cpp, stage 7), the reciprocal of a direction component and the
// predicate "the segment [tmin, tmax] of this ray reaches the cluster's box".  Host and device code: tests/test_flat_cull_cpu.py
// compiles these for the host.  The boxes only cull, so nothing here has to be bit-exact: the predicate must never reject a cluster
// that holds a triangle the pair test accepts, and that is all.
//   MTS_FLAT_CULL_FORM 0: lo / hi boxes, three IEEE divisions per query, a min / max per axis, the pair mask shifted together per lane
//                         (the loops of device_scene.h keep that code as it was: the library then assembles to what it was before)
//   MTS_FLAT_CULL_FORM 1: centre / half-extent boxes with the pair mask built on the host, v_rcp_f32, the ray's sign folded into the
//                         query once, so that the near and far planes need no min / max per axis
// Every form's predicate is here whatever the switch says, so that the test holds them against each other in one program.
#pragma once
#include <hip/hip_runtime.h>      // float4, make_float4, __host__ __device__
#include <cmath>
#include <cstdint>
#include <cstring>

#ifndef MTS_FLAT_CULL_FORM
#define MTS_FLAT_CULL_FORM 1
#endif

namespace mtsamd {

// ---- the record: two float4 per cluster of `count` consecutive pairs starting at pair `first` ------------------------------------------
//   form 0: (lo.xyz, count) (hi.xyz, 0)
//   form 1: (c.xyz, count) (h.xyz, mask): the box [c - h, c + h] contains [lo, hi] (c is the rounded midpoint, h is rounded up from the
//           larger of the two exact distances); mask = `count` ones shifted to bit `first`, which the device ORs in under the compare
// lo / hi: the padded box (the builder's pad is what covers the rounding of the slab arithmetic, see cull_slabs).
template <int FORM>
inline void cull_encode(const float lo[3], const float hi[3], uint32_t first, uint32_t count, float4 &r0, float4 &r1) {
    float cntf; std::memcpy(&cntf, &count, 4);
    if (FORM == 0) {
        r0 = make_float4(lo[0], lo[1], lo[2], cntf);
        r1 = make_float4(hi[0], hi[1], hi[2], 0.0f);
        return;
    }
    float c[3], h[3];
    for (int a = 0; a < 3; ++a) {
        c[a] = (float) (0.5 * ((double) lo[a] + (double) hi[a]));
        const double hd = std::fmax((double) hi[a] - (double) c[a], (double) c[a] - (double) lo[a]);      // exact: differences of floats
        h[a] = (float) hd;
        if ((double) h[a] < hd) h[a] = std::nextafterf(h[a], INFINITY);
    }
    const uint32_t mask = (uint32_t) ((1ull << count) - 1ull) << first;
    float maskf; std::memcpy(&maskf, &mask, 4);
    r0 = make_float4(c[0], c[1], c[2], cntf);
    r1 = make_float4(h[0], h[1], h[2], maskf);
}
__host__ __device__ inline uint32_t cull_count(const float4 &r0) { return __builtin_bit_cast(uint32_t, r0.w); }
__host__ __device__ inline uint32_t cull_mask(const float4 &r1) { return __builtin_bit_cast(uint32_t, r1.w); }

// ---- the reciprocal ----------------------------------------------------------------------------------------------------------------
// |r| <= 3e38 with the sign of d: a zero, -0 or denormal component (v_rcp_f32 takes a denormal for zero) gives +-3e38, finite, so that
// the slab test stays NaN-free (0 * huge = 0, never inf * 0).  At the other end v_rcp_f32 gives 0 where the exact reciprocal is a
// denormal, |d| > 2^126 = 8.5e37: near = far = 0 on that axis, and a cluster is then rejected for mint > 0 that the division kept.  The
// cull is conservative for |d| <= 8.5e37 -- far beyond any direction the pair test itself can take without overflowing.
__host__ __device__ inline float cull_clamp_inv(float r, float d) { return std::fabs(r) <= 3.0e38f ? r : copysignf(3.0e38f, d); }
__host__ __device__ inline float cull_inv(float d) {
#if defined(__HIP_DEVICE_COMPILE__)
    return cull_clamp_inv(__builtin_amdgcn_rcpf(d), d);      // within 1 ulp; error budget: cull_slabs
#else
    return cull_clamp_inv(1.0f / d, d);
#endif
}

// ---- the query ---------------------------------------------------------------------------------------------------------------------
// With s = the sign of d (+-1) the ray runs UP the mirrored coordinate us = (c - o) * s along every axis, whatever its direction: it
// enters the slab at (us - h) * a and leaves it at (us + h) * a, a = |1 / d|.  Two ways to hold that:
//   CullFolded: s, n = -(o * s), a.  us = fma(c, s, n): one instruction, rounded once (a product with +-1 is exact).  Nine values; for
//               the work lists, whose cull loop holds nothing else.
//   CullLean:   o, s, a.  us = (c - o) * s: one instruction more per axis and three values less, o being live anyway.  For the clustered
//               loops, which keep the query across their pair tests: with CullFolded there the headline kernel spills 9-10 VGPRs
//               (36-40 B of scratch) instead of 5 (24 B); it spilled 6 with form 0.
struct CullFolded { float sx, sy, sz, nx, ny, nz, ax, ay, az; };
struct CullLean { float ox, oy, oz, sx, sy, sz, ax, ay, az; };
struct CullLoHi { float ox, oy, oz, ix, iy, iz; };      // form 0

// (ix, iy, iz): cull_inv of the direction, or anything within the error budget of it (the test moves it by an ulp either way)
__host__ __device__ inline void cull_ray_inv(CullFolded &q, float ox, float oy, float oz, float dx, float dy, float dz, float ix, float iy, float iz) {
    const float sx = copysignf(1.0f, dx), sy = copysignf(1.0f, dy), sz = copysignf(1.0f, dz);
    q = CullFolded{ sx, sy, sz, -(ox * sx), -(oy * sy), -(oz * sz), std::fabs(ix), std::fabs(iy), std::fabs(iz) };
}
__host__ __device__ inline void cull_ray_inv(CullLean &q, float ox, float oy, float oz, float dx, float dy, float dz, float ix, float iy, float iz) {
    q = CullLean{ ox, oy, oz, copysignf(1.0f, dx), copysignf(1.0f, dy), copysignf(1.0f, dz), std::fabs(ix), std::fabs(iy), std::fabs(iz) };
}
__host__ __device__ inline void cull_ray_inv(CullLoHi &q, float ox, float oy, float oz, float, float, float, float ix, float iy, float iz) {
    q = CullLoHi{ ox, oy, oz, ix, iy, iz };
}
template <typename Q>
__host__ __device__ inline Q cull_ray(float ox, float oy, float oz, float dx, float dy, float dz) {
    Q q;
    cull_ray_inv(q, ox, oy, oz, dx, dy, dz, cull_inv(dx), cull_inv(dy), cull_inv(dz));
    return q;
}

// tn = max(near.xyz, tmin) and tf = min(far.xyz, tmax) without a min / max per axis.  The subtraction comes before the product, so a
// clamped a = 3e38 never meets inf - inf: us -+ h is finite, its product with a finite a is a number (0 * 3e38 = 0), and tn <= tf has no
// NaN on either side for finite o, d and box.
// Error budget, relative to the pad of 1e-4 of the scene's extent E (|c|, h <= E): us is off by half an ulp of |c - o| (CullLean: twice
// that), us -+ h by another half ulp, a by 1 ulp (v_rcp_f32) and the product by half an ulp: a plane moves by less than
// 3 * 2^-23 * (|c - o| + h), i.e. 7e-7 * E from inside the scene and 4e-5 * E from 100 extents away -- inside the pad; form 0 spends the
// same budget without the rcp ulp.
__host__ __device__ inline bool cull_slabs(float ux, float uy, float uz, float ax, float ay, float az, const float4 &r1, float tmin, float tmax) {
    const float tn = fmaxf(fmaxf(fmaxf((ux - r1.x) * ax, (uy - r1.y) * ay), (uz - r1.z) * az), tmin);
    const float tf = fminf(fminf(fminf((ux + r1.x) * ax, (uy + r1.y) * ay), (uz + r1.z) * az), tmax);
    return tn <= tf;
}
__host__ __device__ inline bool cull_reach(const CullFolded &q, const float4 &r0, const float4 &r1, float tmin, float tmax) {
    return cull_slabs(fmaf(r0.x, q.sx, q.nx), fmaf(r0.y, q.sy, q.ny), fmaf(r0.z, q.sz, q.nz), q.ax, q.ay, q.az, r1, tmin, tmax);
}
__host__ __device__ inline bool cull_reach(const CullLean &q, const float4 &r0, const float4 &r1, float tmin, float tmax) {
    return cull_slabs((r0.x - q.ox) * q.sx, (r0.y - q.oy) * q.sy, (r0.z - q.oz) * q.sz, q.ax, q.ay, q.az, r1, tmin, tmax);
}
// Form 0: the slab test as it was, (plane - o) * inv with a min / max per axis (restated for the test; the device keeps its own copy).
__host__ __device__ inline bool cull_reach(const CullLoHi &q, const float4 &r0, const float4 &r1, float tmin, float tmax) {
    const float ax = (r0.x - q.ox) * q.ix, bx = (r1.x - q.ox) * q.ix;
    const float ay = (r0.y - q.oy) * q.iy, by = (r1.y - q.oy) * q.iy;
    const float az = (r0.z - q.oz) * q.iz, bz = (r1.z - q.oz) * q.iz;
    const float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), tmin));
    const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), tmax));
    return tn <= tf;
}

}  // namespace mtsamd

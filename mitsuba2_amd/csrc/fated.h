// Fated paths (bounce_step / bounce_step_spectral, kernels.hip): a path whose end at the NEXT step is already decided when its ray is
// spawned -- by max_depth, or by a Russian roulette whose inputs (thr, eta, depth, the next PCG32 output) are all known by then --
// can only change its sample if the ray's closest hit is an area emitter.  If the ray cannot reach any emitter's triangles the step
// ends the path at once and the ray query of the next launch never runs ("Fated paths").
// Host and device code: tests/test_fated_box_cpu.py compiles the predicates for the host.
//
// The record.  DevEmitter::aux of an AREA emitter (pad0 == 0; the delta emitters use aux[0..12] for themselves, nobody uses aux[13..15]):
//   aux[0..3]   (centre.xyz, 0)         the padded box over the emitter's triangles, in the centre / half-extent form of flat_cull.h,
//   aux[4..7]   (half-extent.xyz, 0)    read by cull_reach; an infinite half-extent is "reach everything" (an invalidated box)
//   aux[8..13]  lo.xyz, hi.xyz          the exact box (host only): the pad follows the scene's extent, which a vertex update of
//                                       ANY shape changes, so the padded box is encoded again from these whenever the scene box moves
//   aux[15] of emitter 0 (any kind)     the scene's list: up to kFatedMaxBoxes bytes (index of an area emitter + 1, low byte first,
//                                       0 ends the list).  0 = the elision is off: an environment emitter, no area emitter, more
//                                       than kFatedMaxBoxes of them, or one whose index does not fit a byte.
// The pad is the cluster boxes' (scene_build.cpp, stage 7): 1e-4 of the largest coordinate magnitude of the scene, 1e-3 at least.
#pragma once
#include "flat_cull.h"

#ifndef MTS_FATED_ELIDE
#define MTS_FATED_ELIDE 1       // 0: the step and the shadow ring of the parent commit, kernel for kernel (profiles/r27_isa_identity.txt)
#endif
#ifndef MTS_FATED_ELIDE_SPECTRAL
// The spectral step.  Shipped at 0: the spectral ring keeps its zombies, so the elision alone removes few
// chunks there, and the helper's live values cost the spectral kernels scratch at their 128-VGPR cap.  Measured with the switch at 1
// (profiles/r27_ab_fated_elide.txt): spectral Cornell box -5.0 %, the 261 k-triangle spectral mesh -1.4 %.  The results are the same
// bits either way (tests/test_gpu_fated_elide.py passes with 1 too).
#define MTS_FATED_ELIDE_SPECTRAL 0
#endif
#ifndef MTS_FATED_STATS
#define MTS_FATED_STATS 0       // diagnostic builds: an elided ray is NOT counted as a closest-hit ray (scripts/debug/fated_stats.py)
#endif

namespace mtsamd {

constexpr uint32_t kFatedMaxBoxes = 4u;
constexpr int kFatedBox = 0, kFatedExact = 8, kFatedList = 15;      // words of DevEmitter::aux

// aux[kFatedBox ..] <- the padded box of [lo, hi] (the exact words are emitter_exact_box's, scene_build.cpp)
inline void fated_encode(const float lo[3], const float hi[3], float pad, float *aux) {
    float plo[3], phi[3];
    for (int a = 0; a < 3; ++a) { plo[a] = lo[a] - pad; phi[a] = hi[a] + pad; }
    float4 r0, r1;
    cull_encode<1>(plo, phi, 0u, 0u, r0, r1);
    aux[kFatedBox + 0] = r0.x; aux[kFatedBox + 1] = r0.y; aux[kFatedBox + 2] = r0.z; aux[kFatedBox + 3] = 0.0f;
    aux[kFatedBox + 4] = r1.x; aux[kFatedBox + 5] = r1.y; aux[kFatedBox + 6] = r1.z; aux[kFatedBox + 7] = 0.0f;
}
// a box every ray reaches (tn = -inf .. tmin, tf = tmax): a NaN-free "keep"
inline void fated_invalidate(float *aux) {
    for (int a = 0; a < 3; ++a) { aux[kFatedBox + a] = 0.0f; aux[kFatedBox + 4 + a] = INFINITY; }
    aux[kFatedBox + 3] = aux[kFatedBox + 7] = 0.0f;
}

// what pcg_next_f32 (device_math.h) would return for a generator in this state; the state is not advanced
__host__ __device__ inline float fated_peek_f32(uint64_t state) {
    const uint32_t xs = (uint32_t) (((state >> 18u) ^ state) >> 27u);
    const uint32_t rot = (uint32_t) (state >> 59u);
    const uint32_t u = (xs >> rot) | (xs << ((~rot + 1u) & 31));
    return __builtin_bit_cast(float, (u >> 9) | 0x3f800000u) - 1.0f;
}

// The next step ends this path whatever it finds.  depth, hm = hmax(thr), eta, rng_state: the state the next step starts from; the
// expressions are that step's own (depth test, q, the roulette compare), so the two cannot disagree.
__host__ __device__ inline bool fated_decide(uint32_t depth, int32_t max_depth, int32_t rr_depth, float hm, float eta, uint64_t rng_state) {
    bool fated = depth >= (uint32_t) max_depth;
    if ((int32_t) depth > rr_depth) {
        const float q = fminf(hm * (eta * eta), 0.95f);
        fated = fated || !(fated_peek_f32(rng_state) < q);
    }
    return fated;
}

// the segment [mint, maxt] of the query's ray reaches the padded box of this area emitter
__host__ __device__ inline bool fated_reach(const CullLean &q, const float *aux, float mint, float maxt) {
    const float4 r0 = make_float4(aux[kFatedBox + 0], aux[kFatedBox + 1], aux[kFatedBox + 2], 0.0f);
    const float4 r1 = make_float4(aux[kFatedBox + 4], aux[kFatedBox + 5], aux[kFatedBox + 6], 0.0f);
    return cull_reach(q, r0, r1, mint, maxt);
}

}  // namespace mtsamd

// lbvh.h -- launch interface of the device accelerator rebuild (lbvh.hip): the topology of bvh.h's build_lbvh, built on the device from
// the positions a scene holds, into buffers the caller hands in.  A translation unit of its own, as refit.hip: kernels.hip knows nothing
// of it.  The host function build_lbvh is the specification; the device is held to its bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "refit.h"

namespace mtsamd {

// What a rebuild writes, sized for the worst case of n primitives: 2n - 1 builder nodes, n - 1 BVH2 nodes, n - 1 wide nodes, n slots.
// lbvh_build fills all of it; the caller owns the memory and swaps it into the scene once the build is accepted.
struct LbvhTarget {
    uint32_t *prim_slot, *slot_prim, *order;
    int2 *kids;
    int32_t *node_child, *wide_child;
    float *boxes;
    float4 *tris, *nodes;
    uint4 *qnodes, *wnodes;
};

struct LbvhResult {
    uint32_t n_builder = 0, n_nodes = 0, n_wide = 0, n_slots = 0, depth = 0, wdepth = 0;
    uint32_t root = 0, wroot = 0;                  // child references of the roots
    std::vector<uint32_t> class_start;             // height classes of `order`
};

struct LbvhScratch;                                 // device scratch of a build of up to n primitives; kept between rebuilds
hipError_t lbvh_scratch_create(uint32_t n_prims, LbvhScratch **out);
void lbvh_scratch_destroy(LbvhScratch *scratch);

// The whole build on stream s, from tri_pos (9 floats per primitive) and the scene box (the exact union of all vertices: 6 floats).
// Waits for the stream several times (counts come back to size the next launches) and returns with everything written.
hipError_t lbvh_build(LbvhScratch *scratch, const float *tri_pos, uint32_t n_prims, uint32_t max_leaf, const float bbox[6], const RefitGrid &grid,
                      const LbvhTarget &target, LbvhResult &result, hipStream_t s);

// SAH cost of the tree (kids, boxes) of n_builder builder nodes with root 0: partial[b] = the sum of block b of kSahBlock terms
// (lbvh_keys.h); the host adds them in order.  partial: (n_builder + kSahBlock - 1) / kSahBlock doubles on the device.
hipError_t launch_sah_partials(const int2 *kids, const float *boxes, uint32_t n_builder, int32_t root, double *partial, hipStream_t s);

} // namespace mtsamd

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

// device scratch of a build of up to n primitives; kept between rebuilds (lbvh_scratch_create allocates it)
struct LbvhScratch {
    uint32_t n = 0;                          // primitives the arrays are sized for; R = 2n - 1 radix-tree nodes
    uint32_t *codes = nullptr, *codes_sorted = nullptr, *iota = nullptr;        // n, n, R
    uint32_t *state = nullptr, *rfirst = nullptr, *rcount = nullptr;            // R each: what a radix-tree node becomes, and its range
    int32_t *rl = nullptr, *rr = nullptr;                                       // n each: children of the inner radix-tree nodes
    uint32_t *any_flag = nullptr, *bid = nullptr, *inner_flag = nullptr, *iid = nullptr;      // R + 1, R + 1, n + 1, n + 1
    uint32_t *ref2 = nullptr, *ref4 = nullptr;                                  // R each, per builder node
    uint32_t *h_a = nullptr, *h_b = nullptr, *h_sorted = nullptr, *hist = nullptr;             // R, R, R, 128
    int32_t *wide_builder = nullptr;                                            // n: the builder node a wide node replaces
    uint32_t *cnt = nullptr, *offs = nullptr;                                   // n + 1 each: inner children per wide node of a level
    void *tmp = nullptr; size_t tmp_bytes = 0;                                  // rocPRIM's
};
hipError_t lbvh_scratch_create(uint32_t n_prims, LbvhScratch **out);
void lbvh_scratch_destroy(LbvhScratch *scratch);

// The whole build on stream s, from tri_pos (9 floats per primitive) and the scene box (the exact union of all vertices: 6 floats).
// Waits for the stream several times (counts come back to size the next launches) and returns with everything written.
hipError_t lbvh_build(LbvhScratch *scratch, const float *tri_pos, uint32_t n_prims, uint32_t max_leaf, const float bbox[6], const RefitGrid &grid,
                      const LbvhTarget &target, LbvhResult &result, hipStream_t s);

// What lbvh_build ends in and another topology builder (sah_build.hip) can end in too, from the heights on: `rounds` rounds of the
// heights, the nodes by height, exact boxes by the refit's kernels, the BVH4 collapse per wide level, the emission.  In: tg.kids,
// tg.node_child, tg.slot_prim, tg.prim_slot and tg.tris of nb builder nodes (root 0) and n_nodes BVH2 nodes; sc->ref2 / sc->ref4 per
// builder node (an inner node's ref4: 0xffffffff, the root's 0) and sc->h_a: 0 for a leaf, kLbvhNoHeight for an inner node.
hipError_t lbvh_finish(LbvhScratch *scratch, const float *tri_pos, uint32_t n_prims, uint32_t n_builder, uint32_t n_nodes, uint32_t rounds, const RefitGrid &grid,
                       const LbvhTarget &target, LbvhResult &result, hipStream_t s);
// prim_slot and the slot records (tris) from slot_prim: lbvh_build's step after the sort
hipError_t launch_lbvh_slots(const float *tri_pos, const uint32_t *slot_prim, uint32_t n_prims, uint32_t *prim_slot, float4 *tris, hipStream_t s);

// SAH cost of the tree (kids, boxes) of n_builder builder nodes with root 0: partial[b] = the sum of block b of kSahBlock terms
// (lbvh_keys.h); the host adds them in order.  partial: (n_builder + kSahBlock - 1) / kSahBlock doubles on the device.
hipError_t launch_sah_partials(const int2 *kids, const float *boxes, uint32_t n_builder, int32_t root, double *partial, hipStream_t s);

} // namespace mtsamd

// sah_build.h -- launch interface of the device binned-SAH build (sah_build.hip): the topology of bvh.h's build_sah_levels, which is
// creation's tree, built level by level on the device from the positions a scene holds, into the buffers of an LbvhTarget.  From the
// heights on it is lbvh.hip's tail (lbvh_finish).  The host function build_sah_levels is the specification; the device is held to its bytes.
#pragma once
#include "lbvh.h"

namespace mtsamd {

// How a level's nodes are shared out.  A node of at most kSahWaveNode primitives is decided by one wave, a larger one by a whole
// workgroup; a level of at least kSahShareLevel nodes puts four consecutive nodes into a workgroup (its small nodes side by side, one
// wave each, its large ones one after the other), a smaller level one node.
constexpr uint32_t kSahWaveNode = 64u, kSahShareLevel = 8u;

struct SahScratch;                                  // device scratch of a build of up to n primitives; kept between rebuilds
hipError_t sah_scratch_create(uint32_t n_prims, SahScratch **out);
void sah_scratch_destroy(SahScratch *scratch);

// The whole build on stream s, from tri_pos (9 floats per primitive).  Waits for the stream once per level (the size of the next level
// comes back) and in the tail; returns with everything written.  Every count that comes back is held against its bound (2n - 1 builder
// nodes, n - 1 inner nodes, n slots) before it sizes a launch or an index: hipErrorUnknown instead of a write past a buffer.
hipError_t sah_build(SahScratch *scratch, LbvhScratch *tail_scratch, const float *tri_pos, uint32_t n_prims, uint32_t max_leaf, const RefitGrid &grid,
                     const LbvhTarget &target, LbvhResult &result, hipStream_t s);

// Host wall time of every level of the last build (launches, scan and the wait for the count), and the level's node count
const std::vector<float> &sah_level_ms(const SahScratch *scratch);
const std::vector<uint32_t> &sah_level_nodes(const SahScratch *scratch);

} // namespace mtsamd

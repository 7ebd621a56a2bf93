// bvh.h -- host-side binned-SAH BVH2 builder for the gfx950 traversal kernels.
//
// Replaces the reference's SAH kd-tree builder (include/mitsuba/render/kdtree.h:676-1881):
// only the *query result* of the accelerator is part of the contract (closest t / any hit,
// kdtree.h:2079-2174), so the structure is chosen for the GPU: 64-byte two-child nodes that a
// lane fetches with four 16-byte loads (LDS or L2), leaves of at most 4 triangles stored as
// 48-byte pre-subtracted (p0, e1, e2) records in leaf order.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mtsamd {

// What a refit needs of the topology (build_bvh fills it, refit_bvh and the device refit read it).  Builder nodes are the nodes of the
// binary tree the SAH build made, leaves included; `boxes` holds the exact (unpadded) box of each, from which every output is emitted.
struct RefitTable {
    std::vector<int32_t> left, right;       // per builder node: children, -1 for a leaf
    std::vector<uint32_t> ref2, ref4;       // per builder node: its child reference in the BVH2 / the BVH4 (a leaf: flag | count << 27 | first slot)
    std::vector<uint32_t> height;           // per builder node: height above its leaves (a leaf: 0)
    std::vector<uint32_t> order, class_start;      // builder nodes sorted by height; class h is order[class_start[h] .. class_start[h + 1])
    // where the boxes are written, read from the side of the output: the builder node whose box is the left / right half of BVH2
    // node i (2 per node) and child c of wide node w (4 per node, -1: absent)
    std::vector<int32_t> node_child, wide_child;
    std::vector<uint32_t> slot_prim;        // per triangle slot: its primitive
    std::vector<float> boxes;               // per builder node: lo[3], hi[3]
    int32_t root = 0;
};

struct BvhOutput {
    std::vector<float> nodes;      // 16 floats per node (see device_scene.h for the layout)
    std::vector<uint32_t> qnodes;  // 8 words per node: the same child boxes on a 16-bit grid over the scene box, rounded outward
    float q_lo[3] = { 0, 0, 0 }, q_step[3] = { 1, 1, 1 };      // grid origin and cell size per axis
    // BVH4 collapsed from the BVH2 (the child of largest surface area is opened until a node has four children): 16 words per node,
    // per child (lo | hi << 16) x, y, z on the grid + child reference; an absent child has reference 0x7fffffff and an inverted box
    std::vector<uint32_t> wnodes;
    // the same BVH4 with the planes as fp16 values of (grid coordinate - 32768), rounded outward (lo down, hi up): the walk reads them
    // straight into v_fma_mix_f32 (no integer -> float conversion); an absent child has lo = +32768, hi = -32768
    std::vector<uint32_t> wnodes_h;
    std::vector<uint32_t> wnodes_p;      // same layout, 15-bit planes stored as 0x8000 | q15 (even cells of the grid): see bvh.cpp
    uint32_t wroot = 0, n_wnodes = 0, wdepth = 0;
    std::vector<float> tris;       // 12 floats per triangle slot
    uint32_t root = 0;             // child reference of the root
    uint32_t n_nodes = 0, n_slots = 0, depth = 0;
    float bbox[6] = { 0, 0, 0, 0, 0, 0 };
    RefitTable refit;
};

// builder knobs (defaults = the shipped configuration; experiment builds read others from the environment, api.cpp)
struct BvhOptions {
    int bins = 16;                 // SAH bins per axis
    double intersect_cost = 1.5;   // cost of a triangle test relative to a traversal step
    uint32_t sweep_below = 0;      // nodes of at most this many primitives: exact SAH sweep instead of the bins (0: never)
    bool dfs_order = false;        // pre-order instead of BFS node layout
};

// positions: 9 floats per primitive (p0, p1, p2), n_prims >= 1
void build_bvh(const float *tri_pos, uint32_t n_prims, uint32_t max_leaf, BvhOutput &out, const BvhOptions *opt = nullptr);

} // namespace mtsamd

namespace mtsamd {
// Same topology, new positions (9 floats per primitive, as for build_bvh): leaf boxes, their propagation upwards, and the emission of
// build_bvh with the new scene box -- extent, padding and quantisation grid are recomputed, nothing is clamped into the old grid.
// With the positions of creation every array comes out byte for byte as build_bvh left it.
void refit_bvh(const float *tri_pos, BvhOutput &out);
// What the emission derives from the scene box (6 floats: lo, hi): `extent` of the box padding and the quantisation grid
void scene_grid(const float bbox[6], double *extent, float q_lo[3], float q_step[3]);

// The topology a device can build (csrc/lbvh.hip does, and is held to these bytes): primitives in the order of (30-bit Morton code of
// the centre of their exact box over the scene box, primitive index); the binary radix tree of Karras 2012 over those keys, equal codes
// split on the bits of the sorted position; a radix-tree node that covers at most max_leaf primitives while its parent covers more is
// a leaf (a root that covers at most max_leaf: the whole scene is one leaf); the BVH4 collapse of build_bvh per wide level.  Numbering:
// triangle slots in sorted order; builder nodes = surviving radix-tree nodes in radix index order (inner nodes, then positions), BVH2
// nodes = surviving inner nodes in the same order; wide nodes level by level, within a level by parent and child position.  Fills
// everything build_bvh fills and ends in the same emission; refit_bvh refits it.  The binary depth is at most 31 + ceil(log2 n).
void build_lbvh(const float *tri_pos, uint32_t n_prims, uint32_t max_leaf, BvhOutput &out);

// build_bvh with the shipped BvhOptions (16 bins, intersect cost 1.5, no sweep, BFS layout; the experiment knobs of the environment are not
// honoured), restated level by level so that a device can build it (csrc/sah_build.hip does, and is held to these bytes).  Every decision
// of build_bvh depends only on the set of primitives of a node, so a level is a loop over independent nodes: node box and centroid box,
// 16 bins per axis of positive centroid extent, the search and the leaf rule of sah_keys.h, then a stable partition of the node's part of
// `perm` (identity at the root) by bin, or its middle when no candidate exists.  The one difference: from depth 40 on (root = 0) a split
// is the middle of the present order, whatever the search said, where build_bvh takes an object median by nth_element, whose order among
// equals is the library's; the depth bound 40 + ceil(log2 n) stays.  Numbering: builder nodes level by level (root 0; the children of a
// level's split nodes follow in parent order, left then right); BVH2 nodes = split nodes in that order (build_bvh's BFS order); triangle
// slots leaf by leaf in ascending builder id, inside a leaf in perm order, which is ascending primitive index (build_bvh's leaf-reach
// order); wide nodes as build_lbvh.  From the heights on it is build_lbvh's tail.  nodes, qnodes, wnodes* and the grid come out byte for
// byte as build_bvh's, tris / slot_prim with the same set in every leaf.  trace (may be null): what was decided, for the tests.
struct SahLevelsTrace {
    std::vector<uint32_t> first, count, depth, mode, left_count;      // per builder node; mode: sah_keys.h (kSahLeaf, ..)
    std::vector<int32_t> axis, bin;                                   // the search's result (-1: no candidate), whatever the mode
    std::vector<double> cost;
    uint32_t bins_of = 0;                                             // in: keep the bins of the first so many nodes of more than one primitive
    std::vector<uint32_t> bins_node, bins;                            // their builder ids, and kSahBinWords words each
};
void build_sah_levels(const float *tri_pos, uint32_t n_prims, uint32_t max_leaf, BvhOutput &out, SahLevelsTrace *trace = nullptr);

// The traversal stack of a hierarchy scene: entries per lane for a tree of these depths, and whether the stack of a 256-lane workgroup
// fits the LDS a launch may ask for (kernels.h: bounce_lds_bytes(v) <= kFlatLdsCap; api.cpp asserts that the constants agree).  An entry
// of the BVH4 walk has 8 bytes, one of the BVH2 walk 4.
constexpr uint32_t kStackEntryBytes = 8u, kStackBlock = 256u, kStackLdsCap = 150u * 1024u;
inline uint32_t bvh_stack_depth(uint32_t depth, uint32_t wdepth, bool bvh4) { return bvh4 ? 3u * wdepth + 2u : (depth > 2u ? depth : 2u); }
inline bool bvh_stack_fits(uint32_t stack_depth, uint32_t entry_bytes = kStackEntryBytes) { return (uint64_t) entry_bytes * stack_depth * kStackBlock <= kStackLdsCap; }

// SAH cost of the tree a refit table describes, from its exact boxes: the sum over inner builder nodes of area / area(root) plus 1.5 times
// the sum over leaves of count * area / area(root), in double, in the blocked order lbvh_keys.h fixes (the device's).  kids: 2 per
// builder node, (left, right) or (-1, leaf reference); boxes: 6 per builder node.
double sah_cost_blocked(const int32_t *kids, const float *boxes, size_t n_builder, int32_t root);
} // namespace mtsamd

// refit.h -- launch interface of the device BVH refit (refit.hip): a mesh's vertices move, the topology of the accelerator stays.
// A translation unit of its own: kernels.hip, SceneView and the argument blocks of the existing kernels know nothing of it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "refit_encode.h"

namespace mtsamd {

// The refit table of bvh.h on the device, beside the arrays it rewrites.  Builder nodes: `kids[t]` = (left, right), or (-1, leaf
// reference) for a leaf; `order` lists them by height above the leaves.
struct RefitView {
    const uint32_t *faces;          // 3 per primitive: vertex indices within the primitive's mesh
    const uint32_t *prim_slot;      // per primitive: its triangle slot
    const uint32_t *slot_prim;
    const int2 *kids;
    const uint32_t *order;
    const int32_t *node_child;      // 2 per BVH2 node
    const int32_t *wide_child;      // 4 per wide node, -1: absent
    float *boxes;                   // 6 per builder node: exact lo, hi
    uint32_t n_nodes, n_wide;
    float *tri_pos, *tri_nrm;       // 9 per primitive (tri_nrm: null if the scene has no normals)
    float4 *tris;                   // 3 per slot
    float4 *nodes;                  // 4 per BVH2 node
    uint4 *qnodes;                  // 2 per BVH2 node
    uint4 *wnodes;                  // 4 per wide node, in the encoding of the build (MTS_NODE_F16 / MTS_NODE_P15)
};

// Reads only: flag |= 1 if one of the n_floats coordinates is not finite; areas (may be null) receives the area of each of the
// n_faces triangles of the shape whose faces start at primitive first_prim
hipError_t launch_refit_check(const RefitView &rv, const float *positions, uint32_t n_floats, uint32_t first_prim, uint32_t n_faces, float *areas,
                              uint32_t *flag, hipStream_t s);
// recompute_vertex_normals of one shape (vertex_normals.h): `normals` (3 per vertex) from the staged positions.  offsets (n_vertices + 1)
// and corners (3 * n_faces, each 3 * face + corner with the face counted within the shape, ascending per vertex): the shape's
// vertex-to-corner table; face_recs: 6 floats per face of scratch.  Two launches; reads nothing the refit writes.
hipError_t launch_refit_normals(const RefitView &rv, const float *positions, uint32_t first_prim, uint32_t n_faces, uint32_t n_vertices,
                                const uint32_t *offsets, const uint32_t *corners, float *face_recs, float *normals, hipStream_t s);
// tri_pos, tri_nrm (normals not null) and the slot records of the shape's primitives
hipError_t launch_refit_gather(const RefitView &rv, const float *positions, const float *normals, uint32_t first_prim, uint32_t n_faces, hipStream_t s);
// boxes of the builder nodes order[first .. first + n): leaves from their triangles (height 0), inner nodes from their children.  One
// launch per height class: a class reads only what earlier launches wrote.
hipError_t launch_refit_boxes(const RefitView &rv, uint32_t first, uint32_t n, bool leaves, hipStream_t s);
// boxes -> nodes, qnodes, wnodes with the grid and extent of the new scene box
hipError_t launch_refit_emit(const RefitView &rv, const RefitGrid &grid, hipStream_t s);

} // namespace mtsamd

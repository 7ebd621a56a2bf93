// refit.hip -- device BVH refit for gfx950 (refit.h).  Four small kernels, and two that recompute vertex normals; the kernel boundary is the only synchronisation: no thread
// waits on another, nothing is handed between workgroups inside a launch, and min / max are exact, so every result is order-free.
// The arithmetic restates bvh.cpp's emission (refit_encode.h) and scene_build.cpp's triangle_area; the build has -ffp-contract=off.
#include "refit.h"
#include "device_scene.h"
#include "vertex_normals.h"

namespace mtsamd {
namespace {

constexpr uint32_t kRefitBlock = 256u;
inline uint32_t refit_blocks(uint64_t n) { return (uint32_t) ((n + kRefitBlock - 1u) / kRefitBlock); }

__global__ void __launch_bounds__(kRefitBlock) k_refit_check(const uint32_t *__restrict__ faces, const float *__restrict__ positions, uint32_t n_floats,
                                                             uint32_t n_faces, float *__restrict__ areas, uint32_t *flag) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i < n_floats) {
        const uint32_t u = __float_as_uint(positions[i]);
        if ((u & 0x7f800000u) == 0x7f800000u) atomicOr(flag, 1u);      // infinity or NaN
    }
    if (areas && i < n_faces) {
        float p[9];
        for (int j = 0; j < 3; ++j) {
            const uint32_t vi = faces[3 * (size_t) i + j];
            for (int k = 0; k < 3; ++k) p[3 * j + k] = positions[3 * (size_t) vi + k];
        }
        const float e1[3] = { p[3] - p[0], p[4] - p[1], p[5] - p[2] }, e2[3] = { p[6] - p[0], p[7] - p[1], p[8] - p[2] };
        const float cx = fmaf(e1[1], e2[2], -(e1[2] * e2[1])), cy = fmaf(e1[2], e2[0], -(e1[0] * e2[2])), cz = fmaf(e1[0], e2[1], -(e1[1] * e2[0]));
        // the correctly rounded fp32 square root, as the host's: a double root rounded once more is exact for 24-bit operands
        areas[i] = 0.5f * (float) sqrt((double) fmaf(cz, cz, fmaf(cy, cy, cx * cx)));
    }
}

__global__ void __launch_bounds__(kRefitBlock) k_refit_gather(RefitView rv, const float *__restrict__ positions, const float *__restrict__ normals,
                                                              uint32_t first_prim, uint32_t n_faces) {
    const uint32_t f = blockIdx.x * kRefitBlock + threadIdx.x;
    if (f >= n_faces) return;
    const uint32_t gp = first_prim + f;
    float p[9];
    for (int j = 0; j < 3; ++j) {
        const uint32_t vi = rv.faces[3 * (size_t) gp + j];
        for (int k = 0; k < 3; ++k) {
            p[3 * j + k] = positions[3 * (size_t) vi + k];
            if (normals) rv.tri_nrm[9 * (size_t) gp + 3 * j + k] = normals[3 * (size_t) vi + k];
        }
    }
    for (int q = 0; q < 9; ++q) rv.tri_pos[9 * (size_t) gp + q] = p[q];
    float4 *rec = rv.tris + 3 * (size_t) rv.prim_slot[gp];
    rec[0] = make_float4(p[0], p[1], p[2], p[3] - p[0]);
    rec[1] = make_float4(p[4] - p[1], p[5] - p[2], p[6] - p[0], p[7] - p[1]);
    rec[2] = make_float4(p[8] - p[2], __uint_as_float(gp), 0.0f, 0.0f);
}

__global__ void __launch_bounds__(kRefitBlock) k_refit_leaves(RefitView rv, uint32_t first, uint32_t n) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = rv.order[first + i];
    const uint32_t ref = (uint32_t) rv.kids[t].y, s0 = ref & 0x07ffffffu, count = (ref >> 27) & 15u;
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (uint32_t s = s0; s < s0 + count; ++s) {
        const float *tp = rv.tri_pos + 9 * (size_t) rv.slot_prim[s];
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) { lo[k] = enc_min(lo[k], tp[3 * j + k]); hi[k] = enc_max(hi[k], tp[3 * j + k]); }
    }
    float *bx = rv.boxes + 6 * (size_t) t;
    for (int k = 0; k < 3; ++k) { bx[k] = lo[k]; bx[3 + k] = hi[k]; }
}

__global__ void __launch_bounds__(kRefitBlock) k_refit_level(RefitView rv, uint32_t first, uint32_t n) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = rv.order[first + i];
    const int2 kd = rv.kids[t];
    const float *l = rv.boxes + 6 * (size_t) kd.x, *r = rv.boxes + 6 * (size_t) kd.y;
    float *bx = rv.boxes + 6 * (size_t) t;
    for (int k = 0; k < 3; ++k) { bx[k] = enc_min(l[k], r[k]); bx[3 + k] = enc_max(l[3 + k], r[3 + k]); }
}

// Vertex normals recomputed from the staged positions (vertex_normals.h holds the arithmetic, the host's too).  One thread per face
// writes the face's record: normal and corner angles, zeros for a skipped face.  `faces`: the shape's own, vertex indices below n_vertices.
__global__ void __launch_bounds__(kRefitBlock) k_normals_faces(const uint32_t *__restrict__ faces, const float *__restrict__ positions, uint32_t n_faces,
                                                               float *__restrict__ face_recs) {
    const uint32_t f = blockIdx.x * kRefitBlock + threadIdx.x;
    if (f >= n_faces) return;
    float p[9], rec[6];
    for (int j = 0; j < 3; ++j) {
        const uint32_t vi = faces[3 * (size_t) f + j];
        for (int k = 0; k < 3; ++k) p[3 * j + k] = positions[3 * (size_t) vi + k];
    }
    vn_face(p, p + 3, p + 6, rec);
    for (int k = 0; k < 6; ++k) face_recs[6 * (size_t) f + k] = rec[k];
}

// One thread per vertex gathers its corners (3 * face + corner) in the order of the table, which is the order of the host's loop over the
// faces: no atomics, the sum of each vertex has one order.
__global__ void __launch_bounds__(kRefitBlock) k_normals_vertices(const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ corners,
                                                                  const float *__restrict__ face_recs, uint32_t n_vertices, float *__restrict__ normals) {
    const uint32_t v = blockIdx.x * kRefitBlock + threadIdx.x;
    if (v >= n_vertices) return;
    float acc[3] = { 0.0f, 0.0f, 0.0f }, out[3];
    for (uint32_t c = offsets[v], end = offsets[v + 1]; c < end; ++c) {
        const uint32_t corner = corners[c], f = corner / 3u;
        float rec[6];
        for (int k = 0; k < 6; ++k) rec[k] = face_recs[6 * (size_t) f + k];
        vn_accumulate(acc, rec, corner - 3u * f);
    }
    vn_finish(acc, out);
    for (int k = 0; k < 3; ++k) normals[3 * (size_t) v + k] = out[k];
}

// one thread per child box: 2 per BVH2 node, then 4 per wide node.  Child references and the words of absent children stay as creation
// wrote them.
__global__ void __launch_bounds__(kRefitBlock) k_refit_emit(RefitView rv, RefitGrid g) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    const uint32_t n2 = 2u * rv.n_nodes;
    if (i >= n2 + 4u * rv.n_wide) return;
    const int32_t t = i < n2 ? rv.node_child[i] : rv.wide_child[i - n2];
    if (t < 0) return;
    const float *bx = rv.boxes + 6 * (size_t) t;
    float lo[3], hi[3];
    uint32_t ql[3], qh[3];
    for (int k = 0; k < 3; ++k) {
        enc_padded(bx[k], bx[3 + k], g.extent, &lo[k], &hi[k]);
        ql[k] = enc_qlo(lo[k], g.glo[k], g.gstep[k]); qh[k] = enc_qhi(hi[k], g.glo[k], g.gstep[k]);
    }
    if (i < n2) {
        float *q = reinterpret_cast<float *>(rv.nodes) + 16 * (size_t) (i >> 1) + 6u * (i & 1u);
        for (int k = 0; k < 3; ++k) { q[k] = lo[k]; q[3 + k] = hi[k]; }
        uint32_t *w = reinterpret_cast<uint32_t *>(rv.qnodes) + 8 * (size_t) (i >> 1) + 3u * (i & 1u);
        for (int k = 0; k < 3; ++k) w[k] = enc_word16(ql[k], qh[k]);
    } else {
        uint32_t *w = reinterpret_cast<uint32_t *>(rv.wnodes) + 4 * (size_t) (i - n2);
        for (int k = 0; k < 3; ++k)
            w[k] = MTS_NODE_P15 ? enc_word_p15(ql[k], qh[k]) : (MTS_NODE_F16 ? enc_word_half(ql[k], qh[k]) : enc_word16(ql[k], qh[k]));
    }
}

} // namespace

hipError_t launch_refit_check(const RefitView &rv, const float *positions, uint32_t n_floats, uint32_t first_prim, uint32_t n_faces, float *areas,
                              uint32_t *flag, hipStream_t s) {
    const uint32_t n = n_floats > n_faces ? n_floats : n_faces;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_refit_check, dim3(refit_blocks(n)), dim3(kRefitBlock), 0, s, rv.faces + 3 * (size_t) first_prim, positions, n_floats, n_faces, areas, flag);
    return hipGetLastError();
}

hipError_t launch_refit_gather(const RefitView &rv, const float *positions, const float *normals, uint32_t first_prim, uint32_t n_faces, hipStream_t s) {
    if (n_faces == 0) return hipSuccess;
    hipLaunchKernelGGL(k_refit_gather, dim3(refit_blocks(n_faces)), dim3(kRefitBlock), 0, s, rv, positions, normals, first_prim, n_faces);
    return hipGetLastError();
}

hipError_t launch_refit_normals(const RefitView &rv, const float *positions, uint32_t first_prim, uint32_t n_faces, uint32_t n_vertices,
                                const uint32_t *offsets, const uint32_t *corners, float *face_recs, float *normals, hipStream_t s) {
    if (n_faces) hipLaunchKernelGGL(k_normals_faces, dim3(refit_blocks(n_faces)), dim3(kRefitBlock), 0, s, rv.faces + 3 * (size_t) first_prim, positions, n_faces, face_recs);
    if (n_vertices) hipLaunchKernelGGL(k_normals_vertices, dim3(refit_blocks(n_vertices)), dim3(kRefitBlock), 0, s, offsets, corners, face_recs, n_vertices, normals);
    return hipGetLastError();
}

hipError_t launch_refit_boxes(const RefitView &rv, uint32_t first, uint32_t n, bool leaves, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (leaves) hipLaunchKernelGGL(k_refit_leaves, dim3(refit_blocks(n)), dim3(kRefitBlock), 0, s, rv, first, n);
    else hipLaunchKernelGGL(k_refit_level, dim3(refit_blocks(n)), dim3(kRefitBlock), 0, s, rv, first, n);
    return hipGetLastError();
}

hipError_t launch_refit_emit(const RefitView &rv, const RefitGrid &grid, hipStream_t s) {
    const uint64_t n = 2ull * rv.n_nodes + 4ull * rv.n_wide;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_refit_emit, dim3(refit_blocks(n)), dim3(kRefitBlock), 0, s, rv, grid);
    return hipGetLastError();
}

} // namespace mtsamd

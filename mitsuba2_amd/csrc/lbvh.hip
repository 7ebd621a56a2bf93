// lbvh.hip -- device accelerator rebuild for gfx950 (lbvh.h): Morton keys, a stable radix sort, the radix tree of Karras 2012, leaves of
// at most max_leaf triangles, compaction by scans, heights, exact boxes (refit.hip's kernels over the new table), the BVH4 collapse per
// wide level and the emission (refit.hip's).  As in refit.hip the kernel boundary is the only synchronisation: no thread waits on
// another and nothing is handed between workgroups inside a launch.  Every per-element step is a function of lbvh_keys.h, which the host
// specification (bvh.cpp: build_lbvh) calls too; sort and scans are rocPRIM's.  The build has -ffp-contract=off.
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "lbvh.h"
#include "lbvh_keys.h"
#include "device_scene.h"

namespace mtsamd {

namespace {

constexpr uint32_t kLbvhBlock = 256u;
constexpr uint32_t kHistBins = 128u;
inline uint32_t lbvh_blocks(uint64_t n) { return (uint32_t) ((n + kLbvhBlock - 1u) / kLbvhBlock); }

struct Box6 { float v[6]; };

__global__ void __launch_bounds__(kLbvhBlock) k_lbvh_iota(uint32_t *__restrict__ iota, uint32_t n) {
    const uint32_t i = blockIdx.x * kLbvhBlock + threadIdx.x;
    if (i < n) iota[i] = i;
}

__global__ void __launch_bounds__(kLbvhBlock) k_lbvh_keys(const float *__restrict__ tri_pos, uint32_t n, Box6 bbox, uint32_t *__restrict__ codes) {
    const uint32_t p = blockIdx.x * kLbvhBlock + threadIdx.x;
    if (p >= n) return;
    float tp[9];
    for (int q = 0; q < 9; ++q) tp[q] = tri_pos[9 * (size_t) p + q];
    codes[p] = lbvh_code(tp, bbox.v);
}

// one thread per inner node of the radix tree: its children, and what each of them becomes (0: below a leaf, 1: leaf, 2: inner).  Every
// node but the root has one parent, so every entry has one writer; thread 0 writes the root's and the zeros that end the flag arrays.
__global__ void __launch_bounds__(kLbvhBlock) k_lbvh_radix(LbvhScratch sc, uint32_t n_, uint32_t max_leaf) {
    const int n = (int) n_, i = (int) (blockIdx.x * kLbvhBlock + threadIdx.x);
    if (i == 0) {
        const uint32_t st = n_ > max_leaf ? 2u : 1u;
        sc.state[0] = st; sc.rfirst[0] = 0u; sc.rcount[0] = n_; sc.any_flag[0] = 1u;
        sc.any_flag[2u * n_ - 1u] = 0u; sc.inner_flag[n_ - 1u] = 0u;
        if (n > 1) sc.inner_flag[0] = st == 2u ? 1u : 0u;
    }
    if (i >= n - 1) return;
    int f, l, split;
    lbvh_radix_node(sc.codes_sorted, n, i, &f, &l, &split);
    const int32_t c[2] = { split == f ? n - 1 + split : split, split + 1 == l ? n - 1 + split + 1 : split + 1 };
    const uint32_t cf[2] = { (uint32_t) f, (uint32_t) split + 1u }, cc[2] = { (uint32_t) (split - f + 1), (uint32_t) (l - split) };
    sc.rl[i] = c[0]; sc.rr[i] = c[1];
    const bool open = (uint32_t) (l - f + 1) > max_leaf;
    for (int k = 0; k < 2; ++k) {
        const uint32_t st = !open ? 0u : (cc[k] > max_leaf ? 2u : 1u);
        sc.state[c[k]] = st; sc.rfirst[c[k]] = cf[k]; sc.rcount[c[k]] = cc[k];
        sc.any_flag[c[k]] = st ? 1u : 0u;
        if (c[k] < n - 1) sc.inner_flag[c[k]] = st == 2u ? 1u : 0u;
    }
}

// one thread per radix-tree node: the survivors write their builder node
__global__ void __launch_bounds__(kLbvhBlock) k_lbvh_compact(LbvhScratch sc, uint32_t n_radix, int2 *__restrict__ kids, int32_t *__restrict__ node_child) {
    const uint32_t x = blockIdx.x * kLbvhBlock + threadIdx.x;
    if (x >= n_radix) return;
    const uint32_t st = sc.state[x];
    if (!st) return;
    const uint32_t t = sc.bid[x];
    if (st == 2u) {
        const int32_t l = (int32_t) sc.bid[sc.rl[x]], r = (int32_t) sc.bid[sc.rr[x]];
        const uint32_t b2 = sc.iid[x];
        kids[t] = make_int2(l, r);
        node_child[2 * (size_t) b2] = l; node_child[2 * (size_t) b2 + 1] = r;
        sc.ref2[t] = b2; sc.ref4[t] = t == 0u ? 0u : 0xffffffffu;
        sc.h_a[t] = kLbvhNoHeight;
    } else {
        const uint32_t ref = kLbvhLeafFlag | (sc.rcount[x] << 27) | sc.rfirst[x];
        kids[t] = make_int2(-1, (int32_t) ref);
        sc.ref2[t] = ref; sc.ref4[t] = ref;
        sc.h_a[t] = 0u;
    }
}

// one thread per triangle slot: the slot's record as refit.hip's gather writes it, and the inverse of slot_prim
__global__ void __launch_bounds__(kLbvhBlock) k_lbvh_slots(const float *__restrict__ tri_pos, const uint32_t *__restrict__ slot_prim, uint32_t n,
                                                           uint32_t *__restrict__ prim_slot, float4 *__restrict__ tris) {
    const uint32_t s = blockIdx.x * kLbvhBlock + threadIdx.x;
    if (s >= n) return;
    const uint32_t gp = slot_prim[s];
    if (gp >= n) return;
    float p[9];
    for (int q = 0; q < 9; ++q) p[q] = tri_pos[9 * (size_t) gp + q];
    prim_slot[gp] = s;
    float4 *rec = tris + 3 * (size_t) s;
    rec[0] = make_float4(p[0], p[1], p[2], p[3] - p[0]);
    rec[1] = make_float4(p[4] - p[1], p[5] - p[2], p[6] - p[0], p[7] - p[1]);
    rec[2] = make_float4(p[8] - p[2], __uint_as_float(gp), 0.0f, 0.0f);
}

// one round of the heights: a node whose children both have theirs gets its own.  From h_in to h_out: a round reads only the round before.
__global__ void __launch_bounds__(kLbvhBlock) k_lbvh_height(const int2 *__restrict__ kids, const uint32_t *__restrict__ h_in, uint32_t *__restrict__ h_out, uint32_t n_builder) {
    const uint32_t t = blockIdx.x * kLbvhBlock + threadIdx.x;
    if (t >= n_builder) return;
    uint32_t v = h_in[t];
    if (v == kLbvhNoHeight) {
        const int2 kd = kids[t];
        const uint32_t a = h_in[kd.x], b = h_in[kd.y];
        if (a != kLbvhNoHeight && b != kLbvhNoHeight) v = 1u + (a > b ? a : b);
    }
    h_out[t] = v;
}

__global__ void __launch_bounds__(kLbvhBlock) k_lbvh_hist(const uint32_t *__restrict__ h, uint32_t n_builder, uint32_t *hist) {
    const uint32_t t = blockIdx.x * kLbvhBlock + threadIdx.x;
    if (t >= n_builder) return;
    const uint32_t v = h[t];
    atomicAdd(&hist[v < kHistBins - 1u ? v : kHistBins - 1u], 1u);       // counts: order-free
}

// one thread per wide node of a level: its children, and how many of them are inner
__global__ void __launch_bounds__(kLbvhBlock) k_lbvh_collapse(const int2 *__restrict__ kids, const float *__restrict__ boxes, const int32_t *__restrict__ wide_builder,
                                                              uint32_t level_start, uint32_t level_cnt, int32_t *__restrict__ wide_child, uint32_t *__restrict__ cnt) {
    const uint32_t j = blockIdx.x * kLbvhBlock + threadIdx.x;
    if (j == 0) cnt[level_cnt] = 0u;
    if (j >= level_cnt) return;
    const uint32_t w = level_start + j;
    int32_t c[4];
    lbvh_collapse(kids, boxes, wide_builder[w], c);
    uint32_t inner = 0;
    for (int k = 0; k < 4; ++k) {
        wide_child[4 * (size_t) w + k] = c[k];
        if (c[k] >= 0 && kids[c[k]].x >= 0) ++inner;
    }
    cnt[j] = inner;
}

// ... and the wide nodes of the next level: the inner children by parent and child position
__global__ void __launch_bounds__(kLbvhBlock) k_lbvh_assign(const int2 *__restrict__ kids, const int32_t *__restrict__ wide_child, const uint32_t *__restrict__ offs,
                                                            uint32_t level_start, uint32_t level_cnt, uint32_t next_start, uint32_t cap,
                                                            uint32_t *__restrict__ ref4, int32_t *__restrict__ wide_builder) {
    const uint32_t j = blockIdx.x * kLbvhBlock + threadIdx.x;
    if (j >= level_cnt) return;
    uint32_t id = next_start + offs[j];
    for (int k = 0; k < 4; ++k) {
        const int32_t c = wide_child[4 * (size_t) (level_start + j) + k];
        if (c < 0 || kids[c].x < 0) continue;
        if (id < cap) { ref4[c] = id; wide_builder[id] = c; }
        ++id;
    }
}

// what the emission leaves alone: the child references of every node and the words of absent children (bvh.cpp: emit_bvh)
__global__ void __launch_bounds__(kLbvhBlock) k_lbvh_refs(const int32_t *__restrict__ node_child, const int32_t *__restrict__ wide_child, const uint32_t *__restrict__ ref2,
                                                          const uint32_t *__restrict__ ref4, uint32_t n_nodes, uint32_t n_wide, float4 *__restrict__ nodes,
                                                          uint4 *__restrict__ qnodes, uint4 *__restrict__ wnodes) {
    const uint32_t i = blockIdx.x * kLbvhBlock + threadIdx.x;
    if (i < n_nodes) {
        const uint32_t l = ref2[node_child[2 * (size_t) i]], r = ref2[node_child[2 * (size_t) i + 1]];
        uint32_t *q = reinterpret_cast<uint32_t *>(nodes) + 16 * (size_t) i, *w = reinterpret_cast<uint32_t *>(qnodes) + 8 * (size_t) i;
        q[12] = l; q[13] = r; q[14] = 0u; q[15] = 0u;
        w[6] = l; w[7] = r;
        return;
    }
    const uint32_t j = i - n_nodes;
    if (j >= 4u * n_wide) return;
    const int32_t t = wide_child[j];
    uint32_t *w = reinterpret_cast<uint32_t *>(wnodes) + 4 * (size_t) j;
    if (t < 0) {
        w[0] = w[1] = w[2] = MTS_NODE_P15 ? (0xffffu | (0x8000u << 16)) : (MTS_NODE_F16 ? (0x7800u | (0xf800u << 16)) : 65535u);
        w[3] = 0x7fffffffu;
    } else {
        w[3] = ref4[t];
    }
}

__global__ void __launch_bounds__(kSahBlock) k_sah_partials(const int2 *__restrict__ kids, const float *__restrict__ boxes, uint32_t n_builder, int32_t root,
                                                           double *__restrict__ partial) {
    __shared__ double v[kSahBlock];
    const uint32_t t = blockIdx.x * kSahBlock + threadIdx.x;
    const double root_area = lbvh_area(boxes + 6 * (size_t) root);
    v[threadIdx.x] = t < n_builder ? lbvh_sah_term(kids[t], boxes + 6 * (size_t) t, root_area) : 0.0;
    __syncthreads();
    for (uint32_t stride = kSahBlock / 2u; stride > 0u; stride /= 2u) {
        if (threadIdx.x < stride) v[threadIdx.x] += v[threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = v[0];
}

#define LBVH_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

template <typename T> hipError_t alloc(T **p, size_t count) { return hipMalloc((void **) p, sizeof(T) * (count ? count : 1)); }

hipError_t sort_pairs(LbvhScratch *sc, const uint32_t *keys_in, uint32_t *keys_out, const uint32_t *values_in, uint32_t *values_out, uint32_t n, uint32_t bits,
                      hipStream_t s) {
    size_t bytes = sc->tmp_bytes;
    return rocprim::radix_sort_pairs(sc->tmp, bytes, keys_in, keys_out, values_in, values_out, (size_t) n, 0u, bits, s);
}
hipError_t scan(LbvhScratch *sc, const uint32_t *in, uint32_t *out, uint32_t n, hipStream_t s) {
    size_t bytes = sc->tmp_bytes;
    return rocprim::exclusive_scan(sc->tmp, bytes, in, out, 0u, (size_t) n, rocprim::plus<uint32_t>(), s);
}

} // namespace

void lbvh_scratch_destroy(LbvhScratch *sc) {
    if (!sc) return;
    void *all[] = { sc->codes, sc->codes_sorted, sc->iota, sc->state, sc->rfirst, sc->rcount, sc->rl, sc->rr, sc->any_flag, sc->bid, sc->inner_flag, sc->iid,
                    sc->ref2, sc->ref4, sc->h_a, sc->h_b, sc->h_sorted, sc->hist, sc->wide_builder, sc->cnt, sc->offs, sc->tmp };
    for (void *p : all) (void) hipFree(p);
    delete sc;
}

hipError_t lbvh_scratch_create(uint32_t n, LbvhScratch **out) {
    *out = nullptr;
    if (n == 0) return hipErrorInvalidValue;
    LbvhScratch *sc = new LbvhScratch();
    sc->n = n;
    const size_t R = 2 * (size_t) n - 1;
    hipError_t e = hipSuccess;
    auto ok = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    ok(alloc(&sc->codes, n)); ok(alloc(&sc->codes_sorted, n)); ok(alloc(&sc->iota, R));
    ok(alloc(&sc->state, R)); ok(alloc(&sc->rfirst, R)); ok(alloc(&sc->rcount, R)); ok(alloc(&sc->rl, n)); ok(alloc(&sc->rr, n));
    ok(alloc(&sc->any_flag, R + 1)); ok(alloc(&sc->bid, R + 1)); ok(alloc(&sc->inner_flag, (size_t) n + 1)); ok(alloc(&sc->iid, (size_t) n + 1));
    ok(alloc(&sc->ref2, R)); ok(alloc(&sc->ref4, R)); ok(alloc(&sc->h_a, R)); ok(alloc(&sc->h_b, R)); ok(alloc(&sc->h_sorted, R));
    ok(alloc(&sc->hist, kHistBins)); ok(alloc(&sc->wide_builder, n)); ok(alloc(&sc->cnt, (size_t) n + 1)); ok(alloc(&sc->offs, (size_t) n + 1));
    // rocPRIM's temporary storage: the largest of the calls a build makes
    size_t need = 0, bytes = 0;
    uint32_t *u = nullptr;
    if (e == hipSuccess) { ok(rocprim::radix_sort_pairs(nullptr, bytes, u, u, u, u, (size_t) n, 0u, 30u, (hipStream_t) nullptr)); need = bytes > need ? bytes : need; }
    if (e == hipSuccess) { ok(rocprim::radix_sort_pairs(nullptr, bytes, u, u, u, u, R, 0u, 7u, (hipStream_t) nullptr)); need = bytes > need ? bytes : need; }
    if (e == hipSuccess) { ok(rocprim::exclusive_scan(nullptr, bytes, u, u, 0u, R + 1, rocprim::plus<uint32_t>(), (hipStream_t) nullptr)); need = bytes > need ? bytes : need; }
    if (e == hipSuccess) { sc->tmp_bytes = 2 * need + 65536; ok(hipMalloc(&sc->tmp, sc->tmp_bytes)); }       // slack: the calls of a build are of every smaller size too
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_lbvh_iota, dim3(lbvh_blocks(R)), dim3(kLbvhBlock), 0, (hipStream_t) nullptr, sc->iota, (uint32_t) R);
        ok(hipGetLastError());
        ok(hipDeviceSynchronize());
    }
    if (e != hipSuccess) { lbvh_scratch_destroy(sc); return e; }
    *out = sc;
    return hipSuccess;
}

hipError_t lbvh_build(LbvhScratch *sc, const float *tri_pos, uint32_t n, uint32_t max_leaf, const float bbox[6], const RefitGrid &grid, const LbvhTarget &tg,
                      LbvhResult &res, hipStream_t s) {
    if (!sc || n == 0 || n > sc->n || n >= (1u << 27)) return hipErrorInvalidValue;
    max_leaf = max_leaf < 1u ? 1u : (max_leaf > 15u ? 15u : max_leaf);
    const uint32_t R = 2u * n - 1u;
    Box6 box; for (int k = 0; k < 6; ++k) box.v[k] = bbox[k];
    // 1, 2. keys and their stable order: slot_prim is the order of the primitives
    hipLaunchKernelGGL(k_lbvh_keys, dim3(lbvh_blocks(n)), dim3(kLbvhBlock), 0, s, tri_pos, n, box, sc->codes);
    LBVH_TRY(hipGetLastError());
    LBVH_TRY(sort_pairs(sc, sc->codes, sc->codes_sorted, sc->iota, tg.slot_prim, n, 30u, s));
    hipLaunchKernelGGL(k_lbvh_slots, dim3(lbvh_blocks(n)), dim3(kLbvhBlock), 0, s, tri_pos, tg.slot_prim, n, tg.prim_slot, tg.tris);
    // 3, 4. the radix tree, what survives of it, and the compact numbering
    hipLaunchKernelGGL(k_lbvh_radix, dim3(lbvh_blocks(n > 1u ? n - 1u : 1u)), dim3(kLbvhBlock), 0, s, *sc, n, max_leaf);
    LBVH_TRY(hipGetLastError());
    LBVH_TRY(scan(sc, sc->any_flag, sc->bid, R + 1u, s));
    LBVH_TRY(scan(sc, sc->inner_flag, sc->iid, n, s));
    uint32_t counts[2] = { 0u, 0u };
    LBVH_TRY(hipMemcpyAsync(&counts[0], sc->bid + R, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LBVH_TRY(hipMemcpyAsync(&counts[1], sc->iid + (n - 1u), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LBVH_TRY(hipStreamSynchronize(s));
    const uint32_t nb = counts[0], n_nodes = counts[1];
    if (nb != 2u * n_nodes + 1u || nb > R) return hipErrorUnknown;       // a binary tree has one more leaf than inner nodes
    hipLaunchKernelGGL(k_lbvh_compact, dim3(lbvh_blocks(R)), dim3(kLbvhBlock), 0, s, *sc, R, tg.kids, tg.node_child);
    LBVH_TRY(hipGetLastError());
    // 5 - 8. as many rounds of the heights as a tree over n keys of 30 + ceil(log2 n) bits can be high
    uint32_t rounds = 32u;
    while ((1ull << (rounds - 32u)) < n) ++rounds;
    return lbvh_finish(sc, tri_pos, n, nb, n_nodes, rounds, grid, tg, res, s);
}

// The tail of a build, from the heights on (lbvh.h): kids, node_child, slot_prim / prim_slot / tris are written, sc->ref2 / ref4 hold the
// references of the builder nodes and sc->h_a their heights as far as known (leaves 0, inner nodes kLbvhNoHeight).
hipError_t lbvh_finish(LbvhScratch *sc, const float *tri_pos, uint32_t n, uint32_t nb, uint32_t n_nodes, uint32_t rounds, const RefitGrid &grid, const LbvhTarget &tg,
                       LbvhResult &res, hipStream_t s) {
    if (!sc || n == 0 || n > sc->n || nb != 2u * n_nodes + 1u || nb > 2u * n - 1u) return hipErrorInvalidValue;
    // 5. heights: `rounds` rounds; then the nodes in the order of their height
    uint32_t *h_in = sc->h_a, *h_out = sc->h_b;
    for (uint32_t r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(k_lbvh_height, dim3(lbvh_blocks(nb)), dim3(kLbvhBlock), 0, s, tg.kids, h_in, h_out, nb);
        uint32_t *t = h_in; h_in = h_out; h_out = t;
    }
    LBVH_TRY(hipGetLastError());
    LBVH_TRY(hipMemsetAsync(sc->hist, 0, kHistBins * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_lbvh_hist, dim3(lbvh_blocks(nb)), dim3(kLbvhBlock), 0, s, h_in, nb, sc->hist);
    LBVH_TRY(hipGetLastError());
    LBVH_TRY(sort_pairs(sc, h_in, sc->h_sorted, sc->iota, tg.order, nb, 7u, s));
    uint32_t hist[kHistBins], top = 0u;
    LBVH_TRY(hipMemcpyAsync(hist, sc->hist, sizeof(hist), hipMemcpyDeviceToHost, s));
    LBVH_TRY(hipMemcpyAsync(&top, h_in, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LBVH_TRY(hipStreamSynchronize(s));
    if (top >= kHistBins - 1u) return hipErrorUnknown;           // the rounds did not reach the root: the depth bound is broken
    res.class_start.assign(top + 2u, 0u);
    for (uint32_t h = 0; h <= top; ++h) res.class_start[h + 1u] = res.class_start[h] + hist[h];
    if (res.class_start[top + 1u] != nb) return hipErrorUnknown;
    // 6. exact boxes over the new table: refit.hip's kernels, one launch per height class
    RefitView rv{};
    rv.prim_slot = tg.prim_slot; rv.slot_prim = tg.slot_prim; rv.kids = tg.kids; rv.order = tg.order; rv.node_child = tg.node_child; rv.wide_child = tg.wide_child;
    rv.boxes = tg.boxes; rv.tri_pos = const_cast<float *>(tri_pos); rv.tris = tg.tris; rv.nodes = tg.nodes; rv.qnodes = tg.qnodes; rv.wnodes = tg.wnodes;
    for (uint32_t h = 0; h <= top; ++h)
        LBVH_TRY(launch_refit_boxes(rv, res.class_start[h], res.class_start[h + 1u] - res.class_start[h], h == 0u, s));
    // 7. BVH4: one wide level after the other, the size of the next read back
    uint32_t n_wide = 0u, wdepth = 1u;
    if (n_nodes) {
        LBVH_TRY(hipMemsetAsync(sc->wide_builder, 0, sizeof(int32_t), s));          // wide node 0 replaces builder node 0, the root
        uint32_t level_start = 0u, level_cnt = 1u;
        wdepth = 0u;
        while (level_cnt) {
            if (level_start + level_cnt > n_nodes || wdepth > 2u * kHistBins) return hipErrorUnknown;
            ++wdepth;
            const uint32_t next_start = level_start + level_cnt;
            hipLaunchKernelGGL(k_lbvh_collapse, dim3(lbvh_blocks(level_cnt)), dim3(kLbvhBlock), 0, s, tg.kids, tg.boxes, sc->wide_builder, level_start, level_cnt,
                               tg.wide_child, sc->cnt);
            LBVH_TRY(hipGetLastError());
            LBVH_TRY(scan(sc, sc->cnt, sc->offs, level_cnt + 1u, s));
            hipLaunchKernelGGL(k_lbvh_assign, dim3(lbvh_blocks(level_cnt)), dim3(kLbvhBlock), 0, s, tg.kids, tg.wide_child, sc->offs, level_start, level_cnt, next_start,
                               n_nodes, sc->ref4, sc->wide_builder);
            LBVH_TRY(hipGetLastError());
            uint32_t next_cnt = 0u;
            LBVH_TRY(hipMemcpyAsync(&next_cnt, sc->offs + level_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            LBVH_TRY(hipStreamSynchronize(s));
            level_start = next_start; level_cnt = next_cnt;
        }
        n_wide = level_start;
    }
    // 8. emission: references and absent children here, every box by refit.hip's kernel
    rv.n_nodes = n_nodes; rv.n_wide = n_wide;
    if (n_nodes) {
        hipLaunchKernelGGL(k_lbvh_refs, dim3(lbvh_blocks((uint64_t) n_nodes + 4ull * n_wide)), dim3(kLbvhBlock), 0, s, tg.node_child, tg.wide_child, sc->ref2, sc->ref4,
                           n_nodes, n_wide, tg.nodes, tg.qnodes, tg.wnodes);
        LBVH_TRY(hipGetLastError());
        LBVH_TRY(launch_refit_emit(rv, grid, s));
    }
    LBVH_TRY(hipStreamSynchronize(s));
    res.n_builder = nb; res.n_nodes = n_nodes; res.n_wide = n_wide; res.n_slots = n; res.depth = top + 1u; res.wdepth = wdepth;
    res.root = res.wroot = n_nodes ? 0u : (kLbvhLeafFlag | (n << 27));
    return hipSuccess;
}

hipError_t launch_lbvh_slots(const float *tri_pos, const uint32_t *slot_prim, uint32_t n, uint32_t *prim_slot, float4 *tris, hipStream_t s) {
    hipLaunchKernelGGL(k_lbvh_slots, dim3(lbvh_blocks(n)), dim3(kLbvhBlock), 0, s, tri_pos, slot_prim, n, prim_slot, tris);
    return hipGetLastError();
}

hipError_t launch_sah_partials(const int2 *kids, const float *boxes, uint32_t n_builder, int32_t root, double *partial, hipStream_t s) {
    if (n_builder == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sah_partials, dim3((n_builder + kSahBlock - 1u) / kSahBlock), dim3(kSahBlock), 0, s, kids, boxes, n_builder, root, partial);
    return hipGetLastError();
}

} // namespace mtsamd

// sah_build.hip -- device binned-SAH build for gfx950 (sah_build.h): build_sah_levels of bvh.h, level by level.  Per level one launch
// decides every active node (node box and centroid box by a reduction, 3 x 16 bins in LDS updated with 32-bit integer min / max / add
// only, the search of sah_keys.h, then the stable partition of the node's part of `perm` into the other buffer), one scan numbers the
// children, the BVH2 nodes and the leaf slots, one launch writes them; the host reads the size of the next level back.  As in lbvh.hip
// the kernel boundary is the only synchronisation: no thread waits on another workgroup and nothing is handed between workgroups inside a
// launch.  Integer min / max / add are order-free and double min / max are exact, so the result does not depend on the schedule.  Every
// per-element step is a function of sah_keys.h, which the host specification calls too.  The build has -ffp-contract=off.
#include <chrono>
#include <rocprim/device/device_scan.hpp>

#include "sah_build.h"
#include "sah_keys.h"

namespace mtsamd {

struct SahScratch {
    uint32_t n = 0;                                             // primitives the arrays are sized for
    uint32_t *perm[2] = { nullptr, nullptr };                   // n each: the primitives of the level's nodes, and of the next level's
    uint32_t *first[2] = { nullptr, nullptr }, *count[2] = { nullptr, nullptr };      // n each: the nodes of the level, and of the next
    uint32_t *left = nullptr;                                   // n: primitives of the left child of a split node
    unsigned long long *made = nullptr, *made_scan = nullptr;   // n + 1 each: (1 << 32) of a split node, the count of a leaf; their scan
    void *tmp = nullptr; size_t tmp_bytes = 0;                  // rocPRIM's
    std::vector<float> level_ms;
    std::vector<uint32_t> level_nodes;
};

namespace {

constexpr uint32_t kSahWg = 256u, kWave = 64u, kWaves = kSahWg / kWave;
inline uint32_t sah_blocks(uint64_t n) { return (uint32_t) ((n + kSahWg - 1u) / kSahWg); }

struct SahLds {
    SahBins bins[kWaves];              // one per wave (small nodes); a large node uses the first
    double cbox[kWaves][6];            // per wave: its part of the centroid box
    float nbox[kWaves][6];             // ... and of the node box
    uint32_t part[2][kWaves][2];       // partition of a large node: per chunk parity and wave, (left, right) of the chunk
};

__global__ void __launch_bounds__(kSahWg) k_sah_iota(uint32_t *__restrict__ perm, uint32_t *__restrict__ first, uint32_t *__restrict__ count, uint32_t n) {
    const uint32_t i = blockIdx.x * kSahWg + threadIdx.x;
    if (i < n) perm[i] = i;
    if (i == 0) { first[0] = 0u; count[0] = n; }
}

struct SahLevel {
    const float *tri_pos;
    const uint32_t *perm_in; uint32_t *perm_out;
    const uint32_t *first, *count;
    uint32_t *left;
    unsigned long long *made;
    uint32_t n, m, depth, max_leaf, per_wg;
};

// One node [first, first + count) of perm_in, decided by a team: the whole workgroup (BLOCK) or the caller's wave, whose lanes are
// `active` or not as one.  Every thread of the workgroup calls this, and meets the same barriers.
template <bool BLOCK> __device__ void sah_node(SahLds &lds, const SahLevel &lv, bool active, uint32_t j, uint32_t first, uint32_t count) {
    const uint32_t tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const uint32_t ti = BLOCK ? tid : lane, ts = BLOCK ? kSahWg : kWave;
    SahBins &bins = lds.bins[BLOCK ? 0u : wave];
    __syncthreads();                                            // whoever read these bins for the node before is done
    // node box and centroid box: per thread, per wave, then over the team's waves
    float nb[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    double cb[6] = { DBL_MAX, DBL_MAX, DBL_MAX, -DBL_MAX, -DBL_MAX, -DBL_MAX };
    if (active) {
        uint32_t *w = reinterpret_cast<uint32_t *>(&bins);
        for (uint32_t i = ti; i < kSahBinWords; i += ts) w[i] = i < 9u * kSahBins ? 0xffffffffu : 0u;
        for (uint32_t i = ti; i < count; i += ts) {
            const uint32_t p = lv.perm_in[first + i];
            if (p >= lv.n) continue;
            float tp[9], lo[3], hi[3]; double c[3];
            for (int q = 0; q < 9; ++q) tp[q] = lv.tri_pos[9 * (size_t) p + q];
            sah_prim(tp, lo, hi, c);
            for (int k = 0; k < 3; ++k) {
                nb[k] = fminf(nb[k], lo[k]); nb[3 + k] = fmaxf(nb[3 + k], hi[k]);
                cb[k] = fmin(cb[k], c[k]); cb[3 + k] = fmax(cb[3 + k], c[k]);
            }
        }
    }
    for (uint32_t d = kWave / 2u; d > 0u; d /= 2u)
        for (int k = 0; k < 3; ++k) {
            nb[k] = fminf(nb[k], __shfl_xor(nb[k], (int) d)); nb[3 + k] = fmaxf(nb[3 + k], __shfl_xor(nb[3 + k], (int) d));
            cb[k] = fmin(cb[k], __shfl_xor(cb[k], (int) d)); cb[3 + k] = fmax(cb[3 + k], __shfl_xor(cb[3 + k], (int) d));
        }
    if (lane == 0u)
        for (int k = 0; k < 6; ++k) { lds.nbox[wave][k] = nb[k]; lds.cbox[wave][k] = cb[k]; }
    __syncthreads();
    // from the stored parts alone, in one order: every thread of the team holds the same bits
    for (int k = 0; k < 3; ++k) { nb[k] = INFINITY; nb[3 + k] = -INFINITY; cb[k] = DBL_MAX; cb[3 + k] = -DBL_MAX; }
    for (uint32_t w = BLOCK ? 0u : wave; w < (BLOCK ? kWaves : wave + 1u); ++w)
            for (int k = 0; k < 3; ++k) {
                nb[k] = fminf(nb[k], lds.nbox[w][k]); nb[3 + k] = fmaxf(nb[3 + k], lds.nbox[w][3 + k]);
                cb[k] = fmin(cb[k], lds.cbox[w][k]); cb[3 + k] = fmax(cb[3 + k], lds.cbox[w][3 + k]);
            }
    // bins: 32-bit integer min / max / add in LDS
    if (active && count > 1u) {
        double scale[3]; bool open[3];
        for (int a = 0; a < 3; ++a) { const double ext = cb[3 + a] - cb[a]; open[a] = ext > 0.0; scale[a] = open[a] ? sah_scale(ext) : 0.0; }
        for (uint32_t i = ti; i < count; i += ts) {
            const uint32_t p = lv.perm_in[first + i];
            if (p >= lv.n) continue;
            float tp[9], lo[3], hi[3]; double c[3];
            for (int q = 0; q < 9; ++q) tp[q] = lv.tri_pos[9 * (size_t) p + q];
            sah_prim(tp, lo, hi, c);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!open[a]) continue;
                const int b = sah_bin(c[a], cb[a], scale[a]);
                for (int k = 0; k < 3; ++k) { atomicMin(&bins.lo[a][b][k], sah_ord(lo[k])); atomicMax(&bins.hi[a][b][k], sah_ord(hi[k])); }
                atomicAdd(&bins.cnt[a][b], 1u);
            }
        }
    }
    __syncthreads();
    // the search and the decision: every thread of the team, from the same words
    int axis = -1, bin = -1; double cost = DBL_MAX;
    uint32_t mode = kSahLeaf, nl = 0u;
    if (active && count > 1u) {
        sah_choose(bins, cb, cb + 3, lbvh_area(nb), &axis, &bin, &cost);
        mode = sah_decide(count, lv.max_leaf, lv.depth, axis, cost);
        if (mode != kSahLeaf) nl = sah_left_count(bins, count, &mode, axis, bin);
    }
    if (active && ti == 0u) {
        lv.made[j] = mode == kSahLeaf ? (unsigned long long) count : (1ull << 32);
        lv.left[j] = nl;
    }
    // the children's primitives, in the present order on either side
    if (mode == kSahSplitMiddle) {
        for (uint32_t i = ti; i < count; i += ts) lv.perm_out[first + i] = lv.perm_in[first + i];
    } else if (mode == kSahSplitBin) {
        const double lo = axis == 0 ? cb[0] : (axis == 1 ? cb[1] : cb[2]), hi = axis == 0 ? cb[3] : (axis == 1 ? cb[4] : cb[5]);
        const double scale = sah_scale(hi - lo);
        const unsigned long long below = (1ull << lane) - 1ull;
        uint32_t lbase = 0u, rbase = 0u, parity = 0u;
        for (uint32_t base = 0; base < count; base += ts, parity ^= 1u) {
            const uint32_t i = base + ti;
            bool valid = i < count;
            uint32_t p = 0u;
            if (valid) { p = lv.perm_in[first + i]; valid = p < lv.n; }
            bool goes_left = false;
            if (valid) {
                const float tp[9] = { lv.tri_pos[9 * (size_t) p + axis], 0.0f, 0.0f, lv.tri_pos[9 * (size_t) p + 3 + axis], 0.0f, 0.0f, lv.tri_pos[9 * (size_t) p + 6 + axis], 0.0f, 0.0f };
                goes_left = sah_bin(sah_centroid_axis(tp, 0), lo, scale) <= bin;
            }
            const unsigned long long lmask = __ballot(goes_left), rmask = __ballot(valid && !goes_left);
            uint32_t lrank = (uint32_t) __popcll(lmask & below), rrank = (uint32_t) __popcll(rmask & below);
            uint32_t ltot = (uint32_t) __popcll(lmask), rtot = (uint32_t) __popcll(rmask);
            if (BLOCK) {
                if (lane == 0u) { lds.part[parity][wave][0] = ltot; lds.part[parity][wave][1] = rtot; }
                __syncthreads();
                ltot = 0u; rtot = 0u;
                for (uint32_t w = 0; w < kWaves; ++w) {
                    if (w < wave) { lrank += lds.part[parity][w][0]; rrank += lds.part[parity][w][1]; }
                    ltot += lds.part[parity][w][0]; rtot += lds.part[parity][w][1];
                }
            }
            const uint32_t at = goes_left ? lbase + lrank : nl + rbase + rrank;
            if (valid && at < count) lv.perm_out[first + at] = p;
            lbase += ltot; rbase += rtot;
        }
    }
}

// One launch decides every node of a level.  Workgroup b has nodes [b * per_wg, (b + 1) * per_wg), per_wg = 1 or 4.
__global__ void __launch_bounds__(kSahWg) k_sah_decide(SahLevel lv) {
    __shared__ SahLds lds;
    const uint32_t base = blockIdx.x * lv.per_wg, wave = threadIdx.x / kWave;
    if (blockIdx.x == 0u && threadIdx.x == 0u) lv.made[lv.m] = 0ull;
    // a range that does not lie in [0, n) is no node: it makes nothing, and the host's sums then miss n
    auto in_range = [&](uint32_t j) { const uint32_t f = lv.first[j], c = lv.count[j]; return c >= 1u && f < lv.n && c <= lv.n - f; };
    {   // the small nodes side by side, one wave each
        const uint32_t j = base + wave;
        const bool mine = wave < lv.per_wg && j < lv.m;
        const bool good = mine && in_range(j);
        if (mine && !good && threadIdx.x % kWave == 0u) { lv.made[j] = 0ull; lv.left[j] = 0u; }
        const uint32_t count = good ? lv.count[j] : 0u;
        const bool active = good && count <= kSahWaveNode;
        sah_node<false>(lds, lv, active, j, active ? lv.first[j] : 0u, active ? count : 0u);
    }
    for (uint32_t k = 0; k < lv.per_wg; ++k) {         // the large ones one after the other: j and count are the same in every thread
        const uint32_t j = base + k;
        if (j >= lv.m) break;
        if (!in_range(j)) continue;
        const uint32_t count = lv.count[j];
        if (count <= kSahWaveNode) continue;
        sah_node<true>(lds, lv, true, j, lv.first[j], count);
    }
}

struct SahWrite {
    const uint32_t *perm, *first, *count, *left;
    const unsigned long long *made, *made_scan;
    uint32_t *next_first, *next_count;
    int2 *kids; int32_t *node_child;
    uint32_t *ref2, *ref4, *height, *slot_prim;
    uint32_t n, m, level_base, next_base, inner_base, slot_base;
};

// one thread per node of the level: a split node writes its children, a leaf its slots
__global__ void __launch_bounds__(kSahWg) k_sah_write(SahWrite a) {
    const uint32_t j = blockIdx.x * kSahWg + threadIdx.x;
    if (j >= a.m) return;
    const uint32_t t = a.level_base + j, first = a.first[j], count = a.count[j];
    const unsigned long long before = a.made_scan[j];
    const uint32_t r = (uint32_t) (before >> 32), off = (uint32_t) before;
    if (t >= 2u * a.n - 1u || count == 0u || first >= a.n || count > a.n - first) return;
    if (a.made[j] >> 32) {
        const uint32_t l = a.next_base + 2u * r, b2 = a.inner_base + r, nl = a.left[j];
        if (l + 1u >= 2u * a.n - 1u || b2 + 1u >= a.n || 2u * r + 1u >= a.n || nl == 0u || nl >= count) return;
        a.kids[t] = make_int2((int32_t) l, (int32_t) l + 1);
        a.node_child[2 * (size_t) b2] = (int32_t) l; a.node_child[2 * (size_t) b2 + 1] = (int32_t) l + 1;
        a.ref2[t] = b2; a.ref4[t] = t == 0u ? 0u : 0xffffffffu;
        a.height[t] = kLbvhNoHeight;
        a.next_first[2u * r] = first; a.next_count[2u * r] = nl;
        a.next_first[2u * r + 1u] = first + nl; a.next_count[2u * r + 1u] = count - nl;
    } else {
        const uint32_t s0 = a.slot_base + off;
        if (count > 15u || (uint64_t) s0 + count > a.n) return;
        const uint32_t ref = kLbvhLeafFlag | (count << 27) | s0;
        a.kids[t] = make_int2(-1, (int32_t) ref);
        a.ref2[t] = ref; a.ref4[t] = ref;
        a.height[t] = 0u;
        for (uint32_t i = 0; i < count; ++i) a.slot_prim[s0 + i] = a.perm[first + i];
    }
}

#define SAH_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

template <typename T> hipError_t alloc(T **p, size_t count) { return hipMalloc((void **) p, sizeof(T) * (count ? count : 1)); }

} // namespace

void sah_scratch_destroy(SahScratch *sc) {
    if (!sc) return;
    void *all[] = { sc->perm[0], sc->perm[1], sc->first[0], sc->first[1], sc->count[0], sc->count[1], sc->left, sc->made, sc->made_scan, sc->tmp };
    for (void *p : all) (void) hipFree(p);
    delete sc;
}

hipError_t sah_scratch_create(uint32_t n, SahScratch **out) {
    *out = nullptr;
    if (n == 0) return hipErrorInvalidValue;
    SahScratch *sc = new SahScratch();
    sc->n = n;
    hipError_t e = hipSuccess;
    auto ok = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    for (int k = 0; k < 2; ++k) { ok(alloc(&sc->perm[k], n)); ok(alloc(&sc->first[k], n)); ok(alloc(&sc->count[k], n)); }
    ok(alloc(&sc->left, n)); ok(alloc(&sc->made, (size_t) n + 1)); ok(alloc(&sc->made_scan, (size_t) n + 1));
    size_t bytes = 0;
    unsigned long long *u = nullptr;
    if (e == hipSuccess) ok(rocprim::exclusive_scan(nullptr, bytes, u, u, 0ull, (size_t) n + 1, rocprim::plus<unsigned long long>(), (hipStream_t) nullptr));
    if (e == hipSuccess) { sc->tmp_bytes = 2 * bytes + 65536; ok(hipMalloc(&sc->tmp, sc->tmp_bytes)); }       // slack: a level's scan is of any smaller size
    if (e != hipSuccess) { sah_scratch_destroy(sc); return e; }
    *out = sc;
    return hipSuccess;
}

const std::vector<float> &sah_level_ms(const SahScratch *sc) { return sc->level_ms; }
const std::vector<uint32_t> &sah_level_nodes(const SahScratch *sc) { return sc->level_nodes; }

hipError_t sah_build(SahScratch *sc, LbvhScratch *tail, const float *tri_pos, uint32_t n, uint32_t max_leaf, const RefitGrid &grid, const LbvhTarget &tg,
                     LbvhResult &res, hipStream_t s) {
    if (!sc || !tail || n == 0 || n > sc->n || n > tail->n || n >= (1u << 27)) return hipErrorInvalidValue;
    max_leaf = max_leaf < 1u ? 1u : (max_leaf > 15u ? 15u : max_leaf);
    sc->level_ms.clear(); sc->level_nodes.clear();
    hipLaunchKernelGGL(k_sah_iota, dim3(sah_blocks(n)), dim3(kSahWg), 0, s, sc->perm[0], sc->first[0], sc->count[0], n);
    SAH_TRY(hipGetLastError());
    // the depth bound of build_sah_levels: the guard halves every node from depth 40 on
    uint32_t max_levels = kSahGuardDepth + 2u;
    while ((1ull << (max_levels - kSahGuardDepth - 2u)) < n) ++max_levels;
    uint32_t m = 1u, level_base = 0u, n_inner = 0u, n_slots = 0u, levels = 0u;
    int cur = 0;
    while (m) {
        const auto t0 = std::chrono::steady_clock::now();
        if (levels >= max_levels) return hipErrorUnknown;
        SahLevel lv{};
        lv.tri_pos = tri_pos; lv.perm_in = sc->perm[cur]; lv.perm_out = sc->perm[cur ^ 1]; lv.first = sc->first[cur]; lv.count = sc->count[cur];
        lv.left = sc->left; lv.made = sc->made; lv.n = n; lv.m = m; lv.depth = levels; lv.max_leaf = max_leaf;
        lv.per_wg = m >= kSahShareLevel ? kWaves : 1u;
        hipLaunchKernelGGL(k_sah_decide, dim3((m + lv.per_wg - 1u) / lv.per_wg), dim3(kSahWg), 0, s, lv);
        SAH_TRY(hipGetLastError());
        size_t bytes = sc->tmp_bytes;
        SAH_TRY(rocprim::exclusive_scan(sc->tmp, bytes, sc->made, sc->made_scan, 0ull, (size_t) m + 1u, rocprim::plus<unsigned long long>(), s));
        unsigned long long total = 0ull;
        SAH_TRY(hipMemcpyAsync(&total, sc->made_scan + m, sizeof(total), hipMemcpyDeviceToHost, s));
        SAH_TRY(hipStreamSynchronize(s));
        // what the level made, against the bounds of n primitives, before any of it sizes a launch or an index
        const uint64_t n_split = total >> 32, n_leaf_prims = total & 0xffffffffull;
        const uint64_t next_base = (uint64_t) level_base + m;
        if (n_split > m || next_base + 2u * n_split > 2ull * n - 1ull || n_inner + n_split > (uint64_t) n - 1u || n_slots + n_leaf_prims > n || 2u * n_split > n)
            return hipErrorUnknown;
        SahWrite w{};
        w.perm = sc->perm[cur]; w.first = sc->first[cur]; w.count = sc->count[cur]; w.left = sc->left; w.made = sc->made; w.made_scan = sc->made_scan;
        w.next_first = sc->first[cur ^ 1]; w.next_count = sc->count[cur ^ 1]; w.kids = tg.kids; w.node_child = tg.node_child;
        w.ref2 = tail->ref2; w.ref4 = tail->ref4; w.height = tail->h_a; w.slot_prim = tg.slot_prim;
        w.n = n; w.m = m; w.level_base = level_base; w.next_base = (uint32_t) next_base; w.inner_base = n_inner; w.slot_base = n_slots;
        hipLaunchKernelGGL(k_sah_write, dim3(sah_blocks(m)), dim3(kSahWg), 0, s, w);
        SAH_TRY(hipGetLastError());
        sc->level_nodes.push_back(m);
        sc->level_ms.push_back(std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count());
        level_base = (uint32_t) next_base; n_inner += (uint32_t) n_split; n_slots += (uint32_t) n_leaf_prims;
        m = 2u * (uint32_t) n_split;
        cur ^= 1; ++levels;
    }
    const uint32_t nb = level_base;
    if (n_slots != n || nb != 2u * n_inner + 1u) return hipErrorUnknown;
    SAH_TRY(launch_lbvh_slots(tri_pos, tg.slot_prim, n, tg.prim_slot, tg.tris, s));
    return lbvh_finish(tail, tri_pos, n, nb, n_inner, levels, grid, tg, res, s);
}

} // namespace mtsamd

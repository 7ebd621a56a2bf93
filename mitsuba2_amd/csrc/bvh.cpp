// bvh.cpp -- binned-SAH BVH2 builder (host).  See bvh.h.
#include "bvh.h"
#include "refit_encode.h"
#include "lbvh_keys.h"
#include "sah_keys.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <queue>

namespace mtsamd {
namespace {

constexpr uint32_t kLeafFlag = 0x80000000u;
constexpr uint32_t kLeafCountShift = 27;
constexpr int kMaxBins = 64;
constexpr double kTraversalCost = 1.0;

struct Box {
    double lo[3], hi[3];
    void reset() { for (int k = 0; k < 3; ++k) { lo[k] = DBL_MAX; hi[k] = -DBL_MAX; } }
    void grow(const Box &b) { for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], b.lo[k]); hi[k] = std::max(hi[k], b.hi[k]); } }
    void grow(const double *p) { for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], p[k]); hi[k] = std::max(hi[k], p[k]); } }
    double area() const {
        double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        if (dx < 0) return 0.0;
        return 2.0 * (dx * dy + dy * dz + dz * dx);
    }
};

struct TmpNode {
    Box box;
    int32_t left = -1, right = -1;   // children (TmpNode indices) or -1
    uint32_t first = 0, count = 0;   // leaf range in the permuted primitive list
    uint32_t depth = 0;
};

struct Builder {
    const float *tri_pos;
    uint32_t n_prims, max_leaf;
    std::vector<Box> prim_box;
    std::vector<double> centroid;    // 3 per prim
    std::vector<uint32_t> perm;
    std::vector<TmpNode> nodes;
    uint32_t max_depth = 0;
    int kBins = 16;                   // BvhOptions
    double kIntersectCost = 1.5;
    uint32_t sweep_below = 0;
    std::vector<uint32_t> scratch;
    std::vector<double> suffix_area;

    int32_t build(uint32_t first, uint32_t count, uint32_t depth) {
        int32_t idx = (int32_t) nodes.size();
        nodes.emplace_back();
        TmpNode n;
        n.depth = depth;
        n.box.reset();
        Box cb; cb.reset();
        for (uint32_t i = 0; i < count; ++i) {
            uint32_t p = perm[first + i];
            n.box.grow(prim_box[p]);
            cb.grow(&centroid[3 * p]);
        }
        max_depth = std::max(max_depth, depth);
        auto make_leaf = [&]() { n.first = first; n.count = count; nodes[idx] = n; return idx; };
        if (count <= 1) return make_leaf();

        // binned SAH over the three axes
        double best_cost = DBL_MAX; int best_axis = -1, best_bin = -1;
        double parent_area = std::max(n.box.area(), 1e-300);
        for (int axis = 0; axis < 3; ++axis) {
            double lo = cb.lo[axis], ext = cb.hi[axis] - cb.lo[axis];
            if (!(ext > 0.0)) continue;
            Box bin_box[kMaxBins]; uint32_t bin_cnt[kMaxBins];
            for (int b = 0; b < kBins; ++b) { bin_box[b].reset(); bin_cnt[b] = 0; }
            double scale = kBins / ext;
            for (uint32_t i = 0; i < count; ++i) {
                uint32_t p = perm[first + i];
                int b = std::min(kBins - 1, std::max(0, (int) ((centroid[3 * p + axis] - lo) * scale)));
                bin_box[b].grow(prim_box[p]); bin_cnt[b]++;
            }
            double right_area[kMaxBins]; uint32_t right_cnt[kMaxBins];
            Box acc; acc.reset(); uint32_t cnt = 0;
            for (int b = kBins - 1; b > 0; --b) {
                if (bin_cnt[b]) acc.grow(bin_box[b]);
                cnt += bin_cnt[b];
                right_area[b] = cnt ? acc.area() : 0.0; right_cnt[b] = cnt;
            }
            acc.reset(); cnt = 0;
            for (int b = 0; b < kBins - 1; ++b) {
                if (bin_cnt[b]) acc.grow(bin_box[b]);
                cnt += bin_cnt[b];
                if (cnt == 0 || right_cnt[b + 1] == 0) continue;
                double cost = kTraversalCost +
                              kIntersectCost * (acc.area() * cnt + right_area[b + 1] * right_cnt[b + 1]) / parent_area;
                if (cost < best_cost) { best_cost = cost; best_axis = axis; best_bin = b; }
            }
        }
        // small nodes: the exact SAH sweep over every split position of every axis (centroid order) instead of the bins
        int sweep_axis = -1; uint32_t sweep_left = 0;
        if (count <= sweep_below) {
            best_cost = DBL_MAX;
            scratch.resize(count); suffix_area.resize(count + 1);
            for (int axis = 0; axis < 3; ++axis) {
                for (uint32_t i = 0; i < count; ++i) scratch[i] = perm[first + i];
                std::sort(scratch.begin(), scratch.end(), [&](uint32_t a, uint32_t b) {
                    const double ca = centroid[3 * a + axis], cbb = centroid[3 * b + axis];
                    return ca < cbb || (ca == cbb && a < b);
                });
                Box acc; acc.reset();
                for (uint32_t i = count; i-- > 0;) { acc.grow(prim_box[scratch[i]]); suffix_area[i] = acc.area(); }
                acc.reset();
                for (uint32_t i = 0; i + 1 < count; ++i) {
                    acc.grow(prim_box[scratch[i]]);
                    const double cost = kTraversalCost + kIntersectCost * (acc.area() * (i + 1) + suffix_area[i + 1] * (count - i - 1)) / parent_area;
                    if (cost < best_cost) { best_cost = cost; sweep_axis = axis; sweep_left = i + 1; }
                }
            }
            if (sweep_axis >= 0) best_axis = 3;                 // marks "sweep split chosen"
        }
        double leaf_cost = kIntersectCost * count;
        if (count <= max_leaf && (best_axis < 0 || leaf_cost <= best_cost)) return make_leaf();

        // Depth guard: the traversal kernels keep a per-lane stack of `depth` entries in LDS (<= 64 KB per 256-thread workgroup).
        // Past depth 40 the split is an object median along the widest centroid axis, which bounds the total depth by
        // 40 + log2(n) whatever the SAH would have done on a pathological primitive distribution.
        if (depth >= 40 && best_axis >= 0) {
            int axis = 0;
            for (int k = 1; k < 3; ++k) if (cb.hi[k] - cb.lo[k] > cb.hi[axis] - cb.lo[axis]) axis = k;
            std::nth_element(perm.begin() + first, perm.begin() + first + count / 2, perm.begin() + first + count,
                             [&](uint32_t a, uint32_t b) { return centroid[3 * a + axis] < centroid[3 * b + axis]; });
            best_axis = -2;
        }
        uint32_t mid;
        if (best_axis == -2) {
            mid = first + count / 2;
        } else if (best_axis == 3) {
            std::sort(perm.begin() + first, perm.begin() + first + count, [&](uint32_t a, uint32_t b) {
                const double ca = centroid[3 * a + sweep_axis], cbb = centroid[3 * b + sweep_axis];
                return ca < cbb || (ca == cbb && a < b);
            });
            mid = first + sweep_left;
        } else if (best_axis >= 0) {
            double lo = cb.lo[best_axis], ext = cb.hi[best_axis] - cb.lo[best_axis];
            double scale = kBins / ext;
            auto it = std::partition(perm.begin() + first, perm.begin() + first + count, [&](uint32_t p) {
                int b = std::min(kBins - 1, std::max(0, (int) ((centroid[3 * p + best_axis] - lo) * scale)));
                return b <= best_bin;
            });
            mid = (uint32_t) (it - perm.begin());
        } else {
            // all centroids coincide: split by index
            std::sort(perm.begin() + first, perm.begin() + first + count);
            mid = first + count / 2;
        }
        if (mid == first || mid == first + count) mid = first + count / 2;
        nodes[idx] = n;
        int32_t l = build(first, mid - first, depth + 1);
        int32_t r = build(mid, first + count - mid, depth + 1);
        nodes[idx].left = l; nodes[idx].right = r;
        return idx;
    }
};

// outward-rounded, padded float bounds: the slab test must never cull a triangle that the fp32
// Moeller-Trumbore test (mesh.h:195-221) would accept.
inline void padded(const Box &b, double scene_extent, float lo[3], float hi[3]) {
    for (int k = 0; k < 3; ++k) {
        double pad = 1e-5 * std::max({ std::fabs(b.lo[k]), std::fabs(b.hi[k]), b.hi[k] - b.lo[k] }) +
                     1e-7 * scene_extent + 1e-30;
        lo[k] = std::nextafter((float) (b.lo[k] - pad), -INFINITY);
        hi[k] = std::nextafter((float) (b.hi[k] + pad), INFINITY);
    }
}

inline float bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

} // namespace

void scene_grid(const float bbox[6], double *extent_out, float q_lo[3], float q_step[3]) {
    double extent = 0.0;
    for (int k = 0; k < 3; ++k) extent = std::max({ extent, std::fabs((double) bbox[k]), std::fabs((double) bbox[3 + k]), (double) bbox[3 + k] - (double) bbox[k] });
    for (int k = 0; k < 3; ++k) {
        const double lo = bbox[k], hi = bbox[3 + k];
        const double pad = (hi - lo + extent + 1.0) * 1e-5;
        const double glo = lo - pad;
        // the padded scene box ends at cell 65532: every snapped plane stays below 65534, so that the 15-bit variant of the BVH4
        // nodes (even cells only) can round a far plane up without leaving the grid
        const double gstep = std::max((hi + pad - glo) / 65532.0, 1e-30);
        q_lo[k] = (float) glo; q_step[k] = (float) gstep;
    }
    *extent_out = extent;
}

// ---- emission: from the exact box of every builder node (RefitTable::boxes) to everything the device reads.  build_bvh and refit_bvh
// both end here; csrc/refit.hip restates it per node, operation by operation, and is held to the same bytes.
static void emit_bvh(const float *tri_pos, BvhOutput &out) {
    const RefitTable &rt = out.refit;
    auto box_of = [&](int32_t t) { Box bx; for (int k = 0; k < 3; ++k) { bx.lo[k] = rt.boxes[6 * (size_t) t + k]; bx.hi[k] = rt.boxes[6 * (size_t) t + 3 + k]; } return bx; };
    for (int k = 0; k < 6; ++k) out.bbox[k] = rt.boxes[6 * (size_t) rt.root + k];
    double extent;
    scene_grid(out.bbox, &extent, out.q_lo, out.q_step);
    const size_t n_nodes = rt.node_child.size() / 2, n_wide = rt.wide_child.size() / 4, n_slots = rt.slot_prim.size();
    out.tris.resize(12 * n_slots);
    for (size_t s = 0; s < n_slots; ++s) {
        const uint32_t p = rt.slot_prim[s];
        const float *tp = tri_pos + 9 * (size_t) p;
        float p0[3] = { tp[0], tp[1], tp[2] };
        float e1[3] = { tp[3] - tp[0], tp[4] - tp[1], tp[5] - tp[2] };
        float e2[3] = { tp[6] - tp[0], tp[7] - tp[1], tp[8] - tp[2] };
        float rec[12] = { p0[0], p0[1], p0[2], e1[0], e1[1], e1[2], e2[0], e2[1], e2[2], bits(p), 0.0f, 0.0f };
        std::memcpy(out.tris.data() + 12 * s, rec, sizeof(rec));
    }
    out.nodes.assign(16 * n_nodes, 0.0f);
    for (size_t i = 0; i < n_nodes; ++i) {
        const int32_t l = rt.node_child[2 * i], r = rt.node_child[2 * i + 1];
        float llo[3], lhi[3], rlo[3], rhi[3];
        padded(box_of(l), extent, llo, lhi);
        padded(box_of(r), extent, rlo, rhi);
        float *q = out.nodes.data() + 16 * i;
        q[0] = llo[0]; q[1] = llo[1]; q[2] = llo[2]; q[3] = lhi[0];
        q[4] = lhi[1]; q[5] = lhi[2]; q[6] = rlo[0]; q[7] = rlo[1];
        q[8] = rlo[2]; q[9] = rhi[0]; q[10] = rhi[1]; q[11] = rhi[2];
        q[12] = bits(rt.ref2[l]); q[13] = bits(rt.ref2[r]); q[14] = 0.0f; q[15] = 0.0f;
    }
    // 32-byte nodes: child boxes snapped outward (by at least 1/8 cell: the device decodes them with an error below 0.07 cells)
    // to a 65536^3 grid over the (padded) scene box.  One traversal step then costs two
    // 16-byte loads per lane instead of four; the walk only culls with the boxes, so hits are unchanged.
    // the device decodes with the float values: they are the reference for the snapping below
    double glo[3], gstep[3];
    for (int k = 0; k < 3; ++k) { glo[k] = (double) out.q_lo[k]; gstep[k] = (double) out.q_step[k]; }
    auto qlo = [&](float v, int k) -> uint32_t {
        double q = std::floor(((double) v - glo[k]) / gstep[k] - 0.125);
        return (uint32_t) std::min(65535.0, std::max(0.0, q));
    };
    auto qhi = [&](float v, int k) -> uint32_t {
        double q = std::ceil(((double) v - glo[k]) / gstep[k] + 0.125);
        return (uint32_t) std::min(65535.0, std::max(0.0, q));
    };
    out.qnodes.assign(8 * n_nodes, 0u);
    for (size_t i = 0; i < n_nodes; ++i) {
        const float *q = out.nodes.data() + 16 * i;
        const float llo[3] = { q[0], q[1], q[2] }, lhi[3] = { q[3], q[4], q[5] }, rlo[3] = { q[6], q[7], q[8] }, rhi[3] = { q[9], q[10], q[11] };
        uint32_t *w = out.qnodes.data() + 8 * i;
        // one word per child and axis: lo | hi << 16 (the walk swaps the halves with one v_perm_b32 according to the sign
        // of the ray direction and so gets (near plane, far plane) without min / max)
        for (int k = 0; k < 3; ++k) {
            w[k] = qlo(llo[k], k) | (qhi(lhi[k], k) << 16);
            w[3 + k] = qlo(rlo[k], k) | (qhi(rhi[k], k) << 16);
        }
        std::memcpy(&w[6], &q[12], 4); std::memcpy(&w[7], &q[13], 4);
    }
    // ---- BVH4, same grid
    out.wnodes.clear(); out.wnodes_h.clear(); out.wnodes_p.clear();
    if (n_wide == 0) return;
    // fp16 with directed rounding: the largest half <= v / the smallest half >= v (v an integer in [-32768, 32768])
    auto half_of = [](float v, bool up) -> uint32_t {
        uint32_t sign = v < 0.0f ? 0x8000u : 0u;
        float a = std::fabs(v);
        if (a == 0.0f) return sign;
        int e; float m = std::frexp(a, &e);                       // a = m 2^e, m in [0.5, 1)
        // 11 significant bits: a = k 2^(e - 11), k in [1024, 2048)
        const float scaled = std::ldexp(m, 11);
        const bool away = (v >= 0.0f) == up;                       // towards +inf of a positive / -inf of a negative value: magnitude up
        float k = away ? std::ceil(scaled) : std::floor(scaled);
        if (k >= 2048.0f) { k = 1024.0f; ++e; }
        const int be = e - 1 + 15;                                // biased exponent of k 2^(e - 11) = (k / 1024) 2^(e - 1)
        return sign | ((uint32_t) be << 10) | ((uint32_t) k - 1024u);
    };
    // wnodes_p: 15-bit planes on the even cells of the same grid, stored as 0x8000 | q15: the two bytes are the upper mantissa (and the
    // lowest exponent bit) of the float 65536 + 2 q15, which the walk assembles with one v_perm_b32 per plane -- no integer-to-float convert
    out.wnodes_h.assign(16 * n_wide, 0u); out.wnodes_p.assign(16 * n_wide, 0u); out.wnodes.assign(16 * n_wide, 0u);
    for (size_t i = 0; i < n_wide; ++i) {
        uint32_t *wh = out.wnodes_h.data() + 16 * i, *wp = out.wnodes_p.data() + 16 * i, *w = out.wnodes.data() + 16 * i;
        for (int c = 0; c < 4; ++c) {
            const int32_t t = rt.wide_child[4 * i + c];
            if (t < 0) {
                wh[4 * c] = wh[4 * c + 1] = wh[4 * c + 2] = 0x7800u | (0xf800u << 16);      // lo = +32768, hi = -32768
                wp[4 * c] = wp[4 * c + 1] = wp[4 * c + 2] = 0xffffu | (0x8000u << 16);      // lo = 65534, hi = 0
                w[4 * c] = w[4 * c + 1] = w[4 * c + 2] = 65535u;                            // lo = 65535, hi = 0
                wh[4 * c + 3] = wp[4 * c + 3] = w[4 * c + 3] = 0x7fffffffu;
                continue;
            }
            float lo[3], hi[3];
            padded(box_of(t), extent, lo, hi);
            for (int k = 0; k < 3; ++k) {
                const uint32_t ql = qlo(lo[k], k), qh = qhi(hi[k], k);
                const float vlo = (float) ql - 32768.0f, vhi = (float) qh - 32768.0f;
                wh[4 * c + k] = half_of(vlo, false) | (half_of(vhi, true) << 16);
                const uint32_t l15 = ql >> 1, h15 = std::min(32767u, (qh + 1u) >> 1);      // qhi <= 65534 (grid above)
                wp[4 * c + k] = (0x8000u | l15) | ((0x8000u | h15) << 16);
                w[4 * c + k] = ql | (qh << 16);
            }
            wh[4 * c + 3] = wp[4 * c + 3] = w[4 * c + 3] = rt.ref4[t];
        }
    }
}

void refit_bvh(const float *tri_pos, BvhOutput &out) {
    RefitTable &rt = out.refit;
    if (rt.order.empty()) return;
    for (uint32_t i = rt.class_start[0]; i < rt.class_start[1]; ++i) {       // leaves: the exact box of their triangles
        const uint32_t t = rt.order[i], ref = rt.ref2[t], first = ref & ((1u << kLeafCountShift) - 1u), count = (ref >> kLeafCountShift) & 15u;
        float *bx = &rt.boxes[6 * (size_t) t];
        for (int k = 0; k < 3; ++k) { bx[k] = INFINITY; bx[3 + k] = -INFINITY; }
        for (uint32_t s = first; s < first + count; ++s) {
            const float *tp = tri_pos + 9 * (size_t) rt.slot_prim[s];
            for (int j = 0; j < 3; ++j) for (int k = 0; k < 3; ++k) { bx[k] = enc_min(bx[k], tp[3 * j + k]); bx[3 + k] = enc_max(bx[3 + k], tp[3 * j + k]); }
        }
    }
    for (size_t i = rt.class_start[1]; i < rt.order.size(); ++i) {            // then every height class from its children
        const uint32_t t = rt.order[i];
        const float *l = &rt.boxes[6 * (size_t) rt.left[t]], *r = &rt.boxes[6 * (size_t) rt.right[t]];
        float *bx = &rt.boxes[6 * (size_t) t];
        for (int k = 0; k < 3; ++k) { bx[k] = enc_min(l[k], r[k]); bx[3 + k] = enc_max(l[3 + k], r[3 + k]); }
    }
    emit_bvh(tri_pos, out);
}

void build_bvh(const float *tri_pos, uint32_t n_prims, uint32_t max_leaf, BvhOutput &out, const BvhOptions *opt) {
    Builder b;
    b.tri_pos = tri_pos; b.n_prims = n_prims; b.max_leaf = std::min<uint32_t>(std::max<uint32_t>(max_leaf, 1), 15);
    const BvhOptions defaults;
    if (!opt) opt = &defaults;
    b.kBins = std::min(std::max(opt->bins, 2), kMaxBins); b.kIntersectCost = opt->intersect_cost; b.sweep_below = opt->sweep_below;
    b.prim_box.resize(n_prims); b.centroid.resize(3 * (size_t) n_prims); b.perm.resize(n_prims);
    for (uint32_t p = 0; p < n_prims; ++p) {
        Box bx; bx.reset();
        for (int j = 0; j < 3; ++j) {
            double v[3] = { tri_pos[9 * (size_t) p + 3 * j], tri_pos[9 * (size_t) p + 3 * j + 1], tri_pos[9 * (size_t) p + 3 * j + 2] };
            bx.grow(v);
        }
        b.prim_box[p] = bx;
        for (int k = 0; k < 3; ++k) b.centroid[3 * (size_t) p + k] = 0.5 * (bx.lo[k] + bx.hi[k]);
        b.perm[p] = p;
    }
    b.nodes.reserve(2 * (size_t) n_prims);
    int32_t root = b.build(0, n_prims, 0);

    // ---- topology: what stays when the vertices move (refit_bvh).  Inner nodes in BFS order (the top of the tree comes first, so a
    // prefix of the node array is what gets staged in LDS), triangle slots in the order their leaves are reached.
    RefitTable &rt = out.refit;
    rt = RefitTable{};
    const size_t n_tmp = b.nodes.size();
    std::vector<int32_t> inner_index(n_tmp, -1);
    std::vector<int32_t> bfs;
    if (opt->dfs_order) {                                          // experiment: pre-order layout
        std::vector<int32_t> st;
        if (b.nodes[root].left >= 0) st.push_back(root);
        while (!st.empty()) {
            int32_t t = st.back(); st.pop_back();
            inner_index[t] = (int32_t) bfs.size(); bfs.push_back(t);
            const TmpNode &n = b.nodes[t];
            if (b.nodes[n.right].left >= 0) st.push_back(n.right);
            if (b.nodes[n.left].left >= 0) st.push_back(n.left);
        }
    } else {
        std::queue<int32_t> q;
        if (b.nodes[root].left >= 0) q.push(root);
        while (!q.empty()) {
            int32_t t = q.front(); q.pop();
            inner_index[t] = (int32_t) bfs.size(); bfs.push_back(t);
            const TmpNode &n = b.nodes[t];
            if (b.nodes[n.left].left >= 0) q.push(n.left);
            if (b.nodes[n.right].left >= 0) q.push(n.right);
        }
    }
    rt.root = root;
    rt.left.resize(n_tmp); rt.right.resize(n_tmp); rt.ref2.assign(n_tmp, 0u); rt.ref4.assign(n_tmp, 0u);
    rt.boxes.resize(6 * n_tmp);
    for (size_t t = 0; t < n_tmp; ++t) {
        rt.left[t] = b.nodes[t].left; rt.right[t] = b.nodes[t].right;
        for (int k = 0; k < 3; ++k) { rt.boxes[6 * t + k] = (float) b.nodes[t].box.lo[k]; rt.boxes[6 * t + 3 + k] = (float) b.nodes[t].box.hi[k]; }
    }
    uint32_t slot = 0;
    auto leaf_slots = [&](int32_t t) -> uint32_t {
        const TmpNode &n = b.nodes[t];
        uint32_t start = slot;
        for (uint32_t i = 0; i < n.count; ++i) { rt.slot_prim.push_back(b.perm[n.first + i]); ++slot; }
        return kLeafFlag | (n.count << kLeafCountShift) | start;
    };
    auto child_ref = [&](int32_t t) -> uint32_t {
        if (b.nodes[t].left >= 0) return rt.ref2[t] = (uint32_t) inner_index[t];
        return rt.ref2[t] = rt.ref4[t] = leaf_slots(t);
    };
    rt.node_child.resize(2 * bfs.size());
    for (size_t i = 0; i < bfs.size(); ++i) {
        const TmpNode &n = b.nodes[bfs[i]];
        rt.node_child[2 * i] = n.left; rt.node_child[2 * i + 1] = n.right;
        child_ref(n.left); child_ref(n.right);
    }
    if (bfs.empty()) out.root = child_ref(root);   // whole scene is one leaf
    else out.root = 0;
    // BVH4: collapse (open the child of largest surface area until four children), BFS order
    out.wroot = out.root; out.n_wnodes = 0; out.wdepth = 1;
    if (!bfs.empty()) {
        struct Wide { int32_t child[4]; int n; uint32_t depth; };
        std::vector<Wide> wide;
        std::vector<int32_t> wide_of(n_tmp, -1);      // BVH2 inner node -> wide node that replaces it
        std::queue<std::pair<int32_t, uint32_t>> q;
        q.push({ root, 1u });
        wide_of[root] = 0; wide.push_back(Wide{});
        while (!q.empty()) {
            const int32_t t = q.front().first; const uint32_t depth = q.front().second; q.pop();
            Wide wn{}; wn.depth = depth;
            wn.child[0] = b.nodes[t].left; wn.child[1] = b.nodes[t].right; wn.n = 2;
            while (wn.n < 4) {
                int best = -1; double best_area = -1.0;
                for (int c = 0; c < wn.n; ++c)
                    if (b.nodes[wn.child[c]].left >= 0 && b.nodes[wn.child[c]].box.area() > best_area) { best = c; best_area = b.nodes[wn.child[c]].box.area(); }
                if (best < 0) break;
                const int32_t open = wn.child[best];
                wn.child[best] = b.nodes[open].left; wn.child[wn.n++] = b.nodes[open].right;
            }
            for (int c = 0; c < wn.n; ++c)
                if (b.nodes[wn.child[c]].left >= 0) { wide_of[wn.child[c]] = (int32_t) wide.size(); wide.push_back(Wide{}); q.push({ wn.child[c], depth + 1 }); }
            wide[wide_of[t]] = wn;
            out.wdepth = std::max(out.wdepth, depth);
        }
        out.n_wnodes = (uint32_t) wide.size();
        rt.wide_child.assign(4 * wide.size(), -1);
        for (size_t i = 0; i < wide.size(); ++i)
            for (int c = 0; c < wide[i].n; ++c) rt.wide_child[4 * i + c] = wide[i].child[c];
        for (size_t t = 0; t < n_tmp; ++t) if (b.nodes[t].left >= 0) rt.ref4[t] = (uint32_t) wide_of[t];
        out.wroot = 0;
    }
    // height above the leaves; children follow their parent in the builder's array, so one backward pass sees them first
    rt.height.assign(n_tmp, 0u);
    uint32_t top = 0;
    for (size_t t = n_tmp; t-- > 0;)
        if (rt.left[t] >= 0) { rt.height[t] = 1u + std::max(rt.height[rt.left[t]], rt.height[rt.right[t]]); top = std::max(top, rt.height[t]); }
    rt.class_start.assign(top + 2, 0u);
    for (size_t t = 0; t < n_tmp; ++t) rt.class_start[rt.height[t] + 1]++;
    for (uint32_t h = 0; h <= top; ++h) rt.class_start[h + 1] += rt.class_start[h];
    rt.order.resize(n_tmp);
    { std::vector<uint32_t> at(rt.class_start.begin(), rt.class_start.end() - 1);
      for (size_t t = 0; t < n_tmp; ++t) rt.order[at[rt.height[t]]++] = (uint32_t) t; }
    emit_bvh(tri_pos, out);
    out.n_nodes = (uint32_t) bfs.size();
    out.n_slots = slot;
    out.depth = b.max_depth + 1;
}

namespace { struct Kid { int32_t x, y; }; }

// ---- what build_lbvh and build_sah_levels share, from the heights on: the table holds left / right, ref2 (and ref4 of the leaves),
// node_child and slot_prim, builder node 0 is the root; heights, order / class_start, exact boxes with the refit's arithmetic, the BVH4
// collapse per wide level, the emission.
static void finish_levels(const float *tri_pos, BvhOutput &out) {
    RefitTable &rt = out.refit;
    const size_t n_tmp = rt.left.size(), n_inner = rt.node_child.size() / 2;
    // heights: a node's is known once both children's are; rounds of that rule, as many as the tree is high
    rt.height.assign(n_tmp, kLbvhNoHeight);
    for (size_t t = 0; t < n_tmp; ++t) if (rt.left[t] < 0) rt.height[t] = 0u;
    for (bool again = true; again;) {
        again = false;
        std::vector<uint32_t> next(rt.height);
        for (size_t t = 0; t < n_tmp; ++t) {
            if (rt.height[t] != kLbvhNoHeight) continue;
            const uint32_t a = rt.height[rt.left[t]], b = rt.height[rt.right[t]];
            if (a != kLbvhNoHeight && b != kLbvhNoHeight) next[t] = 1u + std::max(a, b); else again = true;
        }
        rt.height.swap(next);
    }
    const uint32_t top = rt.height[0];
    rt.class_start.assign(top + 2, 0u);
    for (size_t t = 0; t < n_tmp; ++t) rt.class_start[rt.height[t] + 1]++;
    for (uint32_t h = 0; h <= top; ++h) rt.class_start[h + 1] += rt.class_start[h];
    rt.order.resize(n_tmp);
    { std::vector<uint32_t> at(rt.class_start.begin(), rt.class_start.end() - 1);
      for (size_t t = 0; t < n_tmp; ++t) rt.order[at[rt.height[t]]++] = (uint32_t) t; }
    // exact boxes, as a refit computes them
    std::vector<Kid> kids(n_tmp);
    for (size_t t = 0; t < n_tmp; ++t) kids[t] = rt.left[t] >= 0 ? Kid{ rt.left[t], rt.right[t] } : Kid{ -1, (int32_t) rt.ref2[t] };
    for (size_t i = 0; i < n_tmp; ++i) {
        const uint32_t t = rt.order[i];
        float *bx = &rt.boxes[6 * (size_t) t];
        if (kids[t].x < 0) {
            const uint32_t ref = rt.ref2[t], s0 = ref & ((1u << kLeafCountShift) - 1u), cnt = (ref >> kLeafCountShift) & 15u;
            for (int k = 0; k < 3; ++k) { bx[k] = INFINITY; bx[3 + k] = -INFINITY; }
            for (uint32_t s = s0; s < s0 + cnt; ++s) {
                const float *tp = tri_pos + 9 * (size_t) rt.slot_prim[s];
                for (int j = 0; j < 3; ++j) for (int k = 0; k < 3; ++k) { bx[k] = enc_min(bx[k], tp[3 * j + k]); bx[3 + k] = enc_max(bx[3 + k], tp[3 * j + k]); }
            }
        } else {
            const float *l = &rt.boxes[6 * (size_t) kids[t].x], *r = &rt.boxes[6 * (size_t) kids[t].y];
            for (int k = 0; k < 3; ++k) { bx[k] = enc_min(l[k], r[k]); bx[3 + k] = enc_max(l[3 + k], r[3 + k]); }
        }
    }
    // BVH4: one wide level after the other; the inner children of a level, by parent and child position, are the next
    out.root = out.wroot = n_inner ? 0u : rt.ref2[0];
    out.n_wnodes = 0; out.wdepth = 1;
    if (n_inner) {
        std::vector<int32_t> level(1, 0), wide_child;
        uint32_t levels = 0;
        while (!level.empty()) {
            ++levels;
            const size_t start = wide_child.size() / 4, next_start = start + level.size();
            std::vector<int32_t> next;
            for (size_t j = 0; j < level.size(); ++j) {
                int32_t c[4];
                lbvh_collapse(kids.data(), rt.boxes.data(), level[j], c);
                for (int k = 0; k < 4; ++k) {
                    wide_child.push_back(c[k]);
                    if (c[k] >= 0 && kids[c[k]].x >= 0) { rt.ref4[c[k]] = (uint32_t) (next_start + next.size()); next.push_back(c[k]); }
                }
            }
            level.swap(next);
        }
        rt.ref4[0] = 0u;
        rt.wide_child = wide_child;
        out.n_wnodes = (uint32_t) (wide_child.size() / 4); out.wdepth = levels;
    }
    emit_bvh(tri_pos, out);
    out.n_nodes = (uint32_t) n_inner;
    out.n_slots = (uint32_t) rt.slot_prim.size();
    out.depth = top + 1;
}

// ---- build_lbvh: the specification of the device build (bvh.h).  Every step is a loop over independent elements, or a scan; the
// element functions are lbvh_keys.h's, which csrc/lbvh.hip calls too.
void build_lbvh(const float *tri_pos, uint32_t n_prims, uint32_t max_leaf, BvhOutput &out) {
    max_leaf = std::min<uint32_t>(std::max<uint32_t>(max_leaf, 1), 15);
    const int n = (int) n_prims;
    RefitTable &rt = out.refit;
    rt = RefitTable{};
    // keys: the scene box is the exact union of all vertices; then one code per primitive and the stable order
    float bbox[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    for (size_t p = 0; p < n_prims; ++p) {
        float lo[3], hi[3];
        lbvh_prim_box(tri_pos + 9 * p, lo, hi);
        for (int k = 0; k < 3; ++k) { bbox[k] = enc_min(bbox[k], lo[k]); bbox[3 + k] = enc_max(bbox[3 + k], hi[k]); }
    }
    std::vector<uint64_t> keys(n_prims);
    for (size_t p = 0; p < n_prims; ++p) keys[p] = ((uint64_t) lbvh_code(tri_pos + 9 * p, bbox) << 32) | p;
    std::sort(keys.begin(), keys.end());
    std::vector<uint32_t> codes(n_prims);
    rt.slot_prim.resize(n_prims);
    for (size_t s = 0; s < n_prims; ++s) { codes[s] = (uint32_t) (keys[s] >> 32); rt.slot_prim[s] = (uint32_t) keys[s]; }
    // radix tree: ids [0, n - 1) are the inner nodes, n - 1 + s the leaf at position s.  Each inner node states what its children are:
    // 0 = below a leaf (dropped), 1 = leaf, 2 = inner
    const size_t n_radix = 2 * (size_t) n_prims - 1;
    std::vector<uint32_t> state(n_radix, 0u), first(n_radix, 0u), count(n_radix, 0u);
    std::vector<int32_t> rl(n_prims - 1), rr(n_prims - 1);
    state[0] = n_prims > max_leaf ? 2u : 1u; first[0] = 0u; count[0] = n_prims;
    for (int i = 0; i + 1 < n; ++i) {
        int f, l, split;
        lbvh_radix_node(codes.data(), n, i, &f, &l, &split);
        const int32_t c[2] = { split == f ? n - 1 + split : split, split + 1 == l ? n - 1 + split + 1 : split + 1 };
        const uint32_t cf[2] = { (uint32_t) f, (uint32_t) split + 1u }, cc[2] = { (uint32_t) (split - f + 1), (uint32_t) (l - split) };
        rl[i] = c[0]; rr[i] = c[1];
        const bool open = (uint32_t) (l - f + 1) > max_leaf;
        for (int k = 0; k < 2; ++k) { state[c[k]] = !open ? 0u : (cc[k] > max_leaf ? 2u : 1u); first[c[k]] = cf[k]; count[c[k]] = cc[k]; }
    }
    // compaction: builder ids and BVH2 ids are exclusive scans of the survivors
    std::vector<int32_t> bid(n_radix, -1), iid(n_radix, -1);
    size_t n_tmp = 0, n_inner = 0;
    for (size_t x = 0; x < n_radix; ++x) {
        if (state[x]) bid[x] = (int32_t) n_tmp++;
        if (state[x] == 2u) iid[x] = (int32_t) n_inner++;
    }
    rt.root = 0;
    rt.left.assign(n_tmp, -1); rt.right.assign(n_tmp, -1); rt.ref2.assign(n_tmp, 0u); rt.ref4.assign(n_tmp, 0xffffffffu);
    rt.boxes.assign(6 * n_tmp, 0.0f); rt.node_child.resize(2 * n_inner);
    for (size_t x = 0; x < n_radix; ++x) {
        if (!state[x]) continue;
        const int32_t t = bid[x];
        if (state[x] == 2u) {
            rt.left[t] = bid[rl[x]]; rt.right[t] = bid[rr[x]];
            rt.ref2[t] = (uint32_t) iid[x];
            rt.node_child[2 * (size_t) iid[x]] = rt.left[t]; rt.node_child[2 * (size_t) iid[x] + 1] = rt.right[t];
        } else {
            rt.ref2[t] = rt.ref4[t] = kLeafFlag | (count[x] << kLeafCountShift) | first[x];
        }
    }
    finish_levels(tri_pos, out);
}

// ---- build_sah_levels: the specification of the device SAH build (bvh.h).  A level is three loops: decide every node (independent), number
// what they made (a scan), write children and leaf slots (independent).  The element functions are sah_keys.h's, which
// csrc/sah_build.hip calls too.
void build_sah_levels(const float *tri_pos, uint32_t n_prims, uint32_t max_leaf, BvhOutput &out, SahLevelsTrace *trace) {
    max_leaf = std::min<uint32_t>(std::max<uint32_t>(max_leaf, 1), 15);
    RefitTable &rt = out.refit;
    rt = RefitTable{};
    std::vector<float> pbox(6 * (size_t) n_prims);
    std::vector<double> cen(3 * (size_t) n_prims);
    std::vector<uint32_t> perm(n_prims), perm_next(n_prims);
    for (size_t p = 0; p < n_prims; ++p) {
        sah_prim(tri_pos + 9 * p, &pbox[6 * p], &pbox[6 * p + 3], &cen[3 * p]);
        perm[p] = (uint32_t) p;
    }
    struct Active { uint32_t first, count; };
    struct Decision { uint32_t mode, left; int axis, bin; double lo, scale, cost; };
    std::vector<Active> level(1, Active{ 0u, n_prims }), next_level;
    size_t level_base = 0, n_inner = 0, n_slots = 0;
    rt.root = 0;
    rt.slot_prim.resize(n_prims);
    for (uint32_t depth = 0; !level.empty(); ++depth) {
        const size_t m = level.size(), next_base = level_base + m;
        // decide
        std::vector<Decision> dec(m);
        for (size_t j = 0; j < m; ++j) {
            const uint32_t first = level[j].first, count = level[j].count;
            Decision &d = dec[j];
            d = Decision{ kSahLeaf, 0u, -1, -1, 0.0, 0.0, DBL_MAX };
            SahBins bins;
            if (count > 1u) {
                float nb[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
                double cb_lo[3] = { DBL_MAX, DBL_MAX, DBL_MAX }, cb_hi[3] = { -DBL_MAX, -DBL_MAX, -DBL_MAX };
                for (uint32_t i = 0; i < count; ++i) {
                    const size_t p = perm[first + i];
                    for (int k = 0; k < 3; ++k) {
                        nb[k] = std::min(nb[k], pbox[6 * p + k]); nb[3 + k] = std::max(nb[3 + k], pbox[6 * p + 3 + k]);
                        cb_lo[k] = std::min(cb_lo[k], cen[3 * p + k]); cb_hi[k] = std::max(cb_hi[k], cen[3 * p + k]);
                    }
                }
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < kSahBins; ++b) { for (int k = 0; k < 3; ++k) { bins.lo[a][b][k] = 0xffffffffu; bins.hi[a][b][k] = 0u; } bins.cnt[a][b] = 0u; }
                for (int a = 0; a < 3; ++a) {
                    const double ext = cb_hi[a] - cb_lo[a];
                    if (!(ext > 0.0)) continue;
                    const double scale = sah_scale(ext);
                    for (uint32_t i = 0; i < count; ++i) {
                        const size_t p = perm[first + i];
                        const int b = sah_bin(cen[3 * p + a], cb_lo[a], scale);
                        for (int k = 0; k < 3; ++k) {
                            bins.lo[a][b][k] = std::min(bins.lo[a][b][k], sah_ord(pbox[6 * p + k]));
                            bins.hi[a][b][k] = std::max(bins.hi[a][b][k], sah_ord(pbox[6 * p + 3 + k]));
                        }
                        bins.cnt[a][b]++;
                    }
                }
                sah_choose(bins, cb_lo, cb_hi, lbvh_area(nb), &d.axis, &d.bin, &d.cost);
                d.mode = sah_decide(count, max_leaf, depth, d.axis, d.cost);
                if (d.mode != kSahLeaf) d.left = sah_left_count(bins, count, &d.mode, d.axis, d.bin);
                if (d.mode == kSahSplitBin) { d.lo = cb_lo[d.axis]; d.scale = sah_scale(cb_hi[d.axis] - cb_lo[d.axis]); }
            }
            if (trace) {
                trace->first.push_back(first); trace->count.push_back(count); trace->depth.push_back(depth); trace->mode.push_back(d.mode);
                trace->left_count.push_back(d.left); trace->axis.push_back(d.axis); trace->bin.push_back(d.bin); trace->cost.push_back(d.cost);
                if (count > 1u && trace->bins_node.size() < trace->bins_of) {
                    trace->bins_node.push_back((uint32_t) (level_base + j));
                    const uint32_t *w = reinterpret_cast<const uint32_t *>(&bins);
                    trace->bins.insert(trace->bins.end(), w, w + kSahBinWords);
                }
            }
        }
        // number: the children and the BVH2 id of every split node, the first slot of every leaf
        std::vector<uint32_t> split_rank(m), leaf_slot(m);
        size_t n_split = 0;
        for (size_t j = 0; j < m; ++j) {
            split_rank[j] = (uint32_t) n_split; leaf_slot[j] = (uint32_t) n_slots;
            if (dec[j].mode != kSahLeaf) ++n_split; else n_slots += level[j].count;
        }
        // write
        rt.left.resize(next_base, -1); rt.right.resize(next_base, -1); rt.ref2.resize(next_base, 0u); rt.ref4.resize(next_base, 0xffffffffu);
        rt.node_child.resize(2 * (n_inner + n_split));
        next_level.assign(2 * n_split, Active{ 0u, 0u });
        for (size_t j = 0; j < m; ++j) {
            const size_t t = level_base + j;
            const uint32_t first = level[j].first, count = level[j].count;
            const Decision &d = dec[j];
            if (d.mode == kSahLeaf) {
                rt.ref2[t] = rt.ref4[t] = kLeafFlag | (count << kLeafCountShift) | leaf_slot[j];
                for (uint32_t i = 0; i < count; ++i) rt.slot_prim[leaf_slot[j] + i] = perm[first + i];
                continue;
            }
            const size_t r = split_rank[j], iid = n_inner + r;
            const int32_t l = (int32_t) (next_base + 2 * r);
            rt.left[t] = l; rt.right[t] = l + 1; rt.ref2[t] = (uint32_t) iid;
            rt.node_child[2 * iid] = l; rt.node_child[2 * iid + 1] = l + 1;
            next_level[2 * r] = Active{ first, d.left }; next_level[2 * r + 1] = Active{ first + d.left, count - d.left };
            if (d.mode == kSahSplitBin) {                     // the stable partition
                uint32_t nl = 0, nr = 0;
                for (uint32_t i = 0; i < count; ++i) {
                    const uint32_t p = perm[first + i];
                    if (sah_bin(cen[3 * (size_t) p + d.axis], d.lo, d.scale) <= d.bin) perm_next[first + nl++] = p;
                    else perm_next[first + d.left + nr++] = p;
                }
            } else {
                for (uint32_t i = 0; i < count; ++i) perm_next[first + i] = perm[first + i];
            }
        }
        n_inner += n_split;
        level_base = next_base;
        level.swap(next_level);
        perm.swap(perm_next);
    }
    rt.boxes.assign(6 * rt.left.size(), 0.0f);
    finish_levels(tri_pos, out);
}

double sah_cost_blocked(const int32_t *kids, const float *boxes, size_t n_builder, int32_t root) {
    const double root_area = lbvh_area(boxes + 6 * (size_t) root);
    double total = 0.0;
    for (size_t base = 0; base < n_builder; base += kSahBlock) {
        double v[kSahBlock];
        for (size_t j = 0; j < kSahBlock; ++j) {
            const size_t t = base + j;
            v[j] = t < n_builder ? lbvh_sah_term(Kid{ kids[2 * t], kids[2 * t + 1] }, boxes + 6 * t, root_area) : 0.0;
        }
        for (uint32_t stride = kSahBlock / 2; stride > 0; stride /= 2)
            for (uint32_t j = 0; j < stride; ++j) v[j] += v[j + stride];
        total += v[0];
    }
    return total;
}

} // namespace mtsamd

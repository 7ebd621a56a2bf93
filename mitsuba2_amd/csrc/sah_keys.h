// sah_keys.h -- the per-element arithmetic of the level-synchronous binned-SAH build (bvh.h: build_sah_levels; sah_build.hip: the device
// build), shared by host and device in the manner of lbvh_keys.h.  The requirement is byte identity of the two builds and, node for node,
// the decisions of build_bvh with the shipped BvhOptions: every function below is one of its expressions, operand for operand, in IEEE
// double (the build has -ffp-contract=off).  Boxes are kept as fp32: a union of fp32 vertices is one, and every use of a box here is a
// difference in double, so neither the width nor the sign of a zero can influence a decision.
#pragma once
#include <cfloat>
#include "lbvh_keys.h"

namespace mtsamd {

constexpr int kSahBins = 16;                     // BvhOptions::bins
constexpr double kSahIntersectCost = 1.5;        // BvhOptions::intersect_cost
constexpr uint32_t kSahGuardDepth = 40u;         // from this depth on (root = 0) a split is the middle of the present order

// fp32 as an unsigned integer of the same order: integer min / max of these are float min / max, whatever the order of the updates
MTS_ENC uint32_t sah_ord(float f) { const uint32_t u = enc_bits(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
MTS_ENC float sah_unord(uint32_t k) { return enc_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// The bins of one node: per axis and bin the box of the primitives whose centroid falls into it, as six order-encoded planes, and their
// number.  An empty bin holds lo = 0xffffffff, hi = 0, cnt = 0.
struct SahBins {
    uint32_t lo[3][kSahBins][3], hi[3][kSahBins][3], cnt[3][kSahBins];
};
constexpr uint32_t kSahBinWords = sizeof(SahBins) / 4u;

// box of the fp32 vertices of a triangle (9 floats) and its centroid
MTS_ENC void sah_prim(const float *tp, float lo[3], float hi[3], double c[3]) {
    lbvh_prim_box(tp, lo, hi);
    for (int k = 0; k < 3; ++k) c[k] = 0.5 * ((double) lo[k] + (double) hi[k]);
}

// one coordinate of that centroid alone (the partition reads three floats per primitive, not nine)
MTS_ENC double sah_centroid_axis(const float *tp, int axis) {
    float lo = INFINITY, hi = -INFINITY;
    for (int j = 0; j < 3; ++j) { lo = enc_min(lo, tp[3 * j + axis]); hi = enc_max(hi, tp[3 * j + axis]); }
    return 0.5 * ((double) lo + (double) hi);
}

// scale of an axis of positive centroid extent, and the bin of a centroid coordinate
MTS_ENC double sah_scale(double ext) { return kSahBins / ext; }
MTS_ENC int sah_bin(double c, double lo, double scale) {
    const int b = (int) ((c - lo) * scale);
    const int m = b > 0 ? b : 0;
    return m < kSahBins - 1 ? m : kSahBins - 1;
}

MTS_ENC void sah_grow(float acc[6], const uint32_t lo[3], const uint32_t hi[3]) {
    for (int k = 0; k < 3; ++k) {
        const float l = sah_unord(lo[k]), h = sah_unord(hi[k]);
        acc[k] = l < acc[k] ? l : acc[k]; acc[3 + k] = acc[3 + k] < h ? h : acc[3 + k];
    }
}

MTS_ENC double sah_cost(double area_l, uint32_t n_l, double area_r, uint32_t n_r, double parent_area) {
    return 1.0 + kSahIntersectCost * (area_l * n_l + area_r * n_r) / parent_area;
}

// build_bvh's search: per axis of positive centroid extent the suffix pass and then the prefix pass over the bins; a strictly smaller
// cost wins, axes 0, 1, 2 outside and bins ascending inside.  No candidate: axis -1.  `area`: of the node's box.
MTS_ENC void sah_choose(const SahBins &bins, const double cb_lo[3], const double cb_hi[3], double area, int *best_axis, int *best_bin, double *best_cost) {
    double best = DBL_MAX; int ba = -1, bb = -1;
    const double parent_area = fmax(area, 1e-300);
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
        const double ext = cb_hi[axis] - cb_lo[axis];
        if (!(ext > 0.0)) continue;
        double right_area[kSahBins]; uint32_t right_cnt[kSahBins];
        float acc[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
        uint32_t cnt = 0;
#pragma unroll
        for (int b = kSahBins - 1; b > 0; --b) {
            if (bins.cnt[axis][b]) sah_grow(acc, bins.lo[axis][b], bins.hi[axis][b]);
            cnt += bins.cnt[axis][b];
            right_area[b] = cnt ? lbvh_area(acc) : 0.0; right_cnt[b] = cnt;
        }
        for (int k = 0; k < 3; ++k) { acc[k] = INFINITY; acc[3 + k] = -INFINITY; }
        cnt = 0;
#pragma unroll
        for (int b = 0; b < kSahBins - 1; ++b) {
            if (bins.cnt[axis][b]) sah_grow(acc, bins.lo[axis][b], bins.hi[axis][b]);
            cnt += bins.cnt[axis][b];
            if (cnt == 0 || right_cnt[b + 1] == 0) continue;
            const double cost = sah_cost(lbvh_area(acc), cnt, right_area[b + 1], right_cnt[b + 1], parent_area);
            if (cost < best) { best = cost; ba = axis; bb = b; }
        }
    }
    *best_axis = ba; *best_bin = bb; *best_cost = best;
}

// What becomes of a node of `count` primitives at `depth`: a leaf, a split by bin, or a split in the middle of the present order
enum : uint32_t { kSahLeaf = 0u, kSahSplitBin = 1u, kSahSplitMiddle = 2u };
MTS_ENC uint32_t sah_decide(uint32_t count, uint32_t max_leaf, uint32_t depth, int best_axis, double best_cost) {
    if (count <= 1u) return kSahLeaf;
    if (count <= max_leaf && (best_axis < 0 || kSahIntersectCost * count <= best_cost)) return kSahLeaf;
    if (best_axis < 0 || depth >= kSahGuardDepth) return kSahSplitMiddle;
    return kSahSplitBin;
}

// primitives left of a split by (axis, bin); a split that would leave a side empty is the middle instead (the bins make no such
// candidate: the rule is build_bvh's last line of defence, kept)
MTS_ENC uint32_t sah_left_count(const SahBins &bins, uint32_t count, uint32_t *mode, int axis, int bin) {
    if (*mode == kSahSplitBin) {
        uint32_t nl = 0;
        for (int b = 0; b < kSahBins; ++b) if (b <= bin) nl += bins.cnt[axis][b];
        if (nl != 0u && nl != count) return nl;
        *mode = kSahSplitMiddle;
    }
    return count / 2u;
}

} // namespace mtsamd

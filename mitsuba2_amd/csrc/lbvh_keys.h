// lbvh_keys.h -- the per-element arithmetic of the LBVH build (bvh.h: build_lbvh; lbvh.hip: the device build), shared by host and device in
// the manner of refit_encode.h.  The requirement is byte identity of the two builds: every step below is a function of one element
// (a primitive, a radix-tree node, a wide node) that both sides call, written with operations IEEE fixes (the build has -ffp-contract=off).
#pragma once
#include "refit_encode.h"

namespace mtsamd {

constexpr uint32_t kLbvhLeafFlag = 0x80000000u;
constexpr uint32_t kLbvhNoHeight = 0xffffffffu;

MTS_ENC uint32_t lbvh_clz(uint32_t x) { uint32_t n = 0; if (x == 0u) return 32u; while (!(x & 0x80000000u)) { x <<= 1; ++n; } return n; }

// bits 0..9 of v to bits 0, 3, .. 27
MTS_ENC uint32_t lbvh_spread(uint32_t v) {
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// The 10-bit cell of centroid coordinate c on an axis of the scene box [lo, hi].  lo + 0.0f: a box whose zero is negative gives the cells
// of one whose zero is positive (the scene box comes from a union whose order decides that sign).  An axis of zero extent gives cell 0,
// and so does whatever is not a number.
MTS_ENC uint32_t lbvh_cell(float c, float lo, float hi) {
    const float l = lo + 0.0f, ext = hi - l;
    if (!(ext > 0.0f)) return 0u;
    const double x = floor(((double) c - (double) l) / (double) ext * 1024.0);
    return (uint32_t) fmin(1023.0, fmax(0.0, x));
}

// exact fp32 box of a triangle (9 floats), in the operand order of the refit's leaves; then the 30-bit Morton code of its centre
MTS_ENC void lbvh_prim_box(const float *tp, float lo[3], float hi[3]) {
    for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) { lo[k] = enc_min(lo[k], tp[3 * j + k]); hi[k] = enc_max(hi[k], tp[3 * j + k]); }
}
MTS_ENC uint32_t lbvh_code(const float *tp, const float *bbox) {
    float lo[3], hi[3];
    lbvh_prim_box(tp, lo, hi);
    uint32_t cell[3];
    for (int k = 0; k < 3; ++k) cell[k] = lbvh_cell(0.5f * (lo[k] + hi[k]), bbox[k], bbox[3 + k]);
    return (lbvh_spread(cell[0]) << 2) | (lbvh_spread(cell[1]) << 1) | lbvh_spread(cell[2]);
}

// Karras 2012 over the sorted codes: the length of the common prefix of the keys (code, sorted position) at positions i and j, -1 outside
MTS_ENC int lbvh_delta(const uint32_t *codes, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    const uint32_t a = codes[i], b = codes[j];
    if (a == b) return 32 + (int) lbvh_clz((uint32_t) i ^ (uint32_t) j);
    return (int) lbvh_clz(a ^ b);
}

// Inner node i of the radix tree over n >= 2 sorted codes: its range [first, last] of sorted positions and the split: the children cover
// [first, split] and [split + 1, last]; a child that covers one position is that leaf, otherwise it is inner node `split` / `split + 1`.
MTS_ENC void lbvh_radix_node(const uint32_t *codes, int n, int i, int *first, int *last, int *split) {
    const int d = lbvh_delta(codes, n, i, i + 1) - lbvh_delta(codes, n, i, i - 1) < 0 ? -1 : 1;
    const int dmin = lbvh_delta(codes, n, i, i - d);
    int lmax = 2;
    while (lbvh_delta(codes, n, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (lbvh_delta(codes, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = lbvh_delta(codes, n, i, j);
    int s = 0;
    for (int t = (l + 1) / 2;; t = (t + 1) / 2) {
        if (lbvh_delta(codes, n, i, i + (s + t) * d) > dnode) s += t;
        if (t <= 1) break;
    }
    *split = i + s * d + (d < 0 ? -1 : 0);
    *first = d > 0 ? i : j; *last = d > 0 ? j : i;
}

// surface area of an exact box (6 floats), in double: the measure of build_bvh's collapse and of the SAH cost
MTS_ENC double lbvh_area(const float *bx) {
    const double dx = (double) bx[3] - (double) bx[0], dy = (double) bx[4] - (double) bx[1], dz = (double) bx[5] - (double) bx[2];
    if (dx < 0) return 0.0;
    return 2.0 * (dx * dy + dy * dz + dz * dx);
}

// The BVH4 collapse of build_bvh for the wide node that replaces builder node t: open the inner child of largest area, the first of
// equals, until there are four children or none is inner.  kids[t] = (left, right), or (-1, leaf reference).  Returns the child count.
template <typename Kids> MTS_ENC int lbvh_collapse(const Kids *kids, const float *boxes, int32_t t, int32_t child[4]) {
    child[0] = kids[t].x; child[1] = kids[t].y; child[2] = child[3] = -1;
    int n = 2;
    while (n < 4) {
        int best = -1; double best_area = -1.0;
        for (int c = 0; c < n; ++c) {
            if (kids[child[c]].x < 0) continue;
            const double a = lbvh_area(boxes + 6 * (size_t) child[c]);
            if (a > best_area) { best = c; best_area = a; }
        }
        if (best < 0) break;
        const int32_t open = child[best];
        child[best] = kids[open].x; child[n++] = kids[open].y;
    }
    return n;
}

// SAH cost of a tree (mtsamd_scene_accel_info): the term of builder node t, relative to the root's area; blocks of kSahBlock consecutive
// terms are summed by halving (lbvh_sah_block: the order of the device's reduction), and the blocks' sums one after the other.
constexpr uint32_t kSahBlock = 256u;
template <typename Kids> MTS_ENC double lbvh_sah_term(const Kids &kd, const float *bx, double root_area) {
    if (!(root_area > 0.0)) return 0.0;
    const double a = lbvh_area(bx) / root_area;
    if (kd.x >= 0) return a;
    return 1.5 * ((double) (((uint32_t) kd.y >> 27) & 15u) * a);
}

} // namespace mtsamd

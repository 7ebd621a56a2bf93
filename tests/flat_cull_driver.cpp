// Stand-alone driver of the flat-scene cluster cull (mitsuba2_amd/csrc/flat_cull.h) for tests/test_flat_cull_cpu.py.  Reads scenes (triangles
// with their shapes) and rays from a binary file, lets the host builder (build_flat_records, scene_build.cpp stage 7) make the pair and
// cluster records, and counts per scene:
//   - violations: a triangle that the scalar restatement of the pair test accepts within [mint, maxt] while the reach predicate leaves its
//     pair's bit clear -- for both queries of the form the library is built with (CullFolded: the work lists, CullLean: the clustered
//     loops; reciprocals exact, an ulp up, an ulp down, and with denormals read as zero, which is what v_rcp_f32 does) and for form 0 on
//     its own lo / hi records, restated here from the padded box;
//   - the (ray, cluster) tests each of them flags, for the tightness bound;
//   - records whose box does not contain the padded box, whose count or whose mask is wrong.
// It decides nothing: every expectation lives in the test.   argv[1]: the input file
#include "scene_build.h"
#include "flat_cull.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace mtsamd;

template <typename T> static std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return v;
}
static uint32_t take_u32(FILE *f) { return take<uint32_t>(f, 1)[0]; }

// pair_test + tri_accept on one element (flat_hit_uv's operations); rcp_nr2 starts from v_rcp_f32 (within an ulp, a denormal taken for
// zero), here from the division moved by `ulp`
static bool accepts(const float *p0, const float *e1, const float *e2, const float *o, const float *d, float mint, float maxt, int ulp) {
    const float pvx = fmaf(d[1], e2[2], -(d[2] * e2[1])), pvy = fmaf(d[2], e2[0], -(d[0] * e2[2])), pvz = fmaf(d[0], e2[1], -(d[1] * e2[0]));
    const float det = fmaf(e1[2], pvz, fmaf(e1[1], pvy, e1[0] * pvx));
    float r = std::fabs(det) < 1.17549435e-38f ? copysignf(INFINITY, det) : 1.0f / det;       // v_rcp_f32 reads a denormal as zero
    if (ulp && std::isfinite(r)) r = std::nextafterf(r, ulp > 0 ? INFINITY : -INFINITY);
    float e = fmaf(-det, r, 1.0f); r = fmaf(e, r, r);
    e = fmaf(-det, r, 1.0f); r = fmaf(e, r, r);
    const float tx = o[0] - p0[0], ty = o[1] - p0[1], tz = o[2] - p0[2];
    const float u = fmaf(tz, pvz, fmaf(ty, pvy, tx * pvx)) * r;
    const float qx = fmaf(ty, e1[2], -(tz * e1[1])), qy = fmaf(tz, e1[0], -(tx * e1[2])), qz = fmaf(tx, e1[1], -(ty * e1[0]));
    const float v = fmaf(d[2], qz, fmaf(d[1], qy, d[0] * qx)) * r;
    const float t = fmaf(e2[2], qz, fmaf(e2[1], qy, e2[0] * qx)) * r;
    const float uv = u + v;
    return (u >= 0.0f) && (v >= 0.0f) && (uv <= 1.0f) && (t >= mint) && (t <= maxt);
}

static float moved(float x, int ulp) { return ulp == 0 || !std::isfinite(x) ? x : std::nextafterf(x, ulp > 0 ? INFINITY : -INFINITY); }
// the reciprocal as the device forms it: a denormal is read as zero; `ulp` moves the result (v_rcp_f32 is within one)
static float device_inv(float d, int ulp, bool flush) {
    if (flush && std::fabs(d) < 1.17549435e-38f) return copysignf(3.0e38f, d);
    return cull_clamp_inv(moved(1.0f / d, ulp), d);
}

// MASKED: the records carry their pair mask (form 1); else it is shifted together from the counts (form 0)
template <typename Q, bool MASKED>
static uint32_t reach_mask(const std::vector<float4> &recs, uint32_t n_clusters, const float *o, const float *d, const float inv[3], float mint, float maxt, uint64_t &flagged) {
    Q q;
    cull_ray_inv(q, o[0], o[1], o[2], d[0], d[1], d[2], inv[0], inv[1], inv[2]);
    uint32_t pairs = 0u, first = 0u;
    for (uint32_t c = 0; c < n_clusters; ++c) {
        const float4 r0 = recs[2 * c], r1 = recs[2 * c + 1];
        const uint32_t n = cull_count(r0);
        const bool hit = cull_reach(q, r0, r1, mint, maxt);
        flagged += hit;
        if (hit) pairs |= MASKED ? cull_mask(r1) : (uint32_t) ((1ull << n) - 1ull) << first;
        first += n;
    }
    return pairs;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const uint32_t n_scenes = take_u32(f);
    for (uint32_t s = 0; s < n_scenes; ++s) {
        const std::vector<char> name = take<char>(f, take_u32(f));
        const uint32_t n_prims = take_u32(f);
        const std::vector<uint32_t> prim_shape = take<uint32_t>(f, n_prims);
        const std::vector<float> tri_pos = take<float>(f, 9 * (size_t) n_prims);
        const uint32_t n_rays = take_u32(f);
        const std::vector<float> rays = take<float>(f, 8 * (size_t) n_rays);
        const std::vector<uint32_t> kind = take<uint32_t>(f, n_rays);          // 1: an interior ray (the non-vacuity count)

        SceneState st;
        st.n_prims = n_prims; st.geometry.prim_shape = prim_shape;
        st.n_shapes = 0;
        for (uint32_t p : prim_shape) st.n_shapes = std::max(st.n_shapes, p + 1u);
        FlatRecords fr;
        build_flat_records(BuildOptions{}, st, tri_pos, fr);
        if (!fr.flat) { std::printf("scene %.*s not_flat\n", (int) name.size(), name.data()); continue; }
        const uint32_t n_pairs = fr.n_pairs, n_clusters = fr.n_clusters;
        const std::vector<float4> cur(fr.pair_recs.begin() + 5 * (size_t) n_pairs, fr.pair_recs.end());

        // the padded lo / hi boxes, restated from the builder's rule (clusters = runs of pairs whose first primitive has one shape; pad =
        // 1e-4 of the largest coordinate magnitude, 1e-3 at least), and form 0's records of them
        float ext = 0.0f;
        for (float x : tri_pos) ext = std::max(ext, std::fabs(x));
        const float pad = 1e-4f * std::max(ext, 1e-3f);
        std::vector<float4> old;
        uint32_t bad_records = n_clusters * 2u != cur.size();
        for (uint32_t k0 = 0, k1; k0 < n_pairs; k0 = k1) {
            k1 = k0 + 1;
            while (k1 < n_pairs && prim_shape[2 * k1] == prim_shape[2 * k0]) ++k1;
            float lo[3] = { 3e38f, 3e38f, 3e38f }, hi[3] = { -3e38f, -3e38f, -3e38f };
            for (uint32_t gp = 2 * k0; gp < std::min(2 * k1, n_prims); ++gp)
                for (int vtx = 0; vtx < 3; ++vtx) for (int a = 0; a < 3; ++a) {
                    lo[a] = std::min(lo[a], tri_pos[9 * (size_t) gp + 3 * vtx + a]); hi[a] = std::max(hi[a], tri_pos[9 * (size_t) gp + 3 * vtx + a]);
                }
            for (int a = 0; a < 3; ++a) { lo[a] -= pad; hi[a] += pad; }
            float4 r0, r1;
            cull_encode<0>(lo, hi, k0, k1 - k0, r0, r1);
            const size_t c = old.size() / 2;
            old.push_back(r0); old.push_back(r1);
            if (2 * c + 1 >= cur.size()) continue;
            const float4 n0 = cur[2 * c], n1 = cur[2 * c + 1];
            bool ok = cull_count(n0) == k1 - k0;
            if (MTS_FLAT_CULL_FORM) {
                ok = ok && cull_mask(n1) == (uint32_t) ((1ull << (k1 - k0)) - 1ull) << k0;
                const float cc[3] = { n0.x, n0.y, n0.z }, hh[3] = { n1.x, n1.y, n1.z };
                for (int a = 0; a < 3; ++a) ok = ok && (double) cc[a] - (double) hh[a] <= (double) lo[a] && (double) cc[a] + (double) hh[a] >= (double) hi[a];
            } else {
                ok = ok && std::memcmp(&n0, &r0, 16) == 0 && std::memcmp(&n1, &r1, 16) == 0;
            }
            bad_records += !ok;
        }

        // p0, e1, e2 per primitive as the pair records hold them
        std::vector<float> p0(3 * (size_t) n_prims), e1(p0.size()), e2(p0.size());
        for (uint32_t gp = 0; gp < n_prims; ++gp) for (int a = 0; a < 3; ++a) {
            const float *tp = &tri_pos[9 * (size_t) gp];
            p0[3 * gp + a] = tp[a]; e1[3 * gp + a] = tp[3 + a] - tp[a]; e2[3 * gp + a] = tp[6 + a] - tp[a];
        }

        uint64_t viol_cur = 0, viol_lean = 0, viol_old = 0, flagged_cur = 0, flagged_lean = 0, flagged_old = 0, accepted = 0, rays_hit = 0, interior = 0, interior_hit = 0, unused = 0;
        for (uint32_t i = 0; i < n_rays; ++i) {
            const float *o = &rays[8 * (size_t) i], *d = o + 3;
            const float mint = o[6], maxt = o[7];
            uint32_t need = 0u;                // pairs that hold an accepted triangle
            for (uint32_t gp = 0; gp < n_prims; ++gp) {
                bool a = false;
                for (int ulp = -1; ulp <= 1; ++ulp) a = a || accepts(&p0[3 * gp], &e1[3 * gp], &e2[3 * gp], o, d, mint, maxt, ulp);
                if (a) { need |= 1u << (gp >> 1); ++accepted; }
            }
            rays_hit += need != 0u;
            if (kind[i] == 1u) { ++interior; interior_hit += need != 0u; }
            for (int variant = 0; variant < 4; ++variant) {            // exact, +1 ulp, -1 ulp, denormals flushed
                const int ulp = variant == 1 ? 1 : (variant == 2 ? -1 : 0);
                const float inv[3] = { device_inv(d[0], ulp, variant == 3), device_inv(d[1], ulp, variant == 3), device_inv(d[2], ulp, variant == 3) };
#if MTS_FLAT_CULL_FORM
                const uint32_t got = reach_mask<CullFolded, true>(cur, n_clusters, o, d, inv, mint, maxt, variant == 0 ? flagged_cur : unused);
                const uint32_t got_lean = reach_mask<CullLean, true>(cur, n_clusters, o, d, inv, mint, maxt, variant == 0 ? flagged_lean : unused);
#else
                const uint32_t got = reach_mask<CullLoHi, false>(cur, n_clusters, o, d, inv, mint, maxt, variant == 0 ? flagged_cur : unused);
                const uint32_t got_lean = got;
#endif
                viol_cur += (uint64_t) __builtin_popcount(need & ~got);
                viol_lean += (uint64_t) __builtin_popcount(need & ~got_lean);
                if ((need & ~got) && viol_cur < 8)
                    std::fprintf(stderr, "%.*s: ray %u variant %d o %a %a %a d %a %a %a mint %a maxt %a: pairs %08x missed\n", (int) name.size(), name.data(), i, variant,
                                 o[0], o[1], o[2], d[0], d[1], d[2], mint, maxt, need & ~got);
            }
            const float inv[3] = { device_inv(d[0], 0, false), device_inv(d[1], 0, false), device_inv(d[2], 0, false) };
            const uint32_t got = reach_mask<CullLoHi, false>(old, n_clusters, o, d, inv, mint, maxt, flagged_old);
            viol_old += (uint64_t) __builtin_popcount(need & ~got);
        }
        std::printf("scene %.*s form %d clusters %u rays %u rays_hit %llu accepted %llu interior %llu interior_hit %llu violations %llu violations_lean %llu violations_form0 %llu "
                    "flagged %llu flagged_lean %llu flagged_form0 %llu bad_records %u\n", (int) name.size(), name.data(), (int) MTS_FLAT_CULL_FORM, n_clusters, n_rays,
                    (unsigned long long) rays_hit, (unsigned long long) accepted, (unsigned long long) interior, (unsigned long long) interior_hit,
                    (unsigned long long) viol_cur, (unsigned long long) viol_lean, (unsigned long long) viol_old, (unsigned long long) flagged_cur,
                    (unsigned long long) flagged_lean, (unsigned long long) flagged_old, bad_records);
    }
    std::fclose(f);
    return 0;
}

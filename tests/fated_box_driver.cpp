// Stand-alone driver of the fated-path predicates (mitsuba2_amd/csrc/fated.h) for tests/test_fated_box_cpu.py.
//   argv[1] = "boxes", argv[2] = input file: scenes (triangles, the area emitter of each or -1) and rays.  The host builder
//     (emitter_exact_box + set_emitter_boxes, scene_build.cpp) makes the emitter records; counted per scene:
//     - violations: a ray for which the scalar restatement of the pair test accepts an EMISSIVE triangle within [mint, maxt] while no
//       listed box is reached (the clustered loops' query, CullLean; reciprocals exact, an ulp up, an ulp down, denormals read as zero);
//     - reached: rays (exact reciprocals) that reach some box, need: rays that meet an emissive triangle;
//     - bad_records: a padded box that does not contain the exact box + pad, or a list that is not the scene's area emitters.
//   argv[1] = "peek": fated_peek_f32 against the oracle's generator (mo_pcg32_next_f32), and fated_decide against the roulette and depth
//     test of the step written out with that generator.
// It decides nothing: every expectation lives in the test.
#include "scene_build.h"
#include "fated.h"
extern "C" {
#include "mo_math.h"
}

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

// pair_test + tri_accept on one element, as tests/flat_cull_driver.cpp restates them
static bool accepts(const float *p0, const float *e1, const float *e2, const float *o, const float *d, float mint, float maxt, int ulp) {
    const float pvx = fmaf(d[1], e2[2], -(d[2] * e2[1])), pvy = fmaf(d[2], e2[0], -(d[0] * e2[2])), pvz = fmaf(d[0], e2[1], -(d[1] * e2[0]));
    const float det = fmaf(e1[2], pvz, fmaf(e1[1], pvy, e1[0] * pvx));
    float r = std::fabs(det) < 1.17549435e-38f ? copysignf(INFINITY, det) : 1.0f / det;
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
static float device_inv(float d, int ulp, bool flush) {
    if (flush && std::fabs(d) < 1.17549435e-38f) return copysignf(3.0e38f, d);
    return cull_clamp_inv(moved(1.0f / d, ulp), d);
}

static int boxes(const char *path) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return 2;
    const uint32_t n_scenes = take_u32(f);
    for (uint32_t s = 0; s < n_scenes; ++s) {
        const std::vector<char> name = take<char>(f, take_u32(f));
        const uint32_t n_prims = take_u32(f), n_emitters = take_u32(f);
        const std::vector<int32_t> prim_emitter = take<int32_t>(f, n_prims);
        const std::vector<float> tri_pos = take<float>(f, 9 * (size_t) n_prims);
        const uint32_t n_rays = take_u32(f);
        const std::vector<float> rays = take<float>(f, 8 * (size_t) n_rays);

        SceneState st;
        st.n_prims = n_prims;
        st.emitters.assign(n_emitters, DevEmitter{});
        float ext = 0.0f;
        for (int a = 0; a < 3; ++a) { st.bvh.bbox[a] = 3e38f; st.bvh.bbox[3 + a] = -3e38f; }
        for (uint32_t gp = 0; gp < n_prims; ++gp) for (int q = 0; q < 9; ++q) {
            const float x = tri_pos[9 * (size_t) gp + q];
            st.bvh.bbox[q % 3] = std::min(st.bvh.bbox[q % 3], x); st.bvh.bbox[3 + q % 3] = std::max(st.bvh.bbox[3 + q % 3], x);
            ext = std::max(ext, std::fabs(x));
        }
        const float pad = 1e-4f * std::max(ext, 1e-3f);
        std::vector<float> lo(3 * (size_t) n_emitters, 3e38f), hi(3 * (size_t) n_emitters, -3e38f);
        for (uint32_t e = 0; e < n_emitters; ++e) {
            std::vector<float> pts;
            for (uint32_t gp = 0; gp < n_prims; ++gp) if (prim_emitter[gp] == (int32_t) e) pts.insert(pts.end(), &tri_pos[9 * (size_t) gp], &tri_pos[9 * (size_t) gp] + 9);
            emitter_exact_box(pts.data(), pts.size() / 3, st.emitters[e]);
            for (size_t i = 0; i < pts.size(); ++i) { lo[3 * e + i % 3] = std::min(lo[3 * e + i % 3], pts[i]); hi[3 * e + i % 3] = std::max(hi[3 * e + i % 3], pts[i]); }
        }
        set_emitter_boxes(st);
        uint32_t list = 0u;
        if (n_emitters) std::memcpy(&list, &st.emitters[0].aux[kFatedList], 4);

        // the records: box contains exact box + pad; the list names emitters 0 .. n - 1 in order, or is empty above the cap
        uint32_t bad_records = 0u, want = 0u;
        for (uint32_t e = 0; e < n_emitters; ++e) {
            const float *aux = st.emitters[e].aux;
            for (int a = 0; a < 3; ++a) {
                const double c = aux[kFatedBox + a], h = aux[kFatedBox + 4 + a];
                bad_records += !(c - h <= (double) (lo[3 * e + a] - pad) && c + h >= (double) (hi[3 * e + a] + pad));
            }
            if (e < kFatedMaxBoxes) want |= (e + 1u) << (8u * e);
        }
        if (n_emitters == 0u || n_emitters > kFatedMaxBoxes) want = 0u;
        bad_records += list != want;

        std::vector<float> p0(3 * (size_t) n_prims), e1(p0.size()), e2(p0.size());
        for (uint32_t gp = 0; gp < n_prims; ++gp) for (int a = 0; a < 3; ++a) {
            const float *tp = &tri_pos[9 * (size_t) gp];
            p0[3 * gp + a] = tp[a]; e1[3 * gp + a] = tp[3 + a] - tp[a]; e2[3 * gp + a] = tp[6 + a] - tp[a];
        }
        uint64_t violations = 0, need_n = 0, reached = 0;
        for (uint32_t i = 0; i < n_rays && list != 0u; ++i) {
            const float *o = &rays[8 * (size_t) i], *d = o + 3;
            const float mint = o[6], maxt = o[7];
            bool need = false;
            for (uint32_t gp = 0; gp < n_prims && !need; ++gp) {
                if (prim_emitter[gp] < 0) continue;
                for (int ulp = -1; ulp <= 1; ++ulp) need = need || accepts(&p0[3 * gp], &e1[3 * gp], &e2[3 * gp], o, d, mint, maxt, ulp);
            }
            need_n += need;
            for (int variant = 0; variant < 4; ++variant) {            // exact, +1 ulp, -1 ulp, denormals flushed
                const int ulp = variant == 1 ? 1 : (variant == 2 ? -1 : 0);
                CullLean q;
                cull_ray_inv(q, o[0], o[1], o[2], d[0], d[1], d[2], device_inv(d[0], ulp, variant == 3), device_inv(d[1], ulp, variant == 3), device_inv(d[2], ulp, variant == 3));
                bool reach = false;
                for (uint32_t l = list; l != 0u; l >>= 8) reach = reach || fated_reach(q, st.emitters[(l & 0xffu) - 1u].aux, mint, maxt);
                if (variant == 0) reached += reach;
                if (need && !reach) {
                    if (violations < 8)
                        std::fprintf(stderr, "%.*s: ray %u variant %d o %a %a %a d %a %a %a mint %a maxt %a: an emissive triangle is accepted, no box reached\n",
                                     (int) name.size(), name.data(), i, variant, o[0], o[1], o[2], d[0], d[1], d[2], mint, maxt);
                    ++violations;
                }
            }
        }
        // an invalidated record is reached by every ray
        uint64_t invalid_missed = 0;
        if (n_emitters) {
            float aux[16] = { 0 };
            fated_invalidate(aux);
            for (uint32_t i = 0; i < n_rays; ++i) {
                const float *o = &rays[8 * (size_t) i], *d = o + 3;
                const CullLean q = cull_ray<CullLean>(o[0], o[1], o[2], d[0], d[1], d[2]);
                invalid_missed += o[6] <= o[7] && !fated_reach(q, aux, o[6], o[7]);      // (an empty segment, mint > maxt, meets nothing)
            }
        }
        std::printf("scene %.*s emitters %u list %u rays %u need %llu reached %llu violations %llu bad_records %u invalid_missed %llu\n", (int) name.size(), name.data(),
                    n_emitters, list, n_rays, (unsigned long long) need_n, (unsigned long long) reached, (unsigned long long) violations, bad_records,
                    (unsigned long long) invalid_missed);
    }
    std::fclose(f);
    return 0;
}

static int peek() {
    uint64_t peek_mismatch = 0, decide_mismatch = 0, n = 0, fated_n = 0;
    uint64_t mix = 0x9e3779b97f4a7c15ull;
    for (uint32_t stream = 0; stream < 4096; ++stream) {
        mo_pcg32 r;
        mo_pcg32_seed(&r, stream * 0x2545f4914f6cdd1dull + 7u, stream);
        for (int k = 0; k < 64; ++k, ++n) {
            mix = mix * 6364136223846793005ull + 1442695040888963407ull;
            const uint32_t depth = 1u + (uint32_t) (mix >> 60);                            // 1 .. 16
            const int32_t max_depth = (int32_t) ((mix >> 52) & 15u) - 1, rr_depth = 1 + (int32_t) ((mix >> 48) & 7u);      // -1 .. 14, 1 .. 8
            const float hm = (float) ((mix >> 24) & 0xffffu) / 40000.0f, eta = ((mix >> 20) & 3u) == 0u ? 1.5f : 1.0f;   // q on both sides of .95
            const uint64_t state = r.state;
            const float got = fated_peek_f32(state);
            const bool fated = fated_decide(depth, max_depth, rr_depth, hm, eta, state);
            // the next step, for a ray that finds a surface (path.cpp:137-145 as bounce_step writes it)
            bool active = true;
            if ((int32_t) depth > rr_depth) {
                const float q = fminf(hm * (eta * eta), 0.95f);
                const float x = mo_pcg32_next_f32(&r);
                peek_mismatch += std::memcmp(&x, &got, 4) != 0;
                active = x < q;
            } else {
                const float x = mo_pcg32_next_f32(&r);
                peek_mismatch += std::memcmp(&x, &got, 4) != 0;
            }
            const bool dies = depth >= (uint32_t) max_depth || !active;
            decide_mismatch += dies != fated;
            fated_n += fated;
        }
    }
    std::printf("peek n %llu fated %llu peek_mismatch %llu decide_mismatch %llu\n", (unsigned long long) n, (unsigned long long) fated_n,
                (unsigned long long) peek_mismatch, (unsigned long long) decide_mismatch);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "peek") return peek();
    if (argc >= 3 && std::string(argv[1]) == "boxes") return boxes(argv[2]);
    return 2;
}

// kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the wavefront path tracer.
//
//   k_bounce        one path segment per in-flight path: BVH closest hit, surface interaction,
//                   emitter hit + MIS, Russian roulette, emitter sampling + BVH any hit, BSDF
//                   sampling, then ballot/prefix-sum compaction of the surviving paths into the
//                   wave's output segment and regeneration of camera paths into the free slots
//                   (PathIntegrator::sample, src/integrators/path.cpp:100-211; render_sample,
//                   src/librender/integrator.cpp:224-271)
//   k_film_gather   ImageBlock::put as a deterministic per-pixel gather over the per-sample
//                   radiance stream (src/librender/imageblock.cpp:80-172)
//   k_ray_intersect / k_ray_test   Scene::ray_intersect / ray_test on SoA ray streams
//   k_camera_rays, k_imageblock_put, k_put_block, k_film_develop
//
// Scheduling: the in-flight paths live in per-wave segments of the SoA pool.  A scheduling wave
// owns `seg_cap` slots and a private range of sample ordinals; no atomics and no inter-workgroup
// traffic are needed, so the result is independent of dispatch order.
#include "kernels.h"
#include "fated.h"

namespace mtsamd {

constexpr int kBlock = 256;
static_assert(kBlock == 64 * (int) kShadeWaves, "k_shade LDS sizing (kernels.h)");

// ---------------------------------------------------------------------------------------------
struct PathState {
    f3 o, d; float mint, maxt;
    f3 thr; float bs_pdf;
    f3 res; float eta;
    Pcg32 rng;
    uint32_t ordinal, depth, flags;
};

// NT: the pool is a once-read / once-written stream (hierarchy scenes: keep it out of the caches the BVH lives in)
template <bool NT = false>
MTS_DEV void load_state(const PoolView &p, size_t i, PathState &s) {
    float4 a = ld_stream<NT>(p.ray_o + i), b = ld_stream<NT>(p.ray_d + i), c = ld_stream<NT>(p.thr + i), e = ld_stream<NT>(p.res + i);
    uint4 r = ld_stream<NT>(p.rng + i); uint2 m = ld_stream<NT>(p.misc + i);
    s.o = mk3(a.x, a.y, a.z); s.mint = a.w;
    s.d = mk3(b.x, b.y, b.z); s.maxt = b.w;
    s.thr = mk3(c.x, c.y, c.z); s.bs_pdf = c.w;
    s.res = mk3(e.x, e.y, e.z); s.eta = e.w;
    s.rng.state = (uint64_t) r.x | ((uint64_t) r.y << 32);
    s.rng.inc = (uint64_t) r.z | ((uint64_t) r.w << 32);
    s.ordinal = m.x; s.depth = m.y & 0xffffu; s.flags = m.y >> 16;
}
template <bool NT = false>
MTS_DEV void store_state(const PoolView &p, size_t i, const PathState &s) {
    st_stream<NT>(p.ray_o + i, make_float4(s.o.x, s.o.y, s.o.z, s.mint));
    st_stream<NT>(p.ray_d + i, make_float4(s.d.x, s.d.y, s.d.z, s.maxt));
    st_stream<NT>(p.thr + i, make_float4(s.thr.x, s.thr.y, s.thr.z, s.bs_pdf));
    p.res[i] = make_float4(s.res.x, s.res.y, s.res.z, s.eta);      // read-modify-written by the shadow-ray stage: default policy
    st_stream<NT>(p.rng + i, make_uint4((uint32_t) s.rng.state, (uint32_t) (s.rng.state >> 32), (uint32_t) s.rng.inc,
                                        (uint32_t) (s.rng.inc >> 32)));
    st_stream<NT>(p.misc + i, make_uint2(s.ordinal, (s.depth & 0xffffu) | (s.flags << 16)));
}

struct Counters { uint32_t closest, any, segments, tri_tests; };

// Split ("wavefront") pipeline: the two ray queries of a segment run in their own kernels.  `hit` / `found` carry the
// closest hit computed by k_trace<false> into the shading step; the shadow ray and the contribution it guards are
// handed back for k_trace<true>, which adds `nee` to the path's radiance if the ray is unoccluded.
struct Deferred {
    Hit hit; bool found;
    bool pending; f3 so, sd; float smint, smaxt; float nee[4];
};

// One iteration of the path.cpp loop, rotated so that it starts with the intersection of the
// ray spawned by the previous iteration (or by the sensor).  Returns true if the path survives.
// GENERAL = false: every BSDF is a one-sided `diffuse` (the code path of the Cornell-box benchmark, unchanged);
// GENERAL = true: switch over the BSDF models of device_bsdf.h (delta lobes, eta, twosided).
constexpr uint32_t kFlagDelta = 4u;       // the ray was spawned by a delta lobe: no emitter-sampling counterpart (path.cpp:198-203)

// What the emitter-sampling block of the step shows a probe: the sample adds ((mis * thr) * bv) * spec to the radiance if it is unoccluded.
struct NeeTerms {
    const DirectionSample &ds; f3 wi, wo;     // wi, wo: local directions on the BSDF's side of the surface (see kMirrorTwoSided)
    f3 bv, spec; float mis;
    float r1, r2; uint32_t kind;              // kFactoredEmitter: spec = (radiance * r1) * r2 of an emitter of this kind (DevEmitter::pad0)
};

// A probe watches the step: a plain struct whose member functions the step calls where something observable happens, in the order below.
// A derivative of the image is a probe next to the kernel that runs it (k_adjoint*); the step itself holds the primal path and nothing
// else.  NoProbe, the probe of every render kernel, sees nothing: its calls and everything computed only for them compile away.
struct NoProbe {
    static constexpr bool kFactoredEmitter = false;      // the emitter sample keeps r1, r2 and the emitter's kind for NeeTerms
    static constexpr bool kMirrorTwoSided = false;       // the diffuse-only step mirrors wi / wo on the back of a `twosided` diffuse BSDF
    // the probe is shown the emitter sample and the BSDF sample (the last three calls).  The step does not spell those calls out for a probe
    // that does not look: building their arguments alone changed the register allocation of the render kernels (scripts/isa_compare.py)
    static constexpr bool kSamples = false;
    // the step starts (thr, eta on arrival); the probe rejects the modes of the step it cannot ride on
    template <int DEFER, bool GENERAL, bool NEST> MTS_DEV void begin(const PathState &s) { }
    // emission picked up, ew = its MIS weight: the area light `emitter` was hit / the ray escaped into the environment `e`
    MTS_DEV void emitted(float ew, int32_t emitter, f3 le) { }
    MTS_DEV void escaped(const SceneView &sv, const PathState &s, const DevEmitter &e, float ew, f3 le) { }
    // Russian roulette: thr before the division by q = 1 / rq, hm = hmax(thr); `free`: q was not clamped to .95
    MTS_DEV void roulette(f3 thr, float hm, float rq, bool free) { }
    // the path goes on at a surface whose reflectance `refl` was looked up (texel, tw1: bilinear footprint); thr after roulette
    MTS_DEV void surface(const SurfaceInteraction &si, const DevBsdf &bsdf, f3 refl, uint32_t texel, f2 tw1, f3 thr) { }
    // an emitter sample was evaluated.  true: trace its shadow ray even if it contributes nothing; then, if the ray is unoccluded:
    MTS_DEV bool emitter_sample(const SceneView &sv, const DevBsdf &bsdf, f3 refl, const NeeTerms &t) { return false; }
    MTS_DEV void unoccluded(const SceneView &sv, const SurfaceInteraction &si, f3 thr, const NeeTerms &t) { }
    // the general step drew the BSDF sample `bs` with the numbers s1, s2; thr before it is multiplied by `weight`
    MTS_DEV void bsdf_sampled(const SceneView &sv, const SurfaceInteraction &si, const DevBsdf &bsdf, f3 refl, f3 thr, const BsdfSample &bs, f3 weight, float s1, f2 s2) { }
};

// `table(i)` of surface_bsdf_sample / surface_bsdf_eval_pdf: record i of the scene's BSDF table as the model code reads it at `uv`.  The
// NEST instantiation resolves the textured parameters of the record -- a blend / mask child, right where it replaces the working record
// (cur = table(child)); NEST = false is the plain load (and is never called: only nests have children).
template <bool NEST, bool FLAT> struct BsdfTable;
template <bool FLAT> struct BsdfTable<false, FLAT> {
    const Geo<FLAT> &geo;
    MTS_DEV BsdfTable(const Geo<FLAT> &g, const f2 &) : geo(g) { }
    MTS_DEV DevBsdf operator()(uint32_t i) const { return geo.bsdf(i); }
};
template <bool FLAT> struct BsdfTable<true, FLAT> {
    const Geo<FLAT> &geo; const f2 &uv;
    MTS_DEV BsdfTable(const Geo<FLAT> &g, const f2 &t) : geo(g), uv(t) { }
    MTS_DEV DevBsdf operator()(uint32_t i) const { DevBsdf rec = geo.bsdf(i); resolve_textured(geo.sv, rec, uv); return rec; }
};

// Fated paths (fated.h): called by the render steps (NoProbe / NoProbeS) on the state they hand to the next step -- the ray
// just spawned, depth already incremented, hm = hmax(thr).  true: that step would end the path whatever it finds (max_depth, or a
// roulette that is already decided) and the ray cannot reach the triangles of any area emitter, so it could not add emission either.
// The query is then counted as the step that ran it would have counted it, and the caller ends the path.  Off, wave-uniformly, where
// the scene's list is empty (an environment emitter, no area emitter, more than kFatedMaxBoxes of them: set_emitter_boxes).
template <bool FLAT>
MTS_DEV bool fated_elide(const RenderParams &P, const LdsView &lds, const f3 &o, const f3 &d, float mint, float maxt, float hm, float eta, uint32_t depth,
                         uint64_t rng_state, Counters &c) {
    const SceneView &sv = P.sv;
    if (sv.env_emitter >= 0 || sv.n_emitters == 0u) return false;
    const DevEmitter *em = FLAT ? lds.emitters : sv.emitters;
    const uint32_t list = __float_as_uint(em[0].aux[kFatedList]);
    if (list == 0u) return false;
    if (!fated_decide(depth, P.max_depth, P.rr_depth, hm, eta, rng_state)) return false;
    const CullLean q = cull_ray<CullLean>(o.x, o.y, o.z, d.x, d.y, d.z);
    for (uint32_t l = list; l != 0u; l >>= 8)
        if (fated_reach(q, em[(l & 0xffu) - 1u].aux, mint, maxt)) return false;
    if (!MTS_FATED_STATS) ++c.closest;
    ++c.segments;
    if (FLAT && !(MTS_CULL_STATS & 1)) c.tri_tests += sv.n_prims;      // the nominal count of the flat closest-hit loops (device_scene.h)
    return true;
}

// DEFER: 0 = both ray queries inline (fused kernel); 1 = closest hit precomputed + shadow ray queued (split pipeline of
// hierarchy scenes); 2 = closest hit inline, shadow ray queued (flat scenes: the any-hit loop then runs on dense batches)
// ELIDE = false: without the fated-path rule (k_mega on diffuse RGB hierarchy scenes, where its registers cost an occupancy step)
template <bool FLAT, int DEFER = 0, bool GENERAL = false, bool NEST = false, class Probe = NoProbe, bool ELIDE = true>
MTS_DEV bool bounce_step(const RenderParams &P, const LdsView &lds, PathState &s, Counters &c, Probe &&probe = Probe{}, Deferred *df = nullptr) {
    using Pr = std::remove_reference_t<Probe>;
    static_assert(!NEST || (GENERAL && DEFER == 0), "blendbsdf / mask run the general fused step");
    const SceneView &sv = P.sv;
    probe.template begin<DEFER, GENERAL, NEST>(s);
    const Geo<FLAT> geo{ sv, lds };
    Hit hit;
    ++c.closest; ++c.segments;
    bool found;
    if (DEFER) df->pending = false;
    if (DEFER == 1) { hit = df->hit; found = df->found; }
    else found = traverse<FLAT, false>(sv, lds, s.o, s.d, s.mint, s.maxt, hit, c.tri_tests,
                                       FLAT && __ballot(s.depth != 1u) == 0ull);      // all active lanes carry camera rays: cluster culling
    if (s.depth == 1u) s.flags = found ? 1u : 0u;          // valid_ray (path.cpp:121)

    SurfaceInteraction si;
    if (found) {
        fill_si(geo, s.d, hit.prim, hit.u, hit.v, si);
        int32_t emitter = si.shape_rec.emitter;
        if (emitter >= 0) {
            const DevEmitter e = geo.emitter((uint32_t) emitter);
            // emission_weight of the previous iteration (path.cpp:194-205); 1 for camera rays
            float ew = 1.0f;
            if (s.depth > 1u) {
                f3 dd = si.p - s.o;                         // DirectionSample(si_bsdf, si), records.h:168-174
                float dist = sqrtf(sqnorm(dd));
                dd = div_s(dd, dist);
                const float pe = pdf_emitter_direction(sv.n_emitters, e.area_norm, dd, si.sh.n, dist);
                ew = mis_weight(s.bs_pdf, (GENERAL && (s.flags & kFlagDelta)) ? 0.0f : pe);
            }
            if (si.wi.z > 0.0f) {                           // AreaLight::eval (area.cpp:71-79)
                s.res.x += (ew * s.thr.x) * e.r; s.res.y += (ew * s.thr.y) * e.g; s.res.z += (ew * s.thr.z) * e.b;
                probe.emitted(ew, emitter, mk3(e.r, e.g, e.b));
            }
        }
    }
    if (GENERAL && !found && sv.env_emitter >= 0) {          // si.emitter(scene) of an escaped ray: the environment
        const DevEmitter e = geo.emitter((uint32_t) sv.env_emitter);
        float ew = 1.0f;
        if (s.depth > 1u) ew = mis_weight(s.bs_pdf, (GENERAL && (s.flags & kFlagDelta)) ? 0.0f : pdf_environment(sv, e, s.d));
        const f3 le = environment_radiance(sv, e, s.d);
        s.res.x += (ew * s.thr.x) * le.x; s.res.y += (ew * s.thr.y) * le.y; s.res.z += (ew * s.thr.z) * le.z;
        probe.escaped(sv, s, e, ew, le);
    }
    bool active = found;

    // Russian roulette (path.cpp:137-141)
    if ((int32_t) s.depth > P.rr_depth) {
        float hm = fmaxf(fmaxf(s.thr.x, s.thr.y), s.thr.z);
        float q = fminf(hm * (s.eta * s.eta), 0.95f);
        if (active) active = pcg_next_f32(s.rng) < q;
        float rq = rcp(q);
        probe.roulette(s.thr, hm, rq, hm * (s.eta * s.eta) < 0.95f);
        s.thr = s.thr * rq;
    }
    if (s.depth >= (uint32_t) P.max_depth || !active) return false;

    DevBsdf bsdf = geo.bsdf((uint32_t) si.shape_rec.bsdf);      // blend / mask: overwritten with the child in use (surface_bsdf_*)
    if (NEST) resolve_textured(sv, bsdf, si.uv);             // textured alpha / specular colours of the record of the hit
    uint32_t texel; f2 tw1;
    const f3 refl = eval_reflectance(sv, bsdf, si.uv, texel, tw1);
    const NestInfo ni = nest_info<NEST>(bsdf, refl.x, refl.y, refl.z);
    auto child_refl = [&](const DevBsdf &rec) { uint32_t t; f2 w; return eval_reflectance(sv, rec, si.uv, t, w); };      // blend / mask children
    const bool smooth = !GENERAL || bsdf_is_smooth(bsdf);
    probe.surface(si, bsdf, refl, texel, tw1, s.thr);
    // kMirrorTwoSided: a `twosided` diffuse BSDF (twosided.cpp:94-175; the primal render of such a scene runs the GENERAL kernels, whose
    // diffuse branch does the same arithmetic): the back side scatters like the front side, mirrored
    f3 wi_b = si.wi;
    const bool flip = Pr::kMirrorTwoSided && !GENERAL && (bsdf.flags & kBsdfTwoSided) != 0u && wi_b.z < 0.0f;
    if (flip) wi_b.z = -wi_b.z;

    // --------------------- Emitter sampling (path.cpp:153-172) ---------------------
    if (smooth) {                                            // active_e: only BSDFs with a smooth component (path.cpp:154)
        f2 s2; s2.x = pcg_next_f32(s.rng); s2.y = pcg_next_f32(s.rng);
        DirectionSample ds; f3 spec;
        float r1 = 0.0f, r2 = 0.0f; uint32_t kind = 0u;
        if (Pr::kFactoredEmitter) {          // the wrapper below, keeping its factors
            sample_emitter_direction<FLAT, GENERAL>(geo, si.p, s2, ds, r1, r2);
            spec = mk3(0.0f, 0.0f, 0.0f);
            if (sv.n_emitters != 0u) {
                const DevEmitter e = geo.emitter(ds.emitter);
                f3 rad = mk3(e.r, e.g, e.b);
                if (GENERAL && e.pad0 == kEmitterEnvmap) rad = envmap_lookup(*sv.envmap, ds.uv.x, ds.uv.y);
                if (GENERAL && ds.delta) rad = mk3(rad.x * ds.falloff, rad.y * ds.falloff, rad.z * ds.falloff);
                spec = mk3(rad.x * r1, rad.y * r1, rad.z * r1);
                if (sv.n_emitters > 1u) spec = spec * r2;
                kind = e.pad0;
            }
        } else sample_emitter_direction<FLAT, GENERAL>(geo, si.p, s2, ds, spec);
        if (ds.pdf != 0.0f) {
            f3 wo = to_local(si.sh, ds.d);
            const f3 wo_b = flip ? mk3(wo.x, wo.y, -wo.z) : wo;
            f3 bv; float bp;
            if (GENERAL) surface_bsdf_eval_pdf<NEST>(bsdf, ni, refl, BsdfTable<NEST, FLAT>(geo, si.uv), child_refl, si.wi, wo, bv, bp);
            else diffuse_eval_pdf(refl, wi_b, wo_b, bv, bp);
            float mis = (GENERAL && ds.delta) ? 1.0f : mis_weight(ds.pdf, bp);      // path.cpp:170
            f3 contrib = mk3(((mis * s.thr.x) * bv.x) * spec.x, ((mis * s.thr.y) * bv.y) * spec.y,
                             ((mis * s.thr.z) * bv.z) * spec.z);
            auto nee = [&] { return NeeTerms{ ds, wi_b, wo_b, bv, spec, mis, r1, r2, kind }; };
            bool watched = false;
            if (Pr::kSamples) watched = probe.emitter_sample(sv, bsdf, refl, nee());
            // The visibility test only ever zeroes `spec` (scene.cpp:178-182): trace the shadow
            // ray only if an unoccluded sample would contribute.
            if (DEFER) {
                if (contrib.x != 0.0f || contrib.y != 0.0f || contrib.z != 0.0f) {
                    ++c.any;
                    df->pending = true; df->so = si.p; df->sd = ds.d;
                    df->smint = kRayEpsilon * (1.0f + hmax_abs(si.p)); df->smaxt = ds.dist * (1.0f - kShadowEpsilon);
                    df->nee[0] = contrib.x; df->nee[1] = contrib.y; df->nee[2] = contrib.z; df->nee[3] = 0.0f;
                }
            } else if (contrib.x != 0.0f || contrib.y != 0.0f || contrib.z != 0.0f || watched) {
                Hit sh;
                ++c.any;
#if defined(MTS_ABLATE_SHADOW)   // diagnostic build only: wrong image, used to price the any-hit loop in situ
                bool occluded = false;
#else
                bool occluded = traverse<FLAT, true>(sv, lds, si.p, ds.d, kRayEpsilon * (1.0f + hmax_abs(si.p)),
                                               ds.dist * (1.0f - kShadowEpsilon), sh, c.tri_tests);
#endif
                if (!occluded) {
                    s.res = s.res + contrib;
                    if (Pr::kSamples) probe.unoccluded(sv, si, s.thr, nee());
                }
            }
        }
    }

    // ----------------------- BSDF sampling (path.cpp:177-190) ----------------------
    const float s1 = pcg_next_f32(s.rng);                    // sample1 (lobe selection; unused by SmoothDiffuse)
    f2 s2; s2.x = pcg_next_f32(s.rng); s2.y = pcg_next_f32(s.rng);
    f3 wo, weight; float pdf;
    if (GENERAL) {
        BsdfSample bs;
        surface_bsdf_sample<NEST>(bsdf, ni, refl, BsdfTable<NEST, FLAT>(geo, si.uv), child_refl, si.wi, s1, s2, bs, weight);
        wo = bs.wo; pdf = bs.pdf;
        s.eta *= bs.eta;                                     // harmless for a failed sample: the path ends below
        s.flags = bs.delta ? (s.flags | kFlagDelta) : (s.flags & ~kFlagDelta);
        if (Pr::kSamples) probe.bsdf_sampled(sv, si, bsdf, refl, s.thr, bs, weight, s1, s2);
    } else {
        diffuse_sample(refl, wi_b, s2, wo, pdf, weight);     // eta *= bs.eta (== 1)
        if (flip) wo.z = -wo.z;
    }
    s.thr = mk3(s.thr.x * weight.x, s.thr.y * weight.y, s.thr.z * weight.z);
    if (!(s.thr.x != 0.0f || s.thr.y != 0.0f || s.thr.z != 0.0f)) return false;
    s.o = si.p;                                              // spawn_ray (interaction.h:58-61)
    s.d = to_world(si.sh, wo);
    s.mint = (1.0f + hmax_abs(si.p)) * kRayEpsilon;
    s.maxt = __builtin_inff();
    s.bs_pdf = pdf;
    s.depth += 1u;
    if constexpr (MTS_FATED_ELIDE && ELIDE && std::is_same_v<Pr, NoProbe>)        // render kernels only: a probe sees every step
        if (fated_elide<FLAT>(P, lds, s.o, s.d, s.mint, s.maxt, fmaxf(fmaxf(s.thr.x, s.thr.y), s.thr.z), s.eta, s.depth, s.rng.state, c)) return false;
    return true;
}

// render_sample up to the camera ray (integrator.cpp:224-246).  `lp` = local pixel index (row-major over the rows
// this render owns), `j` = sample number inside the pixel; the RNG stream is seeded with the GLOBAL sample index
// pixel * spp + j, so the image does not depend on how the film is partitioned.
template <bool GENERAL = true>
MTS_DEV void generate_path(const RenderParams &P, uint64_t ordinal, uint32_t lp, uint32_t j, PathState &s, float2 *pos_out = nullptr) {
    const uint32_t w = (uint32_t) P.crop_w;
    const uint32_t lr = lp / w, px = lp - lr * w;
    const uint32_t py = (uint32_t) row_to_global(P.rows, (int32_t) lr);
    const uint64_t index = ((uint64_t) py * w + px) * (uint64_t) P.spp + j;
    seed_sample(s.rng, index, P.base_seed);
    float jx = pcg_next_f32(s.rng), jy = pcg_next_f32(s.rng);
    float psx = ((float) px + (float) P.crop_x) + jx, psy = ((float) py + (float) P.crop_y) + jy;
    f2 ap; ap.x = ap.y = 0.5f;                               // needs_aperture_sample(): integrator.cpp:229-231
    if (GENERAL && P.cam.aperture_radius > 0.0f) { ap.x = pcg_next_f32(s.rng); ap.y = pcg_next_f32(s.rng); }
    (void) pcg_next_f32(s.rng);                              // wavelength sample (drawn even in RGB mode)
    float ax = (psx - (float) P.crop_x) / (float) P.crop_w, ay = (psy - (float) P.crop_y) / (float) P.crop_h;
    camera_ray<GENERAL>(P.cam, ax, ay, ap, s.o, s.d, s.mint, s.maxt);
    s.thr = mk3(1.0f, 1.0f, 1.0f); s.bs_pdf = 0.0f;
    s.res = mk3(0.0f, 0.0f, 0.0f); s.eta = 1.0f;
    s.ordinal = P.plane_pixels ? j * P.plane_pixels + (lp - P.plane_pix0) : (uint32_t) (ordinal - P.first_ordinal);
    s.depth = 1u; s.flags = 0u;
    if (P.out_pos) P.out_pos[s.ordinal] = make_float2(psx, psy);
    if (pos_out) *pos_out = make_float2(psx, psy);
}

// final radiance of a terminated path -> per-sample stream
MTS_DEV void store_result(const RenderParams &P, const PathState &s) {
    float alpha = (s.flags & 1u) ? 1.0f : 0.0f;
    if (P.store_xyz) {
        f3 xyz = P.store_xyz == 1 ? srgb_to_xyz(s.res) : s.res;   // integrator.cpp:254-262; 2: linear RGB film (autodiff.py:53-57)
        // ImageBlock::put drops invalid samples (imageblock.cpp:85-109); the autodiff film is created with
        // warn_negative = False (autodiff.py:60-67), so there only non-finite values are dropped
        const float lo = P.store_xyz == 1 ? -1e-5f : -__builtin_inff();
        bool valid = (xyz.x >= lo) && (xyz.y >= lo) && (xyz.z >= lo) && isfinite(xyz.x) && isfinite(xyz.y) && isfinite(xyz.z);
        P.out_rgba[s.ordinal] = make_float4(xyz.x, xyz.y, xyz.z, valid ? alpha : -1.0f);
    } else {
        P.out_rgba[s.ordinal] = make_float4(s.res.x, s.res.y, s.res.z, alpha);
    }
}

// Sample ordinals are dealt to the scheduling waves in chunks of P.chunk, round-robin: wave k traces the chunks k, k + n_waves, ... of
// the pass.  LDS-resident scenes use chunks of 64, so that every wave sees the same mix of cheap and expensive pixels and the pool
// stays full until all cursors run dry together (contiguous ranges per wave left waves over easy pixels idle from a third of the pass
// on: 94 -> 82 launches per render); hierarchy scenes keep one chunk per wave -- consecutive pixels -- because the rays of a
// workgroup's scheduling waves should walk the same part of the BVH (64-sample chunks cost them 5 %).  The cursor of a wave counts
// its own samples; this maps the v-th of them to its place in the pass, (local pixel, sample number) included.  Which wave traces a
// sample has no influence on the result: its RNG stream and its slot in the sample stream depend on the ordinal alone.
MTS_DEV void cursor_sample(const RenderParams &P, uint32_t wave, uint64_t v, uint64_t &ordinal, uint32_t &lp, uint32_t &j) {
    const uint32_t t = (uint32_t) v / P.chunk, within = (uint32_t) v - t * P.chunk;
    const uint32_t in_pass = (t * P.n_waves + chunk_owner(wave, P.n_waves, P.n_chains)) * P.chunk + within;      // < 2^31
    ordinal = P.first_ordinal + in_pass;
    const uint32_t r = in_pass + P.first_rem, q = r / (uint32_t) P.spp;
    lp = P.first_pix + q; j = r - q * (uint32_t) P.spp;
}

#ifndef MTS_BOUNCE_WAVES
#define MTS_BOUNCE_WAVES 4
#endif
template <bool FLAT, bool GENERAL, bool NEST = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(MTS_BOUNCE_WAVES, MTS_BOUNCE_WAVES)))
void k_bounce(const RenderParams P) {
    extern __shared__ float4 smem[];
    const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6;
    {   // a workgroup whose scheduling waves are all idle (pool drain at the end of a pass) leaves before staging the scene
        const bool work = wave < P.n_waves && (P.count_in[wave] > 0u || P.cursor[wave] < P.cursor_end[wave]);
        if (!__syncthreads_or(work ? 1 : 0)) {
            if (wave < P.n_waves && lane_id() == 0u) P.count_out[wave] = 0u;
            return;
        }
    }
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    if (wave >= P.n_waves) return;
    const uint32_t lane = lane_id();
    const uint32_t n_in = __builtin_amdgcn_readfirstlane(P.count_in[wave]);
    const size_t base = (size_t) wave * P.seg_cap;
    uint32_t n_out = 0;
    Counters c = { 0u, 0u, 0u, 0u };

    for (uint32_t i0 = 0; i0 < n_in; i0 += 64u) {
        PathState s;
        bool alive = false;
        if (i0 + lane < n_in) {
            load_state(P.in, base + i0 + lane, s);
            alive = bounce_step<FLAT, 0, GENERAL, NEST>(P, lds, s, c);
            if (!alive) store_result(P, s);
        }
        // wavefront ballot + prefix rank: compact the survivors to the front of the output segment
        const uint64_t m = __ballot(alive);
        if (alive) store_state(P.out, base + n_out + mask_rank(m), s);
        n_out += (uint32_t) __popcll(m);
    }

    // regenerate camera paths into the free slots of this wave's segment.  The cursor is kept decomposed as
    // (local pixel, sample-in-pixel) so that no 64-bit division is needed per generated path.
    uint64_t cursor = P.cursor[wave];
    const uint64_t end = P.cursor_end[wave];
    while (n_out < P.target && cursor < end) {
        uint64_t left = end - cursor;
        uint32_t n_new = min(64u, P.target - n_out);
        if ((uint64_t) n_new > left) n_new = (uint32_t) left;
        if (lane < n_new) {
            PathState s;
            uint64_t ordinal; uint32_t lp, sj;
            cursor_sample(P, wave, cursor + lane, ordinal, lp, sj);
            generate_path<GENERAL>(P, ordinal, lp, sj, s);
            store_state(P.out, base + n_out + lane, s);
        }
        n_out += n_new; cursor += n_new;
    }

    // per-wave bookkeeping (each wave owns its slots: no atomics)
    uint32_t tot[4] = { c.closest, c.any, c.segments, c.tri_tests };
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int off = 32; off > 0; off >>= 1) tot[k] += __shfl_xor(tot[k], off);
    if (lane == 0) {
        P.count_out[wave] = n_out;
        P.cursor[wave] = cursor;
        uint64_t *ws = P.wave_stats + 4u * (size_t) wave;
        ws[0] += tot[0]; ws[1] += tot[1]; ws[2] += tot[2]; ws[3] += tot[3];
    }
}

size_t bounce_lds_bytes(const SceneView &sv) { return lds_bytes(sv, kBlock); }
// Dynamic LDS above 48 KiB is something a kernel opts into.  Deep hierarchies ask for that much, and so do flat scenes with large shape,
// BSDF or emitter tables (kernels.h, flat_launch_lds_max): every launch whose LDS grows with the scene goes through launch_lds, which
// opts the instantiation it launches into the byte count it passes.
static hipError_t allow_lds(const void *fn, size_t bytes) {
    return bytes > 48u * 1024u ? hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes) : hipSuccess;
}
template <typename... P, typename... A>
static hipError_t launch_lds(void (*fn)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A &&...args) {
    if (hipError_t e = allow_lds(reinterpret_cast<const void *>(fn), lds)) return e;
    hipLaunchKernelGGL(fn, grid, block, lds, s, static_cast<P>(args)...);
    return hipGetLastError();
}


// ---------------------------------------------------------------------------------------------
// Spectral variant: the same path logic on 4 wavelengths per camera sample (scalar_spectral / gpu_spectral semantics).
// Geometry, sampling decisions and the RNG consumption are wavelength independent; reflectances and emission are
// smooth spectra evaluated per wavelength, and the result is converted to XYZ with the CIE 1931 observer.
__device__ SpectralTables g_spectral;

hipError_t upload_spectral_tables(const float *x, const float *y, const float *z, const float *d65) {
    SpectralTables t;
    for (int i = 0; i < 95; ++i) { t.x[i] = x[i]; t.y[i] = y[i]; t.z[i] = z[i]; t.d65[i] = d65[i]; }
    return hipMemcpyToSymbol(HIP_SYMBOL(g_spectral), &t, sizeof(t));
}

struct PathStateS {
    f3 o, d; float mint, maxt;
    Spec4 thr, res, wav; float bs_pdf, eta, xi;      // wav = wavelengths_from_sample(xi): not stored
    Pcg32 rng;
    uint32_t ordinal, depth, flags;
};

// The path state of a spectral scene that binds tabulated / analytic spectra: the same record; the type selects the instantiations of the
// schedules (k_shade, k_mega, k_finish) whose step evaluates the spectrum pool, and leaves those of every other scene as they are.
struct PathStateT : PathStateS { };

template <bool NT = false>
MTS_DEV void load_state(const PoolView &p, size_t i, PathStateS &s) {
    float4 a = ld_stream<NT>(p.ray_o + i), b = ld_stream<NT>(p.ray_d + i), c = ld_stream<NT>(p.thr + i), e = ld_stream<NT>(p.res + i);
    s.xi = ld_stream<NT>(p.xi + i);
    wavelengths_from_sample(s.xi, s.wav);
    float2 x = ld_stream<NT>(p.aux + i); uint4 r = ld_stream<NT>(p.rng + i); uint2 m = ld_stream<NT>(p.misc + i);
    s.o = mk3(a.x, a.y, a.z); s.mint = a.w;
    s.d = mk3(b.x, b.y, b.z); s.maxt = b.w;
    s.thr.v[0] = c.x; s.thr.v[1] = c.y; s.thr.v[2] = c.z; s.thr.v[3] = c.w;
    s.res.v[0] = e.x; s.res.v[1] = e.y; s.res.v[2] = e.z; s.res.v[3] = e.w;
    s.bs_pdf = x.x; s.eta = x.y;
    s.rng.state = (uint64_t) r.x | ((uint64_t) r.y << 32);
    s.rng.inc = (uint64_t) r.z | ((uint64_t) r.w << 32);
    s.ordinal = m.x; s.depth = m.y & 0xffffu; s.flags = m.y >> 16;
}
template <bool NT = false>
MTS_DEV void store_state(const PoolView &p, size_t i, const PathStateS &s) {
    st_stream<NT>(p.ray_o + i, make_float4(s.o.x, s.o.y, s.o.z, s.mint));
    st_stream<NT>(p.ray_d + i, make_float4(s.d.x, s.d.y, s.d.z, s.maxt));
    st_stream<NT>(p.thr + i, make_float4(s.thr.v[0], s.thr.v[1], s.thr.v[2], s.thr.v[3]));
    p.res[i] = make_float4(s.res.v[0], s.res.v[1], s.res.v[2], s.res.v[3]);      // read-modify-written by the shadow-ray stage
    st_stream<NT>(p.xi + i, s.xi);
    st_stream<NT>(p.aux + i, make_float2(s.bs_pdf, s.eta));
    st_stream<NT>(p.rng + i, make_uint4((uint32_t) s.rng.state, (uint32_t) (s.rng.state >> 32), (uint32_t) s.rng.inc,
                                        (uint32_t) (s.rng.inc >> 32)));
    st_stream<NT>(p.misc + i, make_uint2(s.ordinal, (s.depth & 0xffffu) | (s.flags << 16)));
}

// spectral variant: `srgb` parameters evaluate the upsampled colour at each wavelength (srgb.cpp:45-52), `uniform` ones are
// constants; conductors carry uniform eta / k.  spectral_channels_tab (a scene that binds spectra, SceneView::n_spectra): a parameter
// with a tabulated spectrum (DevBsdf::spectra0 / spectra1) evaluates it at each wavelength instead -- regular.cpp:68-75,
// irregular.cpp:76-83 -- and that includes eta / k of conductors.  Only the step instantiated with TAB calls it.
MTS_DEV SpectrumPool spectrum_pool(const SceneView &sv) {
    const DevSpectrum *headers = reinterpret_cast<const DevSpectrum *>(sv.bsdfs + sv.n_bsdfs);
    return SpectrumPool{ headers, reinterpret_cast<const float *>(headers + sv.n_spectra) };
}
MTS_DEV BsdfChannels<kWav> spectral_channels_tab(const DevBsdf &b, const Spec4 &wav, const SceneView &sv) {
    BsdfChannels<kWav> c;
    const SpectrumPool pool = spectrum_pool(sv);
    const uint32_t t_refl = bsdf_spectrum(b, kSpecRefl), t_spec = bsdf_spectrum(b, kSpecSpec), t_trans = bsdf_spectrum(b, kSpecTrans),
                   t_eta = bsdf_spectrum(b, kSpecEta), t_k = bsdf_spectrum(b, kSpecK);
#pragma unroll
    for (int k = 0; k < kWav; ++k) {
        const float l = wav.v[k];
        c.refl[k] = t_refl ? spectrum_eval(pool, t_refl - 1u, l) : (b.flags & kBsdfUniformRefl) ? b.r : srgb_model_eval(b.c0, b.c1, b.c2, l);
        c.spec[k] = t_spec ? spectrum_eval(pool, t_spec - 1u, l) : (b.flags & kBsdfUniformSpec) ? b.sr : srgb_model_eval(b.sc0, b.sc1, b.sc2, l);
        c.trans[k] = t_trans ? spectrum_eval(pool, t_trans - 1u, l) : (b.flags & kBsdfUniformTrans) ? b.kr : srgb_model_eval(b.tc0, b.tc1, b.tc2, l);
        c.eta[k] = t_eta ? spectrum_eval(pool, t_eta - 1u, l) : b.er;
        c.k[k] = t_k ? spectrum_eval(pool, t_k - 1u, l) : b.kr;
    }
    return c;
}
MTS_DEV BsdfChannels<kWav> spectral_channels(const DevBsdf &b, const Spec4 &wav) {
    BsdfChannels<kWav> c;
#pragma unroll
    for (int k = 0; k < kWav; ++k) {
        c.refl[k] = (b.flags & kBsdfUniformRefl) ? b.r : srgb_model_eval(b.c0, b.c1, b.c2, wav.v[k]);
        c.spec[k] = (b.flags & kBsdfUniformSpec) ? b.sr : srgb_model_eval(b.sc0, b.sc1, b.sc2, wav.v[k]);
        c.trans[k] = (b.flags & kBsdfUniformTrans) ? b.kr : srgb_model_eval(b.tc0, b.tc1, b.tc2, wav.v[k]);
        c.eta[k] = b.er; c.k[k] = b.kr;
    }
    return c;
}

// radiance spectrum of an emitter at the path's 4 wavelengths: SRGBEmitterSpectrum::eval = d65 * srgb_model_eval
// (srgb_d65.cpp:54-62) for `area` / `constant`; eval_spectrum's spectral branch (envmap.cpp:283-306) at texture
// coordinates (u, v) for `envmap`, whose texels hold (model coefficients, scale) and whose whitepoint is D65 / 10568
MTS_DEV Spec4 envmap_lookup_spectral(const DevEnvmap &e, float u, float v, const Spec4 &wav) {
    u *= (float) (e.w - 1); v *= (float) (e.h - 1);
    const uint32_t px = min((uint32_t) u, (uint32_t) (e.w - 2)), py = min((uint32_t) v, (uint32_t) (e.h - 2));
    const float w1x = u - (float) px, w1y = v - (float) py, w0x = 1.0f - w1x, w0y = 1.0f - w1y;
    const float4 *p = e.data + (size_t) py * e.w + px;
    const float4 v00 = p[0], v10 = p[1], v01 = p[e.w], v11 = p[e.w + 1];
    const float f0 = fmaf(w0x, v00.w, w1x * v10.w), f1 = fmaf(w0x, v01.w, w1x * v11.w);
    const float f = fmaf(w0y, f0, w1y * f1);
    Spec4 r;
#pragma unroll
    for (int k = 0; k < kWav; ++k) {
        const float l = wav.v[k];
        const float s00 = srgb_model_eval(v00.x, v00.y, v00.z, l), s10 = srgb_model_eval(v10.x, v10.y, v10.z, l);
        const float s01 = srgb_model_eval(v01.x, v01.y, v01.z, l), s11 = srgb_model_eval(v11.x, v11.y, v11.z, l);
        const float s0 = fmaf(w0x, s00, w1x * s10), s1 = fmaf(w0x, s01, w1x * s11);
        const float sp = fmaf(w0y, s0, w1y * s1);
        const float wp = table_eval(g_spectral.d65, 1.0f / 10568.0f, l);
        r.v[k] = ((sp * wp) * f) * e.scale;
    }
    return r;
}
// textured reflectance in the spectral variant: bitmap texels hold srgb model coefficients, evaluated at the four corners and
// then interpolated (bitmap.cpp:274-286); checkerboard colours are `srgb` spectra (checkerboard.cpp:46-63).  texel, w1: the bilinear
// footprint of a bitmap lookup, as eval_reflectance hands it out (kNoPrim: a checkerboard)
MTS_DEV Spec4 eval_reflectance_spectral(const SceneView &sv, const DevBsdf &b, f2 uv, const Spec4 &wav, uint32_t &texel, f2 &w1) {
    texel = kNoPrim; w1.x = w1.y = 0.0f;
    const DevTexture t = sv.textures[b.texture];
    {
        const float u2 = fmaf(t.uvm[0], uv.x, fmaf(t.uvm[1], uv.y, t.uvm[2])), v2 = fmaf(t.uvm[3], uv.x, fmaf(t.uvm[4], uv.y, t.uvm[5]));
        uv.x = u2; uv.y = v2;
    }
    Spec4 r;
    if (t.kind == 1u) {
        const bool mx = (uv.x - floorf(uv.x)) > 0.5f, my = (uv.y - floorf(uv.y)) > 0.5f;
        const float *c = mx == my ? t.c0 : t.c1;
        const float a0 = c[0], a1 = c[1], a2 = c[2];
#pragma unroll
        for (int k = 0; k < kWav; ++k) r.v[k] = srgb_model_eval(a0, a1, a2, wav.v[k]);
        return r;
    }
    float ux = uv.x - floorf(uv.x), uy = uv.y - floorf(uv.y);
    ux *= (float) (uint32_t) (t.w - 1); uy *= (float) (uint32_t) (t.h - 1);
    const uint32_t px = min((uint32_t) ux, (uint32_t) (t.w - 2)), py = min((uint32_t) uy, (uint32_t) (t.h - 2));
    const float w1x = ux - (float) px, w1y = uy - (float) py, w0x = 1.0f - w1x, w0y = 1.0f - w1y;
    texel = px + py * (uint32_t) t.w; w1.x = w1x; w1.y = w1y;
    const float *v00 = t.data + 3u * (size_t) (px + py * (uint32_t) t.w), *v01 = v00 + 3u * (size_t) t.w;
#pragma unroll
    for (int k = 0; k < kWav; ++k) {
        const float l = wav.v[k];
        const float c00 = srgb_model_eval(v00[0], v00[1], v00[2], l), c10 = srgb_model_eval(v00[3], v00[4], v00[5], l);
        const float c01 = srgb_model_eval(v01[0], v01[1], v01[2], l), c11 = srgb_model_eval(v01[3], v01[4], v01[5], l);
        const float c0 = fmaf(w0x, c00, w1x * c10), c1 = fmaf(w0x, c01, w1x * c11);
        r.v[k] = fmaf(w0y, c0, w1y * c1);
    }
    return r;
}
// TAB: a tabulated / analytic radiance (DevEmitter::spectrum) is the radiance itself, not a factor of D65
template <bool TAB = false>
MTS_DEV Spec4 emitter_spectrum(const SceneView &sv, const DevEmitter &e, const Spec4 &wav, f2 uv) {
    if (e.pad0 == kEmitterEnvmap) return envmap_lookup_spectral(*sv.envmap, uv.x, uv.y, wav);
    Spec4 r;
    if constexpr (TAB) {
        if (e.spectrum) {
            const SpectrumPool pool = spectrum_pool(sv);
#pragma unroll
            for (int k = 0; k < kWav; ++k) r.v[k] = spectrum_eval(pool, e.spectrum - 1u, wav.v[k]);
            return r;
        }
    }
#pragma unroll
    for (int k = 0; k < kWav; ++k) r.v[k] = table_eval(g_spectral.d65, e.d65_scale, wav.v[k]) * srgb_model_eval(e.c0, e.c1, e.c2, wav.v[k]);
    return r;
}

// What the emitter-sampling block of the spectral step shows a probe: the sample adds ((mis * thr) * bv) * spec per wavelength if it is unoccluded.
struct NeeTermsS {
    const DirectionSample &ds; f3 wi, wo;     // local directions as the BSDF models take them (they mirror a `twosided` record themselves)
    Spec4 bv, spec; float mis;
    float r1, r2; uint32_t kind;              // spec = ((radiance * falloff) * r1) * r2 (r2: several emitters only) of an emitter of this kind (DevEmitter::pad0)
};

// The probe of the spectral step: the hooks of NoProbe (bounce_step) in the same order, on four wavelengths.  NoProbeS, the probe of
// every spectral render kernel, sees nothing: the step spells out a hook and what it builds for it only for another probe (kWatch
// there), because even the unused per-wavelength copies changed the machine code of the render kernels (scripts/isa_compare.py).
struct NoProbeS {
    template <int DEFER, bool GENERAL, bool NEST> MTS_DEV void begin(const PathStateS &s) { }
    MTS_DEV void emitted(float ew, int32_t emitter, const Spec4 &le) { }
    MTS_DEV void escaped(const SceneView &sv, const PathStateS &s, const DevEmitter &e, float ew, const Spec4 &le) { }
    // thr before the division by q = 1 / rq, hm = hmax(thr); `free`: q was not clamped to .95
    MTS_DEV void roulette(const Spec4 &thr, float hm, float rq, bool free) { }
    // the reflectance spectrum `refl` of the record was evaluated (texel, tw1: footprint of a bitmap lookup, whose four corner
    // coefficient triples the probe re-reads from sv.textures[bsdf.texture]); thr after roulette
    MTS_DEV void surface(const SurfaceInteraction &si, const DevBsdf &bsdf, const Spec4 &refl, uint32_t texel, f2 tw1, const Spec4 &thr) { }
    MTS_DEV bool emitter_sample(const SceneView &sv, const DevBsdf &bsdf, const Spec4 &refl, const NeeTermsS &t) { return false; }
    MTS_DEV void unoccluded(const SceneView &sv, const SurfaceInteraction &si, const Spec4 &thr, const NeeTermsS &t) { }
    // the general step drew the BSDF sample `bs`; thr before it is multiplied by `weight`
    MTS_DEV void bsdf_sampled(const SceneView &sv, const SurfaceInteraction &si, const DevBsdf &bsdf, const Spec4 &refl, const Spec4 &thr, const BsdfSample &bs,
                              const float (&weight)[kWav]) { }
};

// TAB: the scene binds tabulated / analytic spectra (general step only): the host selects these instantiations per scene
template <bool FLAT, int DEFER = 0, bool GENERAL = false, bool NEST = false, class Probe = NoProbeS, bool TAB = false>
MTS_DEV bool bounce_step_spectral(const RenderParams &P, const LdsView &lds, PathStateS &s, Counters &c, Deferred *df = nullptr, Probe &&probe = Probe{}) {
    static_assert(!TAB || GENERAL, "spectra ride on the general step");
    constexpr bool kWatch = !std::is_same_v<std::remove_reference_t<Probe>, NoProbeS>;
    const SceneView &sv = P.sv;
    if constexpr (kWatch) probe.template begin<DEFER, GENERAL, NEST>(s);
    const Geo<FLAT> geo{ sv, lds };
    Hit hit;
    ++c.closest; ++c.segments;
    bool found;
    if (DEFER) df->pending = false;
    if (DEFER == 1) { hit = df->hit; found = df->found; }
    else found = traverse<FLAT, false>(sv, lds, s.o, s.d, s.mint, s.maxt, hit, c.tri_tests,
                                       FLAT && __ballot(s.depth != 1u) == 0ull);      // camera rays only: cluster culling (as bounce_step)
    if (s.depth == 1u) s.flags = found ? 1u : 0u;

    SurfaceInteraction si;
    if (found) {
        fill_si(geo, s.d, hit.prim, hit.u, hit.v, si);
        int32_t emitter = si.shape_rec.emitter;
        if (emitter >= 0) {
            const DevEmitter e = geo.emitter((uint32_t) emitter);
            float ew = 1.0f;
            if (s.depth > 1u) {
                f3 dd = si.p - s.o;
                float dist = sqrtf(sqnorm(dd));
                dd = div_s(dd, dist);
                const float pe = pdf_emitter_direction(sv.n_emitters, e.area_norm, dd, si.sh.n, dist);
                ew = mis_weight(s.bs_pdf, (GENERAL && (s.flags & kFlagDelta)) ? 0.0f : pe);
            }
            if (si.wi.z > 0.0f) {
                Spec4 le4, tab;
                if constexpr (TAB) tab = emitter_spectrum<true>(sv, e, s.wav, f2{ 0.0f, 0.0f });
#pragma unroll
                for (int k = 0; k < kWav; ++k) {       // SRGBEmitterSpectrum::eval = d65 * srgb_model_eval (srgb_d65.cpp:54-62)
                    float le = table_eval(g_spectral.d65, e.d65_scale, s.wav.v[k]) * srgb_model_eval(e.c0, e.c1, e.c2, s.wav.v[k]);
                    if constexpr (TAB) le = tab.v[k];      // a tabulated radiance, or the same product
                    s.res.v[k] += (ew * s.thr.v[k]) * le;
                    if constexpr (kWatch) le4.v[k] = le;
                }
                if constexpr (kWatch) probe.emitted(ew, emitter, le4);
            }
        }
    }
    if (GENERAL && !found && sv.env_emitter >= 0) {          // si.emitter(scene) of an escaped ray: the environment
        const DevEmitter e = geo.emitter((uint32_t) sv.env_emitter);
        float ew = 1.0f;
        if (s.depth > 1u) ew = mis_weight(s.bs_pdf, (GENERAL && (s.flags & kFlagDelta)) ? 0.0f : pdf_environment(sv, e, s.d));
        f2 uv; uv.x = uv.y = 0.0f;
        if (e.pad0 == kEmitterEnvmap) env_dir_to_uv(mat3_apply(sv.envmap->to_local, s.d), uv.x, uv.y);      // envmap.cpp:135-144
        const Spec4 le = emitter_spectrum<TAB>(sv, e, s.wav, uv);
#pragma unroll
        for (int k = 0; k < kWav; ++k) s.res.v[k] += (ew * s.thr.v[k]) * le.v[k];
        if constexpr (kWatch) probe.escaped(sv, s, e, ew, le);
    }
    bool active = found;

    if ((int32_t) s.depth > P.rr_depth) {
        float hm = fmaxf(fmaxf(s.thr.v[0], s.thr.v[1]), fmaxf(s.thr.v[2], s.thr.v[3]));
        float q = fminf(hm * (s.eta * s.eta), 0.95f);
        if (active) active = pcg_next_f32(s.rng) < q;
        float rq = rcp(q);
        if constexpr (kWatch) probe.roulette(s.thr, hm, rq, hm * (s.eta * s.eta) < 0.95f);
#pragma unroll
        for (int k = 0; k < kWav; ++k) s.thr.v[k] *= rq;
    }
    if (s.depth >= (uint32_t) P.max_depth || !active) return false;

    DevBsdf bsdf = geo.bsdf((uint32_t) si.shape_rec.bsdf);      // blend / mask: overwritten with the child in use (surface_bsdf_*)
    Spec4 refl;
#pragma unroll
    for (int k = 0; k < kWav; ++k)       // srgb.cpp:45-52 / uniform.cpp
        refl.v[k] = (bsdf.flags & kBsdfUniformRefl) ? bsdf.r : srgb_model_eval(bsdf.c0, bsdf.c1, bsdf.c2, s.wav.v[k]);
    uint32_t texel = kNoPrim; f2 tw1; tw1.x = tw1.y = 0.0f;
    if (bsdf.texture >= 0) refl = eval_reflectance_spectral(sv, bsdf, si.uv, s.wav, texel, tw1);
    if constexpr (kWatch) probe.surface(si, bsdf, refl, texel, tw1, s.thr);
    BsdfChannels<kWav> chan;
    if (GENERAL) {
        if constexpr (TAB) chan = spectral_channels_tab(bsdf, s.wav, sv);
        else chan = spectral_channels(bsdf, s.wav);
        if constexpr (TAB) {
            if (bsdf_spectrum(bsdf, kSpecRefl)) {
#pragma unroll
                for (int k = 0; k < kWav; ++k) refl.v[k] = chan.refl[k];
            }
        }
#pragma unroll
        for (int k = 0; k < kWav; ++k) chan.refl[k] = refl.v[k];
    }
    // blend / mask: per-wavelength inputs of a child record (its own constant parameters)
    // a scalar weight in the spectral variant is a constant (a textured one is refused at scene creation)
    const NestInfo ni = nest_info<NEST>(bsdf, refl.v[0], refl.v[1], refl.v[2]);
    const bool smooth = !GENERAL || bsdf_is_smooth(bsdf);
    auto chan_of = [&](const DevBsdf &rec, bool child) {
        if constexpr (TAB) return child ? spectral_channels_tab(rec, s.wav, sv) : chan;
        else return child ? spectral_channels(rec, s.wav) : chan;
    };

    if (smooth) {
        f2 s2; s2.x = pcg_next_f32(s.rng); s2.y = pcg_next_f32(s.rng);
        DirectionSample ds; float r1, r2;
        sample_emitter_direction<FLAT, GENERAL>(geo, si.p, s2, ds, r1, r2);
        if (ds.pdf != 0.0f) {
            const DevEmitter e = geo.emitter(ds.emitter);
            f3 wo = to_local(si.sh, ds.d);
            bool front = si.wi.z > 0.0f && wo.z > 0.0f;
            float bp = front ? kInvPi * wo.z : 0.0f;
            float bvs[kWav];
            if (GENERAL) surface_bsdf_eval_pdf<NEST, kWav>(bsdf, ni, [&](uint32_t i) { return geo.bsdf(i); }, chan_of, si.wi, wo, bvs, bp);
            float mis = (GENERAL && ds.delta) ? 1.0f : mis_weight(ds.pdf, bp);
            Spec4 contrib; bool nz = false;
            Spec4 bv4, spec4;                   // for the probe
            const Spec4 le4 = emitter_spectrum<TAB>(sv, e, s.wav, ds.uv);
#pragma unroll
            for (int k = 0; k < kWav; ++k) {
                float le = (GENERAL && ds.delta) ? le4.v[k] * ds.falloff : le4.v[k];
                float spec = le * r1;
                if (sv.n_emitters > 1) spec *= r2;
                float bv = GENERAL ? bvs[k] : (front ? (refl.v[k] * kInvPi) * wo.z : 0.0f);
                contrib.v[k] = ((mis * s.thr.v[k]) * bv) * spec;
                nz = nz || contrib.v[k] != 0.0f;
                if constexpr (kWatch) { bv4.v[k] = bv; spec4.v[k] = spec; }
            }
            auto nee = [&] { return NeeTermsS{ ds, si.wi, wo, bv4, spec4, mis, r1, r2, e.pad0 }; };
            bool watched = false;
            if constexpr (kWatch) watched = probe.emitter_sample(sv, bsdf, refl, nee());
            if (DEFER) {
                if (nz) {
                    ++c.any;
                    df->pending = true; df->so = si.p; df->sd = ds.d;
                    df->smint = kRayEpsilon * (1.0f + hmax_abs(si.p)); df->smaxt = ds.dist * (1.0f - kShadowEpsilon);
#pragma unroll
                    for (int k = 0; k < kWav; ++k) df->nee[k] = contrib.v[k];
                }
            } else if (nz || watched) {
                Hit sh;
                ++c.any;
                bool occluded = traverse<FLAT, true>(sv, lds, si.p, ds.d, kRayEpsilon * (1.0f + hmax_abs(si.p)),
                                               ds.dist * (1.0f - kShadowEpsilon), sh, c.tri_tests);
                if (!occluded) {
#pragma unroll
                    for (int k = 0; k < kWav; ++k) s.res.v[k] += contrib.v[k];
                    if constexpr (kWatch) probe.unoccluded(sv, si, s.thr, nee());
                }
            }
        }
    }

    const float s1 = pcg_next_f32(s.rng);
    f2 s2; s2.x = pcg_next_f32(s.rng); s2.y = pcg_next_f32(s.rng);
    f3 wo = mk3(0.0f, 0.0f, 0.0f); float pdf = 0.0f; bool ok = false;
    bool nz = false;
    if (GENERAL) {
        BsdfSample bs; float w[kWav];
        surface_bsdf_sample<NEST, kWav>(bsdf, ni, [&](uint32_t i) { return geo.bsdf(i); }, chan_of, si.wi, s1, s2, bs, w);
        wo = bs.wo; pdf = bs.pdf;
        s.eta *= bs.eta;
        s.flags = bs.delta ? (s.flags | kFlagDelta) : (s.flags & ~kFlagDelta);
        if constexpr (kWatch) probe.bsdf_sampled(sv, si, bsdf, refl, s.thr, bs, w);
#pragma unroll
        for (int k = 0; k < kWav; ++k) { s.thr.v[k] = s.thr.v[k] * w[k]; nz = nz || s.thr.v[k] != 0.0f; }
    } else {
        if (si.wi.z > 0.0f) {
            wo = square_to_cosine_hemisphere(s2);
            pdf = kInvPi * wo.z;
            ok = pdf > 0.0f;
        }
#pragma unroll
        for (int k = 0; k < kWav; ++k) { s.thr.v[k] = s.thr.v[k] * (ok ? refl.v[k] : 0.0f); nz = nz || s.thr.v[k] != 0.0f; }
    }
    if (!nz) return false;
    s.o = si.p;
    s.d = to_world(si.sh, wo);
    s.mint = (1.0f + hmax_abs(si.p)) * kRayEpsilon;
    s.maxt = __builtin_inff();
    s.bs_pdf = pdf;
    s.depth += 1u;
    if constexpr (MTS_FATED_ELIDE && MTS_FATED_ELIDE_SPECTRAL && !kWatch)      // as bounce_step; shipped off (fated.h)
        if (fated_elide<FLAT>(P, lds, s.o, s.d, s.mint, s.maxt, fmaxf(fmaxf(s.thr.v[0], s.thr.v[1]), fmaxf(s.thr.v[2], s.thr.v[3])), s.eta, s.depth,
                              s.rng.state, c)) return false;
    return true;
}

MTS_DEV void generate_path_spectral(const RenderParams &P, uint64_t ordinal, uint32_t lp, uint32_t j, PathStateS &s, float2 *pos_out = nullptr) {
    const uint32_t w = (uint32_t) P.crop_w;
    const uint32_t lr = lp / w, px = lp - lr * w;
    const uint32_t py = (uint32_t) row_to_global(P.rows, (int32_t) lr);
    const uint64_t index = ((uint64_t) py * w + px) * (uint64_t) P.spp + j;
    seed_sample(s.rng, index, P.base_seed);
    float jx = pcg_next_f32(s.rng), jy = pcg_next_f32(s.rng);
    float psx = ((float) px + (float) P.crop_x) + jx, psy = ((float) py + (float) P.crop_y) + jy;
    f2 ap; ap.x = ap.y = 0.5f;
    if (P.cam.aperture_radius > 0.0f) { ap.x = pcg_next_f32(s.rng); ap.y = pcg_next_f32(s.rng); }
    s.xi = pcg_next_f32(s.rng);                                // integrator.cpp:237, perspective.cpp:196: sample_wavelength(sample)
    wavelengths_from_sample(s.xi, s.wav);
    float ax = (psx - (float) P.crop_x) / (float) P.crop_w, ay = (psy - (float) P.crop_y) / (float) P.crop_h;
    camera_ray(P.cam, ax, ay, ap, s.o, s.d, s.mint, s.maxt);
#pragma unroll
    for (int k = 0; k < kWav; ++k) { s.thr.v[k] = 1.0f; s.res.v[k] = 0.0f; }
    s.bs_pdf = 0.0f; s.eta = 1.0f;
    s.ordinal = P.plane_pixels ? j * P.plane_pixels + (lp - P.plane_pix0) : (uint32_t) (ordinal - P.first_ordinal);
    s.depth = 1u; s.flags = 0u;
    if (P.out_pos) P.out_pos[s.ordinal] = make_float2(psx, psy);
    if (pos_out) *pos_out = make_float2(psx, psy);
}

MTS_DEV void store_result_spectral(const RenderParams &P, const PathStateS &s) {
    float alpha = (s.flags & 1u) ? 1.0f : 0.0f;
    Spec4 v;
#pragma unroll
    for (int k = 0; k < kWav; ++k) v.v[k] = wavelength_weight(s.wav.v[k]) * s.res.v[k];    // ray_weight * L (integrator.cpp:250)
    f3 xyz = spectrum_to_xyz(v, s.wav);                                                       // integrator.cpp:259-261
    bool valid = (xyz.x >= -1e-5f) && (xyz.y >= -1e-5f) && (xyz.z >= -1e-5f) && isfinite(xyz.x) && isfinite(xyz.y) && isfinite(xyz.z);
    P.out_rgba[s.ordinal] = make_float4(xyz.x, xyz.y, xyz.z, (valid || !P.store_xyz) ? alpha : -1.0f);
}

// (k_bounce_spectra below repeats this round for scenes with tabulated spectra: a change here is made there too)
template <bool FLAT, bool GENERAL, bool NEST = false>
__global__ __launch_bounds__(kBlock) void k_bounce_spectral(const RenderParams P) {
    extern __shared__ float4 smem[];
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6;
    if (wave >= P.n_waves) return;
    const uint32_t lane = lane_id();
    const uint32_t n_in = __builtin_amdgcn_readfirstlane(P.count_in[wave]);
    const size_t base = (size_t) wave * P.seg_cap;
    uint32_t n_out = 0;
    Counters c = { 0u, 0u, 0u, 0u };
    for (uint32_t i0 = 0; i0 < n_in; i0 += 64u) {
        PathStateS s;
        bool alive = false;
        if (i0 + lane < n_in) {
            load_state(P.in, base + i0 + lane, s);
            alive = bounce_step_spectral<FLAT, 0, GENERAL, NEST>(P, lds, s, c);
            if (!alive) store_result_spectral(P, s);
        }
        const uint64_t m = __ballot(alive);
        if (alive) store_state(P.out, base + n_out + mask_rank(m), s);
        n_out += (uint32_t) __popcll(m);
    }
    uint64_t cursor = P.cursor[wave];
    const uint64_t end = P.cursor_end[wave];
    while (n_out < P.target && cursor < end) {
        uint64_t left = end - cursor;
        uint32_t n_new = min(64u, P.target - n_out);
        if ((uint64_t) n_new > left) n_new = (uint32_t) left;
        if (lane < n_new) {
            PathStateS s;
            uint64_t ordinal; uint32_t lp, sj;
            cursor_sample(P, wave, cursor + lane, ordinal, lp, sj);
            generate_path_spectral(P, ordinal, lp, sj, s);
            store_state(P.out, base + n_out + lane, s);
        }
        n_out += n_new; cursor += n_new;
    }
    uint32_t tot[4] = { c.closest, c.any, c.segments, c.tri_tests };
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int off = 32; off > 0; off >>= 1) tot[k] += __shfl_xor(tot[k], off);
    if (lane == 0) {
        P.count_out[wave] = n_out;
        P.cursor[wave] = cursor;
        uint64_t *ws = P.wave_stats + 4u * (size_t) wave;
        ws[0] += tot[0]; ws[1] += tot[1]; ws[2] += tot[2]; ws[3] += tot[3];
    }
}
// The same round for a scene that binds tabulated / analytic spectra: the general step with the spectrum pool.  A copy, because the
// round shared through an inlined function assembled k_bounce_spectral differently (scripts/isa_compare.py).
template <bool FLAT, bool NEST>
__global__ __launch_bounds__(kBlock) void k_bounce_spectra(const RenderParams P) {
    extern __shared__ float4 smem[];
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6;
    if (wave >= P.n_waves) return;
    const uint32_t lane = lane_id();
    const uint32_t n_in = __builtin_amdgcn_readfirstlane(P.count_in[wave]);
    const size_t base = (size_t) wave * P.seg_cap;
    uint32_t n_out = 0;
    Counters c = { 0u, 0u, 0u, 0u };
    for (uint32_t i0 = 0; i0 < n_in; i0 += 64u) {
        PathStateS s;
        bool alive = false;
        if (i0 + lane < n_in) {
            load_state(P.in, base + i0 + lane, s);
            alive = bounce_step_spectral<FLAT, 0, true, NEST, NoProbeS, true>(P, lds, s, c);
            if (!alive) store_result_spectral(P, s);
        }
        const uint64_t m = __ballot(alive);
        if (alive) store_state(P.out, base + n_out + mask_rank(m), s);
        n_out += (uint32_t) __popcll(m);
    }
    uint64_t cursor = P.cursor[wave];
    const uint64_t end = P.cursor_end[wave];
    while (n_out < P.target && cursor < end) {
        uint64_t left = end - cursor;
        uint32_t n_new = min(64u, P.target - n_out);
        if ((uint64_t) n_new > left) n_new = (uint32_t) left;
        if (lane < n_new) {
            PathStateS s;
            uint64_t ordinal; uint32_t lp, sj;
            cursor_sample(P, wave, cursor + lane, ordinal, lp, sj);
            generate_path_spectral(P, ordinal, lp, sj, s);
            store_state(P.out, base + n_out + lane, s);
        }
        n_out += n_new; cursor += n_new;
    }
    uint32_t tot[4] = { c.closest, c.any, c.segments, c.tri_tests };
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int off = 32; off > 0; off >>= 1) tot[k] += __shfl_xor(tot[k], off);
    if (lane == 0) {
        P.count_out[wave] = n_out;
        P.cursor[wave] = cursor;
        uint64_t *ws = P.wave_stats + 4u * (size_t) wave;
        ws[0] += tot[0]; ws[1] += tot[1]; ws[2] += tot[2]; ws[3] += tot[3];
    }
}

// ---------------------------------------------------------------------------------------------
// `direct` (src/integrators/direct.cpp:105-196) and `depth` (depth.cpp:19-33): no path state survives a sample, so one
// thread carries a camera sample from the sensor to its result.
template <bool FLAT, bool GENERAL, bool NEST = false>
__global__ __launch_bounds__(kBlock) void k_direct(const RenderParams P, uint64_t n) {
    extern __shared__ float4 smem[];
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    const uint64_t gid = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    Counters c = { 0u, 0u, 0u, 0u };
    if (gid < n) {
        const SceneView &sv = P.sv;
        const Geo<FLAT> geo{ sv, lds };
        const uint64_t ordinal = P.first_ordinal + gid;
        const uint32_t lp = (uint32_t) (ordinal / (uint64_t) P.spp), j = (uint32_t) (ordinal - (uint64_t) lp * (uint64_t) P.spp);
        PathState s;
        generate_path(P, ordinal, lp, j, s);
        Hit hit;
        ++c.closest; ++c.segments;
        const bool found = traverse<FLAT, false>(sv, lds, s.o, s.d, s.mint, s.maxt, hit, c.tri_tests, FLAT);      // camera rays of consecutive samples: cluster culling
        s.flags = found ? 1u : 0u;
        if (P.integrator == 2) {
            const float t = found ? hit.t : 0.0f;
            s.res = mk3(t, t, t);
        } else if (!found) {
            if (GENERAL && !P.hide_emitters && sv.env_emitter >= 0) {
                const DevEmitter e = geo.emitter((uint32_t) sv.env_emitter);
                const f3 le = environment_radiance(sv, e, s.d);
                s.res = mk3(s.res.x + le.x, s.res.y + le.y, s.res.z + le.z);
            }
        } else {
            int32_t ne = P.emitter_samples, nb = P.bsdf_samples;
            if (ne == 0 && nb == 0) ne = nb = 1;
            const float sum = (float) (ne + nb);
            const float weight_bsdf = 1.0f / (float) nb, weight_lum = 1.0f / (float) ne;
            const float frac_bsdf = (float) nb / sum, frac_lum = (float) ne / sum;
            SurfaceInteraction si;
            fill_si(geo, s.d, hit.prim, hit.u, hit.v, si);
            if (!P.hide_emitters && si.shape_rec.emitter >= 0 && si.wi.z > 0.0f) {
                const DevEmitter e = geo.emitter((uint32_t) si.shape_rec.emitter);
                s.res = mk3(s.res.x + e.r, s.res.y + e.g, s.res.z + e.b);
            }
            DevBsdf bsdf = geo.bsdf((uint32_t) si.shape_rec.bsdf);      // blend / mask: overwritten with the child in use (surface_bsdf_*)
            if (NEST) resolve_textured(sv, bsdf, si.uv);
            uint32_t texel; f2 tw1;
            const f3 refl = eval_reflectance(sv, bsdf, si.uv, texel, tw1);
            const NestInfo ni = nest_info<NEST>(bsdf, refl.x, refl.y, refl.z);
            auto child_refl = [&](const DevBsdf &rec) { uint32_t t; f2 w; return eval_reflectance(sv, rec, si.uv, t, w); };
            if (!GENERAL || bsdf_is_smooth(bsdf)) {
                for (int32_t i = 0; i < ne; ++i) {
                    f2 s2; s2.x = pcg_next_f32(s.rng); s2.y = pcg_next_f32(s.rng);
                    DirectionSample ds; f3 spec;
                    sample_emitter_direction<FLAT, GENERAL>(geo, si.p, s2, ds, spec);
                    if (ds.pdf == 0.0f) continue;
                    const f3 wo = to_local(si.sh, ds.d);
                    f3 bv; float bp;
                    if (GENERAL) surface_bsdf_eval_pdf<NEST>(bsdf, ni, refl, BsdfTable<NEST, FLAT>(geo, si.uv), child_refl, si.wi, wo, bv, bp);
                    else diffuse_eval_pdf(refl, si.wi, wo, bv, bp);
                    const float mis = (GENERAL && ds.delta) ? 1.0f : mis_weight(ds.pdf * frac_lum, bp * frac_bsdf) * weight_lum;      // direct.cpp:155-156
                    const f3 contrib = mk3((mis * bv.x) * spec.x, (mis * bv.y) * spec.y, (mis * bv.z) * spec.z);
                    if (contrib.x != 0.0f || contrib.y != 0.0f || contrib.z != 0.0f) {
                        Hit sh;
                        ++c.any;
                        if (!traverse<FLAT, true>(sv, lds, si.p, ds.d, kRayEpsilon * (1.0f + hmax_abs(si.p)),
                                                  ds.dist * (1.0f - kShadowEpsilon), sh, c.tri_tests))
                            s.res = s.res + contrib;
                    }
                }
            }
            for (int32_t i = 0; i < nb; ++i) {
                const float s1 = pcg_next_f32(s.rng);
                f2 s2; s2.x = pcg_next_f32(s.rng); s2.y = pcg_next_f32(s.rng);
                f3 wo, weight; float pdf; bool delta = false;
                if (GENERAL) {
                    BsdfSample bs;
                    surface_bsdf_sample<NEST>(bsdf, ni, refl, BsdfTable<NEST, FLAT>(geo, si.uv), child_refl, si.wi, s1, s2, bs, weight);
                    wo = bs.wo; pdf = bs.pdf; delta = bs.delta;
                } else {
                    diffuse_sample(refl, si.wi, s2, wo, pdf, weight);
                }
                if (!(weight.x != 0.0f || weight.y != 0.0f || weight.z != 0.0f)) continue;
                Hit h2;
                ++c.closest; ++c.segments;
                const f3 d2 = to_world(si.sh, wo);
                f3 le; float pe;
                if (!traverse<FLAT, false>(sv, lds, si.p, d2, (1.0f + hmax_abs(si.p)) * kRayEpsilon, __builtin_inff(), h2, c.tri_tests)) {
                    if (!GENERAL || sv.env_emitter < 0) continue;
                    const DevEmitter e = geo.emitter((uint32_t) sv.env_emitter);
                    le = environment_radiance(sv, e, d2);
                    pe = delta ? 0.0f : pdf_environment(sv, e, d2);
                } else {
                    SurfaceInteraction si2;
                    fill_si(geo, d2, h2.prim, h2.u, h2.v, si2);
                    if (si2.shape_rec.emitter < 0) continue;
                    const DevEmitter e = geo.emitter((uint32_t) si2.shape_rec.emitter);
                    le = si2.wi.z > 0.0f ? mk3(e.r, e.g, e.b) : mk3(0.0f, 0.0f, 0.0f);
                    f3 dd = si2.p - si.p;
                    const float dist = sqrtf(sqnorm(dd));
                    dd = div_s(dd, dist);
                    pe = delta ? 0.0f : pdf_emitter_direction(sv.n_emitters, e.area_norm, dd, si2.sh.n, dist);
                }
                const float w = mis_weight(pdf * frac_bsdf, pe * frac_lum) * weight_bsdf;
                s.res = mk3(s.res.x + (weight.x * le.x) * w, s.res.y + (weight.y * le.y) * w, s.res.z + (weight.z * le.z) * w);
            }
        }
        store_result(P, s);
    }
    uint32_t tot[4] = { c.closest, c.any, c.segments, c.tri_tests };
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int off = 32; off > 0; off >>= 1) tot[k] += __shfl_xor(tot[k], off);
    if (lane_id() == 0) {
        unsigned long long *ws = reinterpret_cast<unsigned long long *>(P.wave_stats + 4u * (size_t) ((gid >> 6) % P.n_waves));
        for (int k = 0; k < 4; ++k) if (tot[k]) atomicAdd(ws + k, (unsigned long long) tot[k]);
    }
}

hipError_t launch_direct(const RenderParams &p, uint64_t n, hipStream_t s) {
    const uint32_t blocks = (uint32_t) ((n + kBlock - 1) / kBlock);
    const size_t lds = bounce_lds_bytes(p.sv);
    if (p.sv.general == 2u) {      // scenes with blendbsdf / mask
        if (p.sv.flat) return launch_lds(k_direct<true, true, true>, dim3(blocks), dim3(kBlock), lds, s, p, n);
        else return launch_lds(k_direct<false, true, true>, dim3(blocks), dim3(kBlock), lds, s, p, n);
    } else if (p.sv.general) {
        if (p.sv.flat) return launch_lds(k_direct<true, true>, dim3(blocks), dim3(kBlock), lds, s, p, n);
        else return launch_lds(k_direct<false, true>, dim3(blocks), dim3(kBlock), lds, s, p, n);
    } else {
        if (p.sv.flat) return launch_lds(k_direct<true, false>, dim3(blocks), dim3(kBlock), lds, s, p, n);
        else return launch_lds(k_direct<false, false>, dim3(blocks), dim3(kBlock), lds, s, p, n);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// `aov` (src/integrators/aov.cpp:166-219): si = scene.ray_intersect(ray) for the camera ray of every sample, zeroed on a miss
// (aov.cpp:171-172), and one film channel per requested field.  The intersection draws no random numbers, so the nested integrator's
// sample -- traced by the render kernels, untouched -- and this one share the ray, the film position and the slot s.ordinal.  One thread
// per camera sample, as k_direct; GENERAL only selects the thin-lens aperture sample.
MTS_DEV float aov_value(const SurfaceInteraction &si, float t, uint32_t source) {
    switch (source) {       // wave-uniform
    case kAovT: return t;
    case kAovP: return si.p.x; case kAovP + 1: return si.p.y; case kAovP + 2: return si.p.z;
    case kAovUV: return si.uv.x; case kAovUV + 1: return si.uv.y;
    case kAovN: return si.n.x; case kAovN + 1: return si.n.y; case kAovN + 2: return si.n.z;
    case kAovShN: return si.sh.n.x; case kAovShN + 1: return si.sh.n.y; case kAovShN + 2: return si.sh.n.z;
    case kAovDpDu: return si.dp_du.x; case kAovDpDu + 1: return si.dp_du.y; case kAovDpDu + 2: return si.dp_du.z;
    case kAovDpDv: return si.dp_dv.x; case kAovDpDv + 1: return si.dp_dv.y; case kAovDpDv + 2: return si.dp_dv.z;
    default: return 0.0f;
    }
}

template <bool FLAT, bool GENERAL>
__global__ __launch_bounds__(kBlock) void k_aov(const AovParams A, uint64_t n) {
    extern __shared__ float4 smem[];
    const RenderParams &P = A.rp;
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    const uint64_t gid = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    Counters c = { 0u, 0u, 0u, 0u };
    if (gid < n) {
        const SceneView &sv = P.sv;
        const Geo<FLAT> geo{ sv, lds };
        const uint64_t ordinal = P.first_ordinal + gid;
        const uint32_t lp = (uint32_t) (ordinal / (uint64_t) P.spp), j = (uint32_t) (ordinal - (uint64_t) lp * (uint64_t) P.spp);
        PathState s;
        generate_path<GENERAL>(P, ordinal, lp, j, s);
        Hit hit;
        ++c.closest;
        const bool found = traverse<FLAT, false>(sv, lds, s.o, s.d, s.mint, s.maxt, hit, c.tri_tests, FLAT);      // camera rays of consecutive samples: cluster culling
        SurfaceInteraction si;
        if (found) fill_si(geo, s.d, hit.prim, hit.u, hit.v, si);
        const float t = found ? hit.t : 0.0f;
        // a group is flagged when one of its own channels is not finite; k_aov_finish extends the flag to every stream of the sample
        // (ImageBlock::put drops the whole sample, imageblock.cpp:85-109, warn_negative = false)
        float4 *out = A.groups + s.ordinal;
        for (uint32_t ch = 0; ch < A.n_channels; ch += 3u, out += A.group_stride) {
            float v[3];
#pragma unroll
            for (uint32_t k = 0; k < 3u; ++k) v[k] = (found && ch + k < A.n_channels) ? aov_value(si, t, A.source[ch + k]) : 0.0f;
            const bool finite = isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]);
            *out = make_float4(v[0], v[1], v[2], finite ? 0.0f : -1.0f);
        }
    }
    uint32_t tot[4] = { c.closest, c.any, c.segments, c.tri_tests };
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int off = 32; off > 0; off >>= 1) tot[k] += __shfl_xor(tot[k], off);
    if (lane_id() == 0) {
        unsigned long long *ws = reinterpret_cast<unsigned long long *>(P.wave_stats + 4u * (size_t) ((gid >> 6) % P.n_waves));
        for (int k = 0; k < 4; ++k) if (tot[k]) atomicAdd(ws + k, (unsigned long long) tot[k]);
    }
}

hipError_t launch_aov(const AovParams &a, uint64_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t) ((n + kBlock - 1) / kBlock);
    const size_t lds = bounce_lds_bytes(a.rp.sv);          // hierarchy scenes: the whole traversal stack of the 256 lanes, as k_direct
    const bool lens = a.rp.cam.aperture_radius > 0.0f;
    const void *fn = a.rp.sv.flat ? (lens ? (const void *) &k_aov<true, true> : (const void *) &k_aov<true, false>)
                                  : (lens ? (const void *) &k_aov<false, true> : (const void *) &k_aov<false, false>);
    if (hipError_t e = allow_lds(fn, lds)) return e;       // deep hierarchies ask for more than 48 KiB
    if (a.rp.sv.flat) {
        if (lens) hipLaunchKernelGGL((k_aov<true, true>), dim3(blocks), dim3(kBlock), lds, s, a, n);
        else hipLaunchKernelGGL((k_aov<true, false>), dim3(blocks), dim3(kBlock), lds, s, a, n);
    } else {
        if (lens) hipLaunchKernelGGL((k_aov<false, true>), dim3(blocks), dim3(kBlock), lds, s, a, n);
        else hipLaunchKernelGGL((k_aov<false, false>), dim3(blocks), dim3(kBlock), lds, s, a, n);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Split pipeline for hierarchy scenes.  In the fused kernel the BVH walks inherit the shading code's ~100 VGPRs
// (4 waves / SIMD) and are latency-bound at that occupancy: 1.5 Gray/s on a 261 k-triangle mesh against ~5 Gray/s
// for a kernel that only traverses.  So here every iteration runs k_trace<false> (closest hits of the in-flight
// rays -> `hit`), k_shade (the path.cpp iteration on the precomputed hits; shadow rays are written next to the
// state) and k_trace<true> (visibility; adds the guarded contribution to the path's radiance).  The order of the
// floating-point additions into the radiance is the fused kernel's, so both pipelines produce identical samples.
constexpr uint32_t kFlagZombie = 2u;      // path already terminated, kept one iteration for its pending shadow ray

template <bool GENERAL, bool FLAT>
MTS_DEV bool step_deferred(const RenderParams &P, const LdsView &lds, PathState &s, Counters &c, Deferred &df) {
    return bounce_step<FLAT, FLAT ? 2 : 1, GENERAL>(P, lds, s, c, NoProbe{}, &df);
}
template <bool GENERAL, bool FLAT>
MTS_DEV bool step_deferred(const RenderParams &P, const LdsView &lds, PathStateS &s, Counters &c, Deferred &df) {
    return bounce_step_spectral<FLAT, FLAT ? 2 : 1, GENERAL>(P, lds, s, c, &df);
}
template <bool GENERAL, bool FLAT>
MTS_DEV bool step_deferred(const RenderParams &P, const LdsView &lds, PathStateT &s, Counters &c, Deferred &df) {
    return bounce_step_spectral<FLAT, FLAT ? 2 : 1, GENERAL, false, NoProbeS, true>(P, lds, s, c, &df);
}
// radiance += nee of an unoccluded shadow ray: the additions drain_shadow_ring / k_trace<any> make on the stored record
MTS_DEV void add_nee(PathState &s, const float (&nee)[4]) { s.res = mk3(s.res.x + nee[0], s.res.y + nee[1], s.res.z + nee[2]); }
MTS_DEV void add_nee(PathStateS &s, const float (&nee)[4]) {
#pragma unroll
    for (int k = 0; k < kWav; ++k) s.res.v[k] += nee[k];
}
MTS_DEV void finish_path(const RenderParams &P, const PathState &s) { store_result(P, s); }
MTS_DEV void finish_path(const RenderParams &P, const PathStateS &s) { store_result_spectral(P, s); }
MTS_DEV void start_path(const RenderParams &P, uint64_t ordinal, uint32_t lp, uint32_t j, PathState &s) { generate_path(P, ordinal, lp, j, s); }
MTS_DEV void start_path(const RenderParams &P, uint64_t ordinal, uint32_t lp, uint32_t j, PathStateS &s) { generate_path_spectral(P, ordinal, lp, j, s); }

// FLAT = false: hierarchy scene, closest hits precomputed by k_trace<false>; FLAT = true: LDS-resident scene, closest hit
// inline (wave-uniform primitive loop), only the shadow rays are queued
// Register budget of k_shade on hierarchy scenes (waves per SIMD the compiler must reach): the kernel streams the path state through
// HBM and gathers vertex data, so it lives on waves in flight.  5 waves (96 VGPRs) fit the RGB diffuse-only variant without spilling
// (+1.5 %); the others get 4 waves (128 VGPRs; the compiler's own choice was 136-185 VGPRs = 2-3 waves): spectral diffuse +2 %,
// general BSDFs +5 % (RGB) / +10 % (spectral, 128 bytes of scratch per lane) on the 261 k-triangle scenes.
#ifndef MTS_SHADE_WAVES_MIN
#define MTS_SHADE_WAVES_MIN 4
#endif
#ifndef MTS_SHADE_WAVES_MIN_RGB_DIFFUSE
#define MTS_SHADE_WAVES_MIN_RGB_DIFFUSE 5
#endif
template <typename State, bool GENERAL> struct ShadeWaves { static constexpr int kMin = MTS_SHADE_WAVES_MIN; };
template <> struct ShadeWaves<PathState, false> { static constexpr int kMin = MTS_SHADE_WAVES_MIN_RGB_DIFFUSE; };
// INLINE (flat scenes only): the shadow rays of consecutive 64-path chunks are collected in a per-wave LDS ring and resolved
// 64 at a time inside this kernel -- the any-hit loop then always runs on full waves (only about two thirds of the paths cast
// a shadow ray) -- and `nee` is added to the radiance the wave has already stored in its output segment.
// The ring of one wave (kernels.h, shadow_ring_bytes): rows o[kShadowRing], d[kShadowRing], nee[kShadowRing] (+ slot[kShadowRing]).
template <typename State> struct ShadowRing {
    static constexpr bool kSlotInNee = false;               // spectral: nee.w is the fourth wavelength
    static constexpr uint32_t kFloat4 = kShadowRing * 13u / 4u;
    float4 *o, *d, *nee; uint32_t *slot;
};
template <> struct ShadowRing<PathState> {
    static constexpr bool kSlotInNee = true;                // RGB: nee.w is 0, the slot index takes its place
    static constexpr uint32_t kFloat4 = kShadowRing * 3u;
    float4 *o, *d, *nee; uint32_t *slot;
};
static_assert(ShadowRing<PathState>::kFloat4 * 16u == 48u * kShadowRing && ShadowRing<PathStateS>::kFloat4 * 16u == 52u * kShadowRing,
              "ring sizes of shadow_ring_bytes()");
// RGB ring: a path that dies with its shadow ray pending is not kept a launch as a zombie.  Its entry carries the sample's ordinal and
// kRingFinal in the slot word (slots and ordinals of a pass stay below 2^31: cursor_sample), and the drain finishes the path.
constexpr uint32_t kRingFinal = 0x80000000u;
template <typename State> constexpr bool kRingFinishes = MTS_FATED_ELIDE != 0 && ShadowRing<State>::kSlotInNee;
// The drain's half: an entry with kRingFinal ends its path here (true).  The slot word holds the sample's ordinal, whose place in the
// sample stream holds (res.xyz, valid_ray) meanwhile (k_shade); res + nee as for a stored path, then store_result as for any other.
MTS_DEV bool finish_ring_entry(const RenderParams &P, const float4 &e, bool occluded) {
    const uint32_t w = __float_as_uint(e.w);
    if (!(w & kRingFinal)) return false;
    PathState t;
    t.ordinal = w & ~kRingFinal;
    const float4 r = P.out_rgba[t.ordinal];
    t.res = occluded ? mk3(r.x, r.y, r.z) : mk3(r.x + e.x, r.y + e.y, r.z + e.z);
    t.flags = r.w != 0.0f ? 1u : 0u;
    store_result(P, t);
    return true;
}

template <typename State, bool GENERAL>
MTS_DEV void drain_shadow_ring(const RenderParams &P, const LdsView &lds, const ShadowRing<State> &q, uint32_t head, uint32_t count,
                               size_t base, Counters &c) {
    // the wave's earlier stores to its output segment must have reached L2 before other lanes read-modify-write them
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    const uint32_t lane = lane_id();
    if (lane < count) {
        const uint32_t k = (head + lane) & (kShadowRing - 1u);
        const float4 o = q.o[k], d = q.d[k];
        Hit h;
        const bool occluded = traverse<true, true>(P.sv, lds, mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z), o.w, d.w, h, c.tri_tests);
        bool finished = false;
        if constexpr (kRingFinishes<State>) finished = finish_ring_entry(P, q.nee[k], occluded);
        if (!finished && !occluded) {
            const float4 e = q.nee[k];
            const size_t slot = base + (ShadowRing<State>::kSlotInNee ? __float_as_uint(e.w) : q.slot[k]);
            float4 r = P.out.res[slot];
            r.x += e.x; r.y += e.y; r.z += e.z;
            if (!ShadowRing<State>::kSlotInNee) r.w += e.w;      // RGB: w = eta, nee adds nothing to it
            P.out.res[slot] = r;
        }
    }
}

// Non-temporal pool / ray / hit / shadow-queue streams on hierarchy scenes: bit 0 = k_trace, bit 1 = k_shade
#ifndef MTS_NT_STREAMS
#define MTS_NT_STREAMS 3
#endif
#ifndef MTS_PRIMARY_SHADOW
#define MTS_PRIMARY_SHADOW 1  // 0 (experiment): the shadow rays of camera-path chunks go through the ring like all others
#endif
#ifndef MTS_SURV_ORDER
#define MTS_SURV_ORDER 1      // 0 (experiment): the pooled list of a workgroup in segment order, survivors and camera paths interleaved
#endif
template <typename State, bool GENERAL, bool FLAT, bool INLINE = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(FLAT ? MTS_BOUNCE_WAVES : ShadeWaves<State, GENERAL>::kMin, FLAT ? MTS_BOUNCE_WAVES : 8)))
void k_shade(const RenderParams P) {
    static_assert(FLAT || !INLINE, "the in-kernel shadow queue is for LDS-resident scenes");
    constexpr bool kNT = !FLAT && (MTS_NT_STREAMS & 2) != 0;      // hierarchy scenes: the pool streams bypass the caches the BVH lives in
    extern __shared__ float4 smem[];
    LdsView lds = {};                      // Geo<false> reads the scene tables from global memory
    // a launch covers the scheduling waves [wave_first, wave_last) (all of them, or one half when two launches share the GPU).
    // Pool drain (FLAT, gather_w > 4): once the sample cursors are dry the host lets one workgroup take the paths of gather_w
    // consecutive scheduling waves and leave the survivors at the front of the group -- hardware wave h fills the segments of the
    // waves h, h + 4, h + 8, ... of the group one after the other: the pool is compacted as it is advanced, and the number of
    // workgroups that stage the scene for a handful of paths shrinks with it.
    const uint32_t gw = (INLINE && P.gather_w > 4u) ? P.gather_w : 4u;      // only the shadow-ring schedule gathers (api.cpp)
    const uint32_t hw = threadIdx.x >> 6;
    const uint32_t wave = gw > 4u ? P.wave_first + blockIdx.x * gw + hw : P.wave_first + ((blockIdx.x * kBlock + threadIdx.x) >> 6);
    const uint32_t wave_last = P.wave_last ? P.wave_last : P.n_waves;
    __shared__ uint32_t s_cnt[kBlock / 64u], s_surv[kBlock / 64u];
    // gather: s_pre[k] = paths in the group's waves before the k-th, in dynamic LDS after the shadow rings (launch_bounce adds
    // gather_w + 1 words to those launches only: the steady-state launches do not reserve it)
    uint32_t *const s_pre = reinterpret_cast<uint32_t *>(smem + P.lds_queue_offset + kShadeWaves * ShadowRing<State>::kFloat4);
    if (FLAT && gw > 4u) {
        const uint32_t g0 = wave - hw;
        for (uint32_t k = threadIdx.x; k < gw; k += kBlock) s_pre[k + 1u] = (g0 + k < wave_last) ? P.count_in[g0 + k] : 0u;
        if (threadIdx.x == 0u) s_pre[0] = 0u;
        __syncthreads();
        if (hw == 0u) {                      // inclusive prefix sums by one wave: a run of `per` entries per lane + a wave scan
            const uint32_t per = (gw + 63u) / 64u, ln = lane_id();
            uint32_t local = 0u;
            for (uint32_t i = 0; i < per; ++i) { const uint32_t idx = ln * per + i; if (idx < gw) local += s_pre[idx + 1u]; }
            uint32_t incl = local;
            for (uint32_t off = 1u; off < 64u; off <<= 1) { const uint32_t v = __shfl_up(incl, off); if (ln >= off) incl += v; }
            uint32_t run = incl - local;
            for (uint32_t i = 0; i < per; ++i) { const uint32_t idx = ln * per + i; if (idx < gw) { run += s_pre[idx + 1u]; s_pre[idx + 1u] = run; } }
        }
        __syncthreads();
        if (s_pre[gw] == 0u) {               // nothing left in the whole group
            for (uint32_t k = threadIdx.x; k < gw; k += kBlock) if (g0 + k < wave_last) P.count_out[g0 + k] = 0u;
            return;
        }
        lds = lds_stage<true>(P.sv, smem);
    } else if (FLAT) {
        // While the pool drains at the end of a pass most scheduling waves have nothing left to do: a workgroup whose four
        // waves are all idle leaves before staging the scene into LDS (its output counts still have to be reset).
        const uint32_t n_own = wave < wave_last ? P.count_in[wave] : 0u;
        // the segment of a wave is [survivors of the last launch | camera paths generated by it]; the second half of the count array says
        // where the border is (a hint: any value <= the count gives a valid order, so stale entries of other schedules are harmless)
        if (lane_id() == 0u) { s_cnt[threadIdx.x >> 6] = n_own; s_surv[threadIdx.x >> 6] = (wave < wave_last && MTS_SURV_ORDER) ? min(P.count_in[P.n_waves + wave], n_own) : 0u; }
        const bool work = wave < wave_last && (n_own > 0u || P.cursor[wave] < P.cursor_end[wave]);
        if (!__syncthreads_or(work ? 1 : 0)) {
            if (wave < wave_last && lane_id() == 0u) {
                P.count_out[wave] = 0u;
                if (!INLINE) P.count_shadow[wave] = 0u;
            }
            return;
        }
        lds = lds_stage<true>(P.sv, smem);
    }
    ShadowRing<State> ring = {};
    if (INLINE) {
        float4 *qb = smem + P.lds_queue_offset + (size_t) (threadIdx.x >> 6) * ShadowRing<State>::kFloat4;
        ring.o = qb; ring.d = qb + kShadowRing; ring.nee = qb + 2u * kShadowRing;
        ring.slot = ShadowRing<State>::kSlotInNee ? nullptr : reinterpret_cast<uint32_t *>(qb + 3u * kShadowRing);
    }
    if (wave >= wave_last) return;
    const uint32_t lane = lane_id();
    const size_t base = (size_t) wave * P.seg_cap;
    uint32_t n_out = 0;
    Counters c = { 0u, 0u, 0u, 0u };
    uint32_t n_sh = 0;
    uint32_t q_head = 0, q_count = 0;
    // FLAT: the input segments of the workgroup's scheduling waves form one list whose 64-path chunks are dealt round-robin to
    // the waves -- at most one partial chunk per workgroup instead of one per wave while the pool drains.  Survivors go to the
    // output segment of the wave that processed them (seg_cap is a multiple of 64, so a wave never gets more than it can hold).
    const uint32_t wg_wave0 = wave - (threadIdx.x >> 6);
    const uint32_t n_valid = FLAT ? min((uint32_t) (kBlock / 64u), wave_last - wg_wave0) : 1u;
    // FLAT: the pooled list is ordered [survivors of wave 0 .. 3 | new camera paths of wave 0 .. 3] (reg[0 .. 7]): the chunks of the second
    // part hold camera rays only -- the samples of one or two pixels -- and take the cluster-culling closest-hit loop (traverse())
    uint32_t reg[2u * (kBlock / 64u)], surv4[kBlock / 64u], n_in = 0;
    if (FLAT && gw > 4u) {
        n_in = s_pre[gw];
    } else if (FLAT) {
#pragma unroll
        for (uint32_t g = 0; g < kBlock / 64u; ++g) {
            const uint32_t cg = g < n_valid ? s_cnt[g] : 0u;
            surv4[g] = g < n_valid ? s_surv[g] : 0u;
            reg[g] = surv4[g]; reg[kBlock / 64u + g] = cg - surv4[g];
            n_in += cg;
        }
    } else {
        n_in = __builtin_amdgcn_readfirstlane(P.count_in[wave]);
    }

    for (uint32_t i0 = FLAT ? 64u * (threadIdx.x >> 6) : 0u; i0 < n_in; i0 += 64u * n_valid) {
        State s;
        Deferred df;
        df.pending = false;
        bool alive = false, zombie_now = false;
        uint32_t depth0 = 0u;                                // depth of the path before this step (0: no path, or a zombie)
        if (i0 + lane < n_in) {
            size_t i = base + i0 + lane;
            if (FLAT && gw > 4u) {          // s_pre[k] <= index < s_pre[k + 1]: the k-th wave of the group holds the path
                const uint32_t idx = i0 + lane;
                uint32_t k = 0u;
                for (uint32_t step = gw >> 1; step; step >>= 1) if (s_pre[k + step] <= idx) k += step;
                i = (size_t) (wg_wave0 + k) * P.seg_cap + (idx - s_pre[k]);
            } else if (FLAT) {
                uint32_t r = 0u, j = i0 + lane;
#pragma unroll
                for (uint32_t g = 0; g + 1 < 2u * (kBlock / 64u); ++g)
                    if (r == g && j >= reg[g]) { j -= reg[g]; ++r; }
                constexpr uint32_t kW = kBlock / 64u;
                const uint32_t g = r >= kW ? r - kW : r;
                uint32_t off = 0u;
#pragma unroll
                for (uint32_t q = 0; q < kW; ++q) off = (r >= kW && g == q) ? surv4[q] : off;
                i = (size_t) (wg_wave0 + g) * P.seg_cap + off + j;
            }
            load_state<kNT>(P.in, i, s);
            if (s.flags & kFlagZombie) {
                finish_path(P, s);
            } else {
                depth0 = s.depth;
                if (!FLAT) {
                    const float4 h = ld_stream<kNT>(P.in.hit + i);
                    df.hit.t = h.x; df.hit.prim = __float_as_uint(h.y); df.hit.u = h.z; df.hit.v = h.w;
                    df.found = df.hit.prim != kNoPrim;
                }
                alive = step_deferred<GENERAL, FLAT>(P, lds, s, c, df);
                if (!alive) {
                    if (df.pending) { s.flags |= kFlagZombie; alive = true; zombie_now = true; }
                    else finish_path(P, s);
                }
            }
        }
        // A chunk of camera paths only (the samples of one or two pixels): nearly every lane casts a shadow ray and the rays leave a
        // pixel-sized patch towards one emitter, so they are resolved here, on the spot, by the cluster-culling any-hit loop instead of
        // going through the ring (same additions to the radiance in the same order: res + nee; a path that died after casting its ray
        // is finished at once instead of waiting one launch as a zombie)
        if (INLINE && MTS_FLAT_CULL && MTS_PRIMARY_SHADOW && P.sv.n_clusters > 1u && __ballot(depth0 != 1u && (i0 + lane < n_in)) == 0ull) {
            if (df.pending) {
                if (!traverse_flat_clustered_any(P.sv, lds, df.so, df.sd, df.smint, df.smaxt, c.tri_tests)) add_nee(s, df.nee);
                df.pending = false;
                if (zombie_now) { s.flags &= ~kFlagZombie; finish_path(P, s); alive = false; }
            }
        }
        // RGB ring: a path that died with its shadow ray pending leaves the pool now.  Its radiance and valid_ray wait in its place of the
        // sample stream, its ring entry (below) tells the drain to finish it; the workgroup fence ahead of the drain orders write and read.
        bool final_now = false;
        if constexpr (INLINE && kRingFinishes<State>) {
            if (zombie_now && df.pending) {          // (not pending: the camera-path chunk above has finished it)
                P.out_rgba[s.ordinal] = make_float4(s.res.x, s.res.y, s.res.z, (s.flags & 1u) ? 1.0f : 0.0f);
                alive = false; final_now = true;
            }
        }
        // survivors are compacted to the front of the output segment, their shadow rays into a dense queue of their own
        const uint64_t m = __ballot(alive), ms = __ballot((alive || final_now) && df.pending);
        if (alive) {
            const uint32_t slot = n_out + mask_rank(m);
            // gathering: the segment of wave + 4 q takes the slots [q seg_cap, (q + 1) seg_cap) of this hardware wave
            const size_t oidx = (FLAT && gw > 4u) ? ((size_t) wave + 4u * (slot / P.seg_cap)) * P.seg_cap + slot % P.seg_cap : base + slot;
            store_state<kNT>(P.out, oidx, s);
            if (df.pending) {
                if (INLINE) {
                    const uint32_t k = (q_head + q_count + mask_rank(ms)) & (kShadowRing - 1u);
                    ring.o[k] = make_float4(df.so.x, df.so.y, df.so.z, df.smint);
                    ring.d[k] = make_float4(df.sd.x, df.sd.y, df.sd.z, df.smaxt);
                    const uint32_t rslot = (uint32_t) (oidx - base);      // may exceed the segment (gathering): an offset from `base` all the same
                    if (ShadowRing<State>::kSlotInNee) {
                        ring.nee[k] = make_float4(df.nee[0], df.nee[1], df.nee[2], __uint_as_float(rslot));
                    } else {
                        ring.nee[k] = make_float4(df.nee[0], df.nee[1], df.nee[2], df.nee[3]);
                        ring.slot[k] = rslot;
                    }
                } else {
                    const size_t q = base + n_sh + mask_rank(ms);
                    st_stream<kNT>(P.out.sh_o + q, make_float4(df.so.x, df.so.y, df.so.z, df.smint));
                    st_stream<kNT>(P.out.sh_d + q, make_float4(df.sd.x, df.sd.y, df.sd.z, df.smaxt));
                    st_stream<kNT>(P.out.nee + q, make_float4(df.nee[0], df.nee[1], df.nee[2], df.nee[3]));
                    st_stream<kNT>(P.out.sh_slot + q, slot);
                }
            }
        }
        if constexpr (INLINE && kRingFinishes<State>) {
            if (final_now) {
                const uint32_t k = (q_head + q_count + mask_rank(ms)) & (kShadowRing - 1u);
                ring.o[k] = make_float4(df.so.x, df.so.y, df.so.z, df.smint);
                ring.d[k] = make_float4(df.sd.x, df.sd.y, df.sd.z, df.smaxt);
                ring.nee[k] = make_float4(df.nee[0], df.nee[1], df.nee[2], __uint_as_float(s.ordinal | kRingFinal));
            }
        }
        n_out += (uint32_t) __popcll(m);
        n_sh += (uint32_t) __popcll(ms);
        if (INLINE) {
            q_count += (uint32_t) __popcll(ms);
            if (q_count >= 64u) {
                drain_shadow_ring<State, GENERAL>(P, lds, ring, q_head, 64u, base, c);
                q_head = (q_head + 64u) & (kShadowRing - 1u); q_count -= 64u;
            }
        }
    }
    if (INLINE && q_count > 0u) drain_shadow_ring<State, GENERAL>(P, lds, ring, q_head, q_count, base, c);

    const uint32_t n_surv = n_out;                           // border between the survivors and the camera paths generated below
    uint64_t cursor = P.cursor[wave];
    const uint64_t end = P.cursor_end[wave];
    while (n_out < P.target && cursor < end) {
        uint64_t left = end - cursor;
        uint32_t n_new = min(64u, P.target - n_out);
        if ((uint64_t) n_new > left) n_new = (uint32_t) left;
        if (lane < n_new) {
            State s;
            uint64_t ordinal; uint32_t lp, sj;
            cursor_sample(P, wave, cursor + lane, ordinal, lp, sj);
            start_path(P, ordinal, lp, sj, s);
            store_state<kNT>(P.out, base + n_out + lane, s);
        }
        n_out += n_new; cursor += n_new;
    }

    uint32_t tot[4] = { c.closest, c.any, c.segments, c.tri_tests };
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int off = 32; off > 0; off >>= 1) tot[k] += __shfl_xor(tot[k], off);
    if (FLAT && gw > 4u) {               // the segments this hardware wave filled: full ones, one partial, empty ones
        for (uint32_t q = lane; q < gw / 4u; q += 64u) {
            const uint32_t w2 = wave + 4u * q, lo = q * P.seg_cap;
            if (w2 < wave_last) P.count_out[w2] = n_out > lo ? min(n_out - lo, P.seg_cap) : 0u;
        }
    }
    if (lane == 0) {
        if (!(FLAT && gw > 4u)) P.count_out[wave] = n_out;
        if (FLAT && !(gw > 4u)) P.count_out[P.n_waves + wave] = n_surv;
        if (!INLINE) P.count_shadow[wave] = n_sh;
        P.cursor[wave] = cursor;
        uint64_t *ws = P.wave_stats + 4u * (size_t) wave;
        ws[0] += tot[0]; ws[1] += tot[1]; ws[2] += tot[2];
        if (FLAT) ws[3] += tot[3];
    }
}

// ---------------------------------------------------------------------------------------------
// End of a pass.  Once the sample cursors are dry the pool only shrinks, and a launch round (two or three dependent kernels per
// chain, every one spanning all scheduling waves) costs its fixed ~0.1 ms however few paths are left; the deepest paths need dozens
// of such rounds.  k_finish takes the pool as it stands and runs every remaining path to its end inside ONE launch: a workgroup of
// one hardware wave gathers the paths of `per` consecutive scheduling waves (prefix sums in LDS), a lane that finishes a path takes
// the next one of the workgroup's list at once, every loop trip is one path.cpp iteration (both ray queries inline, as in k_bounce:
// the floating-point operations on a sample and their order are those of the other schedules, the film is unchanged).
constexpr uint32_t kFinishMaxPer = 1024u, kFinishLdsDepth = 8u;      // the spill area is sized for k_trace AND for this depth (trace_spill_words)
template <bool GENERAL, bool FLAT, bool ELIDE = true>
MTS_DEV bool step_fused(const RenderParams &P, const LdsView &lds, PathState &s, Counters &c) { return bounce_step<FLAT, 0, GENERAL, false, NoProbe, ELIDE>(P, lds, s, c); }
template <bool GENERAL, bool FLAT, bool ELIDE = true>
MTS_DEV bool step_fused(const RenderParams &P, const LdsView &lds, PathStateS &s, Counters &c) { return bounce_step_spectral<FLAT, false, GENERAL>(P, lds, s, c); }
template <bool GENERAL, bool FLAT, bool ELIDE = true>
MTS_DEV bool step_fused(const RenderParams &P, const LdsView &lds, PathStateT &s, Counters &c) { return bounce_step_spectral<FLAT, 0, GENERAL, false, NoProbeS, true>(P, lds, s, c); }

template <typename State, bool GENERAL, bool FLAT>
__global__ __launch_bounds__(64) void k_finish(const RenderParams P, uint32_t per) {
    extern __shared__ float4 smem[];
    __shared__ uint32_t s_pre[kFinishMaxPer + 1];
    const uint32_t lane = threadIdx.x, w0 = blockIdx.x * per;
    const uint32_t n_w = min(per, P.n_waves - min(P.n_waves, w0));
    {   // s_pre[k] = paths in the workgroup's scheduling waves before the k-th (a run of entries per lane + a wave scan)
        const uint32_t run = (n_w + 63u) / 64u;
        uint32_t local = 0u;
        for (uint32_t i = 0; i < run; ++i) { const uint32_t k = lane * run + i; if (k < n_w) local += P.count_in[w0 + k]; }
        uint32_t incl = local;
        for (uint32_t off = 1u; off < 64u; off <<= 1) { const uint32_t v = __shfl_up(incl, off); if (lane >= off) incl += v; }
        uint32_t sum = incl - local;
        if (lane == 0u) s_pre[0] = 0u;
        for (uint32_t i = 0; i < run; ++i) { const uint32_t k = lane * run + i; if (k < n_w) { sum += P.count_in[w0 + k]; s_pre[k + 1u] = sum; } }
    }
    __syncthreads();
    const uint32_t total = s_pre[n_w];
    if (total == 0u) return;
    for (uint32_t k = lane; k < n_w; k += 64u) P.count_out[w0 + k] = 0u;
    LdsView lds = {};
    if (FLAT) lds = lds_stage<true>(P.sv, smem);
    else {          // the BVH walks keep the first entries of their stack in LDS, the rest in this workgroup's slice of the k_trace spill area
        lds.stride = 64u; lds.stack = reinterpret_cast<uint32_t *>(smem);
        lds.stack_lds_depth = min(P.sv.stack_depth, kFinishLdsDepth);
        lds.spill = reinterpret_cast<StackEntry *>(P.trace_spill) + (size_t) blockIdx.x * (P.sv.stack_depth - lds.stack_lds_depth) * 64u + lane;
        lds.spill_stride = 64u;
    }
    Counters c = { 0u, 0u, 0u, 0u };
    State s;
    bool busy = false;
    uint32_t next = 0u;
    while (true) {
        const uint64_t m = __ballot(!busy);
        if (m != 0ull && next < total) {
            const uint32_t idx = next + mask_rank(m);
            if (!busy && idx < total) {
                uint32_t k = 0u;          // s_pre[k] <= idx < s_pre[k + 1]
                for (uint32_t step = kFinishMaxPer >> 1; step; step >>= 1) if (k + step < n_w && s_pre[k + step] <= idx) k += step;
                load_state(P.in, (size_t) (w0 + k) * P.seg_cap + (idx - s_pre[k]), s);
                if (s.flags & kFlagZombie) finish_path(P, s);      // only its shadow ray was outstanding
                else busy = true;
            }
            next += (uint32_t) __popcll(m);
        }
        if (__ballot(busy) == 0ull) {
            if (next >= total) break;
            continue;
        }
        if (busy && !step_fused<GENERAL, FLAT>(P, lds, s, c)) { finish_path(P, s); busy = false; }
    }
    uint32_t tot[4] = { c.closest, c.any, c.segments, c.tri_tests };
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int off = 32; off > 0; off >>= 1) tot[k] += __shfl_xor(tot[k], off);
    if (lane == 0u) {                  // the workgroup owns its scheduling waves: no atomics
        uint64_t *ws = P.wave_stats + 4u * (size_t) w0;
        ws[0] += tot[0]; ws[1] += tot[1]; ws[2] += tot[2]; ws[3] += tot[3];
    }
}

// Small passes (and, in experiment builds, MTSAMD_MEGA=1 for any pass): the whole pass as ONE launch of persistent lanes -- no pool, no
// launch rounds, no host polling.  A workgroup (one hardware wave) owns the samples of one scheduling wave; a lane whose path ends starts
// the next sample at once.  In steady state the wavefront schedule is faster (1.9 x on the 261 k-triangle mesh, 2 % on
// the Cornell box); a pass of a few samples per lane -- one iteration of an inverse-rendering loop at 1 spp -- is bound by the number of
// launches instead: a dozen launch rounds against one launch.  Same floating-point operations per sample in the same order.
template <typename State, bool GENERAL, bool FLAT>
__global__ __launch_bounds__(64) void k_mega(const RenderParams P) {
    extern __shared__ float4 smem[];
    const uint32_t lane = threadIdx.x, wave = blockIdx.x;
    uint64_t cursor = P.cursor[wave];
    const uint64_t end = P.cursor_end[wave];
    if (cursor >= end) return;
    LdsView lds = {};
    if (FLAT) lds = lds_stage<true>(P.sv, smem);
    else {
        lds.stride = 64u; lds.stack = reinterpret_cast<uint32_t *>(smem);
        lds.stack_lds_depth = min(P.sv.stack_depth, kFinishLdsDepth);
        lds.spill = reinterpret_cast<StackEntry *>(P.trace_spill) + (size_t) blockIdx.x * (P.sv.stack_depth - lds.stack_lds_depth) * 64u + lane;
        lds.spill_stride = 64u;
    }
    Counters c = { 0u, 0u, 0u, 0u };
    State s;
    bool busy = false;
    while (true) {
        const uint64_t m = __ballot(!busy);
        if (m != 0ull && cursor < end) {
            const uint64_t v = cursor + mask_rank(m);
            if (!busy && v < end) {
                uint64_t ordinal; uint32_t lp, sj;
                cursor_sample(P, wave, v, ordinal, lp, sj);
                start_path(P, ordinal, lp, sj, s);
                busy = true;
            }
            cursor += (uint64_t) __popcll(m);
        }
        if (__ballot(busy) == 0ull) {
            if (cursor >= end) break;
            continue;
        }
        // diffuse RGB hierarchy scenes: the fated-path rule would cost this kernel its fourth wave per SIMD (126 -> 134 VGPRs), measured
        // as -6 % on a 261 k-triangle mesh (profiles/r27_ab_fated_elide.txt); the spectral states ignore the flag
        if (busy && !step_fused<GENERAL, FLAT, FLAT || GENERAL>(P, lds, s, c)) { finish_path(P, s); busy = false; }
    }
    uint32_t tot[4] = { c.closest, c.any, c.segments, c.tri_tests };
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int off = 32; off > 0; off >>= 1) tot[k] += __shfl_xor(tot[k], off);
    if (lane == 0u) {
        P.cursor[wave] = end;
        uint64_t *ws = P.wave_stats + 4u * (size_t) wave;
        ws[0] += tot[0]; ws[1] += tot[1]; ws[2] += tot[2]; ws[3] += tot[3];
    }
}

// Host side: the variant of a path kernel a launch needs.  `f` is called with the state type (tabulated spectra / spectral / RGB) as a
// VariantState tag and with GENERAL (the BSDF switch is compiled in) as a std::bool_constant; with_flag does the same for one bool.
template <typename S> struct VariantState { using type = S; };
template <typename F> static void with_variant(const RenderParams &p, F &&f) {
    if (p.spectral && p.sv.n_spectra) f(VariantState<PathStateT>{}, std::true_type{});
    else if (p.spectral && p.sv.general) f(VariantState<PathStateS>{}, std::true_type{});
    else if (p.spectral) f(VariantState<PathStateS>{}, std::false_type{});
    else if (p.sv.general) f(VariantState<PathState>{}, std::true_type{});
    else f(VariantState<PathState>{}, std::false_type{});
}
template <typename F> static void with_flag(bool v, F &&f) { if (v) f(std::true_type{}); else f(std::false_type{}); }
#define MTS_VARIANT(st, general) typename decltype(st)::type, decltype(general)::value

hipError_t launch_mega(const RenderParams &p, hipStream_t s) {
    const size_t lds = p.sv.flat ? lds_bytes(p.sv, 64u) : sizeof(StackEntry) * (std::min(p.sv.stack_depth, kFinishLdsDepth) + 1u) * 64u;
    const uint32_t blocks = p.n_waves;
    hipError_t err = hipSuccess;
    with_flag(p.sv.flat != 0u, [&](auto flat) {
        with_variant(p, [&](auto st, auto general) { err = launch_lds(k_mega<MTS_VARIANT(st, general), decltype(flat)::value>, dim3(blocks), dim3(64), lds, s, p); });
    });
    return err;
}

hipError_t launch_finish(const RenderParams &p, uint64_t alive, hipStream_t s) {
    // about four paths per lane (alive: upper bound of the paths left), at least 2048 workgroups if there are that many scheduling waves
    const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(alive / 256u, 2048u), p.n_waves);
    const uint32_t per = std::min((uint32_t) ((p.n_waves + want - 1u) / want), kFinishMaxPer);
    const uint32_t blocks = (p.n_waves + per - 1u) / per;
    const size_t lds = p.sv.flat ? lds_bytes(p.sv, 64u) : sizeof(StackEntry) * (std::min(p.sv.stack_depth, kFinishLdsDepth) + 1u) * 64u;
    hipError_t err = hipSuccess;
    with_flag(p.sv.flat != 0u, [&](auto flat) {
        with_variant(p, [&](auto st, auto general) { err = launch_lds(k_finish<MTS_VARIANT(st, general), decltype(flat)::value>, dim3(blocks), dim3(64), lds, s, p, per); });
    });
    return err;
}

// k_trace<false>: closest hit of every path's ray (input pool).
// k_trace<true>: visibility of the queued shadow rays (output pool of k_shade), radiance[slot] += nee if unoccluded.
// A workgroup drains the rays of a GROUP of consecutive scheduling waves back to back (dynamic fetch, see the kernel body): kTraceGroup
// waves on hierarchy scenes, kFlatGroup on LDS-resident scenes (shadow queues only: about a third of the paths queue a shadow ray;
// 64-thread workgroups sized to the queues were measured slower).
// kTraceBlock: threads per workgroup on hierarchy scenes.  256; MTS_TRACE_BLOCK=1024 (two workgroups per CU, each with a copy of the
// top of the BVH in LDS next to its stack rows) was built and measured slower.
#ifndef MTS_TRACE_BLOCK
#define MTS_TRACE_BLOCK 256
#endif
// Scheduling waves per workgroup: the longer a workgroup's ray list, the smaller the share of its rounds that run in the tail of the
// list (a few lanes finishing the longest walks, profiles/r03_trace_phases.txt), the fewer workgroups a launch has to balance:
// 4 / 8 / 16 / 32 / 64 waves per 256 threads -> mesh render 55.1 / 51.5 / 49.9 / 51.0 / 58.8 ms (profiles/r03_ab_trace_group.txt).
#ifndef MTS_TRACE_GROUP
#define MTS_TRACE_GROUP (MTS_TRACE_BLOCK / 16)
#endif
constexpr uint32_t kTraceBlock = MTS_TRACE_BLOCK;      // threads per k_trace workgroup (hierarchy scenes)
constexpr uint32_t kTraceGroup = MTS_TRACE_GROUP;      // hierarchy scenes: scheduling waves per workgroup (a power of two)
constexpr uint32_t kFlatGroup = 8u;                    // LDS-resident scenes (shadow queues only)
static_assert((kTraceGroup & (kTraceGroup - 1u)) == 0u, "locate() searches a power-of-two table");
static_assert(kChainAlign % kTraceGroup == 0u, "a k_trace group must not straddle two launch chains");
// LDS part of k_trace's per-lane stack: entries of 8 bytes (BVH4: reference + entry distance); the full 41-entry stack of the
// 261 k-triangle mesh would cap the CU at a fraction of a workgroup.  Deeper entries go to a global spill area (rare).
#ifndef MTS_TRACE_LDS_DEPTH
#define MTS_TRACE_LDS_DEPTH (MTS_BVH4 ? (MTS_TRACE_BLOCK >= 1024 ? 6 : 8) : 16)
#endif
constexpr uint32_t kTraceLdsDepth = MTS_TRACE_LDS_DEPTH;
// Top of the BVH4 staged in LDS by every k_trace workgroup: the first kTraceTopNodes nodes in BFS order (64 B each).
#ifndef MTS_TRACE_TOP_NODES
#define MTS_TRACE_TOP_NODES 0
#endif
constexpr uint32_t kTraceTopNodes = MTS_TRACE_TOP_NODES;

// Register budget of k_trace: 64 VGPRs = 8 waves per SIMD.  The walks are bound by the latency of their node / triangle fetches
// (L2 and beyond for a 261 k-triangle scene), which only more waves in flight hide: 5 waves (84 VGPRs, the compiler's own choice)
// -> 8 waves: +7.5 % on the whole render (RGB and spectral).
#ifndef MTS_TRACE_WAVES
#define MTS_TRACE_WAVES 8
#endif
template <bool ANY, bool FLAT = false>
__global__ __launch_bounds__(FLAT ? kBlock : kTraceBlock)
#if MTS_TRACE_WAVES > 0
__attribute__((amdgpu_waves_per_eu(MTS_TRACE_WAVES, MTS_TRACE_WAVES)))
#endif
void k_trace(const RenderParams P) {
    constexpr uint32_t kShadowGroup = FLAT ? kFlatGroup : kTraceGroup;
    extern __shared__ float4 smem[];
    __shared__ uint32_t s_pre[kShadowGroup + 1u];            // s_pre[g] = work items of the group's scheduling waves before the g-th
    LdsView lds = {};
    const uint32_t n_top = (FLAT || kTraceTopNodes == 0u) ? 0u : P.trace_top_nodes;
    if (FLAT) {
        lds = lds_stage<true>(P.sv, smem);
    } else {
        // LDS: [top of the BVH4: n_top nodes of 4 x 16 B][traversal stack rows]
        uint4 *top = reinterpret_cast<uint4 *>(smem);
        for (uint32_t i = threadIdx.x; i < 4u * n_top; i += blockDim.x) top[i] = P.sv.wnodes[i];
        lds.stride = blockDim.x;
        lds.stack = reinterpret_cast<uint32_t *>(smem + 4u * n_top);
    }
    uint32_t tri_tests = 0;
    // work list of this workgroup: the shadow queues (ANY) or the path slots (closest hit) of kShadowGroup scheduling waves
    const PoolView &pool = ANY ? P.out : P.in;
    // a launch covers the scheduling waves [wave_first, wave_last) (wave_first is a multiple of kShadowGroup)
    const uint32_t wave_last = P.wave_last ? P.wave_last : P.n_waves;
    const uint32_t group = P.wave_first / kShadowGroup + blockIdx.x;      // global group index
    const uint32_t w0 = group * kShadowGroup;
    const uint32_t *counts = ANY ? P.count_shadow : P.count_in;
    // small groups: the counts are wave-uniform and stay in scalar registers; large groups (1024-thread workgroups): prefix sums in LDS
    constexpr bool kCountsInLds = kShadowGroup > 8u;
    uint32_t cnt[kCountsInLds ? 1u : kShadowGroup], total = 0;
    if (kCountsInLds) {
        if (threadIdx.x < 64u) {                             // prefix sums of the group's counts by the first wave
            const uint32_t ln = threadIdx.x;
            uint32_t incl = (ln < kShadowGroup && w0 + ln < wave_last) ? counts[w0 + ln] : 0u;
            for (uint32_t off = 1u; off < kShadowGroup; off <<= 1) { const uint32_t v = __shfl_up(incl, off); if (ln >= off) incl += v; }
            if (ln < kShadowGroup) s_pre[ln + 1u] = incl;
            if (ln == 0u) s_pre[0] = 0u;
        }
    } else {
#pragma unroll
        for (uint32_t g = 0; g < kShadowGroup; ++g) { cnt[g] = (w0 + g < wave_last) ? counts[w0 + g] : 0u; total += cnt[g]; }
    }
    __shared__ uint32_t s_next;
    if (threadIdx.x == 0) s_next = 0u;
    __syncthreads();
    if (kCountsInLds) total = s_pre[kShadowGroup];
    auto locate = [&](uint32_t idx) -> size_t {              // work item -> pool index
        if (kCountsInLds) {                                  // s_pre[g] <= idx < s_pre[g + 1]
            uint32_t g = 0u;
#pragma unroll
            for (uint32_t step = kShadowGroup >> 1; step; step >>= 1) if (s_pre[g + step] <= idx) g += step;
            return (size_t) (w0 + g) * P.seg_cap + (idx - s_pre[g]);
        }
        uint32_t wave = w0, i = idx;
#pragma unroll
        for (uint32_t g = 0; g + 1 < kShadowGroup; ++g)
            if (wave == w0 + g && i >= cnt[g]) { i -= cnt[g]; ++wave; }
        return (size_t) wave * P.seg_cap + i;
    };
    constexpr bool kNT = !FLAT && (MTS_NT_STREAMS & 1) != 0;
    auto retire_any = [&](size_t k) {                        // unoccluded shadow ray: radiance[slot] += nee
        const size_t slot = (k / P.seg_cap) * P.seg_cap + ld_stream<kNT>(pool.sh_slot + k);
        float4 r = pool.res[slot];
        const float4 e = ld_stream<kNT>(pool.nee + k);
        r.x += e.x; r.y += e.y; r.z += e.z; r.w += e.w;      // RGB: w = eta + 0
        pool.res[slot] = r;
    };
    if (FLAT) {
        Hit h;
        for (uint32_t idx = threadIdx.x; idx < total; idx += blockDim.x) {
            const size_t k = locate(idx);
            const float4 o = pool.sh_o[k], d = pool.sh_d[k];
            if (!traverse<true, true>(P.sv, lds, mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z), o.w, d.w, h, tri_tests)) retire_any(k);
        }
    } else {
        // Dynamic ray fetch: a lane that has finished its walk takes the next item of the workgroup's list at once instead of
        // idling until the slowest lane of its wave is done (the walks of incoherent rays differ several-fold in length: with
        // one ray per lane and loop trip only 22-29 % of the VALU lane-cycles were useful).
        const uint32_t lane = lane_id();
        // LDS holds the first P.trace_lds_depth stack entries of every lane; deeper entries spill to this workgroup's slice of
        // P.trace_spill ([entry][thread])
        const uint32_t spill_depth = P.sv.stack_depth > P.trace_lds_depth ? P.sv.stack_depth - P.trace_lds_depth : 0u;
        const WalkStack st = { reinterpret_cast<StackEntry *>(lds.stack) + threadIdx.x, log2_stride(lds.stride), P.trace_lds_depth,
                               reinterpret_cast<StackEntry *>(P.trace_spill) + ((size_t) (ANY ? (P.n_waves + kShadowGroup - 1u) / kShadowGroup : 0u) + group) * spill_depth * kTraceBlock + threadIdx.x, blockDim.x,
                               reinterpret_cast<const uint4 *>(smem), n_top };
        BvhWalk w;
        w.cur = kNoNode; w.sp = 0u; w.found = false;
        constexpr uint32_t kNoItem = 0xffffffffu;
        uint32_t k = kNoItem;                                // pool index of the work item the lane holds (the pools have fewer than 2^32 slots)
        bool exhausted = false;
        while (true) {
            const bool need = w.cur == kNoNode;
            MTS_PROF(ANY, 12);                               // iterations of the work loop
            if (need && k != kNoItem) {                      // retire the finished item
                MTS_PROF(ANY, 14);
                if (ANY) { if (!w.found) retire_any(k); }
                else st_stream<kNT>(pool.hit + k, w.found ? make_float4(w.best, __uint_as_float(w.best_prim), w.hit.u, w.hit.v)
                                                          : make_float4(__builtin_inff(), __uint_as_float(kNoPrim), 0.0f, 0.0f));
                k = kNoItem;
            }
            const uint64_t m = __ballot(need);
            if (m && !exhausted) {
                const uint32_t first = (uint32_t) __ffsll((long long) m) - 1u, want = (uint32_t) __popcll(m);
                uint32_t base = 0u;
                if (lane == first) base = atomicAdd(&s_next, want);
                base = __shfl(base, (int) first);
                exhausted = base + want >= total;
                if (need) {
                    MTS_PROF(ANY, 10);                       // fetches
                    const uint32_t idx = base + mask_rank(m);
                    if (idx < total) {
                        const uint32_t item = (uint32_t) locate(idx);
                        if (ANY) {
                            const float4 o = ld_stream<kNT>(pool.sh_o + item), d = ld_stream<kNT>(pool.sh_d + item);
                            walk_begin(w, P.sv, mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z), o.w, d.w);
                            k = item;
                        } else if (!((pool.misc[item].y >> 16) & kFlagZombie)) {      // zombies only wait for their shadow ray
                            const float4 o = ld_stream<kNT>(pool.ray_o + item), d = ld_stream<kNT>(pool.ray_d + item);
                            walk_begin(w, P.sv, mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z), o.w, d.w);
                            k = item;
                        }
                    }
                }
            }
            if (__ballot(w.cur != kNoNode) == 0ull) {
                if (exhausted) break;
                continue;                                    // only zombies were fetched: try again
            }
            MTS_PROF_MASK(ANY, exhausted ? 22 : 20, __ballot(w.cur != kNoNode));      // rounds before / after the list ran out: lanes with a ray
            if (__ballot(w.cur != kNoNode && w.far) != 0ull) {      // wave-uniform choice of the slab-test form
                if (w.cur != kNoNode) walk_round<ANY, true, kTraceTopNodes != 0u>(w, P.sv, st, tri_tests);
            } else {
                if (w.cur != kNoNode) walk_round<ANY, false, kTraceTopNodes != 0u>(w, P.sv, st, tri_tests);
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) tri_tests += __shfl_xor(tri_tests, off);
    if (lane_id() == 0 && tri_tests)
        atomicAdd(reinterpret_cast<unsigned long long *>(P.wave_stats + 4u * (size_t) w0 + 3u),
                  (unsigned long long) tri_tests);
}

#if MTS_TRACE_PROF
// experiment builds: the phase counters of device_scene.h (scripts/debug/trace_prof.py)
extern "C" __attribute__((visibility("default"))) int mtsamd_debug_trace_prof(unsigned long long *out, int reset) {
    static unsigned long long host[64 * 64];
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_trace_prof), sizeof(host)) != hipSuccess) return -1;
    for (int i = 0; i < 64; ++i) { out[i] = 0; for (int c = 0; c < 64; ++c) out[i] += host[64 * c + i]; }
    if (reset) { for (auto &h : host) h = 0; if (hipMemcpyToSymbol(HIP_SYMBOL(g_trace_prof), host, sizeof(host)) != hipSuccess) return -1; }
    return 0;
}
#endif

uint32_t trace_top_nodes(const SceneView &sv) { return std::min(sv.n_wnodes, kTraceTopNodes); }
uint32_t trace_group() { return kTraceGroup; }
size_t trace_lds_bytes(const SceneView &sv) {      // top of the tree + the stack rows (+ the scratch row of stack_row())
    return (size_t) 64 * trace_top_nodes(sv) + sizeof(StackEntry) * (std::min(sv.stack_depth, kTraceLdsDepth) + 1u) * kTraceBlock;
}
uint32_t trace_lds_depth(const SceneView &sv) { return std::min(sv.stack_depth, kTraceLdsDepth); }
// spill area shared by k_trace (closest-hit and any-hit launches may overlap: two slices per group) and k_finish (its workgroups are
// single waves that keep kFinishLdsDepth entries in LDS)
size_t trace_spill_words(const SceneView &sv, uint32_t n_waves) {
    const uint32_t spill = sv.stack_depth > kTraceLdsDepth ? sv.stack_depth - kTraceLdsDepth : 0u;
    const uint32_t spill_f = sv.stack_depth > kFinishLdsDepth ? sv.stack_depth - kFinishLdsDepth : 0u;
    const size_t trace = (size_t) 2 * ((n_waves + kTraceGroup - 1) / kTraceGroup) * spill * kTraceBlock;
    const size_t finish = (size_t) n_waves * spill_f * 64u;      // at most one k_finish workgroup per scheduling wave
    return (sizeof(StackEntry) / 4) * std::max(trace, finish);
}

// split pipeline of hierarchy scenes, one stage at a time: 0 = k_trace<closest>, 1 = k_shade, 2 = k_trace<any>.  Stage 2 of one
// iteration and stage 0 of the next touch disjoint arrays, so the host runs them on two streams (api.cpp).
hipError_t launch_split_stage(const RenderParams &p, int stage, hipStream_t s) {
    const uint32_t n_launch = (p.wave_last ? p.wave_last : p.n_waves) - p.wave_first;
    const uint32_t shade_blocks = (n_launch * 64u + kBlock - 1) / kBlock, trace_blocks = (n_launch + kTraceGroup - 1) / kTraceGroup;
    if (stage == 0) {
        if (hipError_t e = allow_lds(reinterpret_cast<const void *>(&k_trace<false, false>), trace_lds_bytes(p.sv))) return e;
        hipLaunchKernelGGL((k_trace<false, false>), dim3(trace_blocks), dim3(kTraceBlock), trace_lds_bytes(p.sv), s, p);
    } else if (stage == 1) {
        with_variant(p, [&](auto st, auto general) { hipLaunchKernelGGL((k_shade<MTS_VARIANT(st, general), false>), dim3(shade_blocks), dim3(kBlock), 0, s, p); });
    } else {
        if (hipError_t e = allow_lds(reinterpret_cast<const void *>(&k_trace<true, false>), trace_lds_bytes(p.sv))) return e;
        hipLaunchKernelGGL((k_trace<true, false>), dim3(trace_blocks), dim3(kTraceBlock), trace_lds_bytes(p.sv), s, p);
    }
    return hipGetLastError();
}

hipError_t launch_bounce(const RenderParams &p_, hipStream_t s) {
    RenderParams p = p_;
    if (p.split == 3) {       // LDS-resident scene, one kernel: shadow rays collected in a per-wave LDS ring and resolved 64 at a time
        const uint32_t n_launch = (p.wave_last ? p.wave_last : p.n_waves) - p.wave_first;
        const uint32_t shade_blocks = p.gather_w > 4u ? (n_launch + p.gather_w - 1u) / p.gather_w : (n_launch * 64u + kBlock - 1) / kBlock;
        p.lds_queue_offset = (uint32_t) (shade_ring_offset(p.sv, kBlock) / 16u);
        const size_t lds = shade_ring_lds_bytes(p.sv, p.spectral != 0, p.gather_w);
        hipError_t err = hipSuccess;
        with_variant(p, [&](auto st, auto general) { err = launch_lds(k_shade<MTS_VARIANT(st, general), true, true>, dim3(shade_blocks), dim3(kBlock), lds, s, p); });
        return err;
    }
    if (p.split == 2) {       // LDS-resident scene: closest hit + shading fused, shadow rays queued and resolved in dense batches
        const uint32_t shade_blocks = (p.n_waves * 64u + kBlock - 1) / kBlock;
        const size_t lds = bounce_lds_bytes(p.sv);
        hipError_t err = hipSuccess;
        with_variant(p, [&](auto st, auto general) { err = launch_lds(k_shade<MTS_VARIANT(st, general), true>, dim3(shade_blocks), dim3(kBlock), lds, s, p); });
        if (err != hipSuccess) return err;
        return launch_lds(k_trace<true, true>, dim3((p.n_waves + kFlatGroup - 1) / kFlatGroup), dim3(kBlock), lds, s, p);
    }
    if (p.split) {
        hipError_t e = launch_split_stage(p, 0, s);
        if (e == hipSuccess) e = launch_split_stage(p, 1, s);
        if (e == hipSuccess) e = launch_split_stage(p, 2, s);
        return e;
    }
    uint32_t blocks = (p.n_waves * 64u + kBlock - 1) / kBlock;
    if (p.spectral) {
        if (p.sv.n_spectra) {
            if (p.sv.general == 2u) {
                if (p.sv.flat) return launch_lds(k_bounce_spectra<true, true>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
                else return launch_lds(k_bounce_spectra<false, true>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
            } else {
                if (p.sv.flat) return launch_lds(k_bounce_spectra<true, false>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
                else return launch_lds(k_bounce_spectra<false, false>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
            }
        } else if (p.sv.general == 2u) {
            if (p.sv.flat) return launch_lds(k_bounce_spectral<true, true, true>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
            else return launch_lds(k_bounce_spectral<false, true, true>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
        } else if (p.sv.general) {
            if (p.sv.flat) return launch_lds(k_bounce_spectral<true, true>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
            else return launch_lds(k_bounce_spectral<false, true>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
        } else {
            if (p.sv.flat) return launch_lds(k_bounce_spectral<true, false>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
            else return launch_lds(k_bounce_spectral<false, false>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
        }
        return hipGetLastError();
    }
    if (p.sv.general == 2u) {
        if (p.sv.flat) return launch_lds(k_bounce<true, true, true>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
        else return launch_lds(k_bounce<false, true, true>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
    } else if (p.sv.general) {
        if (p.sv.flat) return launch_lds(k_bounce<true, true>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
        else return launch_lds(k_bounce<false, true>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
    } else {
        if (p.sv.flat) return launch_lds(k_bounce<true, false>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
        else return launch_lds(k_bounce<false, false>, dim3(blocks), dim3(kBlock), bounce_lds_bytes(p.sv), s, p);
    }
    return hipGetLastError();
}
#undef MTS_VARIANT

// reconstruction filter (rfilter.h:62-65, gaussian.cpp:45-47, box.cpp:34-36, tent.cpp:33-35, catmullrom.cpp:29-43,
// mitchell.cpp:41-56, lanczos.cpp:38-48); FilterView::alpha / bias carry tent's 1 / radius and mitchell's B / C
MTS_DEV float cubic_filter(float x, float B, float C) {
    x = fabsf(x);
    const float x2 = x * x, x3 = x2 * x;
    const float result = (1.0f / 6.0f) * (x < 1.0f
        ? (12.0f - 9.0f * B - 6.0f * C) * x3 + (-18.0f + 12.0f * B + 6.0f * C) * x2 + (6.0f - 2.0f * B)
        : (-B - 6.0f * C) * x3 + (6.0f * B + 30.0f * C) * x2 + (-12.0f * B - 48.0f * C) * x + (8.0f * B + 24.0f * C));
    return x < 2.0f ? result : 0.0f;
}
MTS_DEV float filter_eval(const FilterView &f, float x) {
    switch (f.kind) {
    case 0: return fmaxf(0.0f, lm_exp(f.alpha * (x * x)) - f.bias);
    case 2: return fmaxf(0.0f, 1.0f - fabsf(x * f.alpha));
    case 3: return cubic_filter(x, 0.0f, 0.5f);
    case 4: return cubic_filter(x, f.alpha, f.bias);
    case 5: {
        x = fabsf(x);
        const float x1 = kPi * x, x2 = x1 / f.radius, result = (lm_sin(x1) * lm_sin(x2)) / (x1 * x2);
        return x < kEpsilon ? 1.0f : (x > f.radius ? 0.0f : result);
    }
    default: return fabsf(x) <= f.radius ? 1.0f : 0.0f;
    }
}
MTS_DEV float filter_weight(const FilterView &f, float x) {
    if (f.analytic) return filter_eval(f, x);
    int idx = min((int) fabsf(x * f.scale_factor), 31);
    return f.table[idx];
}


// ---------------------------------------------------------------------------------------------
// Derivatives of the rendered image.  Each k_adjoint* kernel below replays every camera sample through bounce_step with a probe of its own,
// which turns what the step shows it into a gradient.  A new derivative is a probe and a kernel here; nothing is added to the step.
constexpr int kAdjointMaxDepth = 16;

// dLoss/dRadiance of the camera sample at film position `pos`: the adjoint of ImageBlock::put (imageblock.cpp:117-169, block = the
// crop window, no border) followed by Image = values / (weight + 1e-8) (autodiff.py:80-91)
template <class Params>      // AdjointParams or ReverseParams: rp, filter, dimage, film
MTS_DEV f3 adjoint_delta(const Params &A, float2 pos) {
    const RenderParams &P = A.rp;
    const FilterView &f = A.filter;
    f3 delta = mk3(0.0f, 0.0f, 0.0f);
    const float px = pos.x - ((float) P.crop_x + 0.5f), py = pos.y - ((float) P.crop_y + 0.5f);
    if (f.radius > 1.0f) {
        const int lox = max((int) ceilf(px - f.radius), 0), loy = max((int) ceilf(py - f.radius), 0);
        const int hix = min((int) floorf(px + f.radius), P.crop_w - 1), hiy = min((int) floorf(py + f.radius), P.crop_h - 1);
        const float bx = (float) (uint32_t) lox - px, by = (float) (uint32_t) loy - py;
        for (int yr = 0; yr < f.taps && loy + yr <= hiy; ++yr) {
            const float wy = filter_weight(f, by + (float) yr);
            for (int xr = 0; xr < f.taps && lox + xr <= hix; ++xr) {
                const float w = wy * filter_weight(f, bx + (float) xr);
                const size_t pix = (size_t) (loy + yr) * P.crop_w + (size_t) (lox + xr);
                const float iw = w / (A.film[5 * pix + 4] + 1e-8f);
                delta.x += iw * A.dimage[3 * pix]; delta.y += iw * A.dimage[3 * pix + 1]; delta.z += iw * A.dimage[3 * pix + 2];
            }
        }
    } else {
        const int lox = (int) ceilf(px - 0.5f), loy = (int) ceilf(py - 0.5f);
        if (lox >= 0 && loy >= 0 && lox < P.crop_w && loy < P.crop_h) {
            const size_t pix = (size_t) loy * P.crop_w + (size_t) lox;
            const float iw = 1.0f / (A.film[5 * pix + 4] + 1e-8f);
            delta = mk3(iw * A.dimage[3 * pix], iw * A.dimage[3 * pix + 1], iw * A.dimage[3 * pix + 2]);
        }
    }
    return delta;
}

// The camera samples of a launch are dealt to its threads grid-stride (the loop at the top of each kernel; launch_adjoint_kernel caps
// the grid).  Sample k is regenerated with the PCG32 stream of the primal pass (`s`: the path state at its camera ray); returns
// dLoss/dRadiance of the sample.
template <class Params>
MTS_DEV f3 adjoint_sample(const Params &A, uint64_t k, PathState &s) {
    const uint32_t spp = (uint32_t) A.rp.spp;
    float2 pos;
    generate_path(A.rp, k, (uint32_t) (k / spp), (uint32_t) (k % spp), s, &pos);
    return adjoint_delta(A, pos);
}

// g (per channel) times the bilinear weights of a texture lookup, added to the gradient of its four texels
MTS_DEV void scatter_texel_grad(float *grad_tex, const DevTexture &t, uint32_t texel, f2 w1, const float g[3]) {
    float *gt = grad_tex + t.grad_offset + 3u * (size_t) texel;
    const float w00 = (1.0f - w1.y) * (1.0f - w1.x), w10 = (1.0f - w1.y) * w1.x, w01 = w1.y * (1.0f - w1.x), w11 = w1.y * w1.x;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        atomicAdd(gt + ch, g[ch] * w00); atomicAdd(gt + 3 + ch, g[ch] * w10);
        atomicAdd(gt + 3 * t.w + ch, g[ch] * w01); atomicAdd(gt + 3 * t.w + 3 + ch, g[ch] * w11);
    }
}

// One workgroup per 256 samples, at most 2048 workgroups (the sample loop strides); the scene is staged like k_bounce's
template <auto K_FLAT, auto K_TREE, class A>
static hipError_t launch_adjoint_kernel(const A &a, hipStream_t s) {
    if (a.n_samples == 0) return hipSuccess;
    uint64_t blocks = (a.n_samples + kBlock - 1) / kBlock;
    if (blocks > 2048) blocks = 2048;
    return launch_lds(a.rp.sv.flat ? K_FLAT : K_TREE, dim3((uint32_t) blocks), dim3(kBlock), bounce_lds_bytes(a.rp.sv), s, a);
}

// ---------------------------------------------------------------------------------------------
// Reverse-mode derivative of the rendered image with respect to diffuse reflectances (constant colours and
// bitmap texels), the role Enoki's autodiff plays for mitsuba.python.autodiff.render (autodiff.py:6-91,121-194).
// One thread replays one camera sample with the same PCG32 stream as the primal pass, records its vertices,
// and sweeps them backwards:   Y_k = Nc_k + X_{k+1},  dL/drho_k = delta * T'_k * Y_k,  X_k = E_k + invq_k rho_k Y_k,
// where delta = dLoss/dRadiance of this sample = sum over its filter footprint of w * dLoss/dImage / (W + 1e-8)
// (Image = values / (weight + 1e-8), autodiff.py:80-91); the sweep below also carries the derivative of the
// Russian-roulette factor 1/q(T) (path.cpp:137-141), as Enoki's autodiff does.
//
// What the adjoint pass remembers about one path vertex k.  With T_k the throughput arriving at the vertex,
//   radiance += T_k * E_k;  T'_k = T_k * invq_k (Russian roulette);  radiance += T'_k * rho_k * Nc_k (next-event
//   estimation);  T_{k+1} = T'_k * rho_k (diffuse BSDF sample weight).
struct VertexRec {
    f3 E, Nc, Tp, rho; float invq;
    f3 T; int32_t rr_channel;       // throughput before Russian roulette; channel that sets q (-1: none / q clamped)
    uint32_t texel; f2 w1; int32_t bsdf; uint32_t has_bsdf;
    // radiance-free coefficients for d/d(emitter radiance): E = ew * Le[em_hit], Nc = nk * Le[em_nee] (-1: none)
    float ew, nk; int32_t em_hit, em_nee;
};

// Fills the VertexRec of one diffuse-only step.  The back of a `twosided` diffuse BSDF is replayed mirrored (kMirrorTwoSided).
struct DiffuseRecorder {
    static constexpr bool kFactoredEmitter = true, kMirrorTwoSided = true, kSamples = true;
    VertexRec &r;
    template <int DEFER, bool GENERAL, bool NEST> MTS_DEV void begin(const PathState &s) {
        static_assert(!GENERAL && DEFER == 0 && !NEST, "the diffuse adjoint replay runs the diffuse-only fused step");
        r.E = r.Nc = r.Tp = r.rho = mk3(0.0f, 0.0f, 0.0f);
        r.invq = 1.0f; r.rr_channel = -1; r.T = s.thr; r.texel = kNoPrim; r.w1.x = r.w1.y = 0.0f; r.bsdf = -1; r.has_bsdf = 0u;
        r.ew = r.nk = 0.0f; r.em_hit = r.em_nee = -1;
    }
    MTS_DEV void emitted(float ew, int32_t emitter, f3 le) { r.E = mk3(ew * le.x, ew * le.y, ew * le.z); r.ew = ew; r.em_hit = emitter; }
    MTS_DEV void escaped(const SceneView &, const PathState &, const DevEmitter &, float, f3) { }
    MTS_DEV void roulette(f3 thr, float hm, float rq, bool free) { r.invq = rq; if (free) r.rr_channel = thr.x == hm ? 0 : (thr.y == hm ? 1 : 2); }
    MTS_DEV void surface(const SurfaceInteraction &si, const DevBsdf &, f3 refl, uint32_t texel, f2 tw1, f3 thr) {
        r.Tp = thr; r.rho = refl; r.texel = texel; r.w1 = tw1; r.bsdf = si.shape_rec.bsdf; r.has_bsdf = 1u;
    }
    MTS_DEV bool emitter_sample(const SceneView &, const DevBsdf &, f3, const NeeTerms &t) { return t.r1 * t.r2 != 0.0f; }
    MTS_DEV void unoccluded(const SceneView &, const SurfaceInteraction &, f3, const NeeTerms &t) {
        if (t.wi.z > 0.0f && t.wo.z > 0.0f) {     // d(contrib)/d(rho) / T'_k
            float k = t.mis * (kInvPi * t.wo.z);
            r.Nc = mk3(k * t.spec.x, k * t.spec.y, k * t.spec.z);
            const float em_geo = t.r1 * t.r2;      // spec / radiance of an area light
            if (em_geo != 0.0f) { r.nk = k * em_geo; r.em_nee = (int32_t) t.ds.emitter; }
        }
    }
    MTS_DEV void bsdf_sampled(const SceneView &, const SurfaceInteraction &, const DevBsdf &, f3, f3, const BsdfSample &, f3, float, f2) { }
};

template <bool FLAT>
__global__ __launch_bounds__(kBlock) void k_adjoint(const AdjointParams A) {
    extern __shared__ float4 smem[];
    const RenderParams &P = A.rp;
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    __shared__ float s_grad[3 * 32];                       // per-workgroup sums for constant reflectances
    __shared__ float s_grad_em[3 * 32];                    // ... and for the radiance of area lights
    for (uint32_t i = threadIdx.x; i < 3u * 32u; i += kBlock) s_grad[i] = s_grad_em[i] = 0.0f;
    __syncthreads();
    for (uint64_t k = (uint64_t) blockIdx.x * kBlock + threadIdx.x; k < A.n_samples; k += (uint64_t) gridDim.x * kBlock) {
        PathState s; const f3 delta = adjoint_sample(A, k, s);
        // ---- replay the path, remembering its vertices
        VertexRec rec[kAdjointMaxDepth];
        int n = 0;
        Counters c = { 0u, 0u, 0u, 0u };
        bool alive = true;
        while (alive && n < kAdjointMaxDepth) { alive = bounce_step<FLAT>(P, lds, s, c, DiffuseRecorder{ rec[n] }); ++n; }
        // ---- backward sweep; a = dLoss/dT_v.  q = min(hmax(T) eta^2, .95) is differentiated like Enoki does (the
        // gradient flows to the maximal channel when q is not clamped); the survival test is not differentiable.
        f3 a = mk3(0.0f, 0.0f, 0.0f);
        for (int v = n - 1; v >= 0; --v) {
            const VertexRec &r = rec[v];
            if (A.grad_emitter) {     // radiance is linear in Le: delta * T_v * ew (emitter hit) + delta * T'_v rho_v nk (emitter sampled)
                if (r.em_hit >= 0 && r.em_hit < 32) {
                    atomicAdd(&s_grad_em[3 * r.em_hit], delta.x * r.T.x * r.ew); atomicAdd(&s_grad_em[3 * r.em_hit + 1], delta.y * r.T.y * r.ew);
                    atomicAdd(&s_grad_em[3 * r.em_hit + 2], delta.z * r.T.z * r.ew);
                }
                if (r.em_nee >= 0 && r.em_nee < 32) {
                    atomicAdd(&s_grad_em[3 * r.em_nee], delta.x * (r.Tp.x * r.rho.x) * r.nk); atomicAdd(&s_grad_em[3 * r.em_nee + 1], delta.y * (r.Tp.y * r.rho.y) * r.nk);
                    atomicAdd(&s_grad_em[3 * r.em_nee + 2], delta.z * (r.Tp.z * r.rho.z) * r.nk);
                }
            }
            if (!r.has_bsdf) { a = mk3(delta.x * r.E.x, delta.y * r.E.y, delta.z * r.E.z); continue; }
            const f3 Y = mk3(delta.x * r.Nc.x + a.x, delta.y * r.Nc.y + a.y, delta.z * r.Nc.z + a.z);
            const f3 g = mk3(r.Tp.x * Y.x, r.Tp.y * Y.y, r.Tp.z * Y.z);
            const f3 b = mk3(r.rho.x * Y.x, r.rho.y * Y.y, r.rho.z * Y.z);
            if (r.texel != kNoPrim) {
                const DevTexture t = P.sv.textures[P.sv.bsdfs[r.bsdf].texture];
                const float gg[3] = { g.x, g.y, g.z };
                if (A.grad_tex) scatter_texel_grad(A.grad_tex, t, r.texel, r.w1, gg);
            } else if (A.grad_bsdf && r.bsdf >= 0 && r.bsdf < 32) {
                atomicAdd(&s_grad[3 * r.bsdf], g.x); atomicAdd(&s_grad[3 * r.bsdf + 1], g.y); atomicAdd(&s_grad[3 * r.bsdf + 2], g.z);
            }
            a = mk3(delta.x * r.E.x + r.invq * b.x, delta.y * r.E.y + r.invq * b.y, delta.z * r.E.z + r.invq * b.z);
            if (r.rr_channel >= 0) {
                const float corr = (r.invq * r.invq) * (b.x * r.T.x + b.y * r.T.y + b.z * r.T.z);
                if (r.rr_channel == 0) a.x -= corr; else if (r.rr_channel == 1) a.y -= corr; else a.z -= corr;
            }
        }
    }
    __syncthreads();
    if (A.grad_bsdf)
        for (uint32_t i = threadIdx.x; i < 3u * min(P.sv.n_bsdfs, 32u); i += kBlock)
            if (s_grad[i] != 0.0f) atomicAdd(A.grad_bsdf + i, s_grad[i]);
    if (A.grad_emitter)
        for (uint32_t i = threadIdx.x; i < 3u * min(P.sv.n_emitters, 32u); i += kBlock)
            if (s_grad_em[i] != 0.0f) atomicAdd(A.grad_emitter + i, s_grad_em[i]);
}

hipError_t launch_adjoint(const AdjointParams &a, hipStream_t s) { return launch_adjoint_kernel<k_adjoint<true>, k_adjoint<false>>(a, s); }

// Derivative w.r.t. the texels of the `envmap` emitter ('data', envmap.cpp:214-218; docs/examples/10_inverse_rendering/invert_bunny.py):
// one thread replays one camera sample with the PCG32 stream of the primal pass through the general fused step -- any BSDF, any depth
// -- and scatters d(loss)/d(envmap texels) = delta * d(radiance)/d(texels) into `grad` (h * w * 3) at every use of the map.  The radiance
// is linear in the texels at its two uses, the emission an escaped ray picks up and the emitter sample; the sampling distribution built
// from their luminances is not differentiated (envmap.cpp:220-253 rebuilds it from plain floats).
struct EnvGradProbe {
    static constexpr bool kFactoredEmitter = true, kMirrorTwoSided = false, kSamples = true;
    f3 delta; float *grad;
    MTS_DEV void add(const DevEnvmap &e, float u, float v, f3 coeff) const {
        u *= (float) (e.w - 1); v *= (float) (e.h - 1);                  // the bilinear footprint of envmap_lookup
        const uint32_t px = min((uint32_t) u, (uint32_t) (e.w - 2)), py = min((uint32_t) v, (uint32_t) (e.h - 2));
        const float w1x = u - (float) px, w1y = v - (float) py, w0x = 1.0f - w1x, w0y = 1.0f - w1y;
        const float wt[4] = { (w0y * w0x) * e.scale, (w0y * w1x) * e.scale, (w1y * w0x) * e.scale, (w1y * w1x) * e.scale };
        const uint32_t idx[4] = { py * (uint32_t) e.w + px, py * (uint32_t) e.w + px + 1u, (py + 1u) * (uint32_t) e.w + px, (py + 1u) * (uint32_t) e.w + px + 1u };
        const f3 c = mk3(delta.x * coeff.x, delta.y * coeff.y, delta.z * coeff.z);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float *g = grad + 3u * (size_t) idx[i];
            atomicAdd(g, c.x * wt[i]); atomicAdd(g + 1, c.y * wt[i]); atomicAdd(g + 2, c.z * wt[i]);
        }
    }
    // spec / radiance of an envmap sample (0 for every other emitter)
    MTS_DEV static float em_geo(const SceneView &sv, const NeeTerms &t) { return t.kind == kEmitterEnvmap ? (sv.n_emitters > 1u ? t.r1 * t.r2 : t.r1) : 0.0f; }
    template <int DEFER, bool GENERAL, bool NEST> MTS_DEV void begin(const PathState &) { static_assert(GENERAL && DEFER == 0 && !NEST, "the envmap gradient rides on the general fused step"); }
    MTS_DEV void emitted(float, int32_t, f3) { }
    MTS_DEV void escaped(const SceneView &sv, const PathState &s, const DevEmitter &e, float ew, f3) {
        if (e.pad0 == kEmitterEnvmap) {
            float u, v;
            env_dir_to_uv(mat3_apply(sv.envmap->to_local, s.d), u, v);
            add(*sv.envmap, u, v, mk3(ew * s.thr.x, ew * s.thr.y, ew * s.thr.z));
        }
    }
    MTS_DEV void roulette(f3, float, float, bool) { }
    MTS_DEV void surface(const SurfaceInteraction &, const DevBsdf &, f3, uint32_t, f2, f3) { }
    MTS_DEV bool emitter_sample(const SceneView &sv, const DevBsdf &, f3, const NeeTerms &t) { return em_geo(sv, t) != 0.0f; }
    MTS_DEV void unoccluded(const SceneView &sv, const SurfaceInteraction &, f3 thr, const NeeTerms &t) {
        const float g = em_geo(sv, t);
        if (g != 0.0f) add(*sv.envmap, t.ds.uv.x, t.ds.uv.y, mk3(((t.mis * thr.x) * t.bv.x) * g, ((t.mis * thr.y) * t.bv.y) * g, ((t.mis * thr.z) * t.bv.z) * g));
    }
    MTS_DEV void bsdf_sampled(const SceneView &, const SurfaceInteraction &, const DevBsdf &, f3, f3, const BsdfSample &, f3, float, f2) { }
};

template <bool FLAT>
__global__ __launch_bounds__(kBlock) void k_adjoint_env(const AdjointParams A) {
    extern __shared__ float4 smem[];
    const RenderParams &P = A.rp;
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    for (uint64_t k = (uint64_t) blockIdx.x * kBlock + threadIdx.x; k < A.n_samples; k += (uint64_t) gridDim.x * kBlock) {
        PathState s; const f3 delta = adjoint_sample(A, k, s);
        EnvGradProbe eg = { delta, A.grad_env };
        Counters c = { 0u, 0u, 0u, 0u };
        while (bounce_step<FLAT, 0, true>(P, lds, s, c, eg)) { }
    }
}

hipError_t launch_adjoint_env(const AdjointParams &a, hipStream_t s) { return launch_adjoint_kernel<k_adjoint_env<true>, k_adjoint_env<false>>(a, s); }

// d(loss)/d(one scalar BSDF parameter): derivative of the path's radiance w.r.t. ONE scalar parameter of ONE BSDF record of any model
// (roughness, complex IOR, reflectances ...), carried forward beside the path as a dual part (dthr = d throughput, dres = d radiance).
// Sampling is DETACHED: the replay takes the decisions and directions of the primal path (same PCG32 stream, same parameter value), and
// differentiates what depends on the parameter for fixed directions -- the BSDF value f(wi, wo) cos in the emitter-sampling term and in
// the sample weight f cos / pdf (pdf, lobe probabilities, MIS weights and Russian-roulette probabilities are held fixed: any fixed
// partition of unity keeps the estimator unbiased).  d f / d theta at fixed (wi, wo) is a central difference of the model code itself
// between two records perturbed by +-h (bp / bm): a smooth closed form at fixed arguments, O(h^2) truncation, no decision can flip.
// The reference differentiates the attached estimator through Enoki's graph (src/python/python/autodiff.py:6-91); both estimate the same
// derivative of the image.
struct ParamGradProbe {
    static constexpr bool kFactoredEmitter = false, kMirrorTwoSided = false, kSamples = true;
    int32_t bsdf; DevBsdf bp, bm; float inv_2h; f3 dthr, dres;
    bool here;                  // is the surface's record the one whose parameter is differentiated?
    // the reflectances of the two perturbed records at the surface
    MTS_DEV void perturbed_refl(const SceneView &sv, const SurfaceInteraction &si, f3 &rp, f3 &rm) const {
        uint32_t tt; f2 tw;
        rp = eval_reflectance(sv, bp, si.uv, tt, tw); rm = eval_reflectance(sv, bm, si.uv, tt, tw);
    }
    // d(value)/d(theta) of the model at fixed directions
    MTS_DEV f3 dvalue(const SceneView &sv, const SurfaceInteraction &si, f3 wo_l) const {
        f3 rp, rm, vp, vm; float pp, pm;
        perturbed_refl(sv, si, rp, rm);
        bsdf_eval_pdf(bp, rp, si.wi, wo_l, vp, pp);      // the model code itself (two-sided adapter included), no nesting
        bsdf_eval_pdf(bm, rm, si.wi, wo_l, vm, pm);
        return mk3((vp.x - vm.x) * inv_2h, (vp.y - vm.y) * inv_2h, (vp.z - vm.z) * inv_2h);
    }
    template <int DEFER, bool GENERAL, bool NEST> MTS_DEV void begin(const PathState &) { static_assert(GENERAL && DEFER == 0 && !NEST, "the parameter gradient rides on the general fused step"); }
    MTS_DEV void emitted(float ew, int32_t, f3 le) { dres = mk3(dres.x + (ew * dthr.x) * le.x, dres.y + (ew * dthr.y) * le.y, dres.z + (ew * dthr.z) * le.z); }
    MTS_DEV void escaped(const SceneView &, const PathState &, const DevEmitter &, float ew, f3 le) { emitted(ew, -1, le); }
    MTS_DEV void roulette(f3, float, float rq, bool) { dthr = dthr * rq; }
    MTS_DEV void surface(const SurfaceInteraction &si, const DevBsdf &, f3, uint32_t, f2, f3) { here = si.shape_rec.bsdf == bsdf; }
    MTS_DEV bool emitter_sample(const SceneView &, const DevBsdf &, f3, const NeeTerms &) { return here; }
    MTS_DEV void unoccluded(const SceneView &sv, const SurfaceInteraction &si, f3 thr, const NeeTerms &t) {      // d(mis thr bv spec) with mis and spec fixed
        f3 dbv = mk3(0.0f, 0.0f, 0.0f);
        if (here) dbv = dvalue(sv, si, t.wo);
        dres = mk3(dres.x + (t.mis * fmaf(dthr.x, t.bv.x, thr.x * dbv.x)) * t.spec.x,
                   dres.y + (t.mis * fmaf(dthr.y, t.bv.y, thr.y * dbv.y)) * t.spec.y,
                   dres.z + (t.mis * fmaf(dthr.z, t.bv.z, thr.z * dbv.z)) * t.spec.z);
    }
    // d(thr weight) = dthr weight + thr dweight;  dweight = d(value)/d(theta) / pdf at the sampled direction
    MTS_DEV void bsdf_sampled(const SceneView &sv, const SurfaceInteraction &si, const DevBsdf &, f3, f3 thr, const BsdfSample &bs, f3 weight, float s1, f2 s2) {
        f3 dw = mk3(0.0f, 0.0f, 0.0f);
        if (here && !bs.delta && bs.pdf > 0.0f) {
            const f3 dv = dvalue(sv, si, bs.wo);
            const float ip = rcp(bs.pdf);
            dw = mk3(dv.x * ip, dv.y * ip, dv.z * ip);
        } else if (here && bs.delta) {
            // a discrete lobe: its weight is a closed form of the parameters (Fresnel term x specular colour / lobe probability);
            // the same lobe is re-evaluated with the perturbed records and the same random numbers, and counts only if both land on
            // the very direction of the primal sample (a refracted direction moves with the index of refraction: detached -> no term)
            f3 rp, rm, wp, wm; BsdfSample bp_, bm_;
            perturbed_refl(sv, si, rp, rm);
            const bool okp = bsdf_sample(bp, rp, si.wi, s1, s2, bp_, wp);
            const bool okm = bsdf_sample(bm, rm, si.wi, s1, s2, bm_, wm);
            if (okp && okm && bp_.delta && bm_.delta && bp_.wo.x == bs.wo.x && bp_.wo.y == bs.wo.y && bp_.wo.z == bs.wo.z &&
                bm_.wo.x == bs.wo.x && bm_.wo.y == bs.wo.y && bm_.wo.z == bs.wo.z)
                dw = mk3((wp.x - wm.x) * inv_2h, (wp.y - wm.y) * inv_2h, (wp.z - wm.z) * inv_2h);
        }
        dthr = mk3(fmaf(dthr.x, weight.x, thr.x * dw.x), fmaf(dthr.y, weight.y, thr.y * dw.y), fmaf(dthr.z, weight.z, thr.z * dw.z));
    }
};

// Every camera sample is replayed through the general fused step with the dual part of ParamGradProbe; its contribution
// delta . d(radiance)/d(theta) is summed over the workgroup and added to A.grad_param[0].
template <bool FLAT>
__global__ __launch_bounds__(kBlock) void k_adjoint_param(const AdjointParams A) {
    extern __shared__ float4 smem[];
    __shared__ float s_sum[kBlock / 64];
    const RenderParams &P = A.rp;
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    float acc = 0.0f;
    for (uint64_t k = (uint64_t) blockIdx.x * kBlock + threadIdx.x; k < A.n_samples; k += (uint64_t) gridDim.x * kBlock) {
        PathState s; const f3 delta = adjoint_sample(A, k, s);
        ParamGradProbe pg = { A.pg_bsdf, A.pg_plus, A.pg_minus, A.pg_inv_2h, mk3(0.0f, 0.0f, 0.0f), mk3(0.0f, 0.0f, 0.0f), false };
        Counters c = { 0u, 0u, 0u, 0u };
        while (bounce_step<FLAT, 0, true>(P, lds, s, c, pg)) { }
        const float g = fmaf(delta.z, pg.dres.z, fmaf(delta.y, pg.dres.y, delta.x * pg.dres.x));
        if (isfinite(g)) acc += g;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane_id() == 0u) s_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float tot = 0.0f;
        for (uint32_t w = 0; w < kBlock / 64; ++w) tot += s_sum[w];
        if (tot != 0.0f) atomicAdd(A.grad_param, tot);
    }
}

hipError_t launch_adjoint_param(const AdjointParams &a, hipStream_t s) { return launch_adjoint_kernel<k_adjoint_param<true>, k_adjoint_param<false>>(a, s); }

// Derivative w.r.t. the texels of bitmap reflectances (diffuse.reflectance, (rough)plastic.diffuse_reflectance) in ANY RGB scene: the
// sweep of k_adjoint over the records of the general step (VertexRecG).  With a = dLoss/dT_{v+1} and delta = dLoss/dRadiance,
//   dL/drho_v = delta * T'_v * dNc_v + a * T'_v * dW_v,     b_v = delta * Nc_v + W_v * a,
//   dL/dT_v   = delta * E_v + invq_v * b_v  -  [q not clamped] invq_v^2 eta_v^2 (b_v . T_v) on the channel that sets q.
// On a diffuse scene (W = rho, Nc = rho * dNc, dW = 1) this is k_adjoint's arithmetic.
//
// What k_adjoint_tex remembers about one vertex of a path through the general step (any BSDF model, any emitter).  With T the
// throughput arriving at the vertex and T' = T * invq after Russian roulette (q = min(hmax(T) eta^2, .95)):
//   radiance += T * E + T' * Nc;  T_next = T' * W,
// E = emission collected (MIS weight included), Nc = mis * bv * spec of the emitter sample, W = the BSDF-sample weight, and dNc / dW
// their derivatives with respect to the textured reflectance at the vertex (diagonal per channel; zero unless `texel` is valid).
struct VertexRecG {
    f3 T; float invq;
    f3 E; float eta2;               // eta^2 of the path at the vertex (the factor of q)
    f3 Nc; int32_t rr_channel;      // channel that sets q (-1: none / q clamped)
    f3 W; uint32_t texel;           // bilinear footprint of the texture lookup (kNoPrim: constant or procedural reflectance)
    f3 dNc; int32_t texture;
    f3 dW; f2 w1;
};

// Fills the VertexRecG of one general step.  Derivatives with respect to the textured reflectance are taken only where a bitmap was
// looked up (`tex`); mis, spec, the pdf and the lobe choice do not depend on the reflectance (detached).
struct GeneralRecorder {
    static constexpr bool kFactoredEmitter = false, kMirrorTwoSided = false, kSamples = true;
    VertexRecG &r;
    bool tex; f3 nc, dnc;           // Nc and dNc / d(refl) of the emitter sample, recorded once it is known to be unoccluded
    template <int DEFER, bool GENERAL, bool NEST> MTS_DEV void begin(const PathState &s) {
        static_assert(GENERAL && DEFER == 0 && !NEST, "the general adjoint replay runs the plain fused step");
        r.T = s.thr; r.invq = 1.0f; r.eta2 = s.eta * s.eta; r.rr_channel = -1;
        r.E = r.Nc = r.W = r.dNc = r.dW = mk3(0.0f, 0.0f, 0.0f);
        r.texel = kNoPrim; r.texture = -1; r.w1.x = r.w1.y = 0.0f;
    }
    MTS_DEV void emitted(float ew, int32_t, f3 le) { r.E = mk3(ew * le.x, ew * le.y, ew * le.z); }
    MTS_DEV void escaped(const SceneView &, const PathState &, const DevEmitter &, float ew, f3 le) { emitted(ew, -1, le); }
    MTS_DEV void roulette(f3 thr, float hm, float rq, bool free) { r.invq = rq; if (free) r.rr_channel = thr.x == hm ? 0 : (thr.y == hm ? 1 : 2); }
    MTS_DEV void surface(const SurfaceInteraction &, const DevBsdf &bsdf, f3, uint32_t texel, f2 tw1, f3) {
        tex = texel != kNoPrim;
        r.texel = texel; r.w1 = tw1; r.texture = bsdf.texture;
    }
    MTS_DEV bool emitter_sample(const SceneView &, const DevBsdf &bsdf, f3 refl, const NeeTerms &t) {
        nc = mk3((t.mis * t.bv.x) * t.spec.x, (t.mis * t.bv.y) * t.spec.y, (t.mis * t.bv.z) * t.spec.z);
        dnc = mk3(0.0f, 0.0f, 0.0f);
        if (tex) {
            const f3 dbv = bsdf_dvalue_drefl(bsdf, refl, t.wi, t.wo);
            dnc = mk3((t.mis * dbv.x) * t.spec.x, (t.mis * dbv.y) * t.spec.y, (t.mis * dbv.z) * t.spec.z);
        }
        return nc.x != 0.0f || nc.y != 0.0f || nc.z != 0.0f || dnc.x != 0.0f || dnc.y != 0.0f || dnc.z != 0.0f;
    }
    MTS_DEV void unoccluded(const SceneView &, const SurfaceInteraction &, f3, const NeeTerms &) { r.Nc = nc; r.dNc = dnc; }
    // T_next = T' * W; dW / d(refl) at the sampled direction
    MTS_DEV void bsdf_sampled(const SceneView &, const SurfaceInteraction &si, const DevBsdf &bsdf, f3 refl, f3, const BsdfSample &bs, f3 weight, float, f2) {
        r.W = weight;
        if (tex) r.dW = bsdf_dweight_drefl(bsdf, refl, si.wi, bs);
    }
};

template <bool FLAT>
__global__ __launch_bounds__(kBlock) void k_adjoint_tex(const AdjointParams A) {
    extern __shared__ float4 smem[];
    const RenderParams &P = A.rp;
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    for (uint64_t k = (uint64_t) blockIdx.x * kBlock + threadIdx.x; k < A.n_samples; k += (uint64_t) gridDim.x * kBlock) {
        PathState s; const f3 delta = adjoint_sample(A, k, s);
        if (delta.x == 0.0f && delta.y == 0.0f && delta.z == 0.0f) continue;       // every term below is proportional to delta
        VertexRecG rec[kAdjointMaxDepth];
        int n = 0;
        Counters c = { 0u, 0u, 0u, 0u };
        bool alive = true;
        while (alive && n < kAdjointMaxDepth) { alive = bounce_step<FLAT, 0, true>(P, lds, s, c, GeneralRecorder{ rec[n] }); ++n; }
        f3 a = mk3(0.0f, 0.0f, 0.0f);
        for (int v = n - 1; v >= 0; --v) {
            const VertexRecG &r = rec[v];
            if (r.texel != kNoPrim) {
                const f3 Tp = r.T * r.invq;
                const float gg[3] = { Tp.x * fmaf(delta.x, r.dNc.x, a.x * r.dW.x), Tp.y * fmaf(delta.y, r.dNc.y, a.y * r.dW.y),
                                      Tp.z * fmaf(delta.z, r.dNc.z, a.z * r.dW.z) };
                const DevTexture t = P.sv.textures[r.texture];
                scatter_texel_grad(A.grad_tex, t, r.texel, r.w1, gg);
            }
            const f3 b = mk3(fmaf(delta.x, r.Nc.x, r.W.x * a.x), fmaf(delta.y, r.Nc.y, r.W.y * a.y), fmaf(delta.z, r.Nc.z, r.W.z * a.z));
            a = mk3(delta.x * r.E.x + r.invq * b.x, delta.y * r.E.y + r.invq * b.y, delta.z * r.E.z + r.invq * b.z);
            if (r.rr_channel >= 0) {
                const float corr = ((r.invq * r.invq) * r.eta2) * (b.x * r.T.x + b.y * r.T.y + b.z * r.T.z);
                if (r.rr_channel == 0) a.x -= corr; else if (r.rr_channel == 1) a.y -= corr; else a.z -= corr;
            }
        }
    }
}

hipError_t launch_adjoint_tex(const AdjointParams &a, hipStream_t s) { return launch_adjoint_kernel<k_adjoint_tex<true>, k_adjoint_tex<false>>(a, s); }


// ---------------------------------------------------------------------------------------------
// Spectral variant: derivative w.r.t. the reflectance family -- diffuse.reflectance and (rough)plastic.diffuse_reflectance, as a constant
// srgb colour or as bitmap texels -- in ANY spectral scene.  One thread replays one camera sample through the general spectral step with
// the PCG32 stream of the primal pass, records its vertices and sweeps them backwards on the four wavelengths, as k_adjoint_tex does on
// three channels:   g_refl_v = T'_v (delta dNc_v + a dW_v),   b_v = delta Nc_v + W_v a,   dL/dT_v = delta E_v + invq_v b_v.
// ALL sampling is detached: directions, pdfs, lobe choices, MIS weights, the plastic lobe weight kr AND the roulette probability q are
// held fixed (only invq is recorded; there is no rr_channel term).  k_adjoint and k_adjoint_tex follow Enoki's attached roulette
// instead; any fixed q keeps the estimator unbiased, so the detached form estimates the true derivative of the image -- what central
// differences of the rendered image estimate too, and what tests/test_gpu_adjoint_spectral.py checks statistically.
// The film channels of the spectral variant are X, Y, Z (store_result_spectral), so the sweep is seeded per wavelength with
//   delta_k = wavelength_weight(l_k) / 4 * (xbar(l_k) dX + ybar(l_k) dY + zbar(l_k) dZ).
// The reflectance spectrum is S(x) = 1/2 + x / (2 sqrt(1 + x^2)), x = c0 l^2 + c1 l + c2 (srgb_model_eval): g_refl goes on to the model
// coefficients with dS/dc = (1 + x^2)^(-3/2) / 2 * (l^2, l, 1) and k_coeff_grad_to_rgb takes the coefficient gradients to RGB.
struct VertexRecS {
    Spec4 T, E, Nc, W, dNc, dW;     // as VertexRecG, per wavelength
    float invq; uint32_t texel; f2 w1;
    int32_t bsdf;                   // record whose reflectance is differentiated at this vertex (-1: none)
};

struct SpectralRecorder {
    VertexRecS &r;
    bool diff; Spec4 nc, dnc;       // Nc and dNc / d(refl) of the emitter sample, recorded once it is known to be unoccluded
    template <int DEFER, bool GENERAL, bool NEST> MTS_DEV void begin(const PathStateS &s) {
        static_assert(GENERAL && DEFER == 0 && !NEST, "the spectral adjoint replay runs the plain general fused step");
        r.T = s.thr; r.invq = 1.0f; r.texel = kNoPrim; r.w1.x = r.w1.y = 0.0f; r.bsdf = -1;
#pragma unroll
        for (int k = 0; k < kWav; ++k) r.E.v[k] = r.Nc.v[k] = r.W.v[k] = r.dNc.v[k] = r.dW.v[k] = 0.0f;
    }
    MTS_DEV void emitted(float ew, int32_t, const Spec4 &le) {
#pragma unroll
        for (int k = 0; k < kWav; ++k) r.E.v[k] = ew * le.v[k];
    }
    MTS_DEV void escaped(const SceneView &, const PathStateS &, const DevEmitter &, float ew, const Spec4 &le) { emitted(ew, -1, le); }
    MTS_DEV void roulette(const Spec4 &, float, float rq, bool) { r.invq = rq; }
    // an srgb colour or a bitmap of the reflectance family (uniform spectra and checkerboards have no RGB parameter here)
    MTS_DEV void surface(const SurfaceInteraction &si, const DevBsdf &bsdf, const Spec4 &, uint32_t texel, f2 tw1, const Spec4 &) {
        diff = (bsdf.type == kBsdfDiffuse || bsdf.type == kBsdfPlastic || bsdf.type == kBsdfRoughPlastic) && !(bsdf.flags & kBsdfUniformRefl) &&
               (bsdf.texture < 0 || texel != kNoPrim);
        r.texel = texel; r.w1 = tw1; r.bsdf = diff ? si.shape_rec.bsdf : -1;
    }
    MTS_DEV bool emitter_sample(const SceneView &, const DevBsdf &bsdf, const Spec4 &refl, const NeeTermsS &t) {
        float dbv[kWav];
        bsdf_dvalue_drefl_n<kWav>(bsdf, refl.v, t.wi, t.wo, dbv);
        bool any = false;
#pragma unroll
        for (int k = 0; k < kWav; ++k) {
            nc.v[k] = (t.mis * t.bv.v[k]) * t.spec.v[k];
            dnc.v[k] = diff ? (t.mis * dbv[k]) * t.spec.v[k] : 0.0f;
            any = any || nc.v[k] != 0.0f || dnc.v[k] != 0.0f;
        }
        return any;
    }
    MTS_DEV void unoccluded(const SceneView &, const SurfaceInteraction &, const Spec4 &, const NeeTermsS &) { r.Nc = nc; r.dNc = dnc; }
    MTS_DEV void bsdf_sampled(const SceneView &, const SurfaceInteraction &si, const DevBsdf &bsdf, const Spec4 &refl, const Spec4 &, const BsdfSample &bs,
                              const float (&weight)[kWav]) {
#pragma unroll
        for (int k = 0; k < kWav; ++k) r.W.v[k] = weight[k];
        if (diff) bsdf_dweight_drefl_n<kWav>(bsdf, refl.v, si.wi, bs, r.dW.v);
    }
};

// acc += sum_k g[k] dS/dc(c, l_k): zero for the black / white sentinels (c2 = -+inf) and where srgb_model_eval clamps at 0.
// The sums are kept in the basis (u^2, u, 1) of the centred wavelength u = (l - kCoeffMid) / kCoeffHalf in [-1, 1], i.e. as the gradient
// w.r.t. (a, b, c) of x = a u^2 + b u + c: in (l^2, l, 1) with l in nanometres the three float32 sums cancel tenfold when the Jacobian
// recombines them.  The Jacobians on the device are composed with d(a, b, c) / d(c0, c1, c2) to match (mtsamd_render_adjoint_spectral).
MTS_DEV void model_coeff_grad(const float *c, const Spec4 &wav, const float (&g)[kWav], float (&acc)[3]) {
    const float c0 = c[0], c1 = c[1], c2 = c[2];
    if (isinf(c2)) return;
#pragma unroll
    for (int k = 0; k < kWav; ++k) {
        const float l = wav.v[k];
        const float x = fmaf(fmaf(c0, l, c1), l, c2);
        const float t = 1.0f / sqrtf(fmaf(x, x, 1.0f));
        if (!(fmaf(0.5f * x, t, 0.5f) > 0.0f)) continue;
        const float d = ((0.5f * t) * (t * t)) * g[k], u = (l - kCoeffMid) * (1.0f / kCoeffHalf);
        acc[0] = fmaf(d * u, u, acc[0]); acc[1] = fmaf(d, u, acc[1]); acc[2] += d;
    }
}

template <bool FLAT>
__global__ __launch_bounds__(kBlock) void k_adjoint_spectral(const AdjointParams A) {
    extern __shared__ float4 smem[];
    const RenderParams &P = A.rp;
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    __shared__ float s_grad[3 * 32];                       // per-workgroup coefficient gradients of constant colours
    for (uint32_t i = threadIdx.x; i < 3u * 32u; i += kBlock) s_grad[i] = 0.0f;
    __syncthreads();
    const uint32_t spp = (uint32_t) P.spp;
    for (uint64_t k = (uint64_t) blockIdx.x * kBlock + threadIdx.x; k < A.n_samples; k += (uint64_t) gridDim.x * kBlock) {
        PathStateS s; float2 pos;
        generate_path_spectral(P, k, (uint32_t) (k / spp), (uint32_t) (k % spp), s, &pos);
        const f3 dxyz = adjoint_delta(A, pos);
        if (dxyz.x == 0.0f && dxyz.y == 0.0f && dxyz.z == 0.0f) continue;       // every term below is proportional to delta
        VertexRecS rec[kAdjointMaxDepth];
        int n = 0;
        Counters c = { 0u, 0u, 0u, 0u };
        bool alive = true;
        while (alive && n < kAdjointMaxDepth) { alive = bounce_step_spectral<FLAT, 0, true>(P, lds, s, c, nullptr, SpectralRecorder{ rec[n] }); ++n; }
        // the adjoint of store_result_spectral; a sample the primal pass drops (alpha = -1) contributes nothing
        Spec4 delta, value;
#pragma unroll
        for (int w = 0; w < kWav; ++w) {
            const float l = s.wav.v[w], ww = wavelength_weight(l);
            const f3 cie = cie1931_xyz(l);
            value.v[w] = ww * s.res.v[w];
            delta.v[w] = (ww * 0.25f) * fmaf(cie.z, dxyz.z, fmaf(cie.y, dxyz.y, cie.x * dxyz.x));
        }
        const f3 xyz = spectrum_to_xyz(value, s.wav);
        if (!((xyz.x >= -1e-5f) && (xyz.y >= -1e-5f) && (xyz.z >= -1e-5f) && isfinite(xyz.x) && isfinite(xyz.y) && isfinite(xyz.z))) continue;
        float a[kWav] = { 0.0f, 0.0f, 0.0f, 0.0f };         // dLoss/dT_{v+1}
        for (int v = n - 1; v >= 0; --v) {
            const VertexRecS &r = rec[v];
            if (r.bsdf >= 0) {
                float g[kWav];
#pragma unroll
                for (int w = 0; w < kWav; ++w) g[w] = (r.T.v[w] * r.invq) * fmaf(delta.v[w], r.dNc.v[w], a[w] * r.dW.v[w]);
                const DevBsdf &b = P.sv.bsdfs[r.bsdf];
                if (r.texel != kNoPrim) {
                    if (A.grad_tex) {      // w_ij * sum_k g[k] dS/dc(texel_ij, l_k) for the four corners of the lookup
                        const DevTexture t = P.sv.textures[b.texture];
                        const float wt[4] = { (1.0f - r.w1.y) * (1.0f - r.w1.x), (1.0f - r.w1.y) * r.w1.x, r.w1.y * (1.0f - r.w1.x), r.w1.y * r.w1.x };
                        const uint32_t at[4] = { r.texel, r.texel + 1u, r.texel + (uint32_t) t.w, r.texel + (uint32_t) t.w + 1u };
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            float gc[3] = { 0.0f, 0.0f, 0.0f };
                            model_coeff_grad(t.data + 3u * (size_t) at[i], s.wav, g, gc);
                            float *gt = A.grad_tex + t.grad_offset + 3u * (size_t) at[i];
                            atomicAdd(gt, gc[0] * wt[i]); atomicAdd(gt + 1, gc[1] * wt[i]); atomicAdd(gt + 2, gc[2] * wt[i]);
                        }
                    }
                } else if (A.grad_bsdf && r.bsdf < 32) {
                    float gc[3] = { 0.0f, 0.0f, 0.0f };
                    model_coeff_grad(&b.c0, s.wav, g, gc);
                    atomicAdd(&s_grad[3 * r.bsdf], gc[0]); atomicAdd(&s_grad[3 * r.bsdf + 1], gc[1]); atomicAdd(&s_grad[3 * r.bsdf + 2], gc[2]);
                }
            }
#pragma unroll
            for (int w = 0; w < kWav; ++w) {
                const float bw = fmaf(delta.v[w], r.Nc.v[w], r.W.v[w] * a[w]);
                a[w] = fmaf(delta.v[w], r.E.v[w], r.invq * bw);
            }
        }
    }
    __syncthreads();
    if (A.grad_bsdf)
        for (uint32_t i = threadIdx.x; i < 3u * min(P.sv.n_bsdfs, 32u); i += kBlock)
            if (s_grad[i] != 0.0f) atomicAdd(A.grad_bsdf + i, s_grad[i]);
}

hipError_t launch_adjoint_spectral(const AdjointParams &a, hipStream_t s) {
    return launch_adjoint_kernel<k_adjoint_spectral<true>, k_adjoint_spectral<false>>(a, s);
}

// out[i] += J_i^T cgrad[i]: the gradient w.r.t. the model coefficients of colour i (a BSDF record or a texel) taken to its RGB value
// through jac[9 i + 3 c + j] = d coeff_j / d rgb_c (srgb_model_fetch_jacobian), both in the centred basis of model_coeff_grad
__global__ __launch_bounds__(kBlock) void k_coeff_grad_to_rgb(const float *cgrad, const float *jac, float *out, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float g0 = cgrad[3u * i], g1 = cgrad[3u * i + 1u], g2 = cgrad[3u * i + 2u];
    if (g0 == 0.0f && g1 == 0.0f && g2 == 0.0f) return;
    const float *j = jac + 9u * (size_t) i;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3u * i + c] += fmaf(j[3 * c + 2], g2, fmaf(j[3 * c + 1], g1, j[3 * c] * g0));
}
hipError_t launch_coeff_grad_to_rgb(const float *cgrad, const float *jac, float *out, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_coeff_grad_to_rgb, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, cgrad, jac, out, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Spectral variant: derivative w.r.t. the emitter family -- the texels of an `envmap` ('data', envmap.cpp:214-218) and the radiance /
// intensity / irradiance of area, `constant`, `point`, `spot` and `directional` emitters -- in ANY spectral scene.  Such a colour is stored
// as (model coefficients c of n = rgb / sc, scale sc = 2 max(r, g, b)), and the radiance at wavelength l is
//   envmap:  sp(l) * f * wp(l) * scale,  sp = sum_i w_i S(c_i; l),  f = sum_i w_i sc_i over the four bilinear corners, wp = D65 / 10568;
//   others:  S(c; l) * sc * wp(l)        (d65_scale = sc / 10568): the one-texel case with w = 1 and scale = 1.
// Throughput, directions, pdfs, MIS weights and roulette do not depend on the emitted spectrum, and the sampling hierarchy built from the
// luminances is not differentiated (as in k_adjoint_env), so there is no backward sweep: the radiance enters at the emission a path picks
// up (coefficient ew * thr) and at an unoccluded emitter sample (coefficient mis * thr * bv * (spec / radiance), from the factors r1, r2
// and falloff: spec is never divided by the radiance, which may be 0).  Whether the primal pass drops a sample is known only at the end
// of its path, so one thread replays one camera sample, records at most two uses per step, and scatters them after that test.  With
// A_k = coefficient * delta_k (the per-wavelength seed of k_adjoint_spectral) and B_k = A_k wp_k scale, a use adds
//   gc_i += w_i f sum_k B_k dS/dc(c_i; l_k)   (centred basis of model_coeff_grad),      gs_i += w_i sum_k B_k sp_k
// into the 4-float row (gc, gs) of each colour it read: texel rows by float atomics in global memory, emitter rows reduced in LDS per
// workgroup first.  k_emitter_grad_to_rgb takes the rows to RGB.  A colour whose largest component is 0 has the sentinel coefficients:
// model_coeff_grad skips it, and its row of the Jacobian table is zero, so its gradient is exactly 0 and it puts no NaN into its neighbours.
struct EmitterUseS {
    Spec4 ce, cn;               // coefficients of the emission picked up at this step and of its emitter sample
    f2 uve, uvn;                // envmap texture coordinates of the two
    int32_t eme, emn;           // their emitters (-1: none)
};

struct EmitterGradProbeS {
    EmitterUseS &r;
    Spec4 thr0;                 // throughput arriving at the vertex (emission is picked up before roulette)
    template <int DEFER, bool GENERAL, bool NEST> MTS_DEV void begin(const PathStateS &s) {
        static_assert(GENERAL && DEFER == 0 && !NEST, "the spectral emitter gradient rides on the plain general fused step");
        thr0 = s.thr; r.eme = r.emn = -1; r.uve.x = r.uve.y = r.uvn.x = r.uvn.y = 0.0f;
#pragma unroll
        for (int k = 0; k < kWav; ++k) r.ce.v[k] = r.cn.v[k] = 0.0f;
    }
    MTS_DEV void emitted(float ew, int32_t emitter, const Spec4 &) {
        r.eme = emitter;
#pragma unroll
        for (int k = 0; k < kWav; ++k) r.ce.v[k] = ew * thr0.v[k];
    }
    MTS_DEV void escaped(const SceneView &sv, const PathStateS &s, const DevEmitter &e, float ew, const Spec4 &) {
        emitted(ew, sv.env_emitter, s.thr);
        if (e.pad0 == kEmitterEnvmap) env_dir_to_uv(mat3_apply(sv.envmap->to_local, s.d), r.uve.x, r.uve.y);
    }
    MTS_DEV void roulette(const Spec4 &, float, float, bool) { }
    MTS_DEV void surface(const SurfaceInteraction &, const DevBsdf &, const Spec4 &, uint32_t, f2, const Spec4 &) { }
    // spec / radiance of the emitter sample
    MTS_DEV static float em_geo(const SceneView &sv, const NeeTermsS &t) {
        const float g = t.ds.delta ? t.ds.falloff * t.r1 : t.r1;
        return sv.n_emitters > 1u ? g * t.r2 : g;
    }
    // the shadow ray is traced whenever the derivative is non-zero, also where the radiance itself is 0
    MTS_DEV bool emitter_sample(const SceneView &sv, const DevBsdf &, const Spec4 &, const NeeTermsS &t) {
        bool any = false;
#pragma unroll
        for (int k = 0; k < kWav; ++k) any = any || t.bv.v[k] != 0.0f;
        return any && em_geo(sv, t) != 0.0f;
    }
    MTS_DEV void unoccluded(const SceneView &sv, const SurfaceInteraction &, const Spec4 &thr, const NeeTermsS &t) {
        const float g = em_geo(sv, t);
        r.emn = (int32_t) t.ds.emitter; r.uvn = t.ds.uv;
#pragma unroll
        for (int k = 0; k < kWav; ++k) r.cn.v[k] = ((t.mis * thr.v[k]) * t.bv.v[k]) * g;
    }
    MTS_DEV void bsdf_sampled(const SceneView &, const SurfaceInteraction &, const DevBsdf &, const Spec4 &, const Spec4 &, const BsdfSample &, const float (&)[kWav]) { }
};

// One use of emitter `em` with the per-wavelength coefficients `a` = coefficient * delta: into the texel rows of grad_env (an `envmap`)
// or into row `em` of the workgroup's s_em (every other emitter).  Either destination may be null.
MTS_DEV void scatter_emitter_use(const SceneView &sv, const Spec4 &wav, int32_t em, f2 uv, const Spec4 &a, float *grad_env, float *s_em) {
    if (em < 0) return;
    bool any = false;
    float bk[kWav];
#pragma unroll
    for (int k = 0; k < kWav; ++k) { bk[k] = a.v[k] * table_eval(g_spectral.d65, 1.0f / 10568.0f, wav.v[k]); any = any || bk[k] != 0.0f; }
    if (!any) return;
    const DevEmitter &e = sv.emitters[em];
    if (e.pad0 == kEmitterEnvmap) {
        if (!grad_env) return;
        const DevEnvmap &env = *sv.envmap;
        const float u = uv.x * (float) (env.w - 1), v = uv.y * (float) (env.h - 1);        // the bilinear footprint of envmap_lookup_spectral
        const uint32_t px = min((uint32_t) u, (uint32_t) (env.w - 2)), py = min((uint32_t) v, (uint32_t) (env.h - 2));
        const float w1x = u - (float) px, w1y = v - (float) py, w0x = 1.0f - w1x, w0y = 1.0f - w1y;
        const float wt[4] = { w0y * w0x, w0y * w1x, w1y * w0x, w1y * w1x };
        const uint32_t at[4] = { py * (uint32_t) env.w + px, py * (uint32_t) env.w + px + 1u, (py + 1u) * (uint32_t) env.w + px, (py + 1u) * (uint32_t) env.w + px + 1u };
        float4 tx[4];
        float f = 0.0f, gsum = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { tx[i] = env.data[at[i]]; f = fmaf(wt[i], tx[i].w, f); }
#pragma unroll
        for (int k = 0; k < kWav; ++k) {
            bk[k] *= env.scale;
            float sp = 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i) sp = fmaf(wt[i], srgb_model_eval(tx[i].x, tx[i].y, tx[i].z, wav.v[k]), sp);
            gsum = fmaf(bk[k], sp, gsum);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (wt[i] == 0.0f) continue;
            const float c[3] = { tx[i].x, tx[i].y, tx[i].z };
            const float g[kWav] = { bk[0] * (wt[i] * f), bk[1] * (wt[i] * f), bk[2] * (wt[i] * f), bk[3] * (wt[i] * f) };
            float gc[3] = { 0.0f, 0.0f, 0.0f };
            model_coeff_grad(c, wav, g, gc);
            float *row = grad_env + 4u * (size_t) at[i];
            atomicAdd(row, gc[0]); atomicAdd(row + 1, gc[1]); atomicAdd(row + 2, gc[2]); atomicAdd(row + 3, wt[i] * gsum);
        }
    } else if (s_em && em < 32) {
        const float c[3] = { e.c0, e.c1, e.c2 };
        const float f = e.d65_scale * 10568.0f;              // sc
        float g[kWav], gsum = 0.0f;
#pragma unroll
        for (int k = 0; k < kWav; ++k) { g[k] = bk[k] * f; gsum = fmaf(bk[k], srgb_model_eval(c[0], c[1], c[2], wav.v[k]), gsum); }
        float gc[3] = { 0.0f, 0.0f, 0.0f };
        model_coeff_grad(c, wav, g, gc);
        atomicAdd(&s_em[4 * em], gc[0]); atomicAdd(&s_em[4 * em + 1], gc[1]); atomicAdd(&s_em[4 * em + 2], gc[2]); atomicAdd(&s_em[4 * em + 3], gsum);
    }
}

// A.grad_emitter (n_emitters rows) and A.grad_env (height * width rows) are the 4-float (gc, gs) scratch rows here; either may be null
template <bool FLAT>
__global__ __launch_bounds__(kBlock) void k_adjoint_spectral_emitters(const AdjointParams A) {
    extern __shared__ float4 smem[];
    const RenderParams &P = A.rp;
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    __shared__ float s_em[4 * 32];                         // per-workgroup (gc, gs) rows of the emitters
    for (uint32_t i = threadIdx.x; i < 4u * 32u; i += kBlock) s_em[i] = 0.0f;
    __syncthreads();
    const uint32_t spp = (uint32_t) P.spp;
    for (uint64_t k = (uint64_t) blockIdx.x * kBlock + threadIdx.x; k < A.n_samples; k += (uint64_t) gridDim.x * kBlock) {
        PathStateS s; float2 pos;
        generate_path_spectral(P, k, (uint32_t) (k / spp), (uint32_t) (k % spp), s, &pos);
        const f3 dxyz = adjoint_delta(A, pos);
        if (dxyz.x == 0.0f && dxyz.y == 0.0f && dxyz.z == 0.0f) continue;       // every term below is proportional to delta
        EmitterUseS use[kAdjointMaxDepth];
        int n = 0;
        Counters c = { 0u, 0u, 0u, 0u };
        bool alive = true;
        while (alive && n < kAdjointMaxDepth) { alive = bounce_step_spectral<FLAT, 0, true>(P, lds, s, c, nullptr, EmitterGradProbeS{ use[n] }); ++n; }
        // the adjoint of store_result_spectral; a sample the primal pass drops (alpha = -1) contributes nothing
        Spec4 delta, value;
#pragma unroll
        for (int w = 0; w < kWav; ++w) {
            const float l = s.wav.v[w], ww = wavelength_weight(l);
            const f3 cie = cie1931_xyz(l);
            value.v[w] = ww * s.res.v[w];
            delta.v[w] = (ww * 0.25f) * fmaf(cie.z, dxyz.z, fmaf(cie.y, dxyz.y, cie.x * dxyz.x));
        }
        const f3 xyz = spectrum_to_xyz(value, s.wav);
        if (!((xyz.x >= -1e-5f) && (xyz.y >= -1e-5f) && (xyz.z >= -1e-5f) && isfinite(xyz.x) && isfinite(xyz.y) && isfinite(xyz.z))) continue;
        for (int v = 0; v < n; ++v) {
            const EmitterUseS &r = use[v];
            Spec4 ae, an;
#pragma unroll
            for (int w = 0; w < kWav; ++w) { ae.v[w] = r.ce.v[w] * delta.v[w]; an.v[w] = r.cn.v[w] * delta.v[w]; }
            scatter_emitter_use(P.sv, s.wav, r.eme, r.uve, ae, A.grad_env, A.grad_emitter ? s_em : nullptr);
            scatter_emitter_use(P.sv, s.wav, r.emn, r.uvn, an, A.grad_env, A.grad_emitter ? s_em : nullptr);
        }
    }
    __syncthreads();
    if (A.grad_emitter)
        for (uint32_t i = threadIdx.x; i < 4u * min(P.sv.n_emitters, 32u); i += kBlock)
            if (s_em[i] != 0.0f) atomicAdd(A.grad_emitter + i, s_em[i]);
}

hipError_t launch_adjoint_spectral_emitters(const AdjointParams &a, hipStream_t s) {
    return launch_adjoint_kernel<k_adjoint_spectral_emitters<true>, k_adjoint_spectral_emitters<false>>(a, s);
}

// out[i] += Jn_i^T gc_i + sel_i gs_i for n emitter colours: rows[4 i] = (gc, gs) of colour i, jac[12 i + 3 ch + j] = d coeff_j / d rgb_ch
// (centred basis) and jac[12 i + 9 + ch] = d scale / d rgb_ch (2 for the channel that attains the maximum, 0 otherwise; all 0 for black)
__global__ __launch_bounds__(kBlock) void k_emitter_grad_to_rgb(const float *rows, const float *jac, float *out, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float g0 = rows[4u * i], g1 = rows[4u * i + 1u], g2 = rows[4u * i + 2u], gs = rows[4u * i + 3u];
    if (g0 == 0.0f && g1 == 0.0f && g2 == 0.0f && gs == 0.0f) return;
    const float *j = jac + 12u * (size_t) i;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3u * i + c] += fmaf(j[9 + c], gs, fmaf(j[3 * c + 2], g2, fmaf(j[3 * c + 1], g1, j[3 * c] * g0)));
}
hipError_t launch_emitter_grad_to_rgb(const float *rows, const float *jac, float *out, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_emitter_grad_to_rgb, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, rows, jac, out, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// ImageBlock::put as a gather: one wave per film pixel, lanes stride over the samples of the
// (2R+1)^2 neighbouring pixels, fixed-order butterfly reduction -> bitwise reproducible film.
// weight of the sample at block-relative position `pos` for block pixel `t` along one axis
// (imageblock.cpp:117-161); `size` = block extent incl. border
MTS_DEV float axis_weight(const FilterView &f, float pos, int t, int size) {
    if (f.radius > 1.0f) {
        int lo = max((int) ceilf(pos - f.radius), 0);
        int hi = min((int) floorf(pos + f.radius), size - 1);
        int i = t - lo;
        if (i < 0 || i >= f.taps || t > hi) return 0.0f;
        float base = (float) (uint32_t) lo - pos;
        return filter_weight(f, base + (float) i);
    } else {
        int lo = (int) ceilf(pos - 0.5f);
        return (lo == t && lo >= 0 && lo < size) ? 1.0f : 0.0f;
    }
}

__global__ __launch_bounds__(kBlock) void k_film_gather(const FilmParams F) {
    const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint32_t lane = lane_id();
    const uint32_t n_rows = (uint32_t) (F.row1 - F.row0);
    if (wave >= n_rows * (uint32_t) F.crop_w) return;
    const int x = (int) (wave % (uint32_t) F.crop_w), y = F.row0 + (int) (wave / (uint32_t) F.crop_w);
    const FilterView &f = F.filter;
    const int b = f.border;
    const int R = (int) ceilf(f.radius);
    const int sx = F.crop_w + 2 * b, sy = F.crop_h + 2 * b;
    // block offset = crop offset, with border: pos = pos_ - (offset - border + 0.5)
    const float offx = (float) (F.crop_x - b) + 0.5f, offy = (float) (F.crop_y - b) + 0.5f;
    const uint64_t i0 = F.first_ordinal, i1 = F.first_ordinal + F.n_samples;
    float acc[5] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    for (int qy = y - R; qy <= y + R; ++qy) {
        if (qy < 0 || qy >= F.crop_h) continue;
        const int lr = row_to_local(F.rows, qy);
        if (lr < 0) continue;
        for (int qx = x - R; qx <= x + R; ++qx) {
            if (qx < 0 || qx >= F.crop_w) continue;
            uint64_t q = (uint64_t) lr * (uint64_t) F.crop_w + (uint64_t) qx;
            uint64_t s_lo = q * (uint64_t) F.spp, s_hi = s_lo + (uint64_t) F.spp;
            if (s_lo < i0) s_lo = i0;
            if (s_hi > i1) s_hi = i1;
            for (uint64_t sidx = s_lo + lane; sidx < s_hi; sidx += 64u) {
                const float4 val = F.out_rgba[sidx - i0];    // (X, Y, Z, alpha), alpha < 0: invalid sample
                if (val.w < 0.0f) continue;
                const float2 pp = F.out_pos[sidx - i0];
                float wx = axis_weight(f, pp.x - offx, x + b, sx);
                if (wx == 0.0f) continue;                 // outside the footprint (or a zero tap: adds nothing)
                float wy = axis_weight(f, pp.y - offy, y + b, sy);
                float w = wy * wx;                        // box filter: exactly 1 or 0
                if (w == 0.0f) continue;
                acc[0] += val.x * w; acc[1] += val.y * w; acc[2] += val.z * w; acc[3] += val.w * w; acc[4] += 1.0f * w;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k)
        for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off);
    if (lane == 0) {
        float *dst = F.film + 5u * ((size_t) y * (size_t) F.crop_w + (size_t) x);
#pragma unroll
        for (int k = 0; k < 5; ++k) dst[k] += acc[k];
    }
}

// ---------------------------------------------------------------------------------------------
// ImageBlock::put, tiled by SOURCE pixels.  A workgroup owns a 16x16 block of source pixels (one thread each) of the pass and
// reads every one of their samples exactly once: 8 samples per pixel at a time, i.e. 128 contiguous bytes of radiance and 64 of
// film position -- whole sectors.  Two samples at a time it turns each sample into a record in LDS -- value (X,Y,Z,A) and the
// <= 4 filter taps per axis, exactly as imageblock.cpp:117-147 computes them, stored source-aligned (tap k <-> film pixel
// q - R + k) -- and the threads gather, branch-free and in a fixed order, the (16 + 2R)^2 film pixels the block's samples reach
// (imageblock.cpp:148-161 as a gather).  The (16 + 2R)^2 x 5 sums go to a scratch tile; k_film_merge adds the <= 4 overlapping
// tiles of every film pixel in a fixed order.  No atomics: the film is bitwise reproducible.  HBM traffic: 24 B per sample, once.
constexpr int kFilmTaps = 5;      // taps per axis seen from the source pixel: 2R+1 <= 5 (kFilmTile, kFilmDest, kFilmPartial: kernels.h)

// Filter weights of one sample along one axis for the 2R+1 film pixels q-R .. q+R around its source pixel q
// (block coordinates t = q + border + k - R), exactly as imageblock.cpp:117-147 evaluates them: 0 outside [lo, hi]
// and beyond the n = `taps` entries starting at lo.
MTS_DEV void axis_taps(const FilterView &f, const float *table, float pos, int size, int t0, int R, float w[kFilmTaps]) {
#pragma unroll
    for (int k = 0; k < kFilmTaps; ++k) w[k] = 0.0f;
    if (f.radius > 1.0f) {
        const int lo = max((int) ceilf(pos - f.radius), 0);
        const int hi = min((int) floorf(pos + f.radius), size - 1);
        const float base = (float) (uint32_t) lo - pos;
#pragma unroll
        for (int k = 0; k < kFilmTaps; ++k) {
            const int t = t0 + k, i = t - lo;
            if (k <= 2 * R && i >= 0 && i < f.taps && t <= hi) {
                const float xx = base + (float) i;
                w[k] = f.analytic ? filter_eval(f, xx) : table[min((int) fabsf(xx * f.scale_factor), 31)];
            }
        }
    } else {
        const int lo = (int) ceilf(pos - 0.5f);
        const int k = lo - t0;
        if (lo >= 0 && lo < size && k >= 0 && k <= 2 * R) w[k] = 1.0f;
    }
}

// The same weights for the common case -- a tabulated filter of radius exactly 2 (gaussian, mitchell, catmullrom) and a source pixel
// whose five taps t0 .. t0 + 4 all lie on the film -- without the per-tap window tests: a tap outside [lo, hi] is more than the radius
// away from the sample, (int) (|x| * 31 / 2) is then >= 31 and the table (extended with zeros to 64 entries) returns the 0 the window
// test would have set; x itself is formed exactly as above, (lo - pos) + i with i = k - (lo - t0), so the weights inside the window
// are the same bits.  (|x| < 4 and radius = 2 exactly: the product with the scale factor cannot round across 31.)  Per tap: three
// cheap VALU ops, one convert, one LDS read -- the window tests, selects and clamps above were 45 % of k_film_accum's VALU time.
MTS_DEV void axis_taps_r2(const float *table64, float scale_factor, float pos, float t0f, float w[kFilmTaps]) {
    const float lo = ceilf(pos - 2.0f), base = lo - pos, dk = lo - t0f;      // lo - t0 is 0 or 1
#pragma unroll
    for (int k = 0; k < kFilmTaps; ++k) {
        const float xx = base + ((float) k - dk);
        w[k] = table64[(int) fabsf(xx * scale_factor)];
    }
}

// One thread per source pixel.  The 5 x 5 x 5 partial sums of its own samples -- for every tap (kx, ky) of the pixel's
// neighbourhood the sum over the samples of w_y[ky] w_x[kx] (X, Y, Z, A, 1) -- stay in registers for the whole pass: the main loop
// touches neither LDS (beyond the 32-entry filter table) nor a barrier.  At the end the block exchanges the sums through LDS, one tap
// row at a time, and every film pixel of the (16 + 2R)^2 region adds up the <= 25 source pixels that reach it.
#ifndef MTS_FILM_PREFETCH
#define MTS_FILM_PREFETCH 2
#endif
#ifndef MTS_FILM_NT
#define MTS_FILM_NT 0
#endif
typedef float film_v4 __attribute__((ext_vector_type(4)));
typedef float film_v2 __attribute__((ext_vector_type(2)));
MTS_DEV float4 film_load(const float4 *p) {
#if MTS_FILM_NT
    const film_v4 v = __builtin_nontemporal_load(reinterpret_cast<const film_v4 *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return *p;
#endif
}
MTS_DEV float2 film_load(const float2 *p) {
#if MTS_FILM_NT
    const film_v2 v = __builtin_nontemporal_load(reinterpret_cast<const film_v2 *>(p));
    return make_float2(v.x, v.y);
#else
    return *p;
#endif
}
#define MTS_FILM_LOAD(p) film_load(p)
constexpr int kFilmPrefetch = MTS_FILM_PREFETCH;     // samples in flight per thread (x 24 B)
// DMA (round 3): the stream is staged through LDS by wave-cooperative loads.  Per-lane loads of the pixel-major stream touch one 128-byte
// line per lane and use 16 bytes of it at a time; the rest has to survive in a 32 KB L1 that 512 lanes share until the lane comes back
// for it, and the bytes a thread can keep in flight are bounded by its registers (125 accumulators leave room for two samples).  Now
// eight adjacent lanes fetch the 8 x 16 bytes of one pixel's line (rgba: 8 samples; positions: 4 lanes x 16 bytes) with
// global_load_lds_dwordx4 -- the data lands in LDS without passing through registers, every line is requested once, by one instruction,
// and used whole -- and after a barrier every thread consumes the 8 samples of its own pixel from LDS (rotated start: conflict-free
// ds_read_b128).  Taken when the runs are whole groups of 8 samples; the per-lane loop stays for the rest.
#ifndef MTS_FILM_DMA
#define MTS_FILM_DMA 1
#endif
constexpr int kFilmRound = 8;                        // samples of a pixel per staging round: one 128-byte line of rgba
typedef __attribute__((address_space(3))) void film_lds_void;
typedef __attribute__((address_space(1))) const void film_glb_void;
template <bool DMA>
__global__ __launch_bounds__(kBlock) void k_film_accum(const FilmParams F) {
    __shared__ float table[64];                          // the filter's 32 entries + zeros (axis_taps_r2)
    // staging: rgba [pixel][8] float4 (32 KB) + positions [pixel][8] float2 (16 KB); the exchange buffer E of the epilogue aliases it
    __shared__ float4 stage[DMA ? kBlock * kFilmRound * 3 / 2 : (kFilmTile * kFilmTile * (kFilmTaps * 5 + 1) + 3) / 4];
    float *E = reinterpret_cast<float *>(stage);         // one tap row of every source pixel: [pixel][kx][channel], padded
    static_assert(kBlock * kFilmRound * 3 / 2 * 16 >= kFilmTile * kFilmTile * (kFilmTaps * 5 + 1) * 4, "the exchange buffer fits the staging area");
    const FilterView &f = F.filter;
    const int b = f.border, R = (int) ceilf(f.radius), DW = kFilmTile + 2 * R;
    if (threadIdx.x < 64) table[threadIdx.x] = threadIdx.x < 32 ? f.table[threadIdx.x] : 0.0f;
    const int tcx = (int) (blockIdx.x % (uint32_t) F.tiles_x), tcy = (int) (blockIdx.x / (uint32_t) F.tiles_x);
    const int sp = (int) threadIdx.x, lx = sp % kFilmTile, ly = sp / kFilmTile;
    // this thread's source pixel: column qx, local row lr (the pass holds whole local rows; a tile's rows are contiguous on the film)
    const int qx = tcx * kFilmTile + lx, lr = F.pass_lr0 + tcy * F.tile_h + ly;
    const bool have = qx < F.crop_w && ly < F.tile_h && lr < F.pass_lr0 + F.pass_rows;
    const int qy = have ? row_to_global(F.rows, lr) : 0;
    const int sx = F.crop_w + 2 * b, sy = F.crop_h + 2 * b;
    const float offx = (float) (F.crop_x - b) + 0.5f, offy = (float) (F.crop_y - b) + 0.5f;
    const int tap_x0 = qx + b - R, tap_y0 = qy + b - R;
    // radius-2 table filter, every tap of this pixel on the film: the short form of the weights (axis_taps_r2)
    const bool fast_taps = !f.analytic && f.radius == 2.0f && f.table[31] == 0.0f && tap_x0 >= 0 && tap_x0 + 4 <= sx - 1 && tap_y0 >= 0 && tap_y0 + 4 <= sy - 1;
    const float tap_x0f = (float) tap_x0, tap_y0f = (float) tap_y0;
    const size_t slot0 = have ? (size_t) (((uint64_t) lr * (uint64_t) F.crop_w + (uint64_t) qx) * (uint64_t) F.spp - F.first_ordinal) : 0;
    __syncthreads();
    float acc[kFilmTaps][kFilmTaps][5];
#pragma unroll
    for (int ky = 0; ky < kFilmTaps; ++ky)
#pragma unroll
        for (int kx = 0; kx < kFilmTaps; ++kx)
#pragma unroll
            for (int c = 0; c < 5; ++c) acc[ky][kx][c] = 0.0f;
    float4 pv[kFilmPrefetch]; float2 pq[kFilmPrefetch];
    // blockIdx.y: which run of the pixel's samples (runs start on multiples of 8: whole 128-byte lines)
    const int run = ((F.spp + F.slices - 1) / F.slices + 7) & ~7;
    const int s_begin = min((int) blockIdx.y * run, F.spp), n_spp = have ? min(s_begin + run, F.spp) : s_begin;
    auto accumulate = [&](const float4 rec, const float2 rp) {
        if (!(rec.w >= 0.0f)) return;                        // (X, Y, Z, alpha); alpha < 0: invalid or absent sample
        float wxs[kFilmTaps], wys[kFilmTaps];
        if (fast_taps) {
            axis_taps_r2(table, f.scale_factor, rp.x - offx, tap_x0f, wxs);
            axis_taps_r2(table, f.scale_factor, rp.y - offy, tap_y0f, wys);
        } else {
            axis_taps(f, table, rp.x - offx, sx, tap_x0, R, wxs);
            axis_taps(f, table, rp.y - offy, sy, tap_y0, R, wys);
        }
        // a zero weight adds (signed) zeros, which leaves the sums as they are: the film equals the one of a loop over the non-zero
        // taps only (imageblock.cpp:148-161)
#pragma unroll
        for (int ky = 0; ky < kFilmTaps; ++ky)
#pragma unroll
            for (int kx = 0; kx < kFilmTaps; ++kx) {
                const float w = wys[ky] * wxs[kx];
                acc[ky][kx][0] += rec.x * w; acc[ky][kx][1] += rec.y * w; acc[ky][kx][2] += rec.z * w; acc[ky][kx][3] += rec.w * w;
                acc[ky][kx][4] += 1.0f * w;
            }
    };
    if (DMA) {
        // (host: DMA only if F.spp % 8 == 0, so every run is a whole number of rounds and the stream offsets are 16-byte aligned)
        float4 *s_rgba = stage;
        float2 *s_pos = reinterpret_cast<float2 *>(stage + kBlock * kFilmRound);
        const int wv = sp >> 6, ln = sp & 63;
        const int n_end = min(s_begin + run, F.spp);         // workgroup-uniform
        const int last_lr = F.pass_lr0 + F.pass_rows;
        auto slot_of = [&](int q, bool &ok) -> size_t {      // first stream slot of tile pixel q (any lane computes any pixel's)
            const int qlx = q % kFilmTile, qly = q / kFilmTile;
            const int qqx = tcx * kFilmTile + qlx, qlr = F.pass_lr0 + tcy * F.tile_h + qly;
            ok = qqx < F.crop_w && qly < F.tile_h && qlr < last_lr;
            return ok ? (size_t) (((uint64_t) qlr * (uint64_t) F.crop_w + (uint64_t) qqx) * (uint64_t) F.spp - F.first_ordinal) : 0;
        };
        for (int s0 = s_begin; s0 < n_end; s0 += kFilmRound) {
            // rgba: 8 instructions per wave, lanes 8 g .. 8 g + 7 fetch the line of pixel 64 wv + 8 i + g
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int q = 64 * wv + 8 * i + (ln >> 3);
                bool ok; const size_t q0 = slot_of(q, ok);
                if (ok) __builtin_amdgcn_global_load_lds((film_glb_void *) (F.out_rgba + q0 + (size_t) (s0 + (ln & 7))),
                                                         (film_lds_void *) (s_rgba + (64 * wv + 8 * i) * kFilmRound), 16, 0, 0);
            }
            // positions: 4 instructions per wave, lanes 4 g .. 4 g + 3 fetch the 64 bytes (8 x float2) of pixel 64 wv + 16 i + g
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = 64 * wv + 16 * i + (ln >> 2);
                bool ok; const size_t q0 = slot_of(q, ok);
                if (ok) __builtin_amdgcn_global_load_lds((film_glb_void *) (F.out_pos + q0 + (size_t) (s0 + 2 * (ln & 3))),
                                                         (film_lds_void *) (s_pos + (64 * wv + 16 * i) * kFilmRound), 16, 0, 0);
            }
            __builtin_amdgcn_s_waitcnt(0);                   // vmcnt(0): the wave's DMA has landed
            __syncthreads();
            if (have) {
#pragma unroll 2
                for (int kk = 0; kk < kFilmRound; ++kk) {
                    const int j = (kk + (sp >> 1)) & (kFilmRound - 1);      // rotated start: the 16 lanes of a ds_read_b128 group hit 16 different banks
                    accumulate(s_rgba[sp * kFilmRound + j], s_pos[sp * kFilmRound + j]);
                }
            }
            __syncthreads();
        }
    } else {
#pragma unroll
    for (int k = 0; k < kFilmPrefetch; ++k) {
        pv[k] = make_float4(0.0f, 0.0f, 0.0f, -1.0f); pq[k] = make_float2(0.0f, 0.0f);
        if (s_begin + k < n_spp) { pv[k] = MTS_FILM_LOAD(F.out_rgba + slot0 + (size_t) (s_begin + k)); pq[k] = MTS_FILM_LOAD(F.out_pos + slot0 + (size_t) (s_begin + k)); }
    }
    for (int s0 = s_begin; s0 < n_spp; s0 += kFilmPrefetch) {
#pragma unroll
        for (int k = 0; k < kFilmPrefetch; ++k) {
            const float4 rec = pv[k]; const float2 rp = pq[k];
            {   // the register is free: fetch the sample that will be processed kFilmPrefetch samples from now
                const int j = s0 + kFilmPrefetch + k;
                pv[k] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
                if (j < n_spp) { pv[k] = MTS_FILM_LOAD(F.out_rgba + slot0 + (size_t) j); pq[k] = MTS_FILM_LOAD(F.out_pos + slot0 + (size_t) j); }
            }
            accumulate(rec, rp);
        }
    }
    }
    // ---- exchange: film pixel (dx, dy) of the region <- tap (dx - sxl, dy - syl) of the source pixel at block position (sxl, syl),
    // in ascending (ky, kx) order
    constexpr int kStride = kFilmTaps * 5 + 1;
    const int n_dest = DW * DW;
    float out0[5] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }, out1[5] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    const int d0 = (int) threadIdx.x, d1 = (int) threadIdx.x + kBlock;
    auto collect = [&](int d, int ky, float (&out)[5]) {
        const int dy = d / DW, dx = d - dy * DW, syl = dy - ky;
        if (syl < 0 || syl >= kFilmTile) return;
#pragma unroll
        for (int kx = 0; kx < kFilmTaps; ++kx) {
            const int sxl = dx - kx;
            if (kx > 2 * R || sxl < 0 || sxl >= kFilmTile) continue;
            const float *e = E + (syl * kFilmTile + sxl) * kStride + kx * 5;
#pragma unroll
            for (int c = 0; c < 5; ++c) out[c] += e[c];
        }
    };
#pragma unroll
    for (int ky = 0; ky < kFilmTaps; ++ky) {
        if (ky > 2 * R) break;
        __syncthreads();
#pragma unroll
        for (int kx = 0; kx < kFilmTaps; ++kx)
#pragma unroll
            for (int c = 0; c < 5; ++c) E[sp * kStride + kx * 5 + c] = acc[ky][kx][c];
        __syncthreads();
        collect(d0, ky, out0);
        if (d1 < n_dest) collect(d1, ky, out1);
    }
    float *dst = F.partials + ((size_t) blockIdx.y * gridDim.x + blockIdx.x) * kFilmPartial;
    if (d0 < n_dest)
#pragma unroll
        for (int k = 0; k < 5; ++k) dst[5 * d0 + k] = out0[k];
    if (d1 < n_dest)
#pragma unroll
        for (int k = 0; k < 5; ++k) dst[5 * d1 + k] = out1[k];
}

// film[y][x] += the scratch tiles that reach (x, y), in ascending (tile row, tile column) order
__global__ __launch_bounds__(kBlock) void k_film_merge(const FilmParams F) {
    const int R = (int) ceilf(F.filter.radius), DW = kFilmTile + 2 * R;
    const uint32_t n_rows = (uint32_t) (F.row1 - F.row0);
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= (uint64_t) n_rows * (uint64_t) F.crop_w) return;
    const int x = (int) (i % (uint64_t) F.crop_w), y = F.row0 + (int) (i / (uint64_t) F.crop_w);
    const int tc0 = max(x - R, 0) / kFilmTile, tc1 = min(x + R, F.crop_w - 1) / kFilmTile;
    float acc[5] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    int prev = -1;
    for (int gy = max(y - R, 0); gy <= min(y + R, F.crop_h - 1); ++gy) {
        const int lr = row_to_local(F.rows, gy);
        if (lr < F.pass_lr0 || lr >= F.pass_lr0 + F.pass_rows) continue;
        const int tr = (lr - F.pass_lr0) / F.tile_h;
        if (tr == prev) continue;
        prev = tr;
        const int g0 = row_to_global(F.rows, F.pass_lr0 + tr * F.tile_h);       // film row of the tile's first source row
        const int dy = y - (g0 - R);
        for (int tc = tc0; tc <= tc1; ++tc) {
            const int dx = x - (tc * kFilmTile - R);
            if (dx < 0 || dx >= DW || dy < 0 || dy >= DW) continue;
            for (int sl = 0; sl < F.slices; ++sl) {
                const float *p = F.partials + ((size_t) sl * (size_t) (F.tiles_x * F.tiles_y) + (size_t) (tr * F.tiles_x + tc)) * kFilmPartial + 5 * (dy * DW + dx);
#pragma unroll
                for (int k = 0; k < 5; ++k) acc[k] += p[k];
            }
        }
    }
    if (prev < 0) return;                  // a film row between two of this rank's row tiles: nothing of this pass reaches it
    float *dst = F.film + 5u * ((size_t) y * (size_t) F.crop_w + (size_t) x);
#pragma unroll
    for (int k = 0; k < 5; ++k) dst[k] += acc[k];
}

hipError_t launch_film_tiles(const FilmParams &p, hipStream_t s) {
    if (p.row1 <= p.row0 || p.pass_rows <= 0) return hipSuccess;
    // LDS-staged loads when every run of a pixel's samples is a whole number of 8-sample rounds (and the stream offsets 16-byte aligned)
    if (MTS_FILM_DMA && p.spp % kFilmRound == 0) hipLaunchKernelGGL(k_film_accum<true>, dim3((uint32_t) (p.tiles_x * p.tiles_y), (uint32_t) p.slices), dim3(kBlock), 0, s, p);
    else hipLaunchKernelGGL(k_film_accum<false>, dim3((uint32_t) (p.tiles_x * p.tiles_y), (uint32_t) p.slices), dim3(kBlock), 0, s, p);
    const uint64_t n = (uint64_t) (p.row1 - p.row0) * (uint64_t) p.crop_w;
    hipLaunchKernelGGL(k_film_merge, dim3((uint32_t) ((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_film_gather(const FilmParams &p, hipStream_t s) {
    uint64_t waves = (uint64_t) (p.row1 - p.row0) * (uint64_t) p.crop_w;
    if (waves == 0) return hipSuccess;
    uint64_t blocks = (waves * 64u + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_film_gather, dim3((uint32_t) blocks), dim3(kBlock), 0, s, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Scene::ray_intersect / ray_intersect_naive / ray_test on SoA ray streams
template <int MODE, bool FLAT>
__global__ __launch_bounds__(kBlock) void k_ray_intersect(const SceneView sv, uint64_t n, const RayStreams r,
                                                          float *t, uint32_t *prim, uint32_t *shape, float *u,
                                                          float *v, float *si26) {
    extern __shared__ float4 smem[];
    const LdsView lds = lds_stage<FLAT>(sv, smem);
    const Geo<FLAT> geo{ sv, lds };
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock) {
        bool active = r.active ? r.active[i] != 0 : true;
        Hit hit; bool found = false;
        f3 o = mk3(r.ox[i], r.oy[i], r.oz[i]), d = mk3(r.dx[i], r.dy[i], r.dz[i]);
        if (active) {
            uint32_t tt = 0;
            if (MODE == 0) found = traverse<FLAT, false>(sv, lds, o, d, r.mint[i], r.maxt[i], hit, tt);
            else found = traverse_naive<false>(sv, o, d, r.mint[i], r.maxt[i], hit);
        }
        t[i] = found ? hit.t : __builtin_inff();
        prim[i] = found ? hit.prim : kNoPrim;
        if (shape) shape[i] = found ? geo.prim_shape(hit.prim) : kNoPrim;
        if (u) u[i] = found ? hit.u : 0.0f;
        if (v) v[i] = found ? hit.v : 0.0f;
        if (si26) {
            float o26[26];
#pragma unroll
            for (int k = 0; k < 26; ++k) o26[k] = 0.0f;
            if (found) {
                SurfaceInteraction si;
                fill_si(geo, d, hit.prim, hit.u, hit.v, si);
                o26[0] = si.p.x; o26[1] = si.p.y; o26[2] = si.p.z; o26[3] = si.n.x; o26[4] = si.n.y; o26[5] = si.n.z;
                o26[6] = si.uv.x; o26[7] = si.uv.y;
                o26[8] = si.sh.s.x; o26[9] = si.sh.s.y; o26[10] = si.sh.s.z;
                o26[11] = si.sh.t.x; o26[12] = si.sh.t.y; o26[13] = si.sh.t.z;
                o26[14] = si.sh.n.x; o26[15] = si.sh.n.y; o26[16] = si.sh.n.z;
                o26[17] = si.dp_du.x; o26[18] = si.dp_du.y; o26[19] = si.dp_du.z;
                o26[20] = si.dp_dv.x; o26[21] = si.dp_dv.y; o26[22] = si.dp_dv.z;
                o26[23] = si.wi.x; o26[24] = si.wi.y; o26[25] = si.wi.z;
            } else {
                o26[23] = -d.x; o26[24] = -d.y; o26[25] = -d.z;   // scene_native.inl:28-31
            }
#pragma unroll
            for (int k = 0; k < 26; ++k) si26[(size_t) k * n + i] = o26[k];
        }
    }
}

template <bool FLAT>
__global__ __launch_bounds__(kBlock) void k_ray_test(const SceneView sv, uint64_t n, const RayStreams r, uint8_t *hit_out) {
    extern __shared__ float4 smem[];
    const LdsView lds = lds_stage<FLAT>(sv, smem);
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock) {
        bool active = r.active ? r.active[i] != 0 : true;
        bool found = false;
        if (active) {
            Hit hit; uint32_t tt = 0;
            found = traverse<FLAT, true>(sv, lds, mk3(r.ox[i], r.oy[i], r.oz[i]), mk3(r.dx[i], r.dy[i], r.dz[i]), r.mint[i],
                                   r.maxt[i], hit, tt);
        }
        hit_out[i] = found ? 1 : 0;
    }
}

static uint32_t stream_grid(uint64_t n) {
    uint64_t blocks = (n + kBlock - 1) / kBlock;
    return (uint32_t) (blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));
}

// Hierarchy scenes, plain hit records (no full SurfaceInteraction): every workgroup owns a contiguous chunk of the stream and its
// lanes fetch the next ray of the chunk as soon as their walk ends (dynamic ray fetch, as k_trace does for the path pool).
constexpr uint32_t kRayChunk = 16u * kBlock;
template <bool ANY>
__global__ __launch_bounds__(kBlock)
#if MTS_TRACE_WAVES > 0
__attribute__((amdgpu_waves_per_eu(MTS_TRACE_WAVES, MTS_TRACE_WAVES)))
#endif
void k_ray_walk(const SceneView sv, uint64_t n, const RayStreams r, float *t, uint32_t *prim,
                                                     uint32_t *shape, float *u, float *v, uint8_t *hit) {
    extern __shared__ float4 smem[];
    __shared__ uint32_t s_next;
    const uint32_t lane = lane_id();
    // the first sv.walk_lds_depth stack entries of a lane live in LDS, deeper ones in this workgroup's slice of sv.walk_spill
    const uint32_t spill_depth = sv.stack_depth > sv.walk_lds_depth ? sv.stack_depth - sv.walk_lds_depth : 0u;
    const WalkStack st = { reinterpret_cast<StackEntry *>(smem) + threadIdx.x, log2_stride(kBlock), sv.walk_lds_depth,
                           sv.walk_spill + (size_t) blockIdx.x * spill_depth * kBlock + threadIdx.x, kBlock };
    const LdsView lds = {};
    const Geo<false> geo{ sv, lds };
    uint32_t tri_tests = 0;
    const uint64_t n_chunks = (n + kRayChunk - 1) / kRayChunk;
    for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {      // persistent workgroups: a bounded spill area
    __syncthreads();
    if (threadIdx.x == 0) s_next = 0u;
    __syncthreads();
    const uint64_t base = chunk * kRayChunk;
    const uint32_t total = (uint32_t) min((uint64_t) kRayChunk, n - base);
    BvhWalk w;
    w.cur = kNoNode; w.sp = 0u; w.found = false;
    bool busy = false, exhausted = false;
    uint64_t i = 0;
    auto retire = [&](uint64_t k, bool found) {
        if (ANY) { hit[k] = found ? 1 : 0; return; }
        t[k] = found ? w.best : __builtin_inff();
        prim[k] = found ? w.best_prim : kNoPrim;
        if (shape) shape[k] = found ? geo.prim_shape(w.best_prim) : kNoPrim;
        if (u) u[k] = found ? w.hit.u : 0.0f;
        if (v) v[k] = found ? w.hit.v : 0.0f;
    };
    while (true) {
        const bool need = w.cur == kNoNode;
        if (need && busy) { retire(i, w.found); busy = false; }
        const uint64_t m = __ballot(need);
        if (m && !exhausted) {
            const uint32_t first = (uint32_t) __ffsll((long long) m) - 1u, want = (uint32_t) __popcll(m);
            uint32_t b0 = 0u;
            if (lane == first) b0 = atomicAdd(&s_next, want);
            b0 = __shfl(b0, (int) first);
            exhausted = b0 + want >= total;
            if (need) {
                const uint32_t idx = b0 + mask_rank(m);
                if (idx < total) {
                    i = base + idx;
                    if (r.active && r.active[i] == 0) {
                        w.found = false; retire(i, false);            // inactive lanes: t = inf, no shape (optix_rt.cu:35-37)
                    } else {
                        walk_begin(w, sv, mk3(r.ox[i], r.oy[i], r.oz[i]), mk3(r.dx[i], r.dy[i], r.dz[i]), r.mint[i], r.maxt[i]);
                        busy = true;
                    }
                }
            }
        }
        if (__ballot(w.cur != kNoNode) == 0ull) {
            if (exhausted) break;
            continue;
        }
        if (__ballot(w.cur != kNoNode && w.far) != 0ull) {
            if (w.cur != kNoNode) walk_round<ANY, true>(w, sv, st, tri_tests);
        } else {
            if (w.cur != kNoNode) walk_round<ANY, false>(w, sv, st, tri_tests);
        }
    }
    }
}
static uint32_t walk_grid(const SceneView &sv, uint64_t n) {
    return (uint32_t) std::min<uint64_t>((n + kRayChunk - 1) / kRayChunk, sv.walk_blocks);
}
static size_t walk_lds(const SceneView &sv) { return sizeof(StackEntry) * (std::min(sv.stack_depth, sv.walk_lds_depth) + 1u) * kBlock; }

hipError_t launch_ray_intersect(const SceneView &sv, uint64_t n, const RayStreams &r, int mode, float *t,
                                uint32_t *prim, uint32_t *shape, float *u, float *v, float *si26, hipStream_t s) {
    if (n == 0) return hipSuccess;
    size_t lds = bounce_lds_bytes(sv);
    if (mode == 0 && !sv.flat && !si26) {
        hipLaunchKernelGGL((k_ray_walk<false>), dim3(walk_grid(sv, n)), dim3(kBlock), walk_lds(sv), s,
                           sv, n, r, t, prim, shape, u, v, (uint8_t *) nullptr);
        return hipGetLastError();
    }
    if (mode == 0 && sv.flat)
        return launch_lds(k_ray_intersect<0, true>, dim3(stream_grid(n)), dim3(kBlock), lds, s, sv, n, r, t, prim, shape, u, v, si26);
    else if (mode == 0)
        return launch_lds(k_ray_intersect<0, false>, dim3(stream_grid(n)), dim3(kBlock), lds, s, sv, n, r, t, prim, shape, u, v, si26);
    else if (sv.flat)
        return launch_lds(k_ray_intersect<1, true>, dim3(stream_grid(n)), dim3(kBlock), lds, s, sv, n, r, t, prim, shape, u, v, si26);
    else
        return launch_lds(k_ray_intersect<1, false>, dim3(stream_grid(n)), dim3(kBlock), lds, s, sv, n, r, t, prim, shape, u, v, si26);
    return hipGetLastError();
}

hipError_t launch_ray_test(const SceneView &sv, uint64_t n, const RayStreams &r, uint8_t *hit, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (sv.flat) return launch_lds(k_ray_test<true>, dim3(stream_grid(n)), dim3(kBlock), bounce_lds_bytes(sv), s, sv, n, r, hit);
    else hipLaunchKernelGGL((k_ray_walk<true>), dim3(walk_grid(sv, n)), dim3(kBlock), walk_lds(sv), s,
                            sv, n, r, (float *) nullptr, (uint32_t *) nullptr, (uint32_t *) nullptr, (float *) nullptr, (float *) nullptr, hit);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Operator API on device streams: BSDF::eval / pdf / sample (bsdf.h), Scene::sample_emitter_direction / pdf_emitter_direction
// (scene.cpp:165-206), Emitter::eval (emitter.h) and the independent sampler (independent.cpp:62-72), one query per row.  The kernels
// call the device functions of the render kernels and restate none of them; the order of operations around them is k_direct's.
// Flat scenes stage their tables in LDS as every other kernel does; on hierarchy scenes Geo<false> reads global memory only and no
// operator walks the tree, so nothing is staged and no traversal stack is reserved (as k_ray_walk).
template <bool FLAT>
MTS_DEV LdsView operator_lds(const SceneView &sv, float4 *smem) {
    if (FLAT) return lds_stage<true>(sv, smem);
    return LdsView{};
}
static size_t operator_lds_bytes(const SceneView &sv) { return sv.flat ? bounce_lds_bytes(sv) : 0u; }

// the BSDF record of a row, or false: inactive row, shape index out of range (never dereferenced)
template <bool FLAT>
MTS_DEV bool operator_bsdf(const Geo<FLAT> &geo, const BsdfStreams &q, uint64_t i, DevBsdf &bsdf) {
    if (q.active && q.active[i] == 0) return false;
    const uint32_t shape = q.shape[i];
    if (shape >= geo.sv.n_shapes) return false;
    const int32_t index = geo.shape(shape).bsdf;
    if (index < 0 || (uint32_t) index >= geo.sv.n_bsdfs) return false;
    bsdf = geo.bsdf((uint32_t) index);      // blend / mask: overwritten with the child in use (surface_bsdf_*)
    return true;
}

// out: 4 planes of n floats -- value (3), pdf
template <bool FLAT, bool NEST>
__global__ __launch_bounds__(kBlock) void k_bsdf_eval_pdf(const SceneView sv, uint64_t n, const BsdfStreams q, float *out) {
    extern __shared__ float4 smem[];
    const LdsView lds = operator_lds<FLAT>(sv, smem);
    const Geo<FLAT> geo{ sv, lds };
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock) {
        f3 value = mk3(0.0f, 0.0f, 0.0f); float pdf = 0.0f;
        DevBsdf bsdf;
        if (operator_bsdf(geo, q, i, bsdf)) {
            const f3 wi = mk3(q.wix[i], q.wiy[i], q.wiz[i]), wo = mk3(q.wox[i], q.woy[i], q.woz[i]);
            f2 uv; uv.x = q.u ? q.u[i] : 0.0f; uv.y = q.v ? q.v[i] : 0.0f;
            if (NEST) resolve_textured(sv, bsdf, uv);      // textured parameters of the row's record
            uint32_t texel; f2 tw1;
            const f3 refl = eval_reflectance(sv, bsdf, uv, texel, tw1);
            const NestInfo ni = nest_info<NEST>(bsdf, refl.x, refl.y, refl.z);
            auto child_refl = [&](const DevBsdf &rec) { uint32_t t; f2 w; return eval_reflectance(sv, rec, uv, t, w); };
            surface_bsdf_eval_pdf<NEST>(bsdf, ni, refl, BsdfTable<NEST, FLAT>(geo, uv), child_refl, wi, wo, value, pdf);
        }
        out[i] = value.x; out[n + i] = value.y; out[2u * n + i] = value.z; out[3u * n + i] = pdf;
    }
}

// out: 10 planes of n floats -- wo (3), pdf, eta, delta flag, weight (3), valid flag
template <bool FLAT, bool NEST>
__global__ __launch_bounds__(kBlock) void k_bsdf_sample(const SceneView sv, uint64_t n, const BsdfStreams q, float *out) {
    extern __shared__ float4 smem[];
    const LdsView lds = operator_lds<FLAT>(sv, smem);
    const Geo<FLAT> geo{ sv, lds };
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock) {
        BsdfSample bs; bs.wo = mk3(0.0f, 0.0f, 0.0f); bs.pdf = 0.0f; bs.eta = 0.0f; bs.delta = false;
        f3 weight = mk3(0.0f, 0.0f, 0.0f);
        bool ok = false;
        DevBsdf bsdf;
        if (operator_bsdf(geo, q, i, bsdf)) {
            const f3 wi = mk3(q.wix[i], q.wiy[i], q.wiz[i]);
            f2 uv; uv.x = q.u ? q.u[i] : 0.0f; uv.y = q.v ? q.v[i] : 0.0f;
            f2 s2; s2.x = q.s2x[i]; s2.y = q.s2y[i];
            if (NEST) resolve_textured(sv, bsdf, uv);      // textured parameters of the row's record
            uint32_t texel; f2 tw1;
            const f3 refl = eval_reflectance(sv, bsdf, uv, texel, tw1);
            const NestInfo ni = nest_info<NEST>(bsdf, refl.x, refl.y, refl.z);
            auto child_refl = [&](const DevBsdf &rec) { uint32_t t; f2 w; return eval_reflectance(sv, rec, uv, t, w); };
            ok = surface_bsdf_sample<NEST>(bsdf, ni, refl, BsdfTable<NEST, FLAT>(geo, uv), child_refl, wi, q.s1[i], s2, bs, weight);
            if (!ok) weight = mk3(0.0f, 0.0f, 0.0f);
        }
        out[i] = bs.wo.x; out[n + i] = bs.wo.y; out[2u * n + i] = bs.wo.z; out[3u * n + i] = bs.pdf; out[4u * n + i] = bs.eta;
        out[5u * n + i] = bs.delta ? 1.0f : 0.0f;
        out[6u * n + i] = weight.x; out[7u * n + i] = weight.y; out[8u * n + i] = weight.z; out[9u * n + i] = ok ? 1.0f : 0.0f;
    }
}

template <bool EVAL>
static hipError_t launch_bsdf_operator(const SceneView &sv, uint64_t n, const BsdfStreams &q, float *out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const dim3 grid(stream_grid(n)), block(kBlock);
    const size_t lds = operator_lds_bytes(sv);
    hipError_t err = hipSuccess;
    // the nesting code is compiled into the instantiation that only scenes with a blendbsdf / mask launch (as k_direct)
    with_flag(sv.flat != 0u, [&](auto flat) {
        with_flag(sv.general == 2u, [&](auto nest) {
            constexpr bool F = decltype(flat)::value, N = decltype(nest)::value;
            if (EVAL) err = launch_lds(k_bsdf_eval_pdf<F, N>, grid, block, lds, s, sv, n, q, out);
            else err = launch_lds(k_bsdf_sample<F, N>, grid, block, lds, s, sv, n, q, out);
        });
    });
    return err;
}
hipError_t launch_bsdf_eval_pdf(const SceneView &sv, uint64_t n, const BsdfStreams &q, float *out4, hipStream_t s) {
    return launch_bsdf_operator<true>(sv, n, q, out4, s);
}
hipError_t launch_bsdf_sample(const SceneView &sv, uint64_t n, const BsdfStreams &q, float *out10, hipStream_t s) {
    return launch_bsdf_operator<false>(sv, n, q, out10, s);
}

// Scene::sample_emitter_direction without the visibility test (the caller traces the shadow rays with k_ray_test): the RGB form of
// sample_emitter_direction<FLAT, true>.  out: 15 planes of n floats -- p (3), n (3), d (3), dist, pdf, delta flag, spec (3)
template <bool FLAT>
__global__ __launch_bounds__(kBlock) void k_sample_emitter_direction(const SceneView sv, uint64_t n, const EmitterSampleStreams q, float *out,
                                                                     uint32_t *emitter) {
    extern __shared__ float4 smem[];
    const LdsView lds = operator_lds<FLAT>(sv, smem);
    const Geo<FLAT> geo{ sv, lds };
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock) {
        float o[15];
#pragma unroll
        for (int k = 0; k < 15; ++k) o[k] = 0.0f;
        uint32_t index = kNoPrim;
        if ((q.active ? q.active[i] != 0 : true) && sv.n_emitters != 0u) {
            f2 s2; s2.x = q.sx[i]; s2.y = q.sy[i];
            DirectionSample ds; f3 spec;
            sample_emitter_direction<FLAT, true>(geo, mk3(q.px[i], q.py[i], q.pz[i]), s2, ds, spec);
            o[0] = ds.p.x; o[1] = ds.p.y; o[2] = ds.p.z; o[3] = ds.n.x; o[4] = ds.n.y; o[5] = ds.n.z;
            o[6] = ds.d.x; o[7] = ds.d.y; o[8] = ds.d.z; o[9] = ds.dist; o[10] = ds.pdf; o[11] = ds.delta ? 1.0f : 0.0f;
            o[12] = spec.x; o[13] = spec.y; o[14] = spec.z;
            index = ds.emitter;
        }
#pragma unroll
        for (int k = 0; k < 15; ++k) out[(size_t) k * n + i] = o[k];
        emitter[i] = index;
    }
}
hipError_t launch_sample_emitter_direction(const SceneView &sv, uint64_t n, const EmitterSampleStreams &q, float *out15, uint32_t *emitter, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const size_t lds = operator_lds_bytes(sv);
    if (sv.flat) return launch_lds(k_sample_emitter_direction<true>, dim3(stream_grid(n)), dim3(kBlock), lds, s, sv, n, q, out15, emitter);
    else return launch_lds(k_sample_emitter_direction<false>, dim3(stream_grid(n)), dim3(kBlock), lds, s, sv, n, q, out15, emitter);
    return hipGetLastError();
}

// The two kernels below read one emitter record per row and nothing else of the scene, so they take it from global memory on flat
// scenes too (staging a whole flat scene in LDS for it would cost more than it saves) and have no FLAT instantiation.
// Scene::pdf_emitter_direction (scene.cpp:191-206) as k_direct evaluates it for a BSDF sample: area emitters pdf_emitter_direction,
// the environment emitter pdf_environment, delta rows / delta emitters / no emitter 0
__global__ __launch_bounds__(kBlock) void k_pdf_emitter_direction(const SceneView sv, uint64_t n, const EmitterQueryStreams q, float *pdf) {
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock) {
        float r = 0.0f;
        const uint32_t index = q.emitter[i];
        if ((q.active ? q.active[i] != 0 : true) && index < sv.n_emitters && !(q.delta && q.delta[i] != 0)) {
            const DevEmitter e = sv.emitters[index];
            const f3 d = mk3(q.dx[i], q.dy[i], q.dz[i]);
            if (e.pad0 == kEmitterConstant || e.pad0 == kEmitterEnvmap) r = pdf_environment(sv, e, d);
            else if (e.pad0 < kEmitterPoint) r = pdf_emitter_direction(sv.n_emitters, e.area_norm, d, mk3(q.nx[i], q.ny[i], q.nz[i]), q.dist[i]);
        }
        pdf[i] = r;
    }
}
// Emitter::eval at a surface interaction (area.cpp:71-76: radiance where wi.z > 0) or for an escaped ray (environment_radiance along
// the world direction d); delta emitters and "none" (0xffffffff) give 0.  out: 3 planes of n floats; q.nx/ny/nz carry the local wi
__global__ __launch_bounds__(kBlock) void k_emitter_eval(const SceneView sv, uint64_t n, const EmitterQueryStreams q, float *out) {
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock) {
        f3 le = mk3(0.0f, 0.0f, 0.0f);
        const uint32_t index = q.emitter[i];
        if ((q.active ? q.active[i] != 0 : true) && index < sv.n_emitters) {
            const DevEmitter e = sv.emitters[index];
            if (e.pad0 == kEmitterConstant || e.pad0 == kEmitterEnvmap) le = environment_radiance(sv, e, mk3(q.dx[i], q.dy[i], q.dz[i]));
            else if (e.pad0 < kEmitterPoint) le = q.nz[i] > 0.0f ? mk3(e.r, e.g, e.b) : mk3(0.0f, 0.0f, 0.0f);
        }
        out[i] = le.x; out[n + i] = le.y; out[2u * n + i] = le.z;
    }
}
hipError_t launch_pdf_emitter_direction(const SceneView &sv, uint64_t n, const EmitterQueryStreams &q, float *pdf, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pdf_emitter_direction, dim3(stream_grid(n)), dim3(kBlock), 0, s, sv, n, q, pdf);
    return hipGetLastError();
}
hipError_t launch_emitter_eval(const SceneView &sv, uint64_t n, const EmitterQueryStreams &q, float *out3, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_emitter_eval, dim3(stream_grid(n)), dim3(kBlock), 0, s, sv, n, q, out3);
    return hipGetLastError();
}

// IndependentSampler (independent.cpp:62-72): one PCG32 stream per lane, held by the caller as (state, inc).  Lane i is the stream
// generate_path gives global sample index first + i.
__global__ __launch_bounds__(kBlock) void k_sampler_seed(uint64_t n, uint64_t first, uint64_t base_seed, uint64_t *state, uint64_t *inc) {
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock) {
        Pcg32 rng;
        seed_sample(rng, first + i, base_seed);
        state[i] = rng.state; inc[i] = rng.inc;
    }
}
// next_1d / next_2d: DIMS floats per lane (planes of n); only active lanes advance (enoki's masked next_float32)
template <int DIMS>
__global__ __launch_bounds__(kBlock) void k_sampler_next(uint64_t n, uint64_t *state, const uint64_t *inc, const uint8_t *active, float *out) {
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock) {
        float v[DIMS];
#pragma unroll
        for (int k = 0; k < DIMS; ++k) v[k] = 0.0f;
        if (active ? active[i] != 0 : true) {
            Pcg32 rng = { state[i], inc[i] };
#pragma unroll
            for (int k = 0; k < DIMS; ++k) v[k] = pcg_next_f32(rng);
            state[i] = rng.state;
        }
#pragma unroll
        for (int k = 0; k < DIMS; ++k) out[(size_t) k * n + i] = v[k];
    }
}
hipError_t launch_sampler_seed(uint64_t n, uint64_t first, uint64_t base_seed, uint64_t *state, uint64_t *inc, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sampler_seed, dim3(stream_grid(n)), dim3(kBlock), 0, s, n, first, base_seed, state, inc);
    return hipGetLastError();
}
hipError_t launch_sampler_next(uint64_t n, int dims, uint64_t *state, const uint64_t *inc, const uint8_t *active, float *out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (dims == 1) hipLaunchKernelGGL(k_sampler_next<1>, dim3(stream_grid(n)), dim3(kBlock), 0, s, n, state, inc, active, out);
    else hipLaunchKernelGGL(k_sampler_next<2>, dim3(stream_grid(n)), dim3(kBlock), 0, s, n, state, inc, active, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_camera_rays(const CameraView cam, uint64_t n, const float *sx, const float *sy,
                                                        const float *apx, const float *apy, float *ox, float *oy, float *oz, float *dx, float *dy, float *dz,
                                                        float *mint, float *maxt) {
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock) {
        f3 o, d; float t0, t1;
        f2 ap; ap.x = apx ? apx[i] : 0.5f; ap.y = apy ? apy[i] : 0.5f;
        camera_ray(cam, sx[i], sy[i], ap, o, d, t0, t1);
        ox[i] = o.x; oy[i] = o.y; oz[i] = o.z; dx[i] = d.x; dy[i] = d.y; dz[i] = d.z; mint[i] = t0; maxt[i] = t1;
    }
}
hipError_t launch_camera_rays(const CameraView &cam, uint64_t n, const float *sx, const float *sy, const float *apx, const float *apy, float *ox, float *oy,
                              float *oz, float *dx, float *dy, float *dz, float *mint, float *maxt, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_camera_rays, dim3(stream_grid(n)), dim3(kBlock), 0, s, cam, n, sx, sy, apx, apy, ox, oy, oz, dx, dy, dz, mint, maxt);
    return hipGetLastError();
}

// ImageBlock::put(pos, value) as a scatter with float atomics (the reference's scatter_add)
__global__ __launch_bounds__(kBlock) void k_imageblock_put(const FilterView f, int32_t w, int32_t h, int32_t ox, int32_t oy,
                                                           int32_t ch, int32_t border, uint64_t n, const float *pos,
                                                           const float *values, float *data) {
    const int sx = w + 2 * border, sy = h + 2 * border;
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock) {
        const float *val = values + (size_t) ch * i;
        bool valid = true;
        for (int k = 0; k < ch; ++k) valid = valid && (val[k] >= -1e-5f) && isfinite(val[k]);
        if (!valid) continue;
        float px = pos[2 * i] - ((float) (ox - border) + 0.5f), py = pos[2 * i + 1] - ((float) (oy - border) + 0.5f);
        if (f.radius > 1.0f) {
            int lox = max((int) ceilf(px - f.radius), 0), loy = max((int) ceilf(py - f.radius), 0);
            int hix = min((int) floorf(px + f.radius), sx - 1), hiy = min((int) floorf(py + f.radius), sy - 1);
            float bx = (float) (uint32_t) lox - px, by = (float) (uint32_t) loy - py;
            for (int yr = 0; yr < f.taps; ++yr) {
                int y = loy + yr;
                if (y > hiy) break;
                float wy = filter_weight(f, by + (float) yr);
                for (int xr = 0; xr < f.taps; ++xr) {
                    int x = lox + xr;
                    if (x > hix) break;
                    float wgt = wy * filter_weight(f, bx + (float) xr);
                    float *dst = data + (size_t) ch * ((size_t) y * sx + x);
                    for (int k = 0; k < ch; ++k) atomicAdd(dst + k, val[k] * wgt);
                }
            }
        } else {
            int lox = (int) ceilf(px - 0.5f), loy = (int) ceilf(py - 0.5f);
            if (lox >= 0 && loy >= 0 && lox < sx && loy < sy) {
                float *dst = data + (size_t) ch * ((size_t) loy * sx + lox);
                for (int k = 0; k < ch; ++k) atomicAdd(dst + k, val[k]);
            }
        }
    }
}
hipError_t launch_imageblock_put(const FilterView &f, int32_t w, int32_t h, int32_t ox, int32_t oy, int32_t ch,
                                 int32_t border, uint64_t n, const float *pos, const float *values, float *data,
                                 hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_imageblock_put, dim3(stream_grid(n)), dim3(kBlock), 0, s, f, w, h, ox, oy, ch, border, n, pos, values, data);
    return hipGetLastError();
}

// ImageBlock::put(block): clipped rectangular += (accumulate_2d, bitmap.h:657-716)
__global__ __launch_bounds__(kBlock) void k_put_block(const float *src, int ssx, int sox, int soy, float *dst, int tsx, int tox,
                                                      int toy, int szx, int szy, int ch) {
    uint64_t total = (uint64_t) szx * szy * ch;
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t) gridDim.x * kBlock) {
        int row_elems = szx * ch;
        int y = (int) (i / row_elems), c = (int) (i % row_elems);
        dst[((size_t) (toy + y) * tsx + tox) * ch + c] += src[((size_t) (soy + y) * ssx + sox) * ch + c];
    }
}
hipError_t launch_put_block(const float *src, int32_t sw, int32_t sh, int32_t sox_, int32_t soy_, int32_t sb, float *dst,
                            int32_t dw, int32_t dh, int32_t dox, int32_t doy, int32_t db, int32_t ch, hipStream_t s) {
    int ssx = sw + 2 * sb, ssy = sh + 2 * sb, tsx = dw + 2 * db, tsy = dh + 2 * db;
    int sox = 0, soy = 0, tox = (sox_ - sb) - (dox - db), toy = (soy_ - sb) - (doy - db);
    int szx = ssx, szy = ssy;
    int shx = std::max(0, std::max(-sox, -tox)), shy = std::max(0, std::max(-soy, -toy));
    sox += shx; tox += shx; soy += shy; toy += shy;
    szx -= std::max(sox + szx - ssx, 0); szx -= std::max(tox + szx - tsx, 0);
    szy -= std::max(soy + szy - ssy, 0); szy -= std::max(toy + szy - tsy, 0);
    if (szx <= 0 || szy <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_put_block, dim3(stream_grid((uint64_t) szx * szy * ch)), dim3(kBlock), 0, s, src, ssx, sox, soy, dst,
                       tsx, tox, toy, szx, szy, ch);
    return hipGetLastError();
}

// HDRFilm::bitmap: (X,Y,Z,A) / W, RGB = M * XYZ (hdrfilm.cpp:278-299, struct.cpp:1761-1811)
// RoughPlastic::parameters_changed (roughplastic.cpp:380-399): one thread per table entry
__global__ __launch_bounds__(kRoughTableRes) void k_roughplastic_tables(DevBsdf *bsdfs, uint32_t index, float *table, const float *gl,
                                                                      int res_t, int res_r) {
    __shared__ float part[kRoughTableRes];
    const DevBsdf b = bsdfs[index];
    const Mdf d = mdf_make((b.flags & kBsdfGGX) != 0u, b.alpha_u, b.alpha_u, true);
    const int i = (int) threadIdx.x;
    const float mu = fmaxf(1e-6f, (float) i / (float) (kRoughTableRes - 1));
    const f3 wi = mk3(sqrtf(1.0f - mu * mu), 0.0f, mu);
    const float eta = b.er, inv_eta = 1.0f / eta;
    table[i] = rough_transmittance(d, wi, eta, res_t, gl, gl + 128);
    part[i] = rough_reflectance(d, wi, inv_eta, res_r, gl + 256, gl + 384) * wi.z;
    __syncthreads();
    if (i == 0) {
        float sum = 0.0f;
        for (int k = 0; k < kRoughTableRes; ++k) sum += part[k];
        bsdfs[index].eb = (sum * (1.0f / (float) kRoughTableRes)) * 2.0f;
        bsdfs[index].table = table;
    }
}
hipError_t launch_roughplastic_tables(DevBsdf *bsdfs, uint32_t index, float *table, const float *gl, int res_t, int res_r, hipStream_t s) {
    hipLaunchKernelGGL(k_roughplastic_tables, dim3(1), dim3(kRoughTableRes), 0, s, bsdfs, index, table, gl, res_t, res_r);
    return hipGetLastError();
}

// Flat scenes: the frame words of the shading records (device_scene.h), one thread per primitive, by the functions fill_si calls per
// hit on every other scene.  n for every primitive; s only where the shape has no vertex normals (the others interpolate per hit).
__global__ __launch_bounds__(kBlock) void k_flat_frames(float4 *flat, uint32_t n_prims, const DevShape *shapes, const float *tri_uv) {
    const uint32_t prim = blockIdx.x * (uint32_t) kBlock + threadIdx.x;
    if (prim >= n_prims) return;
    float4 r0 = flat[4u * prim], r2 = flat[4u * prim + 2u];
    const float4 r3 = flat[4u * prim + 3u];
    const f3 p0 = mk3(r0.x, r0.y, r0.z), p1 = mk3(r2.y, r2.z, r2.w), p2 = mk3(r3.x, r3.y, r3.z);
    const uint32_t flags = shapes[__float_as_uint(r3.w)].flags;
    const f3 dp0 = p1 - p0, dp1 = p2 - p0;
    const f3 n = tri_normal(dp0, dp1);
    f3 s = mk3(0.0f, 0.0f, 0.0f);
    if (!(flags & kShapeHasNormals)) {
        f2 uv; f3 dp_du, dp_dv;
        tri_parameterization(n, dp0, dp1, flags, tri_uv, prim, 1.0f, 0.0f, 0.0f, uv, dp_du, dp_dv);
        s = shading_tangent(n, dp_du);
    }
    r0.w = n.x; r2.x = s.z;
    flat[4u * prim] = r0;
    flat[4u * prim + 1u] = make_float4(n.y, n.z, s.x, s.y);
    flat[4u * prim + 2u] = r2;
}
hipError_t launch_flat_frames(float4 *flat, uint32_t n_prims, const DevShape *shapes, const float *tri_uv, hipStream_t s) {
    if (n_prims == 0) return hipSuccess;
    hipLaunchKernelGGL(k_flat_frames, dim3((n_prims + (uint32_t) kBlock - 1u) / (uint32_t) kBlock), dim3(kBlock), 0, s, flat, n_prims, shapes, tri_uv);
    return hipGetLastError();
}

__global__ __launch_bounds__(kBlock) void k_square_stream(float4 *rgba, uint64_t n) {
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float4 v = rgba[i];
    v.x *= v.x; v.y *= v.y; v.z *= v.z;            // m2 AOVs: sqr of the nested integrator's XYZ (moment.cpp:91-93)
    rgba[i] = v;
}
__global__ __launch_bounds__(kBlock) void k_moment_pack(const float *a, const float *b, float *out, uint64_t n) {
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *pa = a + 5u * i, *pb = b + 5u * i;
    float *o = out + 11u * i;
    o[0] += pa[0]; o[1] += pa[1]; o[2] += pa[2]; o[3] += pa[3]; o[4] += pa[4];
    o[5] += pa[0]; o[6] += pa[1]; o[7] += pa[2];
    o[8] += pb[0]; o[9] += pb[1]; o[10] += pb[2];
}
hipError_t launch_square_stream(float4 *rgba, uint64_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_square_stream, dim3((uint32_t) ((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, rgba, n);
    return hipGetLastError();
}
hipError_t launch_moment_pack(const float *values5, const float *squares5, float *film11, uint64_t n_pixels, hipStream_t s) {
    if (n_pixels) hipLaunchKernelGGL(k_moment_pack, dim3((uint32_t) ((n_pixels + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, values5, squares5, film11, n_pixels);
    return hipGetLastError();
}

// aov integrator: the sample streams of a pass -- the nested integrator's and the channel groups of k_aov -- are made to drop the same
// samples, and the nested stream gets its second colour space (kernels.h, launch_aov_finish)
__global__ __launch_bounds__(kBlock) void k_aov_finish(float4 *stream, float4 *conv, float4 *groups, uint64_t group_stride, uint32_t n_groups,
                                                       int mode, uint64_t n) {
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c = v;
    if (mode != 0) v = stream[i];
    bool drop = v.w < 0.0f;
    if (mode == 1) {                // integrator.cpp:254-262, the arithmetic of store_result
        const f3 xyz = srgb_to_xyz(mk3(v.x, v.y, v.z));
        c = make_float4(xyz.x, xyz.y, xyz.z, v.w);
    } else if (mode == 2) {         // the matrix of k_film_develop, before the film's sum instead of after it
        float r = 0.0f, g = 0.0f, b = 0.0f;
        r += 3.240479f * v.x; r += -1.537150f * v.y; r += -0.498535f * v.z;
        g += -0.969256f * v.x; g += 1.875991f * v.y; g += 0.041556f * v.z;
        b += 0.055648f * v.x; b += -0.204043f * v.y; b += 1.057311f * v.z;
        c = make_float4(r, g, b, v.w);
    }
    drop = drop || !(isfinite(c.x) && isfinite(c.y) && isfinite(c.z));
    for (uint32_t g = 0; g < n_groups; ++g) drop = drop || groups[(size_t) g * group_stride + i].w < 0.0f;
    if (drop) {
        for (uint32_t g = 0; g < n_groups; ++g) groups[(size_t) g * group_stride + i].w = -1.0f;
        v.w = c.w = -1.0f;
    }
    if (mode == 0 || drop) stream[i] = v;
    if (mode != 0) conv[i] = c;
}
__global__ __launch_bounds__(kBlock) void k_aov_pack(const float *films5, uint64_t n_pixels, uint32_t n_channels, int nested, float *film) {
    const uint32_t stride = 5u + n_channels + (nested ? 4u : 0u);
    const uint64_t e = (uint64_t) blockIdx.x * kBlock + threadIdx.x;       // one thread per float of the film
    if (e >= n_pixels * stride) return;
    const uint64_t i = e / stride;
    const uint32_t c = (uint32_t) (e - i * stride);
    uint32_t f = 0u, k = c;                                                // film, channel inside it
    if (c >= 5u + n_channels) { f = 1u + (n_channels + 2u) / 3u; k = c - 5u - n_channels; }
    else if (c >= 5u) { f = 1u + (c - 5u) / 3u; k = (c - 5u) % 3u; }
    film[e] += films5[((size_t) f * n_pixels + i) * 5u + k];
}
__global__ __launch_bounds__(kBlock) void k_aov_unpack(const float4 *groups, uint64_t group_stride, uint32_t n_channels, uint64_t n, float *out) {
    const uint64_t e = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (e >= n * n_channels) return;
    const uint64_t i = e / n_channels;
    const uint32_t c = (uint32_t) (e - i * n_channels);
    const float4 v = groups[(size_t) (c / 3u) * group_stride + i];
    out[e] = c % 3u == 0u ? v.x : (c % 3u == 1u ? v.y : v.z);
}
hipError_t launch_aov_finish(float4 *stream, float4 *conv, float4 *groups, uint64_t group_stride, uint32_t n_groups, int mode, uint64_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_aov_finish, dim3((uint32_t) ((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, stream, conv, groups, group_stride, n_groups, mode, n);
    return hipGetLastError();
}
hipError_t launch_aov_pack(const float *films5, uint64_t n_pixels, uint32_t n_channels, int nested, float *film, hipStream_t s) {
    const uint64_t n = n_pixels * (5u + n_channels + (nested ? 4u : 0u));
    if (n) hipLaunchKernelGGL(k_aov_pack, dim3((uint32_t) ((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, films5, n_pixels, n_channels, nested, film);
    return hipGetLastError();
}
hipError_t launch_aov_unpack(const float4 *groups, uint64_t group_stride, uint32_t n_channels, uint64_t n, float *out, hipStream_t s) {
    const uint64_t e = n * n_channels;
    if (e) hipLaunchKernelGGL(k_aov_unpack, dim3((uint32_t) ((e + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, groups, group_stride, n_channels, n, out);
    return hipGetLastError();
}

__global__ __launch_bounds__(kBlock) void k_film_develop(const float *xyzaw, uint64_t n, float *rgba) {
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock) {
        const float *p = xyzaw + 5 * i;
        float inv_w = 1.0f / p[4];
        float r = 0.0f, g = 0.0f, b = 0.0f;
        r += 3.240479f * p[0]; r += -1.537150f * p[1]; r += -0.498535f * p[2];
        g += -0.969256f * p[0]; g += 1.875991f * p[1]; g += 0.041556f * p[2];
        b += 0.055648f * p[0]; b += -0.204043f * p[1]; b += 1.057311f * p[2];
        rgba[4 * i] = r * inv_w; rgba[4 * i + 1] = g * inv_w; rgba[4 * i + 2] = b * inv_w; rgba[4 * i + 3] = p[3] * inv_w;
    }
}
hipError_t launch_film_develop(const float *xyzaw, uint64_t n, float *rgba, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_film_develop, dim3(stream_grid(n)), dim3(kBlock), 0, s, xyzaw, n, rgba);
    return hipGetLastError();
}

// device_libm.h on argument streams (mtsamd_libm_eval: host / device bit-equality tests)
__global__ __launch_bounds__(kBlock) void k_libm_eval(int fn, uint64_t n, const float *x, const float *y, float *out) {
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float a = x[i];
    float r;
    switch (fn) {
    case 0: r = lm_sin(a); break;
    case 1: r = lm_cos(a); break;
    case 2: r = lm_tan(a); break;
    case 3: r = lm_exp(a); break;
    case 4: r = lm_log(a); break;
    case 5: r = lm_erf(a); break;
    case 6: r = lm_acos(a); break;
    case 8: r = lm_atanh(a); break;
    case 9: r = lm_cosh(a); break;
    default: r = lm_atan2(a, y[i]); break;
    }
    out[i] = r;
}
hipError_t launch_libm_eval(int fn, uint64_t n, const float *x, const float *y, float *out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_libm_eval, dim3((uint32_t) ((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, fn, n, x, y, out);
    return hipGetLastError();
}

// spectrum_eval() on a wavelength stream (mtsamd_spectrum_eval): the function the render kernels call, on a pool of one spectrum
__global__ __launch_bounds__(kBlock) void k_spectrum_eval(const DevSpectrum *headers, const float *data, uint64_t n, const float *lambda, float *out) {
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[i] = spectrum_eval(SpectrumPool{ headers, data }, 0u, lambda[i]);
}
hipError_t launch_spectrum_eval(const DevSpectrum *headers, const float *data, uint64_t n, const float *lambda, float *out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_spectrum_eval, dim3((uint32_t) ((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, headers, data, n, lambda, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// (Last in the file on purpose: the assembler numbers functions and long-branch labels in the order the kernels are emitted, and
// scripts/isa_compare.py compares every kernel above with its text before this one existed.)
// Derivative w.r.t. the texels of bitmaps bound to a BSDF PARAMETER (resolve_textured: alpha_u / alpha_v of the rough models, the specular
// colours of the conductors and dielectrics) in any RGB scene of plain records: the backward sweep of k_adjoint_tex joined with the central
// difference of ParamGradProbe.  One launch differentiates ONE slot (A.pg_bsdf: kTexAlphaU .. kTexTrans, uniform over the launch) for every
// record that binds it (a textured `alpha` -- one bitmap behind alpha_u and alpha_v -- is differentiated as the one parameter it is, in
// the alpha_u launch: ParamTexRecorder::surface).  Sampling is detached as in k_adjoint_param: directions, pdfs, lobe choices, MIS
// weights AND the Russian-roulette probability are those of the primal path (only invq is recorded, there is no rr_channel term), so
// the texel gradients of a uniform map sum to what k_adjoint_param gives for the constant, at any depth.
//
// What the replay keeps of one vertex: T, invq, E, Nc, W as VertexRecG, and dNc / dW = (f(rec + h) - f(rec - h)) / 2h with respect to the
// slot's parameter at the vertex, per colour channel.  The two working records are perturbed AFTER resolve_textured, as
// ParamGradProbe::dvalue perturbs bp / bm.  A colour slot moves its three channels with one +- pair (the models are diagonal in their
// specular colours); a roughness slot differentiates every channel with respect to the scalar, `lum` says how resolve_textured made it
// from the RGB texel.  texel / w1: the bilinear footprint of the SLOT's lookup (kNoPrim: constant or checkerboard -- no gradient).
struct VertexRecP {
    f3 T; float invq;
    f3 E; uint32_t texel;
    f3 Nc; int32_t texture;
    f3 W; uint32_t lum;
    f3 dNc; f3 dW; f2 w1;
};
static_assert(sizeof(VertexRecP) <= sizeof(VertexRecG), "the per-lane record array of k_adjoint_param_tex stays within that of k_adjoint_tex");

// Fills the VertexRecP of one step.  The step is absolute (`h`, the same at every vertex; <= 0: 1 % of the value looked up at the hit,
// of at least 0.05 as mtsamd_render_adjoint_param takes it); it must stay below the smallest roughness of the map.
struct ParamTexRecorder {
    static constexpr bool kFactoredEmitter = false, kMirrorTwoSided = false, kSamples = true;
    VertexRecP &r;
    const SceneView &sv; int slot; float h;
    bool here;                  // does the record of the hit read the slot from a bitmap?
    bool pair;                  // ... alpha_u AND alpha_v from that one bitmap (a textured `alpha`): the lookup moves both
    f3 hs, i2h;                 // the step per channel at this vertex and 1 / ((v + h) - (v - h))
    f3 nc, dnc;                 // Nc and dNc of the emitter sample, recorded once it is known to be unoccluded
    MTS_DEV void perturbed(const DevBsdf &b, DevBsdf &bp, DevBsdf &bm) const {
        bp = b; bm = b;
        if (slot == kTexAlphaU) {
            bp.alpha_u = b.alpha_u + hs.x; bm.alpha_u = b.alpha_u - hs.x;
            if (pair) { bp.alpha_v = b.alpha_v + hs.x; bm.alpha_v = b.alpha_v - hs.x; }
        } else if (slot == kTexAlphaV) { bp.alpha_v = b.alpha_v + hs.x; bm.alpha_v = b.alpha_v - hs.x; }
        else if (slot == kTexSpec) {
            bp.sr = b.sr + hs.x; bp.sg = b.sg + hs.y; bp.sb = b.sb + hs.z;
            bm.sr = b.sr - hs.x; bm.sg = b.sg - hs.y; bm.sb = b.sb - hs.z;
        } else {                // dielectrics: k.* holds the transmittance
            bp.kr = b.kr + hs.x; bp.kg = b.kg + hs.y; bp.kb = b.kb + hs.z;
            bm.kr = b.kr - hs.x; bm.kg = b.kg - hs.y; bm.kb = b.kb - hs.z;
        }
    }
    // d(value)/d(parameter) of the model at fixed directions, per channel
    MTS_DEV f3 dvalue(const DevBsdf &b, f3 refl, f3 wi, f3 wo) const {
        DevBsdf bp, bm; f3 vp, vm; float pp, pm;
        perturbed(b, bp, bm);
        bsdf_eval_pdf(bp, refl, wi, wo, vp, pp);
        bsdf_eval_pdf(bm, refl, wi, wo, vm, pm);
        return mk3((vp.x - vm.x) * i2h.x, (vp.y - vm.y) * i2h.y, (vp.z - vm.z) * i2h.z);
    }
    template <int DEFER, bool GENERAL, bool NEST> MTS_DEV void begin(const PathState &s) {
        static_assert(GENERAL && DEFER == 0, "the textured-parameter gradient rides on the general fused step");
        r.T = s.thr; r.invq = 1.0f;
        r.E = r.Nc = r.W = r.dNc = r.dW = mk3(0.0f, 0.0f, 0.0f);
        r.texel = kNoPrim; r.texture = -1; r.lum = 0u; r.w1.x = r.w1.y = 0.0f;
        here = pair = false;
    }
    MTS_DEV void emitted(float ew, int32_t, f3 le) { r.E = mk3(ew * le.x, ew * le.y, ew * le.z); }
    MTS_DEV void escaped(const SceneView &, const PathState &, const DevEmitter &, float ew, f3 le) { emitted(ew, -1, le); }
    MTS_DEV void roulette(f3, float, float rq, bool) { r.invq = rq; }
    // `bsdf` is the working record after resolve_textured; the footprint of the slot's lookup is taken here, by one more lookup
    MTS_DEV void surface(const SurfaceInteraction &si, const DevBsdf &bsdf, f3, uint32_t, f2, f3) {
        here = pair = false;
        const uint32_t ti = (bsdf.flags & kBsdfTexParams) ? bsdf_param_texture(bsdf, slot) : 0u;
        if (!ti) return;
        // one texture behind alpha_u and alpha_v is ONE parameter, alpha(texel) -> f(alpha, alpha): its central difference moves both
        // roughnesses together, in the alpha_u launch, and the alpha_v launch leaves the record alone.  (The sum of the two partial
        // differences misses the mixed third derivatives: 0.8 % of the derivative of a GGX lobe at alpha = 0.1, h = 0.01.)
        if (slot <= kTexAlphaV && bsdf_param_texture(bsdf, kTexAlphaU) == bsdf_param_texture(bsdf, kTexAlphaV)) {
            if (slot == kTexAlphaV) return;
            pair = true;
        }
        uint32_t texel; f2 w1;
        f3 v = eval_reflectance<false>(sv, bsdf, si.uv, texel, w1, (int32_t) (ti - 1u));
        if (texel == kNoPrim) return;                        // a checkerboard has no texels
        here = true;
        r.texel = texel; r.w1 = w1; r.texture = (int32_t) (ti - 1u);
        if (slot == kTexAlphaU) { r.lum = (bsdf.flags & kBsdfAlphaULum) ? 1u : 0u; v = mk3(bsdf.alpha_u, bsdf.alpha_u, bsdf.alpha_u); }
        if (slot == kTexAlphaV) { r.lum = (bsdf.flags & kBsdfAlphaVLum) ? 1u : 0u; v = mk3(bsdf.alpha_v, bsdf.alpha_v, bsdf.alpha_v); }
        hs = mk3(h, h, h);
        if (!(h > 0.0f)) hs = mk3(0.01f * fmaxf(fabsf(v.x), 0.05f), 0.01f * fmaxf(fabsf(v.y), 0.05f), 0.01f * fmaxf(fabsf(v.z), 0.05f));
        i2h = mk3(1.0f / ((v.x + hs.x) - (v.x - hs.x)), 1.0f / ((v.y + hs.y) - (v.y - hs.y)), 1.0f / ((v.z + hs.z) - (v.z - hs.z)));
    }
    MTS_DEV bool emitter_sample(const SceneView &, const DevBsdf &bsdf, f3 refl, const NeeTerms &t) {
        nc = mk3((t.mis * t.bv.x) * t.spec.x, (t.mis * t.bv.y) * t.spec.y, (t.mis * t.bv.z) * t.spec.z);
        dnc = mk3(0.0f, 0.0f, 0.0f);
        if (here) {
            const f3 dbv = dvalue(bsdf, refl, t.wi, t.wo);
            dnc = mk3((t.mis * dbv.x) * t.spec.x, (t.mis * dbv.y) * t.spec.y, (t.mis * dbv.z) * t.spec.z);
        }
        return nc.x != 0.0f || nc.y != 0.0f || nc.z != 0.0f || dnc.x != 0.0f || dnc.y != 0.0f || dnc.z != 0.0f;
    }
    MTS_DEV void unoccluded(const SceneView &, const SurfaceInteraction &, f3, const NeeTerms &) { r.Nc = nc; r.dNc = dnc; }
    // T_next = T' * W; dW at the sampled direction: d(value) / pdf for a smooth lobe, the re-sampled weight for a discrete one
    MTS_DEV void bsdf_sampled(const SceneView &, const SurfaceInteraction &si, const DevBsdf &bsdf, f3 refl, f3, const BsdfSample &bs, f3 weight, float s1, f2 s2) {
        r.W = weight;
        if (here && !bs.delta && bs.pdf > 0.0f) {
            const f3 dv = dvalue(bsdf, refl, si.wi, bs.wo);
            const float ip = rcp(bs.pdf);
            r.dW = mk3(dv.x * ip, dv.y * ip, dv.z * ip);
        } else if (here && bs.delta) {
            // a discrete lobe (ParamGradProbe::bsdf_sampled): both perturbed records are re-sampled with the same numbers and count only
            // if they land on the very direction of the primal sample
            DevBsdf bp, bm; f3 wp, wm; BsdfSample bp_, bm_;
            perturbed(bsdf, bp, bm);
            const bool okp = bsdf_sample(bp, refl, si.wi, s1, s2, bp_, wp);
            const bool okm = bsdf_sample(bm, refl, si.wi, s1, s2, bm_, wm);
            if (okp && okm && bp_.delta && bm_.delta && bp_.wo.x == bs.wo.x && bp_.wo.y == bs.wo.y && bp_.wo.z == bs.wo.z &&
                bm_.wo.x == bs.wo.x && bm_.wo.y == bs.wo.y && bm_.wo.z == bs.wo.z)
                r.dW = mk3((wp.x - wm.x) * i2h.x, (wp.y - wm.y) * i2h.y, (wp.z - wm.z) * i2h.z);
        }
    }
};

// Every camera sample is replayed through the fused step of nested scenes (the one that resolves textured parameters) and swept
// backwards:  b = delta Nc + W a,  a = delta E + invq b;  at a vertex whose record reads the slot from a bitmap
//   colours:    gg[c] = T'_c (delta_c dNc_c + a_c dW_c)
//   roughness:  g = sum_c T'_c (delta_c dNc_c + a_c dW_c), chained to the RGB texel by what resolve_textured applied: the luminance
//               weights where the kBsdfAlpha?Lum flag is set, else (1, 0, 0)
// is scattered over the footprint of the slot's lookup at the texture's grad_offset.
template <bool FLAT>
__global__ __launch_bounds__(kBlock) void k_adjoint_param_tex(const AdjointParams A) {
    extern __shared__ float4 smem[];
    const RenderParams &P = A.rp;
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    const int slot = A.pg_bsdf;
    for (uint64_t k = (uint64_t) blockIdx.x * kBlock + threadIdx.x; k < A.n_samples; k += (uint64_t) gridDim.x * kBlock) {
        PathState s; const f3 delta = adjoint_sample(A, k, s);
        if (delta.x == 0.0f && delta.y == 0.0f && delta.z == 0.0f) continue;       // every term below is proportional to delta
        VertexRecP rec[kAdjointMaxDepth];
        int n = 0;
        Counters c = { 0u, 0u, 0u, 0u };
        bool alive = true;
        while (alive && n < kAdjointMaxDepth) {
            ParamTexRecorder pr = { rec[n], P.sv, slot, A.pg_inv_2h };
            alive = bounce_step<FLAT, 0, true, true>(P, lds, s, c, pr);
            ++n;
        }
        f3 a = mk3(0.0f, 0.0f, 0.0f);
        for (int v = n - 1; v >= 0; --v) {
            const VertexRecP &r = rec[v];
            if (r.texel != kNoPrim) {
                const f3 Tp = r.T * r.invq;
                float gg[3] = { Tp.x * fmaf(delta.x, r.dNc.x, a.x * r.dW.x), Tp.y * fmaf(delta.y, r.dNc.y, a.y * r.dW.y),
                                Tp.z * fmaf(delta.z, r.dNc.z, a.z * r.dW.z) };
                if (slot == kTexAlphaU || slot == kTexAlphaV) {
                    const float g = (gg[0] + gg[1]) + gg[2];
                    gg[0] = r.lum ? 0.212671f * g : g; gg[1] = r.lum ? 0.715160f * g : 0.0f; gg[2] = r.lum ? 0.072169f * g : 0.0f;
                }
                // a sample whose derivative is not finite is dropped, as k_adjoint_param drops it
                if (isfinite(gg[0]) && isfinite(gg[1]) && isfinite(gg[2])) {
                    const DevTexture t = P.sv.textures[r.texture];
                    scatter_texel_grad(A.grad_tex, t, r.texel, r.w1, gg);
                }
            }
            const f3 b = mk3(fmaf(delta.x, r.Nc.x, r.W.x * a.x), fmaf(delta.y, r.Nc.y, r.W.y * a.y), fmaf(delta.z, r.Nc.z, r.W.z * a.z));
            a = mk3(delta.x * r.E.x + r.invq * b.x, delta.y * r.E.y + r.invq * b.y, delta.z * r.E.z + r.invq * b.z);
        }
    }
}

hipError_t launch_adjoint_param_tex(const AdjointParams &a, hipStream_t s) { return launch_adjoint_kernel<k_adjoint_param_tex<true>, k_adjoint_param_tex<false>>(a, s); }

// One map slot at one hit outside k_adjoint_param_tex -- the NEST forms of TangentProbe / ReverseProbe, which visit EVERY bound slot of a
// record in one replay -- is ParamTexRecorder itself on a vertex record of its own: its footprint and step rules (surface), its central
// difference (dvalue) and its rule for the sampled direction (bsdf_sampled) are called, not restated.
// Does the record `bsdf` (after resolve_textured) read q.slot from a bitmap at uv?  Fills q.r.texel / w1 / texture / lum and the step
MTS_DEV bool param_tex_hit(ParamTexRecorder &q, const DevBsdf &bsdf, f2 uv) {
    SurfaceInteraction si; si.uv = uv;
    q.r.texel = kNoPrim;
    q.surface(si, bsdf, mk3(0.0f, 0.0f, 0.0f), kNoPrim, uv, mk3(0.0f, 0.0f, 0.0f));
    return q.here;
}
// d(weight)/d(parameter) at the sampled direction: d(value) / pdf of a smooth lobe, the re-sampled difference of a discrete one
MTS_DEV f3 param_tex_dweight(ParamTexRecorder &q, const DevBsdf &bsdf, f3 refl, f3 wi, f3 wo, float pdf, bool delta, float s1, f2 s2) {
    SurfaceInteraction si; si.wi = wi;
    BsdfSample bs; bs.wo = wo; bs.pdf = pdf; bs.delta = delta;
    q.r.dW = mk3(0.0f, 0.0f, 0.0f);
    q.bsdf_sampled(q.sv, si, bsdf, refl, mk3(0.0f, 0.0f, 0.0f), bs, mk3(0.0f, 0.0f, 0.0f), s1, s2);
    return q.r.dW;
}
// A roughness reaches the RGB texel through what resolve_textured applied (the sweep of k_adjoint_param_tex): the luminance weights where
// the kBsdfAlpha?Lum flag is set, else channel 0.  gg: the per-channel gradient with respect to the slot's parameter
MTS_DEV void param_tex_chain(int slot, uint32_t lum, float gg[3]) {
    if (slot == kTexAlphaU || slot == kTexAlphaV) {
        const float g = (gg[0] + gg[1]) + gg[2];
        gg[0] = lum ? 0.212671f * g : g; gg[1] = lum ? 0.715160f * g : 0.0f; gg[2] = lum ? 0.072169f * g : 0.0f;
    }
}


// ---------------------------------------------------------------------------------------------
// Forward mode: the image of d(radiance)/d(t) along ONE tangent direction t over the scene parameters -- what ek.forward() leaves in
// ek.gradient(image) (docs/examples/10_inverse_rendering/forward_diff.py, docs/src/inverse_rendering/diff_render.rst:332-398).  A tangent
// is one direction, so one dual part (dthr = d throughput, dres = d radiance) beside the replayed path serves every parameter at once:
//   BSDF constants     d f / d t at the fixed directions = the central difference of the model code between the records plus[b] and
//                      minus[b] (theta +- eps t, built on the host: build_tangent_records), the rule of ParamGradProbe, discrete lobes included;
//   reflectance texels d refl = the bilinear lookup of the tangent texels over the footprint the step reports, chained through the closed
//                      forms of GeneralRecorder (bsdf_dvalue_drefl / bsdf_dweight_drefl);
//   emitter colours    radiance is linear in them: emission picked up adds (ew thr) dLe, an unoccluded emitter sample mis thr bv em_geo dLe
//                      with em_geo = spec / radiance from the factors r1, r2 and falloff (never a division by the radiance, which may be 0);
//   envmap texels      dLe = scale * the bilinear lookup of the tangent image over the footprint of envmap_lookup, at the two uses
//                      EnvGradProbe names; the sampling hierarchy is not differentiated.
// Russian roulette (path.cpp:137-141): thr' = thr rq with rq = 1 / q, q = min(hmax(thr) eta^2, .95).  Attached (the default, as the
// reference and k_adjoint / k_adjoint_tex): where q is not clamped, d rq = -rq^2 eta^2 d thr_c on the channel c that sets q -- the forward
// form of the `corr` term of those sweeps.  kForwardDetachRoulette: dthr *= rq only (ParamGradProbe::roulette).  Everything else is
// detached, as in the adjoints: directions, pdfs, lobe choices, MIS weights, the survival test.
// the fields of `cur` (after resolve_textured) that a texture wrote, copied into another copy of the same record
MTS_DEV void copy_textured(const DevBsdf &cur, DevBsdf &b) {
    if (!(cur.flags & kBsdfTexParams)) return;
    if (bsdf_param_texture(cur, kTexAlphaU)) b.alpha_u = cur.alpha_u;
    if (bsdf_param_texture(cur, kTexAlphaV)) b.alpha_v = cur.alpha_v;
    if (bsdf_param_texture(cur, kTexSpec)) { b.sr = cur.sr; b.sg = cur.sg; b.sb = cur.sb; }
    if (bsdf_param_texture(cur, kTexTrans)) { b.kr = cur.kr; b.kg = cur.kg; b.kb = cur.kb; }
}

template <bool NEST = false>
struct TangentProbe {
    static constexpr bool kFactoredEmitter = true, kMirrorTwoSided = false, kSamples = true;
    const ForwardParams &F;
    f3 dthr, dres;
    f3 thr0; float eta2;            // throughput and eta^2 on arrival (emission is picked up before roulette)
    const DevBsdf *cur; f3 refl0;   // the record and reflectance of the surface of this step
    int32_t rec; float inv_2h;      // its index; != 0: the record carries a BSDF tangent
    bool tex; f3 drefl;             // a bitmap reflectance with a texel tangent was looked up: d refl
    f3 dle;                         // d radiance of the emitter sample of this step (falloff, r1, r2 not applied)
    bool maps;                      // NEST: the record reads parameters from textures and there are texel tangents

    MTS_DEV static float em_geo(const SceneView &sv, const NeeTerms &t) {       // spec / radiance of the emitter sample (EmitterGradProbeS::em_geo)
        const float g = t.ds.delta ? t.ds.falloff * t.r1 : t.r1;
        return sv.n_emitters > 1u ? g * t.r2 : g;
    }
    MTS_DEV f3 emitter_tangent(uint32_t e) const {
        if (!F.em_tangent) return mk3(0.0f, 0.0f, 0.0f);
        const float *row = F.em_tangent + 3u * (size_t) e;
        return mk3(row[0], row[1], row[2]);
    }
    // envmap_lookup over the tangent image: the same footprint and arithmetic
    MTS_DEV f3 env_tangent(const DevEnvmap &e, float u, float v) const {
        if (!F.env_tangent) return mk3(0.0f, 0.0f, 0.0f);
        u *= (float) (e.w - 1); v *= (float) (e.h - 1);
        const uint32_t px = min((uint32_t) u, (uint32_t) (e.w - 2)), py = min((uint32_t) v, (uint32_t) (e.h - 2));
        const float w1x = u - (float) px, w1y = v - (float) py, w0x = 1.0f - w1x, w0y = 1.0f - w1y;
        const float *v00 = F.env_tangent + 3u * ((size_t) py * e.w + px), *v01 = v00 + 3u * (size_t) e.w;
        f3 r;
        { const float a = fmaf(w0x, v00[0], w1x * v00[3]), b = fmaf(w0x, v01[0], w1x * v01[3]); r.x = fmaf(w0y, a, w1y * b) * e.scale; }
        { const float a = fmaf(w0x, v00[1], w1x * v00[4]), b = fmaf(w0x, v01[1], w1x * v01[4]); r.y = fmaf(w0y, a, w1y * b) * e.scale; }
        { const float a = fmaf(w0x, v00[2], w1x * v00[5]), b = fmaf(w0x, v01[2], w1x * v01[5]); r.z = fmaf(w0y, a, w1y * b) * e.scale; }
        return r;
    }
    MTS_DEV void perturbed_refl(const SceneView &sv, const SurfaceInteraction &si, const DevBsdf &bp, const DevBsdf &bm, f3 &rp, f3 &rm) const {
        uint32_t tt; f2 tw;
        rp = eval_reflectance(sv, bp, si.uv, tt, tw); rm = eval_reflectance(sv, bm, si.uv, tt, tw);
    }
    // the record of this step in a perturbed table; NEST: its textured fields carry what resolve_textured looked up at the hit, bit for bit
    MTS_DEV DevBsdf side(const DevBsdf *table) const {
        DevBsdf b = table[rec];
        if constexpr (NEST) copy_textured(*cur, b);
        return b;
    }
    // NEST, slot `slot` of the record of this step: its footprint and step, and the tangent of its parameter -- the bilinear lookup of the
    // tangent texels over that footprint, per channel for a colour, through the luminance / channel-0 rule for a roughness
    MTS_DEV bool map_slot(const SurfaceInteraction &si, ParamTexRecorder &q, f3 &dt) const {
        if (!param_tex_hit(q, *cur, si.uv)) return false;
        const VertexRecP &m = q.r;
        const DevTexture t = q.sv.textures[m.texture];
        const float *tt = F.tex_tangent + t.grad_offset + 3u * (size_t) m.texel;
        const float w00 = (1.0f - m.w1.y) * (1.0f - m.w1.x), w10 = (1.0f - m.w1.y) * m.w1.x, w01 = m.w1.y * (1.0f - m.w1.x), w11 = m.w1.y * m.w1.x;
        float d[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) d[ch] = fmaf(w11, tt[3 * t.w + 3 + ch], fmaf(w01, tt[3 * t.w + ch], fmaf(w10, tt[3 + ch], w00 * tt[ch])));
        if (q.slot <= kTexAlphaV) d[0] = d[1] = d[2] = m.lum ? fmaf(0.072169f, d[2], fmaf(0.715160f, d[1], 0.212671f * d[0])) : d[0];
        dt = mk3(d[0], d[1], d[2]);
        return true;
    }
    // NEST: the map texels' part of d(value)/d(t) at wo_l (bs: of d(weight)/d(t) at the sampled direction instead): over every bound slot,
    // the slot's central difference (ParamTexRecorder's) times the tangent of its parameter
    MTS_DEV f3 map_dvalue(const SceneView &sv, const SurfaceInteraction &si, f3 wo_l, const BsdfSample *bs, float s1, f2 s2) const {
        f3 sum = mk3(0.0f, 0.0f, 0.0f);
#pragma unroll 1
        for (int slot = kTexAlphaU; slot <= kTexTrans; ++slot) {
            VertexRecP v; ParamTexRecorder q = { v, sv, slot, F.map_h };
            f3 dt;
            if (!map_slot(si, q, dt)) continue;
            const f3 dv = bs ? param_tex_dweight(q, *cur, refl0, si.wi, bs->wo, bs->pdf, bs->delta, s1, s2) : q.dvalue(*cur, refl0, si.wi, wo_l);
            sum = mk3(fmaf(dv.x, dt.x, sum.x), fmaf(dv.y, dt.y, sum.y), fmaf(dv.z, dt.z, sum.z));
        }
        return sum;
    }
    // d(value)/d(t) of the model at fixed directions: the central difference over the BSDF constants (ParamGradProbe::dvalue) ...
    MTS_DEV f3 dvalue(const SceneView &sv, const SurfaceInteraction &si, f3 wo_l) const {
        if (inv_2h == 0.0f) return mk3(0.0f, 0.0f, 0.0f);
        const DevBsdf bp = side(F.plus), bm = side(F.minus);
        f3 rp, rm, vp, vm; float pp, pm;
        perturbed_refl(sv, si, bp, bm, rp, rm);
        bsdf_eval_pdf(bp, rp, si.wi, wo_l, vp, pp);      // the model code itself (two-sided adapter included), no nesting
        bsdf_eval_pdf(bm, rm, si.wi, wo_l, vm, pm);
        return mk3((vp.x - vm.x) * inv_2h, (vp.y - vm.y) * inv_2h, (vp.z - vm.z) * inv_2h);
    }
    // ... + d: the chain through the textured reflectance, dr = d(value or weight)/d(refl) in closed form
    MTS_DEV f3 chain(f3 d, f3 dr) const { return mk3(fmaf(dr.x, drefl.x, d.x), fmaf(dr.y, drefl.y, d.y), fmaf(dr.z, drefl.z, d.z)); }
    template <int DEFER, bool GENERAL, bool NEST_> MTS_DEV void begin(const PathState &s) {
        static_assert(GENERAL && DEFER == 0 && NEST_ == NEST, "the forward-mode derivative rides on the general fused step of its scene");
        thr0 = s.thr; eta2 = s.eta * s.eta;
        cur = nullptr; rec = -1; inv_2h = 0.0f; tex = false;
        if constexpr (NEST) maps = false;
        refl0 = drefl = dle = mk3(0.0f, 0.0f, 0.0f);
    }
    MTS_DEV void pick_up(float ew, f3 le, f3 d_le) {
        dres = mk3(dres.x + ((ew * dthr.x) * le.x + (ew * thr0.x) * d_le.x), dres.y + ((ew * dthr.y) * le.y + (ew * thr0.y) * d_le.y),
                   dres.z + ((ew * dthr.z) * le.z + (ew * thr0.z) * d_le.z));
    }
    MTS_DEV void emitted(float ew, int32_t emitter, f3 le) { pick_up(ew, le, emitter_tangent((uint32_t) emitter)); }
    MTS_DEV void escaped(const SceneView &sv, const PathState &s, const DevEmitter &e, float ew, f3 le) {
        f3 d_le;
        if (e.pad0 == kEmitterEnvmap) {
            float u, v;
            env_dir_to_uv(mat3_apply(sv.envmap->to_local, s.d), u, v);
            d_le = env_tangent(*sv.envmap, u, v);
        } else d_le = emitter_tangent((uint32_t) sv.env_emitter);
        pick_up(ew, le, d_le);
    }
    MTS_DEV void roulette(f3 thr, float hm, float rq, bool free) {
        f3 d = dthr * rq;
        if (free && !(F.flags & kForwardDetachRoulette)) {
            const float dc = thr.x == hm ? dthr.x : (thr.y == hm ? dthr.y : dthr.z);
            const float drq = -((rq * rq) * eta2) * dc;
            d = mk3(fmaf(thr.x, drq, d.x), fmaf(thr.y, drq, d.y), fmaf(thr.z, drq, d.z));
        }
        dthr = d;
    }
    MTS_DEV void surface(const SurfaceInteraction &si, const DevBsdf &bsdf, f3 refl, uint32_t texel, f2 tw1, f3) {
        cur = &bsdf; refl0 = refl; rec = si.shape_rec.bsdf;
        inv_2h = F.inv_2h ? F.inv_2h[rec] : 0.0f;
        tex = F.tex_tangent != nullptr && texel != kNoPrim;
        if (tex) {          // the weights scatter_texel_grad hands the four texels
            const DevTexture t = F.rp.sv.textures[bsdf.texture];
            const float *tt = F.tex_tangent + t.grad_offset + 3u * (size_t) texel;
            const float w00 = (1.0f - tw1.y) * (1.0f - tw1.x), w10 = (1.0f - tw1.y) * tw1.x, w01 = tw1.y * (1.0f - tw1.x), w11 = tw1.y * tw1.x;
            float d[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) d[ch] = fmaf(w11, tt[3 * t.w + 3 + ch], fmaf(w01, tt[3 * t.w + ch], fmaf(w10, tt[3 + ch], w00 * tt[ch])));
            drefl = mk3(d[0], d[1], d[2]);
        }
        if constexpr (NEST) maps = F.tex_tangent != nullptr && (bsdf.flags & kBsdfTexParams) != 0u;
    }
    // the shadow ray is traced wherever the derivative may be non-zero, also where the radiance itself is 0
    MTS_DEV bool emitter_sample(const SceneView &sv, const DevBsdf &, f3, const NeeTerms &t) {
        dle = mk3(0.0f, 0.0f, 0.0f);
        if (sv.n_emitters != 0u) dle = t.kind == kEmitterEnvmap ? env_tangent(*sv.envmap, t.ds.uv.x, t.ds.uv.y) : emitter_tangent(t.ds.emitter);
        const bool lit = em_geo(sv, t) != 0.0f && (dle.x != 0.0f || dle.y != 0.0f || dle.z != 0.0f);
        if constexpr (NEST) if (maps) return true;
        return lit || inv_2h != 0.0f || tex || dthr.x != 0.0f || dthr.y != 0.0f || dthr.z != 0.0f;
    }
    // d(mis thr bv spec) with mis fixed: (dthr bv + thr dbv) spec + thr bv em_geo dLe
    MTS_DEV void unoccluded(const SceneView &sv, const SurfaceInteraction &si, f3 thr, const NeeTerms &t) {
        f3 dbv = dvalue(sv, si, t.wo);
        if (tex) dbv = chain(dbv, bsdf_dvalue_drefl(*cur, refl0, t.wi, t.wo));
        if constexpr (NEST) if (maps) dbv = dbv + map_dvalue(sv, si, t.wo, nullptr, 0.0f, f2{ 0.0f, 0.0f });
        const float g = em_geo(sv, t);
        const f3 ds = mk3(g * dle.x, g * dle.y, g * dle.z);
        dres = mk3(dres.x + ((t.mis * fmaf(dthr.x, t.bv.x, thr.x * dbv.x)) * t.spec.x + ((t.mis * thr.x) * t.bv.x) * ds.x),
                   dres.y + ((t.mis * fmaf(dthr.y, t.bv.y, thr.y * dbv.y)) * t.spec.y + ((t.mis * thr.y) * t.bv.y) * ds.y),
                   dres.z + ((t.mis * fmaf(dthr.z, t.bv.z, thr.z * dbv.z)) * t.spec.z + ((t.mis * thr.z) * t.bv.z) * ds.z));
    }
    // d(thr weight) = dthr weight + thr dweight;  dweight = d(value)/d(t) / pdf at the sampled direction (ParamGradProbe::bsdf_sampled)
    MTS_DEV void bsdf_sampled(const SceneView &sv, const SurfaceInteraction &si, const DevBsdf &bsdf, f3 refl, f3 thr, const BsdfSample &bs, f3 weight, float s1, f2 s2) {
        f3 dw = mk3(0.0f, 0.0f, 0.0f);
        if (inv_2h != 0.0f && !bs.delta && bs.pdf > 0.0f) {
            const f3 dv = dvalue(sv, si, bs.wo);
            const float ip = rcp(bs.pdf);
            dw = mk3(dv.x * ip, dv.y * ip, dv.z * ip);
        } else if (inv_2h != 0.0f && bs.delta) {
            // a discrete lobe: re-sampled with the perturbed records and the same numbers; counts only if both land on the primal direction
            const DevBsdf bp = side(F.plus), bm = side(F.minus);
            f3 rp, rm, wp, wm; BsdfSample bp_, bm_;
            perturbed_refl(sv, si, bp, bm, rp, rm);
            const bool okp = bsdf_sample(bp, rp, si.wi, s1, s2, bp_, wp);
            const bool okm = bsdf_sample(bm, rm, si.wi, s1, s2, bm_, wm);
            if (okp && okm && bp_.delta && bm_.delta && bp_.wo.x == bs.wo.x && bp_.wo.y == bs.wo.y && bp_.wo.z == bs.wo.z &&
                bm_.wo.x == bs.wo.x && bm_.wo.y == bs.wo.y && bm_.wo.z == bs.wo.z)
                dw = mk3((wp.x - wm.x) * inv_2h, (wp.y - wm.y) * inv_2h, (wp.z - wm.z) * inv_2h);
        }
        if (tex) dw = chain(dw, bsdf_dweight_drefl(bsdf, refl, si.wi, bs));
        if constexpr (NEST) if (maps) dw = dw + map_dvalue(sv, si, bs.wo, &bs, s1, s2);
        dthr = mk3(fmaf(dthr.x, weight.x, thr.x * dw.x), fmaf(dthr.y, weight.y, thr.y * dw.y), fmaf(dthr.z, weight.z, thr.z * dw.z));
    }
};

// One thread replays one camera sample with the PCG32 stream of the primal pass and writes (dR, dG, dB, a) and the film position into
// its slot of the sample stream (generate_path / store_result), so that the film kernels splat the stream unchanged.  a = the primal
// alpha, or -1 where the primal pass drops the sample (non-finite radiance: the store_xyz == 2 rule), so that the A and W channels of
// the derivative film equal those of the primal film.  A derivative that is not finite while the radiance is finite is written as
// zero and keeps its weight (the isfinite(g) rule of k_adjoint_param).
template <bool FLAT, bool NEST = false>
__global__ __launch_bounds__(kBlock) void k_forward(const ForwardParams F) {
    extern __shared__ float4 smem[];
    const RenderParams &P = F.rp;
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    const uint32_t spp = (uint32_t) P.spp;
    for (uint64_t k = (uint64_t) blockIdx.x * kBlock + threadIdx.x; k < F.n_samples; k += (uint64_t) gridDim.x * kBlock) {
        const uint64_t ordinal = P.first_ordinal + k;
        PathState s;
        generate_path(P, ordinal, (uint32_t) (ordinal / spp), (uint32_t) (ordinal % spp), s);
        TangentProbe<NEST> tp = { F };
        tp.dthr = tp.dres = mk3(0.0f, 0.0f, 0.0f);
        Counters c = { 0u, 0u, 0u, 0u };
        while (bounce_step<FLAT, 0, true, NEST>(P, lds, s, c, tp)) { }
        float alpha = (s.flags & 1u) ? 1.0f : 0.0f;
        if (P.store_xyz && !(isfinite(s.res.x) && isfinite(s.res.y) && isfinite(s.res.z))) alpha = -1.0f;
        f3 d = tp.dres;
        if (!(isfinite(d.x) && isfinite(d.y) && isfinite(d.z))) d = mk3(0.0f, 0.0f, 0.0f);
        P.out_rgba[s.ordinal] = make_float4(d.x, d.y, d.z, alpha);
    }
}

static hipError_t launch_forward_nest(const ForwardParams &f, hipStream_t s);      // at the end of the file, with the kernels it instantiates
hipError_t launch_forward(const ForwardParams &f, bool nest, hipStream_t s) {
    return nest ? launch_forward_nest(f, s) : launch_adjoint_kernel<k_forward<true, false>, k_forward<false, false>>(f, s);
}

// ---------------------------------------------------------------------------------------------
// Reverse mode: the transpose of k_forward.  One replay of every camera sample with one dLoss/dImage gives the gradient of every parameter
// k_forward takes a tangent for, with k_forward's conventions term for term (everything detached but the Russian-roulette factor; the
// detach flag holds that fixed too), so that <dL, J t> of a forward render equals <J^T dL, t> here up to the order of the sums:
//   emitter colours    need no suffix of the path: emission picked up adds delta (ew T) to the emitter's row, an unoccluded emitter sample
//                      delta (mis T' bv em_geo), em_geo from r1, r2 and the falloff as TangentProbe::em_geo forms it;
//   envmap texels      scattered at the two sites of EnvGradProbe;
//   reflectance texels the sweep of k_adjoint_tex over the recorded vertices, bsdf_dvalue_drefl / bsdf_dweight_drefl and scatter_texel_grad;
//   BSDF constants     at a vertex whose record has wanted slots, slot j adds  g_j += sum_c T'_c (delta_c dNc_jc + a_c dW_jc)  with
//                      dNc_j = (mis spec) dbv_j, dW_j = dv_j / pdf, both the central difference of bsdf_eval_pdf between the slot's pair
//                      at the recorded directions; a discrete lobe is re-sampled with s1, s2 (ParamGradProbe::bsdf_sampled).
// RECORD = false (no BSDF scalar, no texel wanted) keeps no vertices and runs at any depth.  RECORD = true is ONE replay with a wider
// record than VertexRecG: besides T, invq, E, Nc, W and the texel terms it keeps what the slot differences need at the sweep -- wi, the two
// wo, the pdf and delta flag, s1 / s2, the reflectance, mis spec and the record index (184 bytes per vertex, 16 vertices per lane).
// Sums per slot and per emitter go to LDS bins of the workgroup (kReverseSlotBins, kReverseEmitterBins), flushed once at the end.
struct VertexRecR {
    f3 T; float invq;
    f3 E; float eta2;
    f3 Nc; int32_t rr_channel;      // channel that sets q (-1: none / q clamped / roulette detached)
    f3 W; uint32_t texel;           // kNoPrim: no texel gradient at this vertex
    f3 dNc; int32_t texture;        // d / d(refl), as VertexRecG
    f3 dW; f2 w1;
    f3 wi; int32_t rec;             // record of the surface if it has wanted slots, else -1
    f3 wo_e; float pdf;             // local direction of the emitter sample; pdf of the BSDF sample
    f3 wo_s; float s1;
    f3 refl; uint32_t flags;        // 1: the emitter sample was unoccluded; 2: a BSDF sample was drawn; 4: from a discrete lobe
    f3 ms; f2 s2;                   // mis * spec of the emitter sample
};

// NEST (textured BSDF parameters): the sweep re-resolves the record and recomputes the footprints of its maps from the uv of the hit
struct VertexRecRN : VertexRecR { f2 uv; };

// the float of DevBsdf at offset `f` (in floats) set to v: a switch over the fields bsdf_param_fields can name, so the record stays in registers
MTS_DEV void reverse_patch(DevBsdf &b, uint32_t f, float v) {
    switch (f) {
    case offsetof(DevBsdf, r) / 4: b.r = v; break; case offsetof(DevBsdf, g) / 4: b.g = v; break; case offsetof(DevBsdf, b) / 4: b.b = v; break;
    case offsetof(DevBsdf, sr) / 4: b.sr = v; break; case offsetof(DevBsdf, sg) / 4: b.sg = v; break; case offsetof(DevBsdf, sb) / 4: b.sb = v; break;
    case offsetof(DevBsdf, er) / 4: b.er = v; break; case offsetof(DevBsdf, eg) / 4: b.eg = v; break; case offsetof(DevBsdf, eb) / 4: b.eb = v; break;
    case offsetof(DevBsdf, kr) / 4: b.kr = v; break; case offsetof(DevBsdf, kg) / 4: b.kg = v; break; case offsetof(DevBsdf, kb) / 4: b.kb = v; break;
    case offsetof(DevBsdf, alpha_u) / 4: b.alpha_u = v; break; case offsetof(DevBsdf, alpha_v) / 4: b.alpha_v = v; break;
    default: break;
    }
}

// the workgroup's emitter bins: one __shared__ array that the probe and the kernel name directly, so that the sums are LDS float atomics
// (a pointer kept in the probe reaches the step as a generic address)
MTS_DEV float *reverse_emitter_bins() {
    __shared__ float s_em[3 * kReverseEmitterBins];
    return s_em;
}

template <bool RECORD, bool NEST = false>
struct ReverseProbe {
    static constexpr bool kFactoredEmitter = true, kMirrorTwoSided = false, kSamples = true;
    using Rec = std::conditional_t<NEST, VertexRecRN, VertexRecR>;
    const ReverseParams &R;
    f3 delta;                       // dLoss/dRadiance of the sample
    Rec *r;                         // RECORD: the vertex of this step
    f3 thr0;                        // throughput on arrival (emission is picked up before roulette)
    const DevBsdf *cur; f3 refl0;   // the record and reflectance of the surface of this step
    bool tex, slotted;              // a texel gradient / slots of the surface's record are wanted here

    // delta * c added to the row of emitter e; a term that is not finite adds nothing
    MTS_DEV void add_emitter(uint32_t e, f3 c) const {
        const float v[3] = { delta.x * c.x, delta.y * c.y, delta.z * c.z };
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            if (v[ch] != 0.0f && isfinite(v[ch])) {
                if (e < kReverseEmitterBins) atomicAdd(&reverse_emitter_bins()[3u * e + (uint32_t) ch], v[ch]);
                else atomicAdd(R.grad_emitter + 3u * (size_t) e + ch, v[ch]);
            }
    }
    // delta * coeff scattered over the footprint of envmap_lookup (EnvGradProbe::add), unless it is not finite
    MTS_DEV void add_envmap(const DevEnvmap &e, float u, float v, f3 coeff) const {
        if (isfinite(delta.x * coeff.x) && isfinite(delta.y * coeff.y) && isfinite(delta.z * coeff.z)) EnvGradProbe{ delta, R.grad_env }.add(e, u, v, coeff);
    }
    template <int DEFER, bool GENERAL, bool NEST_> MTS_DEV void begin(const PathState &s) {
        static_assert(GENERAL && DEFER == 0 && NEST_ == NEST, "the reverse-mode derivative rides on the general fused step of its scene");
        thr0 = s.thr; cur = nullptr; tex = slotted = false; refl0 = mk3(0.0f, 0.0f, 0.0f);
        if (RECORD) {
            r->T = s.thr; r->invq = 1.0f; r->eta2 = s.eta * s.eta; r->rr_channel = -1;
            r->E = r->Nc = r->W = r->dNc = r->dW = mk3(0.0f, 0.0f, 0.0f);
            r->texel = kNoPrim; r->texture = -1; r->w1.x = r->w1.y = 0.0f;
            r->rec = -1; r->flags = 0u;
        }
    }
    MTS_DEV void emitted(float ew, int32_t emitter, f3 le) {
        if (R.grad_emitter) add_emitter((uint32_t) emitter, mk3(ew * thr0.x, ew * thr0.y, ew * thr0.z));
        if (RECORD) r->E = mk3(ew * le.x, ew * le.y, ew * le.z);
    }
    MTS_DEV void escaped(const SceneView &sv, const PathState &s, const DevEmitter &e, float ew, f3 le) {
        const f3 c = mk3(ew * s.thr.x, ew * s.thr.y, ew * s.thr.z);
        if (e.pad0 == kEmitterEnvmap) {
            if (R.grad_env) {
                float u, v;
                env_dir_to_uv(mat3_apply(sv.envmap->to_local, s.d), u, v);
                add_envmap(*sv.envmap, u, v, c);
            }
        } else if (R.grad_emitter) add_emitter((uint32_t) sv.env_emitter, c);
        if (RECORD) r->E = mk3(ew * le.x, ew * le.y, ew * le.z);
    }
    MTS_DEV void roulette(f3 thr, float hm, float rq, bool free) {
        if (RECORD) {
            r->invq = rq;
            if (free && !(R.flags & kReverseDetachRoulette)) r->rr_channel = thr.x == hm ? 0 : (thr.y == hm ? 1 : 2);
        }
    }
    MTS_DEV void surface(const SurfaceInteraction &si, const DevBsdf &bsdf, f3 refl, uint32_t texel, f2 tw1, f3) {
        cur = &bsdf; refl0 = refl;
        if (RECORD) {
            tex = R.grad_tex != nullptr && texel != kNoPrim;
            if (tex) { r->texel = texel; r->w1 = tw1; r->texture = bsdf.texture; }
            const int32_t b = si.shape_rec.bsdf;
            slotted = R.slot_range != nullptr && R.slot_range[b + 1] > R.slot_range[b];
            // NEST: the texels of the record's maps are wanted -- the vertex keeps what their central differences need, as for a slot
            if constexpr (NEST) { slotted = slotted || (R.grad_tex != nullptr && (bsdf.flags & kBsdfTexParams) != 0u); r->uv = si.uv; }
            if (slotted) { r->rec = b; r->wi = si.wi; r->refl = refl; }
        }
    }
    // the shadow ray is traced wherever a gradient may be non-zero, also where the radiance itself is 0
    MTS_DEV bool emitter_sample(const SceneView &sv, const DevBsdf &, f3, const NeeTerms &t) {
        const bool lit = TangentProbe<>::em_geo(sv, t) != 0.0f && (t.kind == kEmitterEnvmap ? R.grad_env != nullptr : R.grad_emitter != nullptr);
        // RECORD: Nc feeds the suffix adjoint of EARLIER vertices, in channels where the throughput here may be 0 (GeneralRecorder)
        const bool nc = (t.mis * t.bv.x) * t.spec.x != 0.0f || (t.mis * t.bv.y) * t.spec.y != 0.0f || (t.mis * t.bv.z) * t.spec.z != 0.0f;
        return lit || (RECORD && (tex || slotted || nc));
    }
    MTS_DEV void unoccluded(const SceneView &sv, const SurfaceInteraction &, f3 thr, const NeeTerms &t) {
        const float g = TangentProbe<>::em_geo(sv, t);
        if (g != 0.0f) {
            const f3 c = mk3(((t.mis * thr.x) * t.bv.x) * g, ((t.mis * thr.y) * t.bv.y) * g, ((t.mis * thr.z) * t.bv.z) * g);
            if (t.kind == kEmitterEnvmap) { if (R.grad_env) add_envmap(*sv.envmap, t.ds.uv.x, t.ds.uv.y, c); }
            else if (R.grad_emitter) add_emitter(t.ds.emitter, c);
        }
        if (RECORD) {
            r->Nc = mk3((t.mis * t.bv.x) * t.spec.x, (t.mis * t.bv.y) * t.spec.y, (t.mis * t.bv.z) * t.spec.z);
            if (tex) {
                const f3 dbv = bsdf_dvalue_drefl(*cur, refl0, t.wi, t.wo);
                r->dNc = mk3((t.mis * dbv.x) * t.spec.x, (t.mis * dbv.y) * t.spec.y, (t.mis * dbv.z) * t.spec.z);
            }
            if (slotted) { r->wo_e = t.wo; r->ms = mk3(t.mis * t.spec.x, t.mis * t.spec.y, t.mis * t.spec.z); r->flags |= 1u; }
        }
    }
    MTS_DEV void bsdf_sampled(const SceneView &, const SurfaceInteraction &si, const DevBsdf &bsdf, f3 refl, f3, const BsdfSample &bs, f3 weight, float s1, f2 s2) {
        if (RECORD) {
            r->W = weight;
            if (tex) r->dW = bsdf_dweight_drefl(bsdf, refl, si.wi, bs);
            if (slotted) { r->wo_s = bs.wo; r->pdf = bs.pdf; r->s1 = s1; r->s2 = s2; r->flags |= bs.delta ? 6u : 2u; }
        }
    }
};

// dNc and dW of one slot at a recorded vertex: the central difference of the model code between the slot's pair
MTS_DEV void reverse_slot_terms(const DevBsdf &base, const ReverseSlot &sl, const VertexRecR &r, f3 &dnc, f3 &dw) {
    DevBsdf bp = base, bm = base;
    reverse_patch(bp, sl.f0, sl.plus); reverse_patch(bm, sl.f0, sl.minus);
    if (sl.f1 != sl.f0) { reverse_patch(bp, sl.f1, sl.plus); reverse_patch(bm, sl.f1, sl.minus); }
    // eval_reflectance of the perturbed records: their own constant, or the texel the primal record looked up
    const f3 rp = base.texture < 0 ? mk3(bp.r, bp.g, bp.b) : r.refl, rm = base.texture < 0 ? mk3(bm.r, bm.g, bm.b) : r.refl;
    dnc = dw = mk3(0.0f, 0.0f, 0.0f);
    if (r.flags & 1u) {
        f3 vp, vm; float pp, pm;
        bsdf_eval_pdf(bp, rp, r.wi, r.wo_e, vp, pp);
        bsdf_eval_pdf(bm, rm, r.wi, r.wo_e, vm, pm);
        dnc = mk3(r.ms.x * ((vp.x - vm.x) * sl.inv_2h), r.ms.y * ((vp.y - vm.y) * sl.inv_2h), r.ms.z * ((vp.z - vm.z) * sl.inv_2h));
    }
    if ((r.flags & 6u) == 2u && r.pdf > 0.0f) {
        f3 vp, vm; float pp, pm;
        bsdf_eval_pdf(bp, rp, r.wi, r.wo_s, vp, pp);
        bsdf_eval_pdf(bm, rm, r.wi, r.wo_s, vm, pm);
        const float ip = rcp(r.pdf);
        dw = mk3(((vp.x - vm.x) * sl.inv_2h) * ip, ((vp.y - vm.y) * sl.inv_2h) * ip, ((vp.z - vm.z) * sl.inv_2h) * ip);
    } else if ((r.flags & 6u) == 6u) {
        // a discrete lobe: re-sampled with the perturbed records and the same numbers; counts only if both land on the primal direction
        f3 wp, wm; BsdfSample bp_, bm_;
        const bool okp = bsdf_sample(bp, rp, r.wi, r.s1, r.s2, bp_, wp);
        const bool okm = bsdf_sample(bm, rm, r.wi, r.s1, r.s2, bm_, wm);
        if (okp && okm && bp_.delta && bm_.delta && bp_.wo.x == r.wo_s.x && bp_.wo.y == r.wo_s.y && bp_.wo.z == r.wo_s.z &&
            bm_.wo.x == r.wo_s.x && bm_.wo.y == r.wo_s.y && bm_.wo.z == r.wo_s.z)
            dw = mk3((wp.x - wm.x) * sl.inv_2h, (wp.y - wm.y) * sl.inv_2h, (wp.z - wm.z) * sl.inv_2h);
    }
}

// dNc and dW of one map slot at a recorded vertex of a NEST replay: the slot's central difference (ParamTexRecorder's) at the recorded
// directions.  `base` is the record re-resolved at the vertex's uv, q the recorder after param_tex_hit
MTS_DEV void reverse_map_terms(const DevBsdf &base, ParamTexRecorder &q, const VertexRecR &r, f3 &dnc, f3 &dw) {
    dnc = dw = mk3(0.0f, 0.0f, 0.0f);
    if (r.flags & 1u) {
        const f3 dv = q.dvalue(base, r.refl, r.wi, r.wo_e);
        dnc = mk3(r.ms.x * dv.x, r.ms.y * dv.y, r.ms.z * dv.z);
    }
    if (r.flags & 2u) dw = param_tex_dweight(q, base, r.refl, r.wi, r.wo_s, r.pdf, (r.flags & 4u) != 0u, r.s1, r.s2);
}

template <bool FLAT, bool RECORD, bool NEST = false>
__global__ __launch_bounds__(kBlock) void k_reverse(const ReverseParams R) {
    extern __shared__ float4 smem[];
    const RenderParams &P = R.rp;
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    float *const s_em = reverse_emitter_bins();
    __shared__ float s_slot[RECORD ? kReverseSlotBins : 1u];
    for (uint32_t i = threadIdx.x; i < 3u * kReverseEmitterBins; i += kBlock) s_em[i] = 0.0f;
    for (uint32_t i = threadIdx.x; i < (RECORD ? kReverseSlotBins : 1u); i += kBlock) s_slot[i] = 0.0f;
    __syncthreads();
    for (uint64_t k = (uint64_t) blockIdx.x * kBlock + threadIdx.x; k < R.n_samples; k += (uint64_t) gridDim.x * kBlock) {
        PathState s; const f3 delta = adjoint_sample(R, k, s);
        if (delta.x == 0.0f && delta.y == 0.0f && delta.z == 0.0f) continue;       // every term below is proportional to delta
        Counters c = { 0u, 0u, 0u, 0u };
        ReverseProbe<RECORD, NEST> pr = { R, delta, nullptr };
        if constexpr (!RECORD) {
            while (bounce_step<FLAT, 0, true, NEST>(P, lds, s, c, pr)) { }
        } else {
        typename ReverseProbe<RECORD, NEST>::Rec rec[kAdjointMaxDepth];
        int n = 0;
        bool alive = true;
        while (alive && n < kAdjointMaxDepth) { pr.r = &rec[n]; alive = bounce_step<FLAT, 0, true, NEST>(P, lds, s, c, pr); ++n; }
        const Geo<FLAT> geo{ P.sv, lds };
        f3 a = mk3(0.0f, 0.0f, 0.0f);
        for (int v = n - 1; v >= 0; --v) {
            const auto &r = rec[v];
            const f3 Tp = r.T * r.invq;
            if (r.texel != kNoPrim) {
                const float gg[3] = { Tp.x * fmaf(delta.x, r.dNc.x, a.x * r.dW.x), Tp.y * fmaf(delta.y, r.dNc.y, a.y * r.dW.y),
                                      Tp.z * fmaf(delta.z, r.dNc.z, a.z * r.dW.z) };
                if (isfinite(gg[0]) && isfinite(gg[1]) && isfinite(gg[2])) {
                    const DevTexture t = P.sv.textures[r.texture];
                    scatter_texel_grad(R.grad_tex, t, r.texel, r.w1, gg);
                }
            }
            if (r.rec >= 0) {
                DevBsdf base = geo.bsdf((uint32_t) r.rec);
                uint32_t j0, j1;
                if constexpr (NEST) {
                    // the working record of the hit, bit for bit: the slots' pairs carry the looked-up values in their textured fields
                    resolve_textured(P.sv, base, r.uv);
                    j0 = R.slot_range ? R.slot_range[r.rec] : 0u; j1 = R.slot_range ? R.slot_range[r.rec + 1] : 0u;
                    // every bound slot's T' (delta dNc + a dW) goes to the texels of its map
                    if (R.grad_tex && (base.flags & kBsdfTexParams)) {
#pragma unroll 1
                        for (int slot = kTexAlphaU; slot <= kTexTrans; ++slot) {
                            VertexRecP m; ParamTexRecorder q = { m, P.sv, slot, R.map_h };
                            if (!param_tex_hit(q, base, r.uv)) continue;
                            f3 dnc, dw;
                            reverse_map_terms(base, q, r, dnc, dw);
                            float gg[3] = { Tp.x * fmaf(delta.x, dnc.x, a.x * dw.x), Tp.y * fmaf(delta.y, dnc.y, a.y * dw.y),
                                            Tp.z * fmaf(delta.z, dnc.z, a.z * dw.z) };
                            param_tex_chain(slot, m.lum, gg);
                            if (isfinite(gg[0]) && isfinite(gg[1]) && isfinite(gg[2])) {
                                const DevTexture t = P.sv.textures[m.texture];
                                scatter_texel_grad(R.grad_tex, t, m.texel, m.w1, gg);
                            }
                        }
                    }
                } else { j0 = R.slot_range[r.rec]; j1 = R.slot_range[r.rec + 1]; }
                for (uint32_t j = j0; j < j1; ++j) {
                    const ReverseSlot sl = R.slots[j];
                    f3 dnc, dw;
                    reverse_slot_terms(base, sl, r, dnc, dw);
                    const float g = fmaf(Tp.z, fmaf(delta.z, dnc.z, a.z * dw.z), fmaf(Tp.y, fmaf(delta.y, dnc.y, a.y * dw.y), Tp.x * fmaf(delta.x, dnc.x, a.x * dw.x)));
                    if (g != 0.0f && isfinite(g)) {
                        if (j < kReverseSlotBins) atomicAdd(&s_slot[j], g);
                        else atomicAdd(R.grad_bsdf + sl.out, g);
                    }
                }
            }
            const f3 b = mk3(fmaf(delta.x, r.Nc.x, r.W.x * a.x), fmaf(delta.y, r.Nc.y, r.W.y * a.y), fmaf(delta.z, r.Nc.z, r.W.z * a.z));
            a = mk3(delta.x * r.E.x + r.invq * b.x, delta.y * r.E.y + r.invq * b.y, delta.z * r.E.z + r.invq * b.z);
            if (r.rr_channel >= 0) {
                const float corr = ((r.invq * r.invq) * r.eta2) * (b.x * r.T.x + b.y * r.T.y + b.z * r.T.z);
                if (r.rr_channel == 0) a.x -= corr; else if (r.rr_channel == 1) a.y -= corr; else a.z -= corr;
            }
        }
        }
    }
    __syncthreads();
    if (R.grad_emitter)
        for (uint32_t i = threadIdx.x; i < 3u * min(P.sv.n_emitters, kReverseEmitterBins); i += kBlock)
            if (s_em[i] != 0.0f) atomicAdd(R.grad_emitter + i, s_em[i]);
    if (RECORD && R.grad_bsdf)
        for (uint32_t i = threadIdx.x; i < min(R.n_slots, kReverseSlotBins); i += kBlock)
            if (s_slot[i] != 0.0f) atomicAdd(R.grad_bsdf + R.slots[i].out, s_slot[i]);
}

static hipError_t launch_reverse_nest(const ReverseParams &r, bool record, hipStream_t s);
hipError_t launch_reverse(const ReverseParams &r, bool record, bool nest, hipStream_t s) {
    if (nest) return launch_reverse_nest(r, record, s);
    return record ? launch_adjoint_kernel<k_reverse<true, true, false>, k_reverse<false, true, false>>(r, s)
                  : launch_adjoint_kernel<k_reverse<true, false, false>, k_reverse<false, false, false>>(r, s);
}

// ---------------------------------------------------------------------------------------------
// (Last in the file, as k_adjoint_param_tex once was and for the same reason: the six kernels below are instantiated here, after every
// other kernel of the file, so that the assembler's function and long-branch label numbers of all the others stay what they were.)
// Scenes with textured BSDF parameters (MTSAMD_FORWARD_PARAM_TEXTURES / MTSAMD_REVERSE_PARAM_TEXTURES): the forward and reverse renders
// on the fused step that resolves the maps at the hit, NEST = true.  Constants: plus / minus / the slots' pairs carry the looked-up values
// in their textured fields (TangentProbe::side, the re-resolved `base` of the sweep).  Map texels: every bound slot of the record of a hit
// is one ParamTexRecorder -- its footprint, step, central difference and discrete-lobe rule -- times the tangent texels looked up over
// the slot's footprint (forward), or scattered over it (reverse); the roulette factor is attached as for every other family.
static hipError_t launch_forward_nest(const ForwardParams &f, hipStream_t s) { return launch_adjoint_kernel<k_forward<true, true>, k_forward<false, true>>(f, s); }
static hipError_t launch_reverse_nest(const ReverseParams &r, bool record, hipStream_t s) {
    return record ? launch_adjoint_kernel<k_reverse<true, true, true>, k_reverse<false, true, true>>(r, s)
                  : launch_adjoint_kernel<k_reverse<true, false, true>, k_reverse<false, false, true>>(r, s);
}

// ---------------------------------------------------------------------------------------------
// Scenes with blendbsdf / mask records (MTSAMD_FORWARD_NESTED / MTSAMD_REVERSE_NESTED), after everything else for the reason above.  The
// probes derive from the NEST = true probes (such a scene has no textured parameters, so their map code is idle) and ride on
// bounce_step<FLAT, 0, true, true>, the step that resolves the nest in the primal render; at a plain record they ARE their base.  At a
// blend / mask record, with w the clamped weight of the hit and dw the tangent of the raw value where 0 <= raw <= 1 (else 0):
//   blendbsdf, evaluated       df = (1 - w) df0 + w df1 + dw (f1 - f0)
//   ... sampled, child i       dW = dW_i + W_i dw s,   s = +1 / w for bsdf_1, -1 / (1 - w) for bsdf_0
//   mask, evaluated            df = w df_c + dw f_c
//   ... sampled                child lobe dW = dW_c + W_c dw / w;   null lobe (W = 1) dW = -dw / (1 - w)
// df_i / dW_i are the child's existing rules on ITS row of the tables: the central difference between plus[i] and minus[i] (a discrete
// lobe re-sampled with the rescaled sample1 the primal handed the child), and the texel chain of a bitmap reflectance.  s is the
// derivative of the selection probability over itself: the probability is a pdf, detached in the denominator and attached in the
// integrand, as plastic's lobe choice is.  Detached as everywhere: directions, lobe and child choices, pdfs, MIS weights, the rescaled
// sample1.  A lobe of probability 0 is reached at sample1 == 0 only; s is infinite there and the isfinite rule drops the term.
struct NestAt { int kind; uint32_t n0, n1; bool two, lum, open; float w; };      // open: 0 <= raw weight <= 1, where d(clamp) = 1
// nest_info's arithmetic on the value the record's weight reads
MTS_DEV NestAt nest_at(const DevBsdf &b, f3 v) {
    NestAt n;
    n.kind = b.type; n.n0 = b.nested0; n.n1 = b.nested1; n.two = (b.flags & kBsdfTwoSided) != 0u; n.lum = (b.flags & kBsdfWeightLum) != 0u;
    const float raw = n.lum ? fmaf(0.072169f, v.z, fmaf(0.715160f, v.y, 0.212671f * v.x)) : v.x;
    n.open = raw >= 0.0f && raw <= 1.0f;
    n.w = fminf(fmaxf(raw, 0.0f), 1.0f);
    return n;
}
// The lobe surface_bsdf_sample took with sample1: k = 0 / 1: child n0 / n1, with the sample1 it was handed; k = 2: the null lobe of a
// mask; k = -1: none (a NaN sample).  s = d(selection probability) / d(w) / (selection probability)
struct NestLobe { int k; float s1, s; };
MTS_DEV NestLobe nest_lobe(const NestAt &n, float sample1) {
    NestLobe l = { -1, sample1, 0.0f };
    const float w = n.w;
    if (n.kind == kBsdfBlend) {
        if (sample1 > w) { l.k = 0; l.s1 = (sample1 - w) / (1.0f - w); l.s = -1.0f / (1.0f - w); }
        else if (sample1 <= w) { l.k = 1; l.s1 = sample1 / w; l.s = 1.0f / w; }
    } else if (sample1 < w) { l.k = 0; l.s1 = sample1 / w; l.s = 1.0f / w; }
    else { l.k = 2; l.s = -1.0f / (1.0f - w); }
    return l;
}
// the bilinear lookup of the tangent texels over a footprint (TangentProbe::surface)
MTS_DEV f3 texel_tangent(const float *tex_tangent, const DevTexture &t, uint32_t texel, f2 tw1) {
    const float *tt = tex_tangent + t.grad_offset + 3u * (size_t) texel;
    const float w00 = (1.0f - tw1.y) * (1.0f - tw1.x), w10 = (1.0f - tw1.y) * tw1.x, w01 = tw1.y * (1.0f - tw1.x), w11 = tw1.y * tw1.x;
    float d[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) d[ch] = fmaf(w11, tt[3 * t.w + 3 + ch], fmaf(w01, tt[3 * t.w + ch], fmaf(w10, tt[3 + ch], w00 * tt[ch])));
    return mk3(d[0], d[1], d[2]);
}

struct NestedTangentProbe : TangentProbe<true> {
    using Base = TangentProbe<true>;
    NestAt nh;          // kind 0: the record of this step is a plain one
    f2 uv; float dwt;   // the hit's uv; the tangent of the weight at the hit

    // central difference of child record c at (wi, wo) between its pair, d(value)/d(t) of the constants
    MTS_DEV f3 child_dvalue(const SceneView &sv, uint32_t c, f3 wi, f3 wo) const {
        const float i2h = F.inv_2h ? F.inv_2h[c] : 0.0f;
        if (i2h == 0.0f) return mk3(0.0f, 0.0f, 0.0f);
        const DevBsdf bp = F.plus[c], bm = F.minus[c];
        uint32_t tt; f2 tw; f3 vp, vm; float pp, pm;
        const f3 rp = eval_reflectance(sv, bp, uv, tt, tw), rm = eval_reflectance(sv, bm, uv, tt, tw);
        bsdf_eval_pdf(bp, rp, wi, wo, vp, pp);
        bsdf_eval_pdf(bm, rm, wi, wo, vm, pm);
        return mk3((vp.x - vm.x) * i2h, (vp.y - vm.y) * i2h, (vp.z - vm.z) * i2h);
    }
    // d(value)/d(t) of the nest at (wi, wo): its children's rules and the weight's closed form
    MTS_DEV f3 nest_dvalue(const SceneView &sv, f3 wi, f3 wo) const {
        f3 sum = mk3(0.0f, 0.0f, 0.0f);
        if (nh.two) {
            if (wi.z == 0.0f) return sum;
            if (wi.z < 0.0f) { wi.z = -wi.z; wo.z = -wo.z; }
        }
        const bool blend = nh.kind == kBsdfBlend;
#pragma unroll 1
        for (uint32_t k = 0; k < (blend ? 2u : 1u); ++k) {
            const uint32_t c = k == 0u ? nh.n0 : nh.n1;
            const DevBsdf b = sv.bsdfs[c];
            uint32_t tx; f2 tw; f3 v; float p;
            const f3 rc = eval_reflectance(sv, b, uv, tx, tw);
            bsdf_eval_pdf(b, rc, wi, wo, v, p);
            f3 dv = child_dvalue(sv, c, wi, wo);
            if (F.tex_tangent && tx != kNoPrim) {
                const f3 dr = bsdf_dvalue_drefl(b, rc, wi, wo), dt = texel_tangent(F.tex_tangent, sv.textures[b.texture], tx, tw);
                dv = mk3(fmaf(dr.x, dt.x, dv.x), fmaf(dr.y, dt.y, dv.y), fmaf(dr.z, dt.z, dv.z));
            }
            const float coef = blend ? (k == 0u ? 1.0f - nh.w : nh.w) : nh.w, dc = blend && k == 0u ? -dwt : dwt;
            sum = mk3(fmaf(dc, v.x, fmaf(coef, dv.x, sum.x)), fmaf(dc, v.y, fmaf(coef, dv.y, sum.y)), fmaf(dc, v.z, fmaf(coef, dv.z, sum.z)));
        }
        return sum;
    }
    MTS_DEV void surface(const SurfaceInteraction &si, const DevBsdf &bsdf, f3 refl, uint32_t texel, f2 tw1, f3 thr) {
        nh.kind = 0;
        if (bsdf.type < kBsdfBlend) { Base::surface(si, bsdf, refl, texel, tw1, thr); return; }
        cur = &bsdf; refl0 = refl; rec = si.shape_rec.bsdf; inv_2h = 0.0f; tex = false; maps = false;
        nh = nest_at(bsdf, refl); uv = si.uv; dwt = 0.0f;
        if (nh.open) {
            if (texel != kNoPrim) {         // a bitmap weight: the functional of nest_info over the tangent texels
                if (F.tex_tangent) {
                    const f3 d = texel_tangent(F.tex_tangent, F.rp.sv.textures[bsdf.texture], texel, tw1);
                    dwt = nh.lum ? fmaf(0.072169f, d.z, fmaf(0.715160f, d.y, 0.212671f * d.x)) : d.x;
                }
            } else if (bsdf.texture < 0 && F.inv_2h) dwt = F.inv_2h[rec];      // a constant weight: its tangent rides in inv_2h (kernels.h)
        }
    }
    MTS_DEV bool emitter_sample(const SceneView &sv, const DevBsdf &bsdf, f3 refl, const NeeTerms &t) {
        const bool base = Base::emitter_sample(sv, bsdf, refl, t);      // (sets dle)
        return base || nh.kind != 0;
    }
    MTS_DEV void unoccluded(const SceneView &sv, const SurfaceInteraction &si, f3 thr, const NeeTerms &t) {
        if (nh.kind == 0) { Base::unoccluded(sv, si, thr, t); return; }
        const f3 dbv = nest_dvalue(sv, t.wi, t.wo);
        const float g = em_geo(sv, t);
        const f3 ds = mk3(g * dle.x, g * dle.y, g * dle.z);
        dres = mk3(dres.x + ((t.mis * fmaf(dthr.x, t.bv.x, thr.x * dbv.x)) * t.spec.x + ((t.mis * thr.x) * t.bv.x) * ds.x),
                   dres.y + ((t.mis * fmaf(dthr.y, t.bv.y, thr.y * dbv.y)) * t.spec.y + ((t.mis * thr.y) * t.bv.y) * ds.y),
                   dres.z + ((t.mis * fmaf(dthr.z, t.bv.z, thr.z * dbv.z)) * t.spec.z + ((t.mis * thr.z) * t.bv.z) * ds.z));
    }
    // `bsdf` is the working record of the step: after surface_bsdf_sample, the child that was sampled
    MTS_DEV void bsdf_sampled(const SceneView &sv, const SurfaceInteraction &si, const DevBsdf &bsdf, f3 refl, f3 thr, const BsdfSample &bs, f3 weight, float s1, f2 s2) {
        if (nh.kind == 0) { Base::bsdf_sampled(sv, si, bsdf, refl, thr, bs, weight, s1, s2); return; }
        f3 wi = si.wi, wo = bs.wo;
        if (nh.two && wi.z < 0.0f) { wi.z = -wi.z; wo.z = -wo.z; }
        const NestLobe l = nest_lobe(nh, s1);
        f3 dw = mk3(0.0f, 0.0f, 0.0f);
        if (l.k == 0 || l.k == 1) {
            const uint32_t c = l.k == 0 ? nh.n0 : nh.n1;
            const float i2h = F.inv_2h ? F.inv_2h[c] : 0.0f;
            uint32_t tx; f2 tw;
            const f3 rc = eval_reflectance(sv, bsdf, uv, tx, tw);
            if (i2h != 0.0f && !bs.delta && bs.pdf > 0.0f) {
                const f3 dv = child_dvalue(sv, c, wi, wo);
                const float ip = rcp(bs.pdf);
                dw = mk3(dv.x * ip, dv.y * ip, dv.z * ip);
            } else if (i2h != 0.0f && bs.delta) {        // TangentProbe::bsdf_sampled's rule for a discrete lobe, with the child's sample1
                const DevBsdf bp = F.plus[c], bm = F.minus[c];
                uint32_t tt; f2 t2; f3 wp, wm; BsdfSample bp_, bm_;
                const f3 rp = eval_reflectance(sv, bp, uv, tt, t2), rm = eval_reflectance(sv, bm, uv, tt, t2);
                const bool okp = bsdf_sample(bp, rp, wi, l.s1, s2, bp_, wp);
                const bool okm = bsdf_sample(bm, rm, wi, l.s1, s2, bm_, wm);
                if (okp && okm && bp_.delta && bm_.delta && bp_.wo.x == wo.x && bp_.wo.y == wo.y && bp_.wo.z == wo.z &&
                    bm_.wo.x == wo.x && bm_.wo.y == wo.y && bm_.wo.z == wo.z)
                    dw = mk3((wp.x - wm.x) * i2h, (wp.y - wm.y) * i2h, (wp.z - wm.z) * i2h);
            }
            if (F.tex_tangent && tx != kNoPrim) {
                BsdfSample bl = bs; bl.wo = wo;
                const f3 dr = bsdf_dweight_drefl(bsdf, rc, wi, bl), dt = texel_tangent(F.tex_tangent, sv.textures[bsdf.texture], tx, tw);
                dw = mk3(fmaf(dr.x, dt.x, dw.x), fmaf(dr.y, dt.y, dw.y), fmaf(dr.z, dt.z, dw.z));
            }
        }
        if (dwt != 0.0f && l.k >= 0) {          // the selection probability, attached in the integrand (weight = 1 at the null lobe)
            const float ds = dwt * l.s;
            dw = mk3(fmaf(weight.x, ds, dw.x), fmaf(weight.y, ds, dw.y), fmaf(weight.z, ds, dw.z));
        }
        dthr = mk3(fmaf(dthr.x, weight.x, thr.x * dw.x), fmaf(dthr.y, weight.y, thr.y * dw.y), fmaf(dthr.z, weight.z, thr.z * dw.z));
    }
};

// k_forward on a scene with blend / mask records
template <bool FLAT>
__global__ __launch_bounds__(kBlock) void k_forward_nested(const ForwardParams F) {
    extern __shared__ float4 smem[];
    const RenderParams &P = F.rp;
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    const uint32_t spp = (uint32_t) P.spp;
    for (uint64_t k = (uint64_t) blockIdx.x * kBlock + threadIdx.x; k < F.n_samples; k += (uint64_t) gridDim.x * kBlock) {
        const uint64_t ordinal = P.first_ordinal + k;
        PathState s;
        generate_path(P, ordinal, (uint32_t) (ordinal / spp), (uint32_t) (ordinal % spp), s);
        NestedTangentProbe tp = { { F } };
        tp.dthr = tp.dres = mk3(0.0f, 0.0f, 0.0f);
        tp.nh.kind = 0;
        Counters c = { 0u, 0u, 0u, 0u };
        while (bounce_step<FLAT, 0, true, true>(P, lds, s, c, tp)) { }
        float alpha = (s.flags & 1u) ? 1.0f : 0.0f;
        if (P.store_xyz && !(isfinite(s.res.x) && isfinite(s.res.y) && isfinite(s.res.z))) alpha = -1.0f;
        f3 d = tp.dres;
        if (!(isfinite(d.x) && isfinite(d.y) && isfinite(d.z))) d = mk3(0.0f, 0.0f, 0.0f);
        P.out_rgba[s.ordinal] = make_float4(d.x, d.y, d.z, alpha);
    }
}
hipError_t launch_forward_nested(const ForwardParams &f, hipStream_t s) { return launch_adjoint_kernel<k_forward_nested<true>, k_forward_nested<false>>(f, s); }

// The transpose.  The probe records a nest vertex as ReverseProbe<RECORD, true> records a vertex with wanted slots -- directions, pdf,
// sample numbers, mis * spec, the uv of the hit; r.refl is what the weight reads -- and the sweep rebuilds the rest from these: the
// children's records and reflectances, the lobe the primal took, w and s.
template <bool RECORD>
struct NestedReverseProbe : ReverseProbe<RECORD, true> {
    using Base = ReverseProbe<RECORD, true>;
    bool nest;
    MTS_DEV void surface(const SurfaceInteraction &si, const DevBsdf &bsdf, f3 refl, uint32_t texel, f2 tw1, f3 thr) {
        nest = bsdf.type >= kBsdfBlend;
        if (!nest) { Base::surface(si, bsdf, refl, texel, tw1, thr); return; }
        this->cur = &bsdf; this->refl0 = refl; this->tex = false; this->slotted = RECORD;
        if (RECORD) { this->r->rec = si.shape_rec.bsdf; this->r->wi = si.wi; this->r->refl = refl; this->r->uv = si.uv; }
    }
};

// One blend / mask vertex of the sweep: T' (delta dNc + a dW) of the weight, of the wanted slots of the children and of their reflectance
// texels.  Tp = T invq; a: the suffix adjoint behind the vertex; s_slot: the workgroup's slot bins
template <bool FLAT>
MTS_DEV void reverse_nest_vertex(const ReverseParams &R, const Geo<FLAT> &geo, const DevBsdf &nrec, const VertexRecRN &r, f3 delta, f3 a, f3 Tp, float *s_slot) {
    const SceneView &sv = R.rp.sv;
    const NestAt nh = nest_at(nrec, r.refl);
    f3 wi = r.wi, wo_e = r.wo_e, wo_s = r.wo_s;
    if (nh.two) {
        if (wi.z == 0.0f) return;
        if (wi.z < 0.0f) { wi.z = -wi.z; wo_e.z = -wo_e.z; wo_s.z = -wo_s.z; }
    }
    const bool blend = nh.kind == kBsdfBlend;
    NestLobe l = { -1, 0.0f, 0.0f };
    if (r.flags & 2u) l = nest_lobe(nh, r.s1);
    float gw = 0.0f;        // d / d(w)
#pragma unroll 1
    for (uint32_t k = 0; k < (blend ? 2u : 1u); ++k) {
        const uint32_t c = k == 0u ? nh.n0 : nh.n1;
        const DevBsdf b = geo.bsdf(c);
        uint32_t tx; f2 tw;
        const f3 rc = eval_reflectance(sv, b, r.uv, tx, tw);
        const float coef = blend ? (k == 0u ? 1.0f - nh.w : nh.w) : nh.w;
        const bool chosen = l.k == (int) k;
        if (r.flags & 1u) {         // the evaluation: d / d(w) of (1 - w) f0 + w f1, or of w f_c
            f3 v; float p;
            bsdf_eval_pdf(b, rc, wi, wo_e, v, p);
            const float sg = blend && k == 0u ? -1.0f : 1.0f;
            gw += sg * fmaf(Tp.z * delta.z, r.ms.z * v.z, fmaf(Tp.y * delta.y, r.ms.y * v.y, (Tp.x * delta.x) * (r.ms.x * v.x)));
        }
        if (chosen) gw += l.s * fmaf(Tp.z * a.z, r.W.z, fmaf(Tp.y * a.y, r.W.y, (Tp.x * a.x) * r.W.x));
        // the child at this vertex as the sweep sees a plain vertex: its share of the evaluation, the sample if it drew it
        VertexRecR q;
        q.wi = wi; q.wo_e = wo_e; q.wo_s = wo_s; q.pdf = r.pdf; q.s1 = l.s1; q.s2 = r.s2; q.refl = rc;
        q.ms = mk3(coef * r.ms.x, coef * r.ms.y, coef * r.ms.z);
        q.flags = (r.flags & 1u) | (chosen ? (r.flags & 6u) : 0u);
        if (R.grad_tex && tx != kNoPrim) {
            f3 dnc = mk3(0.0f, 0.0f, 0.0f), dw = dnc;
            if (q.flags & 1u) { const f3 dv = bsdf_dvalue_drefl(b, rc, wi, wo_e); dnc = mk3(q.ms.x * dv.x, q.ms.y * dv.y, q.ms.z * dv.z); }
            if (q.flags & 2u) { BsdfSample bs; bs.wo = wo_s; bs.pdf = r.pdf; bs.delta = (q.flags & 4u) != 0u; dw = bsdf_dweight_drefl(b, rc, wi, bs); }
            const float gg[3] = { Tp.x * fmaf(delta.x, dnc.x, a.x * dw.x), Tp.y * fmaf(delta.y, dnc.y, a.y * dw.y), Tp.z * fmaf(delta.z, dnc.z, a.z * dw.z) };
            if (isfinite(gg[0]) && isfinite(gg[1]) && isfinite(gg[2])) {
                const DevTexture t = sv.textures[b.texture];
                scatter_texel_grad(R.grad_tex, t, tx, tw, gg);
            }
        }
        const uint32_t j0 = R.slot_range ? R.slot_range[c] : 0u, j1 = R.slot_range ? R.slot_range[c + 1] : 0u;
        for (uint32_t j = j0; j < j1; ++j) {
            const ReverseSlot sl = R.slots[j];
            f3 dnc, dw;
            reverse_slot_terms(b, sl, q, dnc, dw);
            const float g = fmaf(Tp.z, fmaf(delta.z, dnc.z, a.z * dw.z), fmaf(Tp.y, fmaf(delta.y, dnc.y, a.y * dw.y), Tp.x * fmaf(delta.x, dnc.x, a.x * dw.x)));
            if (g != 0.0f && isfinite(g)) {
                if (j < kReverseSlotBins) atomicAdd(&s_slot[j], g);
                else atomicAdd(R.grad_bsdf + sl.out, g);
            }
        }
    }
    if (l.k == 2) gw += l.s * fmaf(Tp.z, a.z, fmaf(Tp.y, a.y, Tp.x * a.x));       // the null lobe: W = 1
    if (!nh.open || gw == 0.0f || !isfinite(gw)) return;
    uint32_t tx; f2 tw;
    (void) eval_reflectance(sv, nrec, r.uv, tx, tw);      // the footprint of a bitmap weight
    if (tx != kNoPrim) {
        if (R.grad_tex) {
            const float gg[3] = { nh.lum ? 0.212671f * gw : gw, nh.lum ? 0.715160f * gw : 0.0f, nh.lum ? 0.072169f * gw : 0.0f };
            const DevTexture t = sv.textures[nrec.texture];
            scatter_texel_grad(R.grad_tex, t, tx, tw, gg);
        }
    } else if (nrec.texture < 0 && R.slot_range) {
        for (uint32_t j = R.slot_range[r.rec]; j < R.slot_range[r.rec + 1]; ++j)
            if (R.slots[j].f0 == kWeightSlot) {
                if (j < kReverseSlotBins) atomicAdd(&s_slot[j], gw);
                else atomicAdd(R.grad_bsdf + R.slots[j].out, gw);
            }
    }
}

// k_reverse on a scene with blend / mask records: its replay and sweep, and reverse_nest_vertex at the nest vertices
template <bool FLAT, bool RECORD>
__global__ __launch_bounds__(kBlock) void k_reverse_nested(const ReverseParams R) {
    extern __shared__ float4 smem[];
    const RenderParams &P = R.rp;
    const LdsView lds = lds_stage<FLAT>(P.sv, smem);
    float *const s_em = reverse_emitter_bins();
    __shared__ float s_slot[RECORD ? kReverseSlotBins : 1u];
    for (uint32_t i = threadIdx.x; i < 3u * kReverseEmitterBins; i += kBlock) s_em[i] = 0.0f;
    for (uint32_t i = threadIdx.x; i < (RECORD ? kReverseSlotBins : 1u); i += kBlock) s_slot[i] = 0.0f;
    __syncthreads();
    for (uint64_t k = (uint64_t) blockIdx.x * kBlock + threadIdx.x; k < R.n_samples; k += (uint64_t) gridDim.x * kBlock) {
        PathState s; const f3 delta = adjoint_sample(R, k, s);
        if (delta.x == 0.0f && delta.y == 0.0f && delta.z == 0.0f) continue;
        Counters c = { 0u, 0u, 0u, 0u };
        NestedReverseProbe<RECORD> pr = { { R, delta, nullptr } };
        pr.nest = false;
        if constexpr (!RECORD) {
            while (bounce_step<FLAT, 0, true, true>(P, lds, s, c, pr)) { }
        } else {
        VertexRecRN rec[kAdjointMaxDepth];
        int n = 0;
        bool alive = true;
        while (alive && n < kAdjointMaxDepth) { pr.r = &rec[n]; alive = bounce_step<FLAT, 0, true, true>(P, lds, s, c, pr); ++n; }
        const Geo<FLAT> geo{ P.sv, lds };
        f3 a = mk3(0.0f, 0.0f, 0.0f);
        for (int v = n - 1; v >= 0; --v) {
            const VertexRecRN &r = rec[v];
            const f3 Tp = r.T * r.invq;
            if (r.texel != kNoPrim) {
                const float gg[3] = { Tp.x * fmaf(delta.x, r.dNc.x, a.x * r.dW.x), Tp.y * fmaf(delta.y, r.dNc.y, a.y * r.dW.y),
                                      Tp.z * fmaf(delta.z, r.dNc.z, a.z * r.dW.z) };
                if (isfinite(gg[0]) && isfinite(gg[1]) && isfinite(gg[2])) {
                    const DevTexture t = P.sv.textures[r.texture];
                    scatter_texel_grad(R.grad_tex, t, r.texel, r.w1, gg);
                }
            }
            if (r.rec >= 0) {
                const DevBsdf base = geo.bsdf((uint32_t) r.rec);
                if (base.type >= kBsdfBlend) reverse_nest_vertex<FLAT>(R, geo, base, r, delta, a, Tp, s_slot);
                else {
                    const uint32_t j0 = R.slot_range ? R.slot_range[r.rec] : 0u, j1 = R.slot_range ? R.slot_range[r.rec + 1] : 0u;
                    for (uint32_t j = j0; j < j1; ++j) {
                        const ReverseSlot sl = R.slots[j];
                        f3 dnc, dw;
                        reverse_slot_terms(base, sl, r, dnc, dw);
                        const float g = fmaf(Tp.z, fmaf(delta.z, dnc.z, a.z * dw.z), fmaf(Tp.y, fmaf(delta.y, dnc.y, a.y * dw.y), Tp.x * fmaf(delta.x, dnc.x, a.x * dw.x)));
                        if (g != 0.0f && isfinite(g)) {
                            if (j < kReverseSlotBins) atomicAdd(&s_slot[j], g);
                            else atomicAdd(R.grad_bsdf + sl.out, g);
                        }
                    }
                }
            }
            const f3 b = mk3(fmaf(delta.x, r.Nc.x, r.W.x * a.x), fmaf(delta.y, r.Nc.y, r.W.y * a.y), fmaf(delta.z, r.Nc.z, r.W.z * a.z));
            a = mk3(delta.x * r.E.x + r.invq * b.x, delta.y * r.E.y + r.invq * b.y, delta.z * r.E.z + r.invq * b.z);
            if (r.rr_channel >= 0) {
                const float corr = ((r.invq * r.invq) * r.eta2) * (b.x * r.T.x + b.y * r.T.y + b.z * r.T.z);
                if (r.rr_channel == 0) a.x -= corr; else if (r.rr_channel == 1) a.y -= corr; else a.z -= corr;
            }
        }
        }
    }
    __syncthreads();
    if (R.grad_emitter)
        for (uint32_t i = threadIdx.x; i < 3u * min(P.sv.n_emitters, kReverseEmitterBins); i += kBlock)
            if (s_em[i] != 0.0f) atomicAdd(R.grad_emitter + i, s_em[i]);
    if (RECORD && R.grad_bsdf)
        for (uint32_t i = threadIdx.x; i < min(R.n_slots, kReverseSlotBins); i += kBlock)
            if (s_slot[i] != 0.0f) atomicAdd(R.grad_bsdf + R.slots[i].out, s_slot[i]);
}
hipError_t launch_reverse_nested(const ReverseParams &r, bool record, hipStream_t s) {
    return record ? launch_adjoint_kernel<k_reverse_nested<true, true>, k_reverse_nested<false, true>>(r, s)
                  : launch_adjoint_kernel<k_reverse_nested<true, false>, k_reverse_nested<false, false>>(r, s);
}

} // namespace mtsamd

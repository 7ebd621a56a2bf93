// kernels.h -- host-visible launch interface of the gfx950 kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "device_scene.h"
#include "device_spectral.h"

namespace mtsamd {

// Path-state streams: SoA of 16-byte vectors, one slot per in-flight path (88 B per path).
//   ray_o = (o.xyz, mint)  ray_d = (d.xyz, maxt)  thr = (throughput rgb, bs_pdf)
//   res = (radiance rgb, eta)  rng = PCG32 (state, inc)  misc = (sample ordinal, depth | flags << 16)
struct PoolView {
    float4 *ray_o, *ray_d, *thr, *res;
    uint4 *rng;
    uint2 *misc;
    // spectral variant (100 B per path): thr / res hold 4 spectral samples, aux = (bs_pdf, eta), xi = the wavelength sample the path's
    // four wavelengths are a function of (wavelengths_from_sample; round 2 stored the wavelengths: 112 B)
    float *xi;
    float2 *aux;
    // split pipeline (hierarchy scenes): hit = (t, prim bits, u, v) of the path's ray; per-wave dense queue of
    // pending shadow rays sh_o = (o, mint), sh_d = (d, maxt), the contribution `nee` each guards and the slot it belongs to
    float4 *hit, *sh_o, *sh_d, *nee;
    uint32_t *sh_slot;
};

// Film rows owned by one render call.  count <= 1: the contiguous window [row0, row0 + local_rows);
// count > 1: the film is cut into tiles of tile_rows rows dealt round-robin, this call owns tiles t % count == part.
struct RowMap { int32_t row0, local_rows, tile_rows, part, count; };
__host__ __device__ __forceinline__ int32_t row_to_global(const RowMap &m, int32_t lr) {
    if (m.count <= 1) return m.row0 + lr;
    int32_t t = lr / m.tile_rows;
    return (t * m.count + m.part) * m.tile_rows + (lr - t * m.tile_rows);
}
MTS_DEV int32_t row_to_local(const RowMap &m, int32_t gr) {     // -1: not owned
    if (m.count <= 1) { int32_t lr = gr - m.row0; return (lr >= 0 && lr < m.local_rows) ? lr : -1; }
    int32_t t = gr / m.tile_rows;
    if (t % m.count != m.part) return -1;
    return (t / m.count) * m.tile_rows + (gr - t * m.tile_rows);
}

struct FilterView {
    float table[32];
    float radius, scale_factor, alpha, bias;
    int32_t kind, analytic, border, taps;   // taps = n in imageblock.cpp:123
};

struct RenderParams {
    SceneView sv;
    CameraView cam;
    PoolView in, out;
    const uint32_t *count_in;   // per scheduling wave
    uint32_t *count_out;
    uint32_t *count_shadow;     // split pipeline: queued shadow rays per scheduling wave (output pool)
    uint64_t *cursor;           // per wave: how many of its samples it has generated (kernels.hip cursor_sample maps them to ordinals)
    const uint64_t *cursor_end;
    uint64_t *wave_stats;       // per wave: closest, any, segments, tri tests
    float4 *out_rgba;           // per sample ordinal: radiance rgb + valid_ray
    float2 *out_pos;            // per sample ordinal: film position sample
    uint32_t chunk;             // samples per chunk dealt to a scheduling wave (kernels.hip, cursor_sample)
    uint32_t n_chains;          // 0 / 1, or the number of launch chains the scheduling waves are cut into (hierarchy scenes): the chunks are dealt
                                // to the chains in turn (chunk_owner), so that every chain sees the same mix of pixels
    uint32_t first_pix, first_rem;       // first_ordinal = first_pix * spp + first_rem (film renders: passes start on a pixel, first_rem == 0)
    uint64_t first_ordinal;     // local sample ordinal of slot 0 of out_rgba / out_pos
    uint64_t base_seed;
    RowMap rows;                // which film rows this render owns (multi-GPU film partition)
    int32_t store_xyz;          // 1: out_rgba holds (X,Y,Z,alpha | -1 if the sample is invalid) for the film, 2: same with
                                // linear RGB instead of XYZ, 0: (R,G,B,alpha) for the per-sample API
    // sample-stream slot of (local pixel lp, sample j): plane_pixels == 0: ordinal - first_ordinal (pixel-major);
    // else j * plane_pixels + (lp - plane_pix0): one plane per sample number, so that a film tile reads contiguous pixels
    uint32_t plane_pix0, plane_pixels;
    uint32_t n_waves, seg_cap, target;
    int32_t spp, crop_x, crop_y, crop_w, crop_h;
    int32_t max_depth, rr_depth;
    int32_t spectral;           // 0: RGB variant, 1: spectral variant (4 wavelengths per sample)
    int32_t integrator, emitter_samples, bsdf_samples, hide_emitters;   // 0 path; 1 direct (direct.cpp); 2 depth (depth.cpp)
    int32_t split;              // 0: fused k_bounce, 1: k_trace<closest> + k_shade + k_trace<any> per iteration, 2: k_shade (flat) + k_trace<any>,
                                // 3: k_shade (flat) with the in-kernel shadow ring
    uint32_t lds_queue_offset;  // split == 3: start of the per-wave shadow rings in LDS, in float4 units
    uint32_t wave_first, wave_last;   // k_shade: scheduling waves covered by this launch (wave_last == 0: all)
    uint32_t gather_w;          // k_shade on LDS-resident scenes: a workgroup gathers the paths of gather_w (4, 16, ... 1024) consecutive scheduling
                                // waves into the first four (pool drain: the sample cursors of the launch are dry); 0 / 4: no gathering
    uint32_t trace_lds_depth;   // k_trace: stack entries per lane kept in LDS; deeper ones go to trace_spill
    uint32_t trace_top_nodes;   // k_trace: BVH4 nodes [0, trace_top_nodes) are staged in LDS by every workgroup
    uint32_t *trace_spill;      // k_trace: [workgroup][entry][thread]
};

// Launch chains of the split pipeline: chain k covers the scheduling waves [chain_first(k), chain_first(k + 1)); the boundaries are
// multiples of kChainAlign (itself a multiple of the k_trace group size: a group never straddles two launches).
constexpr uint32_t kMaxChains = 8u, kChainAlign = 64u;
constexpr uint32_t kTraceChains = 2u;       // chains a render runs
__host__ __device__ inline uint32_t chain_first(uint32_t k, uint32_t n, uint32_t chains) {
    if (k >= chains) return n;
    const uint32_t lo = ((uint32_t) ((uint64_t) n * k / chains) + kChainAlign - 1u) & ~(kChainAlign - 1u);
    return lo < n ? lo : n;
}
// Index of the (first) chunk owned by scheduling wave `wave`: the identity, or -- `chains` launch chains -- chunk i * chains + k for
// the i-th wave of chain k as long as every chain has an i-th wave; the few waves beyond that take the remaining chunks in order.
// A bijection of [0, n).
__host__ __device__ inline uint32_t chunk_owner(uint32_t wave, uint32_t n, uint32_t chains) {
    if (chains <= 1u) return wave;
    uint32_t s_min = n, k = 0u, lo_k = 0u, extra_before = 0u;
    for (uint32_t c = 0; c < chains; ++c) {
        const uint32_t lo = chain_first(c, n, chains), hi = chain_first(c + 1u, n, chains);
        s_min = hi - lo < s_min ? hi - lo : s_min;
        if (wave >= lo && wave < hi) { k = c; lo_k = lo; }
    }
    const uint32_t i = wave - lo_k;
    if (i < s_min) return i * chains + k;
    for (uint32_t c = 0; c < k; ++c) extra_before += chain_first(c + 1u, n, chains) - chain_first(c, n, chains) - s_min;
    return s_min * chains + extra_before + (i - s_min);
}

// tiled film splat: source tiles of kFilmTile^2 pixels; scratch tiles of kFilmPartial floats, laid out for the widest supported apron (R = 2)
constexpr int kFilmTile = 16, kFilmDest = kFilmTile + 4, kFilmPartial = kFilmDest * kFilmDest * 5;

struct FilmParams {
    const float4 *out_rgba;
    const float2 *out_pos;
    float *film;                // crop_h * crop_w * 5
    FilterView filter;
    uint64_t first_ordinal, n_samples;   // local sample ordinals held by out_rgba / out_pos (pixel-major layout)
    uint32_t plane_pix0, plane_pixels;   // plane layout (see RenderParams): the pass holds whole local rows
    RowMap rows;
    int32_t spp, crop_x, crop_y, crop_w, crop_h;
    int32_t row0, row1;         // target (global) rows [row0,row1)
    // tiled splat: the pass holds the local rows [pass_lr0, pass_lr0 + pass_rows), cut into 16x16 source tiles; every tile
    // accumulates the film pixels it reaches into its scratch tile of `partials`
    int32_t pass_lr0, pass_rows, tiles_x, tiles_y;
    int32_t tile_h;             // local rows per source tile (<= 16; 16 unless a partitioned film forces less)
    int32_t slices;             // the samples of a pixel are cut into this many runs, each accumulated by a workgroup of its own (few tiles, many samples)
    float *partials;
};

struct AdjointParams {
    RenderParams rp;            // scene, sensor, sampler, integrator of the primal render (rows = the whole crop)
    FilterView filter;
    uint64_t n_samples;         // crop_w * crop_h * spp
    const float *dimage;        // dLoss/dImage, crop_h * crop_w * 3
    const float *film;          // primal film (5 channels; only the weight channel is read)
    float *grad_bsdf;           // n_bsdfs * 3, accumulated (may be null)
    float *grad_tex;            // all textures concatenated in index order, accumulated (may be null)
    float *grad_emitter;        // n_emitters * 3 (radiance of area lights), accumulated (may be null)
    float *grad_env;            // k_adjoint_env: envmap height * width * 3, accumulated
    // k_adjoint_param: record `pg_bsdf` of the BSDF table with ONE scalar parameter at +h / -h, 1 / (2 h), and the float the derivative is added to
    int32_t pg_bsdf; DevBsdf pg_plus, pg_minus; float pg_inv_2h; float *grad_param;
    // k_adjoint_param_tex reads two of these fields in its own way (no field of its own: the argument block of the kernels above stays
    // what it was): pg_bsdf = the slot of the launch (kTexAlphaU .. kTexTrans), pg_inv_2h = the step h itself (<= 0: 1 % of the value at
    // the hit); it adds into grad_tex
};

// k_forward: the forward-mode derivative render.  The camera samples [rp.first_ordinal, rp.first_ordinal + n_samples) of the whole crop
// window are replayed; d(radiance) along ONE tangent direction over four parameter families goes to rp.out_rgba / rp.out_pos in the slot
// layout of the sample stream (slot = ordinal - first_ordinal), ready for the film kernels.  An argument block of its own: AdjointParams,
// and with it the argument block of every k_adjoint* kernel, stays what it was.
constexpr uint32_t kForwardDetachRoulette = 1u;      // MTSAMD_FORWARD_DETACH_ROULETTE
struct ForwardParams {
    RenderParams rp;            // as AdjointParams::rp, with out_rgba / out_pos and store_xyz (0: plain alpha; else -1 marks a dropped sample)
    uint64_t n_samples;
    // BSDF constants: record b of the table at theta + eps t / theta - eps t and 1 / (2 eps); inv_2h[b] == 0: no tangent on record b.
    // All three null: no BSDF tangents
    const DevBsdf *plus, *minus; const float *inv_2h;
    const float *tex_tangent;   // tangent texels of the reflectance family, layout of grad_textures (mtsamd_scene_texture_info), or null
    const float *em_tangent;    // n_emitters * 3: tangent of the emitter colours (row of an envmap: not read), or null
    const float *env_tangent;   // envmap height * width * 3, or null
    uint32_t flags;             // kForwardDetachRoulette
    float map_h;                // nest launches: the absolute step of the map slots' central differences (<= 0: 1 % of the value at the hit);
                                // it sits in what was the struct's tail padding, so the argument block keeps its size
};
// nest: the scene has textured BSDF parameters (k_forward<FLAT, true>: the step that resolves them, and tangents on the maps' texels)
hipError_t launch_forward(const ForwardParams &f, bool nest, hipStream_t s);

// k_reverse: the transpose of k_forward -- one replay of every camera sample, one dLoss/dImage, the gradient of every parameter the
// forward mode knows.  An argument block of its own: AdjointParams and ForwardParams stay what they were.
// One wanted BSDF scalar: record `record` with the floats f0 and f1 (offsets in floats into DevBsdf; f1 == f0 unless ALPHA moves both
// roughnesses) set to `plus` / `minus` is the perturbed pair of its central difference, inv_2h = 1 / (plus - minus); the gradient is
// added to grad_bsdf[out], out = 18 * record + 3 * kind + component (the layout of mtsamd_tangent_desc::bsdf_tangents).
struct ReverseSlot { uint32_t record; uint16_t f0, f1; float plus, minus, inv_2h; uint32_t out; };
static_assert(sizeof(ReverseSlot) == 24, "a slot is a 24-byte patch, not a pair of records");
constexpr uint32_t kReverseDetachRoulette = 1u;      // MTSAMD_REVERSE_DETACH_ROULETTE
// Per-workgroup LDS bins of k_reverse: the sums of the first kReverseSlotBins slots and of the first kReverseEmitterBins emitters are
// kept in LDS (float atomics) and flushed with one global atomicAdd per non-zero bin; slots and emitters beyond go straight to global
// atomics.  (64 + 3 * 32) * 4 = 640 bytes of static LDS beside a flat scene's kFlatLdsCap = 150 KiB of the CU's 160 KiB.
constexpr uint32_t kReverseSlotBins = 64u, kReverseEmitterBins = 32u;
struct ReverseParams {
    RenderParams rp;            // as AdjointParams::rp
    FilterView filter;
    uint64_t n_samples;         // crop_w * crop_h * spp
    const float *dimage;        // dLoss/dImage, crop_h * crop_w * 3
    const float *film;          // primal film (5 channels; only the weight channel is read)
    const ReverseSlot *slots;   // n_slots wanted scalars in record order; the slots of record b are slot_range[b] .. slot_range[b + 1]
    const uint32_t *slot_range; // n_bsdfs + 1 (null with slots)
    uint32_t n_slots;
    float *grad_bsdf;           // n_bsdfs * 18, accumulated at the wanted entries (null iff there are no slots)
    float *grad_emitter;        // n_emitters * 3, accumulated (row of an envmap untouched), or null
    float *grad_tex;            // layout of AdjointParams::grad_tex, accumulated, or null
    float *grad_env;            // envmap height * width * 3, accumulated, or null
    uint32_t flags;             // kReverseDetachRoulette
    float map_h;                // nest launches: as ForwardParams::map_h (tail padding as well)
};
// record = true: the replay keeps its vertices (at most 16, 0 <= max_depth <= 16) and sweeps them backwards -- BSDF scalars and texels;
// false: emitter colours and envmap texels only, accumulated while the path runs, any max_depth
// nest: the scene has textured BSDF parameters (k_reverse<FLAT, RECORD, true>); grad_tex then also collects the texels of the maps
hipError_t launch_reverse(const ReverseParams &r, bool record, bool nest, hipStream_t s);

// Scenes with blendbsdf / mask records (MTSAMD_FORWARD_NESTED / MTSAMD_REVERSE_NESTED): k_forward_nested<FLAT> / k_reverse_nested<FLAT,
// RECORD>, on the same argument blocks.  The weight / opacity of a nested record has a closed-form derivative, so it needs no +- pair:
// forward, inv_2h[b] of a nested record b carries the TANGENT of its constant weight (no plain rule ever reads that entry); reverse, a
// wanted constant weight is a slot of its record with f0 = f1 = kWeightSlot and out = 18 * b.  Texels of a bitmap weight use tex_tangent /
// grad_tex like every other bitmap.
constexpr uint16_t kWeightSlot = 0xffffu;
hipError_t launch_forward_nested(const ForwardParams &f, hipStream_t s);
hipError_t launch_reverse_nested(const ReverseParams &r, bool record, hipStream_t s);

struct RayStreams {
    const float *ox, *oy, *oz, *dx, *dy, *dz, *mint, *maxt;
    const uint8_t *active;
};

size_t bounce_lds_bytes(const SceneView &sv);
// k_shade with the in-kernel shadow ring (split 3): per wave a ring of kShadowRing shadow rays.  An entry is o (+ mint), d (+ maxt) and
// nee as three float4 (48 B); RGB paths keep the output slot in nee.w (always 0 there), spectral ones need all four wavelengths and
// keep it in a word of its own (52 B).  Dynamic LDS of a launch: the scene (+ work lists), the four rings and, when a workgroup gathers
// the paths of gather_w > 4 scheduling waves, their prefix sums (gather_w + 1 words).
constexpr uint32_t kShadowRing = 128u;                       // >= 63 queued + 64 pushed
constexpr uint32_t kShadeWaves = 4u;                         // waves per k_shade workgroup (kBlock / 64)
inline size_t shadow_ring_bytes(bool spectral) { return (size_t) kShadowRing * (spectral ? 52u : 48u); }
inline size_t shade_ring_offset(const SceneView &sv, uint32_t block) { return (lds_bytes(sv, block) + 15u) & ~(size_t) 15u; }
inline size_t shade_ring_lds_bytes(const SceneView &sv, bool spectral, uint32_t gather_w) {
    return shade_ring_offset(sv, 64u * kShadeWaves) + kShadeWaves * shadow_ring_bytes(spectral) + (gather_w > 4u ? 4u * ((size_t) gather_w + 1u) : 0u);
}
// The largest dynamic LDS any launch asks for on a flat scene (sv.flat set; the counts n_prims, n_pairs, n_clusters, n_shapes, n_bsdfs and
// n_emitters are all it reads).  Every launch that stages a flat scene sizes its LDS by one of three formulas: lds_bytes(sv, 64)
// (k_mega, k_finish), lds_bytes(sv, 256) (every other kernel) or shade_ring_lds_bytes (k_shade with the ring; gathering launches use
// gather_w <= 1024).  The tables grow with the BSDF, emitter and shape counts, which the triangle count does not bound, so the builder
// keeps a scene flat only while this fits kFlatLdsCap (scene_build.cpp); kernels.hip opts every flat launch into its byte count.
constexpr uint32_t kGatherMax = 1024u;
constexpr size_t kFlatLdsCap = 150u * 1024u;                 // of the 160 KiB of a CU: room for static LDS
inline size_t flat_launch_lds_max(const SceneView &sv, bool spectral) {
    const size_t a = lds_bytes(sv, 64u), b = lds_bytes(sv, 64u * kShadeWaves), c = shade_ring_lds_bytes(sv, spectral, kGatherMax);
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}
// The headline's k_shade runs 4 workgroups per CU (160 KiB of LDS): the fixed part -- rings, work lists, static LDS (<= 512 B) -- has
// to leave room for a Cornell-box-sized scene (5.2 KB; 6 KiB here).  A larger MTS_FLAT_WL_ROUNDS fails here instead of silently
// costing a workgroup per CU (tests/test_shade_lds_cpu.py checks the real Cornell box against the compiler's figures).
static_assert(kShadeWaves * (48u * kShadowRing + 4u * kWlWords) + 4u + 512u + 6144u <= 160u * 1024u / 4u,
              "work lists + shadow rings no longer fit 4 k_shade workgroups per CU");
hipError_t launch_bounce(const RenderParams &p, hipStream_t s);
hipError_t launch_split_stage(const RenderParams &p, int stage, hipStream_t s);
uint32_t trace_lds_depth(const SceneView &sv);
uint32_t trace_top_nodes(const SceneView &sv);
uint32_t trace_group();          // scheduling waves per k_trace workgroup (a power of two): launch ranges start on multiples of it
size_t trace_spill_words(const SceneView &sv, uint32_t n_waves);
// `direct` / `depth` integrators: every sample of [first_ordinal, first_ordinal + n) is finished by one thread
hipError_t launch_direct(const RenderParams &p, uint64_t n, hipStream_t s);
// `aov` integrator (src/integrators/aov.cpp:166-219): k_aov re-traces the camera ray of every sample of [first_ordinal, first_ordinal + n)
// and writes the requested SurfaceInteraction fields as groups of three channels: groups[g * group_stride + slot] = (channel 3g, 3g + 1,
// 3g + 2, 0 | -1 if a channel of the group is not finite; launch_aov_finish extends the flag to the whole sample) -- the (X, Y, Z, alpha | -1) layout of the sample stream, so that the
// 5-channel film kernels splat a group as they splat radiance.  rp needs sv, cam, wave_stats, n_waves, out_pos (may be null), the sampler and
// film fields generate_path reads; no path pool.
constexpr uint32_t kAovMaxChannels = 32u;
// what a channel shows: t, p.xyz, uv, n.xyz, sh_frame.n.xyz, dp_du.xyz, dp_dv.xyz, or nothing (duv_dx / duv_dy: kdtree.h:2353 zeroes
// them and aov.cpp never calls compute_partials)
enum AovSource : uint8_t { kAovT = 0, kAovP = 1, kAovUV = 4, kAovN = 6, kAovShN = 9, kAovDpDu = 12, kAovDpDv = 15, kAovZero = 18 };
struct AovParams {
    RenderParams rp;
    float4 *groups;
    uint64_t group_stride;      // slots per group
    uint32_t n_channels;        // <= kAovMaxChannels; (n_channels + 2) / 3 groups
    uint8_t source[kAovMaxChannels];
};
hipError_t launch_aov(const AovParams &a, uint64_t n, hipStream_t s);
// Samples of an AOV pass agree on what is dropped: sample i is dropped in `stream` and in every group if it is dropped in one of them
// (ImageBlock::put drops a sample when any channel is not finite, imageblock.cpp:85-109).  mode 0: no nested integrator, stream[i] =
// (0, 0, 0, 0 | -1); 1: stream holds linear RGB (store_xyz = 2), conv[i] = its XYZ (integrator.cpp:254-262); 2: stream holds XYZ (spectral
// variant), conv[i] = its linear RGB
hipError_t launch_aov_finish(float4 *stream, float4 *conv, float4 *groups, uint64_t group_stride, uint32_t n_groups, int mode, uint64_t n, hipStream_t s);
// films5: 1 + n_groups (+ 1 with `nested`) films of n_pixels x 5 floats -> film (n_pixels x (5 + n_channels (+ 4))), accumulating:
// X, Y, Z, A, W of film 0, channel c from film 1 + c / 3, then R, G, B, A of the last film
hipError_t launch_aov_pack(const float *films5, uint64_t n_pixels, uint32_t n_channels, int nested, float *film, hipStream_t s);
// groups -> out[i * n_channels + c] (mtsamd_sample_aovs)
hipError_t launch_aov_unpack(const float4 *groups, uint64_t group_stride, uint32_t n_channels, uint64_t n, float *out, hipStream_t s);
hipError_t launch_adjoint(const AdjointParams &a, hipStream_t s);
hipError_t launch_adjoint_env(const AdjointParams &a, hipStream_t s);
hipError_t launch_adjoint_param(const AdjointParams &a, hipStream_t s);
hipError_t launch_adjoint_tex(const AdjointParams &a, hipStream_t s);      // k_adjoint_tex: into grad_tex (not null)
hipError_t launch_adjoint_param_tex(const AdjointParams &a, hipStream_t s);      // k_adjoint_param_tex: one slot of the textured parameters, into grad_tex (not null)
// k_adjoint_spectral accumulates in the coefficients (a, b, c) of x = a u^2 + b u + c over the centred wavelength u = (l - kCoeffMid) / kCoeffHalf
constexpr float kCoeffMid = 595.0f, kCoeffHalf = 235.0f;
// k_adjoint_spectral: gradients w.r.t. the srgb MODEL COEFFICIENTS (centred basis) of the reflectance family, into grad_bsdf / grad_tex (either may be null)
hipError_t launch_adjoint_spectral(const AdjointParams &a, hipStream_t s);
// out[i] += J_i^T cgrad[i] for n colours (3 floats each): jac[9 i + 3 c + j] = d coeff_j / d rgb_c (centred basis)
hipError_t launch_coeff_grad_to_rgb(const float *cgrad, const float *jac, float *out, uint32_t n, hipStream_t s);
// k_adjoint_spectral_emitters: gradients w.r.t. the (model coefficients in the centred basis, scale) of the emitter colours, as 4-float rows:
// a.grad_emitter = n_emitters rows, a.grad_env = envmap height * width rows (either may be null)
hipError_t launch_adjoint_spectral_emitters(const AdjointParams &a, hipStream_t s);
// out[i] += Jn_i^T rows[i].xyz + sel_i rows[i].w for n emitter colours: jac[12 i + 3 c + j] = d coeff_j / d rgb_c (centred basis),
// jac[12 i + 9 + c] = d scale / d rgb_c
hipError_t launch_emitter_grad_to_rgb(const float *rows, const float *jac, float *out, uint32_t n, hipStream_t s);
// end of a pass: every path of p.in (counts p.count_in) is run to its end in one launch; needs dry sample cursors (kernels.hip, k_finish)
hipError_t launch_finish(const RenderParams &p, uint64_t alive, hipStream_t s);
hipError_t launch_mega(const RenderParams &p, hipStream_t s);      // small passes: the whole pass in one launch of persistent lanes
// CIE x, y, z and D65 tables (95 floats each) -> device; call once before the first spectral launch
hipError_t upload_spectral_tables(const float *x, const float *y, const float *z, const float *d65);
hipError_t launch_film_gather(const FilmParams &p, hipStream_t s);
// tiled variant for filters with <= 4 taps (gaussian stddev 0.5, box, tent): k_film_accum + k_film_merge; which filters it takes, its
// tile grid and the size of `partials` are host arithmetic (schedule.h, film splat)
hipError_t launch_film_tiles(const FilmParams &p, hipStream_t s);
// mode 0: closest (BVH), 1: closest (brute force)
hipError_t launch_ray_intersect(const SceneView &sv, uint64_t n, const RayStreams &r, int mode, float *t,
                                uint32_t *prim, uint32_t *shape, float *u, float *v, float *si26,
                                hipStream_t s);
hipError_t launch_ray_test(const SceneView &sv, uint64_t n, const RayStreams &r, uint8_t *hit, hipStream_t s);
// Operator API on device streams (kernels.hip, "Operator API"): one query per row, SoA planes, optional byte mask
struct BsdfStreams {
    const uint32_t *shape;
    const float *wix, *wiy, *wiz, *u, *v, *wox, *woy, *woz, *s1, *s2x, *s2y;      // u, v may be null (0); wo: eval / pdf, s1, s2: sample
    const uint8_t *active;
};
struct EmitterSampleStreams { const float *px, *py, *pz, *sx, *sy; const uint8_t *active; };
// pdf: n = normal at the emitter, dist, delta flags (may be null); eval: n = the local wi of the interaction, d = world direction of the ray
struct EmitterQueryStreams { const uint32_t *emitter; const float *dx, *dy, *dz, *nx, *ny, *nz, *dist; const uint8_t *delta, *active; };
hipError_t launch_bsdf_eval_pdf(const SceneView &sv, uint64_t n, const BsdfStreams &q, float *out4, hipStream_t s);
hipError_t launch_bsdf_sample(const SceneView &sv, uint64_t n, const BsdfStreams &q, float *out10, hipStream_t s);
hipError_t launch_sample_emitter_direction(const SceneView &sv, uint64_t n, const EmitterSampleStreams &q, float *out15, uint32_t *emitter, hipStream_t s);
hipError_t launch_pdf_emitter_direction(const SceneView &sv, uint64_t n, const EmitterQueryStreams &q, float *pdf, hipStream_t s);
hipError_t launch_emitter_eval(const SceneView &sv, uint64_t n, const EmitterQueryStreams &q, float *out3, hipStream_t s);
hipError_t launch_sampler_seed(uint64_t n, uint64_t first, uint64_t base_seed, uint64_t *state, uint64_t *inc, hipStream_t s);
hipError_t launch_sampler_next(uint64_t n, int dims, uint64_t *state, const uint64_t *inc, const uint8_t *active, float *out, hipStream_t s);
hipError_t launch_camera_rays(const CameraView &cam, uint64_t n, const float *sx, const float *sy, const float *apx, const float *apy, float *ox,
                              float *oy, float *oz, float *dx, float *dy, float *dz, float *mint, float *maxt,
                              hipStream_t s);
hipError_t launch_imageblock_put(const FilterView &f, int32_t w, int32_t h, int32_t ox, int32_t oy, int32_t ch,
                                 int32_t border, uint64_t n, const float *pos, const float *values, float *data,
                                 hipStream_t s);
hipError_t launch_put_block(const float *src, int32_t sw, int32_t sh, int32_t sox, int32_t soy, int32_t sb,
                            float *dst, int32_t dw, int32_t dh, int32_t dox, int32_t doy, int32_t db, int32_t ch,
                            hipStream_t s);
// moment integrator: squares the (X,Y,Z) of every valid sample of the stream in place; packs the two 5-channel films
// (values, squared values) into the 11-channel film of moment.cpp (accumulating)
hipError_t launch_square_stream(float4 *rgba, uint64_t n, hipStream_t s);
hipError_t launch_moment_pack(const float *values5, const float *squares5, float *film11, uint64_t n_pixels, hipStream_t s);
// roughplastic: fills the 64-entry external transmittance table of bsdfs[index] and its internal diffuse reflectance
// (DevBsdf::eb).  gl = Gauss-Legendre nodes / weights: [nodes_t(128) | weights_t(128) | nodes_r(128) | weights_r(128)]
hipError_t launch_roughplastic_tables(DevBsdf *bsdfs, uint32_t index, float *table, const float *gl, int res_t, int res_r, hipStream_t s);
hipError_t launch_flat_frames(float4 *flat, uint32_t n_prims, const DevShape *shapes, const float *tri_uv, hipStream_t s);
hipError_t launch_film_develop(const float *xyzaw, uint64_t n, float *rgba, hipStream_t s);
hipError_t launch_libm_eval(int fn, uint64_t n, const float *x, const float *y, float *out, hipStream_t s);
hipError_t launch_spectrum_eval(const DevSpectrum *headers, const float *data, uint64_t n, const float *lambda, float *out, hipStream_t s);

} // namespace mtsamd

// scene_build.h -- host-only scene ingestion: everything mtsamd_scene_create computes before the first byte goes to the device, and the
// host half of every parameter setter.  Nothing declared here calls the HIP runtime (kernels.h is included for the record types), so the
// whole path runs -- and is tested -- on a machine without a GPU (tests/test_scene_build_cpu.py); api.cpp uploads what it produces.
#pragma once
#include "../../include/mtsamd.h"
#include "bvh.h"
#include "envmap.h"
#include "kernels.h"
#include "spectral_upsampling.h"

#include <cstdint>
#include <vector>

namespace mtsamd {

// the thread's last error (mtsamd_last_error): fail() formats and stores the text and returns `code`
int fail(int code, const char *fmt, ...);
const char *last_error();

// ---- one function per conversion, shared by creation and by every setter ---------------------------------------------------
inline float rgb_mean(const float c[3]) { return (c[0] + c[1] + c[2]) * (1.0f / 3.0f); }       // Texture::mean() of a constant colour
// plastic.cpp:170-175: specular sampling weight from Texture::mean() of the diffuse and the specular reflectance
inline float plastic_lobe_weight(float d_mean, float s_mean) { return s_mean / (d_mean + s_mean); }
inline bool srgb_in_range(const float c[3]) { return !(c[0] < 0 || c[1] < 0 || c[2] < 0 || c[0] > 1 || c[1] > 1 || c[2] > 1); }
// `srgb` spectrum of a reflectance colour (srgb.cpp:31-41): range check with the constructor's message, model coefficients, their mean
// and -- jac9 not null -- d coeff / d rgb
int srgb_colour(const Rgb2Spec &model, const float rgb[3], float coeff[3], float *mean, float *jac9);
// `srgb_d65` spectrum of an emitter colour (srgb_d65.cpp:31-46, d65.cpp:44-50): coefficients of the normalised colour and d65_scale
void srgb_d65_colour(const Rgb2Spec &model, const float rgb[3], DevEmitter &e);
float bitmap_luminance_mean(const float *rgb, size_t n_texels);              // Texture::mean() of an RGB bitmap (bitmap.cpp:124-136)
bool invert_linear3(const float to_world[16], float inv[9]);                 // inverse of the upper 3x3, in double; false: singular
void bounding_sphere(const float bbox[6], float centre[3], float *radius);  // of Scene::bbox() (constant.cpp:47-51, directional.cpp:65-70)

// ---- tabulated / analytic spectra -------------------------------------------------------------------------------------------
int check_spectrum(const mtsamd_spectrum_desc &sp, uint32_t index, double *integral);
float spectrum_table_mean(double integral);
void build_spectrum_pool(const mtsamd_spectrum_desc *spectra, uint32_t n, std::vector<DevSpectrum> &headers, std::vector<float> &data);

// The geometry a scene keeps for mtsamd_scene_set_vertex_positions: counts and face indices are those of creation
struct SceneGeometry {
    std::vector<DevShape> shapes;                       // host copy of the shape records (first_prim, emitter, flags)
    std::vector<uint32_t> shape_vertices, shape_faces;  // per shape
    std::vector<uint32_t> faces;                        // 3 per primitive: vertex indices within the primitive's mesh
    std::vector<uint32_t> prim_shape;
    bool flat = false;
    std::vector<float> tri_pos, tri_nrm, area_pmf, area_cdf;      // flat scenes only (at most kFlatMaxPrims primitives): their records are rebuilt on the host
};

// What stays on the host for the life of a scene (mtsamd_scene embeds it): the records the setters edit and the queries read.
struct SceneState {
    int32_t environment = -1;        // index of the `constant` / `envmap` emitter
    bool general_bsdfs = false;      // any BSDF other than one-sided `diffuse`: the kernels with the BSDF switch are used
    bool nested_bsdfs = false;       // blendbsdf / mask: the fused schedule (k_bounce*, k_direct) is the one that carries the nesting code
    bool textured_params = false;    // some record reads alpha / specular colours from a texture (kBsdfTexParams): implies nested_bsdfs, whose
                                     // kernels resolve them; the setters refuse such a parameter and the adjoints such a scene (all but
                                     // mtsamd_render_adjoint_param_textures, which differentiates the texels of these maps)
    bool non_diffuse_bsdfs = false;  // any BSDF other than `diffuse` (one- or two-sided): what the adjoint path replay cannot differentiate
    bool delta_emitters = false;     // point / spot / directional emitters: handled by the same general kernels
    bool spectral = false;
    BvhOutput bvh;
    uint32_t n_prims = 0, n_shapes = 0;
    std::vector<DevBsdf> bsdfs;
    std::vector<DevEmitter> emitters;
    std::vector<DevTexture> textures;       // `data`: null until api.cpp uploads the texels (device pointers, owned by the scene)
    std::vector<float> spec_mean;           // per BSDF: mean of specular_reflectance
    std::vector<float> diff_mean;           // spectral variant, per BSDF: Texture::mean() of a constant reflectance
    Rgb2Spec rgb2spec;                      // spectral variant: the upsampling model, kept for parameter updates
    // spectral variant: d(model coefficients) / d(rgb) (srgb_model_fetch_jacobian) of every constant reflectance (9 floats per BSDF) and of
    // every bitmap texel (9 floats per texel, at 3 * grad_offset), recomputed whenever a colour is converted; `jac_dirty`: the device copy
    // (mtsamd_render_adjoint_spectral) is stale
    std::vector<float> jac_bsdf, jac_tex;
    bool jac_dirty = true;
    // spectral variant, emitter colours: the RGB texels of the envmap as the scene holds them (the device keeps coefficients); `ejac_dirty`:
    // the table of mtsamd_render_adjoint_spectral_emitters is stale
    std::vector<float> env_rgb;
    bool ejac_dirty = true;
    int32_t env_w = 0, env_h = 0;           // envmap emitter: its size (0: none)
    SceneGeometry geometry;
};

// builder knobs: the shipped values; experiment builds (-DMTSAMD_EXPERIMENTS) fill them from the environment in api.cpp
struct BuildOptions {
    uint32_t max_leaf = 4;
    BvhOptions bvh;
    uint32_t flat_max = kFlatMaxPrims;
};

// flat scenes: the LDS-resident records (build_flat_records)
struct FlatRecords {
    bool flat = false;                                  // n_prims <= flat_max and flat_launch_lds_max() <= kFlatLdsCap: the scene lives in LDS
    std::vector<float4> flat_recs, pair_recs;           // pair_recs: 5 per pair, then 2 per cluster
    uint32_t n_pairs = 0, n_clusters = 0;
};

// Everything creation computes on the host.  `state` outlives creation; the rest is uploaded and dropped.
struct HostScene : FlatRecords {
    SceneState state;
    std::vector<float> tri_pos, tri_nrm, tri_uv;       // 9 / 9 / 6 floats per primitive (normals, uvs: empty if no mesh has them)
    std::vector<uint32_t> prim_shape;
    std::vector<DevShape> shapes;
    std::vector<float> area_pmf, area_cdf;
    std::vector<DevBsdf> bsdf_block;                    // state.bsdfs, and behind them the spectrum pool (spectrum_pool() in kernels.hip)
    uint32_t n_spectra = 0;
    // texels of bitmap t as they are uploaded: tex_src[t] points into the description (RGB variant) or into tex_coeffs[t] (spectral
    // variant: model coefficients); null for a checkerboard
    std::vector<const float *> tex_src;
    std::vector<std::vector<float>> tex_coeffs;
    bool has_envmap = false;
    EnvmapHost env;                                     // texels (spectral variant: coefficients + scale) and sampling hierarchy
    DevEnvmap dev_env{};                                // all fields but the two device pointers
};

// Returns the ABI error code; the error text is set exactly as mtsamd_scene_create sets it.  tex_bindings: the textured parameters of
// mtsamd_scene_create_with_textures; they end up in the records (DevBsdf::nested0/1 and flags), so state.bsdfs shows them.
int build_host_scene(const mtsamd_scene_desc *desc, const mtsamd_spectrum_desc *spectra, uint32_t n_spectra,
                     const mtsamd_spectrum_binding *bindings, uint32_t n_bindings, const BuildOptions &options, HostScene &hs,
                     const mtsamd_texture_binding *tex_bindings = nullptr, uint32_t n_tex_bindings = 0);

// ---- the parts of creation that depend on vertex positions, callable on their own: creation and the vertex update share them ----------
float triangle_area(const float *tri_pos9);
// cdf and emitter fields (area_sum, area_norm, valid_lo / hi) of `face_count` areas; an emitter without area is refused with the reference's text
int area_distribution(const float *areas, uint32_t face_count, float *cdf, DevEmitter &e);
// bounding sphere of st.bvh.bbox into the records of the constant, envmap and directional emitters; then set_emitter_boxes
void set_scene_bounds(SceneState &st);
// Fated paths (fated.h): the exact box of an area emitter over `n_points` xyz triples that hold all its vertices (creation and every
// vertex update of its shape), and from these and st.bvh.bbox the padded boxes the device tests and the scene's list of them
void emitter_exact_box(const float *xyz, size_t n_points, DevEmitter &e);
void set_emitter_boxes(SceneState &st);
void build_flat_records(const BuildOptions &opt, const SceneState &st, const std::vector<float> &tri_pos, FlatRecords &out);
// refusals of a vertex update that need no look at the data, and the one that needs the (host) data
int check_vertex_update(const SceneState &st, uint32_t shape, const float *positions, const float *normals);
int check_finite(uint32_t shape, const float *positions, size_t n_floats);
// per primitive of `shape`: 9 floats of positions (and normals) from its vertex arrays, in primitive order from 0
void gather_shape(const SceneGeometry &g, uint32_t shape, const float *positions, const float *normals, float *tri_pos, float *tri_nrm);
// Mesh::recompute_vertex_normals (mesh.cpp:199-276) in fp32, built from vertex_normals.h: the specification the device kernels of
// refit.hip are held to, bit for bit, and what a flat scene uses.  faces: 3 vertex indices per face, each below vertex_count;
// normals_out: 3 per vertex, always finite (a vertex without a valid normal gets (1, 0, 0)).
void compute_vertex_normals(uint32_t vertex_count, const float *positions, uint32_t face_count, const uint32_t *faces, float *normals_out);
// The vertex-to-corner table of one mesh in CSR form, as the device gathers through it: corners[offsets[v] .. offsets[v + 1]) are the
// corners 3 * face + corner at which vertex v occurs, ascending, i.e. in the order compute_vertex_normals meets them.
void build_corner_table(uint32_t vertex_count, uint32_t face_count, const uint32_t *faces, std::vector<uint32_t> &offsets, std::vector<uint32_t> &corners);
// refusals of mtsamd_scene_update_vertices that concern its flags; what is left is check_vertex_update's with the normals the call will have
int check_vertex_flags(const SceneState &st, uint32_t shape, const float *normals, uint32_t flags);
// The whole update on the host: parameters_changed({"vertex_positions_buf"}) of one mesh over whole-scene arrays.  Flat scenes are
// updated this way; for hierarchy scenes it is the specification the device refit (refit.hip) is held to.  Nothing is written on a refusal.
int set_vertex_positions(SceneState &st, const BuildOptions &opt, uint32_t shape, const float *positions, const float *normals,
                         std::vector<float> &tri_pos, std::vector<float> &tri_nrm, std::vector<float> &area_pmf, std::vector<float> &area_cdf, FlatRecords &flat);

// ---- host half of the setters: they edit `st` and name what the device copy now lacks ------------------------------------------
// One scalar parameter of a BSDF record: which float(s) of DevBsdf it is.  false: the model has no such (differentiable) parameter.
bool bsdf_param_fields(const DevBsdf &b, int32_t kind, int32_t comp, float DevBsdf::*&f0, float DevBsdf::*&f1);
// Forward-mode render: the BSDF table at theta + eps t and theta - eps t and 1 / (2 eps) per record (0: no tangent), from
// bsdf_tangents[MTSAMD_BSDF_TANGENT_FLOATS * b + 3 * kind + comp] (null: no tangents, both tables are the scene's).  A non-zero entry must
// name a field bsdf_param_fields accepts for its record; a refusal names record, type and kind through fail().
int build_tangent_records(const SceneState &st, const float *bsdf_tangents, float h, std::vector<DevBsdf> &plus, std::vector<DevBsdf> &minus,
                          std::vector<float> &inv_2h);
// Reverse-mode render (k_reverse): one ReverseSlot (kernels.h) per wanted scalar, wanted[MTSAMD_BSDF_TANGENT_FLOATS * b + 3 * kind + comp] != 0,
// in record order, and range[b] .. range[b + 1] = the slots of record b (range has bsdf_count + 1 entries).  The pair of a slot and its
// inv_2h are bit for bit what build_tangent_records gives for the tangent that is 1 on that scalar and 0 elsewhere, stored as a patch
// of the record: the float offsets it moves and their plus / minus values.  Refusals are those of build_tangent_records, by name.
int build_reverse_slots(const SceneState &st, const uint8_t *wanted, float h, std::vector<ReverseSlot> &slots, std::vector<uint32_t> &range);
// blendbsdf / mask records in the forward and reverse renders (MTSAMD_FORWARD_NESTED / MTSAMD_REVERSE_NESTED, bit 4 of either descriptor).
bool has_nested_records(const SceneState &st);
// The flag rule of both descriptors and the refusals that depend on it: a bit is known only in a scene where it means something (bit 2:
// textured BSDF parameters; bit 4: an RGB scene with a blend / mask record).  `nested`: the call runs the nested kernels.
int check_derivative_flags(const SceneState &st, uint32_t flags, bool reverse, bool &nested);
// Takes the rows of blend / mask records out of a tangent and / or a wanted list (either may be null): entry 18 * b + 0 of nested record b
// is its weight / opacity -> weight_tangent[b] / weight_wanted[b]; everything else on such a row, and entry 0 of a textured weight, is
// refused by name.  rest_*: the inputs with those rows zeroed (empty for a null input), for build_tangent_records / build_reverse_slots.
int split_nested_rows(const SceneState &st, const float *bsdf_tangents, const uint8_t *bsdf_wanted, std::vector<float> &rest_tangents,
                      std::vector<float> &weight_tangent, std::vector<uint8_t> &rest_wanted, std::vector<uint8_t> &weight_wanted);
// One slot per wanted weight merged into the table of build_reverse_slots, in record order: f0 = f1 = kWeightSlot, out = 18 * record
void add_weight_slots(const std::vector<uint8_t> &weight_wanted, std::vector<ReverseSlot> &slots, std::vector<uint32_t> &range);
// these three change record `bsdf` / `emitter` only (valid indices) and the Jacobians behind jac_dirty / ejac_dirty
int set_bsdf_reflectance(SceneState &st, uint32_t bsdf, const float *rgb);
int set_bsdf_param(SceneState &st, uint32_t bsdf, int32_t kind, const float *value3);
int set_emitter_radiance(SceneState &st, uint32_t emitter, const float *rgb);
bool texture_feeds_lobe_weight(const SceneState &st, uint32_t texture);      // some (rough)plastic reads its mean
// New texels of bitmap `texture` (host copy, w * h * 3).  Spectral variant: clamps them to [0, 1] in place and returns their model
// coefficients in `coeffs` (what the device holds).  Either variant: updates the mean and lists the BSDF records whose lobe weight moved.
void set_texture_texels(SceneState &st, uint32_t texture, float *rgb, std::vector<float> &coeffs, std::vector<uint32_t> &changed_bsdfs);
// New texels of the envmap: `eh` receives the texel table (spectral variant: coefficients + scale) and the hierarchy to push
int set_envmap_texels(SceneState &st, const float *rgb, EnvmapHost &eh);

} // namespace mtsamd

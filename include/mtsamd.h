/* mtsamd.h -- C ABI of the MI355X (gfx950) wavefront path-tracing backend.
 *
 * This is the drop-in boundary for Mitsuba 2's path-tracing hot path.  Every entry
 * point names the reference interface it stands in for (paths relative to the
 * Mitsuba 2 source tree).  Conventions:
 *   - plain C, opaque handles, explicit sizes; no C++/torch types cross the boundary;
 *   - "dev" pointers are device (HIP) addresses owned by the caller; "host" pointers
 *     are ordinary host memory; the library never frees caller memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are
 *     asynchronous on that stream unless stated otherwise;
 *   - every function returns 0 on success and a negative mtsamd_status on failure;
 *     mtsamd_last_error() returns a thread-local description (the reference throws
 *     std::runtime_error via Throw(), include/mitsuba/core/logger.h:155-159);
 *   - handles are externally synchronised (one render at a time per handle), except
 *     mtsamd_cancel() which may be called from any thread
 *     (Integrator::cancel, include/mitsuba/render/integrator.h:44-51).
 */
#ifndef MTSAMD_H
#define MTSAMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTSAMD_ABI_VERSION 6
/* the library is built with -fvisibility=hidden: only the entry points below are exported */
#define MTSAMD_API __attribute__((visibility("default")))

typedef enum {
    MTSAMD_OK = 0,
    MTSAMD_ERR_INVALID = -1,   /* bad argument (the reference would Throw) */
    MTSAMD_ERR_DEVICE = -2,    /* HIP runtime error */
    MTSAMD_ERR_NOMEM = -3,
    MTSAMD_ERR_CANCELLED = -4, /* render stopped by mtsamd_cancel (render() returns false) */
    MTSAMD_ERR_UNSUPPORTED = -5
} mtsamd_status;

typedef struct mtsamd_scene mtsamd_scene;

/* ---- library ------------------------------------------------------------- */
MTSAMD_API int mtsamd_abi_version(void);
MTSAMD_API const char *mtsamd_last_error(void);
/* Number of HIP devices visible to this process (<0 on error). */
MTSAMD_API int mtsamd_device_count(void);
/* Plugin ABI of the reference (include/mitsuba/core/class.h:205-211, MTS_EXPORT_PLUGIN): PluginManager dlopen()s a
 * plugin .so and reads these two symbols (src/libcore/plugin.cpp:19-31).  The library answers for the `path_amd`
 * integrator shim shown in INTEGRATION.md, so that the shim can be this very shared object. */
MTSAMD_API const char *plugin_name(void);
MTSAMD_API const char *plugin_descr(void);

/* ---- scene description ----------------------------------------------------
 * Mesh buffers exactly as Mesh exposes them (include/mitsuba/render/mesh.h:80-90,
 * 328-332): packed xyz positions, optional packed normals / uv texcoords, u32 faces.
 * Geometry must already be in world space (the OBJ/PLY loaders bake to_world at load
 * time, src/shapes/obj.cpp:94-342). */
typedef struct {
    uint32_t vertex_count;
    uint32_t face_count;
    const float *positions;    /* host, 3 * vertex_count */
    const float *normals;      /* host, 3 * vertex_count, or NULL */
    const float *texcoords;    /* host, 2 * vertex_count, or NULL */
    const uint32_t *faces;     /* host, 3 * face_count */
    int32_t bsdf;              /* index into the bsdf table */
    int32_t emitter;           /* index into the emitter table, or -1 */
} mtsamd_mesh_desc;

/* BSDF plugins (constructor parameters after the host resolved defaults and named IORs):
 *   diffuse src/bsdfs/diffuse.cpp, conductor conductor.cpp, roughconductor roughconductor.cpp + microfacet.h,
 *   dielectric dielectric.cpp, roughdielectric roughdielectric.cpp, plastic plastic.cpp, roughplastic roughplastic.cpp (isotropic alpha_u);
 *   `twosided` = wrapped in the TwoSidedBRDF adapter (twosided.cpp). */
typedef enum { MTSAMD_BSDF_DIFFUSE = 0, MTSAMD_BSDF_CONDUCTOR = 1, MTSAMD_BSDF_ROUGHCONDUCTOR = 2, MTSAMD_BSDF_DIELECTRIC = 3,
               MTSAMD_BSDF_PLASTIC = 4, MTSAMD_BSDF_ROUGHPLASTIC = 5,
               MTSAMD_BSDF_ROUGHDIELECTRIC = 6,
               MTSAMD_BSDF_THINDIELECTRIC = 7 /* src/bsdfs/thindielectric.cpp: delta reflection + null transmission of a thin slab */,
               /* src/bsdfs/blendbsdf.cpp (weight * nested[1] + (1 - weight) * nested[0]) and src/bsdfs/mask.cpp (opacity * nested[0] +
                * a null lobe): `nested` index plain records of the same table (constant parameters; RGB variant: also a textured reflectance); the weight / opacity
                * is reflectance[0], or Texture::eval_1 of `texture` (luminance of a bitmap texel, bitmap.cpp:215-231; first colour
                * channel of a checkerboard cell).  `twosided` wraps a whole blend (mask transmits: twosided.cpp:78-80 refuses it). */
               MTSAMD_BSDF_BLEND = 8, MTSAMD_BSDF_MASK = 9 } mtsamd_bsdf_type;
typedef struct {
    int32_t type;              /* mtsamd_bsdf_type */
    float reflectance[3];      /* diffuse.reflectance / plastic.diffuse_reflectance: constant `srgb` value (src/spectra/srgb.cpp:27-52) */
    int32_t texture;           /* diffuse.reflectance as a bitmap: index into the texture table or -1 (src/textures/bitmap.cpp) */
    int32_t twosided;          /* != 0: both sides scatter like the front side (twosided.cpp:94-175) */
    float specular_reflectance[3];     /* default 1 */
    float specular_transmittance[3];   /* dielectric, default 1 */
    float eta[3], k[3];        /* conductors: complex index of refraction per colour channel (material "none": 0, 1) */
    float int_ior, ext_ior;    /* dielectric / plastic (ior.h) */
    float alpha_u, alpha_v;    /* roughconductor roughness */
    int32_t distribution;      /* 0 = beckmann, 1 = ggx */
    int32_t sample_visible;    /* visible-normal sampling (default true) */
    int32_t nonlinear;         /* plastic.nonlinear */
    int32_t uniform_mask;      /* spectral variant: bit 0 / 1 / 2 = reflectance / specular_reflectance / specular_transmittance is a
                                  constant (`uniform` spectrum, xml.cpp:1069-1083) rather than an RGB colour (`srgb`, upsampled);
                                  conductors need the same eta and k in all three channels (uniform) */
    int32_t nested[2];         /* MTSAMD_BSDF_BLEND: bsdf_0, bsdf_1; MTSAMD_BSDF_MASK: nested_bsdf, -1; otherwise ignored (ABI 5) */
} mtsamd_bsdf_desc;

/* area: src/emitters/area.cpp (attached to a mesh); constant: src/emitters/constant.cpp and envmap: src/emitters/envmap.cpp
 * (environment emitters, at most one per scene; spectral variant: `constant` radiance is upsampled like an area light's,
 * `envmap` texels become (model coefficients, scale) as in envmap.cpp:96-109) */
/* delta emitters: point src/emitters/point.cpp, spot spot.cpp (without projection texture), directional directional.cpp */
typedef enum { MTSAMD_EMITTER_AREA = 0, MTSAMD_EMITTER_CONSTANT = 1, MTSAMD_EMITTER_ENVMAP = 2, MTSAMD_EMITTER_POINT = 3,
               MTSAMD_EMITTER_SPOT = 4, MTSAMD_EMITTER_DIRECTIONAL = 5 } mtsamd_emitter_type;
typedef struct {
    int32_t type;              /* mtsamd_emitter_type; AreaLight = src/emitters/area.cpp */
    float radiance[3];         /* area / constant: radiance; point / spot: intensity; directional: irradiance */
    /* envmap: latitude-longitude image, linear RGB, host pointer (height * width * 3), `scale`, and the emitter's to_world
     * (row-major 4x4; the linear part is used) */
    const float *envmap_data;
    int32_t envmap_width, envmap_height;
    float envmap_scale;
    float to_world[16];        /* envmap; point / spot: position = translation; spot / directional: orientation (the light points
                                  along the local +z axis: spot.cpp:129-151, directional.cpp:104-129) */
    float cutoff_angle, beam_width;   /* spot, degrees (spot.cpp:81-82: defaults 20 and 3/4 of the cutoff angle, resolved by the host) */
} mtsamd_emitter_desc;

typedef struct {
    int32_t width, height;     /* bitmap (src/textures/bitmap.cpp): texels; channels = 3 (RGB) */
    const float *data;         /* host, height*width*3 (NULL for a checkerboard) */
    int32_t kind;              /* 0 = bitmap, 1 = checkerboard (src/textures/checkerboard.cpp) with constant colours */
    float color0[3], color1[3];
    float to_uv[6];            /* (m00, m01, m02, m10, m11, m12) of the extracted to_uv transform; all zero = identity */
} mtsamd_texture_desc;

typedef struct {
    const mtsamd_mesh_desc *meshes;       uint32_t mesh_count;
    const mtsamd_bsdf_desc *bsdfs;        uint32_t bsdf_count;
    const mtsamd_emitter_desc *emitters;  uint32_t emitter_count;
    const mtsamd_texture_desc *textures;  uint32_t texture_count;
    /* variant: 0 = *_rgb, 1 = *_spectral (4 wavelength samples, mitsuba.conf.template:135-138).  In spectral mode
     * RGB reflectances become SRGBReflectanceSpectrum and RGB radiances SRGBEmitterSpectrum (src/libcore/xml.cpp:1045-1146,
     * src/spectra/srgb.cpp, srgb_d65.cpp) through the coefficient table at rgb2spec_path ("data/srgb.coeff" in the
     * reference, src/librender/srgb.cpp:14-40; see mtsamd_rgb2spec_build). */
    int32_t spectral;
    const char *rgb2spec_path;
} mtsamd_scene_desc;

/* Scene::Scene + accel_init (src/librender/scene.cpp:22-98): uploads the geometry to
 * `device`, builds the BVH (replaces ShapeKDTree::build, include/mitsuba/render/kdtree.h:1710)
 * and the emitter sampling tables (Mesh::area_distr_build, src/librender/mesh.cpp:284-307).
 * Synchronous. */
MTSAMD_API int mtsamd_scene_create(const mtsamd_scene_desc *desc, int device, mtsamd_scene **out);
MTSAMD_API void mtsamd_scene_destroy(mtsamd_scene *scene);

/* ---- tabulated and analytic spectra (spectral variant) -----------------------
 * The spectrum plugins a spectral parameter may hold besides `srgb` / `uniform`:
 *   REGULAR    src/spectra/regular.cpp: `size` values at equal spacing over [lambda_min, lambda_max], evaluated as
 *              ContinuousDistribution::eval_pdf (include/mitsuba/core/distr_1d.h:378-393); `d65` (src/spectra/d65.cpp:44-66) is the
 *              95-entry table over 360..830 nm with values data[i] * (scale / 10568), expanded by the host
 *   IRREGULAR  src/spectra/irregular.cpp: `size` (wavelengths, values) nodes, IrregularContinuousDistribution::eval_pdf (distr_1d.h:655-677)
 *   BLACKBODY  src/spectra/blackbody.cpp:46-83: Planck's law at `temperature` kelvin, 0 outside 360..830 nm; emitters only
 * All are 0 outside their range.  The XML loader creates the first two from `<spectrum value="400:0.1, 500:0.7"/>` and
 * `<spectrum filename=.../>` (src/libcore/xml.cpp:1084-1125).  Arrays are host pointers, copied by the call. */
typedef enum { MTSAMD_SPECTRUM_REGULAR = 0, MTSAMD_SPECTRUM_IRREGULAR = 1, MTSAMD_SPECTRUM_BLACKBODY = 2 } mtsamd_spectrum_type;
typedef struct {
    int32_t type;              /* mtsamd_spectrum_type */
    uint32_t size;             /* REGULAR / IRREGULAR: number of entries, >= 2 */
    float lambda_min, lambda_max;      /* REGULAR: lambda_min < lambda_max (distr_1d.h:299) */
    const float *wavelengths;  /* IRREGULAR: `size` strictly increasing nodes (distr_1d.h:605); otherwise ignored */
    const float *values;       /* REGULAR / IRREGULAR: `size` non-negative values */
    float temperature;         /* BLACKBODY */
} mtsamd_spectrum_desc;
/* Binds spectrum `spectrum` of the call to one parameter: of BSDF record `index` -- param = MTSAMD_PARAM_REFLECTANCE (diffuse.reflectance,
 * (rough)plastic.diffuse_reflectance), SPECULAR_REFLECTANCE, SPECULAR_TRANSMITTANCE (dielectrics), ETA or K (conductors); children of
 * blendbsdf / mask are records of their own -- or the radiance / intensity / irradiance of emitter `index` (param ignored), which then IS
 * that spectrum: it is not multiplied by D65 as an `srgb_d65` colour is (src/spectra/srgb_d65.cpp:54-62).  The value the description
 * holds for a bound parameter is ignored.  Not bindable: blendbsdf / mask weights, textured reflectances, envmaps, dielectric IORs. */
typedef enum { MTSAMD_SPECTRUM_TARGET_BSDF = 0, MTSAMD_SPECTRUM_TARGET_EMITTER = 1 } mtsamd_spectrum_target;
typedef struct {
    int32_t target;            /* mtsamd_spectrum_target */
    uint32_t index;            /* bsdf record / emitter */
    int32_t param;             /* mtsamd_bsdf_param (BSDF targets) */
    uint32_t spectrum;         /* index into `spectra` */
} mtsamd_spectrum_binding;
/* mtsamd_scene_create for a scene whose parameters hold such spectra (what the reference's loader builds when the variant is spectral,
 * xml.cpp:1111-1125); mtsamd_scene_create is its case of no spectra.  Errors carry the reference's messages where it has them
 * (distr_1d.h:296-339, 564-618); a spectrum in an RGB-variant scene and a blackbody on a BSDF are refused.  Texture::mean() of a table --
 * its trapezoid integral / (830 - 360), regular.cpp:99-101, irregular.cpp:111-113 -- feeds the plastic lobe weights (plastic.cpp:170-175).
 * The setters below refuse a parameter that holds a spectrum, and the spectral adjoint entry points refuse such a scene. */
MTSAMD_API int mtsamd_scene_create_with_spectra(const mtsamd_scene_desc *desc, const mtsamd_spectrum_desc *spectra, uint32_t n_spectra,
                                     const mtsamd_spectrum_binding *bindings, uint32_t n_bindings, int device, mtsamd_scene **out);
/* ---- textured BSDF parameters (RGB variant) -------------------------------------
 * Binds texture `texture` of the description's texture table to one parameter of plain BSDF record `bsdf`, as the reference's
 * props.texture<Texture>(...) parameters allow: param = MTSAMD_PARAM_ALPHA (alpha_u and alpha_v share the texture), MTSAMD_PARAM_ALPHA_U,
 * MTSAMD_PARAM_ALPHA_V (roughconductor.cpp:173-182, roughdielectric.cpp:177-186; read per hit with Texture::eval_1: the luminance of a
 * bitmap texel, the first colour channel of a checkerboard cell; not clamped), MTSAMD_PARAM_SPECULAR_REFLECTANCE (conductor,
 * roughconductor, dielectric, roughdielectric, thindielectric) or MTSAMD_PARAM_SPECULAR_TRANSMITTANCE (the three dielectrics), read with
 * Texture::eval.  The value the description holds for a bound parameter is ignored by the kernels.  Children of blendbsdf / mask are
 * records of their own and bindable; blend / mask records themselves are not (their weight is mtsamd_bsdf_desc::texture), nor are
 * (rough)plastic parameters, eta / k, or anything in a spectral scene.  A texture may serve several bindings;
 * mtsamd_scene_update_texture updates it for all of them. */
typedef struct {
    uint32_t bsdf;             /* bsdf record */
    int32_t param;             /* mtsamd_bsdf_param */
    int32_t texture;           /* index into mtsamd_scene_desc::textures */
} mtsamd_texture_binding;
/* mtsamd_scene_create for a scene with such bindings; mtsamd_scene_create is its case of no bindings.  Such a scene renders with the
 * fused kernels that blendbsdf / mask scenes run (every `pipeline` value gives the same samples).  mtsamd_scene_set_bsdf_param refuses a
 * parameter that holds a texture.  The texels of such bitmaps are differentiated by mtsamd_render_adjoint_param_textures; the other adjoint
 * entry points refuse such a scene. */
MTSAMD_API int mtsamd_scene_create_with_textures(const mtsamd_scene_desc *desc, const mtsamd_texture_binding *bindings, uint32_t n_bindings,
                                      int device, mtsamd_scene **out);
/* Texture::eval of one spectrum (regular.cpp:68-75, irregular.cpp:76-83, blackbody.cpp:64-83) at n wavelengths: runs the device function
 * the render kernels call.  lambda_dev / out_dev: n floats on the device.  Returns when out_dev is complete. */
MTSAMD_API int mtsamd_spectrum_eval(const mtsamd_spectrum_desc *desc, uint64_t n, const float *lambda_dev, float *out_dev, void *stream);
/* Texture::mean() of a REGULAR / IRREGULAR spectrum (regular.cpp:99-101, irregular.cpp:111-113).  Host only. */
MTSAMD_API int mtsamd_spectrum_mean(const mtsamd_spectrum_desc *desc, float *mean);

/* Scene::bbox (include/mitsuba/render/scene.h): out6 = min xyz, max xyz (host). */
MTSAMD_API int mtsamd_scene_bbox(const mtsamd_scene *scene, float *out6);
/* Scene info: out[0]=primitive count, [1]=BVH node count, [2]=BVH depth, [3]=shape count,
 * [4]=emitter count, [5]=nodes resident in LDS. */
MTSAMD_API int mtsamd_scene_info(const mtsamd_scene *scene, uint32_t *out6);
/* parameters_changed() for constant reflectance / radiance / texture data
 * (src/spectra/srgb.cpp:59-61, src/textures/bitmap.cpp:295-299): host data, synchronous.
 * Spectral variant: the colours are `srgb` / `srgb_d65` spectra -- the setters redo the range check and the
 * coefficient fetch of scene creation (srgb.cpp:31-41, srgb_d65.cpp:31-46); a parameter that was given as a
 * `uniform` spectrum or a texture is not settable this way (MTSAMD_ERR_UNSUPPORTED). */
MTSAMD_API int mtsamd_scene_set_bsdf_reflectance(mtsamd_scene *scene, uint32_t bsdf, const float *rgb);
MTSAMD_API int mtsamd_scene_set_emitter_radiance(mtsamd_scene *scene, uint32_t emitter, const float *rgb);
/* BitmapTexture `data` parameter (bitmap.cpp:295-299): rgb is a host OR device pointer to height*width*3 floats;
 * asynchronous on `stream`.  Spectral variant: the texels are clamped to [0, 1] and converted to model coefficients on the host, as
 * scene creation converts them (the call waits for `stream` first and returns when the scene holds the new texels). */
MTSAMD_API int mtsamd_scene_update_texture(mtsamd_scene *scene, uint32_t texture, const float *rgb, void *stream);
/* Mesh `vertex_positions_buf` (mesh.cpp:781-804) of shape `shape`, i.e. parameters_changed({"vertex_positions_buf"}) of that mesh: its
 * vertex and face counts and its face indices stay those of creation.  positions / normals: host OR device pointers (told apart as
 * mtsamd_scene_update_texture tells them apart) to 3 * vertex_count floats of that mesh; `normals` is required exactly when the mesh was
 * created with normals and an error otherwise (recompute_vertex_normals: mtsamd_scene_update_vertices below).  The accelerator keeps its topology and
 * gets new boxes (a refit: on the device for hierarchy scenes); the area distribution of an emitter shape, the scene's bounding box,
 * the bounding sphere in the constant / envmap / directional emitter records and the records of a flat scene follow.  Samples and
 * queries afterwards equal, bit for bit, those of a scene created from the moved vertices.  Refused with MTSAMD_ERR_INVALID before
 * anything is written: a shape index out of range, missing or surplus normals, a non-finite coordinate, an area emitter left without
 * area ("DiscreteDistribution: no probability mass found!").  Every other setter's state is kept.  Waits for `stream` and returns when
 * the scene is consistent. */
MTSAMD_API int mtsamd_scene_set_vertex_positions(mtsamd_scene *scene, uint32_t shape, const float *positions, const float *normals, void *stream);
/* mtsamd_scene_set_vertex_positions with flags.  flags == 0: exactly that call (normals_out is not written).
 * MTSAMD_VERTICES_RECOMPUTE_NORMALS: the other half of parameters_changed({"vertex_positions_buf"}), recompute_vertex_normals
 * (mesh.cpp:199-276, called at mesh.cpp:797): `normals` must be NULL and the call behaves like mtsamd_scene_set_vertex_positions given
 * the normals mtsamd_compute_vertex_normals computes from `positions` and the mesh's faces -- on the device for hierarchy scenes (no
 * vertex data crosses to the host), bit for bit the same values.  normals_out (may be NULL): a host OR device pointer that receives
 * those 3 * vertex_count floats.  Refused with MTSAMD_ERR_INVALID, beside the refusals of mtsamd_scene_set_vertex_positions and like
 * them before anything is written: unknown flag bits; the flag together with `normals`; the flag on a mesh created without vertex
 * normals (the reference Throws: "Storing new normals in a Mesh that didn't have normals at construction time is not implemented
 * yet."). */
enum {
    MTSAMD_VERTICES_RECOMPUTE_NORMALS = 1,
    /* the update, then mtsamd_scene_rebuild_accel(scene, 0, stream) in the same call; combinable with the flag above.  The refusals of
     * the update come first and write nothing; a refused rebuild leaves the scene updated and refitted. */
    MTSAMD_VERTICES_REBUILD_ACCEL = 2,
    /* valid only together with MTSAMD_VERTICES_REBUILD_ACCEL (alone it is refused as an unknown flag): that rebuild is
     * mtsamd_scene_rebuild_accel_with(scene, MTSAMD_BUILDER_SAH, 0, stream).  Bit 2 (value 4) is not assigned. */
    MTSAMD_VERTICES_ACCEL_SAH = 8
};
MTSAMD_API int mtsamd_scene_update_vertices(mtsamd_scene *scene, uint32_t shape, const float *positions, const float *normals, uint32_t flags,
                                            float *normals_out, void *stream);
/* recompute_vertex_normals (mesh.cpp:199-276) in single precision, on the host; needs no scene and no device.  Face normals weighted by
 * the face's angle at each vertex (Thuermer & Wuethrich 1998), summed per vertex in the order of the faces; a face whose cross product
 * or one of whose edges has a squared length that is zero or not finite in fp32 is skipped; a vertex without a valid normal gets
 * (1, 0, 0).  positions: 3 * vertex_count floats; faces: 3 * face_count vertex indices; normals_out: 3 * vertex_count floats, always
 * finite.  MTSAMD_ERR_INVALID: a null array or a face index out of range. */
MTSAMD_API int mtsamd_compute_vertex_normals(uint32_t vertex_count, const float *positions, uint32_t face_count, const uint32_t *faces, float *normals_out);
/* Test aid: copies one device array of the accelerator to the host.  MTSAMD_ERR_INVALID unless `bytes` is that array's size. */
enum {
    MTSAMD_ACCEL_NODES = 0,      /* BVH2 nodes, 64 bytes each */
    MTSAMD_ACCEL_QNODES = 1,     /* BVH2 nodes on the 16-bit grid, 32 bytes each */
    MTSAMD_ACCEL_WNODES = 2,     /* BVH4 nodes in the encoding the build uses, 64 bytes each */
    MTSAMD_ACCEL_TRIS = 3,       /* triangle slots, 48 bytes each */
    MTSAMD_ACCEL_TRI_POS = 4,    /* 36 bytes per primitive */
    MTSAMD_ACCEL_TRI_NRM = 5,    /* 36 bytes per primitive; empty if no mesh has normals */
    MTSAMD_ACCEL_AREA_PMF = 6,   /* 4 bytes per primitive */
    MTSAMD_ACCEL_AREA_CDF = 7,
    MTSAMD_ACCEL_GRID = 8,       /* q_lo[3], q_step[3] as the kernels receive them: 24 bytes */
    /* the refit table of a hierarchy scene (empty for a flat one); builder nodes are the nodes of the binary tree, leaves included */
    MTSAMD_ACCEL_KIDS = 9,       /* per builder node (left, right), or (-1, leaf reference): 8 bytes */
    MTSAMD_ACCEL_ORDER = 10,     /* builder nodes by height above the leaves: 4 bytes each */
    MTSAMD_ACCEL_NODE_CHILD = 11,   /* per BVH2 node the builder nodes of its two children: 8 bytes */
    MTSAMD_ACCEL_WIDE_CHILD = 12,   /* per BVH4 node the builder nodes of its four children, -1: absent: 16 bytes */
    MTSAMD_ACCEL_BOXES = 13,     /* per builder node its exact box lo[3], hi[3]: 24 bytes */
    MTSAMD_ACCEL_SLOT_PRIM = 14  /* per triangle slot its primitive: 4 bytes */
};
MTSAMD_API int mtsamd_scene_read_accel(const mtsamd_scene *scene, int32_t which, void *host_dst, uint64_t bytes);
/* Rebuilds the topology of the accelerator on the device from the positions the scene holds now: after large vertex moves a refitted
 * tree keeps correctness, not quality (the reference rebuilds its acceleration structure on every parameters_changed,
 * src/librender/scene_optix.inl:260-411).  The new tree is an LBVH: Morton order of the triangle centres, the radix tree of Karras 2012,
 * leaves of the builder's leaf size, the BVH4 collapse of creation (the host function build_lbvh of csrc/bvh.h is its specification and
 * the device writes the same bytes).  flags must be 0 (MTSAMD_ERR_INVALID otherwise).  A flat scene (at most 64 primitives, no tree)
 * is left alone: MTSAMD_OK.  The hit of a ray does not depend on the tree, so queries and samples afterwards equal those before, bit for
 * bit; every setter's state is kept, and later vertex updates refit the new topology.  Refused with the scene exactly as it was:
 * MTSAMD_ERR_NOMEM, and MTSAMD_ERR_UNSUPPORTED for a tree too deep for the LDS traversal stack.  Waits for `stream` and returns when the
 * scene is consistent. */
MTSAMD_API int mtsamd_scene_rebuild_accel(mtsamd_scene *scene, uint32_t flags, void *stream);
/* mtsamd_scene_rebuild_accel with the builder named; the values are those mtsamd_scene_accel_info reports.  MTSAMD_BUILDER_LBVH: exactly
 * that call.  MTSAMD_BUILDER_SAH: the binned-SAH tree of creation, built level by level on the device (the host function
 * build_sah_levels of csrc/bvh.h is its specification and the device writes the same bytes): BVH2 and BVH4 nodes and the grid come out
 * byte for byte as those of a scene created from the positions the scene holds now, every leaf holds the same triangles (in ascending
 * primitive order), and mtsamd_scene_accel_info reports builder 0 afterwards.  One documented difference to creation: from depth 40 on a
 * node is split in the middle of its primitives' order, where creation takes an object median; only pathological sets reach it.
 * flags must be 0; an unknown builder is MTSAMD_ERR_INVALID.  Commit protocol, refusals (MTSAMD_ERR_NOMEM, MTSAMD_ERR_UNSUPPORTED: the
 * scene stays as it was), flat scenes (left alone, MTSAMD_OK) and later refits are those of mtsamd_scene_rebuild_accel. */
enum { MTSAMD_BUILDER_SAH = 0, MTSAMD_BUILDER_LBVH = 1 };
MTSAMD_API int mtsamd_scene_rebuild_accel_with(mtsamd_scene *scene, uint32_t builder, uint32_t flags, void *stream);
/* Measurement aid: the levels of the scene's last MTSAMD_BUILDER_SAH build.  *levels: their number (0: none yet); the first `capacity`
 * of them get nodes[i], the nodes of level i, and ms[i], the host's wall time for it (launches, scan and the wait for its count). */
MTSAMD_API int mtsamd_scene_rebuild_levels(const mtsamd_scene *scene, uint32_t capacity, uint32_t *nodes, float *ms, uint32_t *levels);
/* The accelerator a scene holds now.  out8: BVH2 nodes, BVH4 nodes, triangle slots, depth of the binary tree, depth of the BVH4,
 * entries of the traversal stack per lane, builder (0: the binned-SAH build of creation or of a MTSAMD_BUILDER_SAH rebuild, 1: the LBVH
 * of a rebuild), rebuilds so far.
 * sah_cost (may be NULL): the sum over the inner nodes of the binary tree of area / area(root) plus 1.5 times the sum over its leaves of
 * count * area / area(root), from the exact boxes the scene holds (computed on the device in double, in a fixed order): the number that
 * tells when a refitted tree has degraded enough to rebuild.  0 for a flat scene. */
MTSAMD_API int mtsamd_scene_accel_info(const mtsamd_scene *scene, uint32_t *out8, double *sah_cost);

/* ---- scene queries on SoA ray streams --------------------------------------
 * The stream layout follows the reference's device-stream precedent OptixParams
 * (include/mitsuba/render/optix/common.h:15-35): one float array per component,
 * one entry per ray, optional byte mask; inactive or missed lanes get t = +inf,
 * prim/shape = 0xffffffff (src/librender/optix/optix_rt.cu:35-37).
 * All array arguments are device pointers of `n` elements. */
typedef struct {
    const float *ox, *oy, *oz, *dx, *dy, *dz, *mint, *maxt;
    const uint8_t *active;     /* may be NULL */
} mtsamd_rays;

/* Scene::ray_intersect (include/mitsuba/render/scene.h:36; closest hit,
 * ShapeKDTree::ray_intersect_scalar<false>, kdtree.h:2079-2174): t, global primitive
 * index, shape index, barycentric u,v (the kd-tree "cache", kdtree.h:2432-2452). */
MTSAMD_API int mtsamd_ray_intersect(const mtsamd_scene *scene, uint64_t n, const mtsamd_rays *rays,
                         float *t, uint32_t *prim, uint32_t *shape, float *u, float *v,
                         void *stream);
/* Same query answered by brute force over all triangles
 * (Scene::ray_intersect_naive, scene.h:38-44 / kdtree.h:2303-2328) -- test aid. */
MTSAMD_API int mtsamd_ray_intersect_naive(const mtsamd_scene *scene, uint64_t n, const mtsamd_rays *rays,
                               float *t, uint32_t *prim, uint32_t *shape, float *u, float *v,
                               void *stream);
/* Scene::ray_test (scene.h:62; any hit, ray_intersect_scalar<true>). */
MTSAMD_API int mtsamd_ray_test(const mtsamd_scene *scene, uint64_t n, const mtsamd_rays *rays,
                    uint8_t *hit, void *stream);
/* Full SurfaceInteraction SoA for the closest hit (create_surface_interaction,
 * kdtree.h:2334-2367 + Mesh::fill_surface_interaction, src/librender/mesh.cpp:399-462;
 * GPU twin __closesthit__mesh, src/shapes/optix/mesh.cuh:27-96).  si26 is a device array of
 * 26 planes of n floats each: p(3) n(3) uv(2) sh_frame.s(3) sh_frame.t(3) sh_frame.n(3)
 * dp_du(3) dp_dv(3) wi(3). */
MTSAMD_API int mtsamd_ray_intersect_si(const mtsamd_scene *scene, uint64_t n, const mtsamd_rays *rays,
                            float *t, uint32_t *prim, uint32_t *shape, float *si26,
                            void *stream);

/* ---- operator API on device streams (RGB variant) ---------------------------
 * The operators a Python integrator or a BSDF plot composes, one query per row.  Every array argument is a device
 * pointer; inputs are one float array of n entries per component, `active` is an optional byte mask.  Outputs are
 * planes of n floats behind one pointer (plane k starts at out + k * n).  Inactive rows write zeros (emitter index
 * 0xffffffff); n = 0 is valid and launches nothing.  A scene of the spectral variant is refused
 * (MTSAMD_ERR_UNSUPPORTED) before the device is touched; component selection (BSDFContext::type_mask / component)
 * and TransportMode::Importance are not built. */
typedef struct {
    const uint32_t *shape;                 /* shape index of the interaction (SurfaceInteraction::shape): selects the BSDF;
                                              a row whose index is out of range is treated as inactive */
    const float *wi_x, *wi_y, *wi_z;       /* SurfaceInteraction::wi (local frame) */
    const float *u, *v;                    /* SurfaceInteraction::uv for textured parameters; may be NULL (0, 0) */
    const float *wo_x, *wo_y, *wo_z;       /* eval / pdf only */
    const float *sample1;                  /* sample only */
    const float *sample2_x, *sample2_y;    /* sample only */
    const uint8_t *active;                 /* may be NULL */
} mtsamd_bsdf_query;
/* BSDF::eval and BSDF::pdf (include/mitsuba/render/bsdf.h, eval / pdf with the default BSDFContext).
 * out4: value r, g, b (the cosine foreshortening factor included, as in the reference), pdf. */
MTSAMD_API int mtsamd_bsdf_eval_pdf(const mtsamd_scene *scene, uint64_t n, const mtsamd_bsdf_query *query, float *out4, void *stream);
/* BSDF::sample (bsdf.h).  out10: wo x, y, z, pdf, eta, delta flag (BSDFFlags::Delta of the sampled lobe, Null included),
 * weight r, g, b (value / pdf), valid flag.  An invalid sample has weight 0 and valid 0. */
MTSAMD_API int mtsamd_bsdf_sample(const mtsamd_scene *scene, uint64_t n, const mtsamd_bsdf_query *query, float *out10, void *stream);
/* Scene::sample_emitter_direction without its visibility test (src/librender/scene.cpp:165-189; the caller traces the
 * shadow rays with mtsamd_ray_test).  ref_p / sample2: 3 / 2 planes of n floats.  out15: DirectionSample p (3), n (3),
 * d (3), dist, pdf, delta flag, then the emitted radiance / pdf (3).  emitter: index of the sampled emitter per row.
 * A scene without emitters writes zeros. */
MTSAMD_API int mtsamd_sample_emitter_direction(const mtsamd_scene *scene, uint64_t n, const float *ref_p3, const float *sample2,
                                    const uint8_t *active, float *out15, uint32_t *emitter, void *stream);
/* Scene::pdf_emitter_direction (scene.cpp:191-206) for the emitter `emitter[i]` seen from the reference point along
 * d (3 planes) at distance dist, n (3 planes) = normal at the emitter.  Rows flagged delta (may be NULL), delta
 * emitters and index 0xffffffff give 0. */
MTSAMD_API int mtsamd_pdf_emitter_direction(const mtsamd_scene *scene, uint64_t n, const uint32_t *emitter, const float *d3, const float *n3,
                                 const float *dist, const uint8_t *delta, const uint8_t *active, float *pdf, void *stream);
/* Emitter::eval (include/mitsuba/render/emitter.h): an area emitter gives its radiance where wi.z > 0 (wi3: local wi of
 * the interaction on the emitter), the environment emitter its radiance for a ray that escaped along the world
 * direction d3; delta emitters and index 0xffffffff ("none") give 0.  out3: r, g, b. */
MTSAMD_API int mtsamd_emitter_eval(const mtsamd_scene *scene, uint64_t n, const uint32_t *emitter, const float *wi3, const float *d3,
                        const uint8_t *active, float *out3, void *stream);
/* IndependentSampler::seed (src/samplers/independent.cpp:62-72): lane i becomes the PCG32 stream the render kernels
 * give global sample index first + i under base_seed.  state / inc: n 64-bit words each, kept by the caller. */
MTSAMD_API int mtsamd_sampler_seed(uint64_t n, uint64_t first, uint64_t base_seed, uint64_t *state, uint64_t *inc, void *stream);
/* IndependentSampler::next_1d / next_2d (independent.cpp:76-94): dims = 1 or 2 planes of n floats; only active lanes
 * draw and advance. */
MTSAMD_API int mtsamd_sampler_next(uint64_t n, int32_t dims, uint64_t *state, const uint64_t *inc, const uint8_t *active, float *out,
                        void *stream);
/* Shape::bsdf / Shape::emitter (include/mitsuba/render/shape.h) for every shape: out3[3 i] = BSDF index, [3 i + 1] =
 * MTSAMD_BSDF_* flag word of that BSDF, [3 i + 2] = emitter index or -1.  Host array of 3 * shape count entries. */
enum { MTSAMD_BSDF_SMOOTH = 1, MTSAMD_BSDF_DELTA = 2, MTSAMD_BSDF_TWOSIDED = 4, MTSAMD_BSDF_NESTED = 8 };
MTSAMD_API int mtsamd_scene_shape_tables(const mtsamd_scene *scene, int32_t *out3);

/* ---- sensor / film / sampler / integrator ----------------------------------- */
/* src/rfilters/{gaussian,box,tent,catmullrom,mitchell,lanczos}.cpp */
typedef enum { MTSAMD_RFILTER_GAUSSIAN = 0, MTSAMD_RFILTER_BOX = 1, MTSAMD_RFILTER_TENT = 2, MTSAMD_RFILTER_CATMULLROM = 3,
               MTSAMD_RFILTER_MITCHELL = 4, MTSAMD_RFILTER_LANCZOS = 5 } mtsamd_rfilter_type;

typedef struct {
    /* PerspectiveCamera (src/sensors/perspective.cpp): to_world is row-major 4x4 */
    float to_world[16];
    float fov_x_deg;           /* horizontal fov in degrees (after parse_fov, src/librender/sensor.cpp:119-169) */
    float near_clip, far_clip; /* defaults 1e-2 / 1e4 (sensor.cpp:100-102) */
    /* Film (src/librender/film.cpp:7-64): size and crop window */
    int32_t film_width, film_height;
    int32_t crop_x, crop_y, crop_width, crop_height;
    /* ReconstructionFilter: gaussian stddev (src/rfilters/gaussian.cpp) / box radius (box.cpp) / mitchell B (mitchell.cpp:33) /
     * lanczos lobes (lanczos.cpp:34); param2: mitchell C; tent and catmullrom take no parameter */
    int32_t rfilter;           /* mtsamd_rfilter_type */
    float rfilter_param, rfilter_param2;
    int32_t rfilter_analytic;  /* 0: eval_discretized (scalar/packet variants, imageblock.cpp:131);
                                  1: eval() as the reference's GPU variants do (:132) */
    /* IndependentSampler (src/samplers/independent.cpp): sample_count, seed */
    int32_t sample_count;
    uint64_t seed;
    /* MonteCarloIntegrator (src/librender/integrator.cpp:283-296) */
    int32_t max_depth;         /* -1 = unbounded */
    int32_t rr_depth;          /* default 5 */
    /* work partition (multi-GPU film partition): only pixels of the rows this call owns are sampled;
     * their splats still land in the full crop-sized film, so the per-GPU films simply add up.
     * Either a window of crop-relative rows [row_begin,row_end) (row_end <= 0: all rows), or -- with
     * part_count > 1 -- tiles of part_tile_rows rows (32 = MTS_BLOCK_SIZE, include/mitsuba/render/spiral.h:10)
     * dealt round-robin: this call owns tiles t with t % part_count == part_index. */
    int32_t row_begin, row_end;
    int32_t part_index, part_count, part_tile_rows;
    /* scheduler knobs (0 = library default) */
    int32_t paths_per_wave;    /* in-flight path slots per scheduling wave */
    int32_t pipeline;          /* 0 = automatic: schedule 4 for LDS-resident scenes (<= 64 primitives), split trace / shade /
                                  trace kernels for hierarchy scenes; 1 = force the fused bounce kernel; 2 = force split;
                                  3 = LDS-resident scenes only: closest hit fused with shading, shadow rays queued and
                                  resolved in dense batches by a second kernel; 4 = LDS-resident scenes only: one kernel,
                                  shadow rays collected in a per-wave LDS ring and resolved 64 at a time (full waves in
                                  the any-hit loop).  All produce identical samples. */
    int32_t film_rgb;          /* 0: film channels X,Y,Z,A,W (integrator.cpp:72-74, 254-268);
                                  1: R,G,B,A,W -- linear RGB as mitsuba.python.autodiff._render_helper accumulates (autodiff.py:53-72) */
    int32_t integrator;        /* 0 = path (src/integrators/path.cpp), 1 = direct (direct.cpp), 2 = depth (depth.cpp) */
    int32_t emitter_samples;   /* direct: samples per technique; 0 and 0 = the shading_samples default (1, 1) (direct.cpp:80-103) */
    int32_t bsdf_samples;
    int32_t hide_emitters;     /* direct: do not add directly visible emitters (integrator.cpp:39, direct.cpp:117-121) */
    int32_t moment;            /* != 0: `moment` integrator around the selected one (src/integrators/moment.cpp:56-99): the film
                                  has 11 channels X,Y,Z,A,W, nested.X,nested.Y,nested.Z, m2_nested.X,m2_nested.Y,m2_nested.Z */
    /* ThinLensCamera (src/sensors/thinlens.cpp:110-118): aperture_radius > 0 selects the thin lens model -- two more sampler
     * dimensions per camera sample (integrator.cpp:229-231) -- focused at focus_distance (sensor.cpp:104); 0: pinhole */
    float aperture_radius, focus_distance;
    /* SamplingIntegrator properties (integrator.cpp:27-39) */
    float timeout;             /* seconds; <= 0: none.  Once exceeded no further pass is started and the running one is abandoned
                                  (should_stop(), integrator.h:143-146); the call still returns MTSAMD_OK: only cancel() makes
                                  render() return false (integrator.cpp:175) */
    int32_t samples_per_pass;  /* <= 0: all of sample_count.  sample_count must be a multiple of it (integrator.cpp:59-66); the
                                  image does not depend on it: the RNG streams are seeded per global sample index */
    int32_t profile;           /* != 0: every trace / shade launch of the split pipeline is bracketed by HIP timing events on
                                  the stream it is launched on (stats_host[8..13]) */
    /* scheduler knobs, continued (ABI 6; 0 = library default).  The image does not depend on them (tests/test_gpu_lifecycle.py). */
    int32_t max_pass_log2;     /* a pass holds at most 2^max_pass_log2 camera samples (10..30; default 30) */
    int32_t finish_kernel;     /* end of a pass: 0 = one k_finish launch once few paths are left, 1 = never (launch rounds until the
                                  pool is empty), 2 = as soon as the sample cursors are dry */
} mtsamd_render_desc;

/* SamplingIntegrator::render for the `path` integrator (src/librender/integrator.cpp:52-176,
 * src/integrators/path.cpp:100-211) followed by Film::put: renders the crop window and ADDS
 * the result into film_xyzaw_dev (crop_height*crop_width*5 floats, channels X,Y,Z,A,W as
 * prepared at integrator.cpp:72-74; zero it first for a fresh image).
 * Seeding follows the reference's wavefront branch (one PCG32 stream per sample index,
 * integrator.cpp:144-169, independent.cpp:69-72) with samples_per_pass = sample_count.
 * Synchronous on `stream` (returns when the film is complete).
 * stats_host (may be NULL, 16 entries): [0] closest-hit queries, [1] any-hit queries, [2] camera samples,
 * [3] scheduler iterations (k_bounce launches), [4] path segments shaded, [5] device time of the bounce loop in ns
 * (HIP events on `stream`), [6] device time of the film gather in ns, [7] triangle tests; with desc->profile and the
 * split pipeline: [8] summed duration of the k_trace<closest> launches in ns, [9] their number, [10] / [11] the same for
 * k_trace<any>, [12] / [13] for k_shade; [14] passes; [15] 1 if the render stopped at its timeout. */
MTSAMD_API int mtsamd_render(mtsamd_scene *scene, const mtsamd_render_desc *desc, float *film_xyzaw_dev,
                  uint64_t *stats_host, void *stream);
/* Integrator::cancel (integrator.h:51): thread-safe, makes a running mtsamd_render return
 * MTSAMD_ERR_CANCELLED at the next scheduling step. */
MTSAMD_API int mtsamd_cancel(mtsamd_scene *scene);

/* SamplingIntegrator::sample for whole sample indices (integrator.h:114-119): per-sample radiance
 * of samples [first, first+count) of the render described by desc, without film accumulation.
 * rgba_dev: count*4 floats (R,G,B, valid_ray mask); pos_dev (may be NULL): count*2 floats film
 * position sample.  Synchronous. */
MTSAMD_API int mtsamd_sample_radiance(mtsamd_scene *scene, const mtsamd_render_desc *desc, uint64_t first,
                           uint64_t count, float *rgba_dev, float *pos_dev, void *stream);

/* ---- aov integrator (src/integrators/aov.cpp) ----------------------------------
 * Fields of the camera ray's SurfaceInteraction as film channels (aov.cpp:92-134): depth = si.t (1 channel), position = si.p,
 * geo_normal = si.n, sh_normal = si.sh_frame.n, dp_du, dp_dv (3 channels each), uv (2 channels); duv_dx / duv_dy (2 channels each) are
 * accepted and always zero, as in the reference: kdtree.h:2353 zeroes them and aov.cpp never calls compute_partials.  Every channel is 0
 * where the camera ray misses (aov.cpp:171-172). */
typedef enum { MTSAMD_AOV_DEPTH = 0, MTSAMD_AOV_POSITION, MTSAMD_AOV_UV, MTSAMD_AOV_GEO_NORMAL, MTSAMD_AOV_SH_NORMAL,
               MTSAMD_AOV_DP_DU, MTSAMD_AOV_DP_DV, MTSAMD_AOV_DUV_DX, MTSAMD_AOV_DUV_DY } mtsamd_aov_type;
/* SamplingIntegrator::render (src/librender/integrator.cpp:52-176) for the `aov` integrator (aov.cpp:166-219) followed by Film::put.  The
 * film has the channels X,Y,Z,A,W, then the C channels of the n_aovs entries of aov_types in order (integrator.cpp:68-77), then -- nested != 0
 * -- R,G,B,A of the nested integrator desc->integrator (path / direct / depth; aov.cpp:195-213), which also fills X,Y,Z,A (nested == 0:
 * they stay 0, aov.cpp:215-216).  Every channel of a sample is splatted with the same filter weights, and the block is created with
 * warn_negative = false (integrator.cpp:249-270): a sample is dropped from all channels when one of them is not finite
 * (imageblock.cpp:85-109), negative values are kept.  The AOVs draw no random numbers: X,Y,Z,A,W equal those of mtsamd_render with the
 * same desc, R,G,B,A those of film_rgb = 1.  Spectral variant: X,Y,Z are the stream of mtsamd_render (which also drops samples below
 * -1e-5) and R,G,B its linear transform, where the reference converts the spectrum itself (equal up to rounding).
 * film_dev: crop_height * crop_width * (5 + C [+ 4]) floats, ADDED into.  desc->moment and desc->film_rgb must be 0, C <= 32, and
 * n_aovs == 0 needs nested != 0.  Row window, tile partition, crop, samples_per_pass, max_pass_log2, timeout and cancel act as in
 * mtsamd_render.  A render of several passes whose sample streams fit the scene's keep limit (below) keeps them for the duration of
 * the call and splats them once, so that its film equals the one-pass film bit for bit; above the limit every pass is splatted before the
 * next is traced and film rows reached from two passes may differ from the one-pass film in the last bits, as they do for mtsamd_render.
 * stats_host as for mtsamd_render; [0] and [7] include the
 * queries of the AOV kernel, [5] its device time, [6] the splats of every channel group (the stream kernel that unifies the drops, the
 * scratch-film clear and the channel interleave are in neither).  Two calls give the same bits. */
MTSAMD_API int mtsamd_render_aov(mtsamd_scene *scene, const mtsamd_render_desc *desc, const int32_t *aov_types, uint32_t n_aovs,
                      int32_t nested, float *film_dev, uint64_t *stats_host, void *stream);
/* Device memory a multi-pass mtsamd_render_aov may take to keep the streams of all its passes (see above): per sample 16 bytes for every
 * three AOV channels, 16 (32 with a nested integrator) for the radiance stream(s) and 8 for the film position (integrator.cpp:224-246
 * hands these to ImageBlock::put one sample at a time).  Default 2^30 bytes; 0: never keep, always splat pass by pass.  The choice
 * depends on the description and this limit only; if the device cannot provide memory within the limit, the render fails with
 * MTSAMD_ERR_NOMEM.  The memory is freed when the render returns. */
MTSAMD_API int mtsamd_scene_set_aov_keep_limit(mtsamd_scene *scene, uint64_t bytes);
/* The AOV part of AOVIntegrator::sample (aov.cpp:166-193) for whole sample indices, as mtsamd_sample_radiance: the C channel values of
 * the samples [first, first + count) of the render described by desc, without film accumulation.  aovs_dev: count * C floats,
 * sample-major; pos_dev (may be NULL): count * 2 floats, the film position (integrator.cpp:224-246).  Synchronous. */
MTSAMD_API int mtsamd_sample_aovs(mtsamd_scene *scene, const mtsamd_render_desc *desc, const int32_t *aov_types, uint32_t n_aovs,
                       uint64_t first, uint64_t count, float *aovs_dev, float *pos_dev, void *stream);

/* Reverse-mode derivative of mitsuba.python.autodiff.render (src/python/python/autodiff.py:6-91,121-194) with respect
 * to diffuse reflectances -- what `ek.backward()` propagates into 'bsdf.reflectance.value' (src/spectra/srgb.cpp:59-61)
 * and 'bsdf.reflectance.data' (src/textures/bitmap.cpp:295-299).  The image is values / (weight + 1e-8) of a film
 * rendered with `desc` and desc->film_rgb = 1 (channels R,G,B,A,W); dloss_dimage_dev holds dLoss/dImage
 * (crop_height*crop_width*3), film_dev that primal film.  Paths are replayed with the same per-sample PCG32 streams.
 * grad_bsdf_dev (bsdf_count*3), grad_textures_dev (all textures concatenated in index order, see
 * mtsamd_scene_texture_info) and grad_emitters_dev (emitter_count*3: the radiance of area lights,
 * 'shape.emitter.radiance.value', docs/src/inverse_rendering/diff_render.rst:76) are ACCUMULATED into; each may be NULL.
 * Needs 0 <= max_depth <= 16. */
MTSAMD_API int mtsamd_render_adjoint(mtsamd_scene *scene, const mtsamd_render_desc *desc, const float *dloss_dimage_dev,
                          const float *film_dev, float *grad_bsdf_dev, float *grad_textures_dev, float *grad_emitters_dev,
                          void *stream);
/* The same derivative with respect to the texels of the `envmap` emitter -- 'my_envmap.data' (src/emitters/envmap.cpp:214-218), the
 * parameter docs/examples/10_inverse_rendering/invert_bunny.py optimises.  The radiance is linear in the texels; the sampling
 * distribution built from their luminances is not differentiated (envmap.cpp:220-253 rebuilds it from plain floats).  Any BSDF,
 * any max_depth, RGB variant.  grad_envmap_dev: envmap height * width * 3 floats, ACCUMULATED into. */
MTSAMD_API int mtsamd_render_adjoint_envmap(mtsamd_scene *scene, const mtsamd_render_desc *desc, const float *dloss_dimage_dev,
                                 const float *film_dev, float *grad_envmap_dev, void *stream);
/* New texels for the envmap emitter (host pointer, height * width * 3 linear RGB; parameters_changed of envmap.cpp:220-253).
 * rebuild_distribution = 0 keeps the importance-sampling hierarchy of the previous texels (a render is then exactly linear in the
 * texels: finite-difference tests); the reference always rebuilds.  Synchronises the device.  Spectral variant: the texels are converted
 * to (model coefficients, scale) on the host as scene creation converts them; the hierarchy is built from the RGB luminances either way. */
/* Parameters of the BSDF models beyond `diffuse` (what traverse() exposes of e.g. roughconductor.cpp:393-404, plastic.cpp:299-307):
 * REFLECTANCE = diffuse.reflectance / (rough)plastic.diffuse_reflectance, SPECULAR_REFLECTANCE, SPECULAR_TRANSMITTANCE (dielectrics),
 * ETA / K (conductors), ALPHA (isotropic roughness of roughconductor / roughdielectric; one component).  ALPHA_U / ALPHA_V name one
 * roughness alone and exist for mtsamd_texture_binding and mtsamd_render_adjoint_param_textures only: the setters and the parameter
 * adjoint do not take them. */
typedef enum { MTSAMD_PARAM_REFLECTANCE = 0, MTSAMD_PARAM_SPECULAR_REFLECTANCE = 1, MTSAMD_PARAM_ETA = 2, MTSAMD_PARAM_K = 3, MTSAMD_PARAM_ALPHA = 4,
               MTSAMD_PARAM_SPECULAR_TRANSMITTANCE = 5, MTSAMD_PARAM_ALPHA_U = 6, MTSAMD_PARAM_ALPHA_V = 7 } mtsamd_bsdf_param;
/* parameters_changed() of a BSDF after one of these parameters was edited (constants): value3 = 3 floats (ALPHA: 1).  Spectral
 * variant: the three colour kinds become srgb spectra (as above), ETA / K must keep three equal components (uniform spectra). */
MTSAMD_API int mtsamd_scene_set_bsdf_param(mtsamd_scene *scene, uint32_t bsdf, int32_t param, const float *value3);
/* d(loss)/d(component of one such parameter) ADDED to *grad1_dev, for the image of mtsamd_render(film_rgb = 1) normalised as
 * mitsuba.python.autodiff.render does (src/python/python/autodiff.py:6-91): every camera sample is replayed with its PCG32 stream through
 * the general path step -- any BSDF, any emitter, any depth -- carrying the derivative forward beside the path.  Sampling is detached:
 * directions, lobe choices, MIS weights and Russian roulette are those of the primal path; the BSDF value at the fixed directions is
 * differentiated by a central difference of the model code (step h; <= 0: 1 % of the value).  The reference differentiates the attached
 * estimator through Enoki's autodiff graph; both are unbiased estimators of the same derivative (up to O(h^2)). */
MTSAMD_API int mtsamd_render_adjoint_param(mtsamd_scene *scene, const mtsamd_render_desc *desc, const float *dloss_dimage_dev,
                                const float *film_dev, uint32_t bsdf, int32_t param, int32_t component, float h,
                                float *grad1_dev, void *stream);
/* Forward-mode derivative render: the image of d(image)/d(t) along ONE tangent direction t over the scene parameters -- what
 * ek.set_gradient(param, t); ek.forward(param); ek.gradient(image) leaves behind in docs/examples/10_inverse_rendering/forward_diff.py
 * (docs/src/inverse_rendering/diff_render.rst:332-398).  RGB variant, `path` integrator, plain BSDF records (blendbsdf / mask under
 * MTSAMD_FORWARD_NESTED only; textured BSDF parameters under MTSAMD_FORWARD_PARAM_TEXTURES only), any emitter mix, any max_depth.  Every camera sample is replayed with its PCG32 stream through the general
 * path step with a dual part beside the path; one replay covers all four tangent families, whose contributions add up:
 *   bsdf_tangents         bsdf_count * MTSAMD_BSDF_TANGENT_FLOATS floats on the host: tangent[18 * bsdf + 3 * param + component] for param =
 *                         MTSAMD_PARAM_REFLECTANCE .. MTSAMD_PARAM_SPECULAR_TRANSMITTANCE (ALPHA: component 0 only).  A non-zero entry must
 *                         name a parameter mtsamd_render_adjoint_param accepts for that record.  Differentiated by a central difference of
 *                         the model code at the fixed directions between theta + eps t and theta - eps t, eps the largest step that moves
 *                         no scalar by more than h (h <= 0: 1 % of max(|theta|, 0.05)), ALPHA and ETA kept above 1e-4;
 *   emitter_tangents      emitter_count * 3 floats on the host: the colour of area, constant, point, spot and directional emitters
 *                         (radiance is linear in them; exact).  The row of an envmap is ignored;
 *   texture_tangents_dev  device, the layout of grad_textures_dev (mtsamd_scene_texture_info): texels of bitmaps used as
 *                         diffuse.reflectance / (rough)plastic.diffuse_reflectance, in closed form as mtsamd_render_adjoint_textures;
 *   envmap_tangent_dev    device, envmap height * width * 3: the texels of the envmap (the sampling hierarchy is not differentiated).
 * Each may be NULL, not all four.  Sampling is detached as in the adjoints: directions, pdfs, lobe choices, MIS weights and the survival
 * test are those of the primal path.  The Russian-roulette factor 1 / q (path.cpp:137-141) is differentiated as the reference and
 * mtsamd_render_adjoint do; MTSAMD_FORWARD_DETACH_ROULETTE holds it fixed, the convention of mtsamd_render_adjoint_param.
 * MTSAMD_FORWARD_PARAM_TEXTURES (opt-in; without it a scene with textured BSDF parameters is refused; in a scene without them the bit has
 * no meaning and stays refused with the unknown flag bits, so nothing such a scene is answered today changes) accepts scenes whose records read alpha / alpha_u / alpha_v / specular_reflectance / specular_transmittance from a
 * texture (mtsamd_texture_binding).  All four families then work as above, the untextured constants of a record with a map included
 * (eta / k beside an alpha map: plus / minus carry the looked-up values in the textured fields); a non-zero bsdf_tangents entry on a
 * parameter that its record reads from a texture is refused by name (ALPHA if either roughness is bound), and texture_tangents_dev also
 * carries the texels of bitmaps bound to BSDF parameters, at the same offsets: at a hit, every bound slot adds its central difference --
 * that of mtsamd_render_adjoint_param_textures, operation for operation: the two working records perturbed after the lookup, step h
 * absolute (<= 0: 1 % of the looked-up value, of at least 0.05; h MUST STAY BELOW THE SMALLEST ROUGHNESS OF A MAP), a colour's channels
 * moved together, one bitmap behind alpha_u and alpha_v moved as one parameter, a discrete lobe counted where both records re-sample the
 * primal direction -- times the bilinear lookup of the tangent texels over the slot's footprint (per channel for a colour; through the
 * luminance weights, or channel 0, for a roughness).  A bitmap that serves two bindings thus receives its total derivative.  Checkerboards
 * have no texels.  The Russian-roulette factor is differentiated for the map texels as for every other family (detached by the detach
 * bit), which mtsamd_render_adjoint_param_textures never does.
 * MTSAMD_FORWARD_NESTED (opt-in, under the same rule: known only in an RGB scene with at least one blendbsdf / mask record, the unknown bit
 * everywhere else; without it such a scene is refused as before) opens scenes with blendbsdf / mask records.  Children are ordinary records:
 * their constants use their own rows of bsdf_tangents, their reflectance texels texture_tangents_dev.  The weight / opacity of nested
 * record b is entry 18 * b + 0 (MTSAMD_PARAM_REFLECTANCE, component 0: the field the record keeps it in); every other entry of such a row
 * is refused by name, and so is entry 0 where the weight holds a texture -- the texels of a bitmap weight take their tangent in
 * texture_tangents_dev (luminance weights, or channel 0), a checkerboard has none.  With w the clamped weight at the hit and dw the
 * tangent of the raw value where 0 <= raw <= 1 (0 elsewhere):  blendbsdf, evaluated: df = (1 - w) df0 + w df1 + dw (f1 - f0); sampled,
 * child i chosen: dW = dW_i + W_i dw s, s = +1 / w for bsdf_1, -1 / (1 - w) for bsdf_0.  mask, evaluated: df = w df_c + dw f_c; child lobe
 * dW = dW_c + W_c dw / w, null lobe dW = -dw / (1 - w).  The s term is the derivative of the selection probability over itself -- the
 * probability is detached in the denominator and attached in the integrand, as plastic's lobe choice is here -- so the result is the
 * derivative of the EXPECTED image; the reference's automatic differentiation has no such term (its comparison masks carry no
 * derivative) and sees the weight through the emitter-sampling evaluation only.  MIS weights stay detached; the primal returns the
 * child's pdf after a child lobe but w * pdf in the evaluation, so with area lights or envmaps the weight derivative is that at frozen
 * MIS weights.  A scene with both nested records and textured BSDF parameters is refused. */
enum { MTSAMD_FORWARD_DETACH_ROULETTE = 1, MTSAMD_FORWARD_PARAM_TEXTURES = 2, MTSAMD_FORWARD_NESTED = 4 };
#define MTSAMD_BSDF_TANGENT_FLOATS 18
typedef struct {
    const float *bsdf_tangents;        /* host, bsdf_count * 18, or NULL */
    const float *emitter_tangents;     /* host, emitter_count * 3, or NULL (row of an envmap: ignored) */
    const float *texture_tangents_dev; /* device, layout of grad_textures, or NULL */
    const float *envmap_tangent_dev;   /* device, h * w * 3, or NULL */
    float h;                           /* as mtsamd_render_adjoint_param; <= 0: default.  Also the absolute step of the map slots (PARAM_TEXTURES) */
    uint32_t flags;                    /* MTSAMD_FORWARD_DETACH_ROULETTE | MTSAMD_FORWARD_PARAM_TEXTURES */
} mtsamd_tangent_desc;
/* The derivative film of the whole crop window: film_dev (crop_height * crop_width * 5 channels dR, dG, dB, A, W) is ADDED into, through
 * the film stage of mtsamd_render, in passes of whole rows (max_pass_log2 is respected); A and W equal those of the film mtsamd_render
 * writes for the same desc with film_rgb = 1, so the derivative image is dvalues / (W + 1e-8).  desc->film_rgb must be 1, integrator 0,
 * moment 0, no row window or tile partition, a reconstruction filter of at most 8 taps.  samples_per_pass, timeout and the scheduler
 * knobs (paths_per_wave, pipeline, finish_kernel, profile) are ignored: one thread replays one sample.  Device scratch belongs to the
 * scene; calls for one scene must be ordered on one stream.  Synchronises the stream. */
MTSAMD_API int mtsamd_render_forward(mtsamd_scene *scene, const mtsamd_render_desc *desc, const mtsamd_tangent_desc *tangent, float *film_dev,
                          void *stream);
/* The counterpart of mtsamd_sample_radiance: (dR, dG, dB, alpha) of the camera samples [first, first + count) into rgba_dev (count * 4)
 * and their film positions into pos_dev (count * 2, may be NULL). */
MTSAMD_API int mtsamd_sample_forward(mtsamd_scene *scene, const mtsamd_render_desc *desc, const mtsamd_tangent_desc *tangent, uint64_t first,
                          uint64_t count, float *rgba_dev, float *pos_dev, void *stream);
/* Reverse-mode render: the transpose of mtsamd_render_forward -- what ek.backward(loss) leaves in ek.gradient(param) for every parameter
 * at once (src/python/python/autodiff.py:6-91, docs/src/inverse_rendering/diff_render.rst:76-120).  ONE replay of every camera sample
 * with its PCG32 stream and ONE dLoss/dImage (dloss_dimage_dev: crop_height * crop_width * 3; film_dev: the primal film of
 * mtsamd_render with film_rgb = 1, whose weights normalise the image) give the gradient of every parameter the forward mode takes a
 * tangent for, in the layouts of mtsamd_tangent_desc, so that a gradient dots with a tangent entry by entry:
 *   bsdf_wanted / grad_bsdf_dev   wanted[18 * bsdf + 3 * param + component] != 0 marks a scalar mtsamd_render_adjoint_param accepts for that
 *                                 record; its derivative -- the central difference mtsamd_render_adjoint_param takes, step h -- is ADDED to
 *                                 the same entry of grad_bsdf_dev; the other entries are not touched.  Both or neither;
 *   grad_emitters_dev             emitter_count * 3: the colour of area, constant, point, spot and directional emitters (exact; the row
 *                                 of an envmap is not touched);
 *   grad_textures_dev             the layout of mtsamd_render_adjoint's grad_textures_dev: texels of bitmaps used as diffuse.reflectance /
 *                                 (rough)plastic.diffuse_reflectance, as mtsamd_render_adjoint_textures;
 *   grad_envmap_dev               envmap height * width * 3, as mtsamd_render_adjoint_envmap.
 * All are ACCUMULATED into; each may be NULL, not all four.  Scope and conventions are those of mtsamd_render_forward: RGB variant, `path`
 * integrator, film_rgb = 1, plain BSDF records, any emitter mix; sampling is detached and the Russian-roulette factor is differentiated
 * unless MTSAMD_REVERSE_DETACH_ROULETTE holds it fixed (the convention of mtsamd_render_adjoint_param).  Emitter and envmap gradients alone
 * run at any max_depth; BSDF scalars and texels record the path's vertices and need 0 <= max_depth <= 16.  The isfinite rule holds per
 * TERM, not per sample as in mtsamd_render_adjoint_param: a term (one vertex's contribution to one slot, one texel footprint, one emitter
 * row or one envmap footprint) that is not finite adds nothing, and the finite terms of the same sample stay.  The slot table uploaded for the wanted scalars belongs to the scene: calls for one scene must be ordered on
 * one stream.  Asynchronous on `stream` once the table is uploaded.
 * MTSAMD_REVERSE_PARAM_TEXTURES (opt-in, as MTSAMD_FORWARD_PARAM_TEXTURES: without it, and in scenes without textured BSDF parameters
 * with it, every refusal and result is what it was)
 * is the transpose of the forward render with that bit in a scene with textured BSDF parameters: wanted constants of every record (a
 * wanted flag on a parameter its record reads from a texture is refused by name), reflectance texels, emitter colours and envmap texels
 * as above, and grad_textures_dev additionally collects, for every bound slot of every recorded vertex, T' (delta dNc + a dW) of the
 * slot's central difference over the footprint of the slot's lookup -- the texel gradients of mtsamd_render_adjoint_param_textures for
 * all slots in this one replay, in the same layout, with the Russian-roulette term attached unless the detach bit is set.  In such a
 * scene any texel gradient records the vertices (8 more bytes each, the uv of the hit) and needs 0 <= max_depth <= 16.
 * MTSAMD_REVERSE_NESTED (opt-in, as MTSAMD_FORWARD_NESTED: known only in an RGB scene with a blendbsdf / mask record) is the transpose of
 * the forward render with that bit: a blend vertex scatters into the wanted slots and reflectance texels of both children, scaled by
 * 1 - w and w (a mask: of its child, by w), and into grad_bsdf_dev[18 * b] of the nested record b -- its weight / opacity, wanted through
 * bsdf_wanted[18 * b] -- or, for a bitmap weight, into its texels in grad_textures_dev.  Any other wanted entry of a nested record, and
 * entry 0 of a textured weight, is refused by name.  A wanted BSDF scalar (weights included) or any texel gradient records the vertices:
 * 0 <= max_depth <= 16; emitter and envmap gradients alone run at any depth.  The per-family adjoints keep refusing nested scenes. */
enum { MTSAMD_REVERSE_DETACH_ROULETTE = 1, MTSAMD_REVERSE_PARAM_TEXTURES = 2, MTSAMD_REVERSE_NESTED = 4 };
typedef struct {
    const uint8_t *bsdf_wanted;   /* host, bsdf_count * MTSAMD_BSDF_TANGENT_FLOATS: non-zero = this scalar is wanted; or NULL */
    float *grad_bsdf_dev;         /* device, bsdf_count * 18 floats, ACCUMULATED into at the wanted entries; NULL iff bsdf_wanted is NULL */
    float *grad_emitters_dev;     /* device, emitter_count * 3, ACCUMULATED; or NULL */
    float *grad_textures_dev;     /* device, layout of mtsamd_render_adjoint's grad_textures_dev, ACCUMULATED; or NULL */
    float *grad_envmap_dev;       /* device, h * w * 3, ACCUMULATED; or NULL */
    float h;                      /* central-difference step, as mtsamd_render_adjoint_param; <= 0: default.  Also the step of the map slots */
    uint32_t flags;               /* MTSAMD_REVERSE_DETACH_ROULETTE | MTSAMD_REVERSE_PARAM_TEXTURES */
} mtsamd_gradient_desc;
MTSAMD_API int mtsamd_render_reverse(mtsamd_scene *scene, const mtsamd_render_desc *desc, const float *dloss_dimage_dev,
                                     const float *film_dev, const mtsamd_gradient_desc *grad, void *stream);
/* The derivative with respect to bitmap texels ('bsdf.reflectance.data', src/textures/bitmap.cpp:295-299) in ANY RGB scene the path
 * integrator renders -- any emitter mix, any of the supported BSDFs -- of mitsuba.python.autodiff.render (autodiff.py:6-91): the texels of
 * bitmaps used as diffuse.reflectance or (rough)plastic.diffuse_reflectance (plain or inside `twosided`).  Every camera sample is replayed
 * with its PCG32 stream through the general path step, its vertices are swept backwards; BSDF values are differentiated in closed form at
 * the directions of the primal path (lobe probabilities, MIS weights and the specular sampling weight of plastic are held fixed), and
 * the Russian-roulette factor as mtsamd_render_adjoint does.  grad_textures_dev: the layout of mtsamd_render_adjoint (all textures
 * concatenated, offsets from mtsamd_scene_texture_info), ACCUMULATED into.  Needs 0 <= max_depth <= 16; no blendbsdf / mask. */
MTSAMD_API int mtsamd_render_adjoint_textures(mtsamd_scene *scene, const mtsamd_render_desc *desc, const float *dloss_dimage_dev,
                                   const float *film_dev, float *grad_textures_dev, void *stream);
/* The derivative with respect to the texels of bitmaps bound to BSDF PARAMETERS (mtsamd_texture_binding; 'bsdf.alpha.data',
 * 'bsdf.specular_reflectance.data', ...: src/textures/bitmap.cpp:295-299 behind roughconductor.cpp:393-404) in any RGB scene of plain BSDF
 * records the path integrator renders.  param = MTSAMD_PARAM_ALPHA_U, _ALPHA_V, _ALPHA (alpha_u then alpha_v), _SPECULAR_REFLECTANCE,
 * _SPECULAR_TRANSMITTANCE, or -1 for all four slots in turn; every slot is one replay of every camera sample with its PCG32 stream, whose
 * vertices are swept backwards as mtsamd_render_adjoint_textures sweeps them.  Sampling is detached as in mtsamd_render_adjoint_param:
 * directions, pdfs, lobe choices, MIS weights AND the Russian-roulette probability are those of the primal path, so the texel gradients of
 * a uniform map sum to what mtsamd_render_adjoint_param gives for the constant.  The model code is differentiated by a central difference
 * at the fixed directions, between two copies of the record perturbed in the slot after the lookup: step h, absolute and the same at
 * every hit (<= 0: 1 % of the value looked up at the hit, of at least 0.05).  h MUST STAY BELOW THE SMALLEST ROUGHNESS OF THE MAP: nothing
 * clamps alpha - h.  A colour slot moves its three channels together (the models are diagonal in their specular colours); a roughness
 * reaches the RGB texel through what Texture::eval_1 applied, the luminance weights of a bitmap.  A texture bound to alpha_u and one
 * bound to alpha_v each receive their own replay.  A texture bound to ALPHA (one lookup behind both roughnesses) is one parameter: the
 * alpha_u replay moves alpha_u and alpha_v of such a record together -- the central difference mtsamd_render_adjoint_param(ALPHA) takes --
 * and the alpha_v replay leaves the record alone, so the two replays of ALPHA still add up to its total derivative (adding the two
 * partial differences instead would miss the mixed third derivatives, 0.8 % at alpha = 0.1, h = 0.01).  A discrete lobe (conductor, dielectric,
 * thindielectric) counts where both perturbed records re-sample the very direction of the primal path.  Checkerboards have no texels.
 * grad_textures_dev: the layout of mtsamd_render_adjoint, ACCUMULATED into; a slot that no record binds leaves it untouched.  Needs
 * 0 <= max_depth <= 16; refuses spectral scenes, blendbsdf / mask records and any other param. */
MTSAMD_API int mtsamd_render_adjoint_param_textures(mtsamd_scene *scene, const mtsamd_render_desc *desc, const float *dloss_dimage_dev,
                                         const float *film_dev, int32_t param, float h, float *grad_textures_dev, void *stream);
/* Spectral variant: the derivative with respect to the reflectance family -- diffuse.reflectance and (rough)plastic.diffuse_reflectance
 * (plain or inside `twosided`), given as a constant `srgb` colour or as a bitmap -- in ANY spectral scene the path integrator renders.
 * The film channels differentiated are the X, Y, Z the spectral variant writes (with or without film_rgb).  Every camera sample is
 * replayed with its PCG32 stream through the general spectral path step and swept backwards on its four wavelengths; ALL sampling is
 * held fixed, the Russian-roulette probability included (the estimator of the true derivative of the image; mtsamd_render_adjoint*
 * differentiate that probability as Enoki does).  The gradient reaches RGB through the model coefficients: dS/dc in the kernel, then the
 * transposed Jacobian of srgb_model_fetch at each colour (kept by the scene).  grad_bsdf_dev: bsdf_count x 3 linear RGB (rows of other
 * records stay untouched); grad_textures_dev: the layout of mtsamd_render_adjoint.  Both are ACCUMULATED into; either may be NULL.
 * Needs 1 <= max_depth <= 16, no blendbsdf / mask, at most 32 BSDFs with grad_bsdf_dev.  The coefficient gradients and the Jacobians
 * live in scratch buffers the scene owns: calls for ONE scene must be ordered on one stream (or otherwise serialised). */
MTSAMD_API int mtsamd_render_adjoint_spectral(mtsamd_scene *scene, const mtsamd_render_desc *desc, const float *dloss_dimage_dev,
                                   const float *film_dev, float *grad_bsdf_dev, float *grad_textures_dev, void *stream);
/* Spectral variant: the derivative with respect to the emitter family -- the texels of the `envmap` emitter ('data', envmap.cpp:214-218)
 * and the radiance / intensity / irradiance of area, `constant`, `point`, `spot` and `directional` emitters -- in ANY spectral scene the
 * path integrator renders; film channels and seed as mtsamd_render_adjoint_spectral.  Such a colour is stored as (model coefficients c of
 * n = rgb / sc, scale sc = 2 max(r, g, b)).  The path's throughput, directions, pdfs, MIS weights and roulette do not depend on the emitted
 * spectrum, so every camera sample is replayed once with its PCG32 stream and each use of an emitter colour -- emission picked up, an
 * unoccluded emitter sample -- adds into the (c, sc) gradients of the colours it read; a finishing kernel takes them to RGB through
 * d c / d rgb (the Jacobian of srgb_model_fetch at n composed with d n / d rgb, kept by the scene) and d sc / d rgb.  Conventions:
 *  - the sampling distribution (the envmap hierarchy built from the luminances, the choice among emitters) is NOT differentiated;
 *  - a colour whose largest component is 0 is not differentiable (n = 0 / 0, sentinel coefficients): its gradient is 0, and it puts no
 *    NaN into the texels that share a bilinear footprint with it;
 *  - on a tie for the maximum, d sc / d rgb goes to the lowest channel that attains it (the one max(max(r, g), b) returns): a subgradient;
 *  - a sample the primal pass drops (negative or non-finite XYZ) contributes nothing.
 * grad_emitters_dev: emitter_count x 3 linear RGB (the row of an `envmap` emitter stays untouched); grad_envmap_dev: envmap height * width
 * * 3.  Both are ACCUMULATED into; either may be NULL.  Needs 1 <= max_depth <= 16, no blendbsdf / mask, at most 32 emitters with
 * grad_emitters_dev, an envmap with grad_envmap_dev.  Scratch buffers of the scene: calls for ONE scene must be ordered on one stream. */
MTSAMD_API int mtsamd_render_adjoint_spectral_emitters(mtsamd_scene *scene, const mtsamd_render_desc *desc, const float *dloss_dimage_dev,
                                            const float *film_dev, float *grad_emitters_dev, float *grad_envmap_dev, void *stream);
MTSAMD_API int mtsamd_scene_update_envmap(mtsamd_scene *scene, const float *rgb, int32_t rebuild_distribution);
/* Size of a bitmap texture and its float offset inside the concatenated texture-gradient buffer. */
/* RoughPlastic precomputation (roughplastic.cpp:380-399) of BSDF `bsdf`: out65[0..63] = external transmittance at
 * cos(theta) = i / 63, out65[64] = internal diffuse reflectance.  Host pointer. */
MTSAMD_API int mtsamd_scene_roughplastic_tables(const mtsamd_scene *scene, uint32_t bsdf, float *out65);
MTSAMD_API int mtsamd_scene_texture_info(const mtsamd_scene *scene, uint32_t texture, int32_t *width, int32_t *height,
                              uint64_t *grad_offset);

/* Generates the RGB -> spectrum coefficient table (the reference builds it at compile time with
 * ext/rgb2spec/rgb2spec_opt.cpp <resolution = 64> srgb.coeff, ext/rgb2spec/CMakeLists.txt:49-54) and writes it to
 * `path` in the same "SPEC" file format.  Host only; takes about a minute at resolution 64 on 8 threads. */
MTSAMD_API int mtsamd_rgb2spec_build(const char *path, int32_t resolution, int32_t threads);
/* srgb_model_fetch (src/librender/srgb.cpp:14-40): coefficients of the smooth spectrum for a linear sRGB colour. */
MTSAMD_API int mtsamd_srgb_model_fetch(const char *path, const float *rgb3, float *coeff3);
/* Its derivative: jac9[3 c + j] = d coeff_j / d rgb_c, the analytic derivative of the trilinear table lookup inside the cell of `rgb3`.
 * Zero for pure black and pure white (their coefficients are sentinels), a zero row for a component outside [0, 1].  Host only. */
MTSAMD_API int mtsamd_srgb_model_fetch_jacobian(const char *path, const float *rgb3, float *jac9);
/* An emitter colour of the spectral variant (envmap texel, radiance): coeff_scale4 = (c0, c1, c2, sc) with sc = 2 max(r, g, b) and
 * c = srgb_model_fetch(rgb3 / max(1e-8, sc)); jac9[3 ch + j] = d c_j / d rgb_ch, the Jacobian above composed with d n / d rgb (n of the
 * maximal channel is the constant 0.5; ties: the lowest such channel).  All zero for a colour whose largest component is <= 0.  Host only. */
MTSAMD_API int mtsamd_srgb_emitter_fetch_jacobian(const char *path, const float *rgb3, float *coeff_scale4, float *jac9);

/* PerspectiveCamera::sample_ray (perspective.cpp:153-188) / ThinLensCamera::sample_ray (thinlens.cpp:175-214) for n
 * film-plane samples in [0,1)^2 and, for a thin lens, n aperture samples (NULL: 0.5, as integrator.cpp:229 initialises them)
 * (device SoA in, device SoA out). */
MTSAMD_API int mtsamd_camera_sample_rays(const mtsamd_render_desc *desc, uint64_t n, const float *sx,
                              const float *sy, const float *aperture_x, const float *aperture_y, float *ox, float *oy, float *oz, float *dx,
                              float *dy, float *dz, float *mint, float *maxt, void *stream);

/* ---- ImageBlock / Film ------------------------------------------------------- */
/* ImageBlock::put(pos, value) (src/librender/imageblock.cpp:80-172) for n samples:
 * block of (width,height) at (offset_x,offset_y) with `border` pixels of apron
 * (0, or the filter's border_size); data_dev holds (height+2b)*(width+2b)*channels floats
 * and is accumulated into (float atomics, as the reference's scatter_add).
 * pos_dev: n*2 floats, values_dev: n*channels floats. */
MTSAMD_API int mtsamd_imageblock_put(int32_t width, int32_t height, int32_t offset_x, int32_t offset_y,
                          int32_t channels, int32_t rfilter, float rfilter_param, float rfilter_param2,
                          int32_t rfilter_analytic, int32_t border, uint64_t n,
                          const float *pos_dev, const float *values_dev, float *data_dev,
                          void *stream);
/* ImageBlock::put(const ImageBlock*) (imageblock.cpp:49-77, accumulate_2d bitmap.h:657-716):
 * target += source with clipping; both described by (w,h,offset,border). */
MTSAMD_API int mtsamd_imageblock_put_block(const float *src_dev, int32_t src_w, int32_t src_h, int32_t src_ox,
                                int32_t src_oy, int32_t src_border, float *dst_dev, int32_t dst_w,
                                int32_t dst_h, int32_t dst_ox, int32_t dst_oy, int32_t dst_border,
                                int32_t channels, void *stream);
/* ReconstructionFilter discretisation (src/libcore/rfilter.cpp:9-20): host outputs. */
MTSAMD_API int mtsamd_rfilter_info(int32_t rfilter, float rfilter_param, float rfilter_param2, float *table32_host,
                        float *radius_host, int32_t *border_host);
/* HDRFilm::bitmap (src/films/hdrfilm.cpp:249-320): XYZAW -> RGBA float32, n pixels. */
MTSAMD_API int mtsamd_film_develop(const float *xyzaw_dev, uint64_t n_pixels, float *rgba_dev, void *stream);
/* Elementary functions of the kernels (csrc/device_libm.h: the reference gets them from Enoki's polynomial kernels, e.g.
 * enoki::sincos in include/mitsuba/core/warp.h:54-90, exp / log / erf in include/mitsuba/render/microfacet.h:187-493), evaluated on
 * the device for n arguments.  fn: 0 sin, 1 cos, 2 tan, 3 exp, 4 log, 5 erf, 6 acos, 7 atan2(x = y-coordinate, y = x-coordinate), 8 atanh, 9 cosh;
 * y_dev is read by fn 7 only.  Lets a test prove that host and device produce the same bits. */
MTSAMD_API int mtsamd_libm_eval(int32_t fn, uint64_t n, const float *x_dev, const float *y_dev, float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif

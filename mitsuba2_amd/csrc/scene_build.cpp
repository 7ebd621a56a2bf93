// scene_build.cpp -- host-only scene ingestion (scene_build.h): description -> HostScene in named stages, the conversions they share with
// the parameter setters, and the host half of those setters.  No HIP runtime call in this file.
//
// Reference call stack this replaces:
//   Scene::Scene -> accel_init -> ShapeKDTree::build          src/librender/scene.cpp:22-98
#include "scene_build.h"
#include "fated.h"
#include "vertex_normals.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

namespace mtsamd {

namespace { thread_local std::string g_last_error; }

int fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    g_last_error = buf;
    return code;
}
const char *last_error() { return g_last_error.c_str(); }

// ---- conversions --------------------------------------------------------------------------------------------------------------
int srgb_colour(const Rgb2Spec &model, const float rgb[3], float coeff[3], float *mean, float *jac9) {
    if (!srgb_in_range(rgb))
        return fail(MTSAMD_ERR_INVALID, "Invalid RGB reflectance value [%g, %g, %g], must be in the range [0, 1]!", rgb[0], rgb[1], rgb[2]);
    srgb_model_fetch(model, rgb, coeff);
    *mean = srgb_model_mean(coeff);
    if (jac9) srgb_model_fetch_jacobian(model, rgb, jac9);
    return MTSAMD_OK;
}

void srgb_d65_colour(const Rgb2Spec &model, const float rgb[3], DevEmitter &e) {
    float color[3] = { rgb[0], rgb[1], rgb[2] }, coeff[3];
    const float scale = std::max(std::max(color[0], color[1]), color[2]) * 2.0f;
    if (scale != 0.0f) { const float r = 1.0f / scale; for (float &v : color) v *= r; }
    srgb_model_fetch(model, color, coeff);
    float d65_scale = 1.0f * scale;
    d65_scale *= 1.0f / 10568.0f;                      // d65.cpp:44-50
    e.c0 = coeff[0]; e.c1 = coeff[1]; e.c2 = coeff[2]; e.d65_scale = d65_scale;
}

float bitmap_luminance_mean(const float *rgb, size_t n_texels) {
    double mean = 0.0;
    for (size_t i = 0; i < n_texels; ++i) {
        const float *p = rgb + 3 * i;
        mean += (double) (p[0] * 0.212671f + p[1] * 0.715160f + p[2] * 0.072169f);
    }
    return (float) (mean / (double) n_texels);
}

bool invert_linear3(const float m[16], float out[9]) {
    const double a = m[0], b = m[1], c = m[2], d2 = m[4], e2 = m[5], f = m[6], g = m[8], h2 = m[9], i2 = m[10];
    const double det = a * (e2 * i2 - f * h2) - b * (d2 * i2 - f * g) + c * (d2 * h2 - e2 * g);
    if (det == 0.0) return false;
    const double inv[9] = { (e2 * i2 - f * h2) / det, (c * h2 - b * i2) / det, (b * f - c * e2) / det,
                            (f * g - d2 * i2) / det, (a * i2 - c * g) / det, (c * d2 - a * f) / det,
                            (d2 * h2 - e2 * g) / det, (b * g - a * h2) / det, (a * e2 - b * d2) / det };
    for (int k = 0; k < 9; ++k) out[k] = (float) inv[k];
    return true;
}

void bounding_sphere(const float bb[6], float centre[3], float *radius) {
    centre[0] = (bb[3] + bb[0]) * 0.5f; centre[1] = (bb[4] + bb[1]) * 0.5f; centre[2] = (bb[5] + bb[2]) * 0.5f;
    const float dx = centre[0] - bb[3], dy = centre[1] - bb[4], dz = centre[2] - bb[5];
    const float r = std::sqrt(std::fma(dz, dz, std::fma(dy, dy, dx * dx)));
    *radius = std::max(kRayEpsilon, r * (1.0f + kRayEpsilon));
}

// Spectral variant: bitmap texels -> model coefficients (bitmap.cpp:116-123) and their Jacobians, 9 floats per texel at 3 * grad_offset
// of `jac`; returns Texture::mean(): the mean of srgb_model_mean over the texels
static float spectral_texels(const Rgb2Spec &model, const float *rgb, size_t n_texels, std::vector<float> &coeffs, std::vector<float> &jac, uint32_t grad_offset) {
    coeffs.resize(3 * n_texels);
    if (jac.size() < 3 * (size_t) grad_offset + 9 * n_texels) jac.resize(3 * (size_t) grad_offset + 9 * n_texels, 0.0f);
    double mean = 0.0;
    for (size_t i = 0; i < n_texels; ++i) {
        srgb_model_fetch(model, rgb + 3 * i, coeffs.data() + 3 * i);
        srgb_model_fetch_jacobian(model, rgb + 3 * i, jac.data() + 3 * (size_t) grad_offset + 9 * i);
        mean += (double) srgb_model_mean(coeffs.data() + 3 * i);
    }
    return (float) (mean / (double) n_texels);
}

// Spectral variant: the RGBA texels of an envmap -> (model coefficients of the colour scaled to a 50% maximum, scale), in place
// (envmap.cpp:96-109); black: (0, 0, -inf), evaluates to 0 (srgb.cpp:31-33)
static void spectral_envmap_texels(const Rgb2Spec &model, float *texels4, size_t n_texels) {
    for (size_t i = 0; i < n_texels; ++i) {
        float *px = texels4 + 4 * i;
        const float sc = std::max(std::max(px[0], px[1]), px[2]) * 2.0f, dn = std::max(1e-8f, sc);
        float rgb_norm[3] = { px[0] / dn, px[1] / dn, px[2] / dn }, coeff[3];
        srgb_model_fetch(model, rgb_norm, coeff);
        px[0] = coeff[0]; px[1] = coeff[1]; px[2] = coeff[2]; px[3] = sc;
    }
}

// ---- tabulated / analytic spectra (mtsamd_spectrum_desc) ------------------------------------------
// the checks of ContinuousDistribution::update (distr_1d.h:293-345) and IrregularContinuousDistribution::update (distr_1d.h:561-622), with
// their messages; *integral (may be null): the trapezoid integral both compute in double
int check_spectrum(const mtsamd_spectrum_desc &sp, uint32_t index, double *integral) {
    if (integral) *integral = 0.0;
    if (sp.type == MTSAMD_SPECTRUM_BLACKBODY) {
        if (!(sp.temperature > 0.0f) || !std::isfinite(sp.temperature)) return fail(MTSAMD_ERR_INVALID, "spectrum %u: blackbody needs a positive temperature", index);
        return MTSAMD_OK;
    }
    if (sp.type != MTSAMD_SPECTRUM_REGULAR && sp.type != MTSAMD_SPECTRUM_IRREGULAR) return fail(MTSAMD_ERR_INVALID, "spectrum %u: unknown type %d", index, sp.type);
    const bool regular = sp.type == MTSAMD_SPECTRUM_REGULAR;
    const char *cls = regular ? "ContinuousDistribution" : "IrregularContinuousDistribution";
    if (sp.size < 2) return fail(MTSAMD_ERR_INVALID, "%s: needs at least two entries!", cls);
    if (!sp.values || (!regular && !sp.wavelengths)) return fail(MTSAMD_ERR_INVALID, "spectrum %u: null array", index);
    if (regular && !(sp.lambda_min < sp.lambda_max)) return fail(MTSAMD_ERR_INVALID, "ContinuousDistribution: invalid range!");
    const double interval = regular ? ((double) sp.lambda_max - (double) sp.lambda_min) / (sp.size - 1) : 0.0;
    double sum = 0.0; bool mass = false;
    for (uint32_t i = 0; i + 1 < sp.size; ++i) {
        const double y0 = (double) sp.values[i], y1 = (double) sp.values[i + 1];
        double dx = interval;
        if (!regular) {
            const double x0 = (double) sp.wavelengths[i], x1 = (double) sp.wavelengths[i + 1];
            if (!(x1 > x0)) return fail(MTSAMD_ERR_INVALID, "IrregularContinuousDistribution: node positions must be strictly increasing!");
            dx = x1 - x0;
        }
        const double value = 0.5 * dx * (y0 + y1);
        sum += value;
        if (!(y0 >= 0.0) || !(y1 >= 0.0)) return fail(MTSAMD_ERR_INVALID, "%s: entries must be non-negative!", cls);
        mass = mass || value > 0.0;
    }
    if (!mass) return fail(MTSAMD_ERR_INVALID, "%s: no probability mass found!", cls);
    if (integral) *integral = sum;
    return MTSAMD_OK;
}
// Texture::mean() of a table: integral / (MTS_WAVELENGTH_MAX - MTS_WAVELENGTH_MIN) (regular.cpp:99-101, irregular.cpp:111-113)
float spectrum_table_mean(double integral) { return (float) integral / (830.0f - 360.0f); }

// headers + node / value arrays of a spectrum pool (device_spectral.h); the descs have passed check_spectrum
void build_spectrum_pool(const mtsamd_spectrum_desc *spectra, uint32_t n, std::vector<DevSpectrum> &headers, std::vector<float> &data) {
    headers.assign(n, DevSpectrum{});
    data.clear();
    for (uint32_t i = 0; i < n; ++i) {
        const mtsamd_spectrum_desc &sp = spectra[i];
        DevSpectrum &h = headers[i];
        if (sp.type == MTSAMD_SPECTRUM_BLACKBODY) { h.kind = kSpectrumBlackbody; h.temperature = sp.temperature; continue; }
        h.size = sp.size;
        if (sp.type == MTSAMD_SPECTRUM_REGULAR) {
            h.kind = kSpectrumRegular; h.lambda_min = sp.lambda_min; h.lambda_max = sp.lambda_max;
            const double interval = ((double) sp.lambda_max - (double) sp.lambda_min) / (sp.size - 1);
            h.inv_interval = (float) (1.0 / interval);
        } else {
            h.kind = kSpectrumIrregular; h.lambda_min = sp.wavelengths[0]; h.lambda_max = sp.wavelengths[sp.size - 1];
            h.nodes = (uint32_t) data.size();
            data.insert(data.end(), sp.wavelengths, sp.wavelengths + sp.size);
        }
        h.values = (uint32_t) data.size();
        data.insert(data.end(), sp.values, sp.values + sp.size);
    }
}

namespace {

bool is_plastic(int32_t type) { return type == kBsdfPlastic || type == kBsdfRoughPlastic; }

// which spectrum slot of a record a mtsamd_bsdf_param names, or -1 if a record of this type has no such spectral parameter
int bsdf_spectrum_slot(int32_t type, int32_t param) {
    const bool conductor = type == MTSAMD_BSDF_CONDUCTOR || type == MTSAMD_BSDF_ROUGHCONDUCTOR;
    const bool dielectric = type == MTSAMD_BSDF_DIELECTRIC || type == MTSAMD_BSDF_ROUGHDIELECTRIC || type == MTSAMD_BSDF_THINDIELECTRIC;
    const bool plastic = type == MTSAMD_BSDF_PLASTIC || type == MTSAMD_BSDF_ROUGHPLASTIC;
    switch (param) {
    case MTSAMD_PARAM_REFLECTANCE: return (type == MTSAMD_BSDF_DIFFUSE || plastic) ? kSpecRefl : -1;
    case MTSAMD_PARAM_SPECULAR_REFLECTANCE: return (conductor || dielectric || plastic) ? kSpecSpec : -1;
    case MTSAMD_PARAM_SPECULAR_TRANSMITTANCE: return dielectric ? kSpecTrans : -1;
    case MTSAMD_PARAM_ETA: return conductor ? kSpecEta : -1;
    case MTSAMD_PARAM_K: return conductor ? kSpecK : -1;
    default: return -1;
    }
}

// Textured parameters (mtsamd_texture_binding): the slots of DevBsdf::nested0/1 a binding fills (bit k = slot k: kTexAlphaU, kTexAlphaV,
// kTexSpec, kTexTrans), or 0 with *why set: a record of this type has no such texture parameter in the reference, or none built here
const char *texture_param_name(int32_t param) {
    switch (param) {
    case MTSAMD_PARAM_REFLECTANCE: return "reflectance";
    case MTSAMD_PARAM_SPECULAR_REFLECTANCE: return "specular_reflectance";
    case MTSAMD_PARAM_SPECULAR_TRANSMITTANCE: return "specular_transmittance";
    case MTSAMD_PARAM_ETA: return "eta";
    case MTSAMD_PARAM_K: return "k";
    case MTSAMD_PARAM_ALPHA: return "alpha";
    case MTSAMD_PARAM_ALPHA_U: return "alpha_u";
    case MTSAMD_PARAM_ALPHA_V: return "alpha_v";
    default: return "(unknown)";
    }
}
uint32_t texture_param_slots(int32_t type, int32_t param, const char **why) {
    const bool conductor = type == MTSAMD_BSDF_CONDUCTOR || type == MTSAMD_BSDF_ROUGHCONDUCTOR;
    const bool dielectric = type == MTSAMD_BSDF_DIELECTRIC || type == MTSAMD_BSDF_ROUGHDIELECTRIC || type == MTSAMD_BSDF_THINDIELECTRIC;
    const bool plastic = type == MTSAMD_BSDF_PLASTIC || type == MTSAMD_BSDF_ROUGHPLASTIC;
    const bool rough = type == MTSAMD_BSDF_ROUGHCONDUCTOR || type == MTSAMD_BSDF_ROUGHDIELECTRIC;
    *why = "this model has no such parameter";
    switch (param) {
    case MTSAMD_PARAM_ALPHA: case MTSAMD_PARAM_ALPHA_U: case MTSAMD_PARAM_ALPHA_V:
        if (type == MTSAMD_BSDF_ROUGHPLASTIC) { *why = "the roughness of roughplastic is a float (roughplastic.cpp:222), not a texture"; return 0u; }
        if (!rough) return 0u;
        return param == MTSAMD_PARAM_ALPHA ? 3u : (param == MTSAMD_PARAM_ALPHA_U ? 1u : 2u);
    case MTSAMD_PARAM_SPECULAR_REFLECTANCE:
        if (plastic) { *why = "the mean of a (rough)plastic's specular_reflectance feeds its lobe weight: a texture there is not implemented"; return 0u; }
        return (conductor || dielectric) ? 4u : 0u;
    case MTSAMD_PARAM_SPECULAR_TRANSMITTANCE: return dielectric ? 8u : 0u;
    case MTSAMD_PARAM_ETA: case MTSAMD_PARAM_K:
        *why = "indices of refraction take no texture here (constants, or spectra in the spectral variant)"; return 0u;
    case MTSAMD_PARAM_REFLECTANCE:
        *why = "a textured reflectance is mtsamd_bsdf_desc::texture"; return 0u;
    default: return 0u;
    }
}

// the description with its spectra, as every stage sees it
struct Input {
    const mtsamd_scene_desc &desc;
    const mtsamd_spectrum_desc *spectra; uint32_t n_spectra;
    const mtsamd_spectrum_binding *bindings; uint32_t n_bindings;
    std::vector<double> integrals;       // per spectrum (check_spectrum)
    uint64_t total = 0;                  // primitives
    bool any_nrm = false, any_uv = false;
    const mtsamd_texture_binding *tex_bindings = nullptr; uint32_t n_tex_bindings = 0;       // textured parameters
    // BSDF `b` has a spectrum bound to the slot of `param` (slot >= 0: to that slot): the value in the description is ignored
    bool bound(uint32_t b, int32_t param, int slot = -1) const {
        for (uint32_t i = 0; i < n_bindings; ++i)
            if (bindings[i].target == MTSAMD_SPECTRUM_TARGET_BSDF && bindings[i].index == b &&
                (slot < 0 ? bindings[i].param == param : bsdf_spectrum_slot(desc.bsdfs[b].type, bindings[i].param) == slot)) return true;
        return false;
    }
};

// ---- stage 1: validate ----------------------------------------------------------------------------------------------------------
int check_spectrum_bindings(Input &in) {
    const mtsamd_scene_desc *desc = &in.desc;
    if ((in.n_spectra && !in.spectra) || (in.n_bindings && !in.bindings)) return fail(MTSAMD_ERR_INVALID, "mtsamd_scene_create_with_spectra: null argument");
    if ((in.n_spectra || in.n_bindings) && !desc->spectral)
        return fail(MTSAMD_ERR_UNSUPPORTED, "tabulated spectra need the spectral variant (the RGB variants pre-integrate them on the host, xml.cpp:1126-1143)");
    if (in.n_spectra > kMaxSpectra) return fail(MTSAMD_ERR_UNSUPPORTED, "at most %u spectra per scene (got %u)", kMaxSpectra, in.n_spectra);
    in.integrals.assign(in.n_spectra, 0.0);
    for (uint32_t i = 0; i < in.n_spectra; ++i)
        if (int rc = check_spectrum(in.spectra[i], i, &in.integrals[i])) return rc;
    for (uint32_t i = 0; i < in.n_bindings; ++i) {
        const mtsamd_spectrum_binding &b = in.bindings[i];
        if (b.spectrum >= in.n_spectra) return fail(MTSAMD_ERR_INVALID, "binding %u: spectrum index %u out of range", i, b.spectrum);
        if (b.target == MTSAMD_SPECTRUM_TARGET_BSDF) {
            if (b.index >= desc->bsdf_count) return fail(MTSAMD_ERR_INVALID, "binding %u: bsdf index %u out of range", i, b.index);
            if (in.spectra[b.spectrum].type == MTSAMD_SPECTRUM_BLACKBODY) return fail(MTSAMD_ERR_INVALID, "binding %u: a blackbody spectrum is an emission spectrum, not a BSDF parameter", i);
            const mtsamd_bsdf_desc &bd = desc->bsdfs[b.index];
            if (bsdf_spectrum_slot(bd.type, b.param) < 0 || (b.param == MTSAMD_PARAM_REFLECTANCE && bd.texture >= 0))
                return fail(MTSAMD_ERR_UNSUPPORTED, "binding %u: bsdf %u (type %d) takes no spectrum for parameter %d (texture weights, textured reflectances and dielectric IORs are not spectra)", i, b.index, bd.type, b.param);
        } else if (b.target == MTSAMD_SPECTRUM_TARGET_EMITTER) {
            if (b.index >= desc->emitter_count) return fail(MTSAMD_ERR_INVALID, "binding %u: emitter index %u out of range", i, b.index);
            if (desc->emitters[b.index].type == MTSAMD_EMITTER_ENVMAP) return fail(MTSAMD_ERR_UNSUPPORTED, "binding %u: an envmap takes no spectrum", i);
        } else return fail(MTSAMD_ERR_INVALID, "binding %u: unknown target %d", i, b.target);
    }
    return MTSAMD_OK;
}

int validate_meshes(Input &in, std::vector<int32_t> &emitter_shape) {
    const mtsamd_scene_desc *desc = &in.desc;
    for (uint32_t i = 0; i < desc->mesh_count; ++i) {
        const mtsamd_mesh_desc &m = desc->meshes[i];
        if (!m.positions || !m.faces || m.face_count == 0 || m.vertex_count == 0)
            return fail(MTSAMD_ERR_INVALID, "mesh %u: empty mesh", i);
        if (m.bsdf < 0 || (uint32_t) m.bsdf >= desc->bsdf_count) return fail(MTSAMD_ERR_INVALID, "mesh %u: invalid bsdf index %d", i, m.bsdf);
        if (m.emitter >= (int32_t) desc->emitter_count) return fail(MTSAMD_ERR_INVALID, "mesh %u: invalid emitter index %d", i, m.emitter);
        if (m.emitter >= 0) {
            // "An area emitter can be only be attached to a single shape." (area.cpp:64-66)
            if (emitter_shape[m.emitter] >= 0) return fail(MTSAMD_ERR_INVALID, "An area emitter can be only be attached to a single shape.");
            emitter_shape[m.emitter] = (int32_t) i;
        }
        for (uint64_t k = 0; k < 3ull * m.face_count; ++k)
            if (m.faces[k] >= m.vertex_count) return fail(MTSAMD_ERR_INVALID, "mesh %u: face index out of range", i);
        in.total += m.face_count;
        in.any_nrm |= m.normals != nullptr; in.any_uv |= m.texcoords != nullptr;
    }
    return MTSAMD_OK;
}

int validate_emitters(const mtsamd_scene_desc *desc, const std::vector<int32_t> &emitter_shape, int32_t &environment) {
    for (uint32_t e = 0; e < desc->emitter_count; ++e) {
        const int32_t et = desc->emitters[e].type;
        if (et == MTSAMD_EMITTER_CONSTANT || et == MTSAMD_EMITTER_ENVMAP) {
            if (emitter_shape[e] >= 0) return fail(MTSAMD_ERR_INVALID, "emitter %u: an environment emitter cannot be attached to a shape", e);
            if (environment >= 0) return fail(MTSAMD_ERR_INVALID, "Only one environment emitter can be specified per scene.");      // scene.cpp:45-46
            if (et == MTSAMD_EMITTER_ENVMAP && (!desc->emitters[e].envmap_data || desc->emitters[e].envmap_width < 2 || desc->emitters[e].envmap_height < 2))
                return fail(MTSAMD_ERR_INVALID, "emitter %u: the environment map must be at least 2x2 pixels in size", e);
            environment = (int32_t) e;
            continue;
        }
        if (et == MTSAMD_EMITTER_POINT || et == MTSAMD_EMITTER_SPOT || et == MTSAMD_EMITTER_DIRECTIONAL) {
            if (emitter_shape[e] >= 0) return fail(MTSAMD_ERR_INVALID, "emitter %u: a point / spot / directional emitter cannot be attached to a shape", e);
            if (et == MTSAMD_EMITTER_SPOT && !(desc->emitters[e].cutoff_angle >= desc->emitters[e].beam_width))
                return fail(MTSAMD_ERR_INVALID, "emitter %u: spot: cutoff_angle must not be smaller than beam_width", e);      // spot.cpp:89
            continue;
        }
        if (et != MTSAMD_EMITTER_AREA) return fail(MTSAMD_ERR_UNSUPPORTED, "emitter %u: unknown emitter type %d", e, et);
        if (emitter_shape[e] < 0) return fail(MTSAMD_ERR_INVALID, "emitter %u is not attached to a shape", e);
    }
    return MTSAMD_OK;
}

// textured parameters: every binding names a texture of the table and a parameter that the reference reads through a texture on a
// plain record of that model; the types of the records and the texture table have been checked
int check_texture_bindings(const Input &in) {
    const mtsamd_scene_desc *desc = &in.desc;
    if (in.n_tex_bindings && !in.tex_bindings) return fail(MTSAMD_ERR_INVALID, "mtsamd_scene_create_with_textures: null argument");
    std::vector<uint32_t> taken(desc->bsdf_count, 0u);       // slots bound so far, per record
    for (uint32_t i = 0; i < in.n_tex_bindings; ++i) {
        const mtsamd_texture_binding &b = in.tex_bindings[i];
        const char *name = texture_param_name(b.param);
        if (desc->spectral) {
            if (b.param == MTSAMD_PARAM_ALPHA || b.param == MTSAMD_PARAM_ALPHA_U || b.param == MTSAMD_PARAM_ALPHA_V)
                return fail(MTSAMD_ERR_UNSUPPORTED, "eval_1(): a bitmap / checkerboard %s is converted into spectra in the spectral variant (bitmap.cpp:218-222); use a constant", name);
            return fail(MTSAMD_ERR_UNSUPPORTED, "binding %u: a textured %s is implemented for the RGB variant only", i, name);
        }
        if (b.bsdf >= desc->bsdf_count) return fail(MTSAMD_ERR_INVALID, "binding %u: bsdf index %u out of range", i, b.bsdf);
        const int32_t type = desc->bsdfs[b.bsdf].type;
        if (type == MTSAMD_BSDF_BLEND || type == MTSAMD_BSDF_MASK)
            return fail(MTSAMD_ERR_UNSUPPORTED, "binding %u: bsdf %u is a blendbsdf / mask: bind %s on its children, which are records of their own", i, b.bsdf, name);
        const char *why;
        const uint32_t slots = texture_param_slots(type, b.param, &why);
        if (!slots) return fail(MTSAMD_ERR_UNSUPPORTED, "binding %u: bsdf %u (type %d) takes no texture for %s: %s", i, b.bsdf, type, name, why);
        if (b.texture < 0 || (uint32_t) b.texture >= desc->texture_count) return fail(MTSAMD_ERR_INVALID, "binding %u: invalid texture index %d for %s", i, b.texture, name);
        if ((uint32_t) b.texture >= kMaxParamTextures) return fail(MTSAMD_ERR_UNSUPPORTED, "binding %u: texture index %d for %s: a parameter can name the first %u textures only", i, b.texture, name, kMaxParamTextures);
        if (taken[b.bsdf] & slots)       // roughconductor.cpp:173-177: 'alpha' together with 'alpha_u' / 'alpha_v', or a parameter given twice
            return fail(MTSAMD_ERR_INVALID, "binding %u: %s of bsdf %u is bound already (Microfacet model: please specify either 'alpha' or 'alpha_u'/'alpha_v'.)", i, name, b.bsdf);
        taken[b.bsdf] |= slots;
    }
    return MTSAMD_OK;
}

int validate_bsdfs(const Input &in) {
    const mtsamd_scene_desc *desc = &in.desc;
    for (uint32_t b = 0; b < desc->bsdf_count; ++b) {
        const mtsamd_bsdf_desc &bd = desc->bsdfs[b];
        if (bd.type < MTSAMD_BSDF_DIFFUSE || bd.type > MTSAMD_BSDF_MASK) return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u: unknown BSDF type %d", b, bd.type);
        if (desc->spectral && (bd.type == MTSAMD_BSDF_CONDUCTOR || bd.type == MTSAMD_BSDF_ROUGHCONDUCTOR) &&
            ((!in.bound(b, MTSAMD_PARAM_ETA) && (bd.eta[0] != bd.eta[1] || bd.eta[0] != bd.eta[2])) || (!in.bound(b, MTSAMD_PARAM_K) && (bd.k[0] != bd.k[1] || bd.k[0] != bd.k[2]))))
            return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u: the spectral variant needs uniform (constant) eta and k spectra, or tabulated ones (mtsamd_scene_create_with_spectra)", b);
        if (bd.texture >= 0 && bd.type != MTSAMD_BSDF_DIFFUSE && bd.type != MTSAMD_BSDF_PLASTIC && bd.type != MTSAMD_BSDF_ROUGHPLASTIC &&
            bd.type != MTSAMD_BSDF_BLEND && bd.type != MTSAMD_BSDF_MASK)
            return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u: textures are implemented for diffuse.reflectance and (rough)plastic.diffuse_reflectance only", b);
        if (bd.type == MTSAMD_BSDF_ROUGHPLASTIC && (bd.int_ior == bd.ext_ior || bd.alpha_u != bd.alpha_v))
            return fail(MTSAMD_ERR_INVALID, bd.int_ior == bd.ext_ior ? "The interior and exterior indices of refraction must be positive and differ!"
                                                                      : "The 'roughplastic' plugin currently does not support anisotropic microfacet distributions!");
        if (bd.type == MTSAMD_BSDF_ROUGHDIELECTRIC && (bd.int_ior < 0.0f || bd.ext_ior < 0.0f || bd.int_ior == bd.ext_ior))
            return fail(MTSAMD_ERR_INVALID, "The interior and exterior indices of refraction must be positive and differ!");      // roughdielectric.cpp:153-155
        if ((bd.type == MTSAMD_BSDF_DIELECTRIC || bd.type == MTSAMD_BSDF_PLASTIC || bd.type == MTSAMD_BSDF_ROUGHPLASTIC || bd.type == MTSAMD_BSDF_ROUGHDIELECTRIC ||
             bd.type == MTSAMD_BSDF_THINDIELECTRIC) &&
            (bd.int_ior < 0.0f || bd.ext_ior < 0.0f || bd.ext_ior == 0.0f))
            return fail(MTSAMD_ERR_INVALID, "The interior and exterior indices of refraction must be positive!");      // dielectric.cpp:183-185
        if ((bd.type == MTSAMD_BSDF_DIELECTRIC || bd.type == MTSAMD_BSDF_ROUGHDIELECTRIC || bd.type == MTSAMD_BSDF_THINDIELECTRIC) && bd.twosided)
            return fail(MTSAMD_ERR_INVALID, "Only materials without a transmission component can be nested!");          // twosided.cpp:90-91
        if (bd.texture >= (int32_t) desc->texture_count) return fail(MTSAMD_ERR_INVALID, "bsdf %u: invalid texture index %d", b, bd.texture);
    }
    for (uint32_t t = 0; t < desc->texture_count; ++t) {
        if (!desc->textures) return fail(MTSAMD_ERR_INVALID, "null texture table");
        const mtsamd_texture_desc &td = desc->textures[t];
        if (td.kind != 0 && td.kind != 1) return fail(MTSAMD_ERR_UNSUPPORTED, "texture %u: unknown texture kind %d", t, td.kind);
        if (td.kind == 0 && (!td.data || td.width < 2 || td.height < 2))
            return fail(MTSAMD_ERR_INVALID, "texture %u: image must be at least 2x2 pixels in size", t);      // bitmap.cpp:101-107
    }
    return check_texture_bindings(in);
}

int validate(Input &in, int32_t &environment) {
    const mtsamd_scene_desc *desc = &in.desc;
    if (int rc = check_spectrum_bindings(in)) return rc;
    // an empty scene is valid (it renders to zeros: scenes.py:262-267 of the reference's integrator tests)
    if (desc->mesh_count > 0 && !desc->meshes) return fail(MTSAMD_ERR_INVALID, "scene has no shapes");
    if (desc->mesh_count > 0 && (desc->bsdf_count == 0 || !desc->bsdfs)) return fail(MTSAMD_ERR_INVALID, "scene has no BSDFs");
    std::vector<int32_t> emitter_shape(desc->emitter_count, -1);
    if (int rc = validate_meshes(in, emitter_shape)) return rc;
    if (int rc = validate_emitters(desc, emitter_shape, environment)) return rc;
    if (int rc = validate_bsdfs(in)) return rc;
    if (in.total >= (1ull << 27)) return fail(MTSAMD_ERR_UNSUPPORTED, "too many primitives (%llu)", (unsigned long long) in.total);
    return MTSAMD_OK;
}

// ---- stage 2: meshes -> one global primitive list, area distributions and the records of the area emitters --------------------
// Mesh::area_distr_build (mesh.cpp:284-307) + DiscreteDistribution::update (distr_1d.h:49-88) over the faces [off, off + face_count)
int area_emitter(const mtsamd_emitter_desc &ed, uint32_t shape, uint32_t off, uint32_t face_count, HostScene &hs, DevEmitter &e) {
    for (uint32_t f = 0; f < face_count; ++f) hs.area_pmf[off + f] = triangle_area(&hs.tri_pos[9 * (size_t) (off + f)]);
    std::memset(&e, 0, sizeof(e));
    e.r = ed.radiance[0]; e.g = ed.radiance[1]; e.b = ed.radiance[2];
    e.shape = shape; e.first_prim = off; e.n_prims = face_count;
    emitter_exact_box(&hs.tri_pos[9 * (size_t) off], 3 * (size_t) face_count, e);      // padded and listed by set_scene_bounds (stage 6)
    return area_distribution(&hs.area_pmf[off], face_count, &hs.area_cdf[off], e);
}

int flatten_meshes(const Input &in, HostScene &hs) {
    const mtsamd_scene_desc *desc = &in.desc;
    const uint64_t total = in.total;
    hs.tri_pos.assign(9 * total, 0.0f); hs.tri_nrm.assign(in.any_nrm ? 9 * total : 0, 0.0f); hs.tri_uv.assign(in.any_uv ? 6 * total : 0, 0.0f);
    hs.prim_shape.assign(total, 0u);
    hs.shapes.assign(desc->mesh_count, DevShape{});
    hs.area_pmf.assign(total, 0.0f); hs.area_cdf.assign(total, 0.0f);
    SceneGeometry &g = hs.state.geometry;       // what a vertex update needs later
    g.faces.assign(3 * total, 0u); g.shape_vertices.assign(desc->mesh_count, 0u); g.shape_faces.assign(desc->mesh_count, 0u);
    uint32_t off = 0;
    for (uint32_t i = 0; i < desc->mesh_count; ++i) {
        const mtsamd_mesh_desc &m = desc->meshes[i];
        DevShape &sh = hs.shapes[i];
        sh.bsdf = m.bsdf; sh.emitter = m.emitter; sh.first_prim = off;
        sh.flags = (m.normals ? kShapeHasNormals : 0u) | (m.texcoords ? kShapeHasUV : 0u);
        g.shape_vertices[i] = m.vertex_count; g.shape_faces[i] = m.face_count;
        for (uint32_t f = 0; f < m.face_count; ++f) {
            uint32_t gp = off + f;
            hs.prim_shape[gp] = i;
            for (int j = 0; j < 3; ++j) {
                uint32_t vi = m.faces[3 * f + j];
                g.faces[3 * (size_t) gp + j] = vi;
                for (int k = 0; k < 3; ++k) hs.tri_pos[9 * (size_t) gp + 3 * j + k] = m.positions[3 * (size_t) vi + k];
                if (m.normals) for (int k = 0; k < 3; ++k) hs.tri_nrm[9 * (size_t) gp + 3 * j + k] = m.normals[3 * (size_t) vi + k];
                if (m.texcoords) for (int k = 0; k < 2; ++k) hs.tri_uv[6 * (size_t) gp + 2 * j + k] = m.texcoords[2 * (size_t) vi + k];
            }
        }
        if (m.emitter >= 0)
            if (int rc = area_emitter(desc->emitters[m.emitter], i, off, m.face_count, hs, hs.state.emitters[m.emitter])) return rc;
        off += m.face_count;
    }
    g.shapes = hs.shapes; g.prim_shape = hs.prim_shape;
    return MTSAMD_OK;
}

// ---- stage 3: delta emitters (point.cpp:52-65, spot.cpp:68-91, directional.cpp:43-63) and the spectra of all emitter colours ----
int build_emitters(const mtsamd_scene_desc *desc, SceneState &st) {
    for (uint32_t ei = 0; ei < desc->emitter_count; ++ei) {
        const mtsamd_emitter_desc &ed = desc->emitters[ei];
        if (ed.type != MTSAMD_EMITTER_POINT && ed.type != MTSAMD_EMITTER_SPOT && ed.type != MTSAMD_EMITTER_DIRECTIONAL) continue;
        DevEmitter &e = st.emitters[ei];
        std::memset(&e, 0, sizeof(e));
        st.delta_emitters = true;
        e.r = ed.radiance[0]; e.g = ed.radiance[1]; e.b = ed.radiance[2];
        e.shape = 0xffffffffu; e.pad0 = (uint32_t) ed.type;
        const float *m = ed.to_world;
        e.cx = m[3]; e.cy = m[7]; e.cz = m[11];
        if (ed.type == MTSAMD_EMITTER_DIRECTIONAL) {             // d = to_world * (0, 0, 1)
            e.aux[0] = m[2]; e.aux[1] = m[6]; e.aux[2] = m[10];
        } else if (ed.type == MTSAMD_EMITTER_SPOT) {
            if (!invert_linear3(m, e.aux)) return fail(MTSAMD_ERR_INVALID, "emitter %u: singular to_world transformation", ei);
            const float cutoff = ed.cutoff_angle * (kPi / 180.0f), beam = ed.beam_width * (kPi / 180.0f);
            e.aux[9] = cutoff; e.aux[10] = std::cos(cutoff); e.aux[11] = std::cos(beam); e.aux[12] = 1.0f / (cutoff - beam);
        }
    }
    // spectral variant: RGB -> spectrum coefficients on the host (srgb.cpp:31-41, srgb_d65.cpp:31-46)
    if (desc->spectral) {
        if (!desc->rgb2spec_path || !rgb2spec_load(desc->rgb2spec_path, st.rgb2spec))
            return fail(MTSAMD_ERR_INVALID, "Could not load sRGB-to-spectrum upsampling model ('%s'); build it with mtsamd_rgb2spec_build",
                        desc->rgb2spec_path ? desc->rgb2spec_path : "(null)");
        st.spectral = true;
        for (uint32_t e = 0; e < desc->emitter_count; ++e) srgb_d65_colour(st.rgb2spec, desc->emitters[e].radiance, st.emitters[e]);
    }
    return MTSAMD_OK;
}

// ---- stage 4: BSDF records --------------------------------------------------------------------------------------------------------
// Model parameters of a BSDF -> device record (see DevBsdf in device_bsdf.h), with the constants the reference's
// constructors derive (plastic.cpp:162-176; fresnel_diffuse_reflectance: fresnel.h:331-358).
float fresnel_diffuse_reflectance(float eta) {
    if (eta < 1.0f) return -1.4399f * (eta * eta) + 0.7099f * eta + 0.6681f + 0.0636f / eta;
    const float i1 = 1.0f / eta, i2 = i1 * i1, i3 = i2 * i1, i4 = i3 * i1, i5 = i4 * i1;
    return 0.919317f - 3.4793f * i1 + 6.75335f * i2 - 7.80989f * i3 + 4.98554f * i4 - 1.36881f * i5;
}
void fill_bsdf_model(const mtsamd_bsdf_desc &bd, DevBsdf &d) {
    d.flags = (bd.twosided ? kBsdfTwoSided : 0u) | (bd.distribution == 1 ? kBsdfGGX : 0u) | (bd.sample_visible ? kBsdfSampleVisible : 0u) |
              (bd.nonlinear ? kBsdfNonlinear : 0u);
    if (bd.type == MTSAMD_BSDF_DIFFUSE) d.flags &= kBsdfTwoSided;
    d.flags |= ((bd.uniform_mask & 1) ? kBsdfUniformRefl : 0u) | ((bd.uniform_mask & 2) ? kBsdfUniformSpec : 0u) |
               ((bd.uniform_mask & 4) ? kBsdfUniformTrans : 0u);
    d.sr = bd.specular_reflectance[0]; d.sg = bd.specular_reflectance[1]; d.sb = bd.specular_reflectance[2];
    d.alpha_u = bd.alpha_u; d.alpha_v = bd.alpha_v;
    if (bd.type == MTSAMD_BSDF_CONDUCTOR || bd.type == MTSAMD_BSDF_ROUGHCONDUCTOR) {
        d.er = bd.eta[0]; d.eg = bd.eta[1]; d.eb = bd.eta[2];
        d.kr = bd.k[0]; d.kg = bd.k[1]; d.kb = bd.k[2];
    } else if (bd.type == MTSAMD_BSDF_DIELECTRIC || bd.type == MTSAMD_BSDF_ROUGHDIELECTRIC || bd.type == MTSAMD_BSDF_THINDIELECTRIC) {
        d.er = bd.int_ior / bd.ext_ior;
        d.kr = bd.specular_transmittance[0]; d.kg = bd.specular_transmittance[1]; d.kb = bd.specular_transmittance[2];
    } else if (bd.type == MTSAMD_BSDF_PLASTIC || bd.type == MTSAMD_BSDF_ROUGHPLASTIC) {
        const float eta = bd.int_ior / bd.ext_ior;
        d.er = eta; d.eg = 1.0f / (eta * eta);
        d.eb = bd.type == MTSAMD_BSDF_PLASTIC ? fresnel_diffuse_reflectance(1.0f / eta) : 0.0f;     // roughplastic: set by the table kernel
        d.kr = plastic_lobe_weight(rgb_mean(bd.reflectance), rgb_mean(bd.specular_reflectance));
    }
}

// blendbsdf.cpp:57-79 / mask.cpp:67-91 over plain records of this table (one level of nesting)
int fill_nested(const mtsamd_scene_desc *desc, uint32_t b, DevBsdf &d) {
    const mtsamd_bsdf_desc &bd = desc->bsdfs[b];
    const int n_child = d.type == kBsdfBlend ? 2 : 1;
    bool smooth = false;
    for (int k = 0; k < n_child; ++k) {
        const int32_t c = bd.nested[k];
        if (c < 0 || (uint32_t) c >= desc->bsdf_count || desc->bsdfs[c].type < MTSAMD_BSDF_DIFFUSE || desc->bsdfs[c].type > MTSAMD_BSDF_THINDIELECTRIC)
            return fail(MTSAMD_ERR_INVALID, "bsdf %u: nested[%d] must index a plain BSDF record", b, k);
        if (desc->spectral && desc->bsdfs[c].texture >= 0)
            return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u: textured children of a blendbsdf / mask are implemented for the RGB variant only", b);
        const int ct = desc->bsdfs[c].type;
        smooth = smooth || ct == kBsdfDiffuse || ct == kBsdfRoughConductor || ct == kBsdfPlastic || ct == kBsdfRoughPlastic || ct == kBsdfRoughDielectric;
    }
    if (d.type == kBsdfMask && bd.twosided) return fail(MTSAMD_ERR_INVALID, "Only materials without a transmission component can be nested!");
    if (desc->spectral && d.texture >= 0)
        return fail(MTSAMD_ERR_UNSUPPORTED, "eval_1(): a bitmap / checkerboard weight is converted into spectra in the spectral variant (bitmap.cpp:218-222); use a constant");
    d.nested0 = (uint32_t) bd.nested[0]; d.nested1 = (uint32_t) (n_child == 2 ? bd.nested[1] : bd.nested[0]);
    d.flags = (bd.twosided ? kBsdfTwoSided : 0u) | kBsdfUniformRefl | (smooth ? kBsdfNestSmooth : 0u) |
              ((d.texture >= 0 && desc->textures[d.texture].kind == 0) ? kBsdfWeightLum : 0u);
    return MTSAMD_OK;
}

// Spectral variant: every colour-valued parameter is a `uniform` constant or an `srgb` texture: range check + coefficient fetch
// (srgb.cpp:31-41); Texture::mean() of either kind feeds the plastic lobe-selection weight (plastic.cpp:170-175)
int spectral_bsdf_colours(const Input &in, uint32_t b, SceneState &st) {
    const mtsamd_bsdf_desc &bd = in.desc.bsdfs[b];
    DevBsdf &d = st.bsdfs[b];
    const float *vals[3] = { bd.reflectance, bd.specular_reflectance, bd.specular_transmittance };
    float *coeffs[3] = { &d.c0, &d.sc0, &d.tc0 };
    float means[3] = { 0.0f, 0.0f, 0.0f };
    for (int p = 0; p < 3; ++p) {
        if (d.type == kBsdfBlend || d.type == kBsdfMask) break;   // the weight is a scalar; the children are records of their own
        if (p == 0 && d.texture >= 0) continue;               // textured: coefficients per texel, mean from the texture (finish_textures)
        if (bd.uniform_mask & (1 << p)) { means[p] = vals[p][0]; continue; }
        if (in.bound(b, 0, p)) continue;              // a bound spectrum (bind_bsdf_spectra) replaces the colour: no range check, no coefficients
        float jac[9];
        if (int rc = srgb_colour(st.rgb2spec, vals[p], coeffs[p], &means[p], p == 0 ? jac : nullptr)) return rc;
        if (p == 0) {
            st.jac_bsdf.resize(9 * (size_t) in.desc.bsdf_count, 0.0f);
            std::copy(jac, jac + 9, st.jac_bsdf.begin() + 9 * (size_t) b);
        }
    }
    if (is_plastic(d.type)) d.kr = plastic_lobe_weight(means[0], means[1]);
    st.spec_mean[b] = means[1];
    st.diff_mean.resize(in.desc.bsdf_count, 0.0f);
    st.diff_mean[b] = means[0];
    return MTSAMD_OK;
}

// bound spectra replace the colour / constant of their parameter; Texture::mean() of the two reflectances feeds the plastic lobe weights
void bind_bsdf_spectra(const Input &in, SceneState &st) {
    for (uint32_t i = 0; i < in.n_bindings; ++i) {
        const mtsamd_spectrum_binding &bn = in.bindings[i];
        if (bn.target != MTSAMD_SPECTRUM_TARGET_BSDF) continue;
        DevBsdf &d = st.bsdfs[bn.index];
        const int slot = bsdf_spectrum_slot(in.desc.bsdfs[bn.index].type, bn.param);
        uint32_t &word = slot < 3 ? d.spectra0 : d.spectra1;
        const int shift = 10 * (slot < 3 ? slot : slot - 3);
        word = (word & ~(1023u << shift)) | ((bn.spectrum + 1u) << shift);
        const float mean = spectrum_table_mean(in.integrals[bn.spectrum]);
        if (slot == kSpecRefl) st.diff_mean[bn.index] = mean;
        if (slot == kSpecSpec) st.spec_mean[bn.index] = mean;
        if (is_plastic(d.type)) d.kr = plastic_lobe_weight(st.diff_mean[bn.index], st.spec_mean[bn.index]);
    }
    if (in.n_spectra) st.general_bsdfs = true;       // the spectrum pool is read by the general step
}

// textured parameters (checked by check_texture_bindings): "1 + texture index" into the 16-bit fields of nested0 / nested1, which a plain
// record does not use otherwise (DevBsdf), and the flags resolve_textured reads.  Such a scene runs the kernels of nested scenes: they
// are the ones that treat the record of a hit as working storage.
void bind_bsdf_textures(const Input &in, SceneState &st) {
    for (uint32_t i = 0; i < in.n_tex_bindings; ++i) {
        const mtsamd_texture_binding &bn = in.tex_bindings[i];
        DevBsdf &d = st.bsdfs[bn.bsdf];
        const char *why;
        const uint32_t slots = texture_param_slots(in.desc.bsdfs[bn.bsdf].type, bn.param, &why);
        const bool lum = in.desc.textures[bn.texture].kind == 0;       // Texture::eval_1 of a bitmap: luminance (bitmap.cpp:215-231)
        for (int slot = 0; slot < 4; ++slot) {
            if (!(slots & (1u << slot))) continue;
            uint32_t &word = slot < 2 ? d.nested0 : d.nested1;
            const int shift = 16 * (slot & 1);
            word = (word & ~(65535u << shift)) | (((uint32_t) bn.texture + 1u) << shift);
            if (lum && slot == kTexAlphaU) d.flags |= kBsdfAlphaULum;
            if (lum && slot == kTexAlphaV) d.flags |= kBsdfAlphaVLum;
        }
        d.flags |= kBsdfTexParams;
        st.textured_params = st.nested_bsdfs = true;
    }
}

int build_bsdfs(const Input &in, SceneState &st) {
    const mtsamd_scene_desc *desc = &in.desc;
    st.bsdfs.resize(desc->bsdf_count);
    st.spec_mean.assign(desc->bsdf_count, 0.0f);          // Texture::mean() of specular_reflectance (plastic lobe weights)
    for (uint32_t b = 0; b < desc->bsdf_count; ++b) {
        const mtsamd_bsdf_desc &bd = desc->bsdfs[b];
        DevBsdf &d = st.bsdfs[b];
        st.spec_mean[b] = rgb_mean(bd.specular_reflectance);
        std::memset(&d, 0, sizeof(d));
        d.r = bd.reflectance[0]; d.g = bd.reflectance[1]; d.b = bd.reflectance[2];
        d.type = bd.type; d.texture = bd.texture < 0 ? -1 : bd.texture;
        fill_bsdf_model(bd, d);
        if (d.type != kBsdfDiffuse || (d.flags & kBsdfTwoSided)) st.general_bsdfs = true;
        if (d.type != kBsdfDiffuse) st.non_diffuse_bsdfs = true;
        if (d.type == kBsdfBlend || d.type == kBsdfMask) {
            st.nested_bsdfs = true;
            if (int rc = fill_nested(desc, b, d)) return rc;
        }
        if (desc->spectral)
            if (int rc = spectral_bsdf_colours(in, b, st)) return rc;
    }
    bind_bsdf_spectra(in, st);
    bind_bsdf_textures(in, st);
    return MTSAMD_OK;
}

// ---- stage 5: textures --------------------------------------------------------------------------------------------------------------
// the lobe weight of a textured (rough)plastic follows Texture::mean() of its texture (plastic.cpp:170-175); true: record b changed
bool textured_lobe_weight(SceneState &st, size_t b, int32_t texture) {
    DevBsdf &d = st.bsdfs[b];
    if (d.texture != texture || !is_plastic(d.type)) return false;
    d.kr = plastic_lobe_weight(st.textures[texture].mean, st.spec_mean[b]);
    return true;
}

int build_textures(const mtsamd_scene_desc *desc, HostScene &hs) {
    SceneState &st = hs.state;
    hs.tex_src.assign(desc->texture_count, nullptr);
    hs.tex_coeffs.resize(desc->texture_count);
    for (uint32_t t = 0; t < desc->texture_count; ++t) {
        const mtsamd_texture_desc &td = desc->textures[t];
        DevTexture dt{};
        dt.kind = (uint32_t) td.kind;
        dt.w = td.kind == 0 ? td.width : 0; dt.h = td.kind == 0 ? td.height : 0;
        dt.grad_offset = st.textures.empty() ? 0u : st.textures.back().grad_offset + 3u * (uint32_t) st.textures.back().w * (uint32_t) st.textures.back().h;
        bool ident = true;
        for (int k = 0; k < 6; ++k) { dt.uvm[k] = td.to_uv[k]; ident = ident && td.to_uv[k] == 0.0f; }
        if (ident) { dt.uvm[0] = 1.0f; dt.uvm[4] = 1.0f; }
        for (int k = 0; k < 3; ++k) { dt.c0[k] = td.color0[k]; dt.c1[k] = td.color1[k]; }
        if (td.kind == 1) {
            // Texture::mean(): mean of the two colours' means (checkerboard.cpp:88-90, srgb.cpp:52-57); spectral variant: `srgb`
            // spectra with the constructor's range check (srgb.cpp:34-35)
            if (desc->spectral) {
                if (!srgb_in_range(td.color0) || !srgb_in_range(td.color1))
                    return fail(MTSAMD_ERR_INVALID, "Invalid RGB reflectance value in checkerboard texture %u, must be in the range [0, 1]!", t);
                srgb_model_fetch(st.rgb2spec, td.color0, dt.c0);
                srgb_model_fetch(st.rgb2spec, td.color1, dt.c1);
                dt.mean = 0.5f * (srgb_model_mean(dt.c0) + srgb_model_mean(dt.c1));
            } else {
                dt.mean = 0.5f * (rgb_mean(td.color0) + rgb_mean(td.color1));
            }
        } else {
            // Texture::mean(): mean luminance (bitmap.cpp:124-136); spectral variant: texels become model coefficients, mean of
            // srgb_model_mean (bitmap.cpp:116-123)
            const size_t n_texels = (size_t) td.width * td.height;
            if (desc->spectral) {
                dt.mean = spectral_texels(st.rgb2spec, td.data, n_texels, hs.tex_coeffs[t], st.jac_tex, dt.grad_offset);
                hs.tex_src[t] = hs.tex_coeffs[t].data();
            } else {
                dt.mean = bitmap_luminance_mean(td.data, n_texels);
                hs.tex_src[t] = td.data;
            }
        }
        st.textures.push_back(dt);
    }
    for (uint32_t b = 0; b < desc->bsdf_count; ++b)
        if (st.bsdfs[b].texture >= 0) textured_lobe_weight(st, b, st.bsdfs[b].texture);
    return MTSAMD_OK;
}

// ---- stage 6: accelerator, and the emitters that need the scene's bounding box --------------------------------------------------
void build_accelerator(const Input &in, const BuildOptions &opt, HostScene &hs) {
    SceneState &st = hs.state;
    if (st.n_prims > 0) build_bvh(hs.tri_pos.data(), st.n_prims, opt.max_leaf, st.bvh, &opt.bvh);
    else { st.bvh = BvhOutput{}; st.bvh.root = st.bvh.wroot = 0x80000000u; st.bvh.wdepth = 1; }       // a leaf with no triangles (BVH2 and BVH4 root: without wroot the walks of the split pipeline started at node 0 of an empty node array)
    if (st.environment >= 0) {       // ConstantBackgroundEmitter::set_scene (constant.cpp:47-51): bounding sphere of Scene::bbox()
        DevEmitter &e = st.emitters[st.environment];
        const float sc[4] = { e.c0, e.c1, e.c2, e.d65_scale };            // spectral variant: filled by build_emitters
        std::memset(&e, 0, sizeof(e));
        e.c0 = sc[0]; e.c1 = sc[1]; e.c2 = sc[2]; e.d65_scale = sc[3];
        const mtsamd_emitter_desc &ed = in.desc.emitters[st.environment];
        e.r = ed.radiance[0]; e.g = ed.radiance[1]; e.b = ed.radiance[2];
        e.shape = 0xffffffffu; e.pad0 = ed.type == MTSAMD_EMITTER_ENVMAP ? kEmitterEnvmap : kEmitterConstant;
    }
    set_scene_bounds(st);
    for (uint32_t i = 0; i < in.n_bindings; ++i)       // a tabulated radiance is the radiance itself (no D65 factor)
        if (in.bindings[i].target == MTSAMD_SPECTRUM_TARGET_EMITTER) st.emitters[in.bindings[i].index].spectrum = in.bindings[i].spectrum + 1u;
}

// ---- stage 7: flat scenes: 64-byte records in primitive order, pair records and cluster boxes (device_scene.h) -----------------
void build_flat_scene(const BuildOptions &opt, HostScene &hs) {
    build_flat_records(opt, hs.state, hs.tri_pos, hs);
    hs.state.geometry.flat = hs.flat;
    if (hs.flat) { hs.state.geometry.tri_pos = hs.tri_pos; hs.state.geometry.tri_nrm = hs.tri_nrm; hs.state.geometry.area_pmf = hs.area_pmf; hs.state.geometry.area_cdf = hs.area_cdf; }
}

} // namespace

void build_flat_records(const BuildOptions &opt, const SceneState &state, const std::vector<float> &tri_pos, FlatRecords &out) {
    const uint32_t n_prims = state.n_prims;
    const std::vector<uint32_t> &prim_shape = state.geometry.prim_shape;
    // Flat: few enough triangles, and tables small enough that the largest launch fits the LDS cap.  The shape, BSDF and emitter counts
    // are not bounded by the triangle count (delta emitters own no triangle, nested materials add records); a scene over the cap is
    // traversed through its hierarchy like any larger one.  The scene's variant decides the figure (spectral ring entries are larger).
    bool flat = n_prims <= opt.flat_max;
    if (flat) {
        SceneView sv = {};
        sv.flat = 1u; sv.n_prims = n_prims; sv.n_pairs = (n_prims + 1) / 2;
        for (uint32_t k = 0; k < sv.n_pairs; ++k) sv.n_clusters += k == 0 || prim_shape[2 * k] != prim_shape[2 * (k - 1)];
        sv.n_shapes = state.n_shapes; sv.n_bsdfs = (uint32_t) state.bsdfs.size(); sv.n_emitters = (uint32_t) state.emitters.size();
        flat = flat_launch_lds_max(sv, state.spectral) <= kFlatLdsCap;
    }
    out.flat = flat;
    out.flat_recs.assign(flat ? 4 * (size_t) n_prims : 0, float4{});
    for (uint32_t gp = 0; flat && gp < n_prims; ++gp) {
        const float *tp = &tri_pos[9 * (size_t) gp];
        uint32_t sh = prim_shape[gp]; float shf; std::memcpy(&shf, &sh, 4);
        // r0.w, r1 and r2.x: the per-triangle frame (n, s), computed on the device at scene creation; zero here
        out.flat_recs[4 * gp + 0] = make_float4(tp[0], tp[1], tp[2], 0.0f);
        out.flat_recs[4 * gp + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        out.flat_recs[4 * gp + 2] = make_float4(0.0f, tp[3], tp[4], tp[5]);
        out.flat_recs[4 * gp + 3] = make_float4(tp[6], tp[7], tp[8], shf);
    }
    const uint32_t n_pairs = out.n_pairs = flat ? (n_prims + 1) / 2 : 0;
    out.pair_recs.assign(5 * (size_t) n_pairs, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (uint32_t k = 0; k < n_pairs; ++k) {
        float a[9] = { 0 }, b[9] = { 0 };       // p0, e1, e2 of primitives 2k and 2k+1 (zero = never hit)
        for (int which = 0; which < 2; ++which) {
            uint32_t gp = 2 * k + which;
            if (gp >= n_prims) continue;
            const float *tp = &tri_pos[9 * (size_t) gp];
            float *r = which ? b : a;
            r[0] = tp[0]; r[1] = tp[1]; r[2] = tp[2];
            r[3] = tp[3] - tp[0]; r[4] = tp[4] - tp[1]; r[5] = tp[5] - tp[2];
            r[6] = tp[6] - tp[0]; r[7] = tp[7] - tp[1]; r[8] = tp[8] - tp[2];
        }
        out.pair_recs[5 * k + 0] = make_float4(a[0], b[0], a[1], b[1]);
        out.pair_recs[5 * k + 1] = make_float4(a[2], b[2], a[3], b[3]);
        out.pair_recs[5 * k + 2] = make_float4(a[4], b[4], a[5], b[5]);
        out.pair_recs[5 * k + 3] = make_float4(a[6], b[6], a[7], b[7]);
        out.pair_recs[5 * k + 4] = make_float4(a[8], b[8], 0.0f, 0.0f);
    }
    // clusters of consecutive pairs that belong to one shape, with their bounding box padded by 1e-4 of the scene's extent (the box
    // test of coherent waves only culls; device_scene.h, traverse_flat_clustered).  Appended to the pair records.
    out.n_clusters = 0;
    if (!flat || n_pairs == 0) return;
    float ext = 0.0f;
    for (uint32_t gp = 0; gp < n_prims; ++gp) for (int q = 0; q < 9; ++q) ext = std::max(ext, std::fabs(tri_pos[9 * (size_t) gp + q]));
    const float pad = 1e-4f * std::max(ext, 1e-3f);
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
        cull_encode<MTS_FLAT_CULL_FORM>(lo, hi, k0, k1 - k0, r0, r1);      // flat_cull.h: the record the device's reach predicate reads
        out.pair_recs.push_back(r0);
        out.pair_recs.push_back(r1);
        ++out.n_clusters;
    }
}

namespace {

// ---- stage 8: the BSDF records, and behind them the spectrum pool: headers, then node / value arrays ---------------------------
void build_bsdf_block(const Input &in, HostScene &hs) {
    const std::vector<DevBsdf> &bsdfs = hs.state.bsdfs;
    hs.bsdf_block = bsdfs;
    hs.n_spectra = in.n_spectra;
    if (!in.n_spectra) return;
    std::vector<DevSpectrum> headers; std::vector<float> data;
    build_spectrum_pool(in.spectra, in.n_spectra, headers, data);
    const size_t bytes = headers.size() * sizeof(DevSpectrum) + data.size() * sizeof(float);
    hs.bsdf_block.resize(bsdfs.size() + (bytes + sizeof(DevBsdf) - 1) / sizeof(DevBsdf));
    char *dst = reinterpret_cast<char *>(hs.bsdf_block.data() + bsdfs.size());
    std::memset(dst, 0, (hs.bsdf_block.size() - bsdfs.size()) * sizeof(DevBsdf));
    std::memcpy(dst, headers.data(), headers.size() * sizeof(DevSpectrum));
    if (!data.empty()) std::memcpy(dst + headers.size() * sizeof(DevSpectrum), data.data(), data.size() * sizeof(float));
}

// ---- stage 9: envmap emitter: texels + sampling hierarchy (envmap.cpp:66-125, distr_2d.h:200-312) ------------------------------
int build_envmap_emitter(const mtsamd_scene_desc *desc, HostScene &hs) {
    SceneState &st = hs.state;
    if (st.environment < 0 || desc->emitters[st.environment].type != MTSAMD_EMITTER_ENVMAP) return MTSAMD_OK;
    const mtsamd_emitter_desc &ed = desc->emitters[st.environment];
    EnvmapHost &eh = hs.env;
    st.env_w = ed.envmap_width; st.env_h = ed.envmap_height;
    if (set_envmap_texels(st, ed.envmap_data, eh) || eh.lv_offset.size() > (size_t) kEnvMaxLevels)
        return fail(MTSAMD_ERR_INVALID, "envmap: unsupported image size %d x %d", ed.envmap_width, ed.envmap_height);
    DevEnvmap &de = hs.dev_env;
    de.w = ed.envmap_width; de.h = ed.envmap_height; de.n_levels = (int32_t) eh.lv_offset.size(); de.scale = ed.envmap_scale;
    for (size_t k = 0; k < eh.lv_offset.size(); ++k) { de.lv_offset[k] = eh.lv_offset[k]; de.lv_width[k] = eh.lv_width[k]; }
    for (int k = 0; k < 2; ++k) { de.patch_size[k] = eh.patch_size[k]; de.inv_patch_size[k] = eh.inv_patch_size[k]; de.max_patch_index[k] = eh.max_patch_index[k]; }
    const float *m = ed.to_world;
    const float lin[9] = { m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10] };
    if (!invert_linear3(m, de.to_local)) return fail(MTSAMD_ERR_INVALID, "envmap: singular to_world transformation");
    for (int k = 0; k < 9; ++k) de.to_world[k] = lin[k];
    hs.has_envmap = true;
    return MTSAMD_OK;
}

} // namespace

int build_host_scene(const mtsamd_scene_desc *desc, const mtsamd_spectrum_desc *spectra, uint32_t n_spectra,
                     const mtsamd_spectrum_binding *bindings, uint32_t n_bindings, const BuildOptions &options, HostScene &hs,
                     const mtsamd_texture_binding *tex_bindings, uint32_t n_tex_bindings) {
    Input in{ *desc, spectra, n_spectra, bindings, n_bindings };
    in.tex_bindings = tex_bindings; in.n_tex_bindings = n_tex_bindings;
    hs = HostScene{};
    SceneState &st = hs.state;
    if (int rc = validate(in, st.environment)) return rc;
    st.n_prims = (uint32_t) in.total; st.n_shapes = desc->mesh_count;
    st.emitters.resize(desc->emitter_count);
    if (int rc = flatten_meshes(in, hs)) return rc;
    if (int rc = build_emitters(desc, st)) return rc;
    if (int rc = build_bsdfs(in, st)) return rc;
    if (int rc = build_textures(desc, hs)) return rc;
    build_accelerator(in, options, hs);
    build_flat_scene(options, hs);
    build_bsdf_block(in, hs);
    return build_envmap_emitter(desc, hs);
}

// ---- host half of the setters ------------------------------------------------------------------------------------------------------
bool bsdf_param_fields(const DevBsdf &b, int32_t kind, int32_t comp, float DevBsdf::*&f0, float DevBsdf::*&f1) {
    static float DevBsdf::*const refl[3] = { &DevBsdf::r, &DevBsdf::g, &DevBsdf::b }, DevBsdf::*const spec[3] = { &DevBsdf::sr, &DevBsdf::sg, &DevBsdf::sb },
                 DevBsdf::*const eta[3] = { &DevBsdf::er, &DevBsdf::eg, &DevBsdf::eb }, DevBsdf::*const kk[3] = { &DevBsdf::kr, &DevBsdf::kg, &DevBsdf::kb };
    f1 = nullptr;
    if (comp < 0 || comp > 2 || b.type >= kBsdfBlend) return false;
    const bool conductor = b.type == kBsdfConductor || b.type == kBsdfRoughConductor;
    const bool dielectric = b.type == kBsdfDielectric || b.type == kBsdfRoughDielectric || b.type == kBsdfThinDielectric;
    switch (kind) {
    case MTSAMD_PARAM_REFLECTANCE:        // diffuse.reflectance, (rough)plastic.diffuse_reflectance -- constants only
        if (b.texture >= 0 || !(b.type == kBsdfDiffuse || b.type == kBsdfPlastic || b.type == kBsdfRoughPlastic)) return false;
        f0 = refl[comp]; return true;
    case MTSAMD_PARAM_SPECULAR_REFLECTANCE:
        if (b.type == kBsdfDiffuse) return false;
        f0 = spec[comp]; return true;
    case MTSAMD_PARAM_SPECULAR_TRANSMITTANCE:
        if (!dielectric) return false;
        f0 = kk[comp]; return true;
    case MTSAMD_PARAM_ETA: if (!conductor) return false; f0 = eta[comp]; return true;
    case MTSAMD_PARAM_K: if (!conductor) return false; f0 = kk[comp]; return true;
    case MTSAMD_PARAM_ALPHA:              // isotropic roughness; roughplastic's alpha also shapes its transmittance tables: not offered
        if (!(b.type == kBsdfRoughConductor || b.type == kBsdfRoughDielectric) || b.alpha_u != b.alpha_v || comp != 0) return false;
        f0 = &DevBsdf::alpha_u; f1 = &DevBsdf::alpha_v; return true;
    default: return false;
    }
}

// Does record d read parameter `kind` from a texture (mtsamd_texture_binding)?  Such a parameter has no constant to differentiate: its
// texels carry the tangent / gradient.  Returns the name of the bound parameter, or null; ALPHA counts if either roughness is bound
static const char *textured_param(const DevBsdf &d, int32_t kind) {
    if (!(d.flags & kBsdfTexParams)) return nullptr;
    if (kind == MTSAMD_PARAM_ALPHA) {
        const uint32_t tu = bsdf_param_texture(d, kTexAlphaU), tv = bsdf_param_texture(d, kTexAlphaV);
        if (!tu && !tv) return nullptr;
        return texture_param_name(tu && tv ? MTSAMD_PARAM_ALPHA : (tu ? MTSAMD_PARAM_ALPHA_U : MTSAMD_PARAM_ALPHA_V));
    }
    if (kind == MTSAMD_PARAM_SPECULAR_REFLECTANCE && bsdf_param_texture(d, kTexSpec)) return texture_param_name(kind);
    if (kind == MTSAMD_PARAM_SPECULAR_TRANSMITTANCE && bsdf_param_texture(d, kTexTrans)) return texture_param_name(kind);
    return nullptr;
}

// The two perturbed copies of the BSDF table a forward-mode render differentiates between (k_forward): plus = theta + eps t, minus =
// theta - eps t per record, eps the largest step that moves no scalar by more than its limit -- h, or with h <= 0 1 % of
// max(|theta|, 0.05) -- shrunk so that ALPHA and ETA stay above 1e-4, as mtsamd_render_adjoint_param shrinks its step.  inv_2h[b] = 1 / (2 eps)
// (0: record b has no tangent), taken from the scalar with the largest |t| as t / (plus - minus): for a tangent that is 1 on one scalar
// and 0 elsewhere the three are bit for bit what mtsamd_render_adjoint_param builds for that scalar.  A tangent on a parameter the record
// reads from a texture is refused by name, so a field a texture overwrites at the hit never enters the eps rule, and the pairs of the
// untextured fields of a record with a map are those of the same record without it.
int build_tangent_records(const SceneState &st, const float *bsdf_tangents, float h, std::vector<DevBsdf> &plus, std::vector<DevBsdf> &minus,
                          std::vector<float> &inv_2h) {
    const size_t n = st.bsdfs.size();
    plus = st.bsdfs; minus = st.bsdfs; inv_2h.assign(n, 0.0f);
    if (!bsdf_tangents) return MTSAMD_OK;
    for (size_t i = 0; i < n * MTSAMD_BSDF_TANGENT_FLOATS; ++i)
        if (!std::isfinite(bsdf_tangents[i]))
            return fail(MTSAMD_ERR_INVALID, "bsdf %u: the tangent of parameter kind %d is not finite", (unsigned) (i / MTSAMD_BSDF_TANGENT_FLOATS), (int) (i % MTSAMD_BSDF_TANGENT_FLOATS) / 3);
    for (size_t b = 0; b < n; ++b) {
        const DevBsdf &rec = st.bsdfs[b];
        const float *t = bsdf_tangents + MTSAMD_BSDF_TANGENT_FLOATS * b;
        struct Scalar { float DevBsdf::*f0, DevBsdf::*f1; float t; int32_t kind; };
        Scalar sc[MTSAMD_BSDF_TANGENT_FLOATS]; int n_sc = 0;
        for (int32_t kind = MTSAMD_PARAM_REFLECTANCE; kind <= MTSAMD_PARAM_SPECULAR_TRANSMITTANCE; ++kind)
            for (int32_t comp = 0; comp < 3; ++comp) {
                if (t[3 * kind + comp] == 0.0f) continue;
                Scalar &x = sc[n_sc];
                if (const char *name = textured_param(rec, kind))
                    return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u: %s holds a texture; its texels carry the tangent (texture_tangents_dev), not a constant",
                                (unsigned) b, name);
                if (!bsdf_param_fields(rec, kind, comp, x.f0, x.f1))
                    return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u (type %d) has no differentiable parameter of kind %d (component %d of its tangent is not zero)",
                                (unsigned) b, rec.type, kind, comp);
                x.t = t[3 * kind + comp]; x.kind = kind; ++n_sc;
            }
        if (!n_sc) continue;
        float eps = std::numeric_limits<float>::infinity();
        for (int k = 0; k < n_sc; ++k) {
            const float theta = rec.*sc[k].f0, at = std::fabs(sc[k].t);
            float lim = h;
            if (!(lim > 0.0f)) lim = 0.01f * std::max(std::fabs(theta), 0.05f);
            eps = std::min(eps, lim / at);
        }
        for (int k = 0; k < n_sc; ++k) {          // the floor of ALPHA and ETA
            const float theta = rec.*sc[k].f0, at = std::fabs(sc[k].t);
            if ((sc[k].kind == MTSAMD_PARAM_ALPHA || sc[k].kind == MTSAMD_PARAM_ETA) && theta - eps * at <= 1e-4f) eps = std::min(eps, (0.5f * (theta - 1e-4f)) / at);
        }
        if (!(eps > 0.0f)) {
            for (int k = 0; k < n_sc; ++k)
                if ((sc[k].kind == MTSAMD_PARAM_ALPHA || sc[k].kind == MTSAMD_PARAM_ETA) && !(rec.*sc[k].f0 > 1e-4f))
                    return fail(MTSAMD_ERR_INVALID, "bsdf %u: parameter value %g leaves no room for a central difference", (unsigned) b, rec.*sc[k].f0);
            return fail(MTSAMD_ERR_INVALID, "bsdf %u: its tangent leaves no room for a central difference", (unsigned) b);
        }
        int lead = 0;
        for (int k = 0; k < n_sc; ++k) {
            const float theta = rec.*sc[k].f0, step = eps * sc[k].t;
            plus[b].*sc[k].f0 = theta + step; minus[b].*sc[k].f0 = theta - step;
            if (sc[k].f1) { plus[b].*sc[k].f1 = theta + step; minus[b].*sc[k].f1 = theta - step; }
            if (std::fabs(sc[k].t) > std::fabs(sc[lead].t)) lead = k;
        }
        const float span = plus[b].*sc[lead].f0 - minus[b].*sc[lead].f0;
        if (!(std::fabs(span) > 0.0f) || !std::isfinite(sc[lead].t / span))
            return fail(MTSAMD_ERR_INVALID, "bsdf %u: parameter value %g leaves no room for a central difference", (unsigned) b, rec.*sc[lead].f0);
        inv_2h[b] = sc[lead].t / span;
    }
    return MTSAMD_OK;
}

// The slot table of a reverse-mode render (k_reverse): per wanted scalar the patch that turns its record into the pair build_tangent_records
// makes for the one-hot tangent on that scalar -- the arithmetic below is that function's with t = 1 (eps = lim / 1, step = eps * 1,
// inv_2h = 1 / span), operation for operation, so the floats agree bit for bit.
int build_reverse_slots(const SceneState &st, const uint8_t *wanted, float h, std::vector<ReverseSlot> &slots, std::vector<uint32_t> &range) {
    const size_t n = st.bsdfs.size();
    slots.clear(); range.assign(n + 1, 0u);
    if (!wanted) return MTSAMD_OK;
    for (size_t b = 0; b < n; ++b) {
        const DevBsdf &rec = st.bsdfs[b];
        range[b] = (uint32_t) slots.size();
        for (int32_t kind = MTSAMD_PARAM_REFLECTANCE; kind <= MTSAMD_PARAM_SPECULAR_TRANSMITTANCE; ++kind)
            for (int32_t comp = 0; comp < 3; ++comp) {
                const uint32_t out = (uint32_t) (MTSAMD_BSDF_TANGENT_FLOATS * b) + (uint32_t) (3 * kind + comp);
                if (!wanted[out]) continue;
                float DevBsdf::*f0, DevBsdf::*f1;
                if (const char *name = textured_param(rec, kind))
                    return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u: %s holds a texture; its texels carry the gradient (grad_textures_dev), not a constant",
                                (unsigned) b, name);
                if (!bsdf_param_fields(rec, kind, comp, f0, f1))
                    return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u (type %d) has no differentiable parameter of kind %d (component %d is wanted)",
                                (unsigned) b, rec.type, kind, comp);
                const float theta = rec.*f0, at = 1.0f;
                float lim = h;
                if (!(lim > 0.0f)) lim = 0.01f * std::max(std::fabs(theta), 0.05f);
                float eps = lim / at;
                if ((kind == MTSAMD_PARAM_ALPHA || kind == MTSAMD_PARAM_ETA) && theta - eps * at <= 1e-4f) eps = std::min(eps, (0.5f * (theta - 1e-4f)) / at);
                if (!(eps > 0.0f))
                    return fail(MTSAMD_ERR_INVALID, "bsdf %u: parameter value %g leaves no room for a central difference", (unsigned) b, theta);
                const float step = eps * at;
                ReverseSlot s{};
                s.plus = theta + step; s.minus = theta - step;
                const float span = s.plus - s.minus;
                if (!(std::fabs(span) > 0.0f) || !std::isfinite(at / span))
                    return fail(MTSAMD_ERR_INVALID, "bsdf %u: parameter value %g leaves no room for a central difference", (unsigned) b, theta);
                s.inv_2h = at / span;
                s.record = (uint32_t) b; s.out = out;
                const char *base = reinterpret_cast<const char *>(&rec);
                s.f0 = (uint16_t) ((reinterpret_cast<const char *>(&(rec.*f0)) - base) / sizeof(float));
                s.f1 = f1 ? (uint16_t) ((reinterpret_cast<const char *>(&(rec.*f1)) - base) / sizeof(float)) : s.f0;
                slots.push_back(s);
            }
    }
    range[n] = (uint32_t) slots.size();
    return MTSAMD_OK;
}

// ---- blendbsdf / mask records in the forward and reverse renders (MTSAMD_FORWARD_NESTED / MTSAMD_REVERSE_NESTED) ---------------------
bool has_nested_records(const SceneState &st) {
    for (const DevBsdf &b : st.bsdfs)
        if (b.type >= kBsdfBlend) return true;
    return false;
}

// Every bit is known only where it means something: PARAM_TEXTURES (2) in a scene with textured BSDF parameters, NESTED (4) in an RGB scene
// with a blend / mask record.  Without bit 4 each refusal is, word for word, what it was before the bit existed.
int check_derivative_flags(const SceneState &st, uint32_t flags, bool reverse, bool &nested) {
    const char *mode = reverse ? "reverse-mode" : "forward-mode";
    const bool nests = has_nested_records(st);
    nested = false;
    const uint32_t known = 1u | (st.textured_params ? 2u : 0u) | (nests && !st.spectral ? 4u : 0u);
    if (flags & ~known) return fail(MTSAMD_ERR_INVALID, "unknown flag bits 0x%x in the %s descriptor", flags, reverse ? "gradient" : "tangent");
    if (st.spectral) return fail(MTSAMD_ERR_UNSUPPORTED, "the %s render is implemented for the RGB variant only", mode);
    if ((flags & 4u) && st.textured_params)
        return fail(MTSAMD_ERR_UNSUPPORTED, "the %s render does not handle blendbsdf / mask materials together with textured BSDF parameters "
                                            "(alpha, specular_reflectance, specular_transmittance) in one scene", mode);
    if (st.textured_params && !(flags & 2u))
        return fail(MTSAMD_ERR_UNSUPPORTED, "the %s render does not handle textured BSDF parameters (alpha, specular_reflectance, specular_transmittance)", mode);
    if (nests && !(flags & 4u)) return fail(MTSAMD_ERR_UNSUPPORTED, "the %s render does not handle blendbsdf / mask materials", mode);
    nested = nests;
    return MTSAMD_OK;
}

// The rows of blend / mask records taken out of a tangent (bsdf_tangents) or of a wanted list (bsdf_wanted); either may be null.  The
// weight / opacity of nested record b is entry 18 * b + 0 -- MTSAMD_PARAM_REFLECTANCE, component 0, the field the record keeps it in: it
// goes to weight_tangent[b] / weight_wanted[b] (bsdf_count entries each, 0 for every other record).  Every other non-zero entry of such a
// row is refused by name, and so is entry 0 where the record reads its weight from a texture (a bitmap's texels carry the tangent /
// gradient; a checkerboard has none).  rest_tangents / rest_wanted are the inputs with the nested rows zeroed: what build_tangent_records
// and build_reverse_slots are then called on, so the rows of every plain record, children included, reach them bit for bit.
int split_nested_rows(const SceneState &st, const float *bsdf_tangents, const uint8_t *bsdf_wanted, std::vector<float> &rest_tangents,
                      std::vector<float> &weight_tangent, std::vector<uint8_t> &rest_wanted, std::vector<uint8_t> &weight_wanted) {
    const size_t n = st.bsdfs.size(), row = MTSAMD_BSDF_TANGENT_FLOATS;
    rest_tangents.clear(); rest_wanted.clear();
    weight_tangent.assign(n, 0.0f); weight_wanted.assign(n, 0);
    if (bsdf_tangents) rest_tangents.assign(bsdf_tangents, bsdf_tangents + n * row);
    if (bsdf_wanted) rest_wanted.assign(bsdf_wanted, bsdf_wanted + n * row);
    for (size_t b = 0; b < n; ++b) {
        const DevBsdf &rec = st.bsdfs[b];
        if (rec.type < kBsdfBlend) continue;
        const char *name = rec.type == kBsdfBlend ? "weight" : "opacity";
        for (size_t i = 0; i < row; ++i) {
            const float t = bsdf_tangents ? bsdf_tangents[row * b + i] : 0.0f;
            const bool want = bsdf_wanted && bsdf_wanted[row * b + i] != 0;
            if (bsdf_tangents && !std::isfinite(t))
                return fail(MTSAMD_ERR_INVALID, "bsdf %u: the tangent of parameter kind %d is not finite", (unsigned) b, (int) i / 3);
            if (t == 0.0f && !want) continue;
            if (i != 0)
                return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u: a %s record has one differentiable scalar, its %s (parameter kind 0, component 0); kind %d, "
                                                    "component %d %s", (unsigned) b, rec.type == kBsdfBlend ? "blendbsdf" : "mask", name, (int) i / 3, (int) i % 3,
                            want ? "is wanted" : "of its tangent is not zero");
            if (rec.texture >= 0)
                return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u: %s holds a texture; its texels carry the %s, not a constant", (unsigned) b, name,
                            want ? "gradient (grad_textures_dev)" : "tangent (texture_tangents_dev)");
            weight_tangent[b] = t; weight_wanted[b] = want ? 1 : 0;
        }
        if (bsdf_tangents) std::fill(rest_tangents.begin() + row * b, rest_tangents.begin() + row * (b + 1), 0.0f);
        if (bsdf_wanted) std::fill(rest_wanted.begin() + row * b, rest_wanted.begin() + row * (b + 1), (uint8_t) 0);
    }
    return MTSAMD_OK;
}

// The slot table of build_reverse_slots with one more slot per wanted weight, in record order: a slot with f0 = f1 = kWeightSlot names
// no field of the record -- the weight's derivative is closed-form, so it has no +- pair -- and out = 18 * record.
void add_weight_slots(const std::vector<uint8_t> &weight_wanted, std::vector<ReverseSlot> &slots, std::vector<uint32_t> &range) {
    std::vector<ReverseSlot> merged; std::vector<uint32_t> r(range.size(), 0u);
    for (size_t b = 0; b + 1 < range.size(); ++b) {
        r[b] = (uint32_t) merged.size();
        merged.insert(merged.end(), slots.begin() + range[b], slots.begin() + range[b + 1]);
        if (b < weight_wanted.size() && weight_wanted[b]) {
            ReverseSlot s{};
            s.record = (uint32_t) b; s.f0 = s.f1 = kWeightSlot; s.out = (uint32_t) (MTSAMD_BSDF_TANGENT_FLOATS * b);
            merged.push_back(s);
        }
    }
    if (!r.empty()) r.back() = (uint32_t) merged.size();
    slots.swap(merged); range.swap(r);
}

// parameters_changed() of a (rough)plastic whose colours were set: the weight from the means the scene holds now.  The specular mean is
// spec_mean[] in both variants, the one textured_lobe_weight reads: every setter of specular_reflectance keeps it current.
static void constant_lobe_weight(SceneState &st, uint32_t bsdf) {
    DevBsdf &d = st.bsdfs[bsdf];
    if (!is_plastic(d.type)) return;
    const float d_mean = d.texture >= 0 ? st.textures[d.texture].mean : (st.spectral ? st.diff_mean[bsdf] : rgb_mean(&d.r));
    d.kr = plastic_lobe_weight(d_mean, st.spec_mean[bsdf]);
}

// Spectral variant: a colour-valued BSDF parameter (p = 0 reflectance, 1 specular_reflectance, 2 specular_transmittance) is an `srgb`
// spectrum (srgb_colour).  Parameters given as `uniform` spectra and textured reflectances are not settable this way.
static int spectral_set_colour(SceneState &st, uint32_t bsdf, int p, const float *rgb) {
    DevBsdf &d = st.bsdfs[bsdf];
    if (bsdf_spectrum(d, p)) return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u: this parameter holds a tabulated spectrum; only srgb colours can be set in the spectral variant", bsdf);
    const uint32_t uniform_flag = p == 0 ? kBsdfUniformRefl : (p == 1 ? kBsdfUniformSpec : kBsdfUniformTrans);
    if (d.type == kBsdfBlend || d.type == kBsdfMask || (d.flags & uniform_flag) || (p == 0 && d.texture >= 0))
        return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u: this parameter is a uniform spectrum, a texture or a nesting weight; only srgb colours can be set in the spectral variant", bsdf);
    float coeff[3], mean, jac[9];
    if (int rc = srgb_colour(st.rgb2spec, rgb, coeff, &mean, p == 0 ? jac : nullptr)) return rc;
    float *dst = p == 0 ? &d.c0 : (p == 1 ? &d.sc0 : &d.tc0);
    dst[0] = coeff[0]; dst[1] = coeff[1]; dst[2] = coeff[2];
    if (p == 0) {
        d.r = rgb[0]; d.g = rgb[1]; d.b = rgb[2]; st.diff_mean[bsdf] = mean;
        st.jac_bsdf.resize(9 * st.bsdfs.size(), 0.0f);
        std::copy(jac, jac + 9, st.jac_bsdf.begin() + 9 * (size_t) bsdf);
        st.jac_dirty = true;
    }
    if (p == 1) { d.sr = rgb[0]; d.sg = rgb[1]; d.sb = rgb[2]; st.spec_mean[bsdf] = mean; }
    if (p == 2) { d.kr = rgb[0]; d.kg = rgb[1]; d.kb = rgb[2]; }       // dielectrics only (bsdf_param_fields): the RGB copy creation fills
    constant_lobe_weight(st, bsdf);
    return MTSAMD_OK;
}

int set_bsdf_reflectance(SceneState &st, uint32_t bsdf, const float *rgb) {
    if (st.spectral) return spectral_set_colour(st, bsdf, 0, rgb);
    DevBsdf &d = st.bsdfs[bsdf];
    d.r = rgb[0]; d.g = rgb[1]; d.b = rgb[2];
    constant_lobe_weight(st, bsdf);
    return MTSAMD_OK;
}

int set_bsdf_param(SceneState &st, uint32_t bsdf, int32_t kind, const float *value3) {
    DevBsdf &d = st.bsdfs[bsdf];
    if (d.flags & kBsdfTexParams) {       // a textured parameter is edited through its texture (mtsamd_scene_update_texture), not set to a constant
        const bool textured = kind == MTSAMD_PARAM_ALPHA ? (bsdf_param_texture(d, kTexAlphaU) || bsdf_param_texture(d, kTexAlphaV))
                            : kind == MTSAMD_PARAM_SPECULAR_REFLECTANCE ? bsdf_param_texture(d, kTexSpec) != 0u
                            : kind == MTSAMD_PARAM_SPECULAR_TRANSMITTANCE ? bsdf_param_texture(d, kTexTrans) != 0u : false;
        if (textured) return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u: %s holds a texture; update the texture instead of setting a constant", bsdf, texture_param_name(kind));
    }
    if (st.spectral) {       // colours become srgb spectra; eta / k must stay uniform spectra (one value); alpha is a plain number
        if (kind == MTSAMD_PARAM_REFLECTANCE || kind == MTSAMD_PARAM_SPECULAR_REFLECTANCE || kind == MTSAMD_PARAM_SPECULAR_TRANSMITTANCE) {
            float DevBsdf::*f0, DevBsdf::*f1;
            if (!bsdf_param_fields(d, kind, 0, f0, f1)) return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u (type %d) has no settable parameter of kind %d", bsdf, d.type, kind);
            return spectral_set_colour(st, bsdf, kind == MTSAMD_PARAM_REFLECTANCE ? 0 : (kind == MTSAMD_PARAM_SPECULAR_REFLECTANCE ? 1 : 2), value3);
        }
        if ((kind == MTSAMD_PARAM_ETA || kind == MTSAMD_PARAM_K) && bsdf_spectrum(d, kind == MTSAMD_PARAM_ETA ? kSpecEta : kSpecK))
            return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u: this parameter holds a tabulated spectrum and cannot be set to a constant", bsdf);
        if ((kind == MTSAMD_PARAM_ETA || kind == MTSAMD_PARAM_K) && !(value3[0] == value3[1] && value3[1] == value3[2]))
            return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u: the spectral variant needs uniform (constant) eta and k spectra", bsdf);
    }
    for (int c = 0; c < (kind == MTSAMD_PARAM_ALPHA ? 1 : 3); ++c) {
        float DevBsdf::*f0, DevBsdf::*f1;
        if (!bsdf_param_fields(d, kind, c, f0, f1)) return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u (type %d) has no settable parameter of kind %d", bsdf, d.type, kind);
        d.*f0 = value3[c];
        if (f1) d.*f1 = value3[c];
    }
    if (st.spectral) return MTSAMD_OK;       // spectral: only colours move the weight (spectral_set_colour)
    if (kind == MTSAMD_PARAM_SPECULAR_REFLECTANCE) st.spec_mean[bsdf] = rgb_mean(&d.sr);       // Texture::mean() follows the colour, as at creation
    constant_lobe_weight(st, bsdf);
    return MTSAMD_OK;
}

int set_emitter_radiance(SceneState &st, uint32_t emitter, const float *rgb) {
    DevEmitter &e = st.emitters[emitter];
    if (e.spectrum) return fail(MTSAMD_ERR_UNSUPPORTED, "emitter %u: its radiance holds a tabulated spectrum; only srgb_d65 colours can be set", emitter);
    e.r = rgb[0]; e.g = rgb[1]; e.b = rgb[2];
    if (st.spectral) { srgb_d65_colour(st.rgb2spec, rgb, e); st.ejac_dirty = true; }
    return MTSAMD_OK;
}

bool texture_feeds_lobe_weight(const SceneState &st, uint32_t texture) {
    for (const DevBsdf &b : st.bsdfs) if (b.texture == (int32_t) texture && is_plastic(b.type)) return true;
    return false;
}

void set_texture_texels(SceneState &st, uint32_t texture, float *rgb, std::vector<float> &coeffs, std::vector<uint32_t> &changed_bsdfs) {
    DevTexture &t = st.textures[texture];
    const size_t n_texels = (size_t) t.w * t.h;
    if (st.spectral) {       // the texels hold model coefficients, converted after the clamp of an srgb colour
        for (size_t i = 0; i < 3 * n_texels; ++i) rgb[i] = std::max(std::min(rgb[i], 1.0f), 0.0f);
        t.mean = spectral_texels(st.rgb2spec, rgb, n_texels, coeffs, st.jac_tex, t.grad_offset);
        st.jac_dirty = true;
    } else {
        t.mean = bitmap_luminance_mean(rgb, n_texels);       // parameters_changed() (bitmap.cpp:308-322): the mean follows the data
    }
    changed_bsdfs.clear();
    for (size_t b = 0; b < st.bsdfs.size(); ++b)       // parameters_changed(): the plastic lobe weights read the mean
        if (textured_lobe_weight(st, b, (int32_t) texture)) changed_bsdfs.push_back((uint32_t) b);
}

int set_envmap_texels(SceneState &st, const float *rgb, EnvmapHost &eh) {
    if (!build_envmap(rgb, st.env_w, st.env_h, eh)) return fail(MTSAMD_ERR_INVALID, "envmap: unsupported image size");
    if (st.spectral) {       // envmap.cpp:96-109: the texels hold (model coefficients, scale); the sampling hierarchy stays the one built from the RGB luminance
        st.env_rgb.assign(rgb, rgb + 3 * (size_t) st.env_w * st.env_h);
        spectral_envmap_texels(st.rgb2spec, eh.texels.data(), eh.texels.size() / 4);
        st.ejac_dirty = true;
    }
    return MTSAMD_OK;
}

// ---- geometry: the pieces of creation that depend on vertex positions, and the vertex update made of them -------------------------
float triangle_area(const float *tp) {       // Mesh::face_area in fp32, the cross product with explicit fma (mesh.cpp:284-307)
    float e1[3] = { tp[3] - tp[0], tp[4] - tp[1], tp[5] - tp[2] }, e2[3] = { tp[6] - tp[0], tp[7] - tp[1], tp[8] - tp[2] };
    float cx = std::fma(e1[1], e2[2], -(e1[2] * e2[1])), cy = std::fma(e1[2], e2[0], -(e1[0] * e2[2])),
          cz = std::fma(e1[0], e2[1], -(e1[1] * e2[0]));
    return 0.5f * std::sqrt(std::fma(cz, cz, std::fma(cy, cy, cx * cx)));
}

// DiscreteDistribution::update (distr_1d.h:49-88): sequential double sum
int area_distribution(const float *areas, uint32_t face_count, float *cdf, DevEmitter &e) {
    double sum = 0.0; uint32_t lo = 0xffffffffu, hi = 0xffffffffu;
    for (uint32_t f = 0; f < face_count; ++f) {
        sum += (double) areas[f];
        cdf[f] = (float) sum;
        if (areas[f] > 0.0f) { if (lo == 0xffffffffu) lo = f; hi = f; }
    }
    if (lo == 0xffffffffu) return fail(MTSAMD_ERR_INVALID, "DiscreteDistribution: no probability mass found!");
    e.area_sum = (float) sum; e.area_norm = (float) (1.0 / sum);
    e.valid_lo = lo; e.valid_hi = hi;
    return MTSAMD_OK;
}

void set_scene_bounds(SceneState &st) {
    float centre[3], radius;
    bounding_sphere(st.bvh.bbox, centre, &radius);
    if (st.environment >= 0) {       // ConstantBackgroundEmitter::set_scene (constant.cpp:47-51): bounding sphere of Scene::bbox()
        DevEmitter &e = st.emitters[st.environment];
        e.cx = centre[0]; e.cy = centre[1]; e.cz = centre[2]; e.radius = radius;
    }
    for (DevEmitter &e : st.emitters)           // DirectionalEmitter::set_scene (directional.cpp:65-70)
        if (e.pad0 == kEmitterDirectional) e.radius = radius;
    set_emitter_boxes(st);
}

void emitter_exact_box(const float *xyz, size_t n_points, DevEmitter &e) {
    float lo[3] = { 3e38f, 3e38f, 3e38f }, hi[3] = { -3e38f, -3e38f, -3e38f };
    for (size_t i = 0; i < n_points; ++i)
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], xyz[3 * i + a]); hi[a] = std::max(hi[a], xyz[3 * i + a]); }
    for (int a = 0; a < 3; ++a) { e.aux[kFatedExact + a] = lo[a]; e.aux[kFatedExact + 3 + a] = hi[a]; }
}

// The padded boxes of the area emitters and the scene's list of them (fated.h), with the pad rule of the cluster boxes (stage 7) on the
// scene box: the largest coordinate magnitude of a box corner is that of a vertex.
void set_emitter_boxes(SceneState &st) {
    if (st.emitters.empty()) return;
    float ext = 0.0f;
    for (int k = 0; k < 6; ++k) ext = std::max(ext, std::fabs(st.bvh.bbox[k]));
    const float pad = 1e-4f * std::max(ext, 1e-3f);
    uint32_t list = 0u, n = 0u;
    bool off = st.environment >= 0;             // an escaped ray adds radiance
    for (size_t i = 0; i < st.emitters.size(); ++i) {
        DevEmitter &e = st.emitters[i];
        if (e.pad0 != 0u) continue;             // environment and delta emitters own no triangle
        const float lo[3] = { e.aux[kFatedExact], e.aux[kFatedExact + 1], e.aux[kFatedExact + 2] };
        const float hi[3] = { e.aux[kFatedExact + 3], e.aux[kFatedExact + 4], e.aux[kFatedExact + 5] };
        if (std::isfinite(pad)) fated_encode(lo, hi, pad, e.aux);
        else fated_invalidate(e.aux);
        if (n < kFatedMaxBoxes && i < 255u) list |= (uint32_t) (i + 1u) << (8u * n);
        else off = true;
        ++n;
    }
    if (off || n == 0u) list = 0u;
    std::memcpy(&st.emitters[0].aux[kFatedList], &list, 4);
}

int check_vertex_update(const SceneState &st, uint32_t shape, const float *positions, const float *normals) {
    const SceneGeometry &g = st.geometry;
    if (shape >= g.shapes.size()) return fail(MTSAMD_ERR_INVALID, "invalid shape index %u (the scene has %u shapes)", shape, (uint32_t) g.shapes.size());
    if (!positions) return fail(MTSAMD_ERR_INVALID, "shape %u: null vertex positions", shape);
    const bool has = (g.shapes[shape].flags & kShapeHasNormals) != 0u;
    if (has && !normals) return fail(MTSAMD_ERR_INVALID, "shape %u was created with vertex normals: new normals are required with new positions", shape);
    if (!has && normals) return fail(MTSAMD_ERR_INVALID, "shape %u was created without vertex normals: none can be set", shape);
    return MTSAMD_OK;
}

int check_vertex_flags(const SceneState &st, uint32_t shape, const float *normals, uint32_t flags) {
    const SceneGeometry &g = st.geometry;
    // the text of this refusal is what it was before MTSAMD_VERTICES_REBUILD_ACCEL existed: every bit beside the recompute flag
    // MTSAMD_VERTICES_ACCEL_SAH chooses the builder of a rebuild: without one it is an unknown bit
    const uint32_t known = MTSAMD_VERTICES_RECOMPUTE_NORMALS | MTSAMD_VERTICES_REBUILD_ACCEL | ((flags & MTSAMD_VERTICES_REBUILD_ACCEL) ? MTSAMD_VERTICES_ACCEL_SAH : 0u);
    if (flags & ~known) return fail(MTSAMD_ERR_INVALID, "unknown vertex update flags 0x%x", flags & ~(uint32_t) MTSAMD_VERTICES_RECOMPUTE_NORMALS);
    if (!(flags & MTSAMD_VERTICES_RECOMPUTE_NORMALS)) return MTSAMD_OK;
    if (shape >= g.shapes.size()) return fail(MTSAMD_ERR_INVALID, "invalid shape index %u (the scene has %u shapes)", shape, (uint32_t) g.shapes.size());
    if (normals) return fail(MTSAMD_ERR_INVALID, "shape %u: MTSAMD_VERTICES_RECOMPUTE_NORMALS computes the normals: none can be passed with it", shape);
    if (!(g.shapes[shape].flags & kShapeHasNormals))      // recompute_vertex_normals' Throw (mesh.cpp:200-202)
        return fail(MTSAMD_ERR_INVALID, "shape %u was created without vertex normals: storing new normals in such a mesh is not implemented", shape);
    return MTSAMD_OK;
}

void compute_vertex_normals(uint32_t vertex_count, const float *positions, uint32_t face_count, const uint32_t *faces, float *normals_out) {
    std::vector<float> acc(3 * (size_t) vertex_count, 0.0f);
    for (uint32_t f = 0; f < face_count; ++f) {
        const uint32_t *fi = faces + 3 * (size_t) f;
        float rec[6];
        if (!vn_face(positions + 3 * (size_t) fi[0], positions + 3 * (size_t) fi[1], positions + 3 * (size_t) fi[2], rec)) continue;
        for (uint32_t j = 0; j < 3; ++j) vn_accumulate(&acc[3 * (size_t) fi[j]], rec, j);
    }
    for (uint32_t v = 0; v < vertex_count; ++v) vn_finish(&acc[3 * (size_t) v], normals_out + 3 * (size_t) v);
}

void build_corner_table(uint32_t vertex_count, uint32_t face_count, const uint32_t *faces, std::vector<uint32_t> &offsets, std::vector<uint32_t> &corners) {
    offsets.assign((size_t) vertex_count + 1, 0u);
    corners.assign(3 * (size_t) face_count, 0u);
    for (size_t c = 0; c < corners.size(); ++c) ++offsets[(size_t) faces[c] + 1];
    for (uint32_t v = 0; v < vertex_count; ++v) offsets[v + 1] += offsets[v];
    std::vector<uint32_t> next(offsets.begin(), offsets.end() - 1);
    for (size_t c = 0; c < corners.size(); ++c) corners[next[faces[c]]++] = (uint32_t) c;       // c = 3 * face + corner, met in ascending order
}

int check_finite(uint32_t shape, const float *positions, size_t n_floats) {
    for (size_t i = 0; i < n_floats; ++i)
        if (!std::isfinite(positions[i])) return fail(MTSAMD_ERR_INVALID, "shape %u: vertex %u has a non-finite coordinate", shape, (uint32_t) (i / 3));
    return MTSAMD_OK;
}

void gather_shape(const SceneGeometry &g, uint32_t shape, const float *positions, const float *normals, float *tri_pos, float *tri_nrm) {
    const uint32_t off = g.shapes[shape].first_prim;
    for (uint32_t f = 0; f < g.shape_faces[shape]; ++f)
        for (int j = 0; j < 3; ++j) {
            const uint32_t vi = g.faces[3 * (size_t) (off + f) + j];
            for (int k = 0; k < 3; ++k) {
                tri_pos[9 * (size_t) f + 3 * j + k] = positions[3 * (size_t) vi + k];
                if (normals) tri_nrm[9 * (size_t) f + 3 * j + k] = normals[3 * (size_t) vi + k];
            }
        }
}

int set_vertex_positions(SceneState &st, const BuildOptions &opt, uint32_t shape, const float *positions, const float *normals,
                         std::vector<float> &tri_pos, std::vector<float> &tri_nrm, std::vector<float> &area_pmf, std::vector<float> &area_cdf, FlatRecords &flat) {
    if (int rc = check_vertex_update(st, shape, positions, normals)) return rc;
    const SceneGeometry &g = st.geometry;
    if (int rc = check_finite(shape, positions, 3 * (size_t) g.shape_vertices[shape])) return rc;
    const uint32_t off = g.shapes[shape].first_prim, n = g.shape_faces[shape];
    std::vector<float> pos(9 * (size_t) n), nrm(normals ? 9 * (size_t) n : 0), pmf(n), cdf(n);
    gather_shape(g, shape, positions, normals, pos.data(), nrm.data());
    const int32_t em = g.shapes[shape].emitter;
    DevEmitter e{};
    if (em >= 0) {       // refused before anything is written
        e = st.emitters[em];
        for (uint32_t f = 0; f < n; ++f) pmf[f] = triangle_area(&pos[9 * (size_t) f]);
        if (int rc = area_distribution(pmf.data(), n, cdf.data(), e)) return rc;
        emitter_exact_box(pos.data(), 3 * (size_t) n, e);
    }
    std::copy(pos.begin(), pos.end(), tri_pos.begin() + 9 * (size_t) off);
    if (normals) std::copy(nrm.begin(), nrm.end(), tri_nrm.begin() + 9 * (size_t) off);
    if (em >= 0) {
        st.emitters[em] = e;
        std::copy(pmf.begin(), pmf.end(), area_pmf.begin() + off); std::copy(cdf.begin(), cdf.end(), area_cdf.begin() + off);
    }
    refit_bvh(tri_pos.data(), st.bvh);
    set_scene_bounds(st);
    const bool was_flat = flat.flat;
    build_flat_records(opt, st, tri_pos, flat);
    if (flat.flat != was_flat) return fail(MTSAMD_ERR_DEVICE, "vertex update: the scene changed its kind");       // flatness depends on counts only
    return MTSAMD_OK;
}

} // namespace mtsamd

// device_spectral.h -- spectral variant (4 wavelengths per camera sample) of the light-transport stages.
//
// Reference semantics followed (paths relative to the Mitsuba 2 tree):
//   sample_wavelength / sample_rgb_spectrum     include/mitsuba/core/spectrum.h:270-314
//   math::sample_shifted                        include/mitsuba/core/math.h:418-442
//   cie1931_xyz / spectrum_to_xyz               include/mitsuba/core/spectrum.h:127-217
//   srgb_model_eval                             include/mitsuba/render/srgb.h:8-24
//   SRGBReflectanceSpectrum / SRGBEmitterSpectrum  src/spectra/srgb.cpp:27-52, src/spectra/srgb_d65.cpp:27-63
//   D65Spectrum -> RegularSpectrum              src/spectra/d65.cpp:44-66, src/spectra/regular.cpp:68-75
//   ContinuousDistribution::eval_pdf            include/mitsuba/core/distr_1d.h:378-394
#pragma once
#include "device_math.h"

namespace mtsamd {

constexpr int kWav = 4;                         // MTS_WAVELENGTH_SAMPLES of the spectral variants (mitsuba.conf.template:135-138)
constexpr float kCieMin = 360.0f, kCieMax = 830.0f;

// 95-sample tables at 5 nm: CIE 1931 x, y, z and CIE D65 (filled once by upload_spectral_tables())
struct SpectralTables { float x[95], y[95], z[95], d65[95]; };
extern __device__ SpectralTables g_spectral;

struct Spec4 { float v[kWav]; };

// sample_wavelength (spectrum.h:270-314): shifted samples (math.h:418-442) + the "importance spectrum" of Radziszewski et al.  The 1 / pdf
// weights are applied when the path ends (wavelength_weight in store_result_spectral).
// the four wavelengths of a path as a function of its one wavelength sample: this is what the path pool stores (4 B instead of the
// 16 B of the wavelengths themselves); recomputed when a path record is loaded -- the same operations on the same number, so the bits
// are those of sample_wavelengths
MTS_DEV void wavelengths_from_sample(float sample, Spec4 &wav) {
#pragma unroll
    for (int k = 0; k < kWav; ++k) {
        float v = sample + (float) k / (float) kWav;
        if (v > 1.0f) v -= 1.0f;
        wav.v[k] = 538.0f - lm_atanh(0.8569106254698279f - 1.8275019724092267f * v) * 138.88888888888889f;
    }
}
MTS_DEV float wavelength_weight(float l) {
    float t = lm_cosh(0.0072f * (l - 538.0f));
    return 253.82f * t * t;
}

MTS_DEV float srgb_model_eval(float c0, float c1, float c2, float l) {
    float v = fmaf(fmaf(c0, l, c1), l, c2);
    if (isinf(c2)) return fmaf(copysignf(1.0f, c2), 0.5f, 0.5f);
    return fmaxf(0.0f, fmaf(0.5f * v, 1.0f / sqrtf(fmaf(v, v, 1.0f)), 0.5f));
}

// linear interpolation in a 95-entry table over [360, 830] nm, 0 outside (values optionally pre-scaled)
MTS_DEV float table_eval(const float *tbl, float scale, float l) {
    if (!(l >= kCieMin && l <= kCieMax)) return 0.0f;
    float x = (l - kCieMin) * 0.2f;               // m_inv_interval_size = float(1 / (470 / 94))
    uint32_t i = min((uint32_t) x, 93u);
    float y0 = tbl[i] * scale, y1 = tbl[i + 1] * scale;
    float w1 = x - (float) i, w0 = 1.0f - w1;
    return fmaf(w0, y0, w1 * y1);
}

// Tabulated and analytic spectra a scene may bind to its spectral parameters (mtsamd_scene_create_with_spectra):
//   regular    RegularSpectrum (src/spectra/regular.cpp:68-75)     -> ContinuousDistribution::eval_pdf (distr_1d.h:378-393)
//   irregular  IrregularSpectrum (src/spectra/irregular.cpp:76-83) -> IrregularContinuousDistribution::eval_pdf (distr_1d.h:655-677)
//   blackbody  BlackBodySpectrum::eval_impl (src/spectra/blackbody.cpp:46-83)
// (`d65` is a regular table the host expands, d65.cpp:44-66.)  The pool is read-only device memory: n headers, then the node and value
// arrays the headers index; it stays in global memory (a few KB, cache-resident).
constexpr uint32_t kSpectrumRegular = 0u, kSpectrumIrregular = 1u, kSpectrumBlackbody = 2u;
struct DevSpectrum {
    uint32_t kind, size, nodes, values;                  // nodes / values: float offsets into the pool's data (nodes: irregular only)
    float lambda_min, lambda_max, inv_interval, temperature;      // inv_interval = float(1 / (double(range) / (size - 1))) (distr_1d.h:314-344)
};
struct SpectrumPool { const DevSpectrum *headers; const float *data; };

MTS_DEV float regular_eval(const DevSpectrum &h, const float *data, float l) {
    if (!(l >= h.lambda_min && l <= h.lambda_max)) return 0.0f;
    const float x = (l - h.lambda_min) * h.inv_interval;
    const uint32_t i = min((uint32_t) x, h.size - 2u);
    const float y0 = data[h.values + i], y1 = data[h.values + i + 1u];
    const float w1 = x - (float) i, w0 = 1.0f - w1;
    return fmaf(w0, y0, w1 * y1);
}
MTS_DEV float irregular_eval(const DevSpectrum &h, const float *data, float l) {
    if (!(l >= h.lambda_min && l <= h.lambda_max)) return 0.0f;
    const float *nodes = data + h.nodes;
    uint32_t lo = 0u, hi = h.size;                      // enoki::binary_search: the first node that is not < l
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (nodes[mid] < l) lo = mid + 1u; else hi = mid;
    }
    const uint32_t i = max(min(lo, h.size - 1u), 1u) - 1u;
    const float x0 = nodes[i], x1 = nodes[i + 1u], y0 = data[h.values + i], y1 = data[h.values + i + 1u];
    const float t = (l - x0) / (x1 - x0);
    return fmaf(t, y1 - y0, y0);
}
MTS_DEV float blackbody_eval(float temperature, float l) {
    constexpr float c = 2.99792458e+8f, h = 6.62607004e-34f, k = 1.38064852e-23f;
    constexpr float c0 = 2 * h * c * c, c1 = h * c / k;
    if (!(l >= kCieMin && l <= kCieMax)) return 0.0f;
    const float lambda = l * 1e-9f, lambda2 = lambda * lambda, lambda5 = (lambda2 * lambda2) * lambda;
    return 1e-9f * c0 / (lambda5 * (lm_exp(c1 / (lambda * temperature)) - 1.0f));
}
MTS_DEV float spectrum_eval(const SpectrumPool &pool, uint32_t index, float l) {
    const DevSpectrum h = pool.headers[index];
    if (h.kind == kSpectrumRegular) return regular_eval(h, pool.data, l);
    if (h.kind == kSpectrumIrregular) return irregular_eval(h, pool.data, l);
    return blackbody_eval(h.temperature, l);
}

// cie1931_xyz (spectrum.h:127-163): the observer's colour matching functions at wavelength l, the table interpolation of spectrum_to_xyz
// below (which keeps its own copy: folding it into this helper changed the machine code of the render kernels)
MTS_DEV f3 cie1931_xyz(float l) {
    float t = (l - kCieMin) * ((95 - 1) / (kCieMax - kCieMin));
    bool active = l >= kCieMin && l <= kCieMax;
    int i0 = min(max((int) t, 0), 93);
    float w1 = t - (float) i0, w0 = 1.0f - w1;
    return mk3(active ? fmaf(w0, g_spectral.x[i0], w1 * g_spectral.x[i0 + 1]) : 0.0f,
               active ? fmaf(w0, g_spectral.y[i0], w1 * g_spectral.y[i0 + 1]) : 0.0f,
               active ? fmaf(w0, g_spectral.z[i0], w1 * g_spectral.z[i0 + 1]) : 0.0f);
}

MTS_DEV f3 spectrum_to_xyz(const Spec4 &value, const Spec4 &wav) {
    float X[kWav], Y[kWav], Z[kWav];
#pragma unroll
    for (int k = 0; k < kWav; ++k) {
        float l = wav.v[k];
        float t = (l - kCieMin) * ((95 - 1) / (kCieMax - kCieMin));
        bool active = l >= kCieMin && l <= kCieMax;
        int i0 = min(max((int) t, 0), 93);
        float w1 = t - (float) i0, w0 = 1.0f - w1;
        X[k] = active ? fmaf(w0, g_spectral.x[i0], w1 * g_spectral.x[i0 + 1]) : 0.0f;
        Y[k] = active ? fmaf(w0, g_spectral.y[i0], w1 * g_spectral.y[i0 + 1]) : 0.0f;
        Z[k] = active ? fmaf(w0, g_spectral.z[i0], w1 * g_spectral.z[i0 + 1]) : 0.0f;
    }
    // hmean over the 4 wavelengths
    return mk3((((X[0] * value.v[0]) + (X[1] * value.v[1])) + ((X[2] * value.v[2]) + (X[3] * value.v[3]))) * 0.25f,
               (((Y[0] * value.v[0]) + (Y[1] * value.v[1])) + ((Y[2] * value.v[2]) + (Y[3] * value.v[3]))) * 0.25f,
               (((Z[0] * value.v[0]) + (Z[1] * value.v[1])) + ((Z[2] * value.v[2]) + (Z[3] * value.v[3]))) * 0.25f);
}

} // namespace mtsamd

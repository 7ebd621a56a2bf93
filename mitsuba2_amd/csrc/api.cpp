// api.cpp -- host side of libmtsamd: scene upload, BVH build, emitter tables, sensor/film setup,
// the wavefront scheduler and the C ABI declared in include/mtsamd.h.  The two host-only halves live beside it: scene_build.{h,cpp}
// computes what is uploaded, schedule.{h,cpp} plans jobs, passes, the pool drain, the film passes and their splats; this file carries
// them out on the device (allocations, streams, events, copies, launches).
//
// Reference call stack this replaces:
//   Scene::Scene -> accel_init -> ShapeKDTree::build          src/librender/scene.cpp:22-98
//   SamplingIntegrator::render (wavefront branch)              src/librender/integrator.cpp:144-169
//   PerspectiveCamera::update_camera_transforms                src/sensors/perspective.cpp:106-151
//   ReconstructionFilter::init_discretization                  src/libcore/rfilter.cpp:9-20
//   HDRFilm::prepare/put                                       src/films/hdrfilm.cpp:188-209
#include "../../include/mtsamd.h"
#include "bvh.h"
#include "envmap.h"
#include "kernels.h"
#include "scene_build.h"
#include "refit.h"
#include "lbvh.h"
#include "lbvh_keys.h"
#include "sah_build.h"
#include "schedule.h"
#include "spectral_upsampling.h"
#include "cie_data.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

using namespace mtsamd;

namespace {

// Experiment switches (scheduler geometry, BVH leaf size, ...) read from the environment exist only in builds made with
// -DMTSAMD_EXPERIMENTS (scripts/ab_build.sh); the release library never looks at the process environment.
#ifdef MTSAMD_EXPERIMENTS
static const char *exp_env(const char *name) { return std::getenv(name); }
#else
static const char *exp_env(const char *) { return nullptr; }
#endif

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(e_ == hipErrorOutOfMemory ? MTSAMD_ERR_NOMEM : MTSAMD_ERR_DEVICE, "%s: %s",    \
                        #expr, hipGetErrorString(e_));                                                 \
    } while (0)

// ---- 4x4 float matrices with Enoki's product order (column-wise fmadd) ---------------------
struct Mat4 {
    float m[4][4];
    static Mat4 identity() { Mat4 r{}; for (int i = 0; i < 4; ++i) r.m[i][i] = 1.0f; return r; }
    Mat4 operator*(const Mat4 &b) const {
        Mat4 c{};
        for (int r = 0; r < 4; ++r)
            for (int j = 0; j < 4; ++j) {
                float acc = m[r][0] * b.m[0][j];
                for (int i = 1; i < 4; ++i) acc = std::fma(m[r][i], b.m[i][j], acc);
                c.m[r][j] = acc;
            }
        return c;
    }
    Mat4 transposed() const { Mat4 c{}; for (int r = 0; r < 4; ++r) for (int j = 0; j < 4; ++j) c.m[r][j] = m[j][r]; return c; }
};
struct Xform {   // Transform: matrix + inverse transpose (include/mitsuba/core/transform.h)
    Mat4 matrix, inv_t;
    Xform operator*(const Xform &o) const { return Xform{ matrix * o.matrix, inv_t * o.inv_t }; }
    static Xform scale(float x, float y, float z) {
        Xform r{ Mat4::identity(), Mat4::identity() };
        r.matrix.m[0][0] = x; r.matrix.m[1][1] = y; r.matrix.m[2][2] = z;
        r.inv_t.m[0][0] = 1.0f / x; r.inv_t.m[1][1] = 1.0f / y; r.inv_t.m[2][2] = 1.0f / z;
        return r;
    }
    static Xform translate(float x, float y, float z) {
        Xform r{ Mat4::identity(), Mat4::identity() };
        r.matrix.m[0][3] = x; r.matrix.m[1][3] = y; r.matrix.m[2][3] = z;
        Mat4 inv = Mat4::identity(); inv.m[0][3] = -x; inv.m[1][3] = -y; inv.m[2][3] = -z;
        r.inv_t = inv.transposed();
        return r;
    }
    static Xform perspective(float fov, float near_, float far_) {   // transform.h:203-220
        float recip = 1.0f / (far_ - near_);
        float tan_ = std::tan((fov * 0.5f) * (3.14159265358979323846f / 180.0f)), cot = 1.0f / tan_;
        Mat4 t{}; t.m[0][0] = cot; t.m[1][1] = cot; t.m[2][2] = far_ * recip; t.m[2][3] = -near_ * far_ * recip; t.m[3][2] = 1.0f;
        Mat4 it{}; it.m[0][0] = tan_; it.m[1][1] = tan_; it.m[3][3] = 1.0f / near_; it.m[2][3] = 1.0f;
        it.m[3][2] = (near_ - far_) / (far_ * near_);
        return Xform{ t, it.transposed() };
    }
};

int make_camera(const mtsamd_render_desc &d, CameraView &c) {
    if (!(d.near_clip > 0.0f)) return fail(MTSAMD_ERR_INVALID, "The 'near_clip' parameter must be greater than zero!");
    if (!(d.near_clip < d.far_clip)) return fail(MTSAMD_ERR_INVALID, "The 'near_clip' parameter must be smaller than 'far_clip'.");
    if (!(d.fov_x_deg > 0.0f && d.fov_x_deg < 180.0f))
        return fail(MTSAMD_ERR_INVALID, "The horizontal field of view must be in the range [0, 180]!");
    float fw = (float) d.film_width, fh = (float) d.film_height;
    float rsx = (float) d.crop_width / fw, rsy = (float) d.crop_height / fh;
    float rox = (float) d.crop_x / fw, roy = (float) d.crop_y / fh;
    float aspect = fw / fh;
    Xform c2s = Xform::scale(1.0f / rsx, 1.0f / rsy, 1.0f) * Xform::translate(-rox, -roy, 0.0f) *
                Xform::scale(-0.5f, -0.5f * aspect, 1.0f) * Xform::translate(-1.0f, -1.0f / aspect, 0.0f) *
                Xform::perspective(d.fov_x_deg, d.near_clip, d.far_clip);
    Mat4 s2c = c2s.inv_t.transposed();              // Transform::inverse()
    for (int r = 0; r < 4; ++r) for (int j = 0; j < 4; ++j) c.s2c[4 * r + j] = s2c.m[r][j];
    std::memcpy(c.c2w, d.to_world, sizeof(float) * 16);
    c.near_clip = d.near_clip; c.far_clip = d.far_clip;
    if (d.aperture_radius < 0.0f) return fail(MTSAMD_ERR_INVALID, "The 'aperture_radius' parameter must not be negative");
    c.aperture_radius = d.aperture_radius; c.focus_distance = d.focus_distance;
    if (d.aperture_radius > 0.0f && !(d.focus_distance > 0.0f)) return fail(MTSAMD_ERR_INVALID, "thinlens: 'focus_distance' must be positive");
    return 0;
}

// B-spline family of mitchell.cpp:41-56 / catmullrom.cpp:29-43 (B = 0, C = 0.5)
static float cubic_filter(float x, float B, float C) {
    x = std::fabs(x);
    const float x2 = x * x, x3 = x2 * x;
    const float result = (1.0f / 6.0f) * (x < 1.0f
        ? (12.0f - 9.0f * B - 6.0f * C) * x3 + (-18.0f + 12.0f * B + 6.0f * C) * x2 + (6.0f - 2.0f * B)
        : (-B - 6.0f * C) * x3 + (6.0f * B + 30.0f * C) * x2 + (-12.0f * B - 48.0f * C) * x + (8.0f * B + 24.0f * C));
    return x < 2.0f ? result : 0.0f;
}

// param / param2: gaussian stddev | box radius | mitchell B, C | lanczos lobes (tent and catmullrom take none)
int make_filter(int32_t kind, float param, float param2, int32_t analytic, FilterView &f) {
    std::memset(&f, 0, sizeof(f));
    f.kind = kind; f.analytic = analytic;
    if (kind == MTSAMD_RFILTER_GAUSSIAN) {
        if (!(param > 0.0f)) return fail(MTSAMD_ERR_INVALID, "gaussian rfilter: stddev must be positive");
        f.radius = 4 * param;
        f.alpha = -1.0f / (2.0f * param * param);
        f.bias = lm_exp(f.alpha * (f.radius * f.radius));
    } else if (kind == MTSAMD_RFILTER_BOX) {
        if (!(param > 0.0f)) return fail(MTSAMD_ERR_INVALID, "box rfilter: radius must be positive");
        f.radius = param + kRayEpsilon;
    } else if (kind == MTSAMD_RFILTER_TENT) {
        f.radius = 1.0f; f.alpha = 1.0f / f.radius;                    // alpha = m_inv_radius (tent.cpp:28-30)
    } else if (kind == MTSAMD_RFILTER_CATMULLROM) {
        f.radius = 2.0f;
    } else if (kind == MTSAMD_RFILTER_MITCHELL) {
        f.radius = 2.0f; f.alpha = param; f.bias = param2;            // alpha = B, bias = C
    } else if (kind == MTSAMD_RFILTER_LANCZOS) {
        if (!(param >= 1.0f) || param > 16.0f) return fail(MTSAMD_ERR_INVALID, "lanczos rfilter: 'lobes' must be in [1, 16]");
        f.radius = (float) (int) param;
    } else {
        return fail(MTSAMD_ERR_UNSUPPORTED, "unsupported reconstruction filter %d (gaussian, box, tent, catmullrom, mitchell, lanczos)", kind);
    }
    auto eval = [&](float x) -> float {
        switch (kind) {
        case MTSAMD_RFILTER_GAUSSIAN: return std::max(0.0f, lm_exp(f.alpha * (x * x)) - f.bias);
        case MTSAMD_RFILTER_TENT: return std::max(0.0f, 1.0f - std::fabs(x * f.alpha));
        case MTSAMD_RFILTER_CATMULLROM: return cubic_filter(x, 0.0f, 0.5f);
        case MTSAMD_RFILTER_MITCHELL: return cubic_filter(x, f.alpha, f.bias);
        case MTSAMD_RFILTER_LANCZOS: {
            x = std::fabs(x);
            const float x1 = kPi * x, x2 = x1 / f.radius, result = (lm_sin(x1) * lm_sin(x2)) / (x1 * x2);
            return x < kEpsilon ? 1.0f : (x > f.radius ? 0.0f : result);
        }
        default: return std::fabs(x) <= f.radius ? 1.0f : 0.0f;
        }
    };
    for (int i = 0; i < 31; ++i) f.table[i] = eval((f.radius * (float) i) / 31.0f);
    f.table[31] = 0.0f;
    f.scale_factor = 31.0f / f.radius;
    f.border = (int) std::ceil(f.radius - 0.5f - 2.0f * kRayEpsilon);
    f.taps = (int) std::ceil((f.radius - 2.0f * kRayEpsilon) * 2.0f);
    return 0;
}

template <typename T> int upload(T **dst, const std::vector<T> &src) {
    *dst = nullptr;
    size_t bytes = std::max<size_t>(src.size(), 1) * sizeof(T);
    HIP_TRY(hipMalloc((void **) dst, bytes));
    if (!src.empty()) HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// Every workspace buffer is zeroed when it is allocated: a kernel that reads a slot before the first write of a render (a count, a
// cursor, the spill area, a pool slot beyond a stale count) then reads zeros on every run, not whatever the allocator handed out
// (round 2's fault came from exactly such a read; tests/conftest.py still dirties device memory before every GPU session).
// Out of device memory is reported as MTSAMD_ERR_NOMEM so that callers can retry with a smaller pass.
static int ws_alloc(void **p, size_t bytes) {
    *p = nullptr;
    bytes = std::max<size_t>(bytes, 4);
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory) { (void) hipGetLastError(); *p = nullptr; return fail(MTSAMD_ERR_NOMEM, "out of device memory (%zu bytes of workspace)", bytes); }
    HIP_TRY(e);
    HIP_TRY(hipMemset(*p, 0, bytes));
    return 0;
}
// A workspace buffer that only grows: it holds `have` elements; if `need` are more, it is freed and allocated anew (zeroed).
template <typename T, typename N> static int grow(T *&p, N &have, size_t need) {
    if (have >= need) return 0;
    (void) hipFree(p); p = nullptr; have = 0;
    if (int rc = ws_alloc((void **) &p, need * sizeof(T))) return rc;
    have = (N) need;
    return 0;
}
// ... two buffers of `have` elements each: both are freed before either is allocated anew, and `have` counts once both are there
template <typename A, typename B, typename N> static int grow(A *&a, B *&b, N &have, size_t need) {
    if (have >= need) return 0;
    (void) hipFree(a); (void) hipFree(b); a = nullptr; b = nullptr; have = 0;
    if (int rc = ws_alloc((void **) &a, need * sizeof(A))) return rc;
    if (int rc = ws_alloc((void **) &b, need * sizeof(B))) return rc;
    have = (N) need;
    return 0;
}

struct Workspace {
    uint32_t n_waves = 0, seg_cap = 0;
    uint64_t pass_cap = 0;
    bool spectral = false, split = false;
    PoolView pool[2] = {};
    uint32_t *count[2] = { nullptr, nullptr };
    uint64_t *cursor = nullptr, *cursor_end = nullptr, *wave_stats = nullptr;
    uint32_t *count_shadow = nullptr;
    float4 *out_rgba = nullptr; float2 *out_pos = nullptr;
    float4 *out_rgba2 = nullptr; float2 *out_pos2 = nullptr; uint64_t pass_cap2 = 0;      // second sample stream: pass k + 1 is traced while pass k is splatted
    hipStream_t film_stream = nullptr; hipEvent_t film_done[2] = {};
    float *moment_film = nullptr; uint64_t moment_floats = 0;     // moment integrator: two scratch 5-channel films
    float4 *aov_stream = nullptr; uint64_t aov_stream_slots = 0;  // aov integrator: channel groups of a pass (+ the nested stream's second colour space)
    float *aov_film = nullptr; uint64_t aov_film_floats = 0;      // ... and its scratch 5-channel films
    float4 *aov_keep = nullptr;                                   // ... and, during a render of several passes, the streams + positions of all of them
    float *film_partials = nullptr; size_t film_partial_floats = 0;      // tiled film splat: one scratch tile per 16x16 source tile of a pass
    uint32_t *trace_spill = nullptr; size_t trace_spill_words = 0;      // k_trace: deep stack entries
    // forward-mode render: the two perturbed BSDF tables, 1 / (2 eps) per record, the emitter tangent rows
    DevBsdf *fw_plus = nullptr, *fw_minus = nullptr; size_t fw_records = 0;
    float *fw_inv_2h = nullptr; size_t fw_inv_floats = 0;
    float *fw_emitters = nullptr; size_t fw_emitter_floats = 0;
    // reverse-mode render: the slot table of the wanted BSDF scalars and the slot range of every record
    ReverseSlot *rv_slots = nullptr; size_t rv_slot_count = 0;
    uint32_t *rv_range = nullptr; size_t rv_range_words = 0;
    uint32_t *h_counts = nullptr;        // pinned, 4 * n_waves
    uint64_t *h_cursor = nullptr;        // pinned, 2 * n_waves
    uint64_t *h_cursor_rb = nullptr;     // pinned, 2 slots x n_waves: cursors read back with the counts (pool-drain gathering)
    hipEvent_t ev[4] = {};               // 0 / 1: count read-back checkpoints, 2: k_shade done, 3: k_trace<any> done
    hipStream_t stream2 = nullptr;       // split pipeline: k_trace<any> of one iteration overlaps k_trace<closest> of the next
    hipStream_t part_stream[3] = {}; hipEvent_t part_ev[3] = {};      // flat scenes: further parts of the scheduling waves
    // hierarchy scenes: launch chain k runs k_trace<closest> + k_shade on chain_main[k] (chain 0: the job's stream) and k_trace<any> on
    // chain_any[k]; chain_ev[2k] = its k_shade is done, chain_ev[2k + 1] = its k_trace<any> is done
    hipStream_t chain_main[kMaxChains] = {}, chain_any[kMaxChains] = {}; hipEvent_t chain_ev[2 * kMaxChains] = {};
    hipEvent_t tev[3] = {};              // timing: bounce loop begin / end, film end
    bool have_events = false;
    std::vector<hipEvent_t> prof_ev;     // desc->profile: begin / end events of the split pipeline's launches, reused pass after pass
    std::vector<hipEvent_t> film_ev;     // begin / end events of the film splats of a render

    void release() {
        for (int k = 0; k < 2; ++k) {
            (void) hipFree(pool[k].ray_o); (void) hipFree(pool[k].ray_d); (void) hipFree(pool[k].thr); (void) hipFree(pool[k].res);
            (void) hipFree(pool[k].rng); (void) hipFree(pool[k].misc); (void) hipFree(count[k]);
            (void) hipFree(pool[k].xi); (void) hipFree(pool[k].aux);
            (void) hipFree(pool[k].hit); (void) hipFree(pool[k].sh_o); (void) hipFree(pool[k].sh_d); (void) hipFree(pool[k].nee); (void) hipFree(pool[k].sh_slot);
            pool[k] = PoolView{}; count[k] = nullptr;
        }
        (void) hipFree(cursor); (void) hipFree(cursor_end); (void) hipFree(wave_stats);
        (void) hipFree(count_shadow); count_shadow = nullptr;
        (void) hipFree(trace_spill); trace_spill = nullptr; trace_spill_words = 0;
        (void) hipFree(fw_plus); (void) hipFree(fw_minus); fw_plus = fw_minus = nullptr; fw_records = 0;
        (void) hipFree(fw_inv_2h); fw_inv_2h = nullptr; fw_inv_floats = 0;
        (void) hipFree(fw_emitters); fw_emitters = nullptr; fw_emitter_floats = 0;
        (void) hipFree(rv_slots); rv_slots = nullptr; rv_slot_count = 0;
        (void) hipFree(rv_range); rv_range = nullptr; rv_range_words = 0;
        (void) hipFree(moment_film); moment_film = nullptr; moment_floats = 0;
        (void) hipFree(aov_stream); aov_stream = nullptr; aov_stream_slots = 0;
        (void) hipFree(aov_film); aov_film = nullptr; aov_film_floats = 0;
        (void) hipFree(aov_keep); aov_keep = nullptr;
        (void) hipFree(film_partials); film_partials = nullptr; film_partial_floats = 0;
        (void) hipFree(out_rgba); (void) hipFree(out_pos);
        (void) hipFree(out_rgba2); (void) hipFree(out_pos2); out_rgba2 = nullptr; out_pos2 = nullptr; pass_cap2 = 0;
        if (film_stream) (void) hipStreamDestroy(film_stream);
        film_stream = nullptr;
        for (auto &e : film_done) { if (e) (void) hipEventDestroy(e); e = nullptr; }
        cursor = cursor_end = wave_stats = nullptr; out_rgba = nullptr; out_pos = nullptr;
        if (h_counts) (void) hipHostFree(h_counts);
        if (h_cursor) (void) hipHostFree(h_cursor);
        if (h_cursor_rb) (void) hipHostFree(h_cursor_rb);
        h_cursor_rb = nullptr;
        h_counts = nullptr; h_cursor = nullptr;
        if (stream2) (void) hipStreamDestroy(stream2);
        stream2 = nullptr;
        for (auto &ps : part_stream) { if (ps) (void) hipStreamDestroy(ps); ps = nullptr; }
        for (auto &ps : chain_main) { if (ps) (void) hipStreamDestroy(ps); ps = nullptr; }
        for (auto &ps : chain_any) { if (ps) (void) hipStreamDestroy(ps); ps = nullptr; }
        for (auto &pe : chain_ev) { if (pe) (void) hipEventDestroy(pe); pe = nullptr; }
        for (auto &pe : part_ev) { if (pe) (void) hipEventDestroy(pe); pe = nullptr; }
        if (have_events) for (auto &e : ev) (void) hipEventDestroy(e);
        have_events = false;
        for (auto &e : prof_ev) (void) hipEventDestroy(e);
        prof_ev.clear();
        for (auto &e : film_ev) (void) hipEventDestroy(e);
        film_ev.clear();
        n_waves = seg_cap = 0; pass_cap = 0;
    }
};

} // namespace

// quad::gauss_legendre (src/libcore/quad.cpp:7-66, legendre_pd: math.h:127-154): nodes / weights on [-1, 1]
static void gauss_legendre(int n, float *nodes, float *weights) {
    auto legendre_pd = [](int l, double x, double &lv, double &dv) {
        double l_cur = 0.0, d_cur = 0.0;
        if (l > 1) {
            double l_p_pred = 1.0, l_pred = x, d_p_pred = 0.0, d_pred = 1.0, k0 = 3.0, k1 = 2.0, k2 = 1.0;
            for (int ki = 2; ki <= l; ++ki) {
                l_cur = (k0 * x * l_pred - k2 * l_p_pred) / k1;
                d_cur = d_p_pred + k0 * l_pred;
                l_p_pred = l_pred; l_pred = l_cur; d_p_pred = d_pred; d_pred = d_cur;
                k2 = k1; k0 += 2.0; k1 += 1.0;
            }
        } else if (l == 0) { l_cur = 1.0; d_cur = 0.0; }
        else { l_cur = x; d_cur = 1.0; }
        lv = l_cur; dv = d_cur;
    };
    n--;
    if (n == 0) { nodes[0] = 0.0f; weights[0] = 2.0f; }
    else if (n == 1) { nodes[0] = (float) -std::sqrt(1.0 / 3.0); nodes[1] = -nodes[0]; weights[0] = weights[1] = 1.0f; }
    const int m = (n + 1) / 2;
    for (int i = 0; i < m; ++i) {
        double x = -std::cos((double) (2 * i + 1) / (double) (2 * n + 2) * 3.14159265358979323846);
        double l, d;
        for (int it = 0; it < 20; ++it) {
            legendre_pd(n + 1, x, l, d);
            const double step = l / d;
            x -= step;
            if (std::fabs(step) <= 4 * std::fabs(x) * 2.220446049250313e-16) break;
        }
        legendre_pd(n + 1, x, l, d);
        weights[i] = weights[n - i] = (float) (2 / ((1 - x * x) * (d * d)));
        nodes[i] = (float) x; nodes[n - i] = (float) -x;
    }
    if ((n % 2) == 0) {
        double l, d;
        legendre_pd(n + 1, 0.0, l, d);
        weights[n / 2] = (float) (2.0 / (d * d));
        nodes[n / 2] = 0.0f;
    }
}

// An emitter colour of the spectral variant (an envmap texel, a radiance / intensity / irradiance) is stored as (c, sc) with
// sc = 2 max(r, g, b), n = rgb / max(1e-8, sc), c = srgb_model_fetch(n).  out4 = (c0, c1, c2, sc); jn[3 ch + j] = d c_j / d rgb_ch, composed
// in double from the Jacobian of the fetch at n:  d n_j / d rgb_j = 1 / sc for j != m,  d n_j / d rgb_m = -n_j / rgb_m,  n_m = 0.5 is a
// constant; *m_out = m, the channel that attains the maximum -- the lowest one on a tie, which is the value std::max(std::max(r, g), b)
// returns.  A colour whose largest component is <= 0 is not differentiable (n = 0 / 0, sentinel coefficients): jn = 0 and m = -1.
static void emitter_colour_jacobian(const Rgb2Spec &model, const float rgb[3], float out4[4], double jn[9], int *m_out) {
    const float sc = std::max(std::max(rgb[0], rgb[1]), rgb[2]) * 2.0f, dn = std::max(1e-8f, sc);
    const float n[3] = { rgb[0] / dn, rgb[1] / dn, rgb[2] / dn };
    srgb_model_fetch(model, n, out4);
    out4[3] = sc;
    for (int k = 0; k < 9; ++k) jn[k] = 0.0;
    *m_out = -1;
    if (!(sc > 0.0f)) return;
    const int m = (rgb[0] >= rgb[1] && rgb[0] >= rgb[2]) ? 0 : (rgb[1] >= rgb[2] ? 1 : 2);
    *m_out = m;
    float jf[9];
    srgb_model_fetch_jacobian(model, n, jf);
    for (int ch = 0; ch < 3; ++ch)
        for (int j = 0; j < 3; ++j) {
            if (sc < 1e-8f) jn[3 * ch + j] = (double) jf[3 * ch + j] / (double) dn;        // below the clamp of the divisor n is linear in rgb
            else if (ch != m) {
                jn[3 * ch + j] = (double) jf[3 * ch + j] / (double) sc;
                jn[3 * m + j] -= (double) n[ch] / (double) rgb[m] * (double) jf[3 * ch + j];
            }
        }
}

// 12 floats of the device table of k_emitter_grad_to_rgb for one emitter colour: jn in the centred basis of model_coeff_grad
// (l = mid + half u gives a = half^2 c0, b = 2 mid half c0 + half c1, c = mid^2 c0 + mid c1 + c2), then d scale / d rgb
static void emitter_jacobian_row(const Rgb2Spec &model, const float rgb[3], float row[12]) {
    float out4[4]; double jn[9]; int m;
    emitter_colour_jacobian(model, rgb, out4, jn, &m);
    const double mid = kCoeffMid, half = kCoeffHalf;
    for (int ch = 0; ch < 3; ++ch) {
        const double *j = jn + 3 * ch;
        row[3 * ch] = (float) (half * half * j[0]);
        row[3 * ch + 1] = (float) (2.0 * mid * half * j[0] + half * j[1]);
        row[3 * ch + 2] = (float) (mid * mid * j[0] + mid * j[1] + j[2]);
        row[9 + ch] = ch == m ? 2.0f : 0.0f;
    }
}

// A scene: the host records the setters edit (SceneState, scene_build.h) and everything that lives on the device
struct mtsamd_scene : SceneState {
    int device = 0;
    int cu_count = 256;
    float4 *d_nodes = nullptr, *d_tris = nullptr;
    uint4 *d_qnodes = nullptr, *d_wnodes = nullptr;
    StackEntry *d_walk_spill = nullptr;
    float *d_tri_pos = nullptr, *d_tri_nrm = nullptr, *d_tri_uv = nullptr;
    uint32_t *d_prim_shape = nullptr;
    DevShape *d_shapes = nullptr; DevBsdf *d_bsdfs = nullptr; DevEmitter *d_emitters = nullptr;
    float *d_area_pmf = nullptr, *d_area_cdf = nullptr;
    float *d_rough_tables = nullptr;     // roughplastic: 64 floats per BSDF that needs them
    float *d_env_texels = nullptr, *d_env_warp = nullptr; DevEnvmap *d_envmap = nullptr;      // envmap emitter
    float4 *d_flat = nullptr, *d_pairs = nullptr;
    // spectral variant: d_jac = the Jacobians [bsdfs | texels] (jac_bsdf, jac_tex; uploaded by mtsamd_render_adjoint_spectral when `jac_dirty`),
    // d_cgrad = its coefficient-gradient scratch (3 floats each); d_ejac = the table of mtsamd_render_adjoint_spectral_emitters, 12 floats per
    // colour for [emitters | envmap texels] (emitter_jacobian_row), rebuilt when `ejac_dirty`; d_egrad = its 4-float (coefficient, scale) rows
    float *d_jac = nullptr, *d_cgrad = nullptr;
    float *d_ejac = nullptr, *d_egrad = nullptr;
    DevTexture *d_textures = nullptr;       // the table `textures`, whose `data` are device pointers owned by the scene
    // vertex updates (mtsamd_scene_set_vertex_positions), hierarchy scenes: the refit table (bvh.h) as refit.hip reads it, and scratch for
    // one shape: staged vertex arrays, triangle areas, the flag of the finite check
    uint32_t *d_faces = nullptr, *d_prim_slot = nullptr, *d_slot_prim = nullptr, *d_order = nullptr, *d_refit_flag = nullptr;
    int2 *d_kids = nullptr;
    int32_t *d_node_child = nullptr, *d_wide_child = nullptr;
    float *d_boxes = nullptr, *d_stage_pos = nullptr, *d_stage_nrm = nullptr, *d_stage_area = nullptr;
    std::vector<uint32_t> class_start;      // height classes of d_order
    // MTSAMD_VERTICES_RECOMPUTE_NORMALS, hierarchy scenes: per shape its vertex-to-corner table (build_corner_table), null until the first
    // recompute of that shape; d_face_recs: 6 floats per face of the largest shape, allocated with the first table
    std::vector<uint32_t *> d_corner_offsets, d_corners;
    float *d_face_recs = nullptr;
    int32_t refit_root = 0;
    size_t n_tri_nrm = 0;                   // floats in d_tri_nrm
    // accelerator rebuilds (mtsamd_scene_rebuild_accel), hierarchy scenes: the scratch of the device build and a second set of every
    // array a build writes, sized for the worst case, both allocated at the first rebuild and kept.  A build goes into `spare`; accepted,
    // it becomes the live set and the former live set the spare (the set of creation, sized for its own tree, is freed instead).
    LbvhScratch *lbvh_scratch = nullptr;
    SahScratch *sah_scratch = nullptr;      // of the SAH builder (sah_build.h), allocated at its first use
    LbvhTarget spare{};
    bool accel_worst_case = false;          // the live set is sized for the worst case
    uint32_t n_builder = 0, builder = 0, rebuilds = 0;      // builder nodes; 0 = binned SAH (creation), 1 = LBVH; rebuilds so far
    size_t walk_spill_entries = 0;          // entries in d_walk_spill
    double *d_sah_partial = nullptr; size_t sah_partial_cap = 0;      // mtsamd_scene_accel_info: per-block sums of the SAH cost
    uint32_t n_pairs = 0, n_clusters = 0;
    BuildOptions options;
    SceneView view{};
    Workspace ws;
    std::atomic<int> cancel{ 0 };
    uint64_t aov_keep_limit = 1ull << 30;      // mtsamd_scene_set_aov_keep_limit
};

namespace {

struct SceneDestroyer { void operator()(mtsamd_scene *s) const { mtsamd_scene_destroy(s); } };

BuildOptions build_options() {       // the shipped values, or what an experiment build finds in the environment
    BuildOptions o;
    if (const char *e = exp_env("MTSAMD_BVH_LEAF")) o.max_leaf = (uint32_t) std::min(15, std::max(1, atoi(e)));
    if (const char *e = exp_env("MTSAMD_BVH_BINS")) o.bvh.bins = atoi(e);
    if (const char *e = exp_env("MTSAMD_BVH_ICOST")) o.bvh.intersect_cost = atof(e);
    if (const char *e = exp_env("MTSAMD_BVH_SWEEP")) o.bvh.sweep_below = (uint32_t) std::max(0, atoi(e));
    if (const char *e = exp_env("MTSAMD_BVH_ORDER")) o.bvh.dfs_order = e[0] == 'd';
    if (const char *e = exp_env("MTSAMD_FLAT_MAX")) o.flat_max = std::min<uint32_t>(kFlatMaxPrims, (uint32_t) std::strtoul(e, nullptr, 10));
    return o;
}

ScheduleSwitches schedule_switches() {       // nothing set, or what an experiment build finds in the environment
    ScheduleSwitches sw;
    if (const char *e = exp_env("MTSAMD_CHUNKS_PER_WAVE")) sw.chunks_per_wave = (uint32_t) std::min(64, std::max(1, atoi(e)));
    if (const char *e = exp_env("MTSAMD_CHAINS")) sw.chains = (uint32_t) std::min<int>(kMaxChains, std::max(1, atoi(e)));
    sw.one_chain = exp_env("MTSAMD_ONE_CHAIN") != nullptr;
    if (const char *e = exp_env("MTSAMD_STREAMS")) sw.streams = (uint32_t) std::min(4, std::max(1, atoi(e)));
    sw.no_gather = exp_env("MTSAMD_NO_GATHER") != nullptr;
    sw.mega = exp_env("MTSAMD_MEGA") != nullptr;
    if (const char *e = exp_env("MTSAMD_WAVES_PER_CU")) sw.waves_per_cu = (uint32_t) std::max(1, atoi(e));
    return sw;
}

// Everything build_host_scene made goes to the device; the scene owns every buffer from the moment it is allocated.
int upload_scene(mtsamd_scene *s, HostScene &hs) {
    for (size_t t = 0; t < s->textures.size(); ++t) {
        DevTexture &dt = s->textures[t];
        if (dt.kind != 0) continue;
        const size_t bytes = sizeof(float) * 3 * (size_t) dt.w * dt.h;
        if (hipMalloc((void **) &dt.data, bytes) != hipSuccess || hipMemcpy((void *) dt.data, hs.tex_src[t], bytes, hipMemcpyHostToDevice) != hipSuccess)
            return fail(MTSAMD_ERR_NOMEM, "texture %u: upload failed", (uint32_t) t);
    }
    if (s->spectral) {
        float tx[95], ty[95], tz[95], td[95];
        for (int i = 0; i < 95; ++i) { tx[i] = (float) kCie_x[i]; ty[i] = (float) kCie_y[i]; tz[i] = (float) kCie_z[i]; td[i] = (float) kCie_d65[i]; }
        if (upload_spectral_tables(tx, ty, tz, td) != hipSuccess) return fail(MTSAMD_ERR_DEVICE, "spectral table upload failed");
    }
    const BvhOutput &bvh = s->bvh;
    std::vector<float4> nodes(4 * (size_t) bvh.n_nodes), tris(3 * (size_t) bvh.n_slots);
    std::memcpy(nodes.data(), bvh.nodes.data(), bvh.nodes.size() * sizeof(float));
    std::vector<uint4> qnodes(2 * (size_t) bvh.n_nodes);
    std::memcpy(qnodes.data(), bvh.qnodes.data(), bvh.qnodes.size() * sizeof(uint32_t));
    std::vector<uint4> wnodes(4 * (size_t) bvh.n_wnodes);
    std::memcpy(wnodes.data(), (MTS_NODE_P15 ? bvh.wnodes_p : (MTS_NODE_F16 ? bvh.wnodes_h : bvh.wnodes)).data(), bvh.wnodes.size() * sizeof(uint32_t));
    std::memcpy(tris.data(), bvh.tris.data(), bvh.tris.size() * sizeof(float));
    int rc = 0;
    if ((rc = upload(&s->d_textures, s->textures)) || (rc = upload(&s->d_flat, hs.flat_recs)) || (rc = upload(&s->d_pairs, hs.pair_recs)) ||
        (rc = upload(&s->d_nodes, nodes)) || (rc = upload(&s->d_qnodes, qnodes)) || (rc = upload(&s->d_wnodes, wnodes)) || (rc = upload(&s->d_tris, tris)) ||
        (rc = upload(&s->d_tri_pos, hs.tri_pos)) || (rc = upload(&s->d_tri_nrm, hs.tri_nrm)) || (rc = upload(&s->d_tri_uv, hs.tri_uv)) ||
        (rc = upload(&s->d_prim_shape, hs.prim_shape)) || (rc = upload(&s->d_shapes, hs.shapes)) || (rc = upload(&s->d_bsdfs, hs.bsdf_block)) ||
        (rc = upload(&s->d_emitters, s->emitters)) || (rc = upload(&s->d_area_pmf, hs.area_pmf)) || (rc = upload(&s->d_area_cdf, hs.area_cdf)))
        return rc;
    if (hs.has_envmap) {
        if ((rc = upload(&s->d_env_texels, hs.env.texels)) || (rc = upload(&s->d_env_warp, hs.env.warp))) return rc;
        std::vector<DevEnvmap> one(1, hs.dev_env);
        one[0].data = reinterpret_cast<const float4 *>(s->d_env_texels); one[0].warp = s->d_env_warp;
        if ((rc = upload(&s->d_envmap, one))) return rc;
    }
    return MTSAMD_OK;
}

// What a vertex update of a hierarchy scene needs on the device.  A flat scene is updated on the host (at most kFlatMaxPrims
// primitives) and keeps the host arrays instead; a hierarchy scene drops the host copies of what the device now owns.
int upload_refit_table(mtsamd_scene *s, HostScene &hs) {
    s->n_tri_nrm = hs.tri_nrm.size(); s->n_pairs = hs.n_pairs; s->n_clusters = hs.n_clusters;
    if (hs.flat || s->n_prims == 0) return MTSAMD_OK;
    BvhOutput &bvh = s->bvh;
    RefitTable &rt = bvh.refit;
    SceneGeometry &g = s->geometry;
    std::vector<uint32_t> prim_slot(s->n_prims, 0u);
    for (size_t i = 0; i < rt.slot_prim.size(); ++i) prim_slot[rt.slot_prim[i]] = (uint32_t) i;
    std::vector<int2> kids(rt.left.size());
    for (size_t t = 0; t < kids.size(); ++t) kids[t] = rt.left[t] >= 0 ? make_int2(rt.left[t], rt.right[t]) : make_int2(-1, (int32_t) rt.ref2[t]);
    uint32_t max_vertices = 0, max_faces = 0;
    for (size_t i = 0; i < g.shapes.size(); ++i) { max_vertices = std::max(max_vertices, g.shape_vertices[i]); max_faces = std::max(max_faces, g.shape_faces[i]); }
    int rc = 0;
    if ((rc = upload(&s->d_faces, g.faces)) || (rc = upload(&s->d_prim_slot, prim_slot)) || (rc = upload(&s->d_slot_prim, rt.slot_prim)) ||
        (rc = upload(&s->d_kids, kids)) || (rc = upload(&s->d_order, rt.order)) || (rc = upload(&s->d_node_child, rt.node_child)) ||
        (rc = upload(&s->d_wide_child, rt.wide_child)) || (rc = upload(&s->d_boxes, rt.boxes)))
        return rc;
    HIP_TRY(hipMalloc((void **) &s->d_stage_pos, sizeof(float) * 3 * (size_t) std::max(max_vertices, 1u)));
    HIP_TRY(hipMalloc((void **) &s->d_stage_nrm, sizeof(float) * 3 * (size_t) std::max(max_vertices, 1u)));
    HIP_TRY(hipMalloc((void **) &s->d_stage_area, sizeof(float) * (size_t) std::max(max_faces, 1u)));
    HIP_TRY(hipMalloc((void **) &s->d_refit_flag, sizeof(uint32_t)));
    s->class_start = rt.class_start; s->refit_root = rt.root; s->n_builder = (uint32_t) kids.size();
    // the device owns these now; the counts (n_nodes, n_wnodes, n_slots), roots, bbox and grid stay
    bvh.nodes = {}; bvh.qnodes = {}; bvh.wnodes = {}; bvh.wnodes_h = {}; bvh.wnodes_p = {}; bvh.tris = {};
    rt = RefitTable{};
    g.faces = {}; g.prim_shape = {};
    return MTSAMD_OK;
}

// flat scenes: the frame words of the shading records, which build_flat_records leaves zero, are computed on the device by the
// functions the path kernels would call per hit (k_flat_frames).  Every upload of flat_recs is followed by this step.
int flat_frames(mtsamd_scene *s, const HostScene &hs) {
    if (!MTS_FLAT_FRAMES || !hs.flat || s->n_prims == 0) return MTSAMD_OK;
    hipError_t err = launch_flat_frames(s->d_flat, s->n_prims, s->d_shapes, hs.tri_uv.empty() ? nullptr : s->d_tri_uv, nullptr);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) return fail(MTSAMD_ERR_DEVICE, "flat frames: %s", hipGetErrorString(err));
    return MTSAMD_OK;
}

// roughplastic: transmittance tables and internal reflectance are integrated on the device (roughplastic.cpp:380-399)
int roughplastic_tables(mtsamd_scene *s) {
    std::vector<uint32_t> rough;
    for (uint32_t b = 0; b < (uint32_t) s->bsdfs.size(); ++b) if (s->bsdfs[b].type == kBsdfRoughPlastic) rough.push_back(b);
    if (rough.empty()) return MTSAMD_OK;
    float *d_gl = nullptr;
    if (hipMalloc((void **) &s->d_rough_tables, rough.size() * kRoughTableRes * sizeof(float)) != hipSuccess ||
        hipMalloc((void **) &d_gl, 512 * sizeof(float)) != hipSuccess)
        return fail(MTSAMD_ERR_NOMEM, "roughplastic tables: allocation failed");
    hipError_t err = hipSuccess;
    for (size_t k = 0; k < rough.size() && err == hipSuccess; ++k) {
        const float eta = s->bsdfs[rough[k]].er;
        const int res_t = eta > 1.0f ? 32 : 128, res_r = (1.0f / eta) > 1.0f ? 32 : 128;      // microfacet.h:476-478,520-522
        float gl[512] = {};
        gauss_legendre(res_t, gl, gl + 128);
        gauss_legendre(res_r, gl + 256, gl + 384);
        err = hipMemcpy(d_gl, gl, sizeof(gl), hipMemcpyHostToDevice);
        if (err == hipSuccess) err = launch_roughplastic_tables(s->d_bsdfs, rough[k], s->d_rough_tables + k * kRoughTableRes, d_gl, res_t, res_r, nullptr);
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    if (err == hipSuccess) err = hipMemcpy(s->bsdfs.data(), s->d_bsdfs, s->bsdfs.size() * sizeof(DevBsdf), hipMemcpyDeviceToHost);
    (void) hipFree(d_gl);
    if (err != hipSuccess) return fail(MTSAMD_ERR_DEVICE, "roughplastic tables: %s", hipGetErrorString(err));
    return MTSAMD_OK;
}

int fill_scene_view(mtsamd_scene *s, const HostScene &hs) {
    SceneView &v = s->view;
    v.nodes = s->d_nodes; v.qnodes = s->d_qnodes; v.wnodes = s->d_wnodes; v.wroot = s->bvh.wroot; v.n_wnodes = s->bvh.n_wnodes; v.tris = s->d_tris; v.root = s->bvh.root;
    for (int k = 0; k < 3; ++k) { v.q_lo[k] = s->bvh.q_lo[k]; v.q_step[k] = s->bvh.q_step[k]; v.q_inv_step[k] = 1.0f / s->bvh.q_step[k]; }
    v.n_nodes = s->bvh.n_nodes; v.n_slots = s->bvh.n_slots; v.n_prims = s->n_prims;
    // LDS residency: flat scenes keep everything in LDS (flat_recs).  For hierarchy scenes staging the
    // top of the tree (nodes are stored in BFS order) was measured to LOSE: 384 staged nodes 2.5-3.2 Gray/s vs none
    // 3.8-4.8 Gray/s on a 261 k-triangle mesh -- the 24 KB cost occupancy and the LDS/global select compiles to
    // generic (flat) loads, while the top levels stay L1/L2-resident anyway.  Only the traversal stack lives in LDS.
    v.lds_nodes = 0; v.lds_slots = 0;      // nodes and triangle slots are always read through L1/L2
    // BVH2: one deferred subtree per level; BVH4: up to three
    v.stack_depth = MTS_BVH4 ? 3u * s->bvh.wdepth + 2u : std::max<uint32_t>(s->bvh.depth, 2);
    // standalone ray streams: 8 persistent workgroups per CU, the first 12 (BVH2: 16) stack entries of a lane in LDS
    v.walk_lds_depth = std::min<uint32_t>(v.stack_depth, MTS_BVH4 ? 8u : 16u);      // 16 KB per workgroup: 8 workgroups (k_ray_walk: 8 waves per SIMD) per CU
    v.walk_blocks = 8u * (uint32_t) s->cu_count;
    if (!hs.flat && v.stack_depth > v.walk_lds_depth) {
        const size_t entries = (size_t) v.walk_blocks * (v.stack_depth - v.walk_lds_depth) * 256u;
        if (ws_alloc((void **) &s->d_walk_spill, entries * sizeof(StackEntry))) return fail(MTSAMD_ERR_NOMEM, "traversal spill area");
        s->walk_spill_entries = entries;
    }
    v.walk_spill = s->d_walk_spill;
    v.tri_pos = s->d_tri_pos; v.tri_nrm = hs.tri_nrm.empty() ? nullptr : s->d_tri_nrm; v.tri_uv = hs.tri_uv.empty() ? nullptr : s->d_tri_uv;
    v.prim_shape = s->d_prim_shape; v.shapes = s->d_shapes; v.bsdfs = s->d_bsdfs;
    v.emitters = s->d_emitters; v.n_emitters = (uint32_t) s->emitters.size();
    v.env_emitter = s->environment; v.envmap = s->d_envmap;
    v.area_pmf = s->d_area_pmf; v.area_cdf = s->d_area_cdf;
    v.n_shapes = s->n_shapes; v.n_bsdfs = (uint32_t) s->bsdfs.size();
    v.textures = s->d_textures; v.n_textures = (uint32_t) s->textures.size();
    v.flat_recs = s->d_flat; v.flat = hs.flat ? 1u : 0u;
    v.general = s->nested_bsdfs ? 2u : (s->general_bsdfs || s->delta_emitters || s->environment >= 0) ? 1u : 0u;       // the diffuse / area-light fast path (kernels.hip) handles none of these
    v.flat_pairs = s->d_pairs; v.n_pairs = hs.n_pairs; v.n_clusters = hs.n_clusters;
    v.n_spectra = hs.n_spectra;
    // hierarchy scenes only: a flat scene is within kFlatLdsCap in every launch, or build_host_scene would not have kept it flat
    static_assert(kStackLdsCap == kFlatLdsCap, "bvh.h restates the LDS cap of kernels.h");
    if (bounce_lds_bytes(v) > kFlatLdsCap || (!hs.flat && !bvh_stack_fits(v.stack_depth, sizeof(StackEntry)))) return fail(MTSAMD_ERR_UNSUPPORTED, "BVH too deep for the LDS traversal stack (depth %u)", v.stack_depth);
    return MTSAMD_OK;
}

} // namespace

extern "C" {

int mtsamd_abi_version(void) { return MTSAMD_ABI_VERSION; }
// MTS_EXPORT_PLUGIN (include/mitsuba/core/class.h:205-211): what PluginManager reads after dlopen (src/libcore/plugin.cpp:19-31)
const char *plugin_name(void) { return "path_amd"; }
const char *plugin_descr(void) { return "Wavefront path tracer for AMD MI355X (gfx950)"; }
const char *mtsamd_last_error(void) { return last_error(); }

int mtsamd_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(MTSAMD_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

static void free_target(LbvhTarget &t) {
    (void) hipFree(t.prim_slot); (void) hipFree(t.slot_prim); (void) hipFree(t.order); (void) hipFree(t.kids); (void) hipFree(t.node_child); (void) hipFree(t.wide_child);
    (void) hipFree(t.boxes); (void) hipFree(t.tris); (void) hipFree(t.nodes); (void) hipFree(t.qnodes); (void) hipFree(t.wnodes);
    t = LbvhTarget{};
}

void mtsamd_scene_destroy(mtsamd_scene *s) {
    if (!s) return;
    (void) hipSetDevice(s->device);
    s->ws.release();
    (void) hipFree(s->d_nodes); (void) hipFree(s->d_qnodes); (void) hipFree(s->d_wnodes); (void) hipFree(s->d_walk_spill); (void) hipFree(s->d_tris); (void) hipFree(s->d_tri_pos); (void) hipFree(s->d_tri_nrm); (void) hipFree(s->d_tri_uv);
    (void) hipFree(s->d_prim_shape); (void) hipFree(s->d_shapes); (void) hipFree(s->d_bsdfs); (void) hipFree(s->d_emitters);
    (void) hipFree(s->d_area_pmf); (void) hipFree(s->d_area_cdf); (void) hipFree(s->d_rough_tables);
    (void) hipFree(s->d_env_texels); (void) hipFree(s->d_env_warp); (void) hipFree(s->d_envmap); (void) hipFree(s->d_flat); (void) hipFree(s->d_pairs);
    for (auto &t : s->textures) (void) hipFree((void *) t.data);
    (void) hipFree(s->d_faces); (void) hipFree(s->d_prim_slot); (void) hipFree(s->d_slot_prim); (void) hipFree(s->d_order); (void) hipFree(s->d_refit_flag); (void) hipFree(s->d_kids);
    (void) hipFree(s->d_node_child); (void) hipFree(s->d_wide_child); (void) hipFree(s->d_boxes); (void) hipFree(s->d_stage_pos); (void) hipFree(s->d_stage_nrm); (void) hipFree(s->d_stage_area);
    for (uint32_t *p : s->d_corner_offsets) (void) hipFree(p);
    for (uint32_t *p : s->d_corners) (void) hipFree(p);
    (void) hipFree(s->d_face_recs);
    lbvh_scratch_destroy(s->lbvh_scratch);
    sah_scratch_destroy(s->sah_scratch);
    free_target(s->spare);
    (void) hipFree(s->d_sah_partial);
    (void) hipFree(s->d_textures); (void) hipFree(s->d_jac); (void) hipFree(s->d_cgrad); (void) hipFree(s->d_ejac); (void) hipFree(s->d_egrad);
    delete s;
}

// the three creation entry points: a scene holds tabulated spectra (spectral variant) or textured parameters (RGB variant), or neither
static int create_scene(const mtsamd_scene_desc *desc, const mtsamd_spectrum_desc *spectra, uint32_t n_spectra, const mtsamd_spectrum_binding *bindings,
                        uint32_t n_bindings, const mtsamd_texture_binding *tex_bindings, uint32_t n_tex_bindings, int device, mtsamd_scene **out);

int mtsamd_scene_create(const mtsamd_scene_desc *desc, int device, mtsamd_scene **out) {
    return create_scene(desc, nullptr, 0, nullptr, 0, nullptr, 0, device, out);
}

int mtsamd_scene_create_with_spectra(const mtsamd_scene_desc *desc, const mtsamd_spectrum_desc *spectra, uint32_t n_spectra,
                                     const mtsamd_spectrum_binding *bindings, uint32_t n_bindings, int device, mtsamd_scene **out) {
    return create_scene(desc, spectra, n_spectra, bindings, n_bindings, nullptr, 0, device, out);
}

int mtsamd_scene_create_with_textures(const mtsamd_scene_desc *desc, const mtsamd_texture_binding *bindings, uint32_t n_bindings, int device, mtsamd_scene **out) {
    return create_scene(desc, nullptr, 0, nullptr, 0, bindings, n_bindings, device, out);
}

static int create_scene(const mtsamd_scene_desc *desc, const mtsamd_spectrum_desc *spectra, uint32_t n_spectra, const mtsamd_spectrum_binding *bindings,
                        uint32_t n_bindings, const mtsamd_texture_binding *tex_bindings, uint32_t n_tex_bindings, int device, mtsamd_scene **out) {
    if (!desc || !out) return fail(MTSAMD_ERR_INVALID, "mtsamd_scene_create: null argument");
    *out = nullptr;
    HostScene hs;       // everything the host can check and compute comes first: it needs no device
    if (int rc = build_host_scene(desc, spectra, n_spectra, bindings, n_bindings, build_options(), hs, tex_bindings, n_tex_bindings)) return rc;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(MTSAMD_ERR_INVALID, "invalid device index %d (have %d)", device, ndev);
    HIP_TRY(hipSetDevice(device));

    std::unique_ptr<mtsamd_scene, SceneDestroyer> s(new mtsamd_scene());       // an error return below frees whatever was uploaded
    s->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) s->cu_count = prop.multiProcessorCount;
    static_cast<SceneState &>(*s) = std::move(hs.state);
    s->options = build_options();
    if (int rc = upload_scene(s.get(), hs)) return rc;
    if (int rc = upload_refit_table(s.get(), hs)) return rc;
    if (int rc = flat_frames(s.get(), hs)) return rc;
    if (int rc = roughplastic_tables(s.get())) return rc;
    if (int rc = fill_scene_view(s.get(), hs)) return rc;
    *out = s.release();
    return MTSAMD_OK;
}

int mtsamd_scene_bbox(const mtsamd_scene *s, float *out6) {
    if (!s || !out6) return fail(MTSAMD_ERR_INVALID, "null argument");
    std::memcpy(out6, s->bvh.bbox, sizeof(float) * 6);
    return MTSAMD_OK;
}

int mtsamd_scene_info(const mtsamd_scene *s, uint32_t *out6) {
    if (!s || !out6) return fail(MTSAMD_ERR_INVALID, "null argument");
    out6[0] = s->n_prims; out6[1] = s->bvh.n_nodes; out6[2] = s->bvh.depth; out6[3] = s->n_shapes;
    out6[4] = (uint32_t) s->emitters.size(); out6[5] = s->view.lds_nodes;
    return MTSAMD_OK;
}

// The setters: the host half (scene_build.h) edits the records, then the records it names are pushed to the device.
static int push_bsdf(mtsamd_scene *s, uint32_t bsdf) {
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(s->d_bsdfs + bsdf, &s->bsdfs[bsdf], sizeof(DevBsdf), hipMemcpyHostToDevice));
    return MTSAMD_OK;
}

int mtsamd_scene_set_bsdf_reflectance(mtsamd_scene *s, uint32_t bsdf, const float *rgb) {
    if (!s || !rgb || bsdf >= s->bsdfs.size()) return fail(MTSAMD_ERR_INVALID, "invalid bsdf index");
    if (int rc = set_bsdf_reflectance(*s, bsdf, rgb)) return rc;
    return push_bsdf(s, bsdf);
}

int mtsamd_scene_roughplastic_tables(const mtsamd_scene *s, uint32_t bsdf, float *out65) {
    if (!s || !out65 || bsdf >= s->bsdfs.size()) return fail(MTSAMD_ERR_INVALID, "invalid bsdf index");
    const DevBsdf &b = s->bsdfs[bsdf];
    if (b.type != kBsdfRoughPlastic || !b.table) return fail(MTSAMD_ERR_INVALID, "bsdf %u is not a roughplastic", bsdf);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(out65, b.table, kRoughTableRes * sizeof(float), hipMemcpyDeviceToHost));
    out65[kRoughTableRes] = b.eb;
    return MTSAMD_OK;
}

int mtsamd_scene_update_texture(mtsamd_scene *s, uint32_t texture, const float *rgb, void *stream) {
    if (!s || !rgb || texture >= s->textures.size()) return fail(MTSAMD_ERR_INVALID, "invalid texture index");
    HIP_TRY(hipSetDevice(s->device));
    const DevTexture &t = s->textures[texture];
    if (t.kind != 0) return fail(MTSAMD_ERR_INVALID, "texture %u is not a bitmap", texture);
    const size_t bytes = sizeof(float) * 3 * (size_t) t.w * t.h;
    if (!s->spectral) {
        HIP_TRY(hipMemcpyAsync((void *) t.data, rgb, bytes, hipMemcpyDefault, (hipStream_t) stream));
        if (!texture_feeds_lobe_weight(*s, texture)) return MTSAMD_OK;       // only plastic lobe weights read the mean
    }
    // the host half needs the texels: the spectral variant converts them (the device holds model coefficients), the RGB one takes their mean
    std::vector<float> host(bytes / sizeof(float)), coeffs;
    HIP_TRY(hipStreamSynchronize((hipStream_t) stream));          // whatever writes `rgb`, and the renders that read the old texels
    HIP_TRY(hipMemcpy(host.data(), rgb, bytes, hipMemcpyDefault));
    std::vector<uint32_t> changed;
    set_texture_texels(*s, texture, host.data(), coeffs, changed);
    if (s->spectral) HIP_TRY(hipMemcpy((void *) t.data, coeffs.data(), coeffs.size() * sizeof(float), hipMemcpyHostToDevice));
    for (uint32_t b : changed) HIP_TRY(hipMemcpy(s->d_bsdfs + b, &s->bsdfs[b], sizeof(DevBsdf), hipMemcpyHostToDevice));
    return MTSAMD_OK;
}

int mtsamd_scene_set_emitter_radiance(mtsamd_scene *s, uint32_t emitter, const float *rgb) {
    if (!s || !rgb || emitter >= s->emitters.size()) return fail(MTSAMD_ERR_INVALID, "invalid emitter index");
    if (int rc = set_emitter_radiance(*s, emitter, rgb)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(s->d_emitters + emitter, &s->emitters[emitter], sizeof(DevEmitter), hipMemcpyHostToDevice));
    return MTSAMD_OK;
}

// ---- vertex updates ------------------------------------------------------------------------------------------------------------------
// A flat scene: everything is rebuilt on the host by the code creation runs (set_vertex_positions) and uploaded again; then the frames.
// recompute: the normals are compute_vertex_normals' of the new positions, which are on the host here anyway.
static int flat_vertex_update(mtsamd_scene *s, uint32_t shape, const float *positions, const float *normals, bool recompute, float *normals_out,
                              hipStream_t stream) {
    SceneGeometry &g = s->geometry;
    const size_t nv = 3 * (size_t) g.shape_vertices[shape];
    const bool with_normals = normals || recompute;
    std::vector<float> pos(nv), nrm(with_normals ? nv : 0);
    HIP_TRY(hipStreamSynchronize(stream));          // whatever writes the arrays, and the renders that read the old scene
    HIP_TRY(hipMemcpy(pos.data(), positions, nv * sizeof(float), hipMemcpyDefault));
    if (normals) HIP_TRY(hipMemcpy(nrm.data(), normals, nv * sizeof(float), hipMemcpyDefault));
    if (recompute) {          // a non-finite coordinate is refused below before anything is written; the normals are finite whatever comes in
        compute_vertex_normals(g.shape_vertices[shape], pos.data(), g.shape_faces[shape], g.faces.data() + 3 * (size_t) g.shapes[shape].first_prim, nrm.data());
    }
    FlatRecords fr; fr.flat = true;
    if (int rc = set_vertex_positions(*s, s->options, shape, pos.data(), with_normals ? nrm.data() : nullptr, g.tri_pos, g.tri_nrm, g.area_pmf, g.area_cdf, fr)) return rc;
    if (recompute && normals_out) HIP_TRY(hipMemcpy(normals_out, nrm.data(), nv * sizeof(float), hipMemcpyDefault));
    if (fr.n_pairs != s->n_pairs || fr.n_clusters != s->n_clusters) return fail(MTSAMD_ERR_DEVICE, "vertex update: the flat records changed their size");
    const BvhOutput &bvh = s->bvh;
    auto put = [](void *dst, const void *src, size_t bytes) { return bytes == 0 ? hipSuccess : hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); };
    HIP_TRY(put(s->d_nodes, bvh.nodes.data(), bvh.nodes.size() * sizeof(float)));
    HIP_TRY(put(s->d_qnodes, bvh.qnodes.data(), bvh.qnodes.size() * sizeof(uint32_t)));
    const std::vector<uint32_t> &wn = MTS_NODE_P15 ? bvh.wnodes_p : (MTS_NODE_F16 ? bvh.wnodes_h : bvh.wnodes);
    HIP_TRY(put(s->d_wnodes, wn.data(), wn.size() * sizeof(uint32_t)));
    HIP_TRY(put(s->d_tris, bvh.tris.data(), bvh.tris.size() * sizeof(float)));
    HIP_TRY(put(s->d_tri_pos, g.tri_pos.data(), g.tri_pos.size() * sizeof(float)));
    HIP_TRY(put(s->d_tri_nrm, g.tri_nrm.data(), g.tri_nrm.size() * sizeof(float)));
    HIP_TRY(put(s->d_area_pmf, g.area_pmf.data(), g.area_pmf.size() * sizeof(float)));
    HIP_TRY(put(s->d_area_cdf, g.area_cdf.data(), g.area_cdf.size() * sizeof(float)));
    HIP_TRY(put(s->d_emitters, s->emitters.data(), s->emitters.size() * sizeof(DevEmitter)));
    HIP_TRY(put(s->d_flat, fr.flat_recs.data(), fr.flat_recs.size() * sizeof(float4)));
    HIP_TRY(put(s->d_pairs, fr.pair_recs.data(), fr.pair_recs.size() * sizeof(float4)));
    for (int k = 0; k < 3; ++k) { s->view.q_lo[k] = bvh.q_lo[k]; s->view.q_step[k] = bvh.q_step[k]; s->view.q_inv_step[k] = 1.0f / bvh.q_step[k]; }
    if (MTS_FLAT_FRAMES) {
        HIP_TRY(launch_flat_frames(s->d_flat, s->n_prims, s->d_shapes, s->view.tri_uv, nullptr));
        HIP_TRY(hipDeviceSynchronize());
    }
    return MTSAMD_OK;
}

static RefitView refit_view(const mtsamd_scene *s) {
    RefitView rv{};
    rv.faces = s->d_faces; rv.prim_slot = s->d_prim_slot; rv.slot_prim = s->d_slot_prim; rv.kids = s->d_kids; rv.order = s->d_order;
    rv.node_child = s->d_node_child; rv.wide_child = s->d_wide_child; rv.boxes = s->d_boxes;
    rv.n_nodes = s->bvh.n_nodes; rv.n_wide = s->bvh.n_wnodes;
    rv.tri_pos = s->d_tri_pos; rv.tri_nrm = s->n_tri_nrm ? s->d_tri_nrm : nullptr;
    rv.tris = s->d_tris; rv.nodes = s->d_nodes; rv.qnodes = s->d_qnodes; rv.wnodes = s->d_wnodes;
    return rv;
}

// The vertex-to-corner table of `shape` on the device, built at the first recompute of that shape from the face indices the device
// holds (the host copy was dropped at creation) and kept until the scene goes.
static int corner_table(mtsamd_scene *s, uint32_t shape, hipStream_t stream) {
    SceneGeometry &g = s->geometry;
    if (s->d_corner_offsets.empty()) { s->d_corner_offsets.assign(g.shapes.size(), nullptr); s->d_corners.assign(g.shapes.size(), nullptr); }
    if (!s->d_face_recs) {
        uint32_t max_faces = 1;
        for (uint32_t n : g.shape_faces) max_faces = std::max(max_faces, n);
        HIP_TRY(hipMalloc((void **) &s->d_face_recs, 6 * sizeof(float) * (size_t) max_faces));
    }
    if (s->d_corner_offsets[shape]) return MTSAMD_OK;
    const uint32_t n_faces = g.shape_faces[shape];
    std::vector<uint32_t> faces(3 * (size_t) n_faces), offsets, corners;
    if (n_faces) HIP_TRY(hipMemcpyAsync(faces.data(), s->d_faces + 3 * (size_t) g.shapes[shape].first_prim, faces.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    build_corner_table(g.shape_vertices[shape], n_faces, faces.data(), offsets, corners);
    uint32_t *d_offsets = nullptr, *d_corners = nullptr;
    if (int rc = upload(&d_offsets, offsets)) return rc;
    if (int rc = upload(&d_corners, corners)) { (void) hipFree(d_offsets); return rc; }
    s->d_corner_offsets[shape] = d_offsets; s->d_corners[shape] = d_corners;
    return MTSAMD_OK;
}

static int vertex_update(mtsamd_scene *s, uint32_t shape, const float *positions, const float *normals, uint32_t flags, float *normals_out, void *stream_) {
    if (!s) return fail(MTSAMD_ERR_INVALID, "null scene");
    if (int rc = check_vertex_flags(*s, shape, normals, flags)) return rc;       // MTSAMD_VERTICES_REBUILD_ACCEL: the caller's, after the update
    const bool recompute = (flags & MTSAMD_VERTICES_RECOMPUTE_NORMALS) != 0u;
    // with the flag the mesh has normals (check_vertex_flags) and the call computes them: what is left to check is the shape and the positions
    if (int rc = check_vertex_update(*s, shape, positions, recompute ? positions : normals)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t) stream_;
    SceneGeometry &g = s->geometry;
    if (g.flat) return flat_vertex_update(s, shape, positions, normals, recompute, normals_out, stream);
    const uint32_t nv = 3u * g.shape_vertices[shape], off = g.shapes[shape].first_prim, n_faces = g.shape_faces[shape];
    const int32_t em = g.shapes[shape].emitter;
    const RefitView rv = refit_view(s);
    if (recompute)
        if (int rc = corner_table(s, shape, stream)) return rc;
    // 1. stage the arrays (host or device pointers alike) and look before writing: finite coordinates, and the areas of an emitter shape
    HIP_TRY(hipMemcpyAsync(s->d_stage_pos, positions, nv * sizeof(float), hipMemcpyDefault, stream));
    if (normals) HIP_TRY(hipMemcpyAsync(s->d_stage_nrm, normals, nv * sizeof(float), hipMemcpyDefault, stream));
    HIP_TRY(hipMemsetAsync(s->d_refit_flag, 0, sizeof(uint32_t), stream));
    HIP_TRY(launch_refit_check(rv, s->d_stage_pos, nv, off, n_faces, em >= 0 ? s->d_stage_area : nullptr, s->d_refit_flag, stream));
    uint32_t flag = 0;
    std::vector<float> pmf(em >= 0 ? n_faces : 0), cdf(pmf.size()), em_pos(em >= 0 ? nv : 0);
    HIP_TRY(hipMemcpyAsync(&flag, s->d_refit_flag, sizeof(flag), hipMemcpyDeviceToHost, stream));
    if (em >= 0 && n_faces) HIP_TRY(hipMemcpyAsync(pmf.data(), s->d_stage_area, n_faces * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (em >= 0 && nv) HIP_TRY(hipMemcpyAsync(em_pos.data(), s->d_stage_pos, nv * sizeof(float), hipMemcpyDeviceToHost, stream));      // an emitter's vertices: its box (fated.h)
    HIP_TRY(hipStreamSynchronize(stream));
    if (flag) return fail(MTSAMD_ERR_INVALID, "shape %u: a vertex has a non-finite coordinate", shape);
    DevEmitter e{};
    if (em >= 0) {       // the cdf is a sequential double sum: the host's, not a scan that rounds differently
        e = s->emitters[em];
        if (int rc = area_distribution(pmf.data(), n_faces, cdf.data(), e)) return rc;
        emitter_exact_box(em_pos.data(), nv / 3u, e);      // over every vertex of the mesh: at least its triangles; padded by set_scene_bounds
    }
    // the normals of the staged positions into the staging buffer the gather reads: after the refusals, before the commit
    if (recompute) {
        HIP_TRY(launch_refit_normals(rv, s->d_stage_pos, off, n_faces, g.shape_vertices[shape], s->d_corner_offsets[shape], s->d_corners[shape],
                                     s->d_face_recs, s->d_stage_nrm, stream));
        if (normals_out) HIP_TRY(hipMemcpyAsync(normals_out, s->d_stage_nrm, nv * sizeof(float), hipMemcpyDefault, stream));
    }
    // 2. commit: primitives and slots of the shape, then every box from the leaves up, one launch per height class
    HIP_TRY(launch_refit_gather(rv, s->d_stage_pos, normals || recompute ? s->d_stage_nrm : nullptr, off, n_faces, stream));
    for (size_t h = 0; h + 1 < s->class_start.size(); ++h)
        HIP_TRY(launch_refit_boxes(rv, s->class_start[h], s->class_start[h + 1] - s->class_start[h], h == 0, stream));
    // 3. the scene box: the root's.  Extent, grid, bounding sphere and the records that hold it are the host's arithmetic.
    HIP_TRY(hipMemcpyAsync(s->bvh.bbox, s->d_boxes + 6 * (size_t) s->refit_root, 6 * sizeof(float), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    RefitGrid grid{};
    scene_grid(s->bvh.bbox, &grid.extent, s->bvh.q_lo, s->bvh.q_step);
    for (int k = 0; k < 3; ++k) {
        grid.glo[k] = (double) s->bvh.q_lo[k]; grid.gstep[k] = (double) s->bvh.q_step[k];
        s->view.q_lo[k] = s->bvh.q_lo[k]; s->view.q_step[k] = s->bvh.q_step[k]; s->view.q_inv_step[k] = 1.0f / s->bvh.q_step[k];
    }
    if (em >= 0) s->emitters[em] = e;
    set_scene_bounds(*s);
    // 4. emit the node arrays, push the emitter tables
    HIP_TRY(launch_refit_emit(rv, grid, stream));
    if (em >= 0 && n_faces) {
        HIP_TRY(hipMemcpyAsync(s->d_area_pmf + off, pmf.data(), n_faces * sizeof(float), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(s->d_area_cdf + off, cdf.data(), n_faces * sizeof(float), hipMemcpyHostToDevice, stream));
    }
    if (!s->emitters.empty()) HIP_TRY(hipMemcpyAsync(s->d_emitters, s->emitters.data(), s->emitters.size() * sizeof(DevEmitter), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return MTSAMD_OK;
}

int mtsamd_scene_set_vertex_positions(mtsamd_scene *s, uint32_t shape, const float *positions, const float *normals, void *stream) {
    return vertex_update(s, shape, positions, normals, 0u, nullptr, stream);
}

// ---- accelerator rebuild ---------------------------------------------------------------------------------------------------------------
static LbvhTarget live_target(const mtsamd_scene *s) {
    LbvhTarget t{};
    t.prim_slot = s->d_prim_slot; t.slot_prim = s->d_slot_prim; t.order = s->d_order; t.kids = s->d_kids; t.node_child = s->d_node_child;
    t.wide_child = s->d_wide_child; t.boxes = s->d_boxes; t.tris = s->d_tris; t.nodes = s->d_nodes; t.qnodes = s->d_qnodes; t.wnodes = s->d_wnodes;
    return t;
}

static int alloc_target(uint32_t n, LbvhTarget &t) {       // the worst case of n primitives (lbvh.h)
    const size_t nb = 2 * (size_t) n - 1, ni = std::max<size_t>(n - 1, 1);
    t = LbvhTarget{};
    auto get = [](auto **p, size_t count) { return hipMalloc((void **) p, sizeof(**p) * count); };
    hipError_t e = hipSuccess;
    auto ok = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    ok(get(&t.prim_slot, n)); ok(get(&t.slot_prim, n)); ok(get(&t.order, nb)); ok(get(&t.kids, nb)); ok(get(&t.node_child, 2 * ni)); ok(get(&t.wide_child, 4 * ni));
    ok(get(&t.boxes, 6 * nb)); ok(get(&t.tris, 3 * (size_t) n)); ok(get(&t.nodes, 4 * ni)); ok(get(&t.qnodes, 2 * ni)); ok(get(&t.wnodes, 4 * ni));
    if (e == hipSuccess) return MTSAMD_OK;
    (void) hipGetLastError();
    free_target(t);
    return fail(MTSAMD_ERR_NOMEM, "accelerator rebuild: out of device memory (%u primitives)", n);
}

// The device build (lbvh.h, or sah_build.h: creation's tree) from the positions the scene holds, into the spare set; then look before writing: the tree must fit the
// traversal stack and the spill area must be there before a single pointer of the scene changes.
static int rebuild_accel(mtsamd_scene *s, uint32_t builder, hipStream_t stream) {
    HIP_TRY(hipSetDevice(s->device));
    if (s->geometry.flat || s->n_prims == 0) return MTSAMD_OK;
    const uint32_t n = s->n_prims;
    HIP_TRY(hipStreamSynchronize(stream));
    if (!s->lbvh_scratch) {
        const hipError_t e = lbvh_scratch_create(n, &s->lbvh_scratch);
        if (e == hipErrorOutOfMemory) { (void) hipGetLastError(); return fail(MTSAMD_ERR_NOMEM, "accelerator rebuild: out of device memory (%u primitives)", n); }
        HIP_TRY(e);
    }
    if (builder == MTSAMD_BUILDER_SAH && !s->sah_scratch) {
        const hipError_t e = sah_scratch_create(n, &s->sah_scratch);
        if (e == hipErrorOutOfMemory) { (void) hipGetLastError(); return fail(MTSAMD_ERR_NOMEM, "accelerator rebuild: out of device memory (%u primitives)", n); }
        HIP_TRY(e);
    }
    if (!s->spare.kids)
        if (int rc = alloc_target(n, s->spare)) return rc;
    RefitGrid grid{};
    float q_lo[3], q_step[3];
    scene_grid(s->bvh.bbox, &grid.extent, q_lo, q_step);          // the box is unchanged by a rebuild, and so is the grid
    for (int k = 0; k < 3; ++k) { grid.glo[k] = (double) q_lo[k]; grid.gstep[k] = (double) q_step[k]; }
    LbvhResult r;
    if (builder == MTSAMD_BUILDER_SAH) HIP_TRY(sah_build(s->sah_scratch, s->lbvh_scratch, s->d_tri_pos, n, s->options.max_leaf, grid, s->spare, r, stream));
    else HIP_TRY(lbvh_build(s->lbvh_scratch, s->d_tri_pos, n, s->options.max_leaf, s->bvh.bbox, grid, s->spare, r, stream));
    SceneView &v = s->view;
    const uint32_t stack_depth = bvh_stack_depth(r.depth, r.wdepth, MTS_BVH4 != 0);
    if (!bvh_stack_fits(stack_depth, sizeof(StackEntry))) return fail(MTSAMD_ERR_UNSUPPORTED, "BVH too deep for the LDS traversal stack (depth %u)", stack_depth);
    const uint32_t walk_lds_depth = std::min<uint32_t>(stack_depth, MTS_BVH4 ? 8u : 16u);
    const size_t entries = stack_depth > walk_lds_depth ? (size_t) v.walk_blocks * (stack_depth - walk_lds_depth) * 256u : 0u;
    StackEntry *spill = nullptr;
    if (entries > s->walk_spill_entries)
        if (ws_alloc((void **) &spill, entries * sizeof(StackEntry))) return fail(MTSAMD_ERR_NOMEM, "traversal spill area");
    // accepted: swap
    LbvhTarget old = live_target(s);
    const LbvhTarget &t = s->spare;
    s->d_prim_slot = t.prim_slot; s->d_slot_prim = t.slot_prim; s->d_order = t.order; s->d_kids = t.kids; s->d_node_child = t.node_child;
    s->d_wide_child = t.wide_child; s->d_boxes = t.boxes; s->d_tris = t.tris; s->d_nodes = t.nodes; s->d_qnodes = t.qnodes; s->d_wnodes = t.wnodes;
    if (s->accel_worst_case) s->spare = old;
    else { free_target(old); s->spare = LbvhTarget{}; s->accel_worst_case = true; }
    if (spill) { (void) hipFree(s->d_walk_spill); s->d_walk_spill = spill; s->walk_spill_entries = entries; }
    BvhOutput &b = s->bvh;
    b.n_nodes = r.n_nodes; b.n_wnodes = r.n_wide; b.n_slots = r.n_slots; b.depth = r.depth; b.wdepth = r.wdepth; b.root = r.root; b.wroot = r.wroot;
    s->class_start = r.class_start; s->refit_root = 0; s->n_builder = r.n_builder;
    v.nodes = s->d_nodes; v.qnodes = s->d_qnodes; v.wnodes = s->d_wnodes; v.tris = s->d_tris; v.root = b.root; v.wroot = b.wroot;
    v.n_nodes = b.n_nodes; v.n_wnodes = b.n_wnodes; v.n_slots = b.n_slots;
    v.stack_depth = stack_depth; v.walk_lds_depth = walk_lds_depth; v.walk_spill = s->d_walk_spill;
    s->builder = builder; ++s->rebuilds;
    return MTSAMD_OK;
}

int mtsamd_scene_update_vertices(mtsamd_scene *s, uint32_t shape, const float *positions, const float *normals, uint32_t flags, float *normals_out,
                                 void *stream) {
    if (int rc = vertex_update(s, shape, positions, normals, flags, normals_out, stream)) return rc;
    if (flags & MTSAMD_VERTICES_REBUILD_ACCEL) return rebuild_accel(s, (flags & MTSAMD_VERTICES_ACCEL_SAH) ? MTSAMD_BUILDER_SAH : MTSAMD_BUILDER_LBVH, (hipStream_t) stream);
    return MTSAMD_OK;
}

int mtsamd_scene_rebuild_accel(mtsamd_scene *s, uint32_t flags, void *stream) {
    if (!s) return fail(MTSAMD_ERR_INVALID, "null scene");
    if (flags) return fail(MTSAMD_ERR_INVALID, "unknown accelerator rebuild flags 0x%x", flags);
    return rebuild_accel(s, MTSAMD_BUILDER_LBVH, (hipStream_t) stream);
}

int mtsamd_scene_rebuild_accel_with(mtsamd_scene *s, uint32_t builder, uint32_t flags, void *stream) {
    if (!s) return fail(MTSAMD_ERR_INVALID, "null scene");
    if (builder != MTSAMD_BUILDER_SAH && builder != MTSAMD_BUILDER_LBVH) return fail(MTSAMD_ERR_INVALID, "unknown accelerator builder %u", builder);
    if (flags) return fail(MTSAMD_ERR_INVALID, "unknown accelerator rebuild flags 0x%x", flags);
    return rebuild_accel(s, builder, (hipStream_t) stream);
}

int mtsamd_scene_rebuild_levels(const mtsamd_scene *s, uint32_t capacity, uint32_t *nodes, float *ms, uint32_t *levels) {
    if (!s || !levels || (capacity && (!nodes || !ms))) return fail(MTSAMD_ERR_INVALID, "null argument");
    *levels = 0;
    if (!s->sah_scratch) return MTSAMD_OK;
    const std::vector<float> &t = sah_level_ms(s->sah_scratch);
    const std::vector<uint32_t> &m = sah_level_nodes(s->sah_scratch);
    *levels = (uint32_t) t.size();
    for (size_t i = 0; i < t.size() && i < capacity; ++i) { nodes[i] = m[i]; ms[i] = t[i]; }
    return MTSAMD_OK;
}

int mtsamd_scene_accel_info(const mtsamd_scene *s_, uint32_t *out8, double *sah_cost) {
    if (!s_ || !out8) return fail(MTSAMD_ERR_INVALID, "null argument");
    mtsamd_scene *s = const_cast<mtsamd_scene *>(s_);          // the scratch of the sum is the scene's
    out8[0] = s->bvh.n_nodes; out8[1] = s->bvh.n_wnodes; out8[2] = s->bvh.n_slots; out8[3] = s->bvh.depth; out8[4] = s->bvh.wdepth;
    out8[5] = s->view.stack_depth; out8[6] = s->builder; out8[7] = s->rebuilds;
    if (!sah_cost) return MTSAMD_OK;
    *sah_cost = 0.0;
    if (s->geometry.flat || s->n_prims == 0 || s->n_builder == 0) return MTSAMD_OK;
    HIP_TRY(hipSetDevice(s->device));
    const size_t blocks = ((size_t) s->n_builder + kSahBlock - 1) / kSahBlock;
    if (blocks > s->sah_partial_cap) {
        (void) hipFree(s->d_sah_partial); s->d_sah_partial = nullptr; s->sah_partial_cap = 0;
        HIP_TRY(hipMalloc((void **) &s->d_sah_partial, blocks * sizeof(double)));
        s->sah_partial_cap = blocks;
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(launch_sah_partials(s->d_kids, s->d_boxes, s->n_builder, s->refit_root, s->d_sah_partial, nullptr));
    std::vector<double> partial(blocks);
    HIP_TRY(hipMemcpy(partial.data(), s->d_sah_partial, blocks * sizeof(double), hipMemcpyDeviceToHost));
    double total = 0.0;
    for (double p : partial) total += p;
    *sah_cost = total;
    return MTSAMD_OK;
}

int mtsamd_compute_vertex_normals(uint32_t vertex_count, const float *positions, uint32_t face_count, const uint32_t *faces, float *normals_out) {
    if ((vertex_count && (!positions || !normals_out)) || (face_count && !faces)) return fail(MTSAMD_ERR_INVALID, "null argument");
    for (size_t c = 0; c < 3 * (size_t) face_count; ++c)
        if (faces[c] >= vertex_count) return fail(MTSAMD_ERR_INVALID, "face %u: vertex index %u out of range (%u vertices)", (uint32_t) (c / 3), faces[c], vertex_count);
    compute_vertex_normals(vertex_count, positions, face_count, faces, normals_out);
    return MTSAMD_OK;
}

int mtsamd_scene_read_accel(const mtsamd_scene *s, int32_t which, void *host_dst, uint64_t bytes) {
    if (!s || !host_dst) return fail(MTSAMD_ERR_INVALID, "null argument");
    const void *src = nullptr; uint64_t size = 0;
    float grid[6];
    switch (which) {
    case MTSAMD_ACCEL_NODES: src = s->d_nodes; size = 64ull * s->bvh.n_nodes; break;
    case MTSAMD_ACCEL_QNODES: src = s->d_qnodes; size = 32ull * s->bvh.n_nodes; break;
    case MTSAMD_ACCEL_WNODES: src = s->d_wnodes; size = 64ull * s->bvh.n_wnodes; break;
    case MTSAMD_ACCEL_TRIS: src = s->d_tris; size = 48ull * s->bvh.n_slots; break;
    case MTSAMD_ACCEL_TRI_POS: src = s->d_tri_pos; size = 36ull * s->n_prims; break;
    case MTSAMD_ACCEL_TRI_NRM: src = s->d_tri_nrm; size = 4ull * s->n_tri_nrm; break;
    case MTSAMD_ACCEL_AREA_PMF: src = s->d_area_pmf; size = 4ull * s->n_prims; break;
    case MTSAMD_ACCEL_AREA_CDF: src = s->d_area_cdf; size = 4ull * s->n_prims; break;
    case MTSAMD_ACCEL_GRID: size = 24; break;
    case MTSAMD_ACCEL_KIDS: src = s->d_kids; size = 8ull * s->n_builder; break;
    case MTSAMD_ACCEL_ORDER: src = s->d_order; size = 4ull * s->n_builder; break;
    case MTSAMD_ACCEL_NODE_CHILD: src = s->d_node_child; size = 8ull * s->bvh.n_nodes; break;
    case MTSAMD_ACCEL_WIDE_CHILD: src = s->d_wide_child; size = 16ull * s->bvh.n_wnodes; break;
    case MTSAMD_ACCEL_BOXES: src = s->d_boxes; size = 24ull * s->n_builder; break;
    case MTSAMD_ACCEL_SLOT_PRIM: src = s->d_slot_prim; size = 4ull * (s->n_builder ? s->bvh.n_slots : 0u); break;
    default: return fail(MTSAMD_ERR_INVALID, "mtsamd_scene_read_accel: unknown array %d", which);
    }
    if (bytes != size) return fail(MTSAMD_ERR_INVALID, "mtsamd_scene_read_accel: array %d holds %llu bytes, not %llu", which, (unsigned long long) size, (unsigned long long) bytes);
    if (which == MTSAMD_ACCEL_GRID) {
        for (int k = 0; k < 3; ++k) { grid[k] = s->view.q_lo[k]; grid[3 + k] = s->view.q_step[k]; }
        std::memcpy(host_dst, grid, sizeof(grid));
        return MTSAMD_OK;
    }
    if (size == 0) return MTSAMD_OK;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(host_dst, src, size, hipMemcpyDeviceToHost));
    return MTSAMD_OK;
}

// ---- scene queries -------------------------------------------------------------------------
static int check_rays(const mtsamd_scene *s, const mtsamd_rays *r, uint64_t n) {
    if (!s || !r) return fail(MTSAMD_ERR_INVALID, "null argument");
    if (n == 0) return 1;               // empty ray stream: nothing to do (pointers may be null)
    if (!r->ox || !r->oy || !r->oz || !r->dx || !r->dy || !r->dz || !r->mint || !r->maxt)
        return fail(MTSAMD_ERR_INVALID, "ray stream has a null component");
    return 0;
}
static RayStreams to_streams(const mtsamd_rays *r) {
    return RayStreams{ r->ox, r->oy, r->oz, r->dx, r->dy, r->dz, r->mint, r->maxt, r->active };
}

int mtsamd_ray_intersect(const mtsamd_scene *s, uint64_t n, const mtsamd_rays *rays, float *t, uint32_t *prim,
                         uint32_t *shape, float *u, float *v, void *stream) {
    if (int rc = check_rays(s, rays, n)) return rc > 0 ? MTSAMD_OK : rc;
    if (!t || !prim) return fail(MTSAMD_ERR_INVALID, "t and prim outputs are required");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch_ray_intersect(s->view, n, to_streams(rays), 0, t, prim, shape, u, v, nullptr, (hipStream_t) stream));
    return MTSAMD_OK;
}

int mtsamd_ray_intersect_naive(const mtsamd_scene *s, uint64_t n, const mtsamd_rays *rays, float *t, uint32_t *prim,
                               uint32_t *shape, float *u, float *v, void *stream) {
    if (int rc = check_rays(s, rays, n)) return rc > 0 ? MTSAMD_OK : rc;
    if (!t || !prim) return fail(MTSAMD_ERR_INVALID, "t and prim outputs are required");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch_ray_intersect(s->view, n, to_streams(rays), 1, t, prim, shape, u, v, nullptr, (hipStream_t) stream));
    return MTSAMD_OK;
}

int mtsamd_ray_intersect_si(const mtsamd_scene *s, uint64_t n, const mtsamd_rays *rays, float *t, uint32_t *prim,
                            uint32_t *shape, float *si26, void *stream) {
    if (int rc = check_rays(s, rays, n)) return rc > 0 ? MTSAMD_OK : rc;
    if (!t || !prim || !si26) return fail(MTSAMD_ERR_INVALID, "t, prim and si26 outputs are required");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch_ray_intersect(s->view, n, to_streams(rays), 0, t, prim, shape, nullptr, nullptr, si26, (hipStream_t) stream));
    return MTSAMD_OK;
}

int mtsamd_ray_test(const mtsamd_scene *s, uint64_t n, const mtsamd_rays *rays, uint8_t *hit, void *stream) {
    if (int rc = check_rays(s, rays, n)) return rc > 0 ? MTSAMD_OK : rc;
    if (!hit) return fail(MTSAMD_ERR_INVALID, "hit output is required");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch_ray_test(s->view, n, to_streams(rays), hit, (hipStream_t) stream));
    return MTSAMD_OK;
}

// ---- operator API on device streams ------------------------------------------------------------
// what the host can check: 1 = nothing to do (n == 0), 0 = go on, < 0 = refused
static int check_operator(const mtsamd_scene *s, uint64_t n, const char *what) {
    if (!s) return fail(MTSAMD_ERR_INVALID, "%s: null scene", what);
    if (s->spectral) return fail(MTSAMD_ERR_UNSUPPORTED, "%s: the operator API is implemented for the RGB variant only", what);
    return n == 0 ? 1 : 0;
}

static int bsdf_operator(const mtsamd_scene *s, uint64_t n, const mtsamd_bsdf_query *q, float *out, bool sample, void *stream) {
    const char *what = sample ? "mtsamd_bsdf_sample" : "mtsamd_bsdf_eval_pdf";
    if (int rc = check_operator(s, n, what)) return rc > 0 ? MTSAMD_OK : rc;
    if (!q || !out || !q->shape || !q->wi_x || !q->wi_y || !q->wi_z || (q->u == nullptr) != (q->v == nullptr))
        return fail(MTSAMD_ERR_INVALID, "%s: null argument", what);
    if (sample ? (!q->sample1 || !q->sample2_x || !q->sample2_y) : (!q->wo_x || !q->wo_y || !q->wo_z))
        return fail(MTSAMD_ERR_INVALID, "%s: the query lacks %s", what, sample ? "sample1 / sample2" : "wo");
    const BsdfStreams b{ q->shape, q->wi_x, q->wi_y, q->wi_z, q->u, q->v, q->wo_x, q->wo_y, q->wo_z, q->sample1, q->sample2_x, q->sample2_y, q->active };
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(sample ? launch_bsdf_sample(s->view, n, b, out, (hipStream_t) stream) : launch_bsdf_eval_pdf(s->view, n, b, out, (hipStream_t) stream));
    return MTSAMD_OK;
}
int mtsamd_bsdf_eval_pdf(const mtsamd_scene *s, uint64_t n, const mtsamd_bsdf_query *q, float *out4, void *stream) {
    return bsdf_operator(s, n, q, out4, false, stream);
}
int mtsamd_bsdf_sample(const mtsamd_scene *s, uint64_t n, const mtsamd_bsdf_query *q, float *out10, void *stream) {
    return bsdf_operator(s, n, q, out10, true, stream);
}

int mtsamd_sample_emitter_direction(const mtsamd_scene *s, uint64_t n, const float *ref_p3, const float *sample2, const uint8_t *active,
                                    float *out15, uint32_t *emitter, void *stream) {
    if (int rc = check_operator(s, n, "mtsamd_sample_emitter_direction")) return rc > 0 ? MTSAMD_OK : rc;
    if (!ref_p3 || !sample2 || !out15 || !emitter) return fail(MTSAMD_ERR_INVALID, "mtsamd_sample_emitter_direction: null argument");
    const EmitterSampleStreams q{ ref_p3, ref_p3 + n, ref_p3 + 2 * n, sample2, sample2 + n, active };
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch_sample_emitter_direction(s->view, n, q, out15, emitter, (hipStream_t) stream));      // no emitters: zeros, as the device function
    return MTSAMD_OK;
}

int mtsamd_pdf_emitter_direction(const mtsamd_scene *s, uint64_t n, const uint32_t *emitter, const float *d3, const float *n3, const float *dist,
                                 const uint8_t *delta, const uint8_t *active, float *pdf, void *stream) {
    if (int rc = check_operator(s, n, "mtsamd_pdf_emitter_direction")) return rc > 0 ? MTSAMD_OK : rc;
    if (!emitter || !d3 || !n3 || !dist || !pdf) return fail(MTSAMD_ERR_INVALID, "mtsamd_pdf_emitter_direction: null argument");
    const EmitterQueryStreams q{ emitter, d3, d3 + n, d3 + 2 * n, n3, n3 + n, n3 + 2 * n, dist, delta, active };
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch_pdf_emitter_direction(s->view, n, q, pdf, (hipStream_t) stream));
    return MTSAMD_OK;
}

int mtsamd_emitter_eval(const mtsamd_scene *s, uint64_t n, const uint32_t *emitter, const float *wi3, const float *d3, const uint8_t *active,
                        float *out3, void *stream) {
    if (int rc = check_operator(s, n, "mtsamd_emitter_eval")) return rc > 0 ? MTSAMD_OK : rc;
    if (!emitter || !wi3 || !d3 || !out3) return fail(MTSAMD_ERR_INVALID, "mtsamd_emitter_eval: null argument");
    const EmitterQueryStreams q{ emitter, d3, d3 + n, d3 + 2 * n, wi3, wi3 + n, wi3 + 2 * n, nullptr, nullptr, active };
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch_emitter_eval(s->view, n, q, out3, (hipStream_t) stream));
    return MTSAMD_OK;
}

int mtsamd_sampler_seed(uint64_t n, uint64_t first, uint64_t base_seed, uint64_t *state, uint64_t *inc, void *stream) {
    if (n && (!state || !inc)) return fail(MTSAMD_ERR_INVALID, "mtsamd_sampler_seed: null argument");
    HIP_TRY(launch_sampler_seed(n, first, base_seed, state, inc, (hipStream_t) stream));
    return MTSAMD_OK;
}

int mtsamd_sampler_next(uint64_t n, int32_t dims, uint64_t *state, const uint64_t *inc, const uint8_t *active, float *out, void *stream) {
    if (dims != 1 && dims != 2) return fail(MTSAMD_ERR_INVALID, "mtsamd_sampler_next: dims must be 1 or 2, not %d", dims);
    if (n && (!state || !inc || !out)) return fail(MTSAMD_ERR_INVALID, "mtsamd_sampler_next: null argument");
    HIP_TRY(launch_sampler_next(n, dims, state, inc, active, out, (hipStream_t) stream));
    return MTSAMD_OK;
}

// BSDFFlags of a record as far as the kernels distinguish them: Smooth (bsdf_is_smooth), Delta (a discrete lobe; mask's null lobe is one)
static int32_t bsdf_flag_word(const std::vector<DevBsdf> &table, const DevBsdf &b) {
    const auto smooth = [](const DevBsdf &r) {
        return r.type == kBsdfDiffuse || r.type == kBsdfRoughConductor || r.type == kBsdfPlastic || r.type == kBsdfRoughPlastic ||
               r.type == kBsdfRoughDielectric || (r.flags & kBsdfNestSmooth) != 0u;
    };
    const auto delta = [](const DevBsdf &r) {
        return r.type == kBsdfConductor || r.type == kBsdfDielectric || r.type == kBsdfThinDielectric || r.type == kBsdfPlastic || r.type == kBsdfMask;
    };
    int32_t w = (smooth(b) ? MTSAMD_BSDF_SMOOTH : 0) | (delta(b) ? MTSAMD_BSDF_DELTA : 0) | ((b.flags & kBsdfTwoSided) ? MTSAMD_BSDF_TWOSIDED : 0);
    if (b.type >= kBsdfBlend) {
        w |= MTSAMD_BSDF_NESTED;
        for (uint32_t c : { b.nested0, b.nested1 })
            if (c < table.size() && delta(table[c])) w |= MTSAMD_BSDF_DELTA;
    }
    return w;
}

int mtsamd_scene_shape_tables(const mtsamd_scene *s, int32_t *out3) {
    if (!s || !out3) return fail(MTSAMD_ERR_INVALID, "null argument");
    std::vector<DevShape> shapes(s->n_shapes);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(shapes.data(), s->d_shapes, shapes.size() * sizeof(DevShape), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < s->n_shapes; ++i) {
        const int32_t b = shapes[i].bsdf;
        out3[3 * i] = b;
        out3[3 * i + 1] = b >= 0 && (size_t) b < s->bsdfs.size() ? bsdf_flag_word(s->bsdfs, s->bsdfs[b]) : 0;
        out3[3 * i + 2] = shapes[i].emitter;
    }
    return MTSAMD_OK;
}

// ---- render ----------------------------------------------------------------------------------
static int check_desc(const mtsamd_render_desc *d) {
    if (!d) return fail(MTSAMD_ERR_INVALID, "null render descriptor");
    // MonteCarloIntegrator (integrator.cpp:288-295)
    if (d->max_depth < 0 && d->max_depth != -1)
        return fail(MTSAMD_ERR_INVALID, "\"max_depth\" must be set to -1 (infinite) or a value >= 0");
    if (d->rr_depth <= 0) return fail(MTSAMD_ERR_INVALID, "\"rr_depth\" must be set to a value greater than zero!");
    if (d->film_width <= 0 || d->film_height <= 0 || d->crop_width <= 0 || d->crop_height <= 0 || d->crop_x < 0 || d->crop_y < 0 ||
        d->crop_x + d->crop_width > d->film_width || d->crop_y + d->crop_height > d->film_height)
        return fail(MTSAMD_ERR_INVALID, "Invalid crop window specification!");      // film.cpp:24-32
    if (d->sample_count <= 0) return fail(MTSAMD_ERR_INVALID, "sample_count must be positive");
    if (d->samples_per_pass > 0 && d->sample_count % std::min(d->samples_per_pass, d->sample_count) != 0)      // integrator.cpp:59-66
        return fail(MTSAMD_ERR_INVALID, "sample_count (%d) must be a multiple of samples_per_pass (%d).", d->sample_count,
                    std::min(d->samples_per_pass, d->sample_count));
    if (d->integrator < 0 || d->integrator > 2) return fail(MTSAMD_ERR_UNSUPPORTED, "integrator %d is not implemented (0 path, 1 direct, 2 depth)", d->integrator);
    if (d->emitter_samples < 0 || d->bsdf_samples < 0) return fail(MTSAMD_ERR_INVALID, "Must have at least 1 BSDF or emitter sample!");
    if (d->pipeline < 0 || d->pipeline > 4) return fail(MTSAMD_ERR_UNSUPPORTED, "pipeline %d is not available in this build", d->pipeline);
    return 0;
}

static int ensure_workspace(mtsamd_scene *s, uint32_t n_waves, uint32_t seg_cap, uint64_t pass_cap, bool split) {
    Workspace &w = s->ws;
    if (w.n_waves == n_waves && w.seg_cap == seg_cap && w.pass_cap >= pass_cap && w.spectral == s->spectral && (w.split || !split)) return 0;
    w.release();
    struct Guard { Workspace &w; bool ok = false; ~Guard() { if (!ok) w.release(); } } guard{ w };      // nothing half-allocated survives an error
    size_t slots = (size_t) n_waves * seg_cap;
    for (int k = 0; k < 2; ++k) {
        if (int rc = ws_alloc((void **) &w.pool[k].ray_o, slots * sizeof(float4))) return rc;
        if (int rc = ws_alloc((void **) &w.pool[k].ray_d, slots * sizeof(float4))) return rc;
        if (int rc = ws_alloc((void **) &w.pool[k].thr, slots * sizeof(float4))) return rc;
        if (int rc = ws_alloc((void **) &w.pool[k].res, slots * sizeof(float4))) return rc;
        if (int rc = ws_alloc((void **) &w.pool[k].rng, slots * sizeof(uint4))) return rc;
        if (int rc = ws_alloc((void **) &w.pool[k].misc, slots * sizeof(uint2))) return rc;
        if (int rc = ws_alloc((void **) &w.count[k], 2 * (size_t) n_waves * sizeof(uint32_t))) return rc;      // counts + survivor borders (k_shade, flat scenes)
        if (s->spectral) {
            if (int rc = ws_alloc((void **) &w.pool[k].xi, slots * sizeof(float))) return rc;
            if (int rc = ws_alloc((void **) &w.pool[k].aux, slots * sizeof(float2))) return rc;
        }
        if (split) {
            if (int rc = ws_alloc((void **) &w.pool[k].hit, slots * sizeof(float4))) return rc;
            if (int rc = ws_alloc((void **) &w.pool[k].sh_o, slots * sizeof(float4))) return rc;
            if (int rc = ws_alloc((void **) &w.pool[k].sh_d, slots * sizeof(float4))) return rc;
            if (int rc = ws_alloc((void **) &w.pool[k].nee, slots * sizeof(float4))) return rc;
            if (int rc = ws_alloc((void **) &w.pool[k].sh_slot, slots * sizeof(uint32_t))) return rc;
        }
    }
    if (int rc = ws_alloc((void **) &w.cursor, n_waves * sizeof(uint64_t))) return rc;
    if (int rc = ws_alloc((void **) &w.cursor_end, n_waves * sizeof(uint64_t))) return rc;
    if (int rc = ws_alloc((void **) &w.wave_stats, 4 * (size_t) n_waves * sizeof(uint64_t))) return rc;
    if (int rc = ws_alloc((void **) &w.count_shadow, n_waves * sizeof(uint32_t))) return rc;
    if (int rc = ws_alloc((void **) &w.out_rgba, pass_cap * sizeof(float4))) return rc;
    if (int rc = ws_alloc((void **) &w.out_pos, pass_cap * sizeof(float2))) return rc;
    HIP_TRY(hipHostMalloc((void **) &w.h_counts, 4 * (size_t) n_waves * sizeof(uint32_t), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void **) &w.h_cursor, 3 * (size_t) n_waves * sizeof(uint64_t), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void **) &w.h_cursor_rb, 2 * (size_t) n_waves * sizeof(uint64_t), hipHostMallocDefault));
    for (auto &e : w.ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (!w.stream2) HIP_TRY(hipStreamCreateWithFlags(&w.stream2, hipStreamNonBlocking));
    for (auto &ps : w.part_stream) if (!ps) HIP_TRY(hipStreamCreateWithFlags(&ps, hipStreamNonBlocking));
    for (auto &pe : w.part_ev) if (!pe) HIP_TRY(hipEventCreateWithFlags(&pe, hipEventDisableTiming));
    for (uint32_t k = 0; k < kMaxChains; ++k) {
        if (k > 0 && !w.chain_main[k]) HIP_TRY(hipStreamCreateWithFlags(&w.chain_main[k], hipStreamNonBlocking));
        if (!w.chain_any[k]) HIP_TRY(hipStreamCreateWithFlags(&w.chain_any[k], hipStreamNonBlocking));
    }
    for (auto &pe : w.chain_ev) if (!pe) HIP_TRY(hipEventCreateWithFlags(&pe, hipEventDisableTiming));
    if (!w.film_stream) HIP_TRY(hipStreamCreateWithFlags(&w.film_stream, hipStreamNonBlocking));      // renders of several passes: the splat of a pass ...
    for (auto &e : w.film_done) if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));      // ... beside the tracing of the next
    for (auto &e : w.tev) HIP_TRY(hipEventCreate(&e));
    w.have_events = true;
    w.n_waves = n_waves; w.seg_cap = seg_cap; w.pass_cap = pass_cap; w.spectral = s->spectral; w.split = split;
    guard.ok = true;
    return 0;
}

} // extern "C"

// ---- render jobs: C++ (templates, an anonymous namespace); the C ABI resumes at mtsamd_render ----
namespace {
struct Job {
    mtsamd_scene *s; const mtsamd_render_desc *d; hipStream_t stream;
    CameraView cam; FilterView filter;
    JobShape shape; uint64_t pass_cap;       // the plan of the job (schedule.h) and the samples a pass holds
    uint64_t iterations = 0;
    double bounce_ms = 0.0, film_ms = 0.0;
    RowMap rows{};
    int store_xyz = 1;
    uint32_t plane_pix0 = 0, plane_pixels = 0;
    // film renders (open_render): samples of one local row, the local sample ordinals [0, total) of the call, its passes of whole rows
    uint64_t per_row = 0, total = 0; FilmPasses fp{};
    struct Pass { uint64_t lr0, nrows, a, n; };      // the local rows [lr0, lr0 + nrows) hold the local sample ordinals [a, a + n)
    Pass pass(uint64_t lr0) {          // the pass that starts at local row lr0; its sample stream is pixel-major from that row's first pixel on
        const uint64_t nrows = std::min<uint64_t>(fp.rows_per_pass, (uint64_t) rows.local_rows - lr0);
        plane_pix0 = (uint32_t) (lr0 * (uint64_t) d->crop_width); plane_pixels = 0u;
        return Pass{ lr0, nrows, lr0 * per_row, nrows * per_row };
    }
    double stage_ms[3] = { 0.0, 0.0, 0.0 }; uint64_t stage_launches[3] = { 0, 0, 0 };      // desc->profile: k_trace<closest>, k_shade, k_trace<any>
    uint64_t passes = 0;
    int buf = 0;                 // sample stream buffer this pass writes
    std::chrono::steady_clock::time_point t_start;       // m_render_timer (integrator.cpp:107)
    bool timed_out = false;
    bool expired() const {                               // should_stop() without m_stop (integrator.h:143-146)
        return d->timeout > 0.0f && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() > (double) d->timeout;
    }
};

// The timed bracket of a pass: `body` issues the pass on j.stream between two events; once the second has completed, the time between
// them is added to bounce_ms.  A body that fails or stops (rc != 0) leaves the bracket open.
template <typename F> int timed(Job &j, F &&body) {
    Workspace &w = j.s->ws;
    HIP_TRY(hipEventRecord(w.tev[0], j.stream));
    if (int rc = body()) return rc;
    HIP_TRY(hipEventRecord(w.tev[1], j.stream));
    HIP_TRY(hipEventSynchronize(w.tev[1]));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, w.tev[0], w.tev[1]));
    j.bounce_ms += ms;
    return 0;
}

// desc->profile: begin / end timing events around the launches of the split pipeline, each on the stream of its launch
struct StageProfile {
    Workspace &w;
    bool on;
    struct Rec { int stage; size_t e0; };
    std::vector<Rec> recs;
    size_t used = 0;
    hipError_t err = hipSuccess;
    size_t mark(hipStream_t st) {
        if (used == w.prof_ev.size()) {
            hipEvent_t e = nullptr;
            const hipError_t rc = hipEventCreate(&e);
            if (rc != hipSuccess) { err = rc; return 0; }
            w.prof_ev.push_back(e);
        }
        const hipError_t rc = hipEventRecord(w.prof_ev[used], st);
        if (rc != hipSuccess) err = rc;
        return used++;
    }
};

// The launch rounds of a pass: every round advances each path of the pool by one segment, over the wave ranges and streams the plan
// names, until the drain state (schedule.h) finds the pool empty or hands what is left to k_finish.  1: the timeout stopped the pass.
int launch_rounds(Job &j, RenderParams &p, const PassPlan &plan, StageProfile &prof) {
    Workspace &w = j.s->ws;
    const uint32_t nw = j.shape.n_waves, n_parts = plan.n_parts, split_parts = plan.split_parts;
    Drain drain(j.shape, plan);
    uint64_t it = 0;
    int cur = 0, pending = -1, slot = 0;
    bool finish = false;
    auto chain_main = [&](uint32_t k) { return k == 0 ? j.stream : w.chain_main[k]; };
    if (split_parts > 1) {       // the other chains start after the cursors and counts are in place
        HIP_TRY(hipEventRecord(w.part_ev[2], j.stream));
        for (uint32_t k = 1; k < split_parts; ++k) HIP_TRY(hipStreamWaitEvent(chain_main(k), w.part_ev[2], 0));
    }
    auto join_chains = [&]() -> int {        // j.stream waits for what the other chains' main streams hold (their k_shade writes their counts)
        for (uint32_t k = 1; k < split_parts; ++k) {
            HIP_TRY(hipEventRecord(w.chain_ev[2 * k], chain_main(k)));
            HIP_TRY(hipStreamWaitEvent(j.stream, w.chain_ev[2 * k], 0));
        }
        return 0;
    };
    auto split_stage = [&](const RenderParams &h, int stage, hipStream_t st) -> int {
        const size_t pe = prof.on ? prof.mark(st) : 0;
        HIP_TRY(launch_split_stage(h, stage, st));
        if (prof.on) { prof.mark(st); prof.recs.push_back({ stage, pe }); }
        return 0;
    };
    auto sync_all = [&]() {
        (void) hipStreamSynchronize(j.stream);
        if (w.film_stream) (void) hipStreamSynchronize(w.film_stream);
        if (w.stream2) (void) hipStreamSynchronize(w.stream2);
        for (auto &ps : w.part_stream) if (ps) (void) hipStreamSynchronize(ps);
        for (auto &ps : w.chain_main) if (ps) (void) hipStreamSynchronize(ps);
        for (auto &ps : w.chain_any) if (ps) (void) hipStreamSynchronize(ps);
    };
    auto join_parts = [&]() -> int {         // j.stream waits for the other parts' streams
        for (uint32_t k = 1; k < n_parts; ++k) {
            HIP_TRY(hipEventRecord(w.part_ev[k - 1], w.part_stream[k - 1]));
            HIP_TRY(hipStreamWaitEvent(j.stream, w.part_ev[k - 1], 0));
        }
        return 0;
    };
    if (n_parts > 1) {          // the other streams start after the cursors and counts are in place
        HIP_TRY(hipEventRecord(w.ev[2], j.stream));
        for (uint32_t k = 1; k < n_parts; ++k) HIP_TRY(hipStreamWaitEvent(w.part_stream[k - 1], w.ev[2], 0));
    }
    while (true) {
        if (j.s->cancel.load(std::memory_order_relaxed)) {
            sync_all();
            return fail(MTSAMD_ERR_CANCELLED, "render cancelled");
        }
        if (j.expired()) {                   // timeout: this pass is abandoned (a block that was not finished is never put)
            sync_all();
            j.timed_out = true;
            return 1;
        }
        p.in = w.pool[cur]; p.out = w.pool[cur ^ 1];
        p.count_in = w.count[cur]; p.count_out = w.count[cur ^ 1];
        if (p.split == 1) {
            // k_trace<any> of iteration i only adds to the radiance of the pool that iteration i + 1 reads its rays from: it runs on
            // a second stream beside k_trace<closest> of iteration i + 1 (the two fill each other's launch tails); k_shade waits for
            // it.  The scheduling waves are independent, so two such chains (halves of the waves) run side by side.
            for (uint32_t k = 0; k < split_parts; ++k) {
                RenderParams h = p;
                h.wave_first = plan.split_lo[k]; h.wave_last = plan.split_lo[k + 1];
                hipStream_t s_main = chain_main(k), s_any = w.chain_any[k];
                hipEvent_t e_shade = w.chain_ev[2 * k], e_any = w.chain_ev[2 * k + 1];
                if (int rc = split_stage(h, 0, s_main)) return rc;
                if (it > 0) HIP_TRY(hipStreamWaitEvent(s_main, e_any, 0));
                if (int rc = split_stage(h, 1, s_main)) return rc;
                HIP_TRY(hipEventRecord(e_shade, s_main));
                HIP_TRY(hipStreamWaitEvent(s_any, e_shade, 0));
                if (int rc = split_stage(h, 2, s_any)) return rc;
                HIP_TRY(hipEventRecord(e_any, s_any));
                HIP_TRY(prof.err);
            }
        } else if (p.split == 3 && n_parts > 1) {
            // the scheduling waves are independent of each other: part-size launches on their own streams advance in their own
            // rhythm and fill each other's launch tails
            RenderParams h = p;
            h.gather_w = drain.gather_w;
            for (uint32_t k = 0; k < n_parts; ++k) {
                h.wave_first = plan.part_lo[k]; h.wave_last = plan.part_lo[k + 1];
                HIP_TRY(launch_bounce(h, k == 0 ? j.stream : w.part_stream[k - 1]));
            }
        } else {
            p.gather_w = drain.gather_w;
            HIP_TRY(launch_bounce(p, j.stream));
        }
        cur ^= 1; ++it;
        if (exp_env("MTSAMD_TRACE_ITERS")) {      // diagnostic: alive paths and wall time of every scheduler iteration (serialises the loop)
            sync_all();
            static thread_local std::vector<uint32_t> hc;
            hc.resize(nw);
            HIP_TRY(hipMemcpy(hc.data(), w.count[cur], nw * sizeof(uint32_t), hipMemcpyDeviceToHost));
            uint64_t alive = 0, busy_waves = 0;
            for (uint32_t k = 0; k < nw; ++k) { alive += hc[k]; busy_waves += hc[k] ? 1 : 0; }
            static thread_local std::chrono::steady_clock::time_point t_prev;
            const auto t_now = std::chrono::steady_clock::now();
            fprintf(stderr, "iter %llu alive %llu waves_with_paths %llu dt_us %.0f gather_w %u\n", (unsigned long long) it, (unsigned long long) alive,
                    (unsigned long long) busy_waves, it > 1 ? std::chrono::duration<double, std::micro>(t_now - t_prev).count() : 0.0, drain.gather_w);
            t_prev = std::chrono::steady_clock::now();
        }
        if (drain.due(it)) {
            if (pending >= 0) {
                HIP_TRY(hipEventSynchronize(w.ev[pending]));
                const uint64_t *hcur = w.h_cursor_rb + (size_t) pending * nw;
                const bool may_gather = drain.gather_w < plan.gather_max;
                const Drain::Verdict v = drain.inspect(it, w.h_counts + (size_t) pending * nw, hcur, w.h_cursor + nw);
                if (v == Drain::Done) break;
                if (v == Drain::Finish) { finish = true; break; }
                if (may_gather && exp_env("MTSAMD_TRACE_ITERS")) {
                    uint32_t wet = 0, first_wet = 0;
                    for (uint32_t k = 0; k < nw; ++k) if (hcur[k] < w.h_cursor[nw + k]) { if (!wet) first_wet = k; ++wet; }
                    fprintf(stderr, "check at it %llu: alive %llu wet %u first_wet %u cur %llu end %llu\n", (unsigned long long) it, (unsigned long long) drain.alive, wet, first_wet,
                            (unsigned long long) hcur[first_wet], (unsigned long long) w.h_cursor[nw + first_wet]);
                }
            }
            if (n_parts > 1) { if (int rc = join_parts()) return rc; }
            if (split_parts > 1) { if (int rc = join_chains()) return rc; }      // the counts of the other chains are written by their k_shade
            HIP_TRY(hipMemcpyAsync(w.h_counts + (size_t) slot * nw, w.count[cur], nw * sizeof(uint32_t), hipMemcpyDeviceToHost, j.stream));
            if (drain.reads_cursors()) HIP_TRY(hipMemcpyAsync(w.h_cursor_rb + (size_t) slot * nw, w.cursor, nw * sizeof(uint64_t), hipMemcpyDeviceToHost, j.stream));
            HIP_TRY(hipEventRecord(w.ev[slot], j.stream));
            pending = slot; slot ^= 1;
        }
        if (it > (1ull << 24)) return fail(MTSAMD_ERR_DEVICE, "wavefront scheduler did not converge");
    }
    if (p.split == 1 && it > 0) {
        for (uint32_t k = 0; k < split_parts; ++k) HIP_TRY(hipStreamWaitEvent(j.stream, w.chain_ev[2 * k + 1], 0));      // the last k_trace<any> of every chain
        if (int rc = join_chains()) return rc;
    }
    if (n_parts > 1) { if (int rc = join_parts()) return rc; }
    if (finish) {          // every stream of the loop has been joined into j.stream
        RenderParams h = p;
        h.in = w.pool[cur]; h.out = w.pool[cur ^ 1];
        h.count_in = w.count[cur]; h.count_out = w.count[cur ^ 1];
        HIP_TRY(launch_finish(h, drain.alive, j.stream));
        ++it;
    }
    j.iterations += it;
    return 0;
}

// Traces the local sample ordinals [first, first+n) of this render's rows to completion; results land in
// ws.out_rgba / out_pos (slot = ordinal - first).
int trace_pass(Job &j, uint64_t first, uint64_t n) {
    Workspace &w = j.s->ws;
    const uint32_t nw = j.shape.n_waves;
    PassPlan plan;
    if (int rc = plan_pass(j.shape, first, n, j.d->finish_kernel, j.d->pipeline, w.h_cursor + nw, plan)) return rc;
    std::fill(w.h_cursor, w.h_cursor + nw, 0);
    HIP_TRY(hipMemcpyAsync(w.cursor, w.h_cursor, nw * sizeof(uint64_t), hipMemcpyHostToDevice, j.stream));
    HIP_TRY(hipMemcpyAsync(w.cursor_end, w.h_cursor + nw, nw * sizeof(uint64_t), hipMemcpyHostToDevice, j.stream));
    HIP_TRY(hipMemsetAsync(w.count[0], 0, 2 * (size_t) nw * sizeof(uint32_t), j.stream));
    HIP_TRY(hipMemsetAsync(w.count[1], 0, 2 * (size_t) nw * sizeof(uint32_t), j.stream));

    RenderParams p{};
    p.sv = j.s->view; p.cam = j.cam;
    if (p.cam.aperture_radius > 0.0f) p.sv.general = std::max(p.sv.general, 1u);      // thin lens: aperture sampling lives in the general kernels
    p.cursor = w.cursor; p.cursor_end = w.cursor_end; p.wave_stats = w.wave_stats;
    p.out_rgba = j.buf ? w.out_rgba2 : w.out_rgba; p.out_pos = j.buf ? w.out_pos2 : w.out_pos;
    p.count_shadow = w.count_shadow;
    p.first_ordinal = first; p.first_pix = plan.first_pix; p.first_rem = plan.first_rem;
    p.chunk = plan.chunk; p.base_seed = j.d->seed;
    p.n_chains = plan.n_chains;
    p.rows = j.rows; p.store_xyz = j.store_xyz;
    p.plane_pix0 = j.plane_pix0; p.plane_pixels = j.plane_pixels;
    p.n_waves = nw; p.seg_cap = w.seg_cap; p.target = j.shape.target;
    p.spp = j.d->sample_count; p.crop_x = j.d->crop_x; p.crop_y = j.d->crop_y; p.crop_w = j.d->crop_width; p.crop_h = j.d->crop_height;
    p.max_depth = j.d->max_depth; p.rr_depth = j.d->rr_depth;
    p.spectral = j.s->spectral ? 1 : 0;
    p.split = plan.split;
    if (p.split == 1) {       // k_trace: short per-lane stack in LDS, deep entries in a global spill area
        if (int rc = grow(w.trace_spill, w.trace_spill_words, trace_spill_words(p.sv, nw))) return rc;
        p.trace_lds_depth = trace_lds_depth(p.sv); p.trace_top_nodes = trace_top_nodes(p.sv); p.trace_spill = w.trace_spill;
    }
    p.integrator = j.d->integrator; p.emitter_samples = j.d->emitter_samples; p.bsdf_samples = j.d->bsdf_samples;
    p.hide_emitters = j.d->hide_emitters;
    if (plan.mode == PassMode::Direct) return timed(j, [&]() -> int { HIP_TRY(launch_direct(p, n, j.stream)); j.iterations += 1; return 0; });
    if (plan.mode == PassMode::Mega) return timed(j, [&]() -> int { HIP_TRY(launch_mega(p, j.stream)); j.iterations += 1; return 0; });
    StageProfile prof{ w, j.d->profile != 0 && p.split == 1 };
    if (int rc = timed(j, [&] { return launch_rounds(j, p, plan, prof); })) return rc;
    for (const StageProfile::Rec &r : prof.recs) {        // every stream has been joined into j.stream: all events are complete
        float sm = 0.0f;
        HIP_TRY(hipEventElapsedTime(&sm, w.prof_ev[r.e0], w.prof_ev[r.e0 + 1]));
        j.stage_ms[r.stage] += sm; j.stage_launches[r.stage] += 1;
    }
    return 0;
}

int setup_job(Job &j, mtsamd_scene *s, const mtsamd_render_desc *d, hipStream_t stream, uint64_t max_pass) {
    j.s = s; j.d = d; j.stream = stream;
    if (int rc = make_camera(*d, j.cam)) return rc;
    if (int rc = make_filter(d->rfilter, d->rfilter_param, d->rfilter_param2, d->rfilter_analytic, j.filter)) return rc;
    const SceneFacts facts{ s->view.flat != 0, s->nested_bsdfs, s->spectral, (uint32_t) s->cu_count };
    if (int rc = plan_job(facts, *d, max_pass, schedule_switches(), j.shape)) return rc;
    for (;;) {       // the pass is halved until its workspace fits the device
        j.pass_cap = pass_capacity(j.shape, max_pass);
        const int rc = ensure_workspace(s, j.shape.n_waves, j.shape.seg_cap, j.pass_cap, j.shape.split_pools());
        if (rc == MTSAMD_ERR_NOMEM && halve_pass(j.shape, max_pass)) continue;
        if (rc) return rc;
        break;
    }
    HIP_TRY(hipMemsetAsync(s->ws.wave_stats, 0, 4 * (size_t) j.shape.n_waves * sizeof(uint64_t), stream));
    s->cancel.store(0);
    j.t_start = std::chrono::steady_clock::now();
    return 0;
}

int collect_stats(Job &j, uint64_t samples, uint64_t *stats_host) {
    if (!stats_host) return 0;
    std::vector<uint64_t> ws(4 * (size_t) j.shape.n_waves);
    HIP_TRY(hipMemcpyAsync(ws.data(), j.s->ws.wave_stats, ws.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, j.stream));
    HIP_TRY(hipStreamSynchronize(j.stream));
    uint64_t tot[4] = { 0, 0, 0, 0 };
    for (uint32_t k = 0; k < j.shape.n_waves; ++k) for (int q = 0; q < 4; ++q) tot[q] += ws[4 * (size_t) k + q];
    stats_host[0] = tot[0]; stats_host[1] = tot[1]; stats_host[2] = samples; stats_host[3] = j.iterations; stats_host[4] = tot[2];
    stats_host[5] = (uint64_t) (j.bounce_ms * 1e6); stats_host[6] = (uint64_t) (j.film_ms * 1e6); stats_host[7] = tot[3];
    stats_host[8] = (uint64_t) (j.stage_ms[0] * 1e6); stats_host[9] = j.stage_launches[0];
    stats_host[10] = (uint64_t) (j.stage_ms[2] * 1e6); stats_host[11] = j.stage_launches[2];
    stats_host[12] = (uint64_t) (j.stage_ms[1] * 1e6); stats_host[13] = j.stage_launches[1];
    stats_host[14] = j.passes; stats_host[15] = j.timed_out ? 1u : 0u;
    return 0;
}

// Film rows owned by this call (include/mtsamd.h: row_begin/row_end window, or interleaved tiles).
int make_rows(const mtsamd_render_desc *d, RowMap &m) {
    if (d->part_count > 1) {
        if (d->part_index < 0 || d->part_index >= d->part_count || d->part_tile_rows <= 0)
            return fail(MTSAMD_ERR_INVALID, "invalid film partition (index %d of %d, %d rows per tile)", d->part_index, d->part_count, d->part_tile_rows);
        if (d->row_begin != 0 || d->row_end > 0) return fail(MTSAMD_ERR_INVALID, "row window and tile partition are mutually exclusive");
        m.row0 = 0; m.tile_rows = d->part_tile_rows; m.part = d->part_index; m.count = d->part_count;
        int32_t rows = 0;
        for (int32_t t = d->part_index; t * d->part_tile_rows < d->crop_height; t += d->part_count)
            rows += std::min(d->part_tile_rows, d->crop_height - t * d->part_tile_rows);
        m.local_rows = rows;
        return 0;
    }
    int row0 = d->row_begin, row1 = d->row_end <= 0 ? d->crop_height : d->row_end;
    if (row0 < 0 || row1 > d->crop_height || row0 > row1) return fail(MTSAMD_ERR_INVALID, "invalid row range [%d,%d)", row0, row1);
    m.row0 = row0; m.local_rows = row1 - row0; m.tile_rows = std::max(d->crop_height, 1); m.part = 0; m.count = 1;
    return 0;
}

// setup_job for a pass that also holds n_streams float4 per sample in ws.aov_stream (0: a plain render): they count when the pass is
// sized -- if the device cannot provide them the pass is halved, as setup_job halves it for the sample stream
int setup_aov_job(Job &j, mtsamd_scene *s, const mtsamd_render_desc *d, hipStream_t stream, uint64_t max_pass, uint32_t n_streams) {
    for (;;) {
        if (int rc = setup_job(j, s, d, stream, max_pass)) return rc;
        Workspace &w = s->ws;
        const int rc = grow(w.aov_stream, w.aov_stream_slots, j.pass_cap * n_streams);
        if (rc == MTSAMD_ERR_NOMEM && j.pass_cap > (1ull << 22)) { max_pass = j.pass_cap >> 1; continue; }
        return rc;
    }
}

// ---- film renders: what mtsamd_render and mtsamd_render_aov share around their pass loops ---------
// trace_pass for a pass loop: false ends the loop -- a timeout inside the pass drops its samples, an error is left in rc_loop
bool trace_rows(Job &j, const Job::Pass &p, int &rc_loop) { const int rc = trace_pass(j, p.a, p.n); if (rc < 0) rc_loop = rc; return rc == 0; }

int check_call(const mtsamd_scene *s, const mtsamd_render_desc *d, const float *out) {          // of a call that renders `d` on `s` into `out`
    if (!s || !out) return fail(MTSAMD_ERR_INVALID, "null argument");
    return check_desc(d);
}

// The opening of a film render once its arguments are checked: the device, the rows the call owns, the job (with aov_streams float4 per
// sample beside the sample stream) and its film passes.
int open_render(Job &j, mtsamd_scene *s, const mtsamd_render_desc *d, hipStream_t stream, uint32_t aov_streams, int store_xyz) {
    HIP_TRY(hipSetDevice(s->device));
    RowMap rows{};
    if (int rc = make_rows(d, rows)) return rc;
    j.per_row = (uint64_t) d->crop_width * (uint64_t) d->sample_count;
    j.total = j.per_row * (uint64_t) rows.local_rows;
    if (int rc = setup_aov_job(j, s, d, stream, j.total, aov_streams)) return rc;
    j.rows = rows; j.store_xyz = store_xyz;
    // passes hold whole local rows so that the sample stream can be stored as one plane per sample number
    return plan_film_passes(rows, j.pass_cap, j.per_row, j.fp);
}

// The film stage of a render call (Film::put): the sample streams of whole local rows are splatted into 5-channel films, by the tiled
// kernels where the filter allows it and by the gather kernel otherwise.  The stage owns that choice, the scratch tiles, the timing events
// of Workspace::film_ev and the film time; the render calls say which rows, which streams into which films, and on which stream.
struct FilmStage {
    Job &j;
    Workspace &w = j.s->ws;
    const bool tiled = film_tiles_supported(j.filter);
    const int32_t R = (int32_t) std::ceil(j.filter.radius);
    size_t brackets = 0;          // begin / end pairs of film_ev in use
    FilmParams f{}; hipStream_t on = nullptr;      // the open bracket: its rows and its stream

    // scratch tiles for every splat the call can issue (schedule.h, film_reserve_floats), before anything is queued
    int reserve(bool per_pass) {
        return tiled ? grow(w.film_partials, w.film_partial_floats, film_reserve_floats(j.fp, j.rows.local_rows, j.d->crop_width, j.d->sample_count, per_pass)) : 0;
    }
    // A bracket: begin event | puts of the local rows [lr0, lr0 + nrows), whatever else the caller queues on `st` between them | end event
    int begin(hipStream_t st, uint64_t lr0, uint64_t nrows, int32_t tile_h) {
        f = FilmParams{}; f.filter = j.filter; on = st;
        film_splat_geometry(j.rows, *j.d, R, tiled, lr0, nrows, tile_h, f);
        if (tiled) {
            // the only regrow rule; after reserve() it never fires (tests/test_schedule_cpu.py).  An earlier splat may still read the tiles.
            const size_t need = film_partial_floats(f);
            if (need > w.film_partial_floats) HIP_TRY(hipStreamSynchronize(st));
            if (int rc = grow(w.film_partials, w.film_partial_floats, need)) return rc;
            f.partials = w.film_partials;
        }
        for (hipEvent_t e = nullptr; w.film_ev.size() < 2 * (brackets + 1); w.film_ev.push_back(e)) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipEventRecord(w.film_ev[2 * brackets], st));
        return 0;
    }
    int put(const float4 *rgba, const float2 *pos, float *film) {
        f.out_rgba = rgba; f.out_pos = pos; f.film = film;
        HIP_TRY(tiled ? launch_film_tiles(f, on) : launch_film_gather(f, on));
        return 0;
    }
    int end() { HIP_TRY(hipEventRecord(w.film_ev[2 * brackets++ + 1], on)); return 0; }
    // The close of a film render, once every stream it used has been synchronised: stage time, statistics, final sync
    int close(uint64_t *stats_host) {
        for (size_t k = 0; k < brackets; ++k) {
            float fms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&fms, w.film_ev[2 * k], w.film_ev[2 * k + 1]));
            j.film_ms += fms;
        }
        if (int rc = collect_stats(j, j.total, stats_host)) return rc;
        HIP_TRY(hipStreamSynchronize(j.stream));
        return MTSAMD_OK;
    }
};
} // namespace

extern "C" {
int mtsamd_render(mtsamd_scene *s, const mtsamd_render_desc *d, float *film, uint64_t *stats_host, void *stream_) {
    if (int rc = check_call(s, d, film)) return rc;
    hipStream_t stream = (hipStream_t) stream_;
    Job j;
    if (int rc = open_render(j, s, d, stream, 0, d->film_rgb ? 2 : 1)) return rc;
    FilmStage fs{ j };
    Workspace &ws = s->ws;
    // moment integrator: the sample stream is splatted twice (values, then squared values) into two scratch films
    float *film_target = film, *film_sq = nullptr;
    const uint64_t n_pixels = (uint64_t) d->crop_width * (uint64_t) d->crop_height;
    if (d->moment) {
        if (d->film_rgb) return fail(MTSAMD_ERR_UNSUPPORTED, "the moment integrator writes XYZ channels (film_rgb must be 0)");
        if (int rc = grow(ws.moment_film, ws.moment_floats, 2 * 5 * n_pixels)) return rc;
        HIP_TRY(hipMemsetAsync(ws.moment_film, 0, 2 * 5 * n_pixels * sizeof(float), stream));
        film_target = ws.moment_film; film_sq = ws.moment_film + 5 * n_pixels;
    }
    // Several passes: the film splat of pass k runs on its own stream while pass k + 1 is traced into the other sample stream buffer.
    bool overlap = j.fp.n_passes > 1;
    hipStream_t fstream = stream;
    if (overlap) {
        const int rc = grow(ws.out_rgba2, ws.out_pos2, ws.pass_cap2, std::min<uint64_t>(j.fp.rows_per_pass * j.per_row, j.pass_cap));
        if (rc == MTSAMD_ERR_NOMEM) {          // no room for the second sample stream: the splat of a pass runs before the next pass
            (void) hipFree(ws.out_rgba2); (void) hipFree(ws.out_pos2); ws.out_rgba2 = nullptr; ws.out_pos2 = nullptr;
            overlap = false;
        } else if (rc) return rc;
    }
    if (overlap) {
        fstream = ws.film_stream;
        // the film (and the moment scratch films) may still be written by work queued on `stream` before this call
        HIP_TRY(hipEventRecord(ws.film_done[0], stream));
        HIP_TRY(hipStreamWaitEvent(fstream, ws.film_done[0], 0));
    }
    if (int rc = fs.reserve(true)) return rc;
    int rc_loop = 0;
    for (uint64_t lr0 = 0; lr0 < (uint64_t) j.rows.local_rows; lr0 += j.fp.rows_per_pass) {          // pass k = j.passes: the loop ends with the first pass that is dropped
        const Job::Pass p = j.pass(lr0);
        j.buf = overlap ? (int) (j.passes & 1u) : 0;
        if (j.expired()) { j.timed_out = true; break; }
        // the buffer this pass writes was read by the splat of pass k - 2
        if (overlap && j.passes >= 2) HIP_TRY(hipStreamWaitEvent(stream, ws.film_done[j.buf], 0));
        if (!trace_rows(j, p, rc_loop)) break;
        j.passes += 1;
        // Film::put: splat this pass into the film rows its samples can reach (trace_pass returns when its samples are complete)
        float4 *rgba = j.buf ? ws.out_rgba2 : ws.out_rgba;
        const float2 *pos = j.buf ? ws.out_pos2 : ws.out_pos;
        if (int rc = fs.begin(fstream, p.lr0, p.nrows, j.fp.tile_h)) return rc;
        if (int rc = fs.put(rgba, pos, film_target)) return rc;
        if (film_sq) {
            HIP_TRY(launch_square_stream(rgba, p.n, fstream));
            if (int rc = fs.put(rgba, pos, film_sq)) return rc;
        }
        if (int rc = fs.end()) return rc;
        if (overlap) HIP_TRY(hipEventRecord(ws.film_done[j.buf], fstream));
    }
    if (overlap) {          // `stream` continues after the last splat
        HIP_TRY(hipEventRecord(ws.film_done[0], fstream));
        HIP_TRY(hipStreamWaitEvent(stream, ws.film_done[0], 0));
        HIP_TRY(hipStreamSynchronize(fstream));
    } else HIP_TRY(hipStreamSynchronize(stream));
    if (rc_loop) return rc_loop;
    if (film_sq) HIP_TRY(launch_moment_pack(film_target, film_sq, film, n_pixels, stream));
    return fs.close(stats_host);
}

// ---- aov integrator (src/integrators/aov.cpp) -------------------------------------------------
// AOV types -> the SurfaceInteraction field every film channel shows (aov.cpp:92-134)
static int aov_channels(const int32_t *types, uint32_t n_aovs, AovParams &a) {
    if (n_aovs && !types) return fail(MTSAMD_ERR_INVALID, "null argument");
    a.n_channels = 0;
    for (uint32_t i = 0; i < n_aovs; ++i) {
        uint32_t src, cnt;
        switch (types[i]) {
        case MTSAMD_AOV_DEPTH: src = kAovT; cnt = 1; break;
        case MTSAMD_AOV_POSITION: src = kAovP; cnt = 3; break;
        case MTSAMD_AOV_UV: src = kAovUV; cnt = 2; break;
        case MTSAMD_AOV_GEO_NORMAL: src = kAovN; cnt = 3; break;
        case MTSAMD_AOV_SH_NORMAL: src = kAovShN; cnt = 3; break;
        case MTSAMD_AOV_DP_DU: src = kAovDpDu; cnt = 3; break;
        case MTSAMD_AOV_DP_DV: src = kAovDpDv; cnt = 3; break;
        case MTSAMD_AOV_DUV_DX: case MTSAMD_AOV_DUV_DY: src = kAovZero; cnt = 2; break;      // never computed by the reference: zeros
        default: return fail(MTSAMD_ERR_INVALID, "Invalid AOV type %d", types[i]);           // aov.cpp:131
        }
        if (a.n_channels + cnt > kAovMaxChannels) return fail(MTSAMD_ERR_UNSUPPORTED, "more than %u AOV channels", kAovMaxChannels);
        for (uint32_t k = 0; k < cnt; ++k) a.source[a.n_channels++] = (uint8_t) (src == kAovZero ? src : src + k);
    }
    return 0;
}

// the part of RenderParams k_aov reads (generate_path, the scene, the statistics); first_ordinal / plane_pix0 are set per pass
static void aov_render_params(const Job &j, RenderParams &p) {
    p = RenderParams{};
    p.sv = j.s->view; p.cam = j.cam;
    p.wave_stats = j.s->ws.wave_stats; p.n_waves = j.shape.n_waves;
    p.out_pos = j.s->ws.out_pos;          // the values the nested integrator's sample wrote there, or the only copy
    p.base_seed = j.d->seed; p.rows = j.rows;
    p.spp = j.d->sample_count; p.crop_x = j.d->crop_x; p.crop_y = j.d->crop_y; p.crop_w = j.d->crop_width; p.crop_h = j.d->crop_height;
    p.spectral = j.s->spectral ? 1 : 0;
}

int mtsamd_render_aov(mtsamd_scene *s, const mtsamd_render_desc *d_, const int32_t *aov_types, uint32_t n_aovs, int32_t nested, float *film,
                      uint64_t *stats_host, void *stream_) {
    if (int rc = check_call(s, d_, film)) return rc;
    if (d_->moment) return fail(MTSAMD_ERR_UNSUPPORTED, "the aov integrator nests path, direct or depth, not moment (desc->moment must be 0)");
    if (d_->film_rgb) return fail(MTSAMD_ERR_UNSUPPORTED, "the aov integrator writes X,Y,Z,A,W and its own R,G,B,A channels (film_rgb must be 0)");
    AovParams ap{};
    if (int rc = aov_channels(aov_types, n_aovs, ap)) return rc;
    if (ap.n_channels == 0 && !nested) return fail(MTSAMD_ERR_INVALID, "the aov integrator needs an AOV or a nested integrator");
    mtsamd_render_desc dd = *d_;
    if (!nested) dd.integrator = 0;       // nothing is traced: the scheduler only sizes the pass
    const mtsamd_render_desc *d = &dd;
    hipStream_t stream = (hipStream_t) stream_;
    const uint32_t C = ap.n_channels, n_groups = (C + 2u) / 3u, n_films = 1u + n_groups + (nested ? 1u : 0u);
    Job j;
    // the linear-RGB stream drops non-finite samples only, the rule of a film with AOVs (integrator.cpp:249-251); spectral variant: XYZ
    if (int rc = open_render(j, s, d, stream, n_groups + (nested ? 1u : 0u), s->spectral ? 1 : 2)) return rc;
    FilmStage fs{ j };
    const int mode = !nested ? 0 : (s->spectral ? 2 : 1);
    Workspace &ws = s->ws;
    const uint64_t n_pixels = (uint64_t) d->crop_width * (uint64_t) d->crop_height;
    // one scratch 5-channel film per stream: X,Y,Z,A,W | the channel groups | R,G,B,A (k_aov_pack interleaves them)
    if (int rc = grow(ws.aov_film, ws.aov_film_floats, n_films * 5 * n_pixels)) return rc;
    HIP_TRY(hipMemsetAsync(ws.aov_film, 0, n_films * 5 * n_pixels * sizeof(float), stream));
    // A film splatted pass by pass is not the film of one pass bit for bit: the film kernels sum per source tile of a pass, so rows
    // reached from two passes are added in another order (tests/test_gpu_lifecycle.py accepts that for mtsamd_render).  A render of
    // several passes whose streams fit the scene's keep limit (mtsamd_scene_set_aov_keep_limit, 1 GiB by default) therefore keeps the
    // streams of all passes -- n_kept float4 + one float2 position per sample -- and splats them once, with the tile grid of a one-pass
    // render: passes then bound the tracing workspace and are where a timeout / cancel stops, and never show in the film.  The buffer
    // lives for this call only.  Whether it is used follows from the description and the limit alone, never from the memory that happens
    // to be free: if the device cannot provide it the call fails.  Above the limit each pass is splatted before the next is traced, as
    // mtsamd_render does.
    const uint32_t n_kept = n_groups + (nested ? 2u : 1u);          // groups, second colour space, the nested stream
    const uint64_t keep_slots = j.total * n_kept + j.total / 2 + 1;
    const bool retain = j.fp.n_passes > 1 && j.total <= (1ull << 30) && keep_slots * sizeof(float4) <= s->aov_keep_limit;
    struct Keep { Workspace &w; ~Keep() { (void) hipFree(w.aov_keep); w.aov_keep = nullptr; } } keep{ ws };
    // the scratch tiles first: they must not fail after the kept streams took the memory
    if (int rc = fs.reserve(!retain)) return rc;
    if (retain) {
        (void) hipFree(ws.aov_keep); ws.aov_keep = nullptr;
        if (int rc = ws_alloc((void **) &ws.aov_keep, keep_slots * sizeof(float4))) return rc;
    }
    float4 *groups = retain ? ws.aov_keep : ws.aov_stream;
    const uint64_t stride = retain ? j.total : j.pass_cap;            // slots per stream
    float4 *conv = nested ? groups + (size_t) n_groups * stride : nullptr;
    float4 *strm = retain ? groups + (size_t) (n_kept - 1u) * stride : ws.out_rgba;
    float2 *spos = retain ? reinterpret_cast<float2 *>(groups + (size_t) n_kept * stride) : ws.out_pos;
    aov_render_params(j, ap.rp);
    ap.group_stride = stride;
    // Film::put of the streams of the local rows [lr0, lr0 + nrows), held from slot 0 on, into their scratch films
    auto splat = [&](uint64_t lr0, uint64_t nrows, int32_t tile_h) -> int {
        if (int rc = fs.begin(stream, lr0, nrows, tile_h)) return rc;
        if (int rc = fs.put(mode == 1 ? conv : strm, spos, ws.aov_film)) return rc;                       // X, Y, Z, A
        for (uint32_t k = 0; k < n_groups; ++k) { if (int rc = fs.put(groups + (size_t) k * stride, spos, ws.aov_film + (size_t) (1u + k) * 5 * n_pixels)) return rc; }
        if (nested) { if (int rc = fs.put(mode == 1 ? strm : conv, spos, ws.aov_film + (size_t) (1u + n_groups) * 5 * n_pixels)) return rc; }      // R, G, B, A
        return fs.end();
    };
    int rc_loop = 0;
    uint64_t rows_done = 0;
    for (uint64_t lr0 = 0; lr0 < (uint64_t) j.rows.local_rows; lr0 += j.fp.rows_per_pass) {
        const Job::Pass p = j.pass(lr0);
        const uint64_t off = retain ? p.a : 0;
        j.buf = 0;
        if (s->cancel.load(std::memory_order_relaxed)) { rc_loop = fail(MTSAMD_ERR_CANCELLED, "render cancelled"); break; }
        if (j.expired()) { j.timed_out = true; break; }
        if (nested) {
            if (!trace_rows(j, p, rc_loop)) break;
            if (retain) HIP_TRY(hipMemcpyAsync(strm + off, ws.out_rgba, p.n * sizeof(float4), hipMemcpyDeviceToDevice, stream));
        }
        j.passes += 1;
        ap.rp.first_ordinal = p.a; ap.rp.plane_pix0 = j.plane_pix0; ap.rp.plane_pixels = 0u;
        ap.rp.out_pos = spos + off; ap.groups = groups + off;
        HIP_TRY(hipEventRecord(ws.tev[0], stream));
        HIP_TRY(launch_aov(ap, p.n, stream));
        HIP_TRY(hipEventRecord(ws.tev[1], stream));
        HIP_TRY(launch_aov_finish(strm + off, conv ? conv + off : nullptr, groups + off, stride, n_groups, mode, p.n, stream));
        if (!retain) { if (int rc = splat(p.lr0, p.nrows, j.fp.tile_h)) return rc; }
        HIP_TRY(hipEventSynchronize(ws.tev[1]));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, ws.tev[0], ws.tev[1]));
        j.bounce_ms += ms; j.iterations += 1;
        rows_done = p.lr0 + p.nrows;
    }
    if (retain && rows_done > 0 && !rc_loop) { if (int rc = splat(0, rows_done, j.fp.tile_h_one)) return rc; }
    HIP_TRY(hipStreamSynchronize(stream));
    if (rc_loop) return rc_loop;
    HIP_TRY(launch_aov_pack(ws.aov_film, n_pixels, C, nested ? 1 : 0, film, stream));
    return fs.close(stats_host);
}

int mtsamd_scene_set_aov_keep_limit(mtsamd_scene *s, uint64_t bytes) {
    if (!s) return fail(MTSAMD_ERR_INVALID, "null argument");
    s->aov_keep_limit = bytes;
    return MTSAMD_OK;
}

int mtsamd_sample_aovs(mtsamd_scene *s, const mtsamd_render_desc *d_, const int32_t *aov_types, uint32_t n_aovs, uint64_t first, uint64_t count,
                       float *aovs, float *pos, void *stream_) {
    if (int rc = check_call(s, d_, aovs)) return rc;
    AovParams ap{};
    if (int rc = aov_channels(aov_types, n_aovs, ap)) return rc;
    if (ap.n_channels == 0) return fail(MTSAMD_ERR_INVALID, "no AOV requested");
    mtsamd_render_desc dd = *d_;
    dd.integrator = 0;                    // nothing is traced: the scheduler only sizes the pass
    const mtsamd_render_desc *d = &dd;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t) stream_;
    const uint64_t total = (uint64_t) d->crop_width * d->crop_height * (uint64_t) d->sample_count;
    if (first + count > total) return fail(MTSAMD_ERR_INVALID, "sample range exceeds W*H*sample_count");
    if (count == 0) return MTSAMD_OK;
    const uint32_t n_groups = (ap.n_channels + 2u) / 3u;
    Job j;
    if (int rc = setup_aov_job(j, s, d, stream, count, n_groups)) return rc;
    j.rows = RowMap{ 0, d->crop_height, std::max(d->crop_height, 1), 0, 1 };
    aov_render_params(j, ap.rp);
    ap.groups = s->ws.aov_stream; ap.group_stride = j.pass_cap;
    for (uint64_t a = 0; a < count; a += j.pass_cap) {
        const uint64_t n = std::min<uint64_t>(j.pass_cap, count - a);
        ap.rp.first_ordinal = first + a;
        HIP_TRY(launch_aov(ap, n, stream));
        HIP_TRY(launch_aov_unpack(s->ws.aov_stream, j.pass_cap, ap.n_channels, n, aovs + (size_t) ap.n_channels * a, stream));
        if (pos) HIP_TRY(hipMemcpyAsync(pos + 2 * a, s->ws.out_pos, n * sizeof(float2), hipMemcpyDeviceToDevice, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return MTSAMD_OK;
}

// sensor / sampler / film part of an adjoint launch: the whole crop window of `d`, the primal film's weights, dLoss/dImage
static int fill_adjoint(mtsamd_scene *s, const mtsamd_render_desc *d, const float *dimage, const float *film, AdjointParams &a, bool spectral = false) {
    if (!s || !dimage || !film) return fail(MTSAMD_ERR_INVALID, "null argument");
    if (int rc = check_desc(d)) return rc;
    if (d->part_count > 1 || d->row_begin != 0 || d->row_end > 0) return fail(MTSAMD_ERR_UNSUPPORTED, "the adjoint pass renders the whole crop window");
    if (s->spectral && !spectral) return fail(MTSAMD_ERR_UNSUPPORTED, "the adjoint pass is implemented for the RGB variant only");
    if (!s->spectral && spectral) return fail(MTSAMD_ERR_UNSUPPORTED, "the spectral adjoint pass needs a scene of the spectral variant");
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = make_camera(*d, a.rp.cam)) return rc;
    if (int rc = make_filter(d->rfilter, d->rfilter_param, d->rfilter_param2, d->rfilter_analytic, a.filter)) return rc;
    if (a.filter.taps > 8) return fail(MTSAMD_ERR_UNSUPPORTED, "reconstruction filter too wide for the adjoint pass");
    a.rp.sv = s->view;
    if (a.rp.cam.aperture_radius > 0.0f) a.rp.sv.general = std::max(a.rp.sv.general, 1u);
    a.rp.base_seed = d->seed; a.rp.spp = d->sample_count;
    a.rp.crop_x = d->crop_x; a.rp.crop_y = d->crop_y; a.rp.crop_w = d->crop_width; a.rp.crop_h = d->crop_height;
    a.rp.max_depth = d->max_depth; a.rp.rr_depth = d->rr_depth;
    a.rp.rows = RowMap{ 0, d->crop_height, std::max(d->crop_height, 1), 0, 1 };
    a.rp.store_xyz = 0; a.rp.out_pos = nullptr; a.rp.out_rgba = nullptr;
    a.n_samples = (uint64_t) d->crop_width * d->crop_height * (uint64_t) d->sample_count;
    a.dimage = dimage; a.film = film;
    return 0;
}

int mtsamd_render_adjoint(mtsamd_scene *s, const mtsamd_render_desc *d, const float *dimage, const float *film, float *grad_bsdf,
                          float *grad_tex, float *grad_emitter, void *stream_) {
    AdjointParams a{};
    if (int rc = fill_adjoint(s, d, dimage, film, a)) return rc;
    if (d->max_depth < 0 || d->max_depth > 16)
        return fail(MTSAMD_ERR_UNSUPPORTED, "the adjoint pass needs a finite max_depth <= 16 (got %d)", d->max_depth);
    if (s->non_diffuse_bsdfs) return fail(MTSAMD_ERR_UNSUPPORTED, "the adjoint pass is implemented for diffuse BSDFs (one- or two-sided) only");
    if (s->environment >= 0 || s->delta_emitters) return fail(MTSAMD_ERR_UNSUPPORTED, "the adjoint pass handles area emitters only");
    if (s->bsdfs.size() > 32 && grad_bsdf) return fail(MTSAMD_ERR_UNSUPPORTED, "at most 32 BSDFs with constant-reflectance gradients");
    if (s->emitters.size() > 32 && grad_emitter) return fail(MTSAMD_ERR_UNSUPPORTED, "at most 32 emitters with radiance gradients");
    a.grad_bsdf = grad_bsdf; a.grad_tex = grad_tex; a.grad_emitter = grad_emitter;
    HIP_TRY(launch_adjoint(a, (hipStream_t) stream_));
    return MTSAMD_OK;
}

int mtsamd_scene_set_bsdf_param(mtsamd_scene *s, uint32_t bsdf, int32_t kind, const float *value3) {
    if (!s || !value3 || bsdf >= s->bsdfs.size()) return fail(MTSAMD_ERR_INVALID, "invalid bsdf index");
    if (int rc = set_bsdf_param(*s, bsdf, kind, value3)) return rc;
    return push_bsdf(s, bsdf);
}

int mtsamd_render_adjoint_param(mtsamd_scene *s, const mtsamd_render_desc *d, const float *dimage, const float *film, uint32_t bsdf, int32_t kind,
                                int32_t component, float h, float *grad1, void *stream_) {
    AdjointParams a{};
    if (int rc = fill_adjoint(s, d, dimage, film, a)) return rc;
    if (!grad1 || bsdf >= s->bsdfs.size()) return fail(MTSAMD_ERR_INVALID, "invalid argument");
    if (s->textured_params) return fail(MTSAMD_ERR_UNSUPPORTED, "the parameter adjoint does not handle textured BSDF parameters (alpha, specular_reflectance, specular_transmittance)");
    if (s->nested_bsdfs) return fail(MTSAMD_ERR_UNSUPPORTED, "the parameter adjoint does not handle blendbsdf / mask materials");
    if (d->integrator != 0) return fail(MTSAMD_ERR_UNSUPPORTED, "the adjoint pass differentiates the path integrator");
    const DevBsdf &b = s->bsdfs[bsdf];
    float DevBsdf::*f0, DevBsdf::*f1;
    if (!bsdf_param_fields(b, kind, component, f0, f1)) return fail(MTSAMD_ERR_UNSUPPORTED, "bsdf %u (type %d) has no differentiable parameter of kind %d", bsdf, b.type, kind);
    const float theta = b.*f0;
    if (!(h > 0.0f)) h = 0.01f * std::max(std::fabs(theta), 0.05f);      // central difference of the model code at fixed directions
    if ((kind == MTSAMD_PARAM_ALPHA || kind == MTSAMD_PARAM_ETA) && theta - h <= 1e-4f) h = 0.5f * (theta - 1e-4f);
    if (!(h > 0.0f)) return fail(MTSAMD_ERR_INVALID, "parameter value %g leaves no room for a central difference", theta);
    a.pg_bsdf = (int32_t) bsdf; a.pg_plus = b; a.pg_minus = b;
    a.pg_plus.*f0 = theta + h; a.pg_minus.*f0 = theta - h;
    if (f1) { a.pg_plus.*f1 = theta + h; a.pg_minus.*f1 = theta - h; }
    a.pg_inv_2h = 1.0f / ((theta + h) - (theta - h));
    a.grad_param = grad1;
    a.rp.sv.general = std::max(a.rp.sv.general, 1u);
    HIP_TRY(launch_adjoint_param(a, (hipStream_t) stream_));
    return MTSAMD_OK;
}

// ---- forward-mode derivative render (docs/examples/10_inverse_rendering/forward_diff.py) -------
// What both entry points refuse before the device is touched, and the host half of the tangent: the perturbed record tables
static int check_forward(const mtsamd_scene *s, const mtsamd_render_desc *d, const mtsamd_tangent_desc *t, const void *out, bool film,
                         std::vector<DevBsdf> &plus, std::vector<DevBsdf> &minus, std::vector<float> &inv_2h, bool &nested) {
    nested = false;
    if (!s || !d || !t || !out) return fail(MTSAMD_ERR_INVALID, "null argument");
    if (!t->bsdf_tangents && !t->emitter_tangents && !t->texture_tangents_dev && !t->envmap_tangent_dev)
        return fail(MTSAMD_ERR_INVALID, "the tangent is empty: bsdf_tangents, emitter_tangents, texture_tangents_dev and envmap_tangent_dev are all null");
    if (int rc = check_desc(d)) return rc;
    // a flag bit is known where it means something (PARAM_TEXTURES: textured BSDF parameters; NESTED: blend / mask records); elsewhere it stays refused
    if (int rc = check_derivative_flags(*s, t->flags, false, nested)) return rc;
    if (d->integrator != 0) return fail(MTSAMD_ERR_UNSUPPORTED, "the forward-mode render differentiates the path integrator");
    if (d->part_count > 1 || d->row_begin != 0 || d->row_end > 0) return fail(MTSAMD_ERR_UNSUPPORTED, "the forward-mode render covers the whole crop window (no row window, no tile partition)");
    if (film) {
        if (d->moment) return fail(MTSAMD_ERR_UNSUPPORTED, "the forward-mode render has no moment channels");
        if (d->film_rgb != 1) return fail(MTSAMD_ERR_UNSUPPORTED, "the forward-mode render writes an R, G, B, A, W film (film_rgb must be 1)");
        FilterView filter;
        if (int rc = make_filter(d->rfilter, d->rfilter_param, d->rfilter_param2, d->rfilter_analytic, filter)) return rc;
        if (filter.taps > 8) return fail(MTSAMD_ERR_UNSUPPORTED, "reconstruction filter too wide for the forward-mode render");
    }
    if (t->envmap_tangent_dev && (s->environment < 0 || !s->d_envmap)) return fail(MTSAMD_ERR_UNSUPPORTED, "envmap_tangent_dev: the scene has no envmap emitter");
    if (t->texture_tangents_dev) {
        bool bitmaps = false;
        for (const DevTexture &tx : s->textures) bitmaps = bitmaps || tx.kind == 0u;
        if (!bitmaps) return fail(MTSAMD_ERR_UNSUPPORTED, "texture_tangents_dev: the scene has no bitmap textures");
    }
    if (t->emitter_tangents)
        for (size_t i = 0; i < 3 * s->emitters.size(); ++i)
            if (!std::isfinite(t->emitter_tangents[i])) return fail(MTSAMD_ERR_INVALID, "emitter %u: its tangent is not finite", (unsigned) (i / 3));
    if (!nested) return build_tangent_records(*s, t->bsdf_tangents, t->h, plus, minus, inv_2h);
    // NESTED: the rows of blend / mask records are taken out first; inv_2h of such a record then carries the tangent of its constant weight
    std::vector<float> rest, weight; std::vector<uint8_t> none_r, none_w;
    if (int rc = split_nested_rows(*s, t->bsdf_tangents, nullptr, rest, weight, none_r, none_w)) return rc;
    if (int rc = build_tangent_records(*s, t->bsdf_tangents ? rest.data() : nullptr, t->h, plus, minus, inv_2h)) return rc;
    for (size_t b = 0; b < s->bsdfs.size(); ++b)
        if (s->bsdfs[b].type >= kBsdfBlend) inv_2h[b] = weight[b];
    return MTSAMD_OK;
}

// The argument block of k_forward but for the samples of a launch; uploads the scene-owned scratch on `stream`.  The host arrays must
// outlive the copies: both callers synchronise the stream before they return.
static int fill_forward(mtsamd_scene *s, const mtsamd_render_desc *d, const mtsamd_tangent_desc *t, const Job &j, int store_xyz, hipStream_t stream,
                        const std::vector<DevBsdf> &plus, const std::vector<DevBsdf> &minus, const std::vector<float> &inv_2h, ForwardParams &f) {
    Workspace &w = s->ws;
    f = ForwardParams{};
    f.rp.sv = s->view; f.rp.cam = j.cam;
    f.rp.sv.general = std::max(f.rp.sv.general, 1u);
    f.rp.base_seed = d->seed; f.rp.spp = d->sample_count;
    f.rp.crop_x = d->crop_x; f.rp.crop_y = d->crop_y; f.rp.crop_w = d->crop_width; f.rp.crop_h = d->crop_height;
    f.rp.max_depth = d->max_depth; f.rp.rr_depth = d->rr_depth;
    f.rp.rows = RowMap{ 0, d->crop_height, std::max(d->crop_height, 1), 0, 1 };
    f.rp.store_xyz = store_xyz; f.rp.out_rgba = w.out_rgba; f.rp.out_pos = w.out_pos;
    f.flags = t->flags; f.map_h = t->h;
    if (t->bsdf_tangents && !plus.empty()) {
        const size_t n = plus.size();
        if (int rc = grow(w.fw_plus, w.fw_minus, w.fw_records, n)) return rc;
        if (int rc = grow(w.fw_inv_2h, w.fw_inv_floats, n)) return rc;
        HIP_TRY(hipMemcpyAsync(w.fw_plus, plus.data(), n * sizeof(DevBsdf), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(w.fw_minus, minus.data(), n * sizeof(DevBsdf), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(w.fw_inv_2h, inv_2h.data(), n * sizeof(float), hipMemcpyHostToDevice, stream));
        f.plus = w.fw_plus; f.minus = w.fw_minus; f.inv_2h = w.fw_inv_2h;
    }
    if (t->emitter_tangents && !s->emitters.empty()) {
        const size_t n = 3 * s->emitters.size();
        if (int rc = grow(w.fw_emitters, w.fw_emitter_floats, n)) return rc;
        HIP_TRY(hipMemcpyAsync(w.fw_emitters, t->emitter_tangents, n * sizeof(float), hipMemcpyHostToDevice, stream));
        f.em_tangent = w.fw_emitters;
    }
    if (f.plus || f.em_tangent) HIP_TRY(hipStreamSynchronize(stream));      // the host arrays are free again, whatever happens next
    f.tex_tangent = t->texture_tangents_dev; f.env_tangent = t->envmap_tangent_dev;
    return 0;
}

int mtsamd_render_forward(mtsamd_scene *s, const mtsamd_render_desc *d, const mtsamd_tangent_desc *t, float *film, void *stream_) {
    std::vector<DevBsdf> plus, minus; std::vector<float> inv_2h; bool nested;
    if (int rc = check_forward(s, d, t, film, true, plus, minus, inv_2h, nested)) return rc;
    hipStream_t stream = (hipStream_t) stream_;
    Job j;
    if (int rc = open_render(j, s, d, stream, 0, 2)) return rc;      // the passes of mtsamd_render for this desc
    FilmStage fs{ j };
    if (int rc = fs.reserve(true)) return rc;
    ForwardParams f;
    if (int rc = fill_forward(s, d, t, j, 2, stream, plus, minus, inv_2h, f)) return rc;
    for (uint64_t lr0 = 0; lr0 < (uint64_t) j.rows.local_rows; lr0 += j.fp.rows_per_pass) {
        const Job::Pass p = j.pass(lr0);
        f.rp.first_ordinal = p.a; f.n_samples = p.n;
        HIP_TRY(nested ? launch_forward_nested(f, stream) : launch_forward(f, s->textured_params, stream));
        j.passes += 1;
        if (int rc = fs.begin(stream, p.lr0, p.nrows, j.fp.tile_h)) return rc;
        if (int rc = fs.put(s->ws.out_rgba, s->ws.out_pos, film)) return rc;
        if (int rc = fs.end()) return rc;
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return fs.close(nullptr);
}

int mtsamd_sample_forward(mtsamd_scene *s, const mtsamd_render_desc *d, const mtsamd_tangent_desc *t, uint64_t first, uint64_t count, float *rgba,
                          float *pos, void *stream_) {
    std::vector<DevBsdf> plus, minus; std::vector<float> inv_2h; bool nested;
    if (int rc = check_forward(s, d, t, rgba, false, plus, minus, inv_2h, nested)) return rc;
    const uint64_t total = (uint64_t) d->crop_width * d->crop_height * (uint64_t) d->sample_count;
    if (first + count > total) return fail(MTSAMD_ERR_INVALID, "sample range exceeds W*H*sample_count");
    if (count == 0) return MTSAMD_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t) stream_;
    Job j;
    if (int rc = setup_job(j, s, d, stream, count)) return rc;
    ForwardParams f;
    if (int rc = fill_forward(s, d, t, j, 0, stream, plus, minus, inv_2h, f)) return rc;
    for (uint64_t a = 0; a < count; a += j.pass_cap) {
        const uint64_t n = std::min<uint64_t>(j.pass_cap, count - a);
        f.rp.first_ordinal = first + a; f.n_samples = n;
        HIP_TRY(nested ? launch_forward_nested(f, stream) : launch_forward(f, s->textured_params, stream));
        HIP_TRY(hipMemcpyAsync(rgba + 4 * a, s->ws.out_rgba, n * sizeof(float4), hipMemcpyDeviceToDevice, stream));
        if (pos) HIP_TRY(hipMemcpyAsync(pos + 2 * a, s->ws.out_pos, n * sizeof(float2), hipMemcpyDeviceToDevice, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return MTSAMD_OK;
}

// ---- reverse-mode render: the transpose of mtsamd_render_forward (k_reverse) -------------------
int mtsamd_render_reverse(mtsamd_scene *s, const mtsamd_render_desc *d, const float *dimage, const float *film, const mtsamd_gradient_desc *g,
                          void *stream_) {
    if (!s || !d || !dimage || !film || !g) return fail(MTSAMD_ERR_INVALID, "null argument");
    if (!g->grad_bsdf_dev && !g->bsdf_wanted && !g->grad_emitters_dev && !g->grad_textures_dev && !g->grad_envmap_dev)
        return fail(MTSAMD_ERR_INVALID, "the gradient is empty: grad_bsdf_dev, grad_emitters_dev, grad_textures_dev and grad_envmap_dev are all null");
    if (!g->grad_bsdf_dev != !g->bsdf_wanted) return fail(MTSAMD_ERR_INVALID, "bsdf_wanted and grad_bsdf_dev go together: one of them is null");
    if (int rc = check_desc(d)) return rc;
    // a flag bit is known where it means something (PARAM_TEXTURES: textured BSDF parameters; NESTED: blend / mask records); elsewhere it stays refused
    bool nested = false;
    if (int rc = check_derivative_flags(*s, g->flags, true, nested)) return rc;
    if (d->integrator != 0) return fail(MTSAMD_ERR_UNSUPPORTED, "the reverse-mode render differentiates the path integrator");
    if (d->part_count > 1 || d->row_begin != 0 || d->row_end > 0) return fail(MTSAMD_ERR_UNSUPPORTED, "the reverse-mode render covers the whole crop window (no row window, no tile partition)");
    if (d->film_rgb != 1) return fail(MTSAMD_ERR_UNSUPPORTED, "the reverse-mode render differentiates an R, G, B, A, W film (film_rgb must be 1)");
    ReverseParams r{};
    if (int rc = make_filter(d->rfilter, d->rfilter_param, d->rfilter_param2, d->rfilter_analytic, r.filter)) return rc;
    if (r.filter.taps > 8) return fail(MTSAMD_ERR_UNSUPPORTED, "reconstruction filter too wide for the reverse-mode render");
    if (g->grad_envmap_dev && (s->environment < 0 || !s->d_envmap)) return fail(MTSAMD_ERR_UNSUPPORTED, "grad_envmap_dev: the scene has no envmap emitter");
    if (g->grad_textures_dev) {
        bool bitmaps = false;
        for (const DevTexture &tx : s->textures) bitmaps = bitmaps || tx.kind == 0u;
        if (!bitmaps) return fail(MTSAMD_ERR_UNSUPPORTED, "grad_textures_dev: the scene has no bitmap textures");
    }
    std::vector<ReverseSlot> slots; std::vector<uint32_t> range;
    if (!nested) { if (int rc = build_reverse_slots(*s, g->bsdf_wanted, g->h, slots, range)) return rc; }
    else {      // NESTED: the rows of blend / mask records are taken out first; a wanted constant weight becomes a slot without a pair
        std::vector<float> none_r, none_w; std::vector<uint8_t> rest, weight;
        if (int rc = split_nested_rows(*s, nullptr, g->bsdf_wanted, none_r, none_w, rest, weight)) return rc;
        if (int rc = build_reverse_slots(*s, g->bsdf_wanted ? rest.data() : nullptr, g->h, slots, range)) return rc;
        add_weight_slots(weight, slots, range);
    }
    if (slots.empty() && !g->grad_emitters_dev && !g->grad_textures_dev && !g->grad_envmap_dev)
        return fail(MTSAMD_ERR_INVALID, "the gradient is empty: no BSDF scalar is wanted and the other gradients are null");
    const bool record = !slots.empty() || g->grad_textures_dev;
    if (record && (d->max_depth < 0 || d->max_depth > 16))
        return fail(MTSAMD_ERR_UNSUPPORTED, "the reverse-mode render of BSDF scalars and texels needs a finite max_depth <= 16 (got %d)", d->max_depth);
    if (int rc = make_camera(*d, r.rp.cam)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t) stream_;
    r.rp.sv = s->view;
    r.rp.sv.general = std::max(r.rp.sv.general, 1u);
    r.rp.base_seed = d->seed; r.rp.spp = d->sample_count;
    r.rp.crop_x = d->crop_x; r.rp.crop_y = d->crop_y; r.rp.crop_w = d->crop_width; r.rp.crop_h = d->crop_height;
    r.rp.max_depth = d->max_depth; r.rp.rr_depth = d->rr_depth;
    r.rp.rows = RowMap{ 0, d->crop_height, std::max(d->crop_height, 1), 0, 1 };
    r.rp.store_xyz = 0; r.rp.out_pos = nullptr; r.rp.out_rgba = nullptr;
    r.n_samples = (uint64_t) d->crop_width * d->crop_height * (uint64_t) d->sample_count;
    r.dimage = dimage; r.film = film;
    r.flags = g->flags; r.map_h = g->h;
    r.grad_emitter = s->emitters.empty() ? nullptr : g->grad_emitters_dev;
    r.grad_tex = g->grad_textures_dev; r.grad_env = g->grad_envmap_dev;
    if (!slots.empty()) {
        Workspace &w = s->ws;
        if (int rc = grow(w.rv_slots, w.rv_slot_count, slots.size())) return rc;
        if (int rc = grow(w.rv_range, w.rv_range_words, range.size())) return rc;
        HIP_TRY(hipMemcpyAsync(w.rv_slots, slots.data(), slots.size() * sizeof(ReverseSlot), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(w.rv_range, range.data(), range.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));      // the host tables are free again
        r.slots = w.rv_slots; r.slot_range = w.rv_range; r.n_slots = (uint32_t) slots.size(); r.grad_bsdf = g->grad_bsdf_dev;
    }
    if (!record && !r.grad_emitter && !r.grad_env) return MTSAMD_OK;      // emitter gradients of a scene without emitters
    HIP_TRY(nested ? launch_reverse_nested(r, record, stream) : launch_reverse(r, record, s->textured_params, stream));
    return MTSAMD_OK;
}

int mtsamd_render_adjoint_envmap(mtsamd_scene *s, const mtsamd_render_desc *d, const float *dimage, const float *film, float *grad_envmap,
                                 void *stream_) {
    AdjointParams a{};
    if (int rc = fill_adjoint(s, d, dimage, film, a)) return rc;
    if (!grad_envmap) return fail(MTSAMD_ERR_INVALID, "null argument");
    if (s->environment < 0 || !s->d_envmap) return fail(MTSAMD_ERR_UNSUPPORTED, "the scene has no envmap emitter");
    if (s->textured_params) return fail(MTSAMD_ERR_UNSUPPORTED, "the envmap adjoint does not handle textured BSDF parameters (alpha, specular_reflectance, specular_transmittance)");
    if (s->nested_bsdfs) return fail(MTSAMD_ERR_UNSUPPORTED, "the envmap adjoint does not handle blendbsdf / mask materials");
    if (d->integrator != 0) return fail(MTSAMD_ERR_UNSUPPORTED, "the adjoint pass differentiates the path integrator");
    a.grad_env = grad_envmap;
    HIP_TRY(launch_adjoint_env(a, (hipStream_t) stream_));
    return MTSAMD_OK;
}

int mtsamd_render_adjoint_textures(mtsamd_scene *s, const mtsamd_render_desc *d, const float *dimage, const float *film, float *grad_tex,
                                   void *stream_) {
    AdjointParams a{};
    if (int rc = fill_adjoint(s, d, dimage, film, a)) return rc;
    if (!grad_tex) return fail(MTSAMD_ERR_INVALID, "null argument");
    if (d->max_depth < 0 || d->max_depth > 16)
        return fail(MTSAMD_ERR_UNSUPPORTED, "the adjoint pass needs a finite max_depth <= 16 (got %d)", d->max_depth);
    if (s->textured_params) return fail(MTSAMD_ERR_UNSUPPORTED, "the texture adjoint does not handle textured BSDF parameters (alpha, specular_reflectance, specular_transmittance)");
    if (s->nested_bsdfs) return fail(MTSAMD_ERR_UNSUPPORTED, "the texture adjoint does not handle blendbsdf / mask materials");
    if (d->integrator != 0) return fail(MTSAMD_ERR_UNSUPPORTED, "the adjoint pass differentiates the path integrator");
    a.grad_tex = grad_tex;
    HIP_TRY(launch_adjoint_tex(a, (hipStream_t) stream_));
    return MTSAMD_OK;
}

int mtsamd_render_adjoint_param_textures(mtsamd_scene *s, const mtsamd_render_desc *d, const float *dimage, const float *film, int32_t param,
                                         float h, float *grad_tex, void *stream_) {
    AdjointParams a{};
    if (int rc = fill_adjoint(s, d, dimage, film, a)) return rc;
    if (!grad_tex) return fail(MTSAMD_ERR_INVALID, "null argument");
    if (d->max_depth < 0 || d->max_depth > 16)
        return fail(MTSAMD_ERR_UNSUPPORTED, "the adjoint pass needs a finite max_depth <= 16 (got %d)", d->max_depth);
    for (const DevBsdf &b : s->bsdfs)
        if (b.type >= kBsdfBlend) return fail(MTSAMD_ERR_UNSUPPORTED, "the textured-parameter adjoint does not handle blendbsdf / mask materials");
    if (d->integrator != 0) return fail(MTSAMD_ERR_UNSUPPORTED, "the adjoint pass differentiates the path integrator");
    int slots[4], n_slots = 0;
    switch (param) {
    case MTSAMD_PARAM_ALPHA_U: slots[n_slots++] = kTexAlphaU; break;
    case MTSAMD_PARAM_ALPHA_V: slots[n_slots++] = kTexAlphaV; break;
    case MTSAMD_PARAM_ALPHA: slots[n_slots++] = kTexAlphaU; slots[n_slots++] = kTexAlphaV; break;
    case MTSAMD_PARAM_SPECULAR_REFLECTANCE: slots[n_slots++] = kTexSpec; break;
    case MTSAMD_PARAM_SPECULAR_TRANSMITTANCE: slots[n_slots++] = kTexTrans; break;
    case -1: for (int k = 0; k < 4; ++k) slots[n_slots++] = k; break;
    default:
        return fail(MTSAMD_ERR_INVALID, "parameter %d cannot hold a differentiable texture (alpha, alpha_u, alpha_v, specular_reflectance, specular_transmittance, or -1 for all)", param);
    }
    a.grad_tex = grad_tex;
    a.pg_inv_2h = h;                  // k_adjoint_param_tex: the step itself
    a.rp.sv.general = std::max(a.rp.sv.general, 1u);
    for (int k = 0; k < n_slots; ++k) {
        bool bound = false;               // a slot no record binds launches nothing; a textured `alpha` (one texture behind both) is alpha_u's
        for (const DevBsdf &b : s->bsdfs) {
            if (!(b.flags & kBsdfTexParams) || bsdf_param_texture(b, slots[k]) == 0u) continue;
            if (slots[k] == kTexAlphaV && bsdf_param_texture(b, kTexAlphaU) == bsdf_param_texture(b, kTexAlphaV)) continue;
            bound = true;
        }
        if (!bound) continue;
        a.pg_bsdf = slots[k];
        HIP_TRY(launch_adjoint_param_tex(a, (hipStream_t) stream_));
    }
    return MTSAMD_OK;
}

int mtsamd_render_adjoint_spectral(mtsamd_scene *s, const mtsamd_render_desc *d, const float *dimage, const float *film, float *grad_bsdf,
                                   float *grad_tex, void *stream_) {
    AdjointParams a{};
    if (int rc = fill_adjoint(s, d, dimage, film, a, true)) return rc;
    if (s->view.n_spectra) return fail(MTSAMD_ERR_UNSUPPORTED, "the spectral adjoint does not replay scenes with tabulated spectra (%u bound here): node values are not differentiated", s->view.n_spectra);
    if (d->max_depth < 1 || d->max_depth > 16)
        return fail(MTSAMD_ERR_UNSUPPORTED, "the adjoint pass needs a finite max_depth <= 16 (got %d)", d->max_depth);
    if (s->textured_params) return fail(MTSAMD_ERR_UNSUPPORTED, "the spectral adjoint does not handle textured BSDF parameters (alpha, specular_reflectance, specular_transmittance)");
    if (s->nested_bsdfs) return fail(MTSAMD_ERR_UNSUPPORTED, "the spectral adjoint does not handle blendbsdf / mask materials");
    if (d->integrator != 0) return fail(MTSAMD_ERR_UNSUPPORTED, "the adjoint pass differentiates the path integrator");
    if (s->bsdfs.size() > 32 && grad_bsdf) return fail(MTSAMD_ERR_UNSUPPORTED, "at most 32 BSDFs with constant-reflectance gradients");
    if (!grad_bsdf && !grad_tex) return MTSAMD_OK;
    hipStream_t stream = (hipStream_t) stream_;
    // coefficient gradients and Jacobians: [BSDF records | texels of all bitmaps in the texture-gradient layout]
    const size_t n_bsdf = s->bsdfs.size();
    const size_t n_texels = s->textures.empty() ? 0 : (s->textures.back().grad_offset + 3u * (size_t) s->textures.back().w * s->textures.back().h) / 3u;
    const size_t n_colours = n_bsdf + n_texels;
    if (!s->d_jac) { HIP_TRY(hipMalloc((void **) &s->d_jac, 9 * n_colours * sizeof(float))); s->jac_dirty = true; }
    if (!s->d_cgrad) HIP_TRY(hipMalloc((void **) &s->d_cgrad, 3 * n_colours * sizeof(float)));
    if (s->jac_dirty) {
        s->jac_bsdf.resize(9 * n_bsdf, 0.0f); s->jac_tex.resize(9 * n_texels, 0.0f);
        // d(c0, c1, c2) / d rgb -> d(a, b, c) / d rgb of the centred basis the kernel accumulates in: l = m + h u gives
        // a = h^2 c0, b = 2 m h c0 + h c1, c = m^2 c0 + m c1 + c2
        std::vector<float> centred(9 * n_colours);
        const double m = kCoeffMid, h = kCoeffHalf;
        for (size_t i = 0; i < 3 * n_colours; ++i) {
            const float *j = i < 3 * n_bsdf ? s->jac_bsdf.data() + 3 * i : s->jac_tex.data() + 3 * (i - 3 * n_bsdf);
            centred[3 * i] = (float) (h * h * j[0]);
            centred[3 * i + 1] = (float) (2.0 * m * h * j[0] + h * j[1]);
            centred[3 * i + 2] = (float) (m * m * j[0] + m * j[1] + j[2]);
        }
        HIP_TRY(hipStreamSynchronize(stream));               // an earlier launch may still read the old Jacobians
        HIP_TRY(hipMemcpy(s->d_jac, centred.data(), centred.size() * sizeof(float), hipMemcpyHostToDevice));
        s->jac_dirty = false;
    }
    HIP_TRY(hipMemsetAsync(s->d_cgrad, 0, 3 * n_colours * sizeof(float), stream));
    a.grad_bsdf = grad_bsdf ? s->d_cgrad : nullptr;
    a.grad_tex = grad_tex && n_texels ? s->d_cgrad + 3 * n_bsdf : nullptr;
    a.rp.spectral = 1;
    HIP_TRY(launch_adjoint_spectral(a, stream));
    if (a.grad_bsdf) HIP_TRY(launch_coeff_grad_to_rgb(s->d_cgrad, s->d_jac, grad_bsdf, (uint32_t) n_bsdf, stream));
    if (a.grad_tex) HIP_TRY(launch_coeff_grad_to_rgb(s->d_cgrad + 3 * n_bsdf, s->d_jac + 9 * n_bsdf, grad_tex, (uint32_t) n_texels, stream));
    return MTSAMD_OK;
}

int mtsamd_render_adjoint_spectral_emitters(mtsamd_scene *s, const mtsamd_render_desc *d, const float *dimage, const float *film,
                                            float *grad_emitters, float *grad_envmap, void *stream_) {
    AdjointParams a{};
    if (int rc = fill_adjoint(s, d, dimage, film, a, true)) return rc;
    if (s->view.n_spectra) return fail(MTSAMD_ERR_UNSUPPORTED, "the spectral adjoint does not replay scenes with tabulated spectra (%u bound here): node values are not differentiated", s->view.n_spectra);
    if (d->max_depth < 1 || d->max_depth > 16)
        return fail(MTSAMD_ERR_UNSUPPORTED, "the adjoint pass needs a finite max_depth <= 16 (got %d)", d->max_depth);
    if (s->textured_params) return fail(MTSAMD_ERR_UNSUPPORTED, "the spectral adjoint does not handle textured BSDF parameters (alpha, specular_reflectance, specular_transmittance)");
    if (s->nested_bsdfs) return fail(MTSAMD_ERR_UNSUPPORTED, "the spectral adjoint does not handle blendbsdf / mask materials");
    if (d->integrator != 0) return fail(MTSAMD_ERR_UNSUPPORTED, "the adjoint pass differentiates the path integrator");
    if (s->emitters.size() > 32 && grad_emitters) return fail(MTSAMD_ERR_UNSUPPORTED, "at most 32 emitters with radiance gradients");
    if (grad_envmap && (s->environment < 0 || !s->d_envmap)) return fail(MTSAMD_ERR_UNSUPPORTED, "the scene has no envmap emitter");
    if (!grad_emitters && !grad_envmap) return MTSAMD_OK;
    hipStream_t stream = (hipStream_t) stream_;
    // gradient rows and Jacobians: [emitters | envmap texels]
    const size_t n_em = s->emitters.size(), n_texels = s->d_envmap ? (size_t) s->env_w * s->env_h : 0, n_colours = n_em + n_texels;
    if (!s->d_ejac) { HIP_TRY(hipMalloc((void **) &s->d_ejac, 12 * n_colours * sizeof(float))); s->ejac_dirty = true; }
    if (!s->d_egrad) HIP_TRY(hipMalloc((void **) &s->d_egrad, 4 * n_colours * sizeof(float)));
    if (s->ejac_dirty) {
        std::vector<float> table(12 * n_colours, 0.0f);
        for (size_t i = 0; i < n_em; ++i) {
            const DevEmitter &e = s->emitters[i];
            const float rgb[3] = { e.r, e.g, e.b };
            if (e.pad0 != kEmitterEnvmap) emitter_jacobian_row(s->rgb2spec, rgb, table.data() + 12 * i);      // (an envmap's `radiance` is not a parameter)
        }
        for (size_t i = 0; i < n_texels && 3 * n_texels == s->env_rgb.size(); ++i)
            emitter_jacobian_row(s->rgb2spec, s->env_rgb.data() + 3 * i, table.data() + 12 * (n_em + i));
        HIP_TRY(hipStreamSynchronize(stream));               // an earlier launch may still read the old table
        HIP_TRY(hipMemcpy(s->d_ejac, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
        s->ejac_dirty = false;
    }
    HIP_TRY(hipMemsetAsync(s->d_egrad, 0, 4 * n_colours * sizeof(float), stream));
    a.grad_emitter = grad_emitters ? s->d_egrad : nullptr;
    a.grad_env = grad_envmap ? s->d_egrad + 4 * n_em : nullptr;
    a.rp.spectral = 1;
    HIP_TRY(launch_adjoint_spectral_emitters(a, stream));
    if (a.grad_emitter) HIP_TRY(launch_emitter_grad_to_rgb(s->d_egrad, s->d_ejac, grad_emitters, (uint32_t) n_em, stream));
    if (a.grad_env) HIP_TRY(launch_emitter_grad_to_rgb(s->d_egrad + 4 * n_em, s->d_ejac + 12 * n_em, grad_envmap, (uint32_t) n_texels, stream));
    return MTSAMD_OK;
}

int mtsamd_scene_update_envmap(mtsamd_scene *s, const float *rgb, int32_t rebuild_distribution) {
    if (!s || !rgb) return fail(MTSAMD_ERR_INVALID, "null argument");
    if (s->environment < 0 || !s->d_envmap) return fail(MTSAMD_ERR_UNSUPPORTED, "the scene has no envmap emitter");
    HIP_TRY(hipSetDevice(s->device));
    EnvmapHost eh;
    if (int rc = set_envmap_texels(*s, rgb, eh)) return rc;
    HIP_TRY(hipDeviceSynchronize());           // renders in flight read the old texels
    HIP_TRY(hipMemcpy(s->d_env_texels, eh.texels.data(), eh.texels.size() * sizeof(float), hipMemcpyHostToDevice));
    if (rebuild_distribution) HIP_TRY(hipMemcpy(s->d_env_warp, eh.warp.data(), eh.warp.size() * sizeof(float), hipMemcpyHostToDevice));
    return MTSAMD_OK;
}

int mtsamd_scene_texture_info(const mtsamd_scene *s, uint32_t texture, int32_t *width, int32_t *height, uint64_t *grad_offset) {
    if (!s || texture >= s->textures.size()) return fail(MTSAMD_ERR_INVALID, "invalid texture index");
    if (width) *width = s->textures[texture].w;
    if (height) *height = s->textures[texture].h;
    if (grad_offset) *grad_offset = s->textures[texture].grad_offset;
    return MTSAMD_OK;
}

int mtsamd_rgb2spec_build(const char *path, int32_t resolution, int32_t threads) {
    if (!path || resolution < 2 || resolution > 256) return fail(MTSAMD_ERR_INVALID, "invalid rgb2spec arguments");
    Rgb2Spec m;
    rgb2spec_build((uint32_t) resolution, m, threads > 0 ? (unsigned) threads : 1u);
    if (!rgb2spec_save(path, m)) return fail(MTSAMD_ERR_INVALID, "could not write '%s'", path);
    return MTSAMD_OK;
}

// the model of the host-only lookups below, loaded once per thread and path (null: could not be loaded)
static const Rgb2Spec *cached_model(const char *path) {
    static thread_local std::string cached_path;
    static thread_local Rgb2Spec cached;
    if (cached_path != path) {
        if (!rgb2spec_load(path, cached)) { cached_path.clear(); fail(MTSAMD_ERR_INVALID, "Could not load sRGB-to-spectrum upsampling model ('%s')", path); return nullptr; }
        cached_path = path;
    }
    return &cached;
}

int mtsamd_srgb_model_fetch(const char *path, const float *rgb, float *coeff) {
    if (!path || !rgb || !coeff) return fail(MTSAMD_ERR_INVALID, "null argument");
    const Rgb2Spec *m = cached_model(path);
    if (!m) return MTSAMD_ERR_INVALID;
    srgb_model_fetch(*m, rgb, coeff);
    return MTSAMD_OK;
}

int mtsamd_srgb_model_fetch_jacobian(const char *path, const float *rgb, float *jac) {
    if (!path || !rgb || !jac) return fail(MTSAMD_ERR_INVALID, "null argument");
    const Rgb2Spec *m = cached_model(path);
    if (!m) return MTSAMD_ERR_INVALID;
    srgb_model_fetch_jacobian(*m, rgb, jac);
    return MTSAMD_OK;
}

int mtsamd_srgb_emitter_fetch_jacobian(const char *path, const float *rgb, float *coeff_scale, float *jac) {
    if (!path || !rgb || !coeff_scale || !jac) return fail(MTSAMD_ERR_INVALID, "null argument");
    const Rgb2Spec *m = cached_model(path);
    if (!m) return MTSAMD_ERR_INVALID;
    double jn[9]; int ch;
    emitter_colour_jacobian(*m, rgb, coeff_scale, jn, &ch);
    for (int k = 0; k < 9; ++k) jac[k] = (float) jn[k];
    return MTSAMD_OK;
}

int mtsamd_cancel(mtsamd_scene *s) {
    if (!s) return fail(MTSAMD_ERR_INVALID, "null argument");
    s->cancel.store(1);
    return MTSAMD_OK;
}

int mtsamd_sample_radiance(mtsamd_scene *s, const mtsamd_render_desc *d, uint64_t first, uint64_t count, float *rgba,
                           float *pos, void *stream_) {
    if (int rc = check_call(s, d, rgba)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t) stream_;
    const uint64_t total = (uint64_t) d->crop_width * d->crop_height * (uint64_t) d->sample_count;
    if (first + count > total) return fail(MTSAMD_ERR_INVALID, "sample range exceeds W*H*sample_count");
    if (count == 0) return MTSAMD_OK;
    Job j;
    if (int rc = setup_job(j, s, d, stream, count)) return rc;
    j.rows = RowMap{ 0, d->crop_height, std::max(d->crop_height, 1), 0, 1 };
    j.store_xyz = 0;
    for (uint64_t a = 0; a < count; a += j.pass_cap) {
        uint64_t n = std::min<uint64_t>(j.pass_cap, count - a);
        if (int rc = trace_pass(j, first + a, n)) return rc > 0 ? fail(MTSAMD_ERR_INVALID, "timeout reached before every requested sample was traced") : rc;
        HIP_TRY(hipMemcpyAsync(rgba + 4 * a, s->ws.out_rgba, n * sizeof(float4), hipMemcpyDeviceToDevice, stream));
        if (pos) HIP_TRY(hipMemcpyAsync(pos + 2 * a, s->ws.out_pos, n * sizeof(float2), hipMemcpyDeviceToDevice, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return MTSAMD_OK;
}

int mtsamd_camera_sample_rays(const mtsamd_render_desc *d, uint64_t n, const float *sx, const float *sy, const float *apx, const float *apy, float *ox, float *oy,
                              float *oz, float *dx, float *dy, float *dz, float *mint, float *maxt, void *stream) {
    if (!d || !sx || !sy || !ox || !oy || !oz || !dx || !dy || !dz || !mint || !maxt) return fail(MTSAMD_ERR_INVALID, "null argument");
    CameraView cam;
    if (int rc = make_camera(*d, cam)) return rc;
    HIP_TRY(launch_camera_rays(cam, n, sx, sy, apx, apy, ox, oy, oz, dx, dy, dz, mint, maxt, (hipStream_t) stream));
    return MTSAMD_OK;
}

// ---- ImageBlock / Film ------------------------------------------------------------------------
int mtsamd_imageblock_put(int32_t width, int32_t height, int32_t offset_x, int32_t offset_y, int32_t channels, int32_t rfilter,
                          float rfilter_param, float rfilter_param2, int32_t analytic, int32_t border, uint64_t n, const float *pos, const float *values,
                          float *data, void *stream) {
    if (width <= 0 || height <= 0 || channels <= 0 || channels > 16 || !pos || !values || !data) return fail(MTSAMD_ERR_INVALID, "invalid ImageBlock arguments");
    FilterView f;
    if (int rc = make_filter(rfilter, rfilter_param, rfilter_param2, analytic, f)) return rc;
    if (border != 0 && border != f.border) return fail(MTSAMD_ERR_INVALID, "border must be 0 or the filter's border_size (%d)", f.border);
    HIP_TRY(launch_imageblock_put(f, width, height, offset_x, offset_y, channels, border, n, pos, values, data, (hipStream_t) stream));
    return MTSAMD_OK;
}

int mtsamd_imageblock_put_block(const float *src, int32_t sw, int32_t sh, int32_t sox, int32_t soy, int32_t sb, float *dst, int32_t dw,
                                int32_t dh, int32_t dox, int32_t doy, int32_t db, int32_t channels, void *stream) {
    if (!src || !dst || sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || channels <= 0 || sb < 0 || db < 0)
        return fail(MTSAMD_ERR_INVALID, "invalid ImageBlock arguments");
    HIP_TRY(launch_put_block(src, sw, sh, sox, soy, sb, dst, dw, dh, dox, doy, db, channels, (hipStream_t) stream));
    return MTSAMD_OK;
}

int mtsamd_rfilter_info(int32_t rfilter, float param, float param2, float *table32, float *radius, int32_t *border) {
    FilterView f;
    if (int rc = make_filter(rfilter, param, param2, 0, f)) return rc;
    if (table32) std::memcpy(table32, f.table, sizeof(float) * 32);
    if (radius) *radius = f.radius;
    if (border) *border = f.border;
    return MTSAMD_OK;
}

int mtsamd_film_develop(const float *xyzaw, uint64_t n, float *rgba, void *stream) {
    if (!xyzaw || !rgba) return fail(MTSAMD_ERR_INVALID, "null argument");
    HIP_TRY(launch_film_develop(xyzaw, n, rgba, (hipStream_t) stream));
    return MTSAMD_OK;
}

int mtsamd_libm_eval(int32_t fn, uint64_t n, const float *x, const float *y, float *out, void *stream) {
    if (fn < 0 || fn > 9) return fail(MTSAMD_ERR_INVALID, "libm_eval: unknown function %d", fn);
    if (n && (!x || !out || (fn == 7 && !y))) return fail(MTSAMD_ERR_INVALID, "libm_eval: null buffer");
    if (n >> 40) return fail(MTSAMD_ERR_INVALID, "libm_eval: too many arguments");
    HIP_TRY(launch_libm_eval(fn, n, x, y, out, (hipStream_t) stream));
    return MTSAMD_OK;
}

int mtsamd_spectrum_mean(const mtsamd_spectrum_desc *desc, float *mean) {
    if (!desc || !mean) return fail(MTSAMD_ERR_INVALID, "null argument");
    if (desc->type == MTSAMD_SPECTRUM_BLACKBODY) return fail(MTSAMD_ERR_UNSUPPORTED, "mean() of a blackbody spectrum is not used by this backend (emitters only)");
    double integral = 0.0;
    if (int rc = check_spectrum(*desc, 0, &integral)) return rc;
    *mean = spectrum_table_mean(integral);
    return MTSAMD_OK;
}

int mtsamd_spectrum_eval(const mtsamd_spectrum_desc *desc, uint64_t n, const float *lambda, float *out, void *stream) {
    if (!desc || (n && (!lambda || !out))) return fail(MTSAMD_ERR_INVALID, "null argument");
    if (int rc = check_spectrum(*desc, 0, nullptr)) return rc;
    std::vector<DevSpectrum> headers; std::vector<float> data;
    build_spectrum_pool(desc, 1, headers, data);
    std::vector<float> block(sizeof(DevSpectrum) / sizeof(float) + data.size());
    std::memcpy(block.data(), headers.data(), sizeof(DevSpectrum));
    if (!data.empty()) std::memcpy(block.data() + sizeof(DevSpectrum) / sizeof(float), data.data(), data.size() * sizeof(float));
    float *d_block = nullptr;
    HIP_TRY(hipMalloc((void **) &d_block, block.size() * sizeof(float)));
    hipError_t e = hipMemcpy(d_block, block.data(), block.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_spectrum_eval(reinterpret_cast<const DevSpectrum *>(d_block), d_block + sizeof(DevSpectrum) / sizeof(float), n, lambda, out, (hipStream_t) stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t) stream);      // the pool is freed below
    (void) hipFree(d_block);
    if (e != hipSuccess) return fail(MTSAMD_ERR_DEVICE, "mtsamd_spectrum_eval: %s", hipGetErrorString(e));
    return MTSAMD_OK;
}

} // extern "C"

// Stand-alone driver of the host-only scene builder (mitsuba2_amd/csrc/scene_build.h) for tests/test_scene_build_cpu.py: reads scene
// descriptions as lines of `record key=v1,v2,...`, builds each with build_host_scene, applies the setters listed after it and dumps
// what the host holds as hex words.  It decides nothing: every expectation lives in the test.
//   argv[1]: the description file; argv[2]: the rgb2spec coefficient file of the spectral scenes
#include "scene_build.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <map>
#include <sstream>
#include <string>

using namespace mtsamd;
using Values = std::vector<double>;
using Args = std::map<std::string, Values>;

static void put(float &d, const Values &v) { d = (float) v.at(0); }
static void put(int32_t &d, const Values &v) { d = (int32_t) v.at(0); }
static void put(uint32_t &d, const Values &v) { d = (uint32_t) v.at(0); }
template <size_t N> static void put(float (&d)[N], const Values &v) { for (size_t i = 0; i < N; ++i) d[i] = (float) v.at(i); }
template <size_t N> static void put(int32_t (&d)[N], const Values &v) { for (size_t i = 0; i < N; ++i) d[i] = (int32_t) v.at(i); }
#define FIELD(T, name) { #name, [](T &d, const Values &v) { put(d.name, v); } }
template <typename T> using Fields = std::map<std::string, std::function<void(T &, const Values &)>>;
static const Fields<mtsamd_bsdf_desc> kBsdf = {
    FIELD(mtsamd_bsdf_desc, type), FIELD(mtsamd_bsdf_desc, reflectance), FIELD(mtsamd_bsdf_desc, texture), FIELD(mtsamd_bsdf_desc, twosided),
    FIELD(mtsamd_bsdf_desc, specular_reflectance), FIELD(mtsamd_bsdf_desc, specular_transmittance), FIELD(mtsamd_bsdf_desc, eta), FIELD(mtsamd_bsdf_desc, k),
    FIELD(mtsamd_bsdf_desc, int_ior), FIELD(mtsamd_bsdf_desc, ext_ior), FIELD(mtsamd_bsdf_desc, alpha_u), FIELD(mtsamd_bsdf_desc, alpha_v),
    FIELD(mtsamd_bsdf_desc, distribution), FIELD(mtsamd_bsdf_desc, sample_visible), FIELD(mtsamd_bsdf_desc, nonlinear), FIELD(mtsamd_bsdf_desc, uniform_mask),
    FIELD(mtsamd_bsdf_desc, nested) };
static const Fields<mtsamd_emitter_desc> kEmitter = {
    FIELD(mtsamd_emitter_desc, type), FIELD(mtsamd_emitter_desc, radiance), FIELD(mtsamd_emitter_desc, envmap_width), FIELD(mtsamd_emitter_desc, envmap_height),
    FIELD(mtsamd_emitter_desc, envmap_scale), FIELD(mtsamd_emitter_desc, to_world), FIELD(mtsamd_emitter_desc, cutoff_angle), FIELD(mtsamd_emitter_desc, beam_width) };
static const Fields<mtsamd_texture_desc> kTexture = {
    FIELD(mtsamd_texture_desc, width), FIELD(mtsamd_texture_desc, height), FIELD(mtsamd_texture_desc, kind), FIELD(mtsamd_texture_desc, color0),
    FIELD(mtsamd_texture_desc, color1), FIELD(mtsamd_texture_desc, to_uv) };
static const Fields<mtsamd_spectrum_desc> kSpectrum = {
    FIELD(mtsamd_spectrum_desc, type), FIELD(mtsamd_spectrum_desc, lambda_min), FIELD(mtsamd_spectrum_desc, lambda_max), FIELD(mtsamd_spectrum_desc, temperature) };
static const Fields<mtsamd_spectrum_binding> kBinding = {
    FIELD(mtsamd_spectrum_binding, target), FIELD(mtsamd_spectrum_binding, index), FIELD(mtsamd_spectrum_binding, param), FIELD(mtsamd_spectrum_binding, spectrum) };

template <typename T> static T filled(const Fields<T> &fields, const Args &a) {       // keys the struct does not have (data, values, ...) are the caller's
    T d{};
    for (const auto &kv : a) { auto f = fields.find(kv.first); if (f != fields.end()) f->second(d, kv.second); }
    return d;
}
static std::vector<float> floats(const Args &a, const char *key) {
    auto it = a.find(key);
    return it == a.end() ? std::vector<float>() : std::vector<float>(it->second.begin(), it->second.end());
}
static double number(const Args &a, const char *key, double fallback) { auto it = a.find(key); return it == a.end() ? fallback : it->second.at(0); }

template <typename T> static void dump(const char *name, const T *data, size_t n) {
    std::printf("%s", name);
    const size_t words = n * sizeof(T) / 4;
    for (size_t i = 0; i < words; ++i) { uint32_t w; std::memcpy(&w, reinterpret_cast<const char *>(data) + 4 * i, 4); std::printf(" %08x", w); }
    std::printf("\n");
}
template <typename T> static void dump(const char *name, const std::vector<T> &v) { dump(name, v.data(), v.size()); }

// A description under construction.  Mesh i: `tris` disjoint triangles (f, 0, i) (f + 1, 0, i) (f, 1, i); the faces listed in `degenerate`
// collapse to one vertex (zero area); badface: one index past the vertices; empty: no faces at all
struct Scene {
    std::vector<std::vector<float>> pos, nrm, uv, tex_data, env_data, sp_values, sp_nodes;
    std::vector<std::vector<uint32_t>> faces;
    std::vector<mtsamd_mesh_desc> meshes;
    std::vector<mtsamd_bsdf_desc> bsdfs;
    std::vector<mtsamd_emitter_desc> emitters;
    std::vector<mtsamd_texture_desc> textures;
    std::vector<mtsamd_spectrum_desc> spectra;
    std::vector<mtsamd_spectrum_binding> bindings;
    int spectral = 0, no_model = 0;

    void add_mesh(const Args &a) {
        const uint32_t n = (uint32_t) number(a, "tris", 1), i = (uint32_t) meshes.size();
        std::vector<float> p, nn, t; std::vector<uint32_t> f;
        for (uint32_t k = 0; k < n; ++k) {
            const float v[9] = { (float) k, 0, (float) i, (float) k + 1, 0, (float) i, (float) k, 1, (float) i };
            p.insert(p.end(), v, v + 9);
            for (int j = 0; j < 3; ++j) { nn.insert(nn.end(), { 0.0f, 0.0f, 1.0f }); t.insert(t.end(), { v[3 * j], v[3 * j + 1] }); f.push_back(3 * k + j); }
        }
        for (double d : a.count("degenerate") ? a.at("degenerate") : Values()) f[3 * (size_t) d + 1] = f[3 * (size_t) d + 2] = f[3 * (size_t) d];
        if (number(a, "badface", 0)) f.back() = 3 * n;
        pos.push_back(p); nrm.push_back(nn); uv.push_back(t); faces.push_back(f);
        mtsamd_mesh_desc m{};
        m.vertex_count = 3 * n; m.face_count = number(a, "empty", 0) ? 0 : n;
        m.bsdf = (int32_t) number(a, "bsdf", 0); m.emitter = (int32_t) number(a, "emitter", -1);
        meshes.push_back(m);
        if (!number(a, "normals", 0)) nrm.back().clear();
        if (!number(a, "uv", 0)) uv.back().clear();
    }
    mtsamd_scene_desc desc(const char *model) {
        for (size_t i = 0; i < meshes.size(); ++i) {
            meshes[i].positions = pos[i].data(); meshes[i].faces = faces[i].data();
            meshes[i].normals = nrm[i].empty() ? nullptr : nrm[i].data(); meshes[i].texcoords = uv[i].empty() ? nullptr : uv[i].data();
        }
        for (size_t i = 0; i < textures.size(); ++i) textures[i].data = tex_data[i].empty() ? nullptr : tex_data[i].data();
        for (size_t i = 0; i < emitters.size(); ++i) emitters[i].envmap_data = env_data[i].empty() ? nullptr : env_data[i].data();
        for (size_t i = 0; i < spectra.size(); ++i) {
            spectra[i].values = sp_values[i].data(); spectra[i].wavelengths = sp_nodes[i].empty() ? nullptr : sp_nodes[i].data();
            spectra[i].size = (uint32_t) sp_values[i].size();
        }
        mtsamd_scene_desc d{};
        d.meshes = meshes.data(); d.mesh_count = (uint32_t) meshes.size();
        d.bsdfs = bsdfs.data(); d.bsdf_count = (uint32_t) bsdfs.size();
        d.emitters = emitters.data(); d.emitter_count = (uint32_t) emitters.size();
        d.textures = textures.data(); d.texture_count = (uint32_t) textures.size();
        d.spectral = spectral; d.rgb2spec_path = spectral && !no_model ? model : (spectral ? "/nonexistent/model.coeff" : nullptr);
        return d;
    }
};

// the setters, as api.cpp drives them: the host half, then (here) the texels that would be pushed
static int apply(const std::string &op, const Args &a, HostScene &hs, std::vector<std::vector<float>> &texels, EnvmapHost &env) {
    SceneState &st = hs.state;
    std::vector<float> v = floats(a, "value");
    if (op == "set_reflectance") return set_bsdf_reflectance(st, (uint32_t) number(a, "bsdf", 0), v.data());
    if (op == "set_param") return set_bsdf_param(st, (uint32_t) number(a, "bsdf", 0), (int32_t) number(a, "kind", 0), v.data());
    if (op == "set_radiance") return set_emitter_radiance(st, (uint32_t) number(a, "emitter", 0), v.data());
    if (op == "set_envmap") return set_envmap_texels(st, v.data(), env);
    const uint32_t t = (uint32_t) number(a, "texture", 0);       // set_texture
    texels[t] = v;
    if (!st.spectral && !texture_feeds_lobe_weight(st, t)) return 0;
    std::vector<float> coeffs; std::vector<uint32_t> changed;
    set_texture_texels(st, t, v.data(), coeffs, changed);
    if (st.spectral) texels[t] = coeffs;
    dump("changed_bsdfs", changed);
    return 0;
}

static void run(Scene &sc, const std::vector<std::pair<std::string, Args>> &ops, const char *model) {
    const mtsamd_scene_desc d = sc.desc(model);
    HostScene hs;
    int rc = build_host_scene(&d, sc.spectra.data(), (uint32_t) sc.spectra.size(), sc.bindings.data(), (uint32_t) sc.bindings.size(), BuildOptions{}, hs);
    std::vector<std::vector<float>> texels(hs.tex_src.size());
    for (size_t t = 0; rc == 0 && t < texels.size(); ++t)
        if (hs.tex_src[t]) texels[t].assign(hs.tex_src[t], hs.tex_src[t] + 3 * (size_t) hs.state.textures[t].w * hs.state.textures[t].h);
    for (size_t i = 0; rc == 0 && i < ops.size(); ++i) rc = apply(ops[i].first, ops[i].second, hs, texels, hs.env);
    std::printf("rc %d\nmessage %s\n", rc, rc ? last_error() : "");
    if (rc) return;
    const SceneState &st = hs.state;
    const uint32_t flags[] = { st.general_bsdfs, st.nested_bsdfs, st.non_diffuse_bsdfs, st.delta_emitters, st.spectral, (uint32_t) st.environment,
                               hs.flat, hs.n_pairs, hs.n_clusters, hs.n_spectra, st.n_prims, st.n_shapes, hs.has_envmap };
    dump("flags", flags, 13);
    const uint32_t bvh[] = { st.bvh.root, st.bvh.wroot, st.bvh.wdepth, st.bvh.n_nodes, st.bvh.n_slots };
    dump("bvh", bvh, 5);
    // LDS demand of the scene as a flat one (kernels.h; whatever hs.flat says, so that the test sees both sides of the cap), and the BVH4 a demoted scene walks
    SceneView sv = {};
    sv.flat = 1u; sv.n_prims = st.n_prims; sv.n_pairs = (st.n_prims + 1) / 2;
    for (uint32_t k = 0; k < sv.n_pairs; ++k) sv.n_clusters += k == 0 || hs.prim_shape[2 * k] != hs.prim_shape[2 * (k - 1)];
    sv.n_shapes = st.n_shapes; sv.n_bsdfs = (uint32_t) st.bsdfs.size(); sv.n_emitters = (uint32_t) st.emitters.size();
    const uint32_t limits[] = { (uint32_t) lds_bytes(sv, 64u), (uint32_t) lds_bytes(sv, 256u), (uint32_t) shade_ring_lds_bytes(sv, false, 4u),
                                (uint32_t) shade_ring_lds_bytes(sv, true, 1024u), (uint32_t) flat_launch_lds_max(sv, false),
                                (uint32_t) flat_launch_lds_max(sv, true), (uint32_t) kFlatLdsCap, st.bvh.n_wnodes, st.bvh.wdepth };
    dump("limits", limits, 9);
    dump("tri_pos", hs.tri_pos); dump("tri_nrm", hs.tri_nrm); dump("tri_uv", hs.tri_uv); dump("prim_shape", hs.prim_shape); dump("shapes", hs.shapes);
    dump("area_pmf", hs.area_pmf); dump("area_cdf", hs.area_cdf);
    dump("bsdfs", st.bsdfs); dump("emitters", st.emitters); dump("textures", st.textures);
    dump("pool", hs.bsdf_block.data() + st.bsdfs.size(), hs.bsdf_block.size() - st.bsdfs.size());
    dump("spec_mean", st.spec_mean); dump("diff_mean", st.diff_mean); dump("jac_bsdf", st.jac_bsdf); dump("jac_tex", st.jac_tex); dump("env_rgb", st.env_rgb);
    dump("flat_recs", hs.flat_recs); dump("pair_recs", hs.pair_recs);
    for (size_t t = 0; t < texels.size(); ++t) dump(("texels" + std::to_string(t)).c_str(), texels[t]);
    dump("env_texels", hs.env.texels); dump("env_warp", hs.env.warp); dump("dev_env", &hs.dev_env, 1);
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    Scene sc; std::vector<std::pair<std::string, Args>> ops;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string rec, tok;
        if (!(ls >> rec)) continue;
        Args a;
        while (ls >> tok) {
            const size_t eq = tok.find('=');
            Values v; std::istringstream vs(tok.substr(eq + 1)); std::string item;
            while (std::getline(vs, item, ',')) v.push_back(std::strtod(item.c_str(), nullptr));
            a[tok.substr(0, eq)] = v;
        }
        if (rec == "scene") { sc = Scene(); ops.clear(); std::printf("scene %s\n", line.substr(6).c_str()); }
        else if (rec == "spectral") { sc.spectral = 1; sc.no_model = (int) number(a, "no_model", 0); }
        else if (rec == "mesh") sc.add_mesh(a);
        else if (rec == "bsdf") sc.bsdfs.push_back(filled(kBsdf, a));
        else if (rec == "emitter") { sc.emitters.push_back(filled(kEmitter, a)); sc.env_data.push_back(floats(a, "data")); }
        else if (rec == "texture") { sc.textures.push_back(filled(kTexture, a)); sc.tex_data.push_back(floats(a, "data")); }
        else if (rec == "spectrum") { sc.spectra.push_back(filled(kSpectrum, a)); sc.sp_values.push_back(floats(a, "values")); sc.sp_nodes.push_back(floats(a, "wavelengths")); }
        else if (rec == "binding") sc.bindings.push_back(filled(kBinding, a));
        else if (rec == "end") run(sc, ops, argv[2]);
        else ops.emplace_back(rec, a);
    }
    return 0;
}

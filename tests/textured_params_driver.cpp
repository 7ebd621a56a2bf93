// Stand-alone driver of the host-only scene builder (mitsuba2_amd/csrc/scene_build.h) for tests/test_textured_params_cpu.py: scenes
// with textured BSDF parameters (mtsamd_texture_binding).  Reads lines of `record key=v1,v2,...`:
//   scene NAME | spectral | mesh bsdf=B [uv=1] | bsdf type=T ... | texture kind=K [width= height= data=] | binding bsdf= param= texture= |
//   set_param bsdf= kind= value= | end
// builds each scene with build_host_scene, applies the setters listed after it and dumps what the host holds about the bindings as hex
// words.  It decides nothing: every expectation lives in the test.  argv[1]: the description file; argv[2]: the rgb2spec coefficient file.
#include "scene_build.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>

using namespace mtsamd;
using Values = std::vector<double>;
using Args = std::map<std::string, Values>;

static double number(const Args &a, const char *key, double fallback) { auto it = a.find(key); return it == a.end() ? fallback : it->second.at(0); }
static void triple(float (&d)[3], const Args &a, const char *key, float fallback) {
    auto it = a.find(key);
    for (int i = 0; i < 3; ++i) d[i] = it == a.end() ? fallback : (float) it->second.at(it->second.size() == 1 ? 0 : i);
}
template <typename T> static void dump(const char *name, const T *data, size_t n) {
    std::printf("%s", name);
    for (size_t i = 0; i < n * sizeof(T) / 4; ++i) { uint32_t w; std::memcpy(&w, reinterpret_cast<const char *>(data) + 4 * i, 4); std::printf(" %08x", w); }
    std::printf("\n");
}

struct Scene {
    std::vector<std::vector<float>> pos, uv, tex_data;
    std::vector<std::vector<uint32_t>> faces;
    std::vector<mtsamd_mesh_desc> meshes;
    std::vector<mtsamd_bsdf_desc> bsdfs;
    std::vector<mtsamd_texture_desc> textures;
    std::vector<mtsamd_texture_binding> bindings;
    std::vector<Args> sets;
    int spectral = 0, null_bindings = 0;
};

static void run(Scene &sc, const char *model) {
    for (size_t i = 0; i < sc.meshes.size(); ++i) {
        sc.meshes[i].positions = sc.pos[i].data(); sc.meshes[i].faces = sc.faces[i].data();
        sc.meshes[i].texcoords = sc.uv[i].empty() ? nullptr : sc.uv[i].data();
    }
    for (size_t i = 0; i < sc.textures.size(); ++i) sc.textures[i].data = sc.tex_data[i].empty() ? nullptr : sc.tex_data[i].data();
    mtsamd_scene_desc d{};
    d.meshes = sc.meshes.data(); d.mesh_count = (uint32_t) sc.meshes.size();
    d.bsdfs = sc.bsdfs.data(); d.bsdf_count = (uint32_t) sc.bsdfs.size();
    d.textures = sc.textures.data(); d.texture_count = (uint32_t) sc.textures.size();
    d.spectral = sc.spectral; d.rgb2spec_path = sc.spectral ? model : nullptr;
    HostScene hs;
    int rc = build_host_scene(&d, nullptr, 0, nullptr, 0, BuildOptions{}, hs, sc.null_bindings ? nullptr : sc.bindings.data(),
                              sc.null_bindings ? 1u : (uint32_t) sc.bindings.size());
    for (size_t i = 0; rc == 0 && i < sc.sets.size(); ++i) {
        const Args &a = sc.sets[i];
        float v[3]; triple(v, a, "value", 0.0f);
        rc = set_bsdf_param(hs.state, (uint32_t) number(a, "bsdf", 0), (int32_t) number(a, "kind", 0), v);
    }
    std::printf("rc %d\nmessage %s\n", rc, rc ? last_error() : "");
    if (rc) return;
    const SceneState &st = hs.state;
    const uint32_t flags[] = { st.general_bsdfs, st.nested_bsdfs, st.textured_params, hs.flat, (uint32_t) st.textures.size() };
    dump("flags", flags, 5);
    std::vector<uint32_t> words;       // per record: type, flags, nested0, nested1, then (1 + texture) of the four slots
    for (const DevBsdf &b : st.bsdfs) {
        words.insert(words.end(), { (uint32_t) b.type, b.flags, b.nested0, b.nested1 });
        for (int slot = 0; slot < 4; ++slot) words.push_back(bsdf_param_texture(b, slot));
    }
    dump("records", words.data(), words.size());
    dump("bsdfs", st.bsdfs.data(), st.bsdfs.size());
    const uint32_t size = (uint32_t) sizeof(DevBsdf);
    dump("record_size", &size, 1);
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    Scene sc;
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
        if (rec == "scene") { sc = Scene(); std::printf("scene %s\n", line.substr(6).c_str()); }
        else if (rec == "spectral") sc.spectral = 1;
        else if (rec == "null_bindings") sc.null_bindings = 1;
        else if (rec == "mesh") {
            const float i = (float) sc.meshes.size();
            sc.pos.push_back({ 0, 0, i, 1, 0, i, 0, 1, i }); sc.faces.push_back({ 0, 1, 2 });
            sc.uv.push_back(number(a, "uv", 0) ? std::vector<float>{ 0, 0, 1, 0, 0, 1 } : std::vector<float>());
            mtsamd_mesh_desc m{};
            m.vertex_count = 3; m.face_count = 1; m.bsdf = (int32_t) number(a, "bsdf", 0); m.emitter = -1;
            sc.meshes.push_back(m);
        } else if (rec == "bsdf") {
            mtsamd_bsdf_desc b{};
            b.type = (int32_t) number(a, "type", 0); b.texture = (int32_t) number(a, "texture", -1); b.twosided = (int32_t) number(a, "twosided", 0);
            triple(b.reflectance, a, "reflectance", 0.5f); triple(b.specular_reflectance, a, "specular_reflectance", 1.0f);
            triple(b.specular_transmittance, a, "specular_transmittance", 1.0f); triple(b.eta, a, "eta", 0.0f); triple(b.k, a, "k", 1.0f);
            b.int_ior = (float) number(a, "int_ior", 1.5046); b.ext_ior = (float) number(a, "ext_ior", 1.000277);
            b.alpha_u = (float) number(a, "alpha_u", 0.1); b.alpha_v = (float) number(a, "alpha_v", 0.1);
            b.distribution = (int32_t) number(a, "distribution", 0); b.sample_visible = 1; b.uniform_mask = (int32_t) number(a, "uniform_mask", 0);
            b.nested[0] = (int32_t) number(a, "nested0", -1); b.nested[1] = (int32_t) number(a, "nested1", -1);
            sc.bsdfs.push_back(b);
        } else if (rec == "texture") {
            mtsamd_texture_desc t{};
            t.kind = (int32_t) number(a, "kind", 1); t.width = (int32_t) number(a, "width", 0); t.height = (int32_t) number(a, "height", 0);
            triple(t.color0, a, "color0", 0.4f); triple(t.color1, a, "color1", 0.2f);
            sc.textures.push_back(t);
            auto it = a.find("data");
            sc.tex_data.push_back(it == a.end() ? std::vector<float>() : std::vector<float>(it->second.begin(), it->second.end()));
        } else if (rec == "binding") {
            sc.bindings.push_back(mtsamd_texture_binding{ (uint32_t) number(a, "bsdf", 0), (int32_t) number(a, "param", 0), (int32_t) number(a, "texture", 0) });
        } else if (rec == "set_param") sc.sets.push_back(a);
        else if (rec == "end") run(sc, argv[2]);
    }
    return 0;
}

// Stand-alone driver of the host half of mtsamd_scene_set_vertex_positions (mitsuba2_amd/csrc/scene_build.h, bvh.h) for
// tests/test_vertex_update_cpu.py and the array comparisons of tests/test_gpu_vertex_update.py: reads a scene and a list of commands
// (tests/vertex_moves.py writes them), builds the scene with build_host_scene, applies vertex moves through set_vertex_positions and
// dumps what the host holds as hex words.  It decides nothing: every expectation lives in the tests.
//   bsdfs N                                   N one-sided diffuse records
//   emitter TYPE CUTOFF BEAM W0 .. W15        to_world as hex words
//   mesh BSDF EMITTER NV NF HAS_NORMALS       then lines `P words`, `F indices`, and `N words` with normals
//   build                                     build_host_scene of the description so far; the live scene
//   move SHAPE HAS_NORMALS                    then `P words` (and `N words`): set_vertex_positions on the live scene; prints rc, message
//   dump LABEL                                the live scene's arrays
//   fresh LABEL                               the arrays of a scene built from the description as the accepted moves left it
//   rebuild LABEL                             refit_bvh of the live scene with its own positions (must change nothing), then dump
//   encode LABEL                              refit_encode.h, the device's restatement, against the live scene's node arrays
#include "scene_build.h"
#include "refit_encode.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

using namespace mtsamd;

template <typename T> static void dump(const char *label, const char *name, const T *data, size_t n) {
    std::printf("%s.%s", label, name);
    const size_t words = n * sizeof(T) / 4;
    for (size_t i = 0; i < words; ++i) { uint32_t w; std::memcpy(&w, reinterpret_cast<const char *>(data) + 4 * i, 4); std::printf(" %08x", w); }
    std::printf("\n");
}
template <typename T> static void dump(const char *label, const char *name, const std::vector<T> &v) { dump(label, name, v.data(), v.size()); }

struct Description {
    std::vector<std::vector<float>> pos, nrm;
    std::vector<std::vector<uint32_t>> faces;
    std::vector<mtsamd_mesh_desc> meshes;
    std::vector<mtsamd_bsdf_desc> bsdfs;
    std::vector<mtsamd_emitter_desc> emitters;
    mtsamd_scene_desc desc() {
        for (size_t i = 0; i < meshes.size(); ++i) {
            meshes[i].positions = pos[i].data(); meshes[i].faces = faces[i].data();
            meshes[i].normals = nrm[i].empty() ? nullptr : nrm[i].data(); meshes[i].texcoords = nullptr;
        }
        mtsamd_scene_desc d{};
        d.meshes = meshes.data(); d.mesh_count = (uint32_t) meshes.size();
        d.bsdfs = bsdfs.data(); d.bsdf_count = (uint32_t) bsdfs.size();
        d.emitters = emitters.data(); d.emitter_count = (uint32_t) emitters.size();
        return d;
    }
};

static std::vector<float> hex_floats(std::istringstream &ls) {
    std::vector<float> v; std::string tok;
    while (ls >> tok) { const uint32_t w = (uint32_t) std::strtoul(tok.c_str(), nullptr, 16); float f; std::memcpy(&f, &w, 4); v.push_back(f); }
    return v;
}
static std::vector<float> float_line(std::ifstream &in, const char *tag) {
    std::string line, t; std::getline(in, line);
    std::istringstream ls(line); ls >> t;
    if (t != tag) { std::fprintf(stderr, "expected a %s line\n", tag); std::exit(2); }
    return hex_floats(ls);
}

static void dump_scene(const char *label, const HostScene &hs) {
    const SceneState &st = hs.state;
    const BvhOutput &b = st.bvh;
    const uint32_t counts[] = { b.root, b.wroot, b.wdepth, b.n_nodes, b.n_wnodes, b.n_slots, b.depth, hs.flat, hs.n_pairs, hs.n_clusters, st.n_prims };
    dump(label, "counts", counts, 11);
    dump(label, "nodes", b.nodes); dump(label, "qnodes", b.qnodes); dump(label, "wnodes", b.wnodes); dump(label, "wnodes_h", b.wnodes_h);
    dump(label, "wnodes_p", b.wnodes_p); dump(label, "tris", b.tris); dump(label, "bbox", b.bbox, 6);
    const float grid[6] = { b.q_lo[0], b.q_lo[1], b.q_lo[2], b.q_step[0], b.q_step[1], b.q_step[2] };
    dump(label, "grid", grid, 6);
    dump(label, "tri_pos", hs.tri_pos); dump(label, "tri_nrm", hs.tri_nrm); dump(label, "area_pmf", hs.area_pmf); dump(label, "area_cdf", hs.area_cdf);
    dump(label, "emitters", st.emitters); dump(label, "flat_recs", hs.flat_recs); dump(label, "pair_recs", hs.pair_recs);
    const RefitTable &rt = b.refit;
    dump(label, "rt_left", rt.left); dump(label, "rt_right", rt.right); dump(label, "rt_ref2", rt.ref2); dump(label, "rt_ref4", rt.ref4);
    dump(label, "rt_height", rt.height); dump(label, "rt_node_child", rt.node_child); dump(label, "rt_wide_child", rt.wide_child);
    dump(label, "rt_slot_prim", rt.slot_prim); dump(label, "rt_boxes", rt.boxes);
    const int32_t root = rt.root; dump(label, "rt_root", &root, 1);
}

// the device's per-box arithmetic, run on the host over every child box and compared word for word with what emit_bvh wrote
static void check_encoding(const char *label, const HostScene &hs) {
    const BvhOutput &b = hs.state.bvh;
    const RefitTable &rt = b.refit;
    RefitGrid g{};
    float q_lo[3], q_step[3];
    scene_grid(b.bbox, &g.extent, q_lo, q_step);
    for (int k = 0; k < 3; ++k) { g.glo[k] = (double) q_lo[k]; g.gstep[k] = (double) q_step[k]; }
    uint64_t mismatches = std::memcmp(q_lo, b.q_lo, 12) != 0 || std::memcmp(q_step, b.q_step, 12) != 0, boxes = 0;
    auto encode = [&](int32_t t, float lo[3], float hi[3], uint32_t ql[3], uint32_t qh[3]) {
        for (int k = 0; k < 3; ++k) {
            enc_padded(rt.boxes[6 * (size_t) t + k], rt.boxes[6 * (size_t) t + 3 + k], g.extent, &lo[k], &hi[k]);
            ql[k] = enc_qlo(lo[k], g.glo[k], g.gstep[k]); qh[k] = enc_qhi(hi[k], g.glo[k], g.gstep[k]);
        }
        ++boxes;
    };
    for (size_t i = 0; i < rt.node_child.size(); ++i) {
        float lo[3], hi[3]; uint32_t ql[3], qh[3];
        encode(rt.node_child[i], lo, hi, ql, qh);
        const float *q = b.nodes.data() + 16 * (i >> 1) + 6 * (i & 1);
        const uint32_t *w = b.qnodes.data() + 8 * (i >> 1) + 3 * (i & 1);
        for (int k = 0; k < 3; ++k)
            mismatches += std::memcmp(&q[k], &lo[k], 4) != 0 || std::memcmp(&q[3 + k], &hi[k], 4) != 0 || w[k] != enc_word16(ql[k], qh[k]);
    }
    for (size_t i = 0; i < rt.wide_child.size(); ++i) {
        if (rt.wide_child[i] < 0) continue;
        float lo[3], hi[3]; uint32_t ql[3], qh[3];
        encode(rt.wide_child[i], lo, hi, ql, qh);
        for (int k = 0; k < 3; ++k)
            mismatches += b.wnodes[4 * i + k] != enc_word16(ql[k], qh[k]) || b.wnodes_h[4 * i + k] != enc_word_half(ql[k], qh[k]) ||
                          b.wnodes_p[4 * i + k] != enc_word_p15(ql[k], qh[k]);
    }
    const uint32_t out[2] = { (uint32_t) boxes, (uint32_t) mismatches };
    dump(label, "encode", out, 2);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    Description sc;
    HostScene live;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string rec;
        if (!(ls >> rec)) continue;
        if (rec == "bsdfs") {
            size_t n; ls >> n;
            mtsamd_bsdf_desc b{};
            b.type = MTSAMD_BSDF_DIFFUSE; b.texture = -1; b.nested[0] = b.nested[1] = -1;
            b.reflectance[0] = b.reflectance[1] = b.reflectance[2] = 0.5f;
            sc.bsdfs.assign(n, b);
        } else if (rec == "emitter") {
            mtsamd_emitter_desc e{};
            ls >> e.type >> e.cutoff_angle >> e.beam_width;
            const std::vector<float> m = hex_floats(ls);
            for (int k = 0; k < 16; ++k) e.to_world[k] = m.at(k);
            e.radiance[0] = e.radiance[1] = e.radiance[2] = 1.0f; e.envmap_scale = 1.0f;
            sc.emitters.push_back(e);
        } else if (rec == "mesh") {
            mtsamd_mesh_desc m{}; int has_normals;
            ls >> m.bsdf >> m.emitter >> m.vertex_count >> m.face_count >> has_normals;
            sc.pos.push_back(float_line(in, "P"));
            std::getline(in, line);
            std::istringstream fs(line); std::string t; fs >> t;
            std::vector<uint32_t> f; uint32_t v;
            while (fs >> v) f.push_back(v);
            sc.faces.push_back(f);
            sc.nrm.push_back(has_normals ? float_line(in, "N") : std::vector<float>());
            sc.meshes.push_back(m);
        } else if (rec == "build") {
            const mtsamd_scene_desc d = sc.desc();
            const int rc = build_host_scene(&d, nullptr, 0, nullptr, 0, BuildOptions{}, live);
            std::printf("build.rc %d\nbuild.message %s\n", rc, rc ? last_error() : "");
            if (rc) return 0;
        } else if (rec == "move") {
            uint32_t shape; int has_normals; std::string label;
            ls >> shape >> has_normals >> label;
            const std::vector<float> p = float_line(in, "P"), n = has_normals ? float_line(in, "N") : std::vector<float>();
            const int rc = set_vertex_positions(live.state, BuildOptions{}, shape, p.data(), has_normals ? n.data() : nullptr, live.tri_pos, live.tri_nrm,
                                                live.area_pmf, live.area_cdf, live);
            std::printf("%s.rc %d\n%s.message %s\n", label.c_str(), rc, label.c_str(), rc ? last_error() : "");
            if (!rc) { sc.pos[shape] = p; if (has_normals) sc.nrm[shape] = n; }
        } else if (rec == "dump" || rec == "fresh" || rec == "rebuild" || rec == "encode") {
            std::string label; ls >> label;
            if (rec == "dump") dump_scene(label.c_str(), live);
            else if (rec == "encode") check_encoding(label.c_str(), live);
            else if (rec == "rebuild") { refit_bvh(live.tri_pos.data(), live.state.bvh); dump_scene(label.c_str(), live); }
            else {
                const mtsamd_scene_desc d = sc.desc();
                HostScene fresh;
                const int rc = build_host_scene(&d, nullptr, 0, nullptr, 0, BuildOptions{}, fresh);
                std::printf("%s.rc %d\n", label.c_str(), rc);
                if (!rc) dump_scene(label.c_str(), fresh);
            }
        }
    }
    return 0;
}

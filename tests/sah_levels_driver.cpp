// Stand-alone driver of the host specification of the SAH accelerator rebuild (mitsuba2_amd/csrc/bvh.h: build_sah_levels) for
// tests/test_sah_levels_cpu.py and the array comparisons of tests/test_gpu_rebuild_sah.py.  It reads a scene in the format of tests/refit_driver.cpp
// (tests/vertex_moves.py writes it) and a list of commands, and dumps arrays as hex words.  It decides nothing: every expectation lives
// in the tests.
//   bsdfs / emitter / mesh / build / move       as tests/refit_driver.cpp
//   sahl LABEL                                  build_sah_levels of the live scene's triangles as they are now (with the trace); the tree is kept
//   lbvh LABEL                                  build_lbvh of the same; the tree is kept
//   bvh LABEL                                   build_bvh of the same (creation's builder); the tree is kept
//   refit LABEL                                 refit_bvh of the kept tree with the live scene's triangles as they are now
//   sah LABEL                                   SAH cost of the live scene's own (binned-SAH, refitted) tree
//   raw LABEL                                   then a line `P words` (9 floats per triangle): build_sah_levels of these triangles as LABEL
//                                               (with the trace: what every node decided, and the bins of the first 16 nodes), refit_bvh
//                                               of that tree with the same triangles as LABELr, and build_bvh of them as LABELb
//   fit LABEL D..                               bvh_stack_fits of each stack depth D
#include "scene_build.h"
#include "lbvh_keys.h"
#include "sah_keys.h"

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

static std::vector<int32_t> kids_of(const RefitTable &rt) {
    std::vector<int32_t> kids(2 * rt.left.size());
    for (size_t t = 0; t < rt.left.size(); ++t) {
        kids[2 * t] = rt.left[t] >= 0 ? rt.left[t] : -1;
        kids[2 * t + 1] = rt.left[t] >= 0 ? rt.right[t] : (int32_t) rt.ref2[t];
    }
    return kids;
}

static void dump_sah(const char *label, const RefitTable &rt) {
    const std::vector<int32_t> kids = kids_of(rt);
    const double cost = rt.left.empty() ? 0.0 : sah_cost_blocked(kids.data(), rt.boxes.data(), rt.left.size(), rt.root);
    dump(label, "sah", &cost, 1);
}

static void dump_tree(const char *label, const BvhOutput &b, const std::vector<float> &tri_pos) {
    const uint32_t counts[] = { b.root, b.wroot, b.wdepth, b.n_nodes, b.n_wnodes, b.n_slots, b.depth, bvh_stack_depth(b.depth, b.wdepth, true) };
    dump(label, "counts", counts, 8);
    dump(label, "nodes", b.nodes); dump(label, "qnodes", b.qnodes); dump(label, "wnodes", b.wnodes); dump(label, "wnodes_h", b.wnodes_h);
    dump(label, "wnodes_p", b.wnodes_p); dump(label, "tris", b.tris); dump(label, "bbox", b.bbox, 6);
    const float grid[6] = { b.q_lo[0], b.q_lo[1], b.q_lo[2], b.q_step[0], b.q_step[1], b.q_step[2] };
    dump(label, "grid", grid, 6);
    dump(label, "tri_pos", tri_pos);
    const RefitTable &rt = b.refit;
    dump(label, "kids", kids_of(rt)); dump(label, "order", rt.order); dump(label, "class_start", rt.class_start); dump(label, "height", rt.height);
    dump(label, "ref2", rt.ref2); dump(label, "ref4", rt.ref4); dump(label, "node_child", rt.node_child); dump(label, "wide_child", rt.wide_child);
    dump(label, "slot_prim", rt.slot_prim); dump(label, "boxes", rt.boxes);
    const int32_t root = rt.root; dump(label, "rt_root", &root, 1);
    dump_sah(label, rt);
}

static void dump_trace(const char *label, const SahLevelsTrace &tr) {
    dump(label, "t_first", tr.first); dump(label, "t_count", tr.count); dump(label, "t_depth", tr.depth); dump(label, "t_mode", tr.mode);
    dump(label, "t_left", tr.left_count); dump(label, "t_axis", tr.axis); dump(label, "t_bin", tr.bin); dump(label, "t_cost", tr.cost);
    dump(label, "t_bins_node", tr.bins_node); dump(label, "t_bins", tr.bins);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    Description sc;
    HostScene live;
    BvhOutput tree;
    const BuildOptions options{};
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
            const int rc = build_host_scene(&d, nullptr, 0, nullptr, 0, options, live);
            std::printf("build.rc %d\nbuild.message %s\n", rc, rc ? last_error() : "");
            if (rc) return 0;
        } else if (rec == "move") {
            uint32_t shape; int has_normals; std::string label;
            ls >> shape >> has_normals >> label;
            const std::vector<float> p = float_line(in, "P"), n = has_normals ? float_line(in, "N") : std::vector<float>();
            const int rc = set_vertex_positions(live.state, options, shape, p.data(), has_normals ? n.data() : nullptr, live.tri_pos, live.tri_nrm,
                                                live.area_pmf, live.area_cdf, live);
            std::printf("%s.rc %d\n%s.message %s\n", label.c_str(), rc, label.c_str(), rc ? last_error() : "");
        } else if (rec == "lbvh" || rec == "refit" || rec == "sah" || rec == "sahl" || rec == "bvh") {
            std::string label; ls >> label;
            if (rec == "sah") { dump_sah(label.c_str(), live.state.bvh.refit); continue; }
            if (rec == "lbvh") build_lbvh(live.tri_pos.data(), live.state.n_prims, options.max_leaf, tree);
            else if (rec == "sahl") {
                SahLevelsTrace tr;
                build_sah_levels(live.tri_pos.data(), live.state.n_prims, options.max_leaf, tree, &tr);
                dump_trace(label.c_str(), tr);
            }
            else if (rec == "bvh") build_bvh(live.tri_pos.data(), live.state.n_prims, options.max_leaf, tree);
            else refit_bvh(live.tri_pos.data(), tree);
            dump_tree(label.c_str(), tree, live.tri_pos);
        } else if (rec == "raw") {
            std::string label; ls >> label;
            const std::vector<float> p = float_line(in, "P");
            BvhOutput t, b;
            SahLevelsTrace tr;
            tr.bins_of = 16;
            build_sah_levels(p.data(), (uint32_t) (p.size() / 9), options.max_leaf, t, &tr);
            dump_tree(label.c_str(), t, p);
            dump_trace(label.c_str(), tr);
            refit_bvh(p.data(), t);
            dump_tree((label + "r").c_str(), t, p);
            build_bvh(p.data(), (uint32_t) (p.size() / 9), options.max_leaf, b);
            dump_tree((label + "b").c_str(), b, p);
        } else if (rec == "fit") {
            std::string label; ls >> label;
            std::vector<uint32_t> out; uint32_t d;
            while (ls >> d) out.push_back(bvh_stack_fits(d) ? 1u : 0u);
            dump(label.c_str(), "fit", out);
        }
    }
    return 0;
}

// Stand-alone driver of build_tangent_records (mitsuba2_amd/csrc/scene_build.h), the host half of the forward-mode render, for
// tests/test_forward_cpu.py.  It reads lines of
//   record type texture r g b sr sg sb er eg eb kr kg kb alpha_u alpha_v     -- appends a BSDF record to the table
//   tangent b k0 .. k17                                                      -- sets the 18 tangent floats of record b ("nan", "inf" allowed)
//   run label h                                                              -- calls build_tangent_records and dumps what it returns
//   null label h                                                             -- the same with a null tangent array
//   clear                                                                    -- empties the table and the tangents
// and prints per run `label rc <code>`, `label msg <text>` and, as hex words, `label plus|minus b <14 words>` per record (the fields
// above from r on) and `label inv_2h <words>`.  It decides nothing: every expectation lives in the test.
//   argv[1]: the case file
#include "scene_build.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

using namespace mtsamd;

static void dump_record(const char *label, const char *name, size_t b, const DevBsdf &d) {
    const float f[14] = { d.r, d.g, d.b, d.sr, d.sg, d.sb, d.er, d.eg, d.eb, d.kr, d.kg, d.kb, d.alpha_u, d.alpha_v };
    std::printf("%s %s %zu", label, name, b);
    for (float x : f) { uint32_t w; std::memcpy(&w, &x, 4); std::printf(" %08x", w); }
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    SceneState st;
    std::vector<float> tangents;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string op; ls >> op;
        if (op == "clear") { st.bsdfs.clear(); tangents.clear(); }
        else if (op == "record") {
            DevBsdf d{};
            std::string tok[16];
            for (auto &t : tok) ls >> t;
            d.type = std::atoi(tok[0].c_str()); d.texture = std::atoi(tok[1].c_str());
            float *dst[14] = { &d.r, &d.g, &d.b, &d.sr, &d.sg, &d.sb, &d.er, &d.eg, &d.eb, &d.kr, &d.kg, &d.kb, &d.alpha_u, &d.alpha_v };
            for (int i = 0; i < 14; ++i) *dst[i] = std::strtof(tok[2 + i].c_str(), nullptr);
            st.bsdfs.push_back(d);
            tangents.resize(MTSAMD_BSDF_TANGENT_FLOATS * st.bsdfs.size(), 0.0f);
        } else if (op == "tangent") {
            size_t b; ls >> b;
            for (int i = 0; i < MTSAMD_BSDF_TANGENT_FLOATS; ++i) { std::string t; ls >> t; tangents.at(MTSAMD_BSDF_TANGENT_FLOATS * b + i) = std::strtof(t.c_str(), nullptr); }
        } else if (op == "run" || op == "null") {
            std::string label, hs; ls >> label >> hs;
            std::vector<DevBsdf> plus, minus; std::vector<float> inv_2h;
            (void) fail(0, "%s", "");
            const int rc = build_tangent_records(st, op == "null" ? nullptr : tangents.data(), std::strtof(hs.c_str(), nullptr), plus, minus, inv_2h);
            std::printf("%s rc %d\n%s msg %s\n", label.c_str(), rc, label.c_str(), last_error());
            if (rc) continue;
            for (size_t b = 0; b < plus.size(); ++b) { dump_record(label.c_str(), "plus", b, plus[b]); dump_record(label.c_str(), "minus", b, minus[b]); }
            std::printf("%s inv_2h", label.c_str());
            for (float x : inv_2h) { uint32_t w; std::memcpy(&w, &x, 4); std::printf(" %08x", w); }
            std::printf("\n");
        }
    }
    return 0;
}

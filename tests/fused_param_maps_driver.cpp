// Stand-alone driver of build_tangent_records and build_reverse_slots (mitsuba2_amd/csrc/scene_build.h) on records that read parameters
// from textures (kBsdfTexParams; DevBsdf::nested0 / nested1 hold "1 + texture index" per slot), for tests/test_fused_param_maps_cpu.py.
// It reads lines of
//   record type texture flags nested0 nested1 r g b sr sg sb er eg eb kr kg kb alpha_u alpha_v   -- appends a BSDF record to the table
//   tangent b k0 .. k17                                                      -- sets the 18 tangent floats of record b
//   wanted b w0 .. w17                                                       -- sets the 18 wanted flags of record b
//   forward label h                                                          -- calls build_tangent_records and dumps what it returns
//   reverse label h                                                          -- calls build_reverse_slots and dumps what it returns
//   clear                                                                    -- empties the table, the tangents and the flags
// and prints per run `label rc <code>`, `label msg <text>` and, as hex words, `label plus|minus b <14 words>` per record and
// `label inv_2h <words>` (forward), or `label range <numbers>` and `label slot j record out f0 f1 <plus minus inv_2h>` (reverse).
// It decides nothing: every expectation lives in the test.
//   argv[1]: the case file
#include "scene_build.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

using namespace mtsamd;

static uint32_t word(float x) { uint32_t w; std::memcpy(&w, &x, 4); return w; }

static void dump_record(const char *label, const char *name, size_t b, const DevBsdf &d) {
    const float f[14] = { d.r, d.g, d.b, d.sr, d.sg, d.sb, d.er, d.eg, d.eb, d.kr, d.kg, d.kb, d.alpha_u, d.alpha_v };
    std::printf("%s %s %zu", label, name, b);
    for (float x : f) std::printf(" %08x", word(x));
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    SceneState st;
    std::vector<float> tangents;
    std::vector<uint8_t> wanted;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string op; ls >> op;
        if (op == "clear") { st.bsdfs.clear(); tangents.clear(); wanted.clear(); }
        else if (op == "record") {
            DevBsdf d{};
            std::string tok[19];
            for (auto &t : tok) ls >> t;
            d.type = std::atoi(tok[0].c_str()); d.texture = std::atoi(tok[1].c_str());
            d.flags = (uint32_t) std::strtoul(tok[2].c_str(), nullptr, 0);
            d.nested0 = (uint32_t) std::strtoul(tok[3].c_str(), nullptr, 0); d.nested1 = (uint32_t) std::strtoul(tok[4].c_str(), nullptr, 0);
            float *dst[14] = { &d.r, &d.g, &d.b, &d.sr, &d.sg, &d.sb, &d.er, &d.eg, &d.eb, &d.kr, &d.kg, &d.kb, &d.alpha_u, &d.alpha_v };
            for (int i = 0; i < 14; ++i) *dst[i] = std::strtof(tok[5 + i].c_str(), nullptr);
            st.bsdfs.push_back(d);
            st.textured_params = st.textured_params || (d.flags & kBsdfTexParams) != 0u;
            tangents.resize(MTSAMD_BSDF_TANGENT_FLOATS * st.bsdfs.size(), 0.0f);
            wanted.resize(MTSAMD_BSDF_TANGENT_FLOATS * st.bsdfs.size(), 0);
        } else if (op == "tangent") {
            size_t b; ls >> b;
            for (int i = 0; i < MTSAMD_BSDF_TANGENT_FLOATS; ++i) { std::string t; ls >> t; tangents.at(MTSAMD_BSDF_TANGENT_FLOATS * b + i) = std::strtof(t.c_str(), nullptr); }
        } else if (op == "wanted") {
            size_t b; ls >> b;
            for (int i = 0; i < MTSAMD_BSDF_TANGENT_FLOATS; ++i) { int w; ls >> w; wanted.at(MTSAMD_BSDF_TANGENT_FLOATS * b + i) = (uint8_t) w; }
        } else if (op == "forward") {
            std::string label, hs; ls >> label >> hs;
            std::vector<DevBsdf> plus, minus; std::vector<float> inv_2h;
            (void) fail(0, "%s", "");
            const int rc = build_tangent_records(st, tangents.data(), std::strtof(hs.c_str(), nullptr), plus, minus, inv_2h);
            std::printf("%s rc %d\n%s msg %s\n", label.c_str(), rc, label.c_str(), last_error());
            if (rc) continue;
            for (size_t b = 0; b < plus.size(); ++b) { dump_record(label.c_str(), "plus", b, plus[b]); dump_record(label.c_str(), "minus", b, minus[b]); }
            std::printf("%s inv_2h", label.c_str());
            for (float x : inv_2h) std::printf(" %08x", word(x));
            std::printf("\n");
        } else if (op == "reverse") {
            std::string label, hs; ls >> label >> hs;
            std::vector<ReverseSlot> slots; std::vector<uint32_t> range;
            (void) fail(0, "%s", "");
            const int rc = build_reverse_slots(st, wanted.data(), std::strtof(hs.c_str(), nullptr), slots, range);
            std::printf("%s rc %d\n%s msg %s\n", label.c_str(), rc, label.c_str(), last_error());
            if (rc) continue;
            std::printf("%s range", label.c_str());
            for (uint32_t x : range) std::printf(" %u", x);
            std::printf("\n");
            for (size_t j = 0; j < slots.size(); ++j) {
                const ReverseSlot &s = slots[j];
                std::printf("%s slot %zu %u %u %u %u %08x %08x %08x\n", label.c_str(), j, s.record, s.out, (unsigned) s.f0, (unsigned) s.f1, word(s.plus),
                            word(s.minus), word(s.inv_2h));
            }
        }
    }
    return 0;
}

// Stand-alone driver of the host half of the forward and reverse renders in scenes with blendbsdf / mask records
// (mitsuba2_amd/csrc/scene_build.h: check_derivative_flags, split_nested_rows, add_weight_slots, and build_tangent_records /
// build_reverse_slots on what is left), for tests/test_nested_diff_cpu.py.  It reads lines of
//   record type texture flags nested0 nested1 r g b sr sg sb er eg eb kr kg kb alpha_u alpha_v   -- appends a BSDF record to the table
//   tangent b k0 .. k17                                                      -- sets the 18 tangent floats of record b
//   wanted b w0 .. w17                                                       -- sets the 18 wanted flags of record b
//   spectral 0|1                                                             -- the scene's variant
//   flags label bits reverse                                                 -- calls check_derivative_flags
//   forward label h                                                          -- split_nested_rows, then build_tangent_records on the rest
//   plain label h                                                            -- build_tangent_records on the tangent as it stands
//   reverse label h                                                          -- split_nested_rows, build_reverse_slots on the rest, add_weight_slots
//   clear                                                                    -- empties the table, the tangents and the flags
// and prints per run `label rc <code>`, `label msg <text>` and, as hex words, `label rest b <18 words>`, `label weight <words>`,
// `label plus|minus b <14 words>`, `label inv_2h <words>` (forward / plain), or `label weight <flags>`, `label range <numbers>` and
// `label slot j record out f0 f1 <plus minus inv_2h>` (reverse); `label nested 0|1` (flags).  It decides nothing: every expectation
// lives in the test.
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

static void dump_tables(const char *label, const std::vector<DevBsdf> &plus, const std::vector<DevBsdf> &minus, const std::vector<float> &inv_2h) {
    for (size_t b = 0; b < plus.size(); ++b) { dump_record(label, "plus", b, plus[b]); dump_record(label, "minus", b, minus[b]); }
    std::printf("%s inv_2h", label);
    for (float x : inv_2h) std::printf(" %08x", word(x));
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
        if (op == "clear") { st.bsdfs.clear(); tangents.clear(); wanted.clear(); st.textured_params = false; st.spectral = false; }
        else if (op == "spectral") { int v; ls >> v; st.spectral = v != 0; }
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
            st.textured_params = st.textured_params || (d.type < kBsdfBlend && (d.flags & kBsdfTexParams) != 0u);
            st.nested_bsdfs = st.nested_bsdfs || d.type >= kBsdfBlend || st.textured_params;
            tangents.resize(MTSAMD_BSDF_TANGENT_FLOATS * st.bsdfs.size(), 0.0f);
            wanted.resize(MTSAMD_BSDF_TANGENT_FLOATS * st.bsdfs.size(), 0);
        } else if (op == "tangent") {
            size_t b; ls >> b;
            for (int i = 0; i < MTSAMD_BSDF_TANGENT_FLOATS; ++i) { std::string t; ls >> t; tangents.at(MTSAMD_BSDF_TANGENT_FLOATS * b + i) = std::strtof(t.c_str(), nullptr); }
        } else if (op == "wanted") {
            size_t b; ls >> b;
            for (int i = 0; i < MTSAMD_BSDF_TANGENT_FLOATS; ++i) { int w; ls >> w; wanted.at(MTSAMD_BSDF_TANGENT_FLOATS * b + i) = (uint8_t) w; }
        } else if (op == "flags") {
            std::string label; unsigned bits; int reverse; ls >> label >> bits >> reverse;
            bool nested = false;
            (void) fail(0, "%s", "");
            const int rc = check_derivative_flags(st, bits, reverse != 0, nested);
            std::printf("%s rc %d\n%s msg %s\n%s nested %d\n", label.c_str(), rc, label.c_str(), last_error(), label.c_str(), nested ? 1 : 0);
        } else if (op == "forward" || op == "plain") {
            std::string label, hs; ls >> label >> hs;
            std::vector<DevBsdf> plus, minus; std::vector<float> inv_2h, rest, weight; std::vector<uint8_t> none_r, none_w;
            (void) fail(0, "%s", "");
            int rc = 0;
            if (op == "forward") rc = split_nested_rows(st, tangents.data(), nullptr, rest, weight, none_r, none_w);
            else rest = tangents;
            if (!rc) rc = build_tangent_records(st, rest.data(), std::strtof(hs.c_str(), nullptr), plus, minus, inv_2h);
            std::printf("%s rc %d\n%s msg %s\n", label.c_str(), rc, label.c_str(), last_error());
            if (rc) continue;
            for (size_t b = 0; b < st.bsdfs.size(); ++b) {
                std::printf("%s rest %zu", label.c_str(), b);
                for (int i = 0; i < MTSAMD_BSDF_TANGENT_FLOATS; ++i) std::printf(" %08x", word(rest[MTSAMD_BSDF_TANGENT_FLOATS * b + i]));
                std::printf("\n");
            }
            std::printf("%s weight", label.c_str());
            for (float x : weight) std::printf(" %08x", word(x));
            std::printf("\n");
            dump_tables(label.c_str(), plus, minus, inv_2h);
        } else if (op == "reverse") {
            std::string label, hs; ls >> label >> hs;
            std::vector<ReverseSlot> slots; std::vector<uint32_t> range; std::vector<float> none_r, none_w; std::vector<uint8_t> rest, weight;
            (void) fail(0, "%s", "");
            int rc = split_nested_rows(st, nullptr, wanted.data(), none_r, none_w, rest, weight);
            if (!rc) rc = build_reverse_slots(st, rest.data(), std::strtof(hs.c_str(), nullptr), slots, range);
            std::printf("%s rc %d\n%s msg %s\n", label.c_str(), rc, label.c_str(), last_error());
            if (rc) continue;
            add_weight_slots(weight, slots, range);
            std::printf("%s weight", label.c_str());
            for (uint8_t x : weight) std::printf(" %u", (unsigned) x);
            std::printf("\n%s range", label.c_str());
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

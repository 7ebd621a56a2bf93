// Stand-alone driver of build_reverse_slots (mitsuba2_amd/csrc/scene_build.h), the host half of the reverse-mode render, for
// tests/test_reverse_cpu.py.  It reads lines of
//   record type texture r g b sr sg sb er eg eb kr kg kb alpha_u alpha_v     -- appends a BSDF record to the table
//   wanted b w0 .. w17                                                       -- sets the 18 wanted bytes of record b
//   run label h                                                              -- calls build_reverse_slots and dumps what it returns
//   null label h                                                             -- the same with a null wanted array
//   clear                                                                    -- empties the table and the wanted bytes
// and prints per run `label rc <code>`, `label msg <text>`, `label range <n + 1 numbers>` and per slot j
//   label slot j <record> <out> <f0> <f1>
//   label plus|minus j <14 hex words>      -- the slot's patch applied to its record (the fields above from r on)
//   label inv j <hex word>
//   label ref_rc j <code>                  -- build_tangent_records for the tangent that is 1 on the slot's scalar and 0 elsewhere, same h
//   label ref_plus|ref_minus j <14 hex words>, label ref_inv j <hex word>      -- what it gives for the slot's record
//   label ref_others j <0 | 1>             -- 1: every other record of that result is untouched and has inv_2h 0
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

static void dump_record(const char *label, const char *name, size_t j, const DevBsdf &d) {
    const float f[14] = { d.r, d.g, d.b, d.sr, d.sg, d.sb, d.er, d.eg, d.eb, d.kr, d.kg, d.kb, d.alpha_u, d.alpha_v };
    std::printf("%s %s %zu", label, name, j);
    for (float x : f) { uint32_t w; std::memcpy(&w, &x, 4); std::printf(" %08x", w); }
    std::printf("\n");
}
static void dump_float(const char *label, const char *name, size_t j, float x) {
    uint32_t w; std::memcpy(&w, &x, 4);
    std::printf("%s %s %zu %08x\n", label, name, j, w);
}
static void patch(DevBsdf &d, uint16_t f, float v) { std::memcpy(reinterpret_cast<char *>(&d) + 4u * f, &v, 4); }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    SceneState st;
    std::vector<uint8_t> wanted;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string op; ls >> op;
        if (op == "clear") { st.bsdfs.clear(); wanted.clear(); }
        else if (op == "record") {
            DevBsdf d{};
            std::string tok[16];
            for (auto &t : tok) ls >> t;
            d.type = std::atoi(tok[0].c_str()); d.texture = std::atoi(tok[1].c_str());
            float *dst[14] = { &d.r, &d.g, &d.b, &d.sr, &d.sg, &d.sb, &d.er, &d.eg, &d.eb, &d.kr, &d.kg, &d.kb, &d.alpha_u, &d.alpha_v };
            for (int i = 0; i < 14; ++i) *dst[i] = std::strtof(tok[2 + i].c_str(), nullptr);
            st.bsdfs.push_back(d);
            wanted.resize(MTSAMD_BSDF_TANGENT_FLOATS * st.bsdfs.size(), 0);
        } else if (op == "wanted") {
            size_t b; ls >> b;
            for (int i = 0; i < MTSAMD_BSDF_TANGENT_FLOATS; ++i) { int w; ls >> w; wanted.at(MTSAMD_BSDF_TANGENT_FLOATS * b + i) = (uint8_t) w; }
        } else if (op == "run" || op == "null") {
            std::string label_, hs; ls >> label_ >> hs;
            const char *label = label_.c_str();
            const float h = std::strtof(hs.c_str(), nullptr);
            std::vector<ReverseSlot> slots; std::vector<uint32_t> range;
            (void) fail(0, "%s", "");
            const int rc = build_reverse_slots(st, op == "null" ? nullptr : wanted.data(), h, slots, range);
            std::printf("%s rc %d\n%s msg %s\n", label, rc, label, last_error());
            if (rc) continue;
            std::printf("%s range", label);
            for (uint32_t x : range) std::printf(" %u", x);
            std::printf("\n");
            for (size_t j = 0; j < slots.size(); ++j) {
                const ReverseSlot &s = slots[j];
                std::printf("%s slot %zu %u %u %u %u\n", label, j, s.record, s.out, (unsigned) s.f0, (unsigned) s.f1);
                DevBsdf p = st.bsdfs.at(s.record), m = p;
                patch(p, s.f0, s.plus); patch(p, s.f1, s.plus); patch(m, s.f0, s.minus); patch(m, s.f1, s.minus);
                dump_record(label, "plus", j, p); dump_record(label, "minus", j, m); dump_float(label, "inv", j, s.inv_2h);
                std::vector<float> hot(MTSAMD_BSDF_TANGENT_FLOATS * st.bsdfs.size(), 0.0f);
                hot.at(s.out) = 1.0f;
                std::vector<DevBsdf> plus, minus; std::vector<float> inv_2h;
                const int ref = build_tangent_records(st, hot.data(), h, plus, minus, inv_2h);
                std::printf("%s ref_rc %zu %d\n", label, j, ref);
                if (ref) continue;
                dump_record(label, "ref_plus", j, plus[s.record]); dump_record(label, "ref_minus", j, minus[s.record]);
                dump_float(label, "ref_inv", j, inv_2h[s.record]);
                bool others = true;
                for (size_t b = 0; b < st.bsdfs.size(); ++b)
                    if (b != s.record) others = others && !std::memcmp(&plus[b], &st.bsdfs[b], sizeof(DevBsdf)) && !std::memcmp(&minus[b], &st.bsdfs[b], sizeof(DevBsdf)) && inv_2h[b] == 0.0f;
                std::printf("%s ref_others %zu %d\n", label, j, others ? 1 : 0);
            }
        }
    }
    return 0;
}

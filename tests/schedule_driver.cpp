// schedule_driver.cpp -- stand-alone host program around mitsuba2_amd/csrc/schedule.{h,cpp} for tests/test_schedule_cpu.py: reads cases
// (one per line: a kind, a name, key=value fields), prints what the plan gives as `name key=value ...` lines.  It holds no expectation
// of its own except the brute-force walks the Python file cannot afford: every sample of a pass exactly once, the row window, and the
// tile grid of a splat over the source pixels of its rows.
#include "schedule.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

using namespace mtsamd;

// fail() / last_error() of scene_build.h, defined here so that the program is schedule.cpp and this file alone: the text is kept for the
// `message` line
static char g_error[512];
int mtsamd::fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}
const char *mtsamd::last_error() { return g_error; }

typedef std::map<std::string, long long> Args;

static long long get(const Args &a, const char *key, long long def = 0) {
    auto it = a.find(key);
    return it == a.end() ? def : it->second;
}

static int make_job(const Args &a, JobShape &js) {
    const SceneFacts facts{ get(a, "flat") != 0, get(a, "nested") != 0, get(a, "spectral") != 0, (uint32_t) get(a, "cu", 1) };
    mtsamd_render_desc d{};
    d.integrator = (int32_t) get(a, "integrator"); d.pipeline = (int32_t) get(a, "pipeline");
    d.paths_per_wave = (int32_t) get(a, "paths_per_wave"); d.max_pass_log2 = (int32_t) get(a, "max_pass_log2");
    d.samples_per_pass = (int32_t) get(a, "samples_per_pass");
    d.crop_width = (int32_t) get(a, "crop_w", 256); d.crop_height = (int32_t) get(a, "crop_h", 256); d.sample_count = (int32_t) get(a, "spp", 64);
    ScheduleSwitches sw;
    sw.chains = (uint32_t) get(a, "chains"); sw.mega = get(a, "mega") != 0;
    return plan_job(facts, d, (uint64_t) get(a, "max_pass", 1ll << 30), sw, js);
}

static void print_job(const JobShape &js) {
    std::printf(" split=%d shadow_queue=%d shadow_ring=%d target=%u n_waves=%u seg_cap=%u pass_limit=%llu", js.split, js.shadow_queue, js.shadow_ring,
                js.target, js.n_waves, js.seg_cap, (unsigned long long) js.pass_limit);
}

template <typename T> static void print_list(const char *key, const T *v, size_t n) {
    std::printf(" %s=", key);
    for (size_t i = 0; i < n; ++i) std::printf("%s%llu", i ? "," : "", (unsigned long long) v[i]);
}

// cursor_sample of kernels.hip, in its 32-bit arithmetic: the v-th sample of scheduling wave `wave` -> its ordinal within the pass
static uint32_t cursor_sample(const PassPlan &p, uint32_t nw, uint32_t wave, uint64_t v) {
    const uint32_t t = (uint32_t) v / p.chunk, within = (uint32_t) v - t * p.chunk;
    return (t * nw + chunk_owner(wave, nw, p.n_chains)) * p.chunk + within;
}

// "" if the waves' cursors walk the pass ordinals 0 .. n - 1 exactly once
static std::string walk(const PassPlan &p, uint32_t nw, const std::vector<uint64_t> &cursor_end, uint64_t n) {
    std::vector<uint8_t> seen(n, 0);
    uint64_t total = 0;
    char msg[128];
    for (uint32_t k = 0; k < nw; ++k)
        for (uint64_t v = 0; v < cursor_end[k]; ++v, ++total) {
            const uint32_t o = cursor_sample(p, nw, k, v);
            if (o >= n || seen[o]++) { std::snprintf(msg, sizeof(msg), "wave_%u_sample_%llu_hits_%u_%s", k, (unsigned long long) v, o, o >= n ? "outside" : "twice"); return msg; }
        }
    if (total != n) { std::snprintf(msg, sizeof(msg), "%llu_of_%llu_samples", (unsigned long long) total, (unsigned long long) n); return msg; }
    return "";
}

// k_film_accum's thread-to-pixel map (kernels.hip): "" if the kFilmTile x kFilmTile threads of the tiles_x * tiles_y workgroups take every
// source pixel of the splat's rows exactly once and the rows of every tile are contiguous on the film
static std::string tile_walk(const FilmParams &f) {
    std::vector<uint8_t> seen((size_t) f.pass_rows * f.crop_w, 0);
    char msg[128];
    for (int tcy = 0; tcy < f.tiles_y; ++tcy)
        for (int tcx = 0; tcx < f.tiles_x; ++tcx)
            for (int ly = 0; ly < kFilmTile; ++ly)
                for (int lx = 0; lx < kFilmTile; ++lx) {
                    const int qx = tcx * kFilmTile + lx, lr = f.pass_lr0 + tcy * f.tile_h + ly;
                    if (!(qx < f.crop_w && ly < f.tile_h && lr < f.pass_lr0 + f.pass_rows)) continue;
                    if (seen[(size_t) (lr - f.pass_lr0) * f.crop_w + qx]++) { std::snprintf(msg, sizeof(msg), "row_%d_column_%d_twice", lr, qx); return msg; }
                    if (ly > 0 && row_to_global(f.rows, lr) != row_to_global(f.rows, lr - 1) + 1) { std::snprintf(msg, sizeof(msg), "tile_row_%d_splits_at_row_%d", tcy, lr); return msg; }
                }
    for (size_t i = 0; i < seen.size(); ++i)
        if (!seen[i]) { std::snprintf(msg, sizeof(msg), "row_%d_column_%d_missed", f.pass_lr0 + (int) (i / f.crop_w), (int) (i % f.crop_w)); return msg; }
    return "";
}

static void print_error(int rc) { std::printf(" rc=%d\nmessage %s\n", rc, last_error()); }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string kind, name, tok;
        ls >> kind >> name;
        Args a;
        std::vector<long long> script;       // drain: alive, dry pairs after `--`
        bool in_script = false;
        while (ls >> tok) {
            if (tok == "--") { in_script = true; continue; }
            if (in_script) { script.push_back(std::stoll(tok)); continue; }
            const size_t eq = tok.find('=');
            a[tok.substr(0, eq)] = std::stoll(tok.substr(eq + 1));
        }
        std::printf("%s", name.c_str());
        if (kind == "film") {
            const RowMap rows{ (int32_t) get(a, "row0"), (int32_t) get(a, "local_rows"), (int32_t) get(a, "tile_rows"), (int32_t) get(a, "part"), (int32_t) get(a, "count", 1) };
            const int32_t R = (int32_t) get(a, "R"), crop_h = (int32_t) get(a, "crop_h");
            FilmPasses fp;
            if (int rc = plan_film_passes(rows, (uint64_t) get(a, "pass_cap"), (uint64_t) get(a, "per_row"), fp)) { print_error(rc); continue; }
            std::printf(" rc=0 rows_per_pass=%llu n_passes=%llu tile_h=%d tile_h_one=%d", (unsigned long long) fp.rows_per_pass, (unsigned long long) fp.n_passes, fp.tile_h, fp.tile_h_one);
            std::vector<long long> lr, window, brute;
            for (uint64_t lr0 = 0; lr0 < (uint64_t) rows.local_rows; lr0 += fp.rows_per_pass) {
                const uint64_t nrows = std::min<uint64_t>(fp.rows_per_pass, (uint64_t) rows.local_rows - lr0);
                int32_t r0, r1, lo = INT32_MAX, hi = INT32_MIN;
                film_row_window(rows, lr0, nrows, R, crop_h, r0, r1);
                for (uint64_t l = lr0; l < lr0 + nrows; ++l) { const int32_t g = row_to_global(rows, (int32_t) l); lo = std::min(lo, g); hi = std::max(hi, g); }
                lr.push_back((long long) lr0); lr.push_back((long long) nrows);
                window.push_back(r0); window.push_back(r1);
                brute.push_back(std::max(0, lo - R)); brute.push_back(std::min(crop_h, hi + R + 1));
            }
            print_list("passes", lr.data(), lr.size()); print_list("window", window.data(), window.size()); print_list("brute", brute.data(), brute.size());
            std::printf("\n");
            continue;
        }
        if (kind == "splat") {
            // the splats of a film render (api.cpp, FilmStage): one `pass` line per pass splatted on its own, one `once` line per row count
            // [0, rows_done) the kept-stream aov path can splat, and the scratch tiles reserved for either
            const RowMap rows{ (int32_t) get(a, "row0"), (int32_t) get(a, "local_rows"), (int32_t) get(a, "tile_rows"), (int32_t) get(a, "part"), (int32_t) get(a, "count", 1) };
            mtsamd_render_desc d{};
            d.crop_x = (int32_t) get(a, "crop_x"); d.crop_y = (int32_t) get(a, "crop_y"); d.crop_width = (int32_t) get(a, "crop_w"); d.crop_height = (int32_t) get(a, "crop_h");
            d.sample_count = (int32_t) get(a, "spp");
            const int32_t R = (int32_t) get(a, "R");
            const uint64_t per_row = (uint64_t) d.crop_width * (uint64_t) d.sample_count, all = (uint64_t) rows.local_rows;
            FilmPasses fp;
            if (int rc = plan_film_passes(rows, (uint64_t) get(a, "pass_cap"), per_row, fp)) { print_error(rc); continue; }
            std::printf(" rc=0 rows_per_pass=%llu n_passes=%llu tile_h=%d tile_h_one=%d reserve_pass=%zu reserve_once=%zu floats_per_tile=%d\n", (unsigned long long) fp.rows_per_pass,
                        (unsigned long long) fp.n_passes, fp.tile_h, fp.tile_h_one, film_reserve_floats(fp, rows.local_rows, d.crop_width, d.sample_count, true),
                        film_reserve_floats(fp, rows.local_rows, d.crop_width, d.sample_count, false), kFilmPartial);
            auto splat = [&](const char *what, uint64_t lr0, uint64_t nrows, int32_t tile_h) {
                FilmParams f{};
                film_splat_geometry(rows, d, R, true, lr0, nrows, tile_h, f);
                int32_t r0, r1;
                film_row_window(rows, lr0, nrows, R, d.crop_height, r0, r1);
                const bool same_rows = f.rows.row0 == rows.row0 && f.rows.local_rows == rows.local_rows && f.rows.tile_rows == rows.tile_rows && f.rows.part == rows.part && f.rows.count == rows.count;
                const std::string w = tile_walk(f);
                std::printf("%s %s lr0=%llu nrows=%llu first_ordinal=%llu n_samples=%llu spp=%d same_rows=%d plane_pix0=%u plane_pixels=%u crop_x=%d crop_y=%d crop_w=%d crop_h=%d"
                            " row0=%d row1=%d window0=%d window1=%d pass_lr0=%d pass_rows=%d tile_h=%d tiles_x=%d tiles_y=%d slices=%d need=%zu walk=%s\n", name.c_str(), what,
                            (unsigned long long) lr0, (unsigned long long) nrows, (unsigned long long) f.first_ordinal, (unsigned long long) f.n_samples, f.spp, same_rows, f.plane_pix0,
                            f.plane_pixels, f.crop_x, f.crop_y, f.crop_w, f.crop_h, f.row0, f.row1, r0, r1, f.pass_lr0, f.pass_rows, f.tile_h, f.tiles_x, f.tiles_y, f.slices,
                            film_partial_floats(f), w.empty() ? "ok" : w.c_str());
            };
            for (uint64_t lr0 = 0; lr0 < all; lr0 += fp.rows_per_pass) splat("pass", lr0, std::min<uint64_t>(fp.rows_per_pass, all - lr0), fp.tile_h);
            for (uint64_t done = fp.rows_per_pass; done < all; done += fp.rows_per_pass) splat("once", 0, done, fp.tile_h_one);
            splat("once", 0, all, fp.tile_h_one);
            continue;
        }
        JobShape js;
        if (int rc = make_job(a, js)) { print_error(rc); continue; }
        if (kind == "job") { std::printf(" rc=0"); print_job(js); std::printf("\n"); continue; }
        const uint32_t nw = js.n_waves;
        const uint64_t n = (uint64_t) get(a, "n");
        std::vector<uint64_t> cursor_end(nw, ~0ull);
        PassPlan p;
        if (int rc = plan_pass(js, (uint64_t) get(a, "first"), n, (int32_t) get(a, "finish_kernel"), (int32_t) get(a, "pipeline"), cursor_end.data(), p)) { print_error(rc); continue; }
        if (kind == "pass") {
            std::printf(" rc=0");
            print_job(js);
            std::printf(" chunk=%u n_chains=%u first_pix=%u first_rem=%u mode=%d split_code=%d min_iters=%llu n_parts=%u split_parts=%u gather_max=%u finish_at=%llu", p.chunk,
                        p.n_chains, p.first_pix, p.first_rem, (int) p.mode, p.split, (unsigned long long) p.min_iters, p.n_parts, p.split_parts, p.gather_max, (unsigned long long) p.finish_at);
            print_list("part_lo", p.part_lo, 5); print_list("split_lo", p.split_lo, kMaxChains + 1);
            std::vector<uint32_t> cf(kMaxChains + 1);
            for (uint32_t k = 0; k <= kMaxChains; ++k) cf[k] = chain_first(k, nw, p.split_parts);
            print_list("chain_first", cf.data(), cf.size());
            const std::string w = get(a, "walk", 1) ? walk(p, nw, cursor_end, n) : "skipped";
            std::printf(" walk=%s\n", w.empty() ? "ok" : w.c_str());
            continue;
        }
        // drain: the loop of launch_rounds (api.cpp) with scripted read-backs.  The k-th checkpoint issues script entry k = (alive, dry) and
        // inspects what the checkpoint before issued; one `cp` line per checkpoint.
        std::printf(" rc=0 min_iters=%llu gather_max=%u finish_at=%llu pool_slots=%llu\n", (unsigned long long) p.min_iters, p.gather_max, (unsigned long long) p.finish_at,
                    (unsigned long long) js.seg_cap * nw);
        Drain drain(js, p);
        std::vector<uint32_t> counts[2] = { std::vector<uint32_t>(nw), std::vector<uint32_t>(nw) };
        std::vector<uint64_t> cursors[2] = { cursor_end, cursor_end };
        int pending = -1, slot = 0;
        size_t issued = 0;
        for (uint64_t it = 1; it <= (uint64_t) get(a, "rounds", 64); ++it) {
            if (!drain.due(it)) continue;
            std::printf("%s cp it=%llu", name.c_str(), (unsigned long long) it);
            if (pending >= 0) {
                const Drain::Verdict v = drain.inspect(it, counts[pending].data(), cursors[pending].data(), cursor_end.data());
                std::printf(" inspected=%zu verdict=%d alive=%llu", issued - 1, (int) v, (unsigned long long) drain.alive);
                if (v != Drain::GoOn) { std::printf("\n"); break; }
            } else std::printf(" inspected=-1 verdict=-1 alive=0");
            std::printf(" gather_w=%u stride=%llu next_check=%llu reads_cursors=%d\n", drain.gather_w, (unsigned long long) drain.stride, (unsigned long long) drain.next_check, drain.reads_cursors());
            if (2 * issued + 1 >= script.size()) break;
            uint64_t alive = (uint64_t) script[2 * issued];
            for (uint32_t k = 0; k < nw; ++k) { counts[slot][k] = (uint32_t) ((alive + nw - 1 - k) / nw); }      // spread over the waves, sum = alive
            cursors[slot] = cursor_end;
            if (!script[2 * issued + 1]) for (uint32_t k = nw; k-- > 0;) if (cursor_end[k]) { cursors[slot][k] -= 1; break; }      // one wave is one sample short
            ++issued;
            pending = slot; slot ^= 1;
        }
    }
    return 0;
}

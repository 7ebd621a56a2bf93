// schedule.cpp -- the plan of the wavefront scheduler (schedule.h): host arithmetic only, no HIP runtime call.
#include "schedule.h"

#include <algorithm>
#include <cmath>

namespace mtsamd {

int plan_job(const SceneFacts &scene, const mtsamd_render_desc &d, uint64_t max_pass, const ScheduleSwitches &sw, JobShape &js) {
    js = JobShape{};
    js.scene = scene; js.sw = sw;
    js.integrator = d.integrator; js.spp = d.sample_count;
    // One pass holds up to 2^30 camera samples (24 GiB of sample stream; a second buffer of that size lets the film splat of a pass run
    // beside the tracing of the next): every pass ends with a drain phase in which the pool empties, so fewer, larger passes waste
    // less (cbox 1024^2 @ 256 spp: 4 passes of 2^26 -> 1 pass: +7 %).
    js.pass_limit = 1ull << 30;
    if (d.max_pass_log2 > 0) js.pass_limit = 1ull << std::min(30, std::max(10, d.max_pass_log2));
    // samples_per_pass (integrator.cpp:59-66): a pass holds at most that many samples of every pixel of the crop window -- it bounds the
    // memory of a pass and is where a timeout / cancel can stop; the image does not depend on it (per-sample RNG streams)
    if (d.samples_per_pass > 0)
        js.pass_limit = std::min<uint64_t>(js.pass_limit, std::max<uint64_t>((uint64_t) d.crop_width * d.crop_height * (uint64_t) d.samples_per_pass,
                                                                              (uint64_t) d.crop_width * (uint64_t) d.sample_count));
    // pipeline 0: one kernel with the in-kernel shadow ring (4) for LDS-resident (flat) scenes, split kernels (2) for hierarchy
    // scenes; 1 / 2 / 3 / 4 force one schedule
    if (scene.spectral && d.integrator != 0) return fail(MTSAMD_ERR_UNSUPPORTED, "the direct and depth integrators are implemented for the RGB variant only");
    js.split = d.integrator == 0 && (d.pipeline == 2 || (d.pipeline == 0 && !scene.flat));
    js.shadow_queue = d.integrator == 0 && scene.flat && d.pipeline == 3;
    js.shadow_ring = d.integrator == 0 && scene.flat && (d.pipeline == 4 || d.pipeline == 0);
    // scenes with a blendbsdf / mask run the fused schedule whatever was asked for: only its kernels carry the nesting code (inside the
    // kernels of the other schedules, capped at 128 VGPRs, it cost every general scene up to 20 %)
    if (scene.nested_bsdfs) js.split = js.shadow_queue = js.shadow_ring = false;
    if ((d.pipeline == 3 || d.pipeline == 4) && !scene.flat) return fail(MTSAMD_ERR_INVALID, "pipelines 3 and 4 (queued shadow rays) apply to LDS-resident scenes only");
    // Paths in flight.  A launch advances every in-flight path by one segment and ends with a tail in which the CUs run
    // dry one by one; the tails (and, for the split pipeline, the gaps between its three launches) only amortise over large
    // launches.  Measured on MI355X -- fused kernel, cbox 1024^2 @ 256 spp, scheduling waves per CU x slots per wave:
    // 16 x 256 -> 1753, 48 x 256 -> 1953, 72 x 512 -> 2366, 104 x 512 -> 2459, 208 x 1024 -> 2507 Msample/s (power-of-two
    // wave counts alias in the memory channels: 64 x 256 is slower than 72 x 256); split pipeline, 261 k-triangle mesh:
    // 16 / 64 / 128 / 208 waves per CU x 256 slots -> 705 / 1162 / 1339 / 1407 Msample/s; shadow-ring kernel (schedule 4), cbox:
    // 72 x 512 -> 2453, 104 x 512 -> 2554, 144 x 512 -> 2576, 208 x 512 -> 2629, 104 x 1024 -> 2598 Msample/s.  Split pipeline
    // after this round's traversal work (two-stream overlap included): 104 / 156 / 208 / 312 / 416 / 624 waves per CU x 256 slots
    // -> 1747 / 1890 / 1946 / 2075 / 2118 / 2142 Msample/s.
    js.target = d.paths_per_wave > 0 ? (uint32_t) d.paths_per_wave : (js.split ? 256u : 512u);
    js.target = std::min<uint32_t>(std::max<uint32_t>(js.target, 64u), 4096u);
    {   // no more scheduling waves than the pass can fill
        const uint64_t want = (std::min<uint64_t>(max_pass, js.pass_limit) + js.target - 1) / js.target;
        const uint64_t lo = (uint64_t) scene.cu_count * 16u, hi = (uint64_t) scene.cu_count * (js.split ? 416u : (js.shadow_ring ? 208u : 104u));
        js.n_waves = (uint32_t) std::min<uint64_t>(std::max<uint64_t>(want, lo), hi);
    }
    if (sw.waves_per_cu) js.n_waves = scene.cu_count * sw.waves_per_cu;
    // segments hold a multiple of 64 slots: k_shade deals whole 64-path chunks of a workgroup's list to its waves
    js.seg_cap = (js.target + 63u) & ~63u;
    return 0;
}

// The sample stream of a 2^30-sample pass is 24 GiB (twice that with the overlap buffer of multi-pass renders): when the device
// cannot provide it -- other scenes, the caller's own tensors -- the pass is halved until the workspace fits.
bool halve_pass(JobShape &js, uint64_t max_pass) {
    if (js.pass_limit <= (1ull << 22) || max_pass <= (1ull << 22)) return false;
    js.pass_limit = std::min(js.pass_limit, max_pass) >> 1;
    return true;
}

int plan_pass(const JobShape &js, uint64_t first, uint64_t n, int32_t finish_kernel, int32_t pipeline, uint64_t *cursor_end, PassPlan &plan) {
    const uint32_t nw = js.n_waves;
    const bool flat = js.scene.flat;
    // the pass's samples are dealt to the scheduling waves in chunks, round-robin (kernels.hip, cursor_sample): wave k owns the
    // chunks k, k + nw, ...; its cursor counts the samples of its own it has generated.  64-sample chunks for LDS-resident scenes
    // hierarchy scenes: four chunks of consecutive pixels per scheduling wave (a wave's 256 slots still hold neighbouring pixels, but
    // every wave sees four regions of the film, which evens out when the waves run dry: 1 / 4 / 16 / 64 chunks: 0 / +2.1 / +2.3 / +1.3 %
    // on the 261 k-triangle mesh at 1024 spp; 64-sample chunks as on flat scenes cost 5 %), at least 256 samples each
    const uint64_t cpw = js.sw.chunks_per_wave ? js.sw.chunks_per_wave : 4u;
    const uint64_t chunk = flat ? 64u : std::max<uint64_t>({ (n + nw * cpw - 1) / (nw * cpw), std::min<uint64_t>(256u, (n + nw - 1) / nw), 1u });
    const uint64_t n_chunks = (n + chunk - 1u) / chunk, last_size = n - (n_chunks - 1u) * chunk;
    // hierarchy scenes run several launch chains over parts of the scheduling waves: their chunks alternate (kernels.h, chunk_owner)
    uint32_t n_chains = 1;
    if (!flat && js.split && nw >= 256u) n_chains = kTraceChains;
    if (js.sw.chains) n_chains = js.sw.chains;
    if (js.sw.one_chain) n_chains = 1;
    while (n_chains > 1 && nw / n_chains < 2u * kChainAlign) --n_chains;
    for (uint32_t k = 0; k < nw; ++k) {
        const uint64_t c0 = chunk_owner(k, nw, n_chains);      // this wave owns the chunks c0, c0 + nw, ...
        const uint64_t mine = c0 < n_chunks ? (n_chunks - 1u - c0) / nw + 1u : 0u;
        uint64_t samples = mine * chunk;
        if (mine && (n_chunks - 1u) % nw == c0) samples -= chunk - last_size;       // the last, partial chunk of the pass
        cursor_end[k] = samples;
    }
    if (n >= (1ull << 31)) return fail(MTSAMD_ERR_INVALID, "a pass holds fewer than 2^31 samples");
    plan = PassPlan{};
    plan.chunk = (uint32_t) chunk; plan.n_chains = n_chains;
    plan.first_pix = (uint32_t) (first / (uint64_t) js.spp); plan.first_rem = (uint32_t) (first % (uint64_t) js.spp);
    plan.split = js.split_code();
    // Small passes of the automatic schedule: one launch of persistent lanes instead of launch rounds (kernels.hip, k_mega).  At most a
    // few samples per lane the launch count, not the kernel, sets the time: differentiable cbox 256^2 @ 1 spp, forward render
    // 0.33 ms of launch rounds.  LDS-resident scenes up to 2^19 samples, hierarchy scenes (where the wavefront kernels win sooner) 2^17.
    const uint64_t small_pass = flat ? (1ull << 19) : (1ull << 17);
    if (js.integrator != 0) plan.mode = PassMode::Direct;          // direct / depth: one launch finishes the whole pass
    else if (((pipeline == 0 && n <= small_pass) || js.sw.mega) && (plan.split == 1 || plan.split == 3) && !js.scene.nested_bsdfs) plan.mode = PassMode::Mega;
    else plan.mode = PassMode::Rounds;
    plan.min_iters = (n + (uint64_t) nw * js.target - 1) / ((uint64_t) nw * js.target);
    plan.n_parts = js.sw.streams ? js.sw.streams : 2u;
    if (plan.split != 3 || nw < 256u) plan.n_parts = 1;
    for (uint32_t k = 0; k < 5; ++k) plan.part_lo[k] = k ? nw : 0u;
    for (uint32_t k = 1; k < plan.n_parts; ++k) plan.part_lo[k] = (uint32_t) (((uint64_t) nw * k / plan.n_parts + 3u) & ~3ull);
    plan.part_lo[plan.n_parts] = nw;
    // pool size below which k_finish ends the pass (0: never).  Hierarchy scenes: measured flat between 2^20 and 2^24 (the fused kernel
    // keeps up with the launch rounds of the split pipeline once they are no longer full): 2^22; LDS-resident scenes, whose drain is
    // already compacted by the gathering: 2^18
    plan.finish_at = plan.split == 1 ? (1ull << 22) : (plan.split == 3 ? (1ull << 18) : 0ull);
    if (finish_kernel == 1) plan.finish_at = 0;                      // never (tests: the launch rounds run the pool dry)
    else if (finish_kernel == 2) plan.finish_at = 1ull << 40;       // as soon as the cursors are dry
    if (js.scene.nested_bsdfs) plan.finish_at = 0;                   // blendbsdf / mask: only the fused kernels carry the nesting code
    plan.gather_max = 4u;
    if (plan.split == 3 && !js.sw.no_gather) {
        plan.gather_max = 1024u;
        for (uint32_t k = 0; k <= plan.n_parts; ++k) while (plan.gather_max > 4u && plan.part_lo[k] % plan.gather_max) plan.gather_max >>= 2;
    }
    plan.split_parts = plan.split == 1 ? n_chains : 1u;
    for (uint32_t k = 0; k <= kMaxChains; ++k) plan.split_lo[k] = chain_first(k, nw, plan.split_parts);      // multiples of the k_trace group size
    return 0;
}

Drain::Verdict Drain::inspect(uint64_t it, const uint32_t *counts, const uint64_t *cursors, const uint64_t *cursor_end) {
    alive = 0;
    for (uint32_t k = 0; k < n_waves; ++k) alive += counts[k];
    if (alive == 0) return Done;
    bool dry = false;
    if (reads_cursors()) {
        dry = true;
        for (uint32_t k = 0; k < n_waves && dry; ++k) dry = cursors[k] >= cursor_end[k];
    }
    // every sample has been generated and few paths are left (the counts are a few launches old: an upper bound): one
    // k_finish launch instead of the dozens of near-empty launch rounds the deepest paths would still need
    if (dry && alive <= finish_at) return Finish;
    if (dry && finish_at) { stride = 1; next_check = it + 1; }
    // a workgroup may take up to eight segments' worth of paths on average (the counts are a few launches old: an
    // upper bound); a fuller group just takes longer, its survivors spill into the group's next waves
    while (dry && gather_w < gather_max && alive * (uint64_t) (4u * gather_w) <= 8ull * pool_slots) gather_w *= 4u;
    return GoOn;
}

int plan_film_passes(const RowMap &rows, uint64_t pass_cap, uint64_t per_row, FilmPasses &fp) {
    if (per_row > pass_cap) return fail(MTSAMD_ERR_UNSUPPORTED, "one film row (%llu samples) exceeds the pass capacity", (unsigned long long) per_row);
    fp.rows_per_pass = std::max<uint64_t>(1, pass_cap / per_row);
    fp.tile_h = 16;
    if (rows.count > 1) while (rows.tile_rows % fp.tile_h) fp.tile_h >>= 1;
    fp.tile_h_one = fp.tile_h;
    if (rows.count > 1) {
        if (fp.rows_per_pass >= (uint64_t) fp.tile_h) fp.rows_per_pass -= fp.rows_per_pass % (uint64_t) fp.tile_h;
        else { while (fp.rows_per_pass & (fp.rows_per_pass - 1)) fp.rows_per_pass &= fp.rows_per_pass - 1; fp.tile_h = (int32_t) fp.rows_per_pass; }
    }
    fp.n_passes = ((uint64_t) rows.local_rows + fp.rows_per_pass - 1) / fp.rows_per_pass;
    return 0;
}

void film_row_window(const RowMap &rows, uint64_t lr0, uint64_t nrows, int32_t R, int32_t crop_h, int32_t &row0, int32_t &row1) {
    // global rows are monotone in the local row index
    const int32_t g0 = row_to_global(rows, (int32_t) lr0), g1 = row_to_global(rows, (int32_t) (lr0 + nrows - 1));
    row0 = std::max<int32_t>(0, g0 - R); row1 = std::min<int32_t>(crop_h, g1 + R + 1);
}

bool film_tiles_supported(const FilterView &f) { return f.taps <= 4 && (int) ceilf(f.radius) <= 2; }
size_t film_partial_floats(const FilmParams &p) { return (size_t) p.slices * (size_t) p.tiles_x * (size_t) p.tiles_y * kFilmPartial; }
void film_tile_grid(FilmParams &p) {
    p.tiles_x = (p.crop_w + kFilmTile - 1) / kFilmTile;
    p.tiles_y = (p.pass_rows + p.tile_h - 1) / p.tile_h;
    // few tiles with many samples each (a rank's share of a partitioned film, a pass of a large film): cut the samples of a pixel
    // into runs of >= 64 so that about 2048 workgroups share the stream
    const int tiles = std::max(p.tiles_x * p.tiles_y, 1);
    p.slices = std::max(1, std::min({ 2048 / tiles, p.spp / 64, 64 }));
}

void film_splat_geometry(const RowMap &rows, const mtsamd_render_desc &d, int32_t R, bool tiled, uint64_t lr0, uint64_t nrows, int32_t tile_h, FilmParams &f) {
    const uint64_t per_row = (uint64_t) d.crop_width * (uint64_t) d.sample_count;
    f.first_ordinal = lr0 * per_row; f.n_samples = nrows * per_row; f.spp = d.sample_count; f.rows = rows;
    f.plane_pix0 = (uint32_t) (lr0 * (uint64_t) d.crop_width); f.plane_pixels = 0u;          // sample stream: pixel-major
    f.crop_x = d.crop_x; f.crop_y = d.crop_y; f.crop_w = d.crop_width; f.crop_h = d.crop_height;
    film_row_window(rows, lr0, nrows, R, d.crop_height, f.row0, f.row1);
    if (!tiled) return;
    f.pass_lr0 = (int32_t) lr0; f.pass_rows = (int32_t) nrows; f.tile_h = tile_h;
    film_tile_grid(f);
}

size_t film_reserve_floats(const FilmPasses &fp, int32_t local_rows, int32_t crop_w, int32_t spp, bool per_pass) {
    const uint64_t all = (uint64_t) local_rows, step = fp.rows_per_pass;
    FilmParams f{};
    f.crop_w = crop_w; f.spp = spp; f.tile_h = per_pass ? fp.tile_h : fp.tile_h_one;
    size_t need = 0;
    // fewer rows have fewer tiles but may have more sample runs: the largest need is found by evaluation, not at the largest row count
    auto take = [&](uint64_t nrows) { f.pass_rows = (int32_t) nrows; film_tile_grid(f); need = std::max(need, film_partial_floats(f)); };
    take(per_pass ? std::min(step, all) : all);
    if (per_pass) take(all % step);          // the short last pass (no rows: no tiles)
    else for (uint64_t done = step; done < all; done += step) take(done);
    return need;
}

} // namespace mtsamd

// schedule.h -- the host-only plan of the wavefront scheduler: everything that decides what a render job, a pass, the drain of a pass,
// the film passes and the splat of their rows (window, tile grid, scratch tiles) look like, as plain arithmetic.  Nothing declared here calls the HIP runtime or reads the environment (kernels.h is
// included for RowMap, chain_first and chunk_owner, which the kernels share), so every constant of the scheduler is tested on a machine
// without a GPU (tests/test_schedule_cpu.py); api.cpp carries the plan out: events, stream waits, copies, launches.
#pragma once
#include "../../include/mtsamd.h"
#include "kernels.h"
#include "scene_build.h"      // fail()

#include <cstdint>

namespace mtsamd {

// Experiment switches that feed the plan.  api.cpp fills them from the environment in builds made with -DMTSAMD_EXPERIMENTS and clamps
// them as it always did; 0 / false: not set, the shipped value holds.
struct ScheduleSwitches {
    uint32_t chunks_per_wave = 0;      // MTSAMD_CHUNKS_PER_WAVE (1 .. 64)
    uint32_t chains = 0;               // MTSAMD_CHAINS (1 .. kMaxChains)
    bool one_chain = false;            // MTSAMD_ONE_CHAIN
    uint32_t streams = 0;              // MTSAMD_STREAMS (1 .. 4)
    bool no_gather = false;            // MTSAMD_NO_GATHER
    bool mega = false;                 // MTSAMD_MEGA
    uint32_t waves_per_cu = 0;         // MTSAMD_WAVES_PER_CU (>= 1)
};

struct SceneFacts { bool flat, nested_bsdfs, spectral; uint32_t cu_count; };

// ---- job shape: the schedule of a render call and the size of its workspace ---------------------------------------------------
struct JobShape {
    SceneFacts scene{};
    ScheduleSwitches sw;
    int32_t integrator = 0, spp = 1;
    bool split = false, shadow_queue = false, shadow_ring = false;
    uint32_t target = 0, n_waves = 0, seg_cap = 0;      // paths a wave aims at, scheduling waves, slots per wave (a multiple of 64 >= target)
    uint64_t pass_limit = 0;                            // a pass holds min(max_pass, pass_limit) samples, at least one
    int32_t split_code() const { return shadow_ring ? 3 : (shadow_queue ? 2 : (split ? 1 : 0)); }      // RenderParams::split
    bool split_pools() const { return split || shadow_queue; }      // the workspace needs the hit / shadow-ray streams
};
// `d` has passed check_desc; max_pass: the samples the caller wants in one pass.  Refuses what the schedule cannot run.
int plan_job(const SceneFacts &scene, const mtsamd_render_desc &d, uint64_t max_pass, const ScheduleSwitches &sw, JobShape &js);
inline uint64_t pass_capacity(const JobShape &js, uint64_t max_pass) { const uint64_t c = max_pass < js.pass_limit ? max_pass : js.pass_limit; return c ? c : 1; }
// the workspace of pass_capacity() did not fit the device: halves the limit; false: the pass is as small as it gets
bool halve_pass(JobShape &js, uint64_t max_pass);

// ---- pass plan ----------------------------------------------------------------------------------------------------------------
enum class PassMode { Direct, Mega, Rounds };      // one k_direct launch | one k_mega launch | launch rounds until the pool is empty
struct PassPlan {
    uint32_t chunk, n_chains;          // RenderParams::chunk / n_chains: how cursor_sample (kernels.hip) deals the samples to the waves
    uint32_t first_pix, first_rem;     // first = first_pix * spp + first_rem
    PassMode mode;
    int32_t split;                     // RenderParams::split
    uint64_t min_iters;                // the sample cursors cannot run dry before this many launch rounds
    uint32_t n_parts, part_lo[5];      // shadow ring: part k = waves [part_lo[k], part_lo[k + 1]) on a stream of its own
    uint32_t split_parts, split_lo[kMaxChains + 1];      // split pipeline: launch chain k = waves [split_lo[k], split_lo[k + 1])
    uint32_t gather_max;               // largest gather_w of the pool drain (4: no gathering)
    uint64_t finish_at;                // pool size below which k_finish ends the pass (0: never)
};
// Plans the local sample ordinals [first, first + n) as one pass; cursor_end[k], k < n_waves: the samples scheduling wave k generates.
int plan_pass(const JobShape &js, uint64_t first, uint64_t n, int32_t finish_kernel, int32_t pipeline, uint64_t *cursor_end, PassPlan &plan);

// ---- drain state of the launch rounds -----------------------------------------------------------------------------------------
// Termination test without stalling the device: every `stride` launches the per-wave path counts (and cursors) are copied to pinned
// memory; the copy issued at the previous checkpoint (long complete) is inspected before a new one is issued.  While samples are left
// to generate a checkpoint every fourth launch round does; once the cursors are dry the pool only shrinks, the rounds get short and
// every round is checked (against the counts of the round before), so that k_finish takes over as soon as the pool is small enough.
// Pool drain of LDS-resident scenes: once every cursor is dry, a workgroup gathers the paths of gather_w consecutive scheduling waves at
// the front of the group (k_shade).  gather_w grows by powers of four as the pool empties -- decided on the counts read back; they are
// upper bounds, counts only shrink from then on -- and its groups lie inside one part.
struct Drain {
    enum Verdict { GoOn, Done, Finish };
    uint64_t min_iters, finish_at, pool_slots;      // pool_slots = seg_cap * n_waves
    uint32_t n_waves, gather_max;
    uint64_t stride = 4, next_check = 0;
    uint32_t gather_w = 4;             // RenderParams::gather_w of the next launch round
    uint64_t alive = 0;                // paths counted by the last inspect(); with Finish: what k_finish takes over
    Drain(const JobShape &js, const PassPlan &plan)
        : min_iters(plan.min_iters), finish_at(plan.finish_at), pool_slots((uint64_t) js.seg_cap * js.n_waves), n_waves(js.n_waves), gather_max(plan.gather_max) { }
    bool reads_cursors() const { return gather_w < gather_max || finish_at; }      // the cursors travel with the counts
    // is a checkpoint due after launch round `it` (1, 2, ...)?  If so the next one is `stride` rounds away.
    bool due(uint64_t it) { if (it < min_iters || it < next_check) return false; next_check = it + stride; return true; }
    // the read-back issued at the previous checkpoint, inspected at the checkpoint after round `it`
    Verdict inspect(uint64_t it, const uint32_t *counts, const uint64_t *cursors, const uint64_t *cursor_end);
};

// ---- film passes --------------------------------------------------------------------------------------------------------------
// Passes hold whole local rows.  The film kernel cuts a pass into source tiles of tile_h <= 16 local rows that must be contiguous on the
// film: with a partitioned film (interleaved row tiles) tile_h divides the partition's tile height and passes start on multiples of it.
struct FilmPasses {
    uint64_t rows_per_pass, n_passes;
    int32_t tile_h;                    // source tile height of these passes
    int32_t tile_h_one;                // ... and of the same rows splatted as one pass
};
// per_row: samples of one local row; refuses a row that exceeds the pass capacity
int plan_film_passes(const RowMap &rows, uint64_t pass_cap, uint64_t per_row, FilmPasses &fp);
// target (global) film rows [row0, row1) that the samples of the local rows [lr0, lr0 + nrows) reach through a filter of radius R
void film_row_window(const RowMap &rows, uint64_t lr0, uint64_t nrows, int32_t R, int32_t crop_h, int32_t &row0, int32_t &row1);

// ---- film splat ---------------------------------------------------------------------------------------------------------------
// Film::put of the local rows [lr0, lr0 + nrows) (api.cpp, FilmStage): launch_film_tiles for the filters it takes, else launch_film_gather.
bool film_tiles_supported(const FilterView &f);
void film_tile_grid(FilmParams &p);                 // tiles_x / tiles_y / slices from crop_w / pass_rows / tile_h / spp
size_t film_partial_floats(const FilmParams &p);    // size of `partials`
// Every geometry field of `f` for those rows of a render of `d` through a filter of radius R: ordinals, plane layout, crop, target row window
// and -- tiled, source tiles of tile_h rows -- the tile grid.  Left to the caller: the streams, the film, the filter and `partials`.
void film_splat_geometry(const RowMap &rows, const mtsamd_render_desc &d, int32_t R, bool tiled, uint64_t lr0, uint64_t nrows, int32_t tile_h, FilmParams &f);
// Scratch-tile floats a render reserves: the most any of its splats needs.  per_pass: every pass on its own (tile_h); otherwise one
// splat of the rows [0, rows_done) with tile_h_one, rows_done being any multiple of rows_per_pass a timeout can leave, or local_rows.
size_t film_reserve_floats(const FilmPasses &fp, int32_t local_rows, int32_t crop_w, int32_t spp, bool per_pass);

} // namespace mtsamd

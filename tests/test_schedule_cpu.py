"""The plan of the wavefront scheduler (mitsuba2_amd/csrc/schedule.{h,cpp}) without a GPU.  tests/schedule_driver.cpp is compiled with
schedule.cpp into a plain host program that prints the plans of the cases written here; every expectation is in this file.  The same
program is built a second time with -fsanitize=address,undefined and has to print the same.

* every sample of a pass is generated exactly once, whatever the chunk size and the number of launch chains;
* the boundaries of stream parts, launch chains and gathering groups;
* the schedule table of mtsamd_render_desc::pipeline / integrator, the clamps of the wave count, the target and the pass limit;
* direct / mega / launch rounds and their thresholds;
* the drain state machine on scripted read-backs;
* film passes and their target row windows;
* the splat of a pass: every geometry field of its FilmParams, the tile grid over its source pixels, the scratch tiles a render reserves."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mitsuba2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

INVALID, UNSUPPORTED = -1, -5
DIRECT, MEGA, ROUNDS = 0, 1, 2
GO_ON, DONE, FINISH = 0, 1, 2
CHAIN_ALIGN, MAX_CHAINS = 64, 8


def case(kind, name, script=(), **fields):
    line = " ".join([kind, name] + ["%s=%d" % kv for kv in fields.items()])
    return line + (" -- " + " ".join("%d %d" % (alive, dry) for alive, dry in script) if script else "")


def _value(text):
    if "," in text:
        return [int(x) for x in text.split(",")]
    try:
        return int(text)
    except ValueError:
        return text


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    tmp = tmp_path_factory.mktemp("schedule")
    exes, builds = [], []
    for tag, flags in (("plain", []), ("sanitized", ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"])):
        exes.append(str(tmp / tag))
        builds.append(subprocess.Popen([HIPCC, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, "-o", exes[-1], "-x", "hip", "--cuda-host-only"] + flags +
                                       [os.path.join(HERE, "schedule_driver.cpp"), os.path.join(CSRC, "schedule.cpp")], stderr=subprocess.PIPE, text=True))
    for b in builds:           # the two builds run side by side
        err = b.communicate()[1]
        assert b.returncode == 0, err

    def run(lines):
        """case lines -> {name: {key: value}}; a drain case also has "cp": the list of its checkpoints, a splat case "pass" and "once": the
        lists of its splats"""
        path = str(tmp / "cases.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        text = subprocess.check_output([exes[0], path], text=True)
        assert subprocess.check_output([exes[1], path], text=True) == text        # the sanitized build: no report, the same plans
        out, last = {}, None
        for line in text.splitlines():
            name, _, rest = line.partition(" ")
            if name == "message":
                last["message"] = rest
                continue
            words = rest.split()
            rec = {k: _value(v) for k, v in (w.split("=", 1) for w in words if "=" in w)}
            if words and words[0] in ("cp", "pass", "once"):
                out[name][words[0]].append(rec)
            else:
                rec.update(cp=[], once=[])
                rec["pass"] = []
                out[name] = last = rec
        assert len(out) == len(lines)
        return out
    return run


# ---- every sample exactly once -----------------------------------------------------------------------------------------------------------
# (name, fields, expected n_waves, expected n_chains): flat scenes take 64-sample chunks.  Scheduling waves per CU: 16 (the floor), 208 (the
# shadow ring's ceiling), 416 (the split pipeline's, pipeline 2 on a flat scene)
FLAT_SHAPES = [("flat_cu%d_w%d" % (cu, w), dict(flat=1, cu=cu, pipeline=pipe, max_pass=w * cu * target), w * cu, 1)
               for cu in (1, 4) for w, pipe, target in ((16, 0, 512), (208, 0, 512), (416, 2, 256))]
# hierarchy scenes: one chain below 256 waves, two from there on; a forced count steps down until every chain has 2 * kChainAlign waves
TREE_SHAPES = [
    ("tree_one_chain", dict(cu=1, max_pass=100 * 256), 100, 1),
    ("tree_two_chains", dict(cu=1, max_pass=416 * 256), 416, 2),
    ("tree_two_chains_cu4", dict(cu=4, max_pass=600 * 256), 600, 2),
    ("tree_three_chains", dict(cu=1, max_pass=1 << 30, chains=3), 416, 3),          # 128 <= 416 / 3
    ("tree_eight_chains", dict(cu=4, max_pass=1024 * 256, chains=8), 1024, 8),      # 128 <= 1024 / 8
    ("tree_eight_to_three", dict(cu=1, max_pass=1 << 30, chains=8), 416, 3),        # 416 / 8 .. 416 / 4 < 128 <= 416 / 3
    ("tree_three_to_two", dict(cu=1, max_pass=300 * 256, chains=3), 300, 2),        # 300 / 3 < 128 <= 300 / 2
    ("tree_three_to_one", dict(cu=1, max_pass=100 * 256, chains=3), 100, 1),
]


def sizes(nw, flat):
    if flat:
        return [1, 63, 64, 65, 64 * nw - 1, 64 * nw, 64 * nw + 1, 3 * 64 * nw + 17]
    return [1, 63, 64, 65, 4 * nw - 1, 4 * nw, 4 * nw + 1, 256 * nw - 1, 256 * nw, 256 * nw + 1, 3 * 256 * nw + 17]


@pytest.fixture(scope="module")
def passes(driver):
    """the pass plans of every shape and size above, walked by the driver: {name: (record, n_waves, n_chains, n, flat)}"""
    lines, expect = [], {}
    for name, fields, nw, chains in FLAT_SHAPES + TREE_SHAPES:
        for n in sizes(nw, fields.get("flat", 0)):
            key = "%s_n%d" % (name, n)
            lines.append(case("pass", key, n=n, **fields))
            expect[key] = (nw, chains, n, fields.get("flat", 0))
    out = driver(lines)
    return {key: (out[key],) + e for key, e in expect.items()}


def test_every_sample_is_generated_exactly_once(passes):
    assert len(passes) == 6 * 8 + 8 * 11
    for key, (rec, nw, chains, n, flat) in passes.items():
        assert rec["rc"] == 0 and rec["n_waves"] == nw and rec["n_chains"] == chains, (key, rec)
        assert rec["walk"] == "ok", (key, rec["walk"])
        if flat:
            assert rec["chunk"] == 64, key


def test_chunk_formula(driver):
    """hierarchy scenes: four chunks per wave, of at least 256 samples while the pass has that many per wave"""
    shape = dict(cu=1, max_pass=100 * 256)           # 100 scheduling waves
    out = driver([case("pass", "large", n=1000000, **shape), case("pass", "medium", n=50000, **shape), case("pass", "tiny", n=70, **shape)])
    assert [out[k]["n_waves"] for k in ("large", "medium", "tiny")] == [100] * 3
    assert out["large"]["chunk"] == 2500             # ceil(1e6 / 400) = 2500 > 256
    assert out["medium"]["chunk"] == 256             # ceil(5e4 / 400) = 125 < min(256, ceil(5e4 / 100) = 500)
    assert out["tiny"]["chunk"] == 1                 # ceil(70 / 400) = 1 = min(256, ceil(70 / 100) = 1)
    assert all(out[k]["walk"] == "ok" for k in out)


def test_a_pass_holds_fewer_than_2_31_samples(driver):
    out = driver([case("pass", "below", flat=1, cu=4, n=(1 << 31) - 1, walk=0), case("pass", "at", flat=1, cu=4, n=1 << 31, walk=0)])
    assert out["below"]["rc"] == 0
    assert (out["at"]["rc"], out["at"]["message"]) == (INVALID, "a pass holds fewer than 2^31 samples")


# ---- boundaries ----------------------------------------------------------------------------------------------------------------------------
def test_boundaries(passes, driver):
    ring = driver([case("pass", "ring_%d" % nw, flat=1, cu=16, pipeline=4, max_pass=nw * 512, n=nw * 512, finish_kernel=1, walk=0)
                   for nw in (256, 260, 1000, 1024, 2048, 3328)] + [case("pass", "ring_small", flat=1, cu=1, pipeline=0, max_pass=208 * 512, n=208 * 512, walk=0)])
    assert [ring["ring_%d" % nw]["gather_max"] for nw in (256, 260, 1000, 1024, 2048, 3328)] == [64, 4, 4, 256, 1024, 64]
    records = [(k, v[0]) for k, v in passes.items()] + list(ring.items())
    for key, rec in records:
        nw, parts, lo = rec["n_waves"], rec["n_parts"], rec["part_lo"]
        assert parts == (2 if rec["split_code"] == 3 and nw >= 256 else 1), key
        assert lo[0] == 0 and all(x % 4 == 0 for x in lo[:parts]) and lo[:parts + 1] == sorted(lo[:parts + 1]) and all(x == nw for x in lo[parts:]), (key, lo)
        g = rec["gather_max"]
        assert g in (4, 16, 64, 256, 1024) and all(x % g == 0 for x in lo[:parts + 1]), (key, g, lo)
        assert g == 1024 or rec["split_code"] != 3 or any(x % (4 * g) for x in lo[:parts + 1]), (key, "a larger group fits")
        if rec["split_code"] != 3:
            assert g == 4, key
        chains, slo = rec["split_parts"], rec["split_lo"]
        assert chains == (rec["n_chains"] if rec["split_code"] == 1 else 1), key
        assert slo == rec["chain_first"] and len(slo) == MAX_CHAINS + 1, key
        assert slo[0] == 0 and all(x % CHAIN_ALIGN == 0 for x in slo[:chains]) and all(x == nw for x in slo[chains:]), (key, slo)
    assert ring["ring_small"]["n_parts"] == 1 and ring["ring_2048"]["part_lo"] == [0, 1024, 2048, 2048, 2048]


# ---- schedule table --------------------------------------------------------------------------------------------------------------------------
# pipeline -> (split, shadow_queue, shadow_ring) of the path integrator on a scene without nested BSDFs
FLAT_TABLE = {0: (0, 0, 1), 1: (0, 0, 0), 2: (1, 0, 0), 3: (0, 1, 0), 4: (0, 0, 1)}
TREE_TABLE = {0: (1, 0, 0), 1: (0, 0, 0), 2: (1, 0, 0)}
SPECTRAL_DIRECT = "the direct and depth integrators are implemented for the RGB variant only"
QUEUES_ON_TREE = "pipelines 3 and 4 (queued shadow rays) apply to LDS-resident scenes only"


def expected_schedule(flat, nested, spectral, pipeline, integrator):
    if spectral and integrator != 0:
        return UNSUPPORTED, SPECTRAL_DIRECT
    if pipeline in (3, 4) and not flat:
        return INVALID, QUEUES_ON_TREE
    if nested or integrator != 0:          # only the fused kernels carry the nesting code; direct / depth are one launch
        return 0, (0, 0, 0)
    return 0, (FLAT_TABLE if flat else TREE_TABLE)[pipeline]


def test_schedule_table(driver):
    combos = [(f, ne, sp, p, i) for f in (0, 1) for ne in (0, 1) for sp in (0, 1) for p in range(5) for i in range(3)]
    out = driver([case("job", "j%d%d%d%d%d" % c, flat=c[0], nested=c[1], spectral=c[2], pipeline=c[3], integrator=c[4], cu=4) for c in combos])
    assert len(out) == 120
    for c in combos:
        rec, (rc, what) = out["j%d%d%d%d%d" % c], expected_schedule(*c)
        assert rec["rc"] == rc, c
        if rc:
            assert rec["message"] == what, c
        else:
            assert (rec["split"], rec["shadow_queue"], rec["shadow_ring"]) == what, c
            assert rec["target"] == (256 if what[0] else 512) and rec["seg_cap"] == rec["target"], c


def test_wave_count_target_and_pass_limit(driver):
    cu = 4
    shapes = {"split": dict(pipeline=0), "ring": dict(flat=1, pipeline=0), "fused": dict(flat=1, pipeline=1), "queue": dict(flat=1, pipeline=3)}
    lines = []
    for name, f in shapes.items():
        lines += [case("job", name + "_lo", cu=cu, max_pass=1, **f), case("job", name + "_hi", cu=cu, max_pass=1 << 30, **f),
                  case("job", name + "_mid", cu=cu, max_pass=100 * cu * 512 - 1, **f)]
    for ppw in (1, 64, 100, 128, 129, 4096, 5000):
        lines.append(case("job", "ppw%d" % ppw, flat=1, cu=cu, paths_per_wave=ppw))
    for log2 in (0, 5, 10, 20, 30, 40):
        lines.append(case("job", "log2_%d" % log2, flat=1, cu=cu, max_pass_log2=log2))
    lines += [case("job", "spass", flat=1, cu=cu, crop_w=100, crop_h=50, spp=64, samples_per_pass=16),
              case("job", "spass_row", flat=1, cu=cu, crop_w=100, crop_h=1, spp=64, samples_per_pass=16),
              case("job", "spass_log2", flat=1, cu=cu, crop_w=100, crop_h=50, spp=64, samples_per_pass=16, max_pass_log2=12),
              case("job", "limit_bounds_waves", flat=1, cu=cu, pipeline=1, max_pass_log2=16)]
    out = driver(lines)
    ceiling = {"split": 416, "ring": 208, "fused": 104, "queue": 104}
    for name in shapes:
        target = 256 if name == "split" else 512
        assert out[name + "_lo"]["n_waves"] == 16 * cu and out[name + "_hi"]["n_waves"] == ceiling[name] * cu, name
        assert out[name + "_mid"]["n_waves"] == (100 * cu * 512 - 1 + target - 1) // target, name       # as many waves as the pass fills
    assert [(out["ppw%d" % p]["target"], out["ppw%d" % p]["seg_cap"]) for p in (1, 64, 100, 128, 129, 4096, 5000)] == \
        [(64, 64), (64, 64), (100, 128), (128, 128), (129, 192), (4096, 4096), (4096, 4096)]
    assert [out["log2_%d" % k]["pass_limit"] for k in (0, 5, 10, 20, 30, 40)] == [1 << 30, 1 << 10, 1 << 10, 1 << 20, 1 << 30, 1 << 30]
    assert out["spass"]["pass_limit"] == 100 * 50 * 16
    assert out["spass_row"]["pass_limit"] == 100 * 64            # never less than one row of the crop window at the full sample count
    assert out["spass_log2"]["pass_limit"] == 1 << 12           # the smaller of the two limits holds
    assert out["limit_bounds_waves"]["n_waves"] == (1 << 16) // 512 > 16 * cu


# ---- mode ------------------------------------------------------------------------------------------------------------------------------------
def test_mode(driver):
    flat_limit, tree_limit = 1 << 19, 1 << 17
    big = dict(cu=4, walk=0)
    cases = {
        "direct": (dict(flat=1, integrator=1, n=1 << 22, **big), DIRECT), "depth": (dict(integrator=2, n=100, **big), DIRECT),
        "direct_small": (dict(flat=1, integrator=1, n=1, **big), DIRECT), "depth_nested": (dict(flat=1, nested=1, integrator=2, n=1 << 20, **big), DIRECT),
        "flat_at": (dict(flat=1, n=flat_limit, **big), MEGA), "flat_above": (dict(flat=1, n=flat_limit + 1, **big), ROUNDS),
        "tree_at": (dict(n=tree_limit, **big), MEGA), "tree_above": (dict(n=tree_limit + 1, **big), ROUNDS),
        "flat_one": (dict(flat=1, n=1, **big), MEGA), "tree_one": (dict(n=1, **big), MEGA),
        "flat_nested": (dict(flat=1, nested=1, n=1000, **big), ROUNDS), "tree_nested": (dict(nested=1, n=1000, **big), ROUNDS),
        "switch_nested": (dict(flat=1, nested=1, n=1000, mega=1, **big), ROUNDS),
        "switch_ring": (dict(flat=1, pipeline=4, n=1 << 22, mega=1, **big), MEGA), "switch_split": (dict(pipeline=2, n=1 << 22, mega=1, **big), MEGA),
        "switch_queue": (dict(flat=1, pipeline=3, n=1000, mega=1, **big), ROUNDS), "switch_fused": (dict(flat=1, pipeline=1, n=1000, mega=1, **big), ROUNDS),
    }
    for pipe in (1, 2, 3, 4):            # a forced schedule always runs launch rounds
        cases["flat_pipeline%d" % pipe] = (dict(flat=1, pipeline=pipe, n=1000, **big), ROUNDS)
    for pipe in (1, 2):
        cases["tree_pipeline%d" % pipe] = (dict(pipeline=pipe, n=1000, **big), ROUNDS)
    out = driver([case("pass", name, **fields) for name, (fields, _) in cases.items()])
    for name, (_, mode) in cases.items():
        assert (out[name]["rc"], out[name]["mode"]) == (0, mode), name
    assert out["flat_at"]["split_code"] == 3 and out["tree_at"]["split_code"] == 1


# ---- drain -----------------------------------------------------------------------------------------------------------------------------------
WET, DRY = 0, 1
RING = dict(flat=1, cu=16, pipeline=4, max_pass=2048 * 512)        # 2048 waves x 512 slots in two parts: gather_max = 1024
POOL = 2048 * 512


def grown(alive, gather_w, gather_max, pool=POOL):
    """the rule of the issue: alive * 4 * gather_w <= 8 * seg_cap * n_waves, by factors of four, never past gather_max"""
    while gather_w < gather_max and alive * 4 * gather_w <= 8 * pool:
        gather_w *= 4
    return gather_w


def test_drain_gathering(driver):
    # launch rounds only (finish_kernel 1); 3 rounds fill the pool
    script = [(100000, WET), (100000, DRY), (90000, DRY), (50, DRY), (0, DRY), (7, DRY)]
    d = driver([case("drain", "g", script, n=3 * POOL, finish_kernel=1, **RING)])["g"]
    assert (d["min_iters"], d["gather_max"], d["finish_at"], d["pool_slots"]) == (3, 1024, 0, POOL)
    cp = d["cp"]
    assert [c["it"] for c in cp] == [3, 7, 11, 15, 19, 23]                       # nothing before min_iters; the stride stays 4 without k_finish
    assert [c["inspected"] for c in cp] == [-1, 0, 1, 2, 3, 4]                   # the read-back of the checkpoint before, never the one just issued
    assert [c["verdict"] for c in cp] == [-1, GO_ON, GO_ON, GO_ON, GO_ON, DONE]
    assert [c["alive"] for c in cp[1:]] == [100000, 100000, 90000, 50, 0]
    w1 = grown(100000, 4, 1024)
    assert w1 == 64 and grown(90000, w1, 1024) == 64 and grown(50, 64, 1024) == 1024
    assert [c["gather_w"] for c in cp[:5]] == [4, 4, 64, 64, 1024]              # wet cursors: no growth, whatever the count
    assert all(c["stride"] == 4 for c in cp[:5])
    assert [c["reads_cursors"] for c in cp[:5]] == [1, 1, 1, 1, 0]               # at gather_max, without k_finish, the cursors stay on the device
    # the inequality, at its edge: 8 * POOL / (4 * 4) paths let 4 -> 16, one more does not
    edge = 8 * POOL // 16
    out = driver([case("drain", "at", [(edge, DRY), (edge, DRY)], n=POOL, finish_kernel=1, **RING),
                  case("drain", "above", [(edge + 1, DRY), (edge + 1, DRY)], n=POOL, finish_kernel=1, **RING),
                  case("drain", "small_groups", [(1, DRY), (1, DRY)], n=1000 * 512, finish_kernel=1, flat=1, cu=16, pipeline=4, max_pass=1000 * 512)])
    assert out["at"]["cp"][1]["gather_w"] == 16 and out["above"]["cp"][1]["gather_w"] == 4
    assert out["small_groups"]["gather_max"] == 4 and out["small_groups"]["cp"][1]["gather_w"] == 4


def test_drain_finish(driver):
    ring_at = 1 << 18
    out = driver([
        # the automatic rule of the shadow ring: k_finish once the cursors are dry and at most 2^18 paths are left
        case("drain", "ring", [(1000, WET), (300000, DRY), (ring_at + 1, DRY), (ring_at, DRY), (5, DRY)], n=2 * POOL, **RING),
        # ... of the split pipeline: 2^22
        case("drain", "split", [((1 << 22) + 1, DRY), (1 << 22, DRY), (1, DRY)], cu=4, n=1 << 24),
        case("drain", "asap", [(900000, WET), (900000, DRY), (1, DRY)], n=POOL, finish_kernel=2, **RING),
        case("drain", "never", [(1, DRY), (1, DRY), (0, DRY), (0, DRY)], n=POOL, finish_kernel=1, **RING),
        case("drain", "nested", [(1, DRY), (1, DRY), (0, DRY), (0, DRY)], n=POOL, finish_kernel=2, nested=1, flat=1, cu=16, max_pass=2048 * 512),
        case("drain", "fused", [(1, DRY), (0, DRY), (0, DRY)], n=POOL, finish_kernel=0, flat=1, pipeline=1, cu=16, max_pass=2048 * 512),
    ])
    cp = out["ring"]["cp"]
    assert out["ring"]["finish_at"] == ring_at and out["ring"]["min_iters"] == 2
    assert [c["verdict"] for c in cp] == [-1, GO_ON, GO_ON, GO_ON, FINISH]
    assert [c["it"] for c in cp] == [2, 6, 10, 11, 12]                            # every round is checked once the cursors are dry
    assert [c["stride"] for c in cp[:4]] == [4, 4, 1, 1] and cp[2]["next_check"] == 11
    assert cp[4]["alive"] == ring_at and cp[4]["inspected"] == 3                  # the hand-over carries the count that allowed it
    assert [c["gather_w"] for c in cp[:4]] == [4, 4, grown(300000, 4, 1024), grown(ring_at + 1, grown(300000, 4, 1024), 1024)]
    cp = out["split"]["cp"]
    assert out["split"]["finish_at"] == 1 << 22 and out["split"]["gather_max"] == 4
    assert [c["verdict"] for c in cp] == [-1, GO_ON, FINISH] and cp[2]["alive"] == 1 << 22 and cp[1]["stride"] == 1
    cp = out["asap"]["cp"]
    assert [c["verdict"] for c in cp] == [-1, GO_ON, FINISH] and cp[2]["alive"] == 900000 and cp[1]["stride"] == 4      # wet: nothing changes
    for name in ("never", "nested", "fused"):
        assert out[name]["finish_at"] == 0, name
        assert [c["verdict"] for c in out[name]["cp"]][-1] == DONE and FINISH not in [c["verdict"] for c in out[name]["cp"]], name
        assert all(c["stride"] == 4 for c in out[name]["cp"][:-1]), name
    assert not any(c["reads_cursors"] for c in out["nested"]["cp"][:-1]) and out["nested"]["gather_max"] == 4


# ---- film passes -----------------------------------------------------------------------------------------------------------------------------
def local_rows(crop_h, tile_rows, part, count):
    return sum(min(tile_rows, crop_h - t * tile_rows) for t in range(part, (crop_h + tile_rows - 1) // tile_rows, count))


def test_film_passes(driver):
    crop_h, per_row = 100, 64
    lines, meta = [], {}
    for rows_fit in (1, 2, 3, 5, 7, 15, 16, 17, 40, 1000):
        for R in (0, 1, 3):
            name = "window_%d_%d" % (rows_fit, R)
            lines.append(case("film", name, row0=10, local_rows=70, tile_rows=crop_h, part=0, count=1, crop_h=crop_h, pass_cap=rows_fit * per_row + 5, per_row=per_row, R=R))
            meta[name] = (rows_fit, 70, 1, crop_h)
            for count in (2, 3):
                for tile_rows in (8, 12, 16):
                    for part in range(count):
                        name = "part_%d_%d_%d_%d_%d" % (rows_fit, R, count, tile_rows, part)
                        lr = local_rows(crop_h, tile_rows, part, count)
                        lines.append(case("film", name, row0=0, local_rows=lr, tile_rows=tile_rows, part=part, count=count, crop_h=crop_h,
                                          pass_cap=rows_fit * per_row + 5, per_row=per_row, R=R))
                        meta[name] = (rows_fit, lr, count, tile_rows)
    lines.append(case("film", "row_too_long", local_rows=10, tile_rows=10, crop_h=10, pass_cap=63, per_row=64))
    out = driver(lines)
    assert (out["row_too_long"]["rc"], out["row_too_long"]["message"]) == (UNSUPPORTED, "one film row (64 samples) exceeds the pass capacity")
    for name, (rows_fit, lr, count, tile_rows) in meta.items():
        rec = out[name]
        rpp, th, th1 = rec["rows_per_pass"], rec["tile_h"], rec["tile_h_one"]
        passes = list(zip(rec["passes"][0::2], rec["passes"][1::2]))
        assert rec["rc"] == 0 and rec["n_passes"] == len(passes) == (lr + rpp - 1) // rpp, name
        # the passes cover every local row once, in order
        assert passes[0][0] == 0 and sum(n for _, n in passes) == lr and all(a + n == b for (a, n), (b, _) in zip(passes, passes[1:])), name
        assert 1 <= rpp <= rows_fit, name
        if count == 1:
            assert (rpp, th, th1) == (rows_fit, 16, 16), name
        else:
            assert th1 == max(h for h in (1, 2, 4, 8, 16) if tile_rows % h == 0), name
            assert tile_rows % th == 0 and th <= th1 and all(a % th == 0 for a, _ in passes), name
            if rows_fit < th1:
                assert rpp & (rpp - 1) == 0 and 2 * rpp > rows_fit and th == rpp, name      # the largest power of two that fits
            else:
                assert th == th1 and rpp == rows_fit - rows_fit % th1, name
        assert rec["window"] == rec["brute"], name          # min / max of row_to_global over the pass, widened by R, clamped to the crop
        assert all(0 <= a < b <= crop_h for a, b in zip(rec["window"][0::2], rec["window"][1::2])), name


# ---- film splat ------------------------------------------------------------------------------------------------------------------------------
FILM_TILE, FLOATS_PER_TILE = 16, 20 * 20 * 5          # source tile width; scratch tile: (16 + 2 * 2)^2 film pixels of 5 channels


def splat_case(name, crop_w, local, spp, rows_fit, R=2, partition=None, extra=0):
    """a render whose passes hold rows_fit local rows (+ `extra` samples); partition = (part, count, tile_rows) or None: rows [3, 3 + local)"""
    crop_h = local + 5 if partition is None else None
    if partition is None:
        rows = dict(row0=3, local_rows=local, tile_rows=crop_h, part=0, count=1)
    else:
        part, count, tile_rows = partition
        crop_h = local           # here `local` is the film height; the call owns its share of it
        rows = dict(row0=0, local_rows=local_rows(crop_h, tile_rows, part, count), tile_rows=tile_rows, part=part, count=count)
    fields = dict(crop_x=7, crop_y=2, crop_w=crop_w, crop_h=crop_h, spp=spp, R=R, pass_cap=rows_fit * crop_w * spp + extra, **rows)
    return case("splat", name, **fields), fields


def slices_rule(tiles, spp):
    """runs of >= 64 samples per pixel so that about 2048 workgroups share the stream, at most 64 of them"""
    return max(1, min(2048 // max(tiles, 1), spp // 64, 64))


SPLATS = [
    ("short_last_pass", dict(crop_w=96, local=64, spp=16, rows_fit=5, extra=11)),          # 12 passes of 5 rows and one of 4
    ("one_pass", dict(crop_w=33, local=40, spp=64, rows_fit=1000)),
    ("one_row_film", dict(crop_w=50, local=1, spp=64, rows_fit=1)),
    ("one_row_passes", dict(crop_w=17, local=9, spp=1, rows_fit=1, R=4)),
    ("spp1", dict(crop_w=100, local=70, spp=1, rows_fit=17, R=0)),
    ("spp64", dict(crop_w=100, local=70, spp=64, rows_fit=32, R=1)),
    ("spp4096", dict(crop_w=100, local=200, spp=4096, rows_fit=96)),                       # 6 x 7 tiles: 2048 // 42 = 48 slices; last pass 7 tiles: 64
    ("spp4096_few_tiles", dict(crop_w=16, local=20, spp=4096, rows_fit=7)),                # 1 - 2 tiles: 64 slices
    # 10 tile rows x 4 tiles take 51 slices (2040 scratch tiles), 8 x 4 take 64 (2048): fewer rows, more scratch
    ("short_needs_more", dict(crop_w=64, local=288, spp=4096, rows_fit=160)),              # per pass: 160 rows, then 128
    ("fewer_done_needs_more", dict(crop_w=64, local=160, spp=4096, rows_fit=128)),         # kept streams: [0, 128) against [0, 160)
] + [("tiles4_%d_%d" % (part, fit), dict(crop_w=40, local=50, spp=spp, rows_fit=fit, partition=(part, 2, 4)))
     for part, fit, spp in ((0, 3, 1), (1, 8, 64), (0, 9, 4096), (1, 1000, 64))] + \
    [("tiles32_%d_%d" % (part, fit), dict(crop_w=70, local=200, spp=spp, rows_fit=fit, partition=(part, 3, 32)))
     for part, fit, spp in ((0, 5, 64), (1, 16, 1), (2, 40, 4096), (0, 1000, 64), (2, 100, 64))]


def test_film_splats(driver):
    lines, meta = zip(*(splat_case(name, **kw) for name, kw in SPLATS))
    out = driver(list(lines))
    more = set()
    for (name, _), f in zip(SPLATS, meta):
        rec = out[name]
        per_row, lr_all, rpp = f["crop_w"] * f["spp"], f["local_rows"], rec["rows_per_pass"]
        assert rec["rc"] == 0 and rec["floats_per_tile"] == FLOATS_PER_TILE, name
        assert [(s["lr0"], s["nrows"]) for s in rec["pass"]] == [(a, min(rpp, lr_all - a)) for a in range(0, lr_all, rpp)] and len(rec["pass"]) == rec["n_passes"], name
        assert [(s["lr0"], s["nrows"]) for s in rec["once"]] == [(0, k) for k in range(rpp, lr_all, rpp)] + [(0, lr_all)], name
        for what, tile_h in (("pass", rec["tile_h"]), ("once", rec["tile_h_one"])):
            for s in rec[what]:
                key = (name, what, s["lr0"], s["nrows"])
                # ordinals and plane layout: the pass holds whole local rows, pixel-major
                assert (s["first_ordinal"], s["n_samples"], s["spp"]) == (s["lr0"] * per_row, s["nrows"] * per_row, f["spp"]), key
                assert (s["plane_pix0"], s["plane_pixels"], s["same_rows"]) == (s["lr0"] * f["crop_w"], 0, 1), key
                assert [s[k] for k in ("crop_x", "crop_y", "crop_w", "crop_h")] == [f[k] for k in ("crop_x", "crop_y", "crop_w", "crop_h")], key
                assert (s["row0"], s["row1"]) == (s["window0"], s["window1"]) and 0 <= s["row0"] < s["row1"] <= f["crop_h"], key          # film_row_window
                # the tile grid covers every source pixel of these rows exactly once, with tiles whose rows are contiguous on the film
                assert (s["pass_lr0"], s["pass_rows"], s["tile_h"]) == (s["lr0"], s["nrows"], tile_h), key
                assert s["tiles_x"] == -(-f["crop_w"] // FILM_TILE) and s["tiles_y"] == -(-s["nrows"] // tile_h), key
                assert s["walk"] == "ok", (key, s["walk"])
                assert s["slices"] == slices_rule(s["tiles_x"] * s["tiles_y"], f["spp"]), key
                assert s["need"] == s["slices"] * s["tiles_x"] * s["tiles_y"] * FLOATS_PER_TILE, key
            # the reservation covers every splat and is the largest need: nothing is reserved that no splat can use
            assert rec["reserve_" + what] == max(s["need"] for s in rec[what]), (name, what)
            assert all(rec["reserve_" + what] >= s["need"] for s in rec[what]), (name, what)
            if max(rec[what], key=lambda s: s["nrows"])["need"] < rec["reserve_" + what]:          # the splat of the most rows is not the largest
                more.add((name, what))
    # `slices` moves between 1 and 64 with the sample count
    assert {s["slices"] for s in out["spp1"]["pass"]} == {1} == {s["slices"] for s in out["spp64"]["pass"]}
    assert {s["slices"] for s in out["spp4096_few_tiles"]["pass"]} == {64} and [s["slices"] for s in out["spp4096"]["pass"]] == [48, 48, 64]
    assert out["one_row_film"]["pass"][0]["tiles_y"] == 1 and out["one_row_film"]["n_passes"] == 1 and out["one_row_passes"]["n_passes"] == 9
    assert out["short_last_pass"]["pass"][-1]["nrows"] == 4 and out["short_last_pass"]["n_passes"] == 13
    assert [out["tiles4_%d_%d" % k]["tile_h"] for k in ((0, 3), (1, 8), (0, 9), (1, 1000))] == [2, 4, 4, 4]
    assert [out["tiles32_%d_%d" % k]["tile_h"] for k in ((0, 5), (1, 16), (2, 40), (0, 1000), (2, 100))] == [4, 16, 16, 16, 16]
    # fewer rows can need more scratch than all of them: the full pass against the short last one, [0, 160) against [0, 128)
    short = out["short_needs_more"]["pass"]
    assert [(s["nrows"], s["slices"], s["need"] // FLOATS_PER_TILE) for s in short] == [(160, 51, 2040), (128, 64, 2048)]
    done = out["fewer_done_needs_more"]["once"]
    assert [(s["nrows"], s["need"] // FLOATS_PER_TILE) for s in done] == [(128, 2048), (160, 2040)]
    assert {("short_needs_more", "pass"), ("fewer_done_needs_more", "once")} <= more

"""The host half of mtsamd_scene_set_vertex_positions without a GPU: tests/refit_driver.cpp (built by vertex_moves.Driver) builds the
scenes of vertex_moves.py, moves vertices through the code the library shares between creation and the update, and dumps the arrays;
every expectation is here.

* build_bvh, now topology + emission, writes the bytes it wrote before the split (digests recorded on the parent commit);
* refit_bvh with the positions of creation reproduces build_bvh byte for byte: the five node arrays, the triangle slots, the box, the grid;
* every refitted child box, decoded from each of the five encodings as the device decodes it (box coordinate = q_lo + q * q_step; an fp16
  plane is a grid coordinate - 32768, a 15-bit plane half a grid coordinate), contains the padded box of every triangle beneath it --
  found by walking the builder's tree in numpy;
* after every move all arrays and host records (tri_pos, tri_nrm, area tables, emitter records, flat, pair and cluster records) equal those
  of a scene built from the moved description -- except the node arrays where the fresh build chose another topology, which is why the
  comparison of the hierarchy itself is the containment above and, after `shrink`, the root box and the grid;
* the device's restatement of the encodings (refit_encode.h) run on the host gives the words emit_bvh wrote, for every child box;
* the refusals: exact code and text, and the live scene's arrays unchanged by them;
* the driver built with -fsanitize=address,undefined runs the same moves clean (a stand-alone program: nothing is preloaded)."""
import os

import numpy as np
import pytest

import deep_walk
import vertex_moves as vm

F32, F64 = np.float32, np.float64
INVALID = -1          # MTSAMD_ERR_INVALID


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(vm.HIPCC):
        pytest.skip("hipcc not installed")
    return vm.Driver(tmp_path_factory.mktemp("refit"))


SCENES = {
    "sphere": lambda: vm.sphere_scene()[0],
    "cbox": lambda: vm.cbox_scene()[0],
    "soup65": lambda: vm.soup_scene(65)[0],
    "soup64": lambda: vm.soup_scene(64)[0],
    "leaf-root": lambda: vm.leaf_root_scene()[0],
    "slivers": lambda: deep_walk.slivers(256),
    "deep-render": deep_walk.deep_render_scene,
}
MOVES = [("sphere", n, m) for n, m in vm.SPHERE_MOVES.items()] + [("cbox", n, m) for n, m in vm.CBOX_MOVES.items()] + \
        [(n, "edge", m) for n, (_, m) in vm.EDGE_MOVES.items()]


def _same(out, a, b, keys):
    for k in keys:
        assert np.array_equal(out["%s.%s" % (a, k)], out["%s.%s" % (b, k)]), (a, b, k)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_refit_with_the_positions_of_creation_is_the_build(driver, name):
    out = driver.run(SCENES[name](), ["dump built", "rebuild refitted", "encode enc"], name)
    assert out["build.rc"] == 0, out["build.message"]
    _same(out, "built", "refitted", vm.ARRAYS + vm.RECORDS)
    # the exact boxes agree as numbers: the build unions triangles in its partition order, the refit children, and where zeros of both
    # signs meet the order decides the sign -- which no output keeps
    assert np.array_equal(out["built.rt_boxes"].view(F32), out["refitted.rt_boxes"].view(F32))
    boxes, mismatches = out["enc.encode"]
    counts = dict(zip(("root", "wroot", "wdepth", "n_nodes", "n_wnodes", "n_slots", "depth", "flat", "n_pairs", "n_clusters", "n_prims"), out["built.counts"]))
    assert mismatches == 0 and boxes >= 2 * counts["n_nodes"]
    if name == "leaf-root":
        assert counts["n_nodes"] == 0 and counts["n_wnodes"] == 0 and not counts["flat"] and counts["n_prims"] <= 4
    if name in ("soup64", "cbox"):
        assert counts["flat"]
    if name in ("soup65", "sphere"):
        assert not counts["flat"] and counts["n_nodes"] > 0


def test_build_bvh_still_writes_what_it_wrote_before_the_split(driver):
    """tests/golden/bvh_build_digests.json: SHA-256 of every array build_bvh produced for these scenes on the commit before build_bvh was
    split into topology and emission (recorded by running that commit's bvh.cpp on the same triangles)"""
    import hashlib
    import json
    with open(os.path.join(vm.HERE, "golden", "bvh_build_digests.json")) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(SCENES)
    for name in sorted(SCENES):
        out = driver.run(SCENES[name](), ["dump built"], name)
        for key, digest in golden[name].items():
            a = out["built." + key][:7] if key == "counts" else out["built." + key]          # root, wroot, wdepth, n_nodes, n_wnodes, n_slots, depth
            assert hashlib.sha256(np.ascontiguousarray(a, np.uint32).tobytes()).hexdigest() == digest, (name, key)


# ---- containment ---------------------------------------------------------------------------------------------------------------------------
def _half(h):
    return np.asarray(h, np.uint16).view(np.float16).astype(F64)


def _contained(out, label):
    """every child box of every encoding contains the padded box of each triangle beneath it; returns the number of boxes looked at"""
    g = lambda k: out["%s.%s" % (label, k)]
    left, right, ref2 = g("rt_left").view(np.int32), g("rt_right").view(np.int32), g("rt_ref2")
    tri = g("tri_pos").view(F32).astype(F64).reshape(-1, 3, 3)
    bbox = g("bbox").view(F32).astype(F64)
    extent = max(np.abs(bbox).max(), (bbox[3:] - bbox[:3]).max())
    lo, hi = tri.min(1), tri.max(1)
    pad = 1e-5 * np.maximum(np.maximum(np.abs(lo), np.abs(hi)), hi - lo) + 1e-7 * extent + 1e-30
    tlo, thi = lo - pad, hi + pad                                  # padded() of a triangle's own box, before the outward float rounding
    slot_prim = g("rt_slot_prim")
    n = len(left)
    need_lo, need_hi = np.full((n, 3), np.inf), np.full((n, 3), -np.inf)
    for t in range(n - 1, -1, -1):                                 # children follow their parent in the builder's array
        if left[t] >= 0:
            need_lo[t] = np.minimum(need_lo[left[t]], need_lo[right[t]]); need_hi[t] = np.maximum(need_hi[left[t]], need_hi[right[t]])
        else:
            first, count = int(ref2[t] & 0x07ffffff), int((ref2[t] >> 27) & 15)
            prims = slot_prim[first:first + count]
            assert count > 0
            need_lo[t], need_hi[t] = tlo[prims].min(0), thi[prims].max(0)
    grid = g("grid").view(F32).astype(F64)
    q_lo, q_step = grid[:3], grid[3:]
    looked = 0
    node_child = g("rt_node_child").view(np.int32)
    if len(node_child):
        nodes = g("nodes").view(F32).astype(F64).reshape(-1, 16)
        qn = g("qnodes").reshape(-1, 8)
        for side in (0, 1):
            t = node_child[side::2]
            assert (nodes[:, 6 * side:6 * side + 3] <= need_lo[t]).all() and (nodes[:, 6 * side + 3:6 * side + 6] >= need_hi[t]).all()
            w = qn[:, 3 * side:3 * side + 3]
            assert (q_lo + (w & 0xffff) * q_step <= need_lo[t]).all() and (q_lo + (w >> 16) * q_step >= need_hi[t]).all()
            looked += 2 * len(t)
    wide_child = g("rt_wide_child").view(np.int32)
    if len(wide_child):
        present = wide_child >= 0
        t = wide_child[present]
        planes = {
            "wnodes": lambda w: ((w & 0xffff).astype(F64), (w >> 16).astype(F64)),
            "wnodes_h": lambda w: (_half(w & 0xffff) + 32768.0, _half(w >> 16) + 32768.0),
            "wnodes_p": lambda w: (2.0 * (w & 0x7fff), 2.0 * ((w >> 16) & 0x7fff)),
        }
        for key, decode in planes.items():
            w = g(key).reshape(-1, 4)[present][:, :3]
            a, b = decode(w)
            assert (q_lo + a * q_step <= need_lo[t]).all() and (q_lo + b * q_step >= need_hi[t]).all(), key
            looked += len(t)
        absent = g("wnodes").reshape(-1, 4)[~present]
        assert (absent[:, 3] == 0x7fffffff).all()
    return looked


@pytest.mark.parametrize("scene,name,move", MOVES, ids=["%s-%s" % (s, n) for s, n, _ in MOVES])
def test_a_move_on_the_host_equals_a_scene_built_from_the_moved_vertices(driver, scene, name, move):
    sd = SCENES[scene]()
    shape, pos, nrm = move(sd)
    out = driver.run(sd, ["dump before"] + vm.move_text("move", shape, pos, nrm) + ["dump after", "fresh fresh", "encode enc"], "%s-%s" % (scene, name))
    assert out["build.rc"] == 0 and out["move.rc"] == 0, out.get("move.message")
    assert not np.array_equal(out["before.tri_pos"], out["after.tri_pos"])
    _same(out, "after", "fresh", vm.RECORDS + ("bbox", "grid"))
    assert _contained(out, "after") > 0 or scene == "leaf-root"
    assert _contained(out, "fresh") > 0 or scene == "leaf-root"
    assert out["enc.encode"][1] == 0
    # the slots hold the same triangle records, in the order of each tree's own leaves
    order = lambda label: np.argsort(out[label + ".rt_slot_prim"], kind="stable")
    assert np.array_equal(out["after.tris"].reshape(-1, 12)[order("after")], out["fresh.tris"].reshape(-1, 12)[order("fresh")])
    if name == "shrink":          # the refit does not only grow
        b0, b1 = out["before.bbox"].view(F32), out["after.bbox"].view(F32)
        assert (b1[3:] - b1[:3] <= b0[3:] - b0[:3]).all()
        hi_after = out["after.rt_boxes"].view(F32).reshape(-1, 6)
        assert (hi_after[:, 3:] - hi_after[:, :3]).sum() < (out["before.rt_boxes"].view(F32).reshape(-1, 6)[:, 3:] - out["before.rt_boxes"].view(F32).reshape(-1, 6)[:, :3]).sum()


def test_moving_back_restores_the_arrays_of_creation(driver):
    sd = SCENES["sphere"]()
    there = vm.SPHERE_MOVES["translate-out"](sd)
    back = (vm.SPHERE, np.asarray(sd["meshes"][vm.SPHERE]["positions"], F32), np.asarray(sd["meshes"][vm.SPHERE]["normals"], F32))
    out = driver.run(sd, ["dump before"] + vm.move_text("there", *there) + vm.move_text("back", *back) + ["dump after"], "back")
    assert out["there.rc"] == 0 and out["back.rc"] == 0
    _same(out, "before", "after", vm.ARRAYS + vm.RECORDS)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _refusals(sd):
    pos = lambda s: np.asarray(sd["meshes"][s]["positions"], F32).reshape(-1, 3).copy()
    nrm = np.asarray(sd["meshes"][vm.SPHERE]["normals"], F32)
    nan = pos(vm.FLOOR); nan[2, 1] = np.nan
    inf = pos(vm.SPHERE); inf[5, 0] = np.inf
    point = np.repeat(pos(vm.LIGHT)[:1], len(pos(vm.LIGHT)), 0)
    return {
        "bad-shape": ((7, pos(vm.FLOOR), None), "invalid shape index 7 (the scene has 3 shapes)"),
        "missing-normals": ((vm.SPHERE, pos(vm.SPHERE), None), "shape 0 was created with vertex normals: new normals are required with new positions"),
        "surplus-normals": ((vm.FLOOR, pos(vm.FLOOR), pos(vm.FLOOR)), "shape 1 was created without vertex normals: none can be set"),
        "nan": ((vm.FLOOR, nan, None), "shape 1: vertex 2 has a non-finite coordinate"),
        "inf": ((vm.SPHERE, inf, nrm), "shape 0: vertex 5 has a non-finite coordinate"),
        "no-area": ((vm.LIGHT, point, None), "DiscreteDistribution: no probability mass found!"),
    }


def test_refusals_on_the_host_write_nothing(driver):
    sd = SCENES["sphere"]()
    cases = _refusals(sd)
    commands = ["dump before"]
    for label, (move, _) in cases.items():
        commands += vm.move_text(label, *move) + ["dump after-" + label]
    good = vm.SPHERE_MOVES["light"](sd)
    out = driver.run(sd, commands + vm.move_text("good", *good) + ["dump after", "fresh fresh"], "refusals")
    for label, (_, text) in cases.items():
        assert out[label + ".rc"] == INVALID and out[label + ".message"] == text, (label, out[label + ".message"])
        _same(out, "before", "after-" + label, vm.ARRAYS + vm.RECORDS + ("rt_boxes",))
    assert out["good.rc"] == 0
    _same(out, "after", "fresh", vm.RECORDS + ("bbox", "grid"))


def test_refusals_through_the_abi_need_no_device():
    """what the C ABI can refuse without a scene, and that both entry points are exported with the declared signatures"""
    import ctypes as C
    from mitsuba2_amd import _lib as L
    lib = L.lib()
    buf = (C.c_float * 9)()
    assert lib.mtsamd_scene_set_vertex_positions(None, 0, buf, None, None) == INVALID
    assert lib.mtsamd_last_error() == b"null scene"
    assert lib.mtsamd_scene_read_accel(None, 0, buf, 36) == INVALID
    assert lib.mtsamd_last_error() == b"null argument"


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path):
    if not os.path.exists(vm.HIPCC):
        pytest.skip("hipcc not installed")
    san = vm.Driver(tmp_path, flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    sd = SCENES["sphere"]()
    commands = []
    for name in ("translate-out", "collapse", "light", "floor"):
        commands += vm.move_text(name, *vm.SPHERE_MOVES[name](sd))
    for label, (move, _) in _refusals(sd).items():
        commands += vm.move_text(label, *move)
    out = san.run(sd, commands + ["dump after", "rebuild again", "encode enc"], "sanitized")
    assert out["translate-out.rc"] == 0 and out["no-area.rc"] == INVALID and out["enc.encode"][1] == 0
    cb = SCENES["cbox"]()
    out = san.run(cb, vm.move_text("light", *vm.CBOX_MOVES["light"](cb)) + ["dump after"], "sanitized-flat")
    assert out["light.rc"] == 0

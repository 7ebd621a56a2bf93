"""build_sah_levels, the host specification of the SAH accelerator rebuild, without a GPU: tests/sah_levels_driver.cpp (built by
sah_cases.Driver) builds the tree for the inputs below beside build_bvh's and dumps every array and what every node decided.

Inputs: lbvh_cases.copies(), coplanar(), one_bit(), soup_triangles(n) for n in 1..5, 65, 255, 256, 257 and 1025, the sphere of vertex_moves
as built and after each of its moves, deep_walk.slivers(256), a skewed set (a level of many nodes with a large one among them), the threshold set
(nodes of 64 and of 65 primitives) and the depth-guard set of sah_cases.

* against build_bvh: the same counts and depths; nodes, qnodes, wnodes, wnodes_h, wnodes_p and grid byte for byte; the leaves tile the
  slots identically and tris / slot_prim are equal after sorting the records of each leaf by primitive; the SAH cost as a multiset of
  terms: the per-node terms of sah_cost_blocked, sorted, are equal bit for bit (the two builders number the builder nodes differently, so
  the blocked sums differ in their order of addition; the sums themselves are also held to 1e-12 relative);
* replay: sah_cases.replay restates the rules in numpy float64 from the triangles alone; kids, node_child, slot_prim, and per builder
  node its range, depth, decision (leaf rule, split choice, cost bit for bit) and left count equal the driver's, the dumped bins of the
  first 16 nodes equal numpy's, heights / order / class_start are consistent, every leaf holds ascending primitives;
* the depth guard: 45 levels, the splits at depth >= 40 are middle-of-order, refit_bvh with the same positions reproduces the output;
* refit_bvh with the positions of the build reproduces it, for every input;
* the driver built with -fsanitize=address,undefined runs the same inputs clean (a stand-alone program: nothing is preloaded)."""
import os

import numpy as np
import pytest

import deep_walk
import lbvh_cases as lc
import sah_cases as sc
import vertex_moves as vm

F32, F64, I32 = np.float32, np.float64, np.int32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(vm.HIPCC):
        pytest.skip("hipcc not installed")
    return sc.Driver(tmp_path_factory.mktemp("sah_levels"))


def _sphere(*moves):
    return deep_walk.triangles(vm.moved(vm.sphere_scene()[0], *moves))


RAW = {"copies": lc.copies, "coplanar": lc.coplanar, "one-bit": lc.one_bit, "sphere": _sphere, "slivers256": lambda: deep_walk.triangles(deep_walk.slivers(256)),
       "skewed": sc.skewed, "threshold": sc.threshold_set, "guard": sc.depth_guard_set}
for _n in (1, 2, 3, 4, 5, 65, 255, 256, 257, 1025):
    RAW["n%d" % _n] = (lambda n: lambda: lc.soup_triangles(n))(_n)
for _m in sorted(vm.SPHERE_MOVES):
    RAW["sphere-" + _m] = (lambda m: lambda: _sphere(vm.SPHERE_MOVES[m]))(_m)


@pytest.fixture(scope="module")
def raw(driver):
    commands = []
    for name in sorted(RAW):
        commands += lc.raw_text(name, RAW[name]())
    return driver.run(None, commands, "raw")


def _kids(out, label):
    return out[label + ".kids"].view(I32).reshape(-1, 2)


def _terms(out, label):
    kids, boxes = _kids(out, label), out[label + ".boxes"].view(F32).reshape(-1, 6)
    area, inner = sc.sah_terms(kids, boxes)
    root = area[int(out[label + ".rt_root"].view(I32)[0])]
    if not root > 0:
        return np.zeros(len(kids))
    count = (kids[:, 1].view(np.uint32) >> 27) & 15
    return np.sort(np.where(inner, area / root, 1.5 * (count.astype(F64) * (area / root))))


def assert_same_tree_as_creation(out, a, b):
    """tree `a` (build_sah_levels) against tree `b` (build_bvh)"""
    assert np.array_equal(out[a + ".counts"], out[b + ".counts"]), (lc.counts(out, a), lc.counts(out, b))
    for k in ("nodes", "qnodes", "wnodes", "wnodes_h", "wnodes_p", "grid", "bbox"):
        assert np.array_equal(out[a + "." + k], out[b + "." + k]), k
    la = sc.leaf_sets(_kids(out, a), out[a + ".slot_prim"], out[a + ".tris"])
    lb = sc.leaf_sets(_kids(out, b), out[b + ".slot_prim"], out[b + ".tris"])
    assert la == lb
    assert all(prims == sorted(prims) for _, prims, _ in la)
    assert np.array_equal(out[a + ".slot_prim"], np.concatenate([np.array(p, np.uint32) for _, p, _ in la]))          # ascending inside every leaf, as stored
    assert _terms(out, a).tobytes() == _terms(out, b).tobytes()
    assert lc.sah(out, a) == pytest.approx(lc.sah(out, b), rel=1e-12)


@pytest.mark.parametrize("name", sorted(set(RAW) - {"guard"}))          # the guard's splits are the one documented difference (bvh.h)
def test_the_tree_is_creations(raw, name):
    assert_same_tree_as_creation(raw, name, name + "b")


@pytest.mark.parametrize("name", sorted(RAW))
def test_the_tree_is_the_replayed_one(raw, name):
    tri = RAW[name]()
    want = sc.replay(tri)
    g = lambda k: raw["%s.%s" % (name, k)]
    kids = _kids(raw, name)
    assert np.array_equal(kids, want["kids"]) and np.array_equal(g("node_child").view(I32).reshape(-1, 2), want["node_child"])
    assert np.array_equal(g("slot_prim"), want["slot_prim"])
    first, count, depth, mode, left, axis, b, cost = (np.array(x) for x in zip(*want["nodes"]))
    for key, col in (("t_first", first), ("t_count", count), ("t_depth", depth), ("t_mode", mode), ("t_left", left)):
        assert np.array_equal(g(key), col.astype(np.uint32)), key
    assert np.array_equal(g("t_axis").view(I32), axis.astype(I32)) and np.array_equal(g("t_bin").view(I32), b.astype(I32))
    assert g("t_cost").view(F64).tobytes() == cost.astype(F64).tobytes()
    # numbering: builder nodes level by level, BVH2 nodes = split nodes in that order, references
    inner = kids[:, 0] >= 0
    assert np.array_equal(g("ref2")[inner], np.arange(inner.sum())) and np.array_equal(g("ref2")[~inner], kids[~inner, 1].view(np.uint32))
    assert np.array_equal(np.sort(depth), depth) and (kids[inner, 1] == kids[inner, 0] + 1).all()
    assert np.array_equal(kids[inner, 0], 1 + 2 * np.arange(inner.sum()))
    # heights, order, classes; the depth
    height = np.zeros(len(kids), np.int64)
    for t in range(len(kids) - 1, -1, -1):          # children follow their parents
        if inner[t]:
            height[t] = 1 + max(height[kids[t, 0]], height[kids[t, 1]])
    assert np.array_equal(height, g("height")) and np.array_equal(g("order"), np.argsort(height, kind="stable"))
    assert np.array_equal(g("class_start"), np.concatenate([[0], np.cumsum(np.bincount(height))]))
    c = lc.counts(raw, name)
    assert c["depth"] == height[0] + 1 == want["levels"] and c["n_nodes"] == inner.sum() and c["n_slots"] == len(tri)
    # the bins of the first nodes: counts, and the boxes of the bins that hold something
    assert [int(x) for x in g("t_bins_node")] == [t for t, _ in want["bins"]]
    words = g("t_bins").reshape(len(want["bins"]), 3 * sc.BINS * 7)
    unord = lambda k: np.where(k & 0x80000000, k & 0x7fffffff, ~k).astype(np.uint32).view(F32)
    for row, (t, bins) in zip(words, want["bins"]):
        lo, hi, cnt = unord(row[:144]).reshape(3, sc.BINS, 3), unord(row[144:288]).reshape(3, sc.BINS, 3), row[288:].reshape(3, sc.BINS)
        for a in range(3):
            if bins[a] is None:
                assert not cnt[a].any()
                continue
            _, ncnt, blo, bhi = bins[a]
            assert np.array_equal(cnt[a], ncnt), (t, a)
            full = ncnt > 0
            assert np.array_equal(lo[a][full].astype(F64), blo[full]) and np.array_equal(hi[a][full].astype(F64), bhi[full]), (t, a)
            assert (row[:144].reshape(3, sc.BINS, 3)[a][~full] == 0xffffffff).all() and (row[144:288].reshape(3, sc.BINS, 3)[a][~full] == 0).all()


@pytest.mark.parametrize("name", sorted(RAW))
def test_refit_with_the_positions_of_the_build_is_the_build(raw, name):
    for k in lc.NODE_ARRAYS + lc.TABLE_ARRAYS + ("counts", "bbox", "class_start", "height", "ref2", "ref4", "sah"):
        assert np.array_equal(raw["%s.%s" % (name, k)], raw["%sr.%s" % (name, k)]), (name, k)


def test_edges(raw):
    for name, leaves in (("n1", 1), ("n2", 2), ("copies", 17)):
        assert (_kids(raw, name)[:, 0] < 0).sum() == leaves, name
    assert set(raw["copies.t_mode"]) == {sc.LEAF, sc.SPLIT_MIDDLE} and (raw["copies.t_axis"].view(I32) == -1).all()          # no candidate anywhere
    # the sizes at which the device takes another path are among the inputs: a node of WAVE_NODE and of WAVE_NODE + 1 primitives, levels
    # of fewer than and of at least SHARE_LEVEL nodes, and a node above WAVE_NODE in a level of at least SHARE_LEVEL
    assert list(raw["threshold.t_count"][:3]) == [2 * sc.WAVE_NODE + 1, sc.WAVE_NODE, sc.WAVE_NODE + 1]
    depth, count = raw["skewed.t_depth"], raw["skewed.t_count"]
    assert any((depth == d).sum() >= sc.SHARE_LEVEL and count[depth == d].max() > sc.WAVE_NODE for d in np.unique(depth))


def test_the_depth_guard(raw):
    """the set of sah_cases.depth_guard_set: 45 levels; from depth 40 on every split is the middle of the order"""
    c = lc.counts(raw, "guard")
    assert c["depth"] == 45
    depth, mode, count, left = (raw["guard.t_" + k] for k in ("depth", "mode", "count", "left"))
    deep = (depth >= sc.GUARD_DEPTH) & (mode != sc.LEAF)
    assert deep.sum() >= 1 and (mode[deep] == sc.SPLIT_MIDDLE).all() and np.array_equal(left[deep], count[deep] // 2)
    assert (raw["guard.t_axis"].view(I32)[deep] >= 0).all()          # the search had a candidate: the guard overrode it
    shallow = (depth < sc.GUARD_DEPTH) & (mode != sc.LEAF)
    assert (mode[shallow] == sc.SPLIT_BIN).all()
    for k in lc.NODE_ARRAYS + lc.TABLE_ARRAYS + ("counts", "bbox", "sah"):
        assert np.array_equal(raw["guard." + k], raw["guardr." + k]), k


@pytest.mark.parametrize("name", sorted(vm.SPHERE_MOVES))
def test_a_live_scene_after_a_move(driver, name):
    """through the scene path: the triangles the live scene holds after set_vertex_positions"""
    sd = vm.sphere_scene()[0]
    out = driver.run(sd, ["sahl before", "bvh before_b"] + vm.move_text("move", *vm.SPHERE_MOVES[name](sd)) + ["sahl after", "bvh after_b", "refit refitted"], "move-" + name)
    assert out["build.rc"] == 0 and out["move.rc"] == 0
    assert_same_tree_as_creation(out, "before", "before_b")
    assert_same_tree_as_creation(out, "after", "after_b")
    assert not np.array_equal(out["before.tri_pos"], out["after.tri_pos"])


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path):
    if not os.path.exists(vm.HIPCC):
        pytest.skip("hipcc not installed")
    san = sc.Driver(tmp_path, flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    commands = []
    for name in sorted(RAW):
        commands += lc.raw_text(name, RAW[name]())
    out = san.run(None, commands, "sanitized-raw")
    assert lc.counts(out, "guard")["depth"] == 45 and lc.counts(out, "n1025")["n_slots"] == 1025
    sd = vm.sphere_scene()[0]
    out = san.run(sd, ["sahl before"] + vm.move_text("move", *vm.SPHERE_MOVES["collapse"](sd)) + ["refit after", "sahl fresh", "bvh creation"], "sanitized-scene")
    assert out["move.rc"] == 0 and lc.counts(out, "fresh") == lc.counts(out, "creation")


def test_refusals_through_the_abi_need_no_device():
    from mitsuba2_amd import _lib as L
    lib = L.lib()
    assert lib.mtsamd_scene_rebuild_accel_with(None, 0, 0, None) == -1 and lib.mtsamd_last_error() == b"null scene"

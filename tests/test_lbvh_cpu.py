"""build_lbvh, the host specification of the accelerator rebuild, without a GPU: tests/lbvh_driver.cpp (built by lbvh_cases.Driver) builds the
tree for the inputs below and dumps every array; every expectation is here, recomputed in numpy from the dumped topology.

Inputs: 1, 2, 4 and 5 triangles (leaf size 4: one leaf up to 4, the first split at 5); flat_limits.soup(65); scenes.bumpy_sphere(8, 16) as
built and after squash / scale / collapse moves; deep_walk.sliver_triangles, whose centres nearly coincide; 65 copies of one triangle
(all codes equal); a coplanar soup (an axis without extent); the 30 one-bit codes (a chain).

* every primitive sits in exactly one slot, the slots are in (code, primitive) order with the codes recomputed here, leaves hold 1..4;
* every builder box is the union of its children's, or of its triangles;
* height / order / class_start are consistent; depth and wdepth are recomputed from kids / wide_child; depth <= 31 + ceil(log2 n);
* the BVH4 collapse is build_bvh's rule, replayed here per wide node; wide nodes are numbered level by level;
* refit_bvh with the same positions reproduces build_lbvh byte for byte; after a move it gives the boxes of the moved triangles over
  the same topology, and the scene box and grid of a tree built for the moved triangles;
* the fit predicate on both sides of its limit; the SAH cost against a plain numpy sum;
* the driver built with -fsanitize=address,undefined runs the same inputs clean (a stand-alone program: nothing is preloaded)."""
import math
import os

import numpy as np
import pytest

import deep_walk
import lbvh_cases as lc
import vertex_moves as vm

F32, F64, I32 = np.float32, np.float64, np.int32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(vm.HIPCC):
        pytest.skip("hipcc not installed")
    return lc.Driver(tmp_path_factory.mktemp("lbvh"))


def _sphere(*moves):
    return deep_walk.triangles(vm.moved(vm.sphere_scene()[0], *moves))


RAW = {
    "n1": lambda: lc.soup_triangles(65)[:1], "n2": lambda: lc.soup_triangles(65)[:2], "n4": lambda: lc.soup_triangles(65)[:4],
    "n5": lambda: lc.soup_triangles(65)[:5], "soup65": lambda: lc.soup_triangles(65), "sphere": _sphere,
    "sphere-squash": lambda: _sphere(vm.SPHERE_MOVES["squash"]), "sphere-scale": lambda: _sphere(vm.SPHERE_MOVES["shrink"]),
    "sphere-collapse": lambda: _sphere(vm.SPHERE_MOVES["collapse"]), "slivers65": lambda: deep_walk.sliver_triangles(65),
    "slivers256": lambda: deep_walk.sliver_triangles(256), "copies": lc.copies, "coplanar": lc.coplanar, "one-bit": lc.one_bit,
}


def _tree(out, label):
    g = lambda k: out["%s.%s" % (label, k)]
    return dict(kids=g("kids").view(I32).reshape(-1, 2), order=g("order"), class_start=g("class_start"), height=g("height"), ref2=g("ref2"), ref4=g("ref4"),
                node_child=g("node_child").view(I32).reshape(-1, 2), wide_child=g("wide_child").view(I32).reshape(-1, 4), slot_prim=g("slot_prim"),
                boxes=g("boxes").view(F32).reshape(-1, 6), tri=g("tri_pos").view(F32).reshape(-1, 3, 3), counts=lc.counts(out, label))


def _boxes(t, tri):
    """exact boxes over the topology, children before parents by the dumped order (whose consistency _check_heights asserts)"""
    kids = t["kids"]
    boxes = np.zeros((len(kids), 6), F32)
    for b in t["order"]:
        l, r = kids[b]
        if l < 0:
            ref = np.uint32(r)
            first, count = int(ref & 0x07ffffff), int((ref >> 27) & 15)
            p = tri[t["slot_prim"][first:first + count]].reshape(-1, 3)
            boxes[b] = np.concatenate([p.min(0), p.max(0)])
        else:
            boxes[b] = np.concatenate([np.minimum(boxes[l, :3], boxes[r, :3]), np.maximum(boxes[l, 3:], boxes[r, 3:])])
    return boxes


def _area(b):
    d = b[..., 3:].astype(F64) - b[..., :3].astype(F64)
    return 2.0 * (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])


def _check(name, t):
    tri, kids, c = t["tri"], t["kids"], t["counts"]
    n = len(tri)
    inner = kids[:, 0] >= 0
    # slots: the (code, primitive) order, every primitive once; leaves tile the slots and hold 1 .. MAX_LEAF
    assert np.array_equal(t["slot_prim"], np.argsort(lc.morton_codes(tri), kind="stable")), name
    assert np.array_equal(np.sort(t["slot_prim"]), np.arange(n))
    refs = kids[~inner, 1].view(np.uint32)
    first, count = refs & 0x07ffffff, (refs >> 27) & 15
    assert (refs >> 31).all() and count.min() >= 1 and count.max() <= lc.MAX_LEAF
    o = np.argsort(first)
    assert first[o][0] == 0 and np.array_equal(first[o][1:], np.cumsum(count[o])[:-1]) and count.sum() == n == c["n_slots"]
    assert len(kids) == 2 * inner.sum() + 1 and c["n_nodes"] == inner.sum()
    # a leaf's parent covers more than MAX_LEAF: the leaves are as large as the rule allows
    covered = np.zeros(len(kids), np.int64)
    covered[~inner] = count
    # heights, order, classes
    height = np.zeros(len(kids), np.int64)
    for b in t["order"]:
        if inner[b]:
            height[b] = 1 + max(height[kids[b, 0]], height[kids[b, 1]])
            covered[b] = covered[kids[b, 0]] + covered[kids[b, 1]]
    assert np.array_equal(height, t["height"])
    assert np.array_equal(t["order"], np.argsort(height, kind="stable"))
    assert np.array_equal(t["class_start"], np.concatenate([[0], np.cumsum(np.bincount(height))]))
    assert covered[0] == n and (covered[inner] > lc.MAX_LEAF).all()
    assert c["depth"] == height[0] + 1 and c["depth"] - 1 <= 31 + math.ceil(math.log2(n)) if n > 1 else c["depth"] == 1
    # every child has one parent, the root none
    parents = np.bincount(kids[inner].reshape(-1), minlength=len(kids))
    assert parents[0] == 0 and (parents[1:] == 1).all()
    # boxes
    assert np.array_equal(_boxes(t, tri), t["boxes"]), name
    # BVH2 numbering: inner builder nodes in index order; references
    assert np.array_equal(t["node_child"], kids[inner])
    assert np.array_equal(t["ref2"][inner], np.arange(inner.sum())) and np.array_equal(t["ref2"][~inner], refs)
    if not inner.any():
        assert c["root"] == c["wroot"] == refs[0] and c["n_wnodes"] == 0 and c["wdepth"] == 1 and len(t["wide_child"]) == 0
        return
    # BVH4: replay the collapse per wide node, level by level
    area = _area(t["boxes"])
    wide, level, depth = [], [0], 0
    ref4 = {0: 0}
    while level:
        depth += 1
        nxt = []
        for b in level:
            ch = [int(kids[b, 0]), int(kids[b, 1])]
            while len(ch) < 4:
                cand = [(area[x], -i) for i, x in enumerate(ch) if inner[x]]
                if not cand:
                    break
                i = -max(cand)[1]
                x = ch[i]
                ch[i] = int(kids[x, 0]); ch.append(int(kids[x, 1]))
            wide.append(ch + [-1] * (4 - len(ch)))
        for ch in wide[len(wide) - len(level):]:
            for x in ch:
                if x >= 0 and inner[x]:
                    ref4[x] = len(wide) + len(nxt); nxt.append(x)
        level = nxt
    assert np.array_equal(np.array(wide, I32), t["wide_child"]), name
    assert c["wdepth"] == depth and c["n_wnodes"] == len(wide) and c["root"] == c["wroot"] == 0
    assert c["stack_depth"] == 3 * depth + 2
    for x, w in ref4.items():
        assert t["ref4"][x] == w
    assert np.array_equal(t["ref4"][~inner], refs)


@pytest.fixture(scope="module")
def raw(driver):
    commands = []
    for name in sorted(RAW):
        commands += lc.raw_text(name, RAW[name]())
    return driver.run(None, commands, "raw")


@pytest.mark.parametrize("name", sorted(RAW))
def test_the_tree_is_the_specified_one(raw, name):
    _check(name, _tree(raw, name))


@pytest.mark.parametrize("name", sorted(RAW))
def test_refit_with_the_positions_of_the_build_is_the_build(raw, name):
    for k in lc.NODE_ARRAYS + lc.TABLE_ARRAYS + ("counts", "bbox", "class_start", "height", "ref2", "ref4", "sah"):
        assert np.array_equal(raw["%s.%s" % (name, k)], raw["%sr.%s" % (name, k)]), (name, k)


def test_edges(raw):
    for name, leaves in (("n1", 1), ("n2", 1), ("n4", 1), ("n5", 2)):
        t = _tree(raw, name)
        assert (t["kids"][:, 0] < 0).sum() == leaves, name
    assert _tree(raw, "n5")["counts"]["n_nodes"] == 1 and _tree(raw, "n5")["counts"]["n_wnodes"] == 1
    assert len(np.unique(lc.morton_codes(RAW["copies"]()))) == 1
    assert _tree(raw, "copies")["counts"]["depth"] == 1 + 5                      # 65 equal keys split on the position: ceil(log2(65 / 4)) + 1 levels
    codes = lc.morton_codes(RAW["coplanar"]())
    assert not (codes & np.uint64(0x12492492)).any() and len(np.unique(codes)) > 32          # no y bit is set
    codes = lc.morton_codes(RAW["one-bit"]())
    assert sorted(int(x) for x in codes) == [0] + [1 << b for b in range(30)] + [(1 << 30) - 1]
    assert _tree(raw, "one-bit")["counts"]["depth"] >= 28                        # a chain: every code opens a level of its own
    assert _tree(raw, "slivers256")["counts"]["stack_depth"] > deep_walk.LDS_DEPTH


MOVES = ("squash", "shrink", "collapse", "jitter", "translate-out")


@pytest.mark.parametrize("name", MOVES)
def test_refit_after_a_move_keeps_the_topology_and_follows_the_triangles(driver, name):
    sd = vm.sphere_scene()[0]
    out = driver.run(sd, ["lbvh before"] + vm.move_text("move", *vm.SPHERE_MOVES[name](sd)) + ["refit after", "lbvh fresh"], "move-" + name)
    assert out["build.rc"] == 0 and out["move.rc"] == 0
    before, after, fresh = _tree(out, "before"), _tree(out, "after"), _tree(out, "fresh")
    assert not np.array_equal(before["tri"], after["tri"])
    for k in ("kids", "order", "node_child", "wide_child", "slot_prim", "class_start", "height", "ref2", "ref4"):
        assert np.array_equal(out["before." + k], out["after." + k]), k
    assert np.array_equal(_boxes(after, after["tri"]), after["boxes"])
    assert np.array_equal(out["after.bbox"].view(F32), out["fresh.bbox"].view(F32)) and np.array_equal(out["after.grid"], out["fresh.grid"])
    by_prim = lambda label: out[label + ".tris"].reshape(-1, 12)[np.argsort(out[label + ".slot_prim"], kind="stable")]
    assert np.array_equal(by_prim("after"), by_prim("fresh"))
    _check("fresh-" + name, fresh)


def test_the_fit_predicate_on_both_sides_of_its_limit(driver):
    """256 lanes x 8 bytes per entry within 150 KiB: 75 entries fit, 76 do not (bounce_lds_bytes(v) > kFlatLdsCap of fill_scene_view)"""
    out = driver.run(None, ["fit f 2 38 74 75 76 77 200"], "fit")
    assert list(out["f.fit"]) == [1, 1, 1, 1, 0, 0, 0]
    assert 8 * 75 * 256 == 150 * 1024


@pytest.mark.parametrize("name", ["soup65", "sphere", "slivers256", "copies", "one-bit", "n1"])
def test_sah_cost_against_numpy(raw, name):
    t = _tree(raw, name)
    inner = t["kids"][:, 0] >= 0
    area = _area(t["boxes"])
    count = (t["kids"][:, 1].view(np.uint32) >> 27) & 15
    want = (area[inner].sum() + 1.5 * (count[~inner] * area[~inner]).sum()) / area[0] if area[0] > 0 else 0.0
    got = lc.sah(raw, name)
    assert got == pytest.approx(want, rel=1e-12) and (got > 0) == (area[0] > 0)


def test_sah_cost_of_the_binned_sah_tree(driver):
    """the same sum over the tree of creation: what accel_info reports before any rebuild; the LBVH of the same triangles costs more"""
    out = driver.run(vm.sphere_scene()[0], ["sah built", "lbvh lbvh"], "sah")
    assert 0 < lc.sah(out, "built") < lc.sah(out, "lbvh")


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path):
    if not os.path.exists(vm.HIPCC):
        pytest.skip("hipcc not installed")
    san = lc.Driver(tmp_path, flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    commands = []
    for name in sorted(RAW):
        commands += lc.raw_text(name, RAW[name]())
    out = san.run(None, commands + ["fit f 75 76"], "sanitized-raw")
    assert lc.counts(out, "one-bit")["n_slots"] == 32 and list(out["f.fit"]) == [1, 0]
    sd = vm.sphere_scene()[0]
    out = san.run(sd, ["lbvh before", "sah built"] + vm.move_text("move", *vm.SPHERE_MOVES["collapse"](sd)) + ["refit after", "lbvh fresh"], "sanitized-scene")
    assert out["move.rc"] == 0 and lc.counts(out, "fresh")["n_slots"] == lc.counts(out, "before")["n_slots"]


def test_refusals_through_the_abi_need_no_device():
    import ctypes as C
    from mitsuba2_amd import _lib as L
    lib = L.lib()
    out = (C.c_uint32 * 8)()
    assert lib.mtsamd_scene_rebuild_accel(None, 0, None) == -1 and lib.mtsamd_last_error() == b"null scene"
    assert lib.mtsamd_scene_accel_info(None, out, None) == -1 and lib.mtsamd_last_error() == b"null argument"

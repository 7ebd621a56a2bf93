"""Scene.rebuild_accel with both builders beyond one block of the device-wide primitives they lean on: the same byte-for-byte checks as
test_gpu_rebuild.py and test_gpu_rebuild_sah.py, at sizes where rocPRIM takes its multi-block paths.

What the sizes reach (rocPRIM as shipped with the toolchain; rocprim/device/device_radix_sort.hpp, detail/device_config_helper.hpp,
detail/config/device_scan.hpp):

* radix_sort_pairs sorts up to single_sort_items_per_block = 256 * 4 = 1 024 items in one block and merge-sorts up to
  merge_sort_limit = 2^20.  The Morton sort has one item per triangle, the height sort (7 bits, stable, long runs of equal keys: every
  leaf has height 0) one per builder node, nb = 2 * leaves - 1.  With leaves of at most four primitives 4 097 triangles make at least
  1 025 leaves, nb >= 2 049 (test_live_scene_cpu.py asserts nb > 1 024 from the host specification): both sorts merge, over three
  blocks and more.
* exclusive_scan runs one block up to block_size * items_per_thread items and the look-back scan above that.  The configurations these
  calls instantiate: uint32_t (lbvh.hip) 256 * 16 = 4 096 items by the generic default (256 * 21 = 5 376 under the tuned gfx942 table),
  unsigned long long (sah_build.hip) 256 * 8 = 2 048 (256 * 15 = 3 840 tuned); the scan tables hold no entry of their own for gfx950.
  At 32 769 triangles the scans of lbvh.hip have at least 65 538 elements, and the widest level of the SAH build has more nodes than
  either 64-bit figure (asserted on the host in test_live_scene_cpu.py), so every scan leaves its block.
* copies(2049): one run of equal Morton codes across three sort blocks; the sorted order is the identity (a stable sort), the tree splits
  on position alone.

Deliberately left out: the onesweep regime of radix_sort_pairs starts above 2^20 sorted items; the shipped workload (261 k triangles,
523 k builder nodes) never reaches it, and neither do these tests.

Which test covers what, per input (n4097, n32769, copies2049), each on a live scene created from the input, moved (the soups by
vm.jitter(0, 0.05) as the soups of the sibling tests, the copies by one translation of all of them, since a jitter would part their codes)
and then rebuilt:

* test_lbvh_rebuild: every DEVICE_ARRAYS array, the accel_info counts and the SAH cost (bit for bit) equal build_lbvh of the host driver;
* test_sah_rebuild_and_refit: LBVH rebuild first, then rebuild_accel(builder="sah"): every array, counts and cost equal build_sah_levels of
  the driver (at every size, not only 4 097); nodes, qnodes, wnodes, grid and accel_info (but for `rebuilds`) equal a fresh scene's; a
  second jitter refits the new tree to the driver's refit;
* after each rebuild 4 096 rays (_rays of test_gpu_vertex_update.py) through ray_intersect(full=False) and ray_test equal
  ray_intersect_naive of the same scene, and at 4 097 and on the copies the oracle's brute force, bit for bit.  On the copies every hit
  is a tie between 2 049 identical triangles: t, u, v and the shape are compared, the primitive only for being one of them."""
import copy
import functools

import numpy as np
import pytest
import torch

import lbvh_cases as lc
import sah_cases as sc
import vertex_moves as vm
from test_gpu_rebuild_sah import DEVICE_ARRAYS, _assert_arrays, _assert_fresh, _assert_info
from test_gpu_vertex_update import _rays

pytestmark = pytest.mark.gpu
F32 = np.float32

INPUTS = {
    "n4097": (lambda: lc.soup_triangles(4097), vm.jitter(0, 0.05), vm.jitter(0, 0.05, seed=6)),
    "n32769": (lambda: lc.soup_triangles(32769), vm.jitter(0, 0.05), vm.jitter(0, 0.05, seed=6)),
    "copies2049": (lambda: lc.copies(2049), vm.translate(0, (0.25, 0.5, -0.125)), vm.jitter(0, 0.05, seed=6)),
}
ORACLE_QUERIES = ("n4097", "copies2049")          # the oracle's brute force at 32 769 x 4 096 would take the test past a few seconds


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return sc.Driver(tmp_path_factory.mktemp("sizes_gpu"))


@functools.lru_cache(maxsize=None)
def _input(name):
    tri, move, jitter = INPUTS[name]
    old = lc.triangle_scene(tri())
    return old, vm.moved(old, move), vm.moved(old, move, jitter)


_HOST = {}


def _host(driver, name):
    """build_lbvh ("l"), build_sah_levels ("s") of the moved input and refit_bvh of the SAH tree after the second jitter ("r"), once"""
    if name not in _HOST:
        old, moved, _ = _input(name)
        _, move, jitter = INPUTS[name]
        host = driver.run(old, vm.move_text("m1", *move(old)) + ["lbvh l", "sahl s"] + vm.move_text("m2", *jitter(moved)) + ["refit r"], name)
        assert host["build.rc"] == 0 and host["m1.rc"] == 0 and host["m2.rc"] == 0
        _HOST[name] = host
    return _HOST[name]


def _live(gpu, name):
    old, moved, _ = _input(name)
    live = gpu.Scene(copy.deepcopy(old))
    rays = _rays(moved, 4096, 11)
    ray = gpu.Ray3f(*(torch.from_numpy(a).cuda() for a in rays))
    live.ray_intersect(ray, full=False)                               # the walk has run on the old tree
    shape, pos, _ = INPUTS[name][1](old)
    live.update_vertices(shape, torch.from_numpy(pos).cuda())
    return live, moved, rays, ray


def _assert_queries(oracle, live, sd, rays, ray, name, what):
    naive = live.ray_intersect_naive(ray)
    walk = live.ray_intersect(ray, full=False)
    ties = name.startswith("copies")
    for field in ("t", "shape_index", "prim_uv") + (() if ties else ("prim_index",)):
        assert torch.equal(getattr(walk, field), getattr(naive, field)), (what, field)
    hits = torch.isfinite(naive.t)
    share = float(hits.float().mean())
    print("%s %s: %.1f %% of the rays hit" % (name, what, 100.0 * share))
    assert 0.05 <= share <= 0.95, (what, share)
    n_prims = live.info()["primitives"]
    assert bool(((walk.prim_index[hits] >= 0) & (walk.prim_index[hits] < n_prims)).all())
    any_hit = live.ray_test(ray)
    if name in ORACLE_QUERIES:
        S = oracle.OracleScene(copy.deepcopy(sd))
        ref, want_any = S.ray_intersect(*rays, naive=True), S.ray_test(*rays, naive=True)
        t, prim, shape, uv = (x.cpu().numpy() for x in (walk.t, walk.prim_index, walk.shape_index, walk.prim_uv))
        assert (t == ref[0]).all() and (shape.astype(np.uint32) == ref[2]).all() and (uv[:, 0] == ref[3]).all() and (uv[:, 1] == ref[4]).all(), what
        assert ties or (prim.astype(np.uint32) == ref[1]).all(), what
        assert (any_hit.cpu().numpy() == want_any).all(), what
    else:              # any hit = a closest hit exists: the brute force of the same scene decides
        assert torch.equal(any_hit, hits), what


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_lbvh_rebuild(gpu, oracle, driver, name):
    host = _host(driver, name)
    live, moved, rays, ray = _live(gpu, name)
    live.rebuild_accel()
    _assert_arrays(live, host, "l")
    _assert_info(live, host, "l", "lbvh", 1)
    if name.startswith("copies"):
        assert np.array_equal(live.read_accel("slot_prim"), np.arange(2049, dtype=np.uint32))          # the sorted order is the identity
    else:
        assert len(host["l.order"]) > 1024 and len(host["l.slot_prim"]) > 1024                        # both sorts leave the single block
    _assert_queries(oracle, live, moved, rays, ray, name, "after the LBVH rebuild")


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_sah_rebuild_and_refit(gpu, oracle, driver, name):
    host = _host(driver, name)
    live, moved, rays, ray = _live(gpu, name)
    live.rebuild_accel()
    live.rebuild_accel(builder="sah")
    _assert_arrays(live, host, "s")
    _assert_info(live, host, "s", "sah", 2)
    _assert_fresh(gpu, live, moved)
    _assert_queries(oracle, live, moved, rays, ray, name, "after the SAH rebuild")
    shape, pos, _ = INPUTS[name][2](moved)
    live.update_vertices(shape, torch.from_numpy(pos).cuda())          # the second jitter refits the rebuilt topology
    _assert_arrays(live, host, "r")
    _assert_info(live, host, "r", "sah", 2)
    assert not np.array_equal(host["s.boxes"], host["r.boxes"])
    assert set(DEVICE_ARRAYS) >= {"nodes", "qnodes", "wnodes", "tris", "grid", "kids", "order", "boxes", "slot_prim"}

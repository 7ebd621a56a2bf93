"""Scene.rebuild_accel(builder="sah") (mtsamd_scene_rebuild_accel_with): creation's binned-SAH tree built on the device, held to the host
specification build_sah_levels (tests/sah_levels_driver.cpp) and to fresh scenes.

* bytes: after the rebuild every array of read_accel (nodes, qnodes, wnodes, tris, grid; kids, order, node_child, wide_child, boxes,
  slot_prim) equals the driver's, accel_info gives its counts and, bit for bit, its SAH cost, and reports builder "sah"; nodes, qnodes,
  wnodes and grid equal those of a fresh gpu.Scene of the moved description byte for byte; a following update_vertices(jitter) refits the
  new tree to the driver's refit.  On 255 / 256 / 257 / 1025 triangles, the node-size threshold of the kernels (a node of 64 primitives is
  decided by a wave, one of 65 by a workgroup: sah_cases.threshold_set), a skewed set (a large node in a level whose workgroups hold four
  nodes), copies, coplanar, slivers, and the sphere as built and after each of its moves;
* streams and films: samples after move + SAH rebuild equal a fresh scene's and the oracle's in both pipelines, the flag form equals the
  two-call form, a rebuild with nothing moved keeps the film (and the node bytes: it is creation's tree), LBVH -> SAH -> LBVH in a row
  each equal their own specification;
* edges: a flat scene, a root that is a leaf, an unknown builder, MTSAMD_VERTICES_ACCEL_SAH without the rebuild flag, a NaN update with
  "rebuild-sah", autodiff.traverse(accel="rebuild-sah"), and the depth-guard set (45 binary levels)."""
import copy
import ctypes as C

import numpy as np
import parity_util
import pytest
import torch

import deep_walk as dw
import lbvh_cases as lc
import sah_cases as sc
import vertex_moves as vm

pytestmark = pytest.mark.gpu
F32 = np.float32
DEVICE_ARRAYS = ("nodes", "qnodes", "wnodes", "tris", "grid") + lc.TABLE_ARRAYS
FRESH_ARRAYS = ("nodes", "qnodes", "wnodes", "grid")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return sc.Driver(tmp_path_factory.mktemp("sah_gpu"))


def _n(p):
    return p["width"] * p["height"] * p["sample_count"]


def _push(scene, sd, move, **kw):
    shape, pos, _ = move(sd)
    scene.update_vertices(shape, torch.from_numpy(pos).cuda(), **kw)


def _sample(integ, scene, sensor, n):
    rgb, mask, pos = integ.sample(scene, sensor, 0, n)
    return rgb.clone(), mask.clone(), pos.clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _assert_arrays(scene, host, label):
    for k in DEVICE_ARRAYS:
        want = host["%s.%s" % (label, k)]
        got = scene.read_accel(k, len(want))
        assert np.array_equal(got, want), (label, k, int((got != want).sum()), len(want))


def _assert_info(scene, host, label, builder, rebuilds):
    info, c = scene.accel_info(sah_cost=True), lc.counts(host, label)
    assert [info[k] for k in ("bvh_nodes", "wide_nodes", "slots", "depth", "wdepth", "stack_depth")] == \
           [c[k] for k in ("n_nodes", "n_wnodes", "n_slots", "depth", "wdepth", "stack_depth")]
    assert info["builder"] == builder and info["rebuilds"] == rebuilds
    assert np.float64(info["sah_cost"]).tobytes() == host[label + ".sah"].tobytes(), (info["sah_cost"], lc.sah(host, label))
    assert scene.info()["bvh_nodes"] == c["n_nodes"] and scene.info()["bvh_depth"] == c["depth"]


def _assert_fresh(gpu, scene, sd):
    fresh = gpu.Scene(copy.deepcopy(sd))
    for k in FRESH_ARRAYS:
        assert np.array_equal(scene.read_accel(k), fresh.read_accel(k)), k
    a, b = scene.accel_info(), fresh.accel_info()
    assert {k: a[k] for k in a if k != "rebuilds"} == {k: b[k] for k in b if k != "rebuilds"}


_sphere = lambda: vm.sphere_scene()[0]
_tri = lambda f: (lambda: lc.triangle_scene(f()))
ARRAY_CASES = {
    "copies": (_tri(lc.copies), [], vm.jitter(0, 0.05)),
    "coplanar": (_tri(lc.coplanar), [], vm.jitter(0, 0.05)),
    "slivers": (lambda: dw.slivers(256), [], vm.jitter(0, 0.01)),
    "threshold": (_tri(sc.threshold_set), [], vm.jitter(0, 0.05)),
    "skewed": (_tri(sc.skewed), [], vm.jitter(0, 0.005)),
    "sphere": (_sphere, [], vm.SPHERE_MOVES["jitter"]),
}
for _k in (255, 256, 257, 1025):
    ARRAY_CASES["n%d" % _k] = ((lambda k: lambda: lc.triangle_scene(lc.soup_triangles(k)))(_k), [], vm.jitter(0, 0.05))
for _m in sorted(vm.SPHERE_MOVES):
    ARRAY_CASES["sphere-" + _m] = (_sphere, [vm.SPHERE_MOVES[_m]], vm.SPHERE_MOVES["jitter"])


@pytest.mark.parametrize("name", sorted(ARRAY_CASES))
def test_arrays_equal_the_host_specification_and_a_fresh_scene(gpu, driver, name):
    scene_fn, moves, jitter = ARRAY_CASES[name]
    old = scene_fn()
    commands, sd = [], old
    for i, move in enumerate(moves):
        commands += vm.move_text("move%d" % i, *move(sd))
        sd = vm.moved(sd, move)
    commands += ["sahl rebuilt"] + vm.move_text("jitter", *jitter(sd)) + ["refit refitted"]
    host = driver.run(old, commands, name)
    assert host["build.rc"] == 0 and host["jitter.rc"] == 0
    if name == "threshold":
        assert list(host["rebuilt.t_count"][:3]) == [2 * sc.WAVE_NODE + 1, sc.WAVE_NODE, sc.WAVE_NODE + 1]
    if name == "skewed":
        depth, count = host["rebuilt.t_depth"], host["rebuilt.t_count"]
        assert any((depth == d).sum() >= sc.SHARE_LEVEL and count[depth == d].max() > sc.WAVE_NODE for d in np.unique(depth))
    live = gpu.Scene(copy.deepcopy(old))
    sd = old
    for move in moves:
        _push(live, sd, move)
        sd = vm.moved(sd, move)
    live.rebuild_accel(builder="sah")
    _assert_arrays(live, host, "rebuilt")
    _assert_info(live, host, "rebuilt", "sah", 1)
    _assert_fresh(gpu, live, sd)
    _push(live, sd, jitter)                                   # later vertex updates refit the new tree
    _assert_arrays(live, host, "refitted")
    _assert_info(live, host, "refitted", "sah", 1)
    assert not np.array_equal(host["rebuilt.boxes"], host["refitted.boxes"])


def test_lbvh_sah_lbvh_in_a_row_each_equal_their_specification(gpu, driver):
    old = _sphere()
    move = vm.SPHERE_MOVES["squash"]
    host = driver.run(old, vm.move_text("move", *move(old)) + ["lbvh l", "sahl s"], "row")
    live = gpu.Scene(copy.deepcopy(old))
    _push(live, old, move)
    for i, (builder, label) in enumerate((("lbvh", "l"), ("sah", "s"), ("lbvh", "l"), ("sah", "s"), ("sah", "s"))):
        live.rebuild_accel(builder=builder)
        _assert_arrays(live, host, label)
        _assert_info(live, host, label, builder, i + 1)


# ---- streams and films -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["squash", "out-and-shrink"])
def test_streams_after_move_and_sah_rebuild(gpu, oracle, name):
    old, p = vm.sphere_scene()
    moves = {"squash": [vm.SPHERE_MOVES["squash"]], "out-and-shrink": [vm.SPHERE_MOVES["translate-out"], vm.SPHERE_MOVES["shrink"]]}[name]
    new = vm.moved(old, *moves)
    desc = oracle.make_desc(p)
    before, _ = oracle.OracleScene(copy.deepcopy(old)).sample_radiance(desc, 0, _n(p))
    want, wpos = oracle.OracleScene(copy.deepcopy(new)).sample_radiance(desc, 0, _n(p))
    assert float((before != want).any(1).mean()) >= 0.05            # no case passes vacuously
    for pipeline in (1, 2):
        integ, sensor = gpu.PathIntegrator(max_depth=6, pipeline=pipeline), gpu.make_sensor(p)
        two_calls, flag = gpu.Scene(copy.deepcopy(old)), gpu.Scene(copy.deepcopy(old))
        assert integ.render(two_calls, sensor) and integ.render(flag, sensor)          # the device holds the old state
        sd = old
        for move in moves:
            _push(two_calls, sd, move)
            _push(flag, sd, move, accel="rebuild-sah")
            sd = vm.moved(sd, move)
        two_calls.rebuild_accel(builder="sah")
        assert two_calls.accel_info()["rebuilds"] == 1 and flag.accel_info()["rebuilds"] == len(moves)
        assert two_calls.accel_info()["builder"] == flag.accel_info()["builder"] == "sah"
        got = _sample(integ, two_calls, sensor, _n(p))
        rgb, mask, pos = got
        assert np.array_equal(pos.cpu().numpy(), wpos) and np.array_equal(mask.cpu().numpy(), want[:, 3] > 0.5)
        parity_util.check("%s pipeline %d" % (name, pipeline), rgb.cpu().numpy(), want[:, :3])
        assert _same(got, _sample(integ, gpu.Scene(copy.deepcopy(new)), sensor, _n(p))), "not the stream of a fresh scene"
        assert _same(got, _sample(integ, flag, sensor, _n(p))), "the flag form differs from the two-call form"
        for k in DEVICE_ARRAYS:
            assert np.array_equal(two_calls.read_accel(k), flag.read_accel(k)), k


def test_a_sah_rebuild_with_nothing_moved_keeps_the_film_and_the_nodes(gpu):
    old, p = vm.sphere_scene()
    sensor = gpu.make_sensor(p)
    live = gpu.Scene(copy.deepcopy(old), sensor=sensor)
    integ = gpu.PathIntegrator(max_depth=6)
    assert integ.render(live, sensor)
    film = sensor.film().bitmap(raw=True).clone()
    before = {k: live.read_accel(k) for k in FRESH_ARRAYS}
    live.rebuild_accel(builder="sah")
    assert live.accel_info()["builder"] == "sah" and live.accel_info()["rebuilds"] == 1
    for k in FRESH_ARRAYS:                                      # creation's tree again
        assert np.array_equal(live.read_accel(k), before[k]), k
    assert integ.render(live, sensor) and torch.equal(sensor.film().bitmap(raw=True), film)


# ---- edges -----------------------------------------------------------------------------------------------------------------------------------
def test_a_flat_scene_is_left_alone(gpu):
    old, p = vm.cbox_scene()
    live = gpu.Scene(copy.deepcopy(old))
    integ, sensor = gpu.PathIntegrator(max_depth=6, pipeline=1), gpu.make_sensor(p)
    first = _sample(integ, live, sensor, _n(p))
    before = live.read_accel("tris")
    live.rebuild_accel(builder="sah")
    info = live.accel_info(sah_cost=True)
    assert info["builder"] == "sah" and info["rebuilds"] == 0 and info["sah_cost"] == 0.0
    assert np.array_equal(live.read_accel("tris"), before) and _same(first, _sample(integ, live, sensor, _n(p)))
    _push(live, old, vm.CBOX_MOVES["light"], accel="rebuild-sah")
    assert live.accel_info()["rebuilds"] == 0
    assert _same(_sample(integ, live, sensor, _n(p)), _sample(integ, gpu.Scene(vm.moved(old, vm.CBOX_MOVES["light"])), sensor, _n(p)))


def test_a_root_that_is_a_leaf(gpu, driver):
    old, p = vm.leaf_root_scene()
    host = driver.run(old, ["sahl rebuilt"], "leaf-root")
    live = gpu.Scene(copy.deepcopy(old))
    integ, sensor = gpu.PathIntegrator(max_depth=3, pipeline=1), gpu.make_sensor(p)
    first = _sample(integ, live, sensor, _n(p))
    live.rebuild_accel(builder="sah")
    _assert_arrays(live, host, "rebuilt")
    _assert_info(live, host, "rebuilt", "sah", 1)
    assert live.info()["bvh_nodes"] == 0 and live.accel_info()["wide_nodes"] == 0
    assert _same(first, _sample(integ, live, sensor, _n(p)))
    _, move = vm.EDGE_MOVES["leaf-root"]
    _push(live, old, move)
    assert _same(_sample(integ, live, sensor, _n(p)), _sample(integ, gpu.Scene(vm.moved(old, move)), sensor, _n(p)))


def test_refusals_leave_the_scene_as_it_was(gpu):
    from mitsuba2_amd import _lib as L
    old, _ = vm.sphere_scene()
    live = gpu.Scene(copy.deepcopy(old))
    before = {k: live.read_accel(k) for k in ("nodes", "qnodes", "wnodes", "tris", "tri_pos", "grid")}
    for builder in (2, 7, 0xffffffff):
        with pytest.raises(RuntimeError, match="unknown accelerator builder %d" % builder):
            L.check(L.lib().mtsamd_scene_rebuild_accel_with(live._handle, builder, 0, None))
    for builder in (0, 1):
        with pytest.raises(RuntimeError, match="unknown accelerator rebuild flags 0x1"):
            L.check(L.lib().mtsamd_scene_rebuild_accel_with(live._handle, builder, 1, None))
    with pytest.raises(RuntimeError, match="builder"):
        live.rebuild_accel(builder="treelet")
    pos = np.asarray(old["meshes"][vm.SPHERE]["positions"], F32).reshape(-1)
    for flags, text in ((8, "0x8"), (1 | 8, "0x8"), (2 | 4 | 8, "0xe")):          # the SAH bit without the rebuild flag; bit 2 stays unknown
        with pytest.raises(RuntimeError, match="unknown vertex update flags " + text):
            L.check(L.lib().mtsamd_scene_update_vertices(live._handle, vm.SPHERE, pos.ctypes.data_as(C.c_void_p), None, flags, None, None))
    for accel in ("sah", "always"):
        with pytest.raises(RuntimeError, match="accel"):
            live.update_vertices(vm.SPHERE, pos, accel=accel)
    nan = pos.copy(); nan[4] = np.nan
    with pytest.raises(RuntimeError, match="non-finite coordinate"):          # a refused update comes first: no rebuild either
        live.update_vertices(vm.SPHERE, nan, accel="rebuild-sah")
    assert live.accel_info() == dict(live.accel_info(), builder="sah", rebuilds=0)
    for k, a in before.items():
        assert np.array_equal(live.read_accel(k), a), k


def test_product_path(gpu):
    from mitsuba2_amd import autodiff
    old, p = vm.sphere_scene()
    old["meshes"][vm.SPHERE] = dict(old["meshes"][vm.SPHERE], id="ball")
    sensor = gpu.make_sensor(p)
    live = gpu.Scene(copy.deepcopy(old), sensor=sensor)
    integ = gpu.PathIntegrator(max_depth=6)
    with pytest.raises(RuntimeError, match="accel"):
        autodiff.traverse(live, geometry=True, accel="sah")
    params = autodiff.traverse(live, geometry=True, accel="rebuild-sah")
    params.update()                                            # nothing moved: the scene is not touched
    assert live.accel_info()["rebuilds"] == 0
    shape, pos, _ = vm.SPHERE_MOVES["squash"](old)
    params["ball.vertex_positions_buf"] = pos.reshape(-1)
    params.update()
    assert live.accel_info()["rebuilds"] == 1 and live.accel_info()["builder"] == "sah"
    new = vm.moved(old, vm.SPHERE_MOVES["squash"])
    _assert_fresh(gpu, live, new)
    assert integ.render(live, sensor)
    film = sensor.film().bitmap(raw=True).clone()
    sensor2 = gpu.make_sensor(p)
    assert integ.render(gpu.Scene(new), sensor2)
    assert torch.equal(film, sensor2.film().bitmap(raw=True))


def test_the_depth_guard_set(gpu, driver):
    """90 triangles, 45 binary levels: the split in the middle of the order is taken on the device too.  The scene starts as a soup of 90
    triangles and is moved onto the set; the tree either fits the traversal stack, and then its bytes are the specification's, or the
    rebuild is refused as unsupported and every array stays as it was."""
    tri = sc.depth_guard_set()
    old = lc.triangle_scene(lc.soup_triangles(len(tri)))
    move = lambda sd: (0, np.ascontiguousarray(tri.reshape(-1, 3)), None)
    host = driver.run(old, vm.move_text("move", *move(old)) + ["sahl rebuilt"], "guard")
    assert host["move.rc"] == 0 and lc.counts(host, "rebuilt")["depth"] == 45
    deep = (host["rebuilt.t_depth"] >= sc.GUARD_DEPTH) & (host["rebuilt.t_mode"] != sc.LEAF)
    assert deep.any() and (host["rebuilt.t_mode"][deep] == sc.SPLIT_MIDDLE).all()
    live = gpu.Scene(copy.deepcopy(old))
    _push(live, old, move)
    if lc.counts(host, "rebuilt")["stack_depth"] <= 75:          # 8 bytes x 256 lanes x 75 entries = 150 KiB (bvh_stack_fits)
        live.rebuild_accel(builder="sah")
        _assert_arrays(live, host, "rebuilt")
        _assert_info(live, host, "rebuilt", "sah", 1)
    else:
        before = {k: live.read_accel(k) for k in DEVICE_ARRAYS}
        with pytest.raises(RuntimeError, match="too deep"):
            live.rebuild_accel(builder="sah")
        assert live.accel_info()["rebuilds"] == 0
        for k, a in before.items():
            assert np.array_equal(live.read_accel(k), a), k

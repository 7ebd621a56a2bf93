"""Scene.rebuild_accel (mtsamd_scene_rebuild_accel): the LBVH the device builds, held to the host specification and to fresh scenes.

* arrays: after a rebuild every array the walkers read (nodes, qnodes, wnodes, tris, grid) and the refit table (kids, order, node_child,
  wide_child, boxes, slot_prim) equal build_lbvh of tests/lbvh_driver.cpp byte for byte -- the sphere scene as built and after squash /
  translate-out / collapse, soup 65, 65 copies of one triangle, a coplanar soup, slivers; after a following update_vertices(jitter) they
  equal the driver's refit of that topology; accel_info gives the driver's counts and, bit for bit, its SAH cost;
* streams: the hit does not depend on the tree, so sample_radiance after move + rebuild equals the stream of a fresh scene and the
  oracle's, the flag form equals the two-call form, and a rebuild with nothing moved leaves the film of render() as it was;
* queries: ray_intersect / ray_test against the oracle's brute force and ray_intersect_naive, also on slivers scenes whose rebuilt
  stack is deeper than the part kept in LDS (65 triangles in leaves of 4 need three wide levels: 3 * 3 + 2 = 11 > 8 entries);
* edges: a flat scene, a root that is a leaf, unknown flags, a rebuild between other setters, two rebuilds in a row, autodiff.traverse."""
import copy
import ctypes as C

import numpy as np
import parity_util
import pytest
import torch

import deep_walk as dw
import lbvh_cases as lc
import vertex_moves as vm

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return lc.Driver(tmp_path_factory.mktemp("lbvh_gpu"))


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


DEVICE_ARRAYS = ("nodes", "qnodes", "wnodes", "tris", "grid") + lc.TABLE_ARRAYS


def _read(scene, host, label):
    return {k: scene.read_accel(k, len(host["%s.%s" % (label, k)])) for k in DEVICE_ARRAYS}


def _assert_arrays(scene, host, label):
    for k, got in _read(scene, host, label).items():
        want = host["%s.%s" % (label, k)]
        assert np.array_equal(got, want), (label, k, int((got != want).sum()), len(want))


def _assert_info(scene, host, label, rebuilds):
    info, c = scene.accel_info(sah_cost=True), lc.counts(host, label)
    assert [info[k] for k in ("bvh_nodes", "wide_nodes", "slots", "depth", "wdepth", "stack_depth")] == \
           [c[k] for k in ("n_nodes", "n_wnodes", "n_slots", "depth", "wdepth", "stack_depth")]
    assert info["builder"] == "lbvh" and info["rebuilds"] == rebuilds
    assert np.float64(info["sah_cost"]).tobytes() == host[label + ".sah"].tobytes(), (info["sah_cost"], lc.sah(host, label))
    assert scene.info()["bvh_nodes"] == c["n_nodes"] and scene.info()["bvh_depth"] == c["depth"]


_sphere = lambda: vm.sphere_scene()[0]
ARRAY_CASES = {
    "sphere": (_sphere, [], vm.SPHERE_MOVES["jitter"]),
    "sphere-squash": (_sphere, [vm.SPHERE_MOVES["squash"]], vm.SPHERE_MOVES["jitter"]),
    "sphere-translate-out": (_sphere, [vm.SPHERE_MOVES["translate-out"]], vm.SPHERE_MOVES["jitter"]),
    "sphere-collapse": (_sphere, [vm.SPHERE_MOVES["collapse"]], vm.SPHERE_MOVES["jitter"]),
    "soup65": (lambda: vm.soup_scene(65)[0], [], vm.jitter(1, 0.05)),
    "copies": (lambda: lc.triangle_scene(lc.copies()), [], vm.jitter(0, 0.05)),
    "coplanar": (lambda: lc.triangle_scene(lc.coplanar()), [], vm.jitter(0, 0.05)),
    "slivers": (lambda: dw.slivers(256), [], vm.jitter(0, 0.01)),
}


@pytest.mark.parametrize("name", sorted(ARRAY_CASES))
def test_arrays_equal_the_host_specification(gpu, driver, name):
    scene_fn, moves, jitter = ARRAY_CASES[name]
    old = scene_fn()
    commands, sd = ["sah built"], old
    for i, move in enumerate(moves):
        commands += vm.move_text("move%d" % i, *move(sd))
        sd = vm.moved(sd, move)
    commands += ["lbvh rebuilt"] + vm.move_text("jitter", *jitter(sd)) + ["refit refitted"]
    host = driver.run(old, commands, name)
    assert host["build.rc"] == 0 and host["jitter.rc"] == 0
    live = gpu.Scene(copy.deepcopy(old))
    info = live.accel_info(sah_cost=True)
    assert info["builder"] == "sah" and info["rebuilds"] == 0 and np.float64(info["sah_cost"]).tobytes() == host["built.sah"].tobytes()
    sd = old
    for move in moves:
        _push(live, sd, move)
        sd = vm.moved(sd, move)
    live.rebuild_accel()
    _assert_arrays(live, host, "rebuilt")
    _assert_info(live, host, "rebuilt", 1)
    _push(live, sd, jitter)                                   # later vertex updates refit the new topology
    _assert_arrays(live, host, "refitted")
    _assert_info(live, host, "refitted", 1)
    assert not np.array_equal(host["rebuilt.boxes"], host["refitted.boxes"])
    live.rebuild_accel()                                      # ... and a second rebuild starts from the moved triangles
    again = {k: live.read_accel(k) for k in DEVICE_ARRAYS}
    live.rebuild_accel()                                      # two rebuilds in a row: the same bytes, out of the other set of buffers
    for k in DEVICE_ARRAYS:
        assert np.array_equal(live.read_accel(k), again[k]), k
    assert live.accel_info()["rebuilds"] == 3


# ---- streams ---------------------------------------------------------------------------------------------------------------------------------
STREAM_MOVES = {"squash": [vm.SPHERE_MOVES["squash"]], "out-and-shrink": [vm.SPHERE_MOVES["translate-out"], vm.SPHERE_MOVES["shrink"]]}


@pytest.mark.parametrize("name", sorted(STREAM_MOVES))
def test_streams_after_move_and_rebuild(gpu, oracle, name):
    old, p = vm.sphere_scene()
    moves = STREAM_MOVES[name]
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
            _push(flag, sd, move, accel="rebuild")
            sd = vm.moved(sd, move)
        two_calls.rebuild_accel()
        assert two_calls.accel_info()["rebuilds"] == 1 and flag.accel_info()["rebuilds"] == len(moves)
        got = _sample(integ, two_calls, sensor, _n(p))
        rgb, mask, pos = got
        assert np.array_equal(pos.cpu().numpy(), wpos) and np.array_equal(mask.cpu().numpy(), want[:, 3] > 0.5)
        parity_util.check("%s pipeline %d" % (name, pipeline), rgb.cpu().numpy(), want[:, :3])
        assert _same(got, _sample(integ, gpu.Scene(copy.deepcopy(new)), sensor, _n(p))), "not the stream of a fresh scene"
        assert _same(got, _sample(integ, flag, sensor, _n(p))), "the flag form differs from the two-call form"
        for k in ("nodes", "wnodes", "tris", "kids", "boxes"):
            assert np.array_equal(two_calls.read_accel(k), flag.read_accel(k)), k


def test_a_rebuild_with_nothing_moved_keeps_the_film(gpu):
    old, p = vm.sphere_scene()
    sensor = gpu.make_sensor(p)
    live = gpu.Scene(copy.deepcopy(old), sensor=sensor)
    integ = gpu.PathIntegrator(max_depth=6)
    assert integ.render(live, sensor)
    film = sensor.film().bitmap(raw=True).clone()
    nodes = live.read_accel("nodes")
    live.rebuild_accel()
    assert live.accel_info()["builder"] == "lbvh" and not np.array_equal(live.read_accel("nodes")[:len(nodes)], nodes)
    assert integ.render(live, sensor) and torch.equal(sensor.film().bitmap(raw=True), film)


# ---- queries ---------------------------------------------------------------------------------------------------------------------------------
def _gpu_ray(gpu, rays):
    o, d, mint, maxt = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in rays)
    return gpu.Ray3f(o=o, d=d, mint=mint, maxt=maxt)


def _assert_queries(gpu, oracle, live, sd, rays, what):
    S = oracle.OracleScene(copy.deepcopy(sd))
    ref, hit = S.ray_intersect(*rays, naive=True), S.ray_test(*rays, naive=True)
    ray = _gpu_ray(gpu, rays)
    for kind, res in (("walk", live.ray_intersect(ray, full=False)), ("brute force", live.ray_intersect_naive(ray))):
        t, prim, shape, uv = (x.cpu().numpy() for x in (res.t, res.prim_index, res.shape_index, res.prim_uv))
        mism = int((t != ref[0]).sum() + (prim.astype(np.uint32) != ref[1]).sum() + (shape.astype(np.uint32) != ref[2]).sum() +
                   (uv[:, 0] != ref[3]).sum() + (uv[:, 1] != ref[4]).sum())
        assert mism == 0, (what, kind, mism)
    assert int((live.ray_test(ray).cpu().numpy() != hit).sum()) == 0, what
    return ref


def _box_rays(sd, n, seed):
    rng = np.random.RandomState(seed)
    allp = np.concatenate([np.asarray(m["positions"], np.float64).reshape(-1, 3) for m in sd["meshes"][:1] + sd["meshes"][2:]])
    o = rng.uniform(allp.min(0) - 1.0, allp.max(0) + 1.0, (n, 3)).astype(F32)
    d = rng.uniform(allp.min(0), allp.max(0), (n, 3)) - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    maxt = np.where(rng.rand(n) < 0.25, rng.uniform(0.5, 4.0, n), np.inf).astype(F32)
    return o, d, np.zeros(n, F32), maxt


@pytest.mark.parametrize("name", ["translate-out", "squash"])
def test_queries_after_move_and_rebuild(gpu, oracle, name):
    old, _ = vm.sphere_scene()
    new = vm.moved(old, vm.SPHERE_MOVES[name])
    rays = _box_rays(new, 4096, 11)
    live = gpu.Scene(copy.deepcopy(old))
    live.ray_intersect(_gpu_ray(gpu, rays), full=False)                  # the walk has run on the old tree
    _push(live, old, vm.SPHERE_MOVES[name])
    live.rebuild_accel()
    ref = _assert_queries(gpu, oracle, live, new, rays, name)
    assert np.isfinite(ref[0]).mean() > 0.25


@pytest.mark.parametrize("K", [65, 256])
def test_queries_on_slivers_walk_the_spill_path_of_the_new_tree(gpu, oracle, driver, K):
    """K = 65 is the smallest hierarchy scene, and already deeper than the LDS part of the stack: the driver says so on the CPU"""
    sd = lc.triangle_scene(dw.sliver_triangles(K))
    host = driver.run(sd, ["lbvh rebuilt"], "slivers%d" % K)
    assert lc.counts(host, "rebuilt")["stack_depth"] > dw.LDS_DEPTH
    live = gpu.Scene(copy.deepcopy(sd))
    live.rebuild_accel()
    assert live.accel_info()["stack_depth"] == lc.counts(host, "rebuilt")["stack_depth"]
    rays = tuple(np.concatenate([a, b]) for a, b in zip(dw.through_rays(3000, 21), dw.aimed_rays(K, 1000, 22)))
    ref = _assert_queries(gpu, oracle, live, sd, rays, "slivers %d" % K)
    assert np.isfinite(ref[0][3000:]).sum() >= 300


# ---- edges -----------------------------------------------------------------------------------------------------------------------------------
def test_a_flat_scene_is_left_alone(gpu):
    old, p = vm.cbox_scene()
    live = gpu.Scene(copy.deepcopy(old))
    integ, sensor = gpu.PathIntegrator(max_depth=6, pipeline=1), gpu.make_sensor(p)
    first = _sample(integ, live, sensor, _n(p))
    before = live.read_accel("tris")
    live.rebuild_accel()
    info = live.accel_info(sah_cost=True)
    assert info["builder"] == "sah" and info["rebuilds"] == 0 and info["sah_cost"] == 0.0
    assert np.array_equal(live.read_accel("tris"), before) and _same(first, _sample(integ, live, sensor, _n(p)))
    _push(live, old, vm.CBOX_MOVES["light"], accel="rebuild")
    assert _same(_sample(integ, live, sensor, _n(p)), _sample(integ, gpu.Scene(vm.moved(old, vm.CBOX_MOVES["light"])), sensor, _n(p)))


def test_a_root_that_is_a_leaf(gpu, driver):
    old, p = vm.leaf_root_scene()
    host = driver.run(old, ["lbvh rebuilt"], "leaf-root")
    live = gpu.Scene(copy.deepcopy(old))
    integ, sensor = gpu.PathIntegrator(max_depth=3, pipeline=1), gpu.make_sensor(p)
    first = _sample(integ, live, sensor, _n(p))
    live.rebuild_accel()
    _assert_arrays(live, host, "rebuilt")
    _assert_info(live, host, "rebuilt", 1)
    assert live.info()["bvh_nodes"] == 0 and live.accel_info()["wide_nodes"] == 0
    assert _same(first, _sample(integ, live, sensor, _n(p)))
    _, move = vm.EDGE_MOVES["leaf-root"]
    _push(live, old, move)
    assert _same(_sample(integ, live, sensor, _n(p)), _sample(integ, gpu.Scene(vm.moved(old, move)), sensor, _n(p)))


def test_unknown_flags_are_refused_with_nothing_changed(gpu):
    from mitsuba2_amd import _lib as L
    old, _ = vm.sphere_scene()
    live = gpu.Scene(copy.deepcopy(old))
    before = {k: live.read_accel(k) for k in ("nodes", "qnodes", "wnodes", "tris", "tri_pos", "grid")}
    for flags in (1, 2, 0x80000000):
        with pytest.raises(RuntimeError, match="unknown accelerator rebuild flags"):
            L.check(L.lib().mtsamd_scene_rebuild_accel(live._handle, flags, None))
    pos = np.asarray(old["meshes"][vm.SPHERE]["positions"], F32).reshape(-1)
    with pytest.raises(RuntimeError, match="unknown vertex update flags 0x6"):
        L.check(L.lib().mtsamd_scene_update_vertices(live._handle, vm.SPHERE, pos.ctypes.data_as(C.c_void_p), None, 1 | 2 | 4, None, None))          # the refusal names every bit beside the recompute flag, as it always did
    with pytest.raises(RuntimeError, match="accel"):
        live.update_vertices(vm.SPHERE, pos, accel="sah")
    assert live.accel_info() == dict(live.accel_info(), builder="sah", rebuilds=0)
    for k, a in before.items():
        assert np.array_equal(live.read_accel(k), a), k
    nan = pos.copy(); nan[4] = np.nan
    with pytest.raises(RuntimeError, match="non-finite coordinate"):          # a refused update comes first: no rebuild either
        live.update_vertices(vm.SPHERE, nan, accel="rebuild")
    assert live.accel_info()["rebuilds"] == 0
    for k, a in before.items():
        assert np.array_equal(live.read_accel(k), a), k


def test_a_rebuild_between_other_setters_keeps_them(gpu):
    """move, rebuild, update_texture / set_bsdf_param / set_emitter_radiance, rebuild, another move: the fresh scene with all of it"""
    tex = lambda seed: np.random.default_rng(seed).uniform(0.1, 0.9, size=(4, 6, 3)).astype(F32)
    old, p = vm.sphere_scene()
    old["bsdfs"][0] = {"type": "plastic", "diffuse_reflectance": {"type": "bitmap", "data": tex(7)}, "specular_reflectance": [0.25, 0.5, 0.75], "int_ior": 1.9}
    moves = [vm.SPHERE_MOVES["translate-small"], vm.SPHERE_MOVES["jitter"]]
    new = vm.moved(old, *moves)
    new["bsdfs"][0] = dict(old["bsdfs"][0], diffuse_reflectance={"type": "bitmap", "data": tex(8)}, specular_reflectance=[0.625, 0.125, 0.375])
    new["emitters"] = [dict(e) for e in old["emitters"]]
    new["emitters"][0]["radiance"] = np.array([3.0, 7.0, 5.0], F32)
    for pipeline in (1, 2):
        integ, sensor = gpu.PathIntegrator(max_depth=6, pipeline=pipeline), gpu.make_sensor(p)
        live = gpu.Scene(copy.deepcopy(old))
        assert integ.render(live, sensor)
        _push(live, old, moves[0])
        live.update_texture(live.texture_index(0), tex(8))
        live.rebuild_accel()
        live.set_bsdf_param(0, 1, [0.625, 0.125, 0.375])
        live.set_emitter_radiance(0, [3.0, 7.0, 5.0])
        live.rebuild_accel()
        _push(live, vm.moved(old, moves[0]), moves[1])
        assert _same(_sample(integ, live, sensor, _n(p)), _sample(integ, gpu.Scene(copy.deepcopy(new)), sensor, _n(p))), pipeline


def test_product_path(gpu):
    from mitsuba2_amd import autodiff
    old, p = vm.sphere_scene()
    old["meshes"][vm.SPHERE] = dict(old["meshes"][vm.SPHERE], id="ball")
    sensor = gpu.make_sensor(p)
    live = gpu.Scene(copy.deepcopy(old), sensor=sensor)
    integ = gpu.PathIntegrator(max_depth=6)
    with pytest.raises(RuntimeError, match="accel"):
        autodiff.traverse(live, geometry=True, accel="always")
    params = autodiff.traverse(live, geometry=True, accel="rebuild")
    params.update()                                            # nothing moved: the scene is not touched
    assert live.accel_info()["rebuilds"] == 0
    shape, pos, _ = vm.SPHERE_MOVES["squash"](old)
    params["ball.vertex_positions_buf"] = pos.reshape(-1)
    params.update()
    assert live.accel_info()["rebuilds"] == 1 and live.accel_info()["builder"] == "lbvh"
    assert integ.render(live, sensor)
    film = sensor.film().bitmap(raw=True).clone()
    sensor2 = gpu.make_sensor(p)
    assert integ.render(gpu.Scene(vm.moved(old, vm.SPHERE_MOVES["squash"])), sensor2)
    assert torch.equal(film, sensor2.film().bitmap(raw=True))

"""mtsamd_scene_update_vertices with MTSAMD_VERTICES_RECOMPUTE_NORMALS (Scene.update_vertices(..., normals="recompute")): the device's
vertex normals against the host specification mtsamd_compute_vertex_normals (vertex_normals_util.spec), bit for bit, and the scene
after such an update against fresh scenes and the oracle.  Scenes and moves are those of vertex_moves.py; only the positions of a move
are used, the normals are the call's own.

* arrays: every SPHERE_MOVES entry that moves the mesh with normals, the same mesh behind another (first_prim != 0), and the edge
  meshes of vertex_normals_util.py inside a hierarchy scene: normals_out and tri_nrm equal the specification and its gather;
* film and streams, hierarchy and flat: the film after the device update equals the film of a fresh scene created from the moved
  positions and the specification's normals, and the film after handing those normals to the old entry point; per-sample radiance equals
  the oracle's on the same arrays;
* the refusals, exact code and text, change nothing;
* the Python path: device clones kept as pending, Scene._dict flushes them; autodiff.traverse(..., normals="recompute")."""
import copy
import ctypes as C

import numpy as np
import parity_util
import pytest
import torch

import vertex_moves as vm
import vertex_normals_util as vn

pytestmark = pytest.mark.gpu

F32 = np.float32
RECOMPUTE = 1          # MTSAMD_VERTICES_RECOMPUTE_NORMALS
INVALID = -1           # MTSAMD_ERR_INVALID
WITH_NORMALS = [k for k in vm.SPHERE_MOVES if k not in ("floor", "light")]          # the moves of the sphere, the mesh with normals


def _arrays(m):
    return np.asarray(m["positions"], F32).reshape(-1, 3), np.asarray(m["faces"], np.uint32).reshape(-1, 3)


def _first_prim(sd, shape):
    return sum(len(_arrays(m)[1]) for m in sd["meshes"][:shape])


def _tri_nrm(scene, sd, shape):
    """the shape's part of the device's tri_nrm: (faces, 3, 3)"""
    n_faces = len(_arrays(sd["meshes"][shape])[1])
    first = _first_prim(sd, shape)
    return scene.read_accel("tri_nrm")[9 * first:9 * (first + n_faces)].view(F32).reshape(-1, 3, 3)


def _with_spec_normals(sd, shape, pos):
    """the description with `pos` and the specification's normals in mesh `shape`"""
    new = dict(sd, meshes=[dict(m) for m in sd["meshes"]])
    faces = _arrays(sd["meshes"][shape])[1]
    new["meshes"][shape] = dict(new["meshes"][shape], positions=np.ascontiguousarray(pos, F32).reshape(-1, 3), normals=vn.spec(pos, faces))
    return new


def _check_arrays(live, sd, shape, pos, got):
    faces = _arrays(sd["meshes"][shape])[1]
    want = vn.spec(pos, faces)
    assert got.is_cuda and got.shape == want.shape
    assert np.array_equal(vn.bits(got.cpu().numpy()), vn.bits(want))
    assert np.array_equal(vn.bits(_tri_nrm(live, sd, shape)), vn.bits(want[faces.astype(np.int64)]))
    first = _first_prim(sd, shape)
    tri_pos = live.read_accel("tri_pos")[9 * first:9 * (first + len(faces))]
    assert np.array_equal(tri_pos, vn.bits(np.ascontiguousarray(pos, F32).reshape(-1, 3)[faces.astype(np.int64)]))
    return want


# ---- arrays --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WITH_NORMALS)
def test_device_normals_equal_the_host_specification(gpu, name):
    sd = vm.sphere_scene()[0]
    shape, pos, _ = vm.SPHERE_MOVES[name](sd)
    assert shape == vm.SPHERE
    live = gpu.Scene(copy.deepcopy(sd))
    before = _tri_nrm(live, sd, shape).copy()
    got = live.update_vertices(shape, torch.from_numpy(pos).cuda(), normals="recompute")
    want = _check_arrays(live, sd, shape, pos, got)
    if name not in ("translate-out", "translate-small"):          # a translation keeps the normals (to rounding)
        assert not np.array_equal(vn.bits(before), vn.bits(want[_arrays(sd["meshes"][shape])[1].astype(np.int64)]))
    # a second update of the same shape goes through the table the first one built
    back = _arrays(sd["meshes"][shape])[0]
    _check_arrays(live, sd, shape, back, live.update_vertices(shape, torch.from_numpy(back).cuda(), normals="recompute"))


def test_a_shape_behind_another(gpu):
    """first_prim != 0: the faces are the shape's own, the corner table counts faces from the shape's first; host pointers for positions
    and normals_out through the C ABI"""
    from mitsuba2_amd import _lib as L
    base = vm.sphere_scene()[0]
    sd = dict(base, meshes=[base["meshes"][vm.FLOOR], base["meshes"][vm.LIGHT], base["meshes"][vm.SPHERE]])
    shape = 2
    assert _first_prim(sd, shape) > 0
    _, pos, _ = vm.jitter(shape, 0.05)(sd)
    live = gpu.Scene(copy.deepcopy(sd))
    others = [_arrays(m) for m in sd["meshes"][:shape]]
    got = live.update_vertices(shape, torch.from_numpy(pos).cuda(), normals="recompute")
    want = _check_arrays(live, sd, shape, pos, got)
    _, pos2, _ = vm.scale_about(shape, 0.5, vm.SPHERE_CENTRE)(sd)
    out = np.full(pos2.shape, np.nan, F32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L.check(L.lib().mtsamd_scene_update_vertices(live._handle, shape, p(pos2), None, RECOMPUTE, p(out), None))
    faces = _arrays(sd["meshes"][shape])[1]
    assert np.array_equal(vn.bits(out), vn.bits(vn.spec(pos2, faces))) and not np.array_equal(vn.bits(out), vn.bits(want))
    assert np.array_equal(vn.bits(_tri_nrm(live, sd, shape)), vn.bits(out[faces.astype(np.int64)]))
    L.check(L.lib().mtsamd_scene_update_vertices(live._handle, shape, p(pos), None, RECOMPUTE, None, None))          # normals_out may be null
    assert np.array_equal(vn.bits(_tri_nrm(live, sd, shape)), vn.bits(want[faces.astype(np.int64)]))
    tri_pos = live.read_accel("tri_pos").view(F32).reshape(-1, 3, 3)
    first = 0
    for opos, ofaces in others:                                         # the shapes in front are where they were
        assert np.array_equal(tri_pos[first:first + len(ofaces)], opos[ofaces.astype(np.int64)])
        first += len(ofaces)


def _edge_scene():
    """the sphere scene with the edge meshes behind it: the fan with its 300-face apex, the isolated vertex and the cancelling faces in
    one mesh, the 257-vertex strip in another; 557 triangles more, a hierarchy scene"""
    sd = vm.sphere_scene()[0]
    meshes = list(sd["meshes"])
    for (pos, faces), offset in ((vn.edge_mesh(), (-2.0, 0.25, -1.0)), (vn.strip257(), (1.0, 0.5, -1.5))):
        pos = (pos + np.asarray(offset, F32)).astype(F32)
        meshes.append(dict(positions=pos, faces=faces, normals=vn.spec(pos, faces), bsdf=sd["meshes"][vm.FLOOR]["bsdf"], emitter=-1))
    return dict(sd, meshes=meshes)


def test_edge_meshes_in_a_hierarchy_scene(gpu):
    sd = _edge_scene()
    live = gpu.Scene(copy.deepcopy(sd))
    assert live.info()["primitives"] >= 65 and live.info()["bvh_nodes"] > 0
    edge, strip = len(sd["meshes"]) - 2, len(sd["meshes"]) - 1
    for shape in (edge, strip):
        pos = (_arrays(sd["meshes"][shape])[0] + np.array([0.25, 0.5, 0.0], F32)).astype(F32)          # binary fractions: what cancels still cancels
        want = _check_arrays(live, sd, shape, pos, live.update_vertices(shape, torch.from_numpy(pos).cuda(), normals="recompute"))
        assert np.isfinite(want).all()
        if shape == edge:
            bogus = (vn.bits(want).reshape(-1, 3) == vn.bits([1.0, 0.0, 0.0])).all(1)
            assert bogus[vn.EDGE_ISOLATED] and bogus[vn.EDGE_CANCELLING].all() and not bogus[:vn.FAN_FACES + 1].any()
            assert want[vn.EDGE_APEX][1] > 0.9


# ---- film and streams ----------------------------------------------------------------------------------------------------------------------
def _n(p):
    return p["width"] * p["height"] * p["sample_count"]


def _film(gpu, integ, scene, p):
    sensor = gpu.make_sensor(p)
    assert integ.render(scene, sensor)
    return sensor.film().bitmap(raw=True).clone()


def _flat_scene():
    """vm.soup_scene(64), the largest LDS-resident soup, with vertex normals added to every mesh"""
    sd, p = vm.soup_scene(64)
    return dict(sd, meshes=[dict(m, normals=vn.spec(*_arrays(m))) for m in sd["meshes"]]), p


FILM_CASES = {
    "hierarchy": (vm.sphere_scene, vm.SPHERE_MOVES["jitter"], (1, 2)),
    "flat": (_flat_scene, vm.EDGE_MOVES["soup64"][1], (1, 4)),
}


@pytest.mark.parametrize("name", sorted(FILM_CASES))
def test_film_and_streams(gpu, oracle, name):
    scene_fn, move, pipelines = FILM_CASES[name]
    old, p = scene_fn()
    shape, pos, _ = move(old)
    new = _with_spec_normals(old, shape, pos)
    desc = oracle.make_desc(p)
    before, _ = oracle.OracleScene(copy.deepcopy(old)).sample_radiance(desc, 0, _n(p))
    want, wpos = oracle.OracleScene(copy.deepcopy(new)).sample_radiance(desc, 0, _n(p))
    assert float((before != want).any(1).mean()) >= 0.05                                  # the move shows
    for pipeline in pipelines:
        integ = gpu.PathIntegrator(max_depth=6, pipeline=pipeline)
        live = gpu.Scene(copy.deepcopy(old))
        old_film = _film(gpu, integ, live, p)                                            # the device holds the old state
        got_normals = live.update_vertices(shape, torch.from_numpy(pos).cuda(), normals="recompute")
        assert np.array_equal(vn.bits(got_normals.cpu().numpy()), vn.bits(new["meshes"][shape]["normals"]))
        film = _film(gpu, integ, live, p)
        assert not torch.equal(film, old_film)
        assert torch.equal(film, _film(gpu, integ, gpu.Scene(copy.deepcopy(new)), p)), "a fresh scene of the moved positions and the specification's normals"
        through_old = gpu.Scene(copy.deepcopy(old))
        through_old.update_vertices(shape, pos, normals=new["meshes"][shape]["normals"])
        assert torch.equal(film, _film(gpu, integ, through_old, p)), "the same normals through the old entry point"
        rgb, mask, spos = integ.sample(live, gpu.make_sensor(p), 0, _n(p))
        assert np.array_equal(spos.cpu().numpy(), wpos) and np.array_equal(mask.cpu().numpy(), want[:, 3] > 0.5)
        parity_util.check("%s pipeline %d" % (name, pipeline), rgb.cpu().numpy(), want[:, :3])
    # pipeline 4 runs LDS-resident scenes only: that it ran is what shows the flat case to be flat
    if name == "hierarchy":
        with pytest.raises(RuntimeError, match="LDS-resident scenes only"):
            gpu.PathIntegrator(max_depth=6, pipeline=4).sample(live, gpu.make_sensor(p), 0, 64)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hierarchy", "flat"])
def test_refusals_change_nothing(gpu, kind):
    from mitsuba2_amd import _lib as L
    if kind == "hierarchy":
        old, body, bare = vm.sphere_scene()[0], vm.SPHERE, vm.FLOOR
    else:
        old = _flat_scene()[0]
        old = dict(old, meshes=[dict(m, normals=None) if i == 2 else m for i, m in enumerate(old["meshes"])])
        body, bare = 1, 2
    live = gpu.Scene(copy.deepcopy(old))
    lib = L.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    pos, bare_pos = _arrays(old["meshes"][body])[0].copy(), _arrays(old["meshes"][bare])[0].copy()
    out = np.full(pos.shape, 7.0, F32)
    nan = pos.copy(); nan[1, 1] = np.nan
    state = lambda: (live.read_accel("tri_nrm").copy(), live.read_accel("tri_pos").copy(), live.read_accel("grid").copy())
    first = state()
    refusals = [
        ((bare, p(bare_pos), None, RECOMPUTE), "shape %d was created without vertex normals: storing new normals in such a mesh is not implemented" % bare),
        ((body, p(pos), p(pos), RECOMPUTE), "shape %d: MTSAMD_VERTICES_RECOMPUTE_NORMALS computes the normals: none can be passed with it" % body),
        ((body, p(pos), None, 6), "unknown vertex update flags 0x6"),
        ((body, p(pos), None, RECOMPUTE | 0x80000000), "unknown vertex update flags 0x80000000"),
        ((len(old["meshes"]), p(pos), None, RECOMPUTE), "invalid shape index %d (the scene has %d shapes)" % (len(old["meshes"]), len(old["meshes"]))),
        ((body, None, None, RECOMPUTE), "shape %d: null vertex positions" % body),
        ((body, p(pos), None, 0), "shape %d was created with vertex normals: new normals are required with new positions" % body),
    ]
    for (shape, positions, normals, flags), text in refusals:
        assert lib.mtsamd_scene_update_vertices(live._handle, shape, positions, normals, flags, p(out), None) == INVALID, text
        assert lib.mtsamd_last_error().decode() == text
        assert all(np.array_equal(a, b) for a, b in zip(first, state())) and (out == 7.0).all(), text
    # a non-finite coordinate with the flag set: refused by the look-before-write stage, tri_nrm as it was
    assert lib.mtsamd_scene_update_vertices(live._handle, body, p(nan), None, RECOMPUTE, None, None) == INVALID
    assert "non-finite coordinate" in lib.mtsamd_last_error().decode()
    with pytest.raises(RuntimeError, match="non-finite coordinate"):
        live.update_vertices(body, torch.from_numpy(nan).cuda(), normals="recompute")
    assert all(np.array_equal(a, b) for a, b in zip(first, state()))
    with pytest.raises(RuntimeError, match="without vertex normals: storing new normals"):
        live.update_vertices(bare, bare_pos, normals="recompute")
    with pytest.raises(RuntimeError, match="expected 3 \\*"):
        live.update_vertices(body, pos[:-1], normals="recompute")
    with pytest.raises(RuntimeError, match="\"recompute\""):
        live.update_vertices(body, pos, normals="again")
    assert all(np.array_equal(a, b) for a, b in zip(first, state()))
    for a, b in zip(live._dict["meshes"], old["meshes"]):                 # nothing was left pending by a refused call
        assert np.array_equal(_arrays(a)[0], _arrays(b)[0])
    # flags == 0 is the old call
    normals = vn.spec(pos * F32(0.5), _arrays(old["meshes"][body])[1])
    half = (pos * F32(0.5)).astype(F32)
    L.check(lib.mtsamd_scene_update_vertices(live._handle, body, p(half), p(normals), 0, p(out), None))
    assert (out == 7.0).all() and not np.array_equal(first[1], live.read_accel("tri_pos"))
    other = gpu.Scene(copy.deepcopy(old))
    L.check(lib.mtsamd_scene_set_vertex_positions(other._handle, body, p(half), p(normals), None))
    assert all(np.array_equal(live.read_accel(k), other.read_accel(k)) for k in ("tri_pos", "tri_nrm", "tris", "grid"))
    # and after all the refusals the flag still works, here with host pointers on both sides
    L.check(lib.mtsamd_scene_update_vertices(live._handle, body, p(pos), None, RECOMPUTE, p(out), None))
    assert np.array_equal(vn.bits(out), vn.bits(vn.spec(pos, _arrays(old["meshes"][body])[1])))
    assert np.array_equal(live.read_accel("tri_pos"), first[1])


# ---- the Python path -------------------------------------------------------------------------------------------------------------------------
def test_python_path_keeps_device_clones_and_flushes_them(gpu):
    from mitsuba2_amd import autodiff
    old, p = vm.sphere_scene()
    old["meshes"][vm.SPHERE] = dict(old["meshes"][vm.SPHERE], id="ball")
    shape, pos, _ = vm.SPHERE_MOVES["jitter"](old)
    new = _with_spec_normals(old, shape, pos)
    integ = gpu.PathIntegrator(max_depth=6)
    want_film = _film(gpu, integ, gpu.Scene(copy.deepcopy(new)), p)

    live = gpu.Scene(copy.deepcopy(old))
    mine = torch.from_numpy(pos).cuda()
    got = live.update_vertices(shape, mine, normals="recompute")
    assert got.is_cuda and got.shape == (len(pos), 3) and list(live._pending_vertices) == [shape]
    mine.fill_(123.0)                                                          # the caller's tensor is theirs again
    got.fill_(-1.0)                                                            # and so is the returned one
    mesh = live._dict["meshes"][shape]
    assert not live._pending_vertices
    assert np.array_equal(vn.bits(mesh["positions"]), vn.bits(pos)) and np.array_equal(vn.bits(mesh["normals"]), vn.bits(new["meshes"][shape]["normals"]))
    assert mesh["positions"].shape == (len(pos), 3) and mesh["normals"].shape == (len(pos), 3)
    assert torch.equal(_film(gpu, integ, live, p), want_film)
    # a host array takes the same path; an update through the old path afterwards sees the flushed description
    live.update_vertices(shape, _arrays(old["meshes"][shape])[0], normals="recompute")
    live.update_vertices(shape, pos)
    assert np.array_equal(vn.bits(live._dict["meshes"][shape]["positions"]), vn.bits(pos))

    sensor = gpu.make_sensor(p)
    live2 = gpu.Scene(copy.deepcopy(old), sensor=sensor)
    params = autodiff.traverse(live2, geometry=True, normals="recompute")
    floor_key = "shape_%d.vertex_positions_buf" % vm.FLOOR
    params[floor_key] = params[floor_key] * 1.0                               # a mesh without normals still moves through the old path
    params.update()
    assert not live2._pending_vertices
    params["ball.vertex_positions_buf"] = pos.reshape(-1)
    params.update()
    assert list(live2._pending_vertices) == [shape]
    assert torch.equal(_film(gpu, integ, live2, p), want_film)
    assert np.array_equal(vn.bits(live2._dict["meshes"][shape]["normals"]), vn.bits(new["meshes"][shape]["normals"]))
    with pytest.raises(RuntimeError, match="recompute"):
        autodiff.traverse(live2, geometry=True, normals="smooth")

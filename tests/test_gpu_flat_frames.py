"""Flat scenes (at most 64 triangles) keep the part of a hit's frame that the triangle alone decides -- the geometric normal n and, for a
shape without vertex normals, s of the shading frame -- in their LDS shading records: k_flat_frames computes both once at scene
creation with the device functions fill_si would call per hit, so nothing a kernel returns may move by a bit.  Everything here is
compared by equality: the SurfaceInteraction planes with OracleScene.ray_intersect(naive=True) / fill_si, the per-sample radiance of
every schedule (pipelines 0-4: automatic, fused, split, k_mega, k_shade with the in-kernel shadow ring), RGB and spectral, with the
oracle's wavefront stream, and a live scene after a setter with a freshly created one.

Scenes, all edits of scenes.cornell_box() (36 triangles: five room quads, the light, two boxes):
  a  cornell_box(texture=...): the room quads carry UVs (dp_du is the parameterisation's), light and boxes are plain
  b  both boxes with vertex normals that differ from the face normal: normalize(face normal + 0.2 (vertex - centre) / radius)
  c  all four shape classes at once: UV (room), plain (light), normals (short box), UV + normals (tall box)
  d  the light quad with vertex normals: sample_emitter_direction interpolates them instead of reading the record's n
  e  two emitters, one plain and one with UVs (the glowing top of the short box)
  f  one triangle and the light
  g  64 triangles, the last flat scene, and 65, the first that takes the hierarchy path (unchanged): c plus a strip of plain triangles

Rays: origins uniform in the scene's box and normal directions as in test_gpu_parity._rays; three rays of four are then turned towards
a point of a primitive drawn uniformly, so that a shape of two triangles gets its share.  No case passes vacuously: at least half the
rays hit, and every shape class of the scene receives at least 100 hits (counted on the oracle alone)."""
import copy

import numpy as np
import pytest
import torch

from mitsuba2_amd import scenes

pytestmark = pytest.mark.gpu

TEX_A = np.random.default_rng(7).uniform(0.1, 0.9, size=(4, 6, 3)).astype(np.float32)
TEX_B = np.random.default_rng(8).uniform(0.1, 0.9, size=(4, 6, 3)).astype(np.float32)
QUAD_UV = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
LIGHT, SHORT, TALL = 5, 6, 7          # meshes of scenes.cornell_box() behind the five room quads
PLAIN, UV, NORMALS, UV_NORMALS = "plain", "uv", "normals", "uv+normals"


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def _bent_normals(mesh):
    """per vertex: normalize(face normal + 0.2 (vertex - centre) / radius); every vertex of these meshes belongs to coplanar faces"""
    pos = np.asarray(mesh["positions"], np.float64)
    out = np.zeros_like(pos)
    for f in np.asarray(mesh["faces"]):
        n = np.cross(pos[f[1]] - pos[f[0]], pos[f[2]] - pos[f[0]])
        out[f] = n / np.linalg.norm(n)
    off = pos - pos.mean(0)
    out += 0.2 * off / np.linalg.norm(off, axis=1).max()
    return np.ascontiguousarray(out / np.linalg.norm(out, axis=1, keepdims=True), dtype=np.float32)


def _with(sd, index, normals=False, uv=False):
    m = dict(sd["meshes"][index])
    if normals:
        m["normals"] = _bent_normals(m)
    if uv:
        m["texcoords"] = np.tile(QUAD_UV, (len(m["positions"]) // 4, 1))
    sd["meshes"][index] = m
    return sd


def _strip(n_tris, y=40.0):
    """n_tris plain triangles above the floor"""
    pos, faces = [], []
    for k in range(n_tris):
        x, z = 60.0 + 15.0 * (k % 8), 300.0 + 30.0 * (k // 8)
        pos += [[x, y, z], [x, y, z + 25.0], [x + 12.0, y + 3.0, z]]
        faces.append([3 * k, 3 * k + 1, 3 * k + 2])
    return dict(positions=np.array(pos, np.float32), faces=np.array(faces, np.uint32), normals=None, texcoords=None, bsdf=1, emitter=-1)


def scene(name):
    if name == "a":
        return scenes.cornell_box(texture=TEX_A)
    if name == "b":
        return _with(_with(scenes.cornell_box(), SHORT, normals=True), TALL, normals=True)
    if name == "c":
        return _with(_with(scenes.cornell_box(texture=TEX_A), SHORT, normals=True), TALL, normals=True, uv=True)
    if name == "d":
        return _with(scenes.cornell_box(), LIGHT, normals=True)
    if name == "e":
        sd = scenes.cornell_box()
        sd["emitters"].append(dict(type="area", radiance=np.array([2.0, 4.0, 8.0], np.float32)))
        quad = np.array([[130, 165.5, 65], [82, 165.5, 225], [240, 165.5, 272], [290, 165.5, 114]], np.float32)
        sd["meshes"].append(dict(positions=quad, faces=np.array([[0, 1, 2], [0, 2, 3]], np.uint32), normals=None, texcoords=QUAD_UV.copy(), bsdf=0, emitter=1))
        return sd
    if name == "f":
        sd = scenes.cornell_box()
        tri = dict(positions=np.array([[100, 20, 150], [150, 60, 420], [450, 30, 250]], np.float32), faces=np.array([[0, 1, 2]], np.uint32),
                   normals=None, texcoords=None, bsdf=1, emitter=-1)
        return dict(sd, meshes=[sd["meshes"][LIGHT], tri])
    if name in ("g64", "g65"):
        sd = scene("c")
        sd["meshes"].append(_strip(int(name[1:]) - 36))
        return sd
    raise KeyError(name)


SCENES = ("a", "b", "c", "d", "e", "f", "g64", "g65")
CLASSES = {"a": {PLAIN, UV}, "b": {PLAIN, NORMALS}, "c": {PLAIN, UV, NORMALS, UV_NORMALS}, "d": {PLAIN, NORMALS}, "e": {PLAIN, UV}, "f": {PLAIN},
           "g64": {PLAIN, UV, NORMALS, UV_NORMALS}, "g65": {PLAIN, UV, NORMALS, UV_NORMALS}}


def _class_of(mesh):
    return {(False, False): PLAIN, (True, False): UV, (False, True): NORMALS, (True, True): UV_NORMALS}[
        (mesh.get("texcoords") is not None, mesh.get("normals") is not None)]


def rays(sd, n, seed):
    rng = np.random.RandomState(seed)
    allp = np.concatenate([m["positions"] for m in sd["meshes"]])
    lo, hi = allp.min(0), allp.max(0)
    o = (lo + (hi - lo) * rng.rand(n, 3)).astype(np.float32)
    d = rng.randn(n, 3)
    tris = np.concatenate([np.asarray(m["positions"], np.float64)[np.asarray(m["faces"])] for m in sd["meshes"]])
    b = rng.dirichlet([1.0, 1.0, 1.0], n)
    target = np.einsum("nk,nkc->nc", b, tris[rng.randint(len(tris), size=n)])
    aimed = np.arange(n) % 4 != 0
    d[aimed] = (target - o)[aimed]
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return o, d, np.full(n, 1e-4, np.float32), np.full(n, np.inf, np.float32)


def _gpu_ray(gpu, o, d, mint, maxt):
    t = lambda a: torch.from_numpy(a).cuda()
    return gpu.Ray3f(o=t(o), d=t(d), mint=t(mint), maxt=t(maxt))


def _si_planes(si):
    return torch.cat([si.t[:, None], si.p, si.n, si.uv, si.sh_frame_s, si.sh_frame_t, si.sh_frame_n, si.dp_du, si.dp_dv, si.wi], dim=1)


# ---- SurfaceInteraction fields -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_si_fields(gpu, oracle, name):
    sd = scene(name)
    n = 4096
    o, d, mint, maxt = rays(sd, n, 5)
    S = oracle.OracleScene(sd)
    t_o, prim_o, shape_o, u_o, v_o = S.ray_intersect(o, d, mint, maxt, naive=True)
    valid = np.isfinite(t_o)
    classes = np.array([_class_of(m) for m in sd["meshes"]])
    hits = {c: int((classes[shape_o[valid]] == c).sum()) for c in (PLAIN, UV, NORMALS, UV_NORMALS)}
    print("scene %s: %d of %d rays hit, per shape class %s" % (name, valid.sum(), n, hits))
    assert valid.sum() >= n // 2
    assert {c for c, k in hits.items() if k} == CLASSES[name] and all(hits[c] >= 100 for c in CLASSES[name]), hits
    g = gpu.Scene(sd)
    info = g.info()
    assert info["primitives"] == sum(len(m["faces"]) for m in sd["meshes"]) == {"f": 3, "e": 38, "g64": 64, "g65": 65}.get(name, 36)
    assert name != "g65" or info["bvh_nodes"] > 0              # 65 triangles: the hierarchy path
    si = g.ray_intersect(_gpu_ray(gpu, o, d, mint, maxt))
    assert (si.t.cpu().numpy() == t_o).all()
    ref = S.fill_si(d, prim_o, u_o, v_o)
    got = _si_planes(si).cpu().numpy()[:, 1:]
    bad = np.nonzero((got != ref).any(1) & valid)[0]
    assert bad.size == 0, (name, bad.size, [(int(i), int(shape_o[i]), np.nonzero(got[i] != ref[i])[0].tolist()) for i in bad[:8]])
    assert (si.wi.cpu().numpy()[~valid] == -d[~valid]).all()


# ---- per-sample radiance -----------------------------------------------------------------------------------------------------------------
_STREAMS = {}


def _oracle_stream(gpu, oracle, name, variant, max_depth):
    key = (name, variant, max_depth)
    if key not in _STREAMS:
        p = scenes.cornell_box_sensor(32, 32, 16, seed=3, max_depth=max_depth)
        S = oracle.OracleScene(scene(name), naive=True, spectral_path=gpu.srgb_coeff_path() if variant == "spectral" else None)
        rgba, pos = S.sample_radiance(oracle.make_desc(p), 0, 32 * 32 * 16)
        rgba.setflags(write=False); pos.setflags(write=False)
        _STREAMS[key] = (p, rgba, pos)
    return _STREAMS[key]


@pytest.mark.parametrize("max_depth", [-1, 3])
@pytest.mark.parametrize("variant", ["rgb", "spectral"])
@pytest.mark.parametrize("name", ["a", "b", "d", "e"])
def test_per_sample_radiance(gpu, oracle, name, variant, max_depth):
    p, ref, ref_pos = _oracle_stream(gpu, oracle, name, variant, max_depth)
    n = 32 * 32 * 16
    assert (ref[:, :3] > 0).any(1).mean() > 0.5                   # most samples carry light
    g, sensor = gpu.Scene(scene(name), variant=variant), gpu.make_sensor(p)
    for pipeline in (0, 1, 2, 3, 4):
        rgb, mask, pos = gpu.PathIntegrator(max_depth=max_depth, rr_depth=5, pipeline=pipeline).sample(g, sensor, 0, n)
        rgb = rgb.cpu().numpy()
        exact = (rgb == ref[:, :3]).all(1)
        assert exact.all(), (pipeline, int((~exact).sum()), np.nonzero(~exact)[0][:8], rgb[~exact][:4], ref[~exact][:4, :3])
        assert (pos.cpu().numpy() == ref_pos).all() and (mask.cpu().numpy() == (ref[:, 3] > 0.5)).all(), pipeline


# ---- setters -------------------------------------------------------------------------------------------------------------------------------
def _edited(sd, what):
    sd = copy.deepcopy(sd)
    if what == "set_bsdf_reflectance":
        sd["bsdfs"][1]["reflectance"] = np.array([0.1, 0.2, 0.9], np.float32)
    elif what == "set_bsdf_param":
        sd["bsdfs"][2]["reflectance"] = np.array([0.625, 0.125, 0.375], np.float32)
    elif what == "set_emitter_radiance":
        sd["emitters"][0]["radiance"] = np.array([10.0, 12.0, 15.0], np.float32)
    else:
        sd["bsdfs"][4]["reflectance"] = dict(sd["bsdfs"][4]["reflectance"], data=TEX_B.copy())
    return sd


def _apply(g, what):
    if what == "set_bsdf_reflectance":
        g.set_bsdf_reflectance(1, [0.1, 0.2, 0.9])
    elif what == "set_bsdf_param":
        g.set_bsdf_param(2, 0, [0.625, 0.125, 0.375])
    elif what == "set_emitter_radiance":
        g.set_emitter_radiance(0, [10.0, 12.0, 15.0])
    else:
        assert g.texture_index(4) is not None
        g.update_texture(g.texture_index(4), TEX_B.copy())


def _film(gpu, g, p):
    sensor = gpu.make_sensor(p)
    assert gpu.PathIntegrator().render(g, sensor)
    return sensor.film().bitmap(raw=True).clone()


@pytest.mark.parametrize("what", ["set_bsdf_reflectance", "set_emitter_radiance", "set_bsdf_param", "update_texture"])
def test_setters_keep_the_frames(gpu, what):
    sd = scene("c")
    p = scenes.cornell_box_sensor(32, 32, 4, seed=21)
    ray = _gpu_ray(gpu, *rays(sd, 1024, 9))
    live = gpu.Scene(copy.deepcopy(sd))
    before_si, before_film = _si_planes(live.ray_intersect(ray)), _film(gpu, live, p)         # the device holds the old state
    _apply(live, what)
    fresh = gpu.Scene(_edited(sd, what))
    si, film = _si_planes(live.ray_intersect(ray)), _film(gpu, live, p)
    assert torch.isfinite(si[:, 0]).sum() >= 512
    assert torch.equal(si, _si_planes(fresh.ray_intersect(ray))) and torch.equal(si, before_si)       # no setter moves geometry
    assert torch.equal(film, _film(gpu, fresh, p))
    assert not torch.equal(film, before_film)


# ---- nothing to compute ----------------------------------------------------------------------------------------------------------------------
def test_scenes_without_primitives_or_with_the_light_alone(gpu, oracle):
    p = scenes.cornell_box_sensor(32, 32, 4, seed=2)
    sensor = gpu.make_sensor(p)
    empty = gpu.Scene(dict(meshes=[], bsdfs=[dict(type="diffuse", reflectance=[0.5] * 3)], emitters=[]))
    assert empty.info()["primitives"] == 0
    assert gpu.PathIntegrator().render(empty, sensor) and (sensor.film().bitmap().cpu().numpy() == 0).all()
    cb = scenes.cornell_box()
    sd = dict(cb, meshes=[cb["meshes"][LIGHT]])
    g = gpu.Scene(sd)
    assert g.info()["primitives"] == 2
    n = 32 * 32 * 4
    ref, ref_pos = oracle.OracleScene(sd, naive=True).sample_radiance(oracle.make_desc(p), 0, n)
    rgb, mask, pos = gpu.PathIntegrator().sample(g, sensor, 0, n)
    assert (ref[:, :3] > 0).any() and (rgb.cpu().numpy() == ref[:, :3]).all() and (pos.cpu().numpy() == ref_pos).all()

"""Scenes, edits and consumers shared by tests/test_live_scene_cpu.py and tests/test_gpu_live_scene.py.

An *edit* is what a caller does to a live scene's geometry: vertex moves pushed with one of the three `accel` values, with the normals
handed over or recomputed by the library, or moves followed by one explicit SAH rebuild.  `apply(live, sd, edit, moves)` performs it on
the live scene and returns the description a fresh scene has to be created from.  A *consumer* is one way of reading the scene: an
integrator's stream or film, a ray operator, a derivative render.  `CONSUMERS[name](gpu, scene, p)` returns a tuple of tensors; the first
is the one the non-vacuity floor is measured on.  Nothing here needs a device at import; the oracle halves (`oracle_*`) need none at all."""
import copy
import functools

import numpy as np

import vertex_moves as vm
from mitsuba2_amd import loaders, scenes

F32 = np.float32
MOVED_MIN = 0.05
ACCELS = ("refit", "rebuild", "rebuild-sah")
ALL_AOVS = "dx:duv_dx dy:duv_dy d:depth p:position uv:uv gn:geo_normal sn:sh_normal du:dp_du dv:dp_dv"          # every type aov_names offers
ROUGH = {"type": "roughconductor", "alpha": 0.3, "distribution": "ggx", "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14], "specular_reflectance": [0.9, 0.8, 0.7]}
REFLECTANCE, SPECULAR_REFLECTANCE, ETA, K, ALPHA = 0, 1, 2, 3, 4

# edit -> (normals, accel).  The flag word mtsamd_scene_update_vertices gets for the three "recompute" edits: 1, 1 | 2, 1 | 2 | 8.
EDITS = {
    "refit": (None, "refit"), "rebuild": (None, "rebuild"), "rebuild-sah": (None, "rebuild-sah"),
    "recompute-refit": ("recompute", "refit"), "recompute-rebuild": ("recompute", "rebuild"), "recompute-rebuild-sah": ("recompute", "rebuild-sah"),
    "moves-then-sah": (None, "refit"),          # every move refitted, then rebuild_accel(builder="sah")
}
HIERARCHY_EDITS = tuple(EDITS)
FLAT_EDITS = ("refit", "recompute-refit")          # a rebuild is a no-op on a flat scene
SPHERE_MOVES = (vm.SPHERE_MOVES["squash"], vm.SPHERE_MOVES["light"])          # the mesh with normals, then the emitter
CBOX_MOVES = (vm.CBOX_MOVES["short-box"], vm.CBOX_MOVES["light"])


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------
def sphere_scene():
    return vm.sphere_scene()


def cbox_scene(texture=None):
    """vm.cbox_scene() with vertex normals on the short box, so that normals="recompute" has a mesh to work on in a flat scene"""
    sd, p = scenes.cornell_box(texture=texture), vm.cbox_scene()[1]
    m = sd["meshes"][vm.CBOX_SHORT_BOX]
    sd["meshes"][vm.CBOX_SHORT_BOX] = dict(m, normals=np.ascontiguousarray(loaders.compute_vertex_normals(m["positions"], m["faces"]), F32))
    return sd, p


def texture(seed=7):
    return np.random.default_rng(seed).uniform(0.1, 0.9, size=(4, 6, 3)).astype(F32)


def envmap(seed=7):
    return np.random.RandomState(seed).uniform(0.2, 1.0, size=(8, 16, 3)).astype(F32)


def derivative_scene():
    """vm.sphere_scene() with a rough conductor sphere ("ball"), a bitmap-textured ground, an envmap (emitter 0) and the area light
    (emitter 1, shape "lamp"): every gradient family of the derivative renders has a parameter here"""
    sd, p = vm.sphere_scene()
    meshes = [dict(m) for m in sd["meshes"]]
    meshes[vm.SPHERE]["id"] = "ball"
    meshes[vm.FLOOR]["texcoords"] = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F32)
    meshes[vm.LIGHT].update(id="lamp", emitter=1)
    bsdfs = [dict(ROUGH, id="sphere"), dict(type="diffuse", id="ground", reflectance=dict(type="bitmap", data=texture())), dict(sd["bsdfs"][2], id="light")]
    emitters = [{"type": "envmap", "id": "sky", "data": envmap(), "scale": 0.8, "to_world": scenes.look_at([0, 0, 0], [1, 0.2, 0.3], [0, 1, 0])},
                dict(sd["emitters"][0])]
    return dict(meshes=meshes, bsdfs=bsdfs, emitters=emitters), p


def constant_table(c):
    """a tabulated spectrum that is the constant c: the oracle has the `uniform` constant c in its place (test_gpu_spectra.py)"""
    return {"type": "irregular", "wavelengths": [360.0, 500.0, 830.0], "values": [c, c, c]}


def spectral_scene(tabulated):
    """(the scene for the GPU, the scene for the oracle): the sphere scene, or the sphere carrying a tabulated / uniform 0.5"""
    sd, p = vm.sphere_scene()
    if not tabulated:
        return sd, sd, p
    with_bsdf = lambda b: dict(sd, bsdfs=[b] + list(sd["bsdfs"][1:]))
    return with_bsdf({"type": "diffuse", "reflectance": constant_table(0.5)}), with_bsdf({"type": "diffuse", "reflectance": 0.5}), p


def n_samples(p):
    return p["width"] * p["height"] * p["sample_count"]


# ---- edits ---------------------------------------------------------------------------------------------------------------------------------
def with_normals(sd, shape, pos, nrm):
    new = dict(sd, meshes=[dict(m) for m in sd["meshes"]])
    new["meshes"][shape] = dict(new["meshes"][shape], positions=np.ascontiguousarray(pos, F32).reshape(-1, 3), normals=np.ascontiguousarray(nrm, F32).reshape(-1, 3))
    return new


def apply(live, sd, edit, moves):
    """the edit on the live scene; returns the description of the scene as it is now.  Under a "recompute" edit a mesh with normals gets
    the normals the call returned (test_gpu_vertex_normals.py holds them to the specification), a mesh without goes the plain way."""
    import torch
    normals, accel = EDITS[edit]
    for move in moves:
        shape, pos, nrm = move(sd)
        dev = torch.from_numpy(pos).cuda()
        if normals == "recompute" and nrm is not None:
            got = live.update_vertices(shape, dev, normals="recompute", accel=accel)
            sd = with_normals(sd, shape, pos, got.cpu().numpy())
        else:
            live.update_vertices(shape, dev, accel=accel)
            sd = vm.moved(sd, move)
    if edit == "moves-then-sah":
        live.rebuild_accel(builder="sah")
    return sd


def rebuilds_of(edit, moves, flat=False):
    """(accel_info()["rebuilds"], builder) the edit leaves behind"""
    if flat:
        return 0, "sah"
    if edit == "moves-then-sah":
        return 1, "sah"
    accel = EDITS[edit][1]
    return (0, "sah") if accel == "refit" else (len(moves), "lbvh" if accel == "rebuild" else "sah")


def share(before, after):
    """the fraction of rows (vectors along the last axis; entries of a 1-D output) that differ; NaN equals NaN"""
    a, b = np.asarray(before), np.asarray(after)
    diff = ~((a == b) | ((a != a) & (b != b)))
    return float(diff.reshape(-1, diff.shape[-1]).any(1).mean()) if diff.ndim > 1 else float(diff.mean())


# ---- rays and reference points -----------------------------------------------------------------------------------------------------------------
def rays_of(sd, n=4096, seed=11):
    """_rays of test_gpu_vertex_update.py, sized by the description: origins round the scene's objects, aimed into their box, a quarter
    with a finite maxt of up to the box diagonal"""
    rng = np.random.RandomState(seed)
    allp = np.concatenate([np.asarray(m["positions"], np.float64).reshape(-1, 3) for m in sd["meshes"][:1] + sd["meshes"][2:]])
    lo, hi = allp.min(0), allp.max(0)
    pad = 0.25 * (hi - lo).max()
    o = rng.uniform(lo - pad, hi + pad, (n, 3)).astype(F32)
    d = rng.uniform(lo, hi, (n, 3)) - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    maxt = np.where(rng.rand(n) < 0.25, rng.uniform(0.1, 1.0, n) * np.linalg.norm(hi - lo), np.inf).astype(F32)
    return o, d, np.zeros(n, F32), maxt


def reference_points(sd, n=1000, seed=3):
    rng = np.random.default_rng(seed)
    allp = np.concatenate([np.asarray(m["positions"], np.float64).reshape(-1, 3) for m in sd["meshes"][:1] + sd["meshes"][2:]])
    return rng.uniform(allp.min(0), allp.max(0), size=(n, 3)).astype(F32), rng.uniform(size=(n, 2)).astype(F32)


def hand_made_directions(n=1000, seed=4):
    """direction samples nobody drew from the scene: unit d, unit n, a distance.  pdf_emitter_direction depends on them and on the
    emitter's record alone, so before and after an edit it differs exactly where the record does."""
    rng = np.random.default_rng(seed)
    unit = lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    return unit(rng.normal(size=(n, 3))), unit(rng.normal(size=(n, 3))), rng.uniform(0.5, 6.0, n).astype(F32)


# ---- the oracle's halves (no device) -----------------------------------------------------------------------------------------------------------
def oracle_stream(ob, sd, p, integrator="path", spectral_path=None):
    op = dict(p, integrator=integrator, **(dict(emitter_samples=1, bsdf_samples=1) if integrator == "direct" else {}))
    return ob.OracleScene(copy.deepcopy(sd), spectral_path=spectral_path).sample_radiance(ob.make_desc(op), 0, n_samples(p))


def oracle_aovs(ob, sd, p):
    """_expected of test_gpu_aov.py for any description: (positions, the 22 channels of ALL_AOVS), zeros on a miss"""
    cx, cy, cw, ch = p["crop"]
    d = ob.make_desc(p)
    o = ob.OracleScene(copy.deepcopy(sd))
    _, pos = o.sample_radiance(d, 0, n_samples(p))
    ro, rd, mint, maxt = ob.camera_rays(d, ((pos[:, 0] - F32(cx)) / F32(cw)).astype(F32), ((pos[:, 1] - F32(cy)) / F32(ch)).astype(F32))
    t, prim, _, u, v = o.ray_intersect(ro, rd, mint, maxt)
    hit = np.isfinite(t)
    want = np.zeros((len(t), 22), F32)
    si = o.fill_si(rd[hit], prim[hit], u[hit], v[hit])
    want[hit, 4] = t[hit]
    want[hit, 5:8], want[hit, 8:10], want[hit, 10:13] = si[:, 0:3], si[:, 6:8], si[:, 3:6]
    want[hit, 13:16], want[hit, 16:19], want[hit, 19:22] = si[:, 14:17], si[:, 17:20], si[:, 20:23]
    return pos, want


def oracle_queries(ob, sd, rays):
    """(t, prim, shape, u, v), any-hit mask, the 26 planes of fill_si (rows of missed rays are not defined)"""
    S = ob.OracleScene(copy.deepcopy(sd))
    ref, hit = S.ray_intersect(*rays, naive=True), S.ray_test(*rays, naive=True)
    return ref, hit, S.fill_si(rays[1], ref[1], ref[3], ref[4])


def oracle_emitter_samples(ob, sd, points, samples):
    S = ob.OracleScene(copy.deepcopy(sd))
    return np.stack([S.sample_emitter(points[i], samples[i]) for i in range(len(points))])


def dimage_of(p, seed=4):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, (p["height"], p["width"], 3)).astype(F32)


def oracle_derivative_gradients(ob, sd, p):
    """on derivative_scene(): the ten scalars of the ball's record through render_adjoint_param, the envmap texels through
    render_adjoint_envmap"""
    S = ob.OracleScene(copy.deepcopy(sd), naive=True)
    desc = ob.make_desc(p, analytic=True, film_rgb=True)
    _, film = S.render_image(desc)
    dimage = dimage_of(p)
    scalars = [(ALPHA, 0)] + [(kind, c) for kind in (SPECULAR_REFLECTANCE, ETA, K) for c in range(3)]
    param = np.array([S.render_adjoint_param(desc, dimage, film, [vm.SPHERE], kind, c, 0.003) for kind, c in scalars])
    return param, S.render_adjoint_envmap(desc, dimage, film, envmap().shape).astype(np.float64)


def oracle_diffuse_gradients(ob, sd, p, tex_floats):
    """on cbox_scene(texture()): reflectances per shape, texels, the lamp through render_adjoint"""
    S = ob.OracleScene(copy.deepcopy(sd), naive=True)
    desc = ob.make_desc(p, analytic=True, film_rgb=True)
    _, film = S.render_image(desc)
    gs, gt, ge = S.render_adjoint(desc, dimage_of(p), film, len(sd["meshes"]), tex_floats, n_emitters=1)
    return np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in (gs, gt, ge)])


# ---- the bound of float-atomic gradient sums ---------------------------------------------------------------------------------------------------
def in_bound(got, want):
    """|got - want| in units of the project's bound for two orders of the same fp32 atomic sum (test_gpu_reverse.py, fused against
    detached: equal bits, or rtol 1e-5, atol 1e-5 max|want|); 0.0 where the bits are equal"""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    if np.array_equal(got, want):
        return 0.0
    return float(np.max(np.abs(got - want) / (1e-5 * np.abs(want) + 1e-5 * np.abs(want).max())))


def gradient_share(before, after):
    """of the entries that are non-zero on either side, the fraction that differs by more than ten times the bound above"""
    a, b = np.asarray(before, np.float64).reshape(-1), np.asarray(after, np.float64).reshape(-1)
    nz = (a != 0) | (b != 0)
    bound = 1e-5 * np.abs(b) + 1e-5 * np.abs(b).max()
    return float((np.abs(a - b)[nz] > 10.0 * bound[nz]).mean()) if nz.any() else 0.0


# ---- consumers (device) ------------------------------------------------------------------------------------------------------------------------
def _clone(*tensors):
    return tuple(t.clone() for t in tensors)


def _stream(integ):
    return lambda gpu, scene, p: _clone(*integ(gpu).sample(scene, gpu.make_sensor(p), 0, n_samples(p)))


def _film(integ):
    def run(gpu, scene, p):
        sensor = gpu.make_sensor(p)
        assert integ(gpu).render(scene, sensor)
        return (sensor.film().bitmap(raw=True).clone(),)
    return run


def _aov_stream(aovs):
    return lambda gpu, scene, p: _clone(*gpu.AOVIntegrator(aovs).sample_aovs(scene, gpu.make_sensor(p), 0, n_samples(p)))


def _aov_nested(gpu, scene, p):
    integ = gpu.AOVIntegrator(ALL_AOVS, nested=gpu.PathIntegrator(max_depth=6))
    sensor = gpu.make_sensor(p)
    assert integ.render(scene, sensor)
    return (sensor.film().bitmap(raw=True).clone(),) + _clone(*integ.sample(scene, sensor, 0, n_samples(p)))


def gpu_ray(gpu, rays):
    import torch
    o, d, mint, maxt = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in rays)
    return gpu.Ray3f(o=o, d=d, mint=mint, maxt=maxt)


def si_planes(si):
    import torch
    return torch.cat([si.p, si.n, si.uv, si.sh_frame_s, si.sh_frame_t, si.sh_frame_n, si.dp_du, si.dp_dv, si.wi], dim=1)


def _zero_misses(t, *tensors):
    """the planes of a missed lane stay as the (uninitialised) output buffer had them: compare them as zeros"""
    import torch
    valid = torch.isfinite(t)
    return tuple(torch.where(valid.reshape([-1] + [1] * (x.dim() - 1)), x, torch.zeros_like(x)) for x in tensors)


def _kind(scene):
    return "cbox" if len(scene._dict["meshes"]) > 3 else "sphere"


@functools.lru_cache(maxsize=None)
def fixed_inputs(kind):
    """(rays, reference points, 2D samples) of the operator consumers, drawn once from the moved description: the same before and after
    an edit and on every scene of the kind"""
    if kind == "sphere":
        sd = vm.moved(sphere_scene()[0], *SPHERE_MOVES)
        return (rays_of(sd),) + reference_points(sd)
    sd = vm.moved(cbox_scene()[0], *CBOX_MOVES)
    rays = tuple(np.concatenate([a, b]) for a, b in zip(rays_of(sd, 2048), cbox_lamp_segments(2048)))
    return (rays,) + reference_points(sd)


def cbox_lamp_segments(n, seed=13):
    """The Cornell box is closed: an unbounded ray always hits something, whatever moves inside.  These segments start inside the room and
    end a quarter of a unit behind the plane of the lamp (half a unit under the ceiling), inside the lamp's quad as created: whether
    they hit anything is whether the lamp is still there."""
    rng = np.random.RandomState(seed)
    o = rng.uniform([20.0, 20.0, 20.0], [530.0, 500.0, 540.0], (n, 3))
    target = np.stack([rng.uniform(213.0, 343.0, n), np.full(n, 548.3), rng.uniform(227.0, 332.0, n)], 1)
    d = target - o
    dist = np.linalg.norm(d, axis=1)
    return o.astype(F32), (d / dist[:, None]).astype(F32), np.zeros(n, F32), (dist + 0.25).astype(F32)


def _ray_intersect_si(gpu, scene, p):
    si = scene.ray_intersect(gpu_ray(gpu, fixed_inputs(_kind(scene))[0]), full=True)
    return _clone(*_zero_misses(si.t, si_planes(si))) + _clone(si.t, si.prim_index, si.shape_index)


def _ray_test(gpu, scene, p):
    return (scene.ray_test(gpu_ray(gpu, fixed_inputs(_kind(scene))[0])).clone(),)


def _reference(gpu, scene):
    import torch
    _, points, samples = fixed_inputs(_kind(scene))
    si = gpu.SurfaceInteraction3f(t=None, prim_index=None, shape_index=None, p=torch.from_numpy(points).cuda())
    return si, torch.from_numpy(samples).cuda()


def _sample_emitter(gpu, scene, p):
    si, samples = _reference(gpu, scene)
    ds, spec = scene.sample_emitter_direction(si, samples, test_visibility=True)
    return _clone(spec, ds.p, ds.n, ds.d, ds.dist, ds.pdf, ds.delta, ds.object)


def _pdf_emitter(gpu, scene, p):
    import torch
    si, samples = _reference(gpu, scene)
    d, n, dist = (torch.from_numpy(a).cuda() for a in hand_made_directions(len(samples)))
    made = gpu.DirectionSample3f(p=None, n=n, d=d, dist=dist, pdf=None, delta=torch.zeros(len(dist), dtype=torch.bool, device="cuda"),
                                 object=torch.zeros(len(dist), dtype=torch.int32, device="cuda"))
    own, _ = scene.sample_emitter_direction(si, samples, test_visibility=False)
    return _clone(scene.pdf_emitter_direction(si, made), scene.pdf_emitter_direction(si, own))


def light_rays(n=4096, seed=12):
    """rays from below, aimed at a fixed region that holds the lamp before and after its move (4 x 4 around its axis: the lamp is 2 x 2 at
    height 4 before, 3 x 3 at 3.5 and shifted after), so that a fixed share of them ends on the emitter's front side"""
    rng = np.random.RandomState(seed)
    o = rng.uniform([-3.0, 0.2, -3.0], [3.0, 3.0, 3.0], (n, 3)).astype(F32)
    d = np.stack([rng.uniform(-2.0, 2.5, n), np.full(n, 4.0), rng.uniform(-2.0, 2.0, n)], 1) - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    return o, d, np.zeros(n, F32), np.full(n, np.inf, F32)


def cbox_light_rays(n=4096, seed=12):
    rng = np.random.RandomState(seed)
    o = rng.uniform([20.0, 20.0, 20.0], [530.0, 400.0, 540.0], (n, 3)).astype(F32)
    d = np.stack([rng.uniform(200.0, 356.0, n), np.full(n, 548.3), rng.uniform(214.0, 345.0, n)], 1) - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    return o, d, np.zeros(n, F32), np.full(n, np.inf, F32)


def _emitter_eval(gpu, scene, p):
    si = scene.ray_intersect(gpu_ray(gpu, cbox_light_rays() if _kind(scene) == "cbox" else light_rays()), full=True)
    return (si.emitter(scene).eval(si).clone(), si.shape_index.clone())


CONSUMERS = {
    "direct": _stream(lambda gpu: gpu.DirectIntegrator()),
    "depth": _stream(lambda gpu: gpu.DepthIntegrator()),
    "moment": _film(lambda gpu: gpu.MomentIntegrator(gpu.PathIntegrator(max_depth=6))),
    "aov-all": _aov_stream(ALL_AOVS),
    "aov-nested": _aov_nested,
    "ray-intersect-si": _ray_intersect_si,
    "ray-test": _ray_test,
    "sample-emitter": _sample_emitter,
    "pdf-emitter": _pdf_emitter,
    "emitter-eval": _emitter_eval,
}
for _name in ALL_AOVS.split():
    CONSUMERS["aov-" + _name.split(":")[1]] = _aov_stream(_name)
SPECTRAL_CONSUMER = _stream(lambda gpu: gpu.PathIntegrator(max_depth=6))
ALWAYS_ZERO = ("aov-duv_dx", "aov-duv_dy")          # zero in the reference too (aov.cpp never calls compute_partials): no floor to assert
# The flat scene's moves are a short translation and a shrinking lamp; dp_dv changes in 4.4 % of its camera samples only (the oracle,
# test_live_scene_cpu.py).  The channel is not run alone there; "aov-all" and "aov-nested" carry it on the flat scene, with the floor.
FLAT_WITHOUT_FLOOR = ("aov-dp_dv",)


# ---- sequences ---------------------------------------------------------------------------------------------------------------------------------
SEQUENCE_SEEDS = (5, 7, 22)
SEQUENCE_STEPS, SEQUENCE_CHECKS = 10, (3, 6, 10)
NORMAL_MODES = ("given", "host", "recompute")


def sequence(seed):
    """ten steps of a fixed random draw: ("move", target, accel, normals mode, numbers) | ("rebuild", builder) | ("texture", seed) |
    ("bsdf", three eighths) | ("radiance", three values) | ("envmap", seed)"""
    rng = np.random.RandomState(seed)
    steps = []
    for _ in range(SEQUENCE_STEPS):
        kind = rng.choice(["move", "move", "move", "move", "rebuild", "rebuild", "texture", "bsdf", "radiance", "envmap"])
        if kind == "move":
            steps.append(("move", ("sphere", "floor", "light")[rng.randint(3)], ACCELS[rng.randint(3)], NORMAL_MODES[rng.randint(3)],
                          (float(rng.uniform(0.6, 1.3)), float(rng.uniform(-0.4, 0.4)), float(rng.uniform(-0.3, 0.3)))))
        elif kind == "rebuild":
            steps.append(("rebuild", ("lbvh", "sah")[rng.randint(2)]))
        elif kind in ("texture", "envmap"):
            steps.append((kind, int(rng.randint(100, 1000))))
        else:
            steps.append((kind, tuple(float(x) / 8.0 for x in rng.randint(1, 8 if kind == "bsdf" else 160, 3))))
    return steps


def sequence_move(step):
    _, target, _, _, (s, dx, dz) = step
    if target == "sphere":
        return vm.scale_about(vm.SPHERE, (s, 1.0 / s, s), vm.SPHERE_CENTRE, shift=(dx, 0.0, dz))
    if target == "floor":
        return vm.scale_about(vm.FLOOR, (s, 1.0, s), (0, 0, 0))
    return vm.scale_about(vm.LIGHT, s, shift=(dx, dz, 0.0))


def sequence_facts(steps):
    """what the CPU test asserts of every seed: a rebuild of each builder followed later by a refit, and a "recompute" after a rebuild"""
    rebuilt, refit_after, recompute_after = set(), set(), False
    for step in steps:
        if step[0] == "rebuild":
            rebuilt.add(step[1])
        elif step[0] == "move":
            if step[2] == "refit":
                refit_after |= rebuilt
            if step[1] == "sphere" and step[3] == "recompute" and rebuilt:
                recompute_after = True
            if step[2] != "refit":
                rebuilt.add("lbvh" if step[2] == "rebuild" else "sah")
    return refit_after, recompute_after


def sequence_step(live, sd, step):
    """one step on the live scene (None: only the tracked description is advanced); returns (description, rebuilds made)"""
    import torch
    if step[0] == "move":
        _, target, accel, mode, _ = step
        shape, pos, nrm = sequence_move(step)(sd)
        made = int(accel != "refit")
        if nrm is None:
            if live is not None:
                live.update_vertices(shape, torch.from_numpy(pos).cuda(), accel=accel)
            return vm.moved(sd, sequence_move(step)), made
        if mode == "recompute":
            if live is None:
                return vm.moved(sd, sequence_move(step)), made
            got = live.update_vertices(shape, torch.from_numpy(pos).cuda(), normals="recompute", accel=accel)
            return with_normals(sd, shape, pos, got.cpu().numpy()), made
        if mode == "given":          # normals of the caller's own: those of the mesh before the move
            nrm = np.ascontiguousarray(sd["meshes"][shape]["normals"], F32)
        if live is not None:
            live.update_vertices(shape, pos, normals=nrm if mode == "given" else None, accel=accel)
        return with_normals(sd, shape, pos, nrm), made
    new = dict(sd, bsdfs=[dict(b) for b in sd["bsdfs"]], emitters=[dict(e) for e in sd["emitters"]])
    if step[0] == "rebuild":
        if live is not None:
            live.rebuild_accel(builder=step[1])
        return sd, 1
    if step[0] == "texture":
        data = texture(step[1])
        if live is not None:
            live.update_texture(live.texture_index(1), data)
        new["bsdfs"][1] = dict(new["bsdfs"][1], reflectance=dict(new["bsdfs"][1]["reflectance"], data=data))
    elif step[0] == "bsdf":
        if live is not None:
            live.set_bsdf_param(0, SPECULAR_REFLECTANCE, step[1])
        new["bsdfs"][0] = dict(new["bsdfs"][0], specular_reflectance=list(step[1]))
    elif step[0] == "radiance":
        if live is not None:
            live.set_emitter_radiance(1, step[1])
        new["emitters"][1] = dict(new["emitters"][1], radiance=np.array(step[1], F32))
    else:
        data = envmap(step[1])
        if live is not None:
            live.update_envmap(data)
        new["emitters"][0] = dict(new["emitters"][0], data=data)
    return new, 0

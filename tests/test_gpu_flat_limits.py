"""LDS-resident scenes at their primitive and table limits, on the device (tests/flat_limits.py builds the scenes and restates the LDS
arithmetic; tests/test_flat_limits_cpu.py pins the arithmetic and the flat / hierarchy boundary without a GPU).

* 1, 2, 3, 63, 64 triangles (64: 32 pairs, a full pair mask; 63: a half-empty last pair) and 65, the smallest hierarchy scene, as one
  shape, as one-triangle shapes (every pair straddles two shapes, every area emitter is a single triangle) and in odd-sized shapes:
  ray queries on hard rays and per-sample radiance in every schedule, bit for bit against the oracle.
* Cornell boxes under hundreds of delta emitters: each launch formula (k_mega / k_finish, the 256-thread kernels, k_shade with its shadow
  rings) with its dynamic LDS between 48 and 64 KiB, near 100 KiB and at the last emitter count that is still flat; one emitter more
  and the scene is a hierarchy scene, seen through the refusal of pipeline 4, with the same samples.
* emitter selection among ~300 emitters, and the adjoint kernel on 64 shapes with 64 emitters.

On an MI355X: 72 cases, the file alone in 6.4 s; the slowest case is test_drain_at_64_triangles[rgb] (three renders of 256 x 256 at
64 spp) at 0.26 s, every other case stays below 0.2 s."""
import ctypes as C
import functools

import numpy as np
import parity_util
import pytest
import torch

import flat_limits as fl
import oracle_binding as ob
from mitsuba2_amd import scenes
from stress_rays import stress_rays

pytestmark = pytest.mark.gpu
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- ray queries -------------------------------------------------------------------------------------------------------------------------
def _reversed(sd):
    """the same triangles in the opposite primitive order (one mesh), and the map from its primitive indices to the original ones"""
    tri = np.concatenate([np.asarray(m["positions"], F32)[np.asarray(m["faces"]).astype(np.int64)] for m in sd["meshes"]])[::-1]
    mesh = dict(positions=np.ascontiguousarray(tri.reshape(-1, 3)), faces=np.arange(3 * len(tri), dtype=np.uint32).reshape(-1, 3), normals=None,
                texcoords=None, bsdf=0, emitter=-1)
    return dict(meshes=[mesh], bsdfs=[dict(type="diffuse", reflectance=F32([0.5, 0.5, 0.5]))], emitters=[]), len(tri) - 1 - np.arange(len(tri))


def _in_plane(sd, d):
    """rays that lie in the plane of some triangle: |d . n| < 1e-6 in double precision (fp32 directions are good to 6e-8, so this is
    'zero up to rounding').  There the determinant of the triangle test is rounding noise and so is its verdict."""
    tri = np.concatenate([np.asarray(m["positions"], np.float64)[np.asarray(m["faces"]).astype(np.int64)] for m in sd["meshes"]])
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return (np.abs(d.astype(np.float64) @ nrm.T) < 1e-6).any(1)


@pytest.mark.parametrize("partition", fl.PARTITIONS)
@pytest.mark.parametrize("n_tris", fl.SOUP_SIZES)
def test_ray_queries_match_brute_force(gpu, oracle, n_tris, partition):
    """ray_intersect (t, primitive, u, v, shape), ray_intersect_naive and ray_test against the oracle's brute force and each other, all
    lanes active and 60 % of them, the last wave partial.  Flat scenes test their triangles in primitive order as brute force does, so
    every field is equal.  The 65-triangle scene walks a BVH, which may meet the two triangles of an exact tie in either order: a ray
    ties iff brute force over the reversed primitive order names another primitive; there the walk may return either of the two, with
    the same t (as a value: a tie at the ray's origin may be +0 on one triangle and -0 on the other).  And a ray in the plane of a triangle
    can be "hit" by the fp32 triangle test far outside that triangle (met here: 1.4 units outside a triangle of size 1, where double
    precision finds u + v = 1.38); brute force reports that, a walk never looks there, no padding of the boxes can make them agree and
    the walk's answer is the geometric one.  So on the 65-triangle scene the walk may differ from brute force on rays in the plane of
    some triangle, on fewer than one ray in a thousand; the device's own brute force equals the oracle's everywhere."""
    sd = fl.soup(n_tris, partition, 64)
    scene, S = gpu.Scene(sd), oracle.OracleScene(sd)
    prim_shape = np.array([i for i, m in enumerate(sd["meshes"]) for _ in range(len(m["faces"]))], np.uint32)
    assert fl.counts(sd)[1] == (n_tris + 1) // 2
    o, d, mint, maxt = stress_rays(sd, 5)
    n = len(o) - 27                                        # the last wave is partial
    o, d, mint, maxt = o[:n], d[:n], mint[:n], maxt[:n]
    ray = gpu.Ray3f(o=_cuda(o), d=_cuda(d), mint=_cuda(mint), maxt=_cuda(maxt))
    t_all, prim_all, shape_all, u_all, v_all = S.ray_intersect(o, d, mint, maxt, naive=True)
    hit_all = S.ray_test(o, d, mint, maxt, naive=True)
    found = np.isfinite(t_all)
    assert found.sum() > n // 4 and (t_all == 0).sum() > 0
    assert np.array_equal(shape_all[found], prim_shape[prim_all[found]])
    if n_tris >= 63:                                       # the last pair (64: the 32nd) is reached
        assert (prim_all[found] == n_tris - 1).any() and (prim_all[found] == n_tris - 2).any()
    alt = prim_all
    if n_tris > fl.FLAT_MAX:
        rsd, back = _reversed(sd)
        t_r, prim_r, _, _, _ = oracle.OracleScene(rsd).ray_intersect(o, d, mint, maxt, naive=True)
        assert np.array_equal(t_r, t_all)                   # as values: the two triangles of a tie at the origin may give +0 and -0
        alt = np.where(found, back[np.minimum(prim_r, n_tris - 1)], prim_all).astype(np.uint32)
        assert 0 < (alt != prim_all).sum() < n // 10
    noise = _in_plane(sd, d) if n_tris > fl.FLAT_MAX else np.zeros(n, bool)
    for partial in (False, True):
        act = (np.random.RandomState(9).rand(n) < 0.6) if partial else np.ones(n, bool)
        active = _cuda(act.astype(np.uint8)) if partial else True
        t_o = np.where(act, t_all, np.inf).astype(F32)
        prim_o = np.where(act, prim_all, np.uint32(0xffffffff)).astype(np.uint32)
        alt_o = np.where(act, alt, np.uint32(0xffffffff)).astype(np.uint32)
        u_o, v_o = np.where(act, u_all, 0.0).astype(F32), np.where(act, v_all, 0.0).astype(F32)
        res = scene.ray_intersect(ray, active=active, full=False)
        rn = scene.ray_intersect_naive(ray, active=active)
        for name, r, exact in (("ray_intersect", res, n_tris <= fl.FLAT_MAX), ("ray_intersect_naive", rn, True)):
            t_g, prim_g, uv_g = r.t.cpu().numpy(), r.prim_index.cpu().numpy().astype(np.uint32), r.prim_uv.cpu().numpy()
            shape_g = r.shape_index.cpu().numpy().astype(np.uint32)
            same = prim_g == prim_o
            mism = np.where(same, _bits(t_g) != _bits(t_o), t_g != t_o) | (same & ((uv_g[:, 0] != u_o) | (uv_g[:, 1] != v_o))) | (~same & (prim_g != alt_o))
            if exact:
                mism |= ~same
            else:
                assert (mism & noise).sum() < n // 1000, (name, partial, int((mism & noise).sum()))
                mism &= ~noise
            assert mism.sum() == 0, (name, partial, int(mism.sum()), [(int(i), float(t_g[i]), int(prim_g[i]), float(t_o[i]), int(prim_o[i])) for i in np.nonzero(mism)[0][:6]])
            hit = act & found
            assert np.array_equal(shape_g[hit], prim_shape[prim_g[hit]]), name
        if n_tris <= fl.FLAT_MAX:
            assert np.array_equal(_bits(rn.prim_uv.cpu().numpy()), _bits(res.prim_uv.cpu().numpy()))
        hit_g = scene.ray_test(ray, active=active).cpu().numpy()
        bad = hit_g != (hit_all & act)
        assert (bad & noise).sum() < n // 1000, ("ray_test", partial, int((bad & noise).sum()))
        bad = np.nonzero(bad & ~noise)[0]
        assert bad.size == 0, ("ray_test", partial, bad[:6].tolist())


# ---- per-sample radiance on the soups ------------------------------------------------------------------------------------------------
RADIANCE_SOUPS = [(n, p) for n in (63, 64, 65) for p in fl.PARTITIONS] + [(n, "per_triangle") for n in (1, 2, 3)]
W, H, SPP = 32, 32, 4


@functools.lru_cache(maxsize=None)
def _reference(n_tris, partition, variant, max_depth, integrator="path"):
    """oracle samples of a soup, computed once and shared by the schedules compared with them"""
    p = dict(fl.soup_sensor(W, H, SPP, max_depth=max_depth))
    if integrator == "direct":
        p.update(integrator="direct", emitter_samples=2, bsdf_samples=1, hide_emitters=False)
    elif integrator == "depth":
        p.update(integrator="depth")
    from mitsuba2_amd import render as R
    S = ob.OracleScene(fl.soup(n_tris, partition, 64), spectral_path=R.srgb_coeff_path() if variant == "spectral" else None)
    want, pos = S.sample_radiance(ob.make_desc(p), 0, W * H * SPP)
    want.setflags(write=False); pos.setflags(write=False)
    return want, pos


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
@pytest.mark.parametrize("n_tris,partition", RADIANCE_SOUPS)
def test_soup_radiance_matches_oracle(gpu, n_tris, partition, variant):
    """every schedule of the path integrator: 0 (small pass: k_mega), 1 (k_bounce*), 3 (k_shade + queued shadow rays), 4 (k_shade with
    shadow rings, k_finish); the 65-triangle scene has the hierarchy schedules 0, 1, 2"""
    sd = fl.soup(n_tris, partition, 64)
    scene, n = gpu.Scene(sd, variant=variant), W * H * SPP
    for max_depth in (-1, 3):
        want, wpos = _reference(n_tris, partition, variant, max_depth)
        assert (want[:, 3] > 0.5).mean() >= 0.25 and (want[:, :3].max(1) > 0).mean() >= 0.10
        sensor = gpu.make_sensor(fl.soup_sensor(W, H, SPP, max_depth=max_depth))
        for pipeline in ((0, 1, 3, 4) if n_tris <= fl.FLAT_MAX else (0, 1, 2)):
            got, mask, pos = gpu.PathIntegrator(max_depth=max_depth, pipeline=pipeline).sample(scene, sensor, 0, n)
            assert np.array_equal(pos.cpu().numpy(), wpos) and np.array_equal(mask.cpu().numpy(), want[:, 3] > 0.5)
            parity_util.check("soup %d %s %s depth %d pipeline %d" % (n_tris, partition, variant, max_depth, pipeline), got.cpu().numpy(), want[:, :3])
    if n_tris > fl.FLAT_MAX:
        with pytest.raises(RuntimeError, match="LDS-resident scenes only"):
            gpu.PathIntegrator(pipeline=4).sample(scene, gpu.make_sensor(fl.soup_sensor(W, H, SPP)), 0, n)


@pytest.mark.parametrize("n_tris,partition", RADIANCE_SOUPS)
def test_soup_direct_and_depth_match_oracle(gpu, n_tris, partition):
    scene, n = gpu.Scene(fl.soup(n_tris, partition, 64)), W * H * SPP
    sensor = gpu.make_sensor(fl.soup_sensor(W, H, SPP))
    for name, integ in (("direct", gpu.DirectIntegrator(emitter_samples=2, bsdf_samples=1)), ("depth", gpu.DepthIntegrator())):
        want, wpos = _reference(n_tris, partition, "rgb", -1, name)
        got, mask, pos = integ.sample(scene, sensor, 0, n)
        assert np.array_equal(pos.cpu().numpy(), wpos) and np.array_equal(mask.cpu().numpy(), want[:, 3] > 0.5)
        parity_util.check("soup %d %s %s" % (n_tris, partition, name), got.cpu().numpy(), want[:, :3])


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
def test_drain_at_64_triangles(gpu, variant):
    """the film of test_gpu_gather_drain.py (256 x 256 at 64 spp: the launch rounds pass through every gathering width) on 64 one-triangle
    shapes: gathering drain, k_finish as soon as the cursors are dry, and the fused kernel give one film"""
    sd = fl.soup(64, "per_triangle", 64)
    p = fl.soup_sensor(256, 256, 64, seed=5)
    films, stats = [], []
    for pipeline, finish_kernel in ((4, 1), (4, 2), (1, 0)):
        scene, sensor = gpu.Scene(sd, variant=variant), gpu.make_sensor(p)
        integ = gpu.PathIntegrator(pipeline=pipeline)
        integ.finish_kernel = finish_kernel
        assert integ.render(scene, sensor)
        films.append(sensor.film().bitmap(raw=True).clone()); stats.append(dict(integ.stats))
    assert stats[0]["iterations"] > stats[1]["iterations"]                   # the launch rounds really drained the pool
    for k in ("samples", "segments", "closest_hit_rays", "any_hit_rays"):
        assert stats[0][k] == stats[1][k] == stats[2][k], (k, [s[k] for s in stats])
    assert torch.equal(films[0], films[1]) and torch.equal(films[0], films[2])
    assert torch.isfinite(films[0]).all() and films[0][..., :3].max() > 0


# ---- table sizes: the Cornell box under many delta emitters ---------------------------------------------------------------------------
CBOX_COUNTS = fl.counts(scenes.cornell_box())
BANDS = fl.bands(CBOX_COUNTS)
CW, CH, CSPP = 32, 32, 4


def _lit_cbox(n_extra):
    return fl.many_lights(scenes.cornell_box(), n_extra - n_extra // 3, n_extra // 3, 0)


@functools.lru_cache(maxsize=None)
def _cbox_reference(n_extra, variant, integrator="path"):
    p = dict(scenes.cornell_box_sensor(CW, CH, CSPP, seed=2, max_depth=4))
    if integrator == "direct":
        p.update(integrator="direct", emitter_samples=2, bsdf_samples=1, hide_emitters=False)
    from mitsuba2_amd import render as R
    S = ob.OracleScene(_lit_cbox(n_extra), spectral_path=R.srgb_coeff_path() if variant == "spectral" else None)
    want, pos = S.sample_radiance(ob.make_desc(p), 0, CW * CH * CSPP)
    want.setflags(write=False); pos.setflags(write=False)
    return want, pos


# (formula, variant, the launches that are sized by it): pipeline 0 on a small pass is k_mega; pipeline 4 is k_shade with the rings, its
# drain gathering (finish_kernel = 1) and k_finish
BAND_CASES = [("mega", "rgb"), ("block", "rgb"), ("ring_rgb", "rgb"), ("ring_spectral", "spectral")]


@pytest.mark.parametrize("place", ["mid", "100k", "last_flat"])
@pytest.mark.parametrize("formula,variant", BAND_CASES)
def test_table_bands_match_oracle(gpu, formula, variant, place):
    n_extra = BANDS[(formula, place)]
    c = fl._with_emitters(CBOX_COUNTS, n_extra)
    assert fl.VARIANT[formula] == variant and fl.is_flat(c, variant == "spectral")
    demand = fl.FORMULAS[formula](c)
    if place == "mid":
        assert 48 * 1024 < demand < 64 * 1024
    scene, n = gpu.Scene(_lit_cbox(n_extra), variant=variant), CW * CH * CSPP
    sensor = gpu.make_sensor(scenes.cornell_box_sensor(CW, CH, CSPP, seed=2, max_depth=4))
    want, wpos = _cbox_reference(n_extra, variant)
    runs = {"mega": [(0, 0)], "block": [(1, 0)], "ring_rgb": [(4, 0), (4, 1)], "ring_spectral": [(4, 0), (4, 1)]}[formula]
    for pipeline, finish_kernel in runs:
        integ = gpu.PathIntegrator(max_depth=4, pipeline=pipeline)
        integ.finish_kernel = finish_kernel
        got, mask, pos = integ.sample(scene, sensor, 0, n)
        assert np.array_equal(pos.cpu().numpy(), wpos) and np.array_equal(mask.cpu().numpy(), want[:, 3] > 0.5)
        parity_util.check("cbox + %d lights (%s %d B) pipeline %d finish %d" % (n_extra, formula, demand, pipeline, finish_kernel), got.cpu().numpy(), want[:, :3])
    if formula == "block":
        want, wpos = _cbox_reference(n_extra, "rgb", "direct")
        got, mask, pos = gpu.DirectIntegrator(emitter_samples=2, bsdf_samples=1).sample(scene, sensor, 0, n)
        assert np.array_equal(pos.cpu().numpy(), wpos) and np.array_equal(mask.cpu().numpy(), want[:, 3] > 0.5)
        parity_util.check("cbox + %d lights direct" % n_extra, got.cpu().numpy(), want[:, :3])


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
def test_first_count_over_the_cap_is_a_hierarchy_scene(gpu, variant):
    """one emitter more than the last flat count: the scene is demoted (pipeline 4 refuses it as it refuses every hierarchy scene) and
    renders the same samples through its BVH"""
    n_extra = BANDS[("ring_spectral" if variant == "spectral" else "ring_rgb", "first_hier")]
    spectral = variant == "spectral"
    assert not fl.is_flat(fl._with_emitters(CBOX_COUNTS, n_extra), spectral) and fl.is_flat(fl._with_emitters(CBOX_COUNTS, n_extra - 1), spectral)
    scene, n = gpu.Scene(_lit_cbox(n_extra), variant=variant), CW * CH * CSPP
    sensor = gpu.make_sensor(scenes.cornell_box_sensor(CW, CH, CSPP, seed=2, max_depth=4))
    with pytest.raises(RuntimeError, match="LDS-resident scenes only"):
        gpu.PathIntegrator(max_depth=4, pipeline=4).sample(scene, sensor, 0, n)
    want, wpos = _cbox_reference(n_extra, variant)
    for pipeline in (0, 2):
        got, mask, pos = gpu.PathIntegrator(max_depth=4, pipeline=pipeline).sample(scene, sensor, 0, n)
        assert np.array_equal(pos.cpu().numpy(), wpos) and np.array_equal(mask.cpu().numpy(), want[:, 3] > 0.5)
        parity_util.check("cbox + %d lights (hierarchy) %s pipeline %d" % (n_extra, variant, pipeline), got.cpu().numpy(), want[:, :3])


# ---- emitter selection among many emitters ---------------------------------------------------------------------------------------------
def test_emitter_selection_among_300(gpu):
    """Scene.sample_emitter_direction / pdf_emitter_direction on the Cornell box with 200 point and 100 spot lights behind its area
    light, all 15 outputs against OracleScene.sample_emitter (no `directional` emitter: the oracle's entry point cannot evaluate one)"""
    R = gpu
    sd = fl.many_lights(scenes.cornell_box(), 200, 100, 0)
    scene, S = R.Scene(sd), ob.OracleScene(sd)
    n_em = len(sd["emitters"])
    assert n_em == 301
    n = 2049
    rng = np.random.default_rng(3)
    ref = rng.uniform((10, 10, 10), (540, 540, 550), size=(n, 3)).astype(F32)
    sample = rng.uniform(size=(n, 2)).astype(F32)
    sample[0], sample[1] = 0.0, np.nextafter(F32(1.0), F32(0.0))
    picked = np.minimum((sample[:, 0] * F32(n_em)).astype(np.uint32), n_em - 1)
    assert picked[0] == 0 and picked[1] == n_em - 1 and len(set(picked.tolist())) > 250
    si = R.SurfaceInteraction3f(t=None, prim_index=None, shape_index=None, p=torch.as_tensor(ref, device="cuda"))
    ds, spec = scene.sample_emitter_direction(si, torch.as_tensor(sample, device="cuda"), test_visibility=False)
    pdf_dir = scene.pdf_emitter_direction(si, ds).cpu().numpy()
    got = np.concatenate([ds.d.cpu().numpy(), ds.dist.cpu().numpy()[:, None], ds.pdf.cpu().numpy()[:, None], ds.n.cpu().numpy(),
                          ds.p.cpu().numpy(), spec.cpu().numpy(), pdf_dir[:, None]], axis=1)
    assert np.array_equal(ds.object.cpu().numpy(), picked.astype(np.int32))
    want = np.stack([S.sample_emitter(ref[i], sample[i]) for i in range(n)])
    for c in range(15):
        assert np.array_equal(got[:, c], want[:, c]), ("output", c, np.nonzero(got[:, c] != want[:, c])[0][:8].tolist())
    types = np.array([sd["emitters"][k].get("type", "area") for k in picked])
    assert np.array_equal(ds.delta.cpu().numpy(), types != "area") and (types == "area").any() and (types == "spot").sum() > 100
    assert np.abs(got[:, 11:14]).max() > 0


# ---- the adjoint kernel with large tables ------------------------------------------------------------------------------------------------
def test_adjoint_on_64_shapes(gpu, oracle):
    """mtsamd_render_adjoint against mo_render_adjoint as tests/test_gpu_autodiff.py::test_adjoint_matches_oracle sets them up (same
    tolerance), on the 64-triangle soup of one-triangle shapes made diffuse: 64 shapes and 64 area emitters in LDS.  The reflectance
    gradients cover 32 records (the kernel's limit), which the 64 shapes share in turn."""
    from mitsuba2_amd import autodiff, _lib as L
    sd = fl.diffuse(fl.soup(64, "per_triangle", 64), 32)
    p = dict(fl.soup_sensor(24, 20, 4, seed=5, max_depth=3))
    sensor = gpu.make_sensor(p)
    scene = gpu.Scene(sd, sensor=sensor, integrator=gpu.PathIntegrator(max_depth=3))
    d = autodiff._desc(scene, sensor, scene.integrator(), None, p["seed"])
    film = autodiff._render_film(scene, d)
    desc = oracle.make_desc(p, analytic=True, film_rgb=True)
    S = oracle.OracleScene(sd, naive=True)
    image_o, film_o = S.render_image(desc)
    assert np.allclose(film.cpu().numpy()[..., 4], film_o[..., 4], rtol=1e-5, atol=1e-6)
    assert np.mean((film.cpu().numpy()[..., :3] - film_o[..., :3]) ** 2 / (film_o[..., :3] ** 2 + 1e-2)) < 1e-5
    dimage = np.random.RandomState(2).randn(20, 24, 3).astype(F32)
    gs_o, _ = S.render_adjoint(desc, dimage, film_o, len(sd["meshes"]), 0)
    g_bsdf = torch.zeros((len(sd["bsdfs"]), 3), device="cuda")
    di = torch.from_numpy(dimage).cuda()
    L.check(L.lib().mtsamd_render_adjoint(scene._handle, C.byref(d), C.c_void_p(di.data_ptr()), C.c_void_p(film.data_ptr()),
                                          C.c_void_p(g_bsdf.data_ptr()), None, None, None))
    torch.cuda.synchronize()
    gb_o = np.zeros((len(sd["bsdfs"]), 3), F32)
    for si, m in enumerate(sd["meshes"]):
        gb_o[m["bsdf"]] += gs_o[si]
    gb = g_bsdf.cpu().numpy()
    assert np.abs(gb_o).max() > 1e-3 and (np.abs(gb_o).max(1) > 0).sum() >= 16
    assert np.allclose(gb, gb_o, rtol=2e-2, atol=2e-3 * np.abs(gb_o).max())

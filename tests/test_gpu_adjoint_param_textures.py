"""Texel gradients of bitmaps bound to BSDF parameters -- alpha / alpha_u / alpha_v of the rough models, specular_reflectance and
specular_transmittance of the conductors and dielectrics (mtsamd_render_adjoint_param_textures, k_adjoint_param_tex):

1. by splitting, against the unchanged oracle (flat scenes): param_texel_scenes.py;
2. the hierarchy instantiation at a launch edge, against the constant-parameter route;
3. anisotropy: one map on alpha_u, another on alpha_v;
4. finite differences through autodiff.render;
5. a small inversion of a roughness map;
6. the keys of traverse() and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import param_texel_scenes as pts
from test_gpu_adjoint_textures import _open_box, _primal, _scene, _sky, _tex_floats
from test_gpu_textured_params import CONDUCTOR_IOR

pytestmark = pytest.mark.gpu
F32 = np.float32
LUM = np.array([0.212671, 0.715160, 0.072169])
ALPHA, ALPHA_U, ALPHA_V, SPEC, TRANS, ETA = 4, 6, 7, 1, 5, 2


def _call(scene, d, film, dimage, param, h, g):
    from mitsuba2_amd import _lib as L
    return L.lib().mtsamd_render_adjoint_param_textures(scene._handle, C.byref(d), C.c_void_p(dimage.data_ptr()), C.c_void_p(film.data_ptr()),
                                                        int(param), float(h), C.c_void_p(g.data_ptr()), None)


def _grad(scene, d, film, dimage, param, h):
    """the whole texture-gradient buffer of one call into zeros (torch, on the device)"""
    from mitsuba2_amd import _lib as L
    g = torch.zeros(_tex_floats(scene), device="cuda")
    L.check(_call(scene, d, film, dimage, param, h, g))
    torch.cuda.synchronize()
    return g


def _texels(scene, g, texture):
    from mitsuba2_amd import autodiff
    return autodiff._texture_slice(scene, g, texture).cpu().numpy().astype(np.float64)


def _constant_route(scene, d, film, dimage, bsdf, kind, comp, h):
    from mitsuba2_amd import _lib as L
    want = torch.zeros(1, device="cuda")
    L.check(L.lib().mtsamd_render_adjoint_param(scene._handle, C.byref(d), C.c_void_p(dimage.data_ptr()), C.c_void_p(film.data_ptr()),
                                                int(bsdf), int(kind), int(comp), float(h), C.c_void_p(want.data_ptr()), None))
    torch.cuda.synchronize()
    return float(want.item())


# ---- 1. split against the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pts.SPLIT_CASES)
def test_split_matches_oracle_parameter_adjoint(gpu, oracle, case):
    """Every lookup of the 2 x 9 maps interpolates equal texels, so the texel gradients of a cell sum to the oracle's derivative with
    respect to the constant of that cell (mo_render_adjoint_param over the cell's mesh, same h): the same paths on both sides (the
    primal films agree), two sums of the same terms -- 2e-3 |want| + 1e-5, the figure of test_bsdf_parameter_adjoint_matches_oracle.
    max_depth 7 is past rr_depth 5: the Russian-roulette factor is held fixed on both sides."""
    from mitsuba2_amd import autodiff
    mine, _, params = pts.split_scenes(case)
    p = pts.sensor_params()
    sensor = gpu.make_sensor(p)
    integ = gpu.PathIntegrator(max_depth=pts.MAX_DEPTH)
    scene = gpu.Scene(mine, sensor=sensor, integrator=integ)
    d = autodiff._desc(scene, sensor, integ, 8, pts.SEED)
    film = autodiff._render_film(scene, d)
    film_o, wants = pts.oracle_wants(case)
    assert np.allclose(film.cpu().numpy(), film_o, rtol=2e-5, atol=1e-6)
    dimage = torch.from_numpy(pts.dimage()).cuda()
    bsdf = len(mine["bsdfs"]) - 1
    for pname in params:
        texture = scene.texture_index(bsdf, pname)
        assert texture is not None
        gt = _texels(scene, _grad(scene, d, film, dimage, pts.KIND[pname], pts.H_STEP), texture)
        assert gt.shape == (2, 9, 3)
        assert np.all(gt[:, 0] == 0.0), (case, pname, gt[:, 0])            # no lookup touches column 0
        for cell, cols in enumerate(pts.CELL_COLUMNS):
            for comp in range(1 if pname == "alpha" else 3):
                want = wants[(pname, cell, comp)]
                got = float(gt[:, cols].sum() if pname == "alpha" else gt[:, cols, comp].sum())
                print("%s %s cell %d comp %d: got %.7g want %.7g rel %.3g" % (case, pname, cell, comp, got, want, abs(got - want) / abs(want)))
                assert abs(want) > 1e-3
                assert abs(got - want) <= 2e-3 * abs(want) + 1e-5, (case, pname, cell, comp, got, want)
        if pname == "alpha":      # the roughness is the luminance of the texel: the channels share the gradient in that ratio
            ch = gt.sum((0, 1))
            print("%s alpha channel shares %s" % (case, (ch / ch.sum()).tolist()))
            assert np.all(np.abs(ch / ch.sum() - LUM) <= 1e-5 * LUM), (case, (ch / ch.sum()).tolist())


# ---- 2. hierarchy scenes, a launch edge ---------------------------------------------------------------------------------------------------
def _sphere_scene(gpu, alpha):
    from mitsuba2_amd import scenes
    sd = scenes.bumpy_sphere(4, 11)        # 70 triangles: the smallest tessellation above the 64 primitives of an LDS-resident scene
    sphere = sd["meshes"][0]
    sphere = dict(sphere, texcoords=np.random.default_rng(8).uniform(0.0, 1.0, size=(sphere["positions"].shape[0], 2)).astype(F32))
    mat = dict(type="roughconductor", distribution="ggx", alpha=alpha, **CONDUCTOR_IOR)
    sd = dict(sd, meshes=[sphere] + sd["meshes"][1:], bsdfs=[mat] + sd["bsdfs"][1:])
    p = scenes.bumpy_sphere_sensor(25, 19, spp=3, seed=5, max_depth=7)          # 1425 samples: no multiple of 64
    sensor = gpu.make_sensor(p)
    scene = gpu.Scene(sd, sensor=sensor, integrator=gpu.PathIntegrator(max_depth=7))
    assert scene.info()["primitives"] > 64
    return p, scene


def test_hierarchy_scene_uniform_map_matches_constant_route(gpu):
    """k_adjoint_param_tex<false> on a film whose sample count is no multiple of the wavefront: the texel gradients of a uniform grey
    3 x 4 roughness map sum to the derivative with respect to the constant (mtsamd_render_adjoint_param, same h, same paths), 2e-3 as
    test_matches_constant_parameter_route.  max_depth 7 > rr_depth."""
    grey, h = 0.25, 0.01
    p, scene_t = _sphere_scene(gpu, {"type": "bitmap", "data": np.full((3, 4, 3), grey, F32)})
    d, film = _primal(scene_t, p)
    dimage = torch.from_numpy(np.random.RandomState(3).uniform(0.0, 1.0, (19, 25, 3)).astype(F32)).cuda()
    got = float(_grad(scene_t, d, film, dimage, ALPHA, h).double().sum().item())
    p, scene_c = _sphere_scene(gpu, grey)
    d_c, film_c = _primal(scene_c, p)
    want = _constant_route(scene_c, d_c, film_c, dimage, 0, ALPHA, 0, h)
    print("hierarchy: got %.7g want %.7g rel %.3g" % (got, want, abs(got - want) / abs(want)))
    assert abs(want) > 1e-2
    assert abs(got - want) <= 2e-3 * abs(want), (got, want)


# ---- 3. anisotropy ------------------------------------------------------------------------------------------------------------------------
def _box_scene(gpu, mat, w=32, h=24, spp=8, max_depth=7, seed=21):
    """Cornell box whose tall box carries `mat` and random texcoords"""
    from mitsuba2_amd import scenes
    cb = scenes.cornell_box()
    box = dict(cb["meshes"][7], texcoords=np.random.default_rng(4).uniform(0, 1, size=(24, 2)).astype(F32), bsdf=len(cb["bsdfs"]))
    sd = dict(cb, bsdfs=list(cb["bsdfs"]) + [mat], meshes=cb["meshes"][:7] + [box])
    return _scene(gpu, sd, w, h, spp, max_depth, seed=seed)


def test_anisotropic_maps_are_differentiated_one_by_one(gpu):
    """alpha_u and alpha_v read two uniform bitmaps of their own (the same grey, so that the constant route's ALPHA -- both roughnesses
    moved together -- is the reference of their sum).  h / alpha = 0.01: the mixed third derivatives the sum of two partial differences
    misses are of order (h / alpha)^2 = 1e-4 of the derivative, below the 2e-3.  param = -1 runs the same launches as the calls slot by
    slot; the float atomics of a launch add in no fixed order, so the two buffers are compared at 1e-5 of the largest entry, not bit
    for bit."""
    grey, h = 0.3, 0.003
    base = dict(type="roughconductor", distribution="ggx", id="tall", **CONDUCTOR_IOR)
    mat = dict(base, alpha_u={"type": "bitmap", "data": np.full((3, 4, 3), grey, F32)}, alpha_v={"type": "bitmap", "data": np.full((2, 5, 3), grey, F32)})
    p, scene = _box_scene(gpu, mat)
    index = len(scene._bsdf_records) - 1
    tu, tv = scene.texture_index(index, "alpha_u"), scene.texture_index(index, "alpha_v")
    assert tu is not None and tv is not None and tu != tv and scene.texture_index(index, "alpha") is None
    d, film = _primal(scene, p)
    dimage = torch.from_numpy(np.random.RandomState(3).uniform(0.0, 1.0, (24, 32, 3)).astype(F32)).cuda()
    gu, gv = _grad(scene, d, film, dimage, ALPHA_U, h), _grad(scene, d, film, dimage, ALPHA_V, h)
    assert np.abs(_texels(scene, gu, tv)).max() == 0.0 and np.abs(_texels(scene, gv, tu)).max() == 0.0      # each launch writes its own map only
    total_u, total_v = float(_texels(scene, gu, tu).sum()), float(_texels(scene, gv, tv).sum())
    p, scene_c = _box_scene(gpu, dict(base, alpha=grey))
    d_c, film_c = _primal(scene_c, p)
    want = _constant_route(scene_c, d_c, film_c, dimage, index, ALPHA, 0, h)
    print("anisotropy: u %.7g v %.7g sum %.7g want %.7g" % (total_u, total_v, total_u + total_v, want))
    assert total_u != 0.0 and total_v != 0.0 and abs(total_u - total_v) > 1e-3 * max(abs(total_u), abs(total_v))
    assert abs(want) > 1e-2
    assert abs(total_u + total_v - want) <= 2e-3 * abs(want), (total_u, total_v, want)
    both, pair, every = (_grad(scene, d, film, dimage, ALPHA, h), gu + gv, _grad(scene, d, film, dimage, -1, h))
    scale = float(pair.abs().max())
    assert float((both - pair).abs().max()) <= 1e-5 * scale and float((every - pair).abs().max()) <= 1e-5 * scale


# ---- 4. finite differences ----------------------------------------------------------------------------------------------------------------
def test_finite_differences_of_a_specular_colour_map(gpu):
    """A conductor floor (and back wall) with a 6 x 6 specular_reflectance bitmap under an envmap and a point light: the directions do
    not depend on the colour and max_depth 4 <= rr_depth, so with common random numbers (a fixed call counter) the image is a
    polynomial in a texel and central differences of the primal render check the replay through autodiff.render."""
    from mitsuba2_amd import autodiff
    rng = np.random.RandomState(3)
    tex = (0.3 + 0.5 * rng.rand(6, 6, 3)).astype(F32)
    floor = dict(type="conductor", specular_reflectance={"type": "bitmap", "data": tex}, **CONDUCTOR_IOR)
    sd = _open_box(tex, floor, emitters=[_sky(), {"type": "point", "position": [278, 450, 279], "intensity": [2e5, 2e5, 3e5]}])
    p, scene = _scene(gpu, sd, 32, 32, 8, 4, rfilter="gaussian")
    params = autodiff.traverse(scene)
    key = "textured.specular_reflectance.data"
    assert key in params and tuple(params[key].shape) == (6, 6, 3)
    params.keep([key])
    params[key].requires_grad_(True)
    target = torch.from_numpy(np.random.RandomState(4).rand(32 * 32 * 3).astype(F32)).cuda()

    def loss_at():
        autodiff._render_counter[id(scene)] = 7
        img = autodiff.render(scene, params=params)
        return ((img - target) ** 2).sum() / img.numel()

    loss_at().backward()
    g = params[key].grad.clone()
    assert g.shape == (6, 6, 3) and float(g.abs().max()) > 0
    h = 2e-2
    checked = 0
    with torch.no_grad():
        for idx in ((2, 3, 1), (4, 1, 0), (1, 4, 2), (3, 2, 0)):
            base = params[key].detach().clone()
            vp, vm = base.clone(), base.clone()
            vp[idx] += h; vm[idx] -= h
            params[key] = vp; lp = loss_at().item()
            params[key] = vm; lm = loss_at().item()
            params[key] = base
            fd = (lp - lm) / (2 * h)
            got = g[idx].item()
            print("fd texel %s: fd %.6g got %.6g" % (idx, fd, got))
            assert abs(fd - got) <= 3e-2 * max(abs(fd), abs(got)) + 1e-6, (idx, fd, got)
            checked += abs(fd) > 1e-5
    assert checked >= 3


# ---- 5. inversion -------------------------------------------------------------------------------------------------------------------------
def test_invert_a_roughness_map(gpu):
    """invert_cbox.py on the roughness of a roughconductor floor under an envmap: a 4 x 4 map in [0.1, 0.4] approached from a uniform
    0.25 -- the loss at the random numbers of the reference image (zero at the true map, free of Monte Carlo noise) falls below half
    its start"""
    from mitsuba2_amd import autodiff
    yy, xx = np.meshgrid(np.linspace(0, 1, 4, dtype=F32), np.linspace(0, 1, 4, dtype=F32), indexing="ij")
    rough = (0.25 + 0.15 * np.sin(5 * xx + 1) * np.cos(4 * yy)).astype(F32)
    assert rough.min() >= 0.1 and rough.max() <= 0.4
    tex = np.repeat(rough[..., None], 3, axis=2)
    floor = dict(type="roughconductor", distribution="ggx", alpha={"type": "bitmap", "data": tex}, **CONDUCTOR_IOR)
    sd = _open_box(tex, floor, emitters=[_sky(8, 16)])
    p, scene = _scene(gpu, sd, 64, 64, 8, 3, seed=2)
    autodiff._render_counter.pop(id(scene), None)
    params = autodiff.traverse(scene)
    key = "textured.alpha.data"
    params.keep([key])
    ref = params[key].clone()
    image_ref = autodiff.render(scene, spp=64).detach()          # render call 0

    def image_loss():
        call = autodiff._render_counter[id(scene)]
        autodiff._render_counter[id(scene)] = 0
        with torch.no_grad():
            out = float(((autodiff.render(scene, spp=64) - image_ref) ** 2).mean().item())
        autodiff._render_counter[id(scene)] = call
        return out

    params[key] = torch.full_like(ref, 0.25)
    params.update()
    loss0 = image_loss()
    opt = autodiff.Adam(params, lr=0.01)
    for it in range(120):
        image = autodiff.render(scene, optimizer=opt, unbiased=True, spp=8)
        (((image - image_ref) ** 2).sum() / image.numel()).backward()
        opt.step()
    loss1 = image_loss()
    print("inversion: loss %.6g -> %.6g (%.3f)" % (loss0, loss1, loss1 / loss0))
    assert torch.isfinite(params[key]).all()
    assert loss1 < 0.5 * loss0, (loss0, loss1)


# ---- 6. keys and refusals -----------------------------------------------------------------------------------------------------------------
def test_traverse_keys(gpu):
    """the `.data` keys of a scene with every kind of binding; a texture that serves two bindings has none"""
    from mitsuba2_amd import autodiff, scenes
    cb = scenes.cornell_box()
    n = len(cb["bsdfs"])
    shared = {"type": "bitmap", "data": np.full((2, 2, 3), 0.9, F32)}
    mats = [dict(type="roughconductor", id="rough", alpha={"type": "bitmap", "data": np.full((3, 4, 3), 0.2, F32)},
                 specular_reflectance={"type": "bitmap", "data": np.full((2, 3, 3), 0.8, F32)}, **CONDUCTOR_IOR),
            {"type": "twosided", "id": "two", "bsdf": dict(type="roughconductor", distribution="ggx", eta=0.0, k=1.0,
                                                            alpha_u={"type": "bitmap", "data": np.full((2, 5, 3), 0.3, F32)},
                                                            alpha_v={"type": "bitmap", "data": np.full((4, 2, 3), 0.1, F32)})},
            dict(type="roughdielectric", id="frosted", alpha=0.2, specular_transmittance={"type": "bitmap", "data": np.full((5, 2, 3), 0.7, F32)},
                 specular_reflectance={"type": "checkerboard"}),
            dict(type="dielectric", id="glass", specular_reflectance=shared, specular_transmittance=shared)]
    meshes = list(cb["meshes"])
    uv = np.random.default_rng(4).uniform(0, 1, size=(24, 2)).astype(F32)
    meshes[7] = dict(meshes[7], texcoords=uv, bsdf=n)
    meshes[6] = dict(meshes[6], texcoords=uv, bsdf=n + 1)
    for m, b in ((0, n + 2), (2, n + 3)):
        meshes[m] = dict(meshes[m], bsdf=b, texcoords=np.random.default_rng(m).uniform(0, 1, size=(meshes[m]["positions"].shape[0], 2)).astype(F32))
    sd = dict(cb, bsdfs=list(cb["bsdfs"]) + mats, meshes=meshes)
    _, scene = _scene(gpu, sd, 16, 16, 2, 4)
    assert scene.texture_index(n + 3, "specular_reflectance") == scene.texture_index(n + 3, "specular_transmittance")
    params = autodiff.traverse(scene)
    shapes = {k: tuple(v.shape) for k, v in params.items() if k.endswith(".data")}
    assert shapes == {"rough.alpha.data": (3, 4, 3), "rough.specular_reflectance.data": (2, 3, 3), "two.brdf_0.alpha_u.data": (2, 5, 3),
                      "two.brdf_0.alpha_v.data": (4, 2, 3), "frosted.specular_transmittance.data": (5, 2, 3)}
    assert np.allclose(params["two.brdf_0.alpha_v.data"].cpu().numpy(), 0.1)
    # every one of them receives a gradient through autodiff.render, and update() reaches the scene
    for v in params.properties.values():
        v.requires_grad_(v.ndim == 3)
    keys = sorted(shapes)
    autodiff.render(scene, params=params).sum().backward()
    for k in keys:
        assert params[k].grad is not None and params[k].grad.shape == params[k].shape and torch.isfinite(params[k].grad).all(), k
    assert float(params["rough.alpha.data"].grad.abs().max()) > 0
    before = autodiff.render(scene).detach().clone()
    autodiff._render_counter[id(scene)] -= 1
    params["rough.alpha.data"] = torch.full((3, 4, 3), 0.45, device="cuda")
    params.update()
    assert not torch.equal(autodiff.render(scene).detach(), before)


def test_refusals_and_unbound_slots(gpu):
    from mitsuba2_amd import _lib as L, autodiff, scenes
    p, scene = _box_scene(gpu, dict(type="roughconductor", alpha={"type": "bitmap", "data": np.full((2, 2, 3), 0.2, F32)}, **CONDUCTOR_IOR), max_depth=3)
    d, film = _primal(scene, p)
    dimage = torch.ones((24, 32, 3), device="cuda")
    g = torch.zeros(_tex_floats(scene), device="cuda")

    def refused(scene_, d_, param, match):
        rc = _call(scene_, d_, film, dimage, param, 0.01, g)
        assert rc < 0 and match in L.lib().mtsamd_last_error(), (rc, L.lib().mtsamd_last_error())

    # a slot that no record binds: success, nothing written (zeros stay zeros, and a buffer of sevens stays what it was)
    for param in (SPEC, TRANS):
        assert _call(scene, d, film, dimage, param, 0.01, g) == 0
        torch.cuda.synchronize()
        assert float(g.abs().max()) == 0.0
    sevens = torch.full_like(g, 7.0)
    assert _call(scene, d, film, dimage, ALPHA_V, 0.01, sevens) == 0       # a textured `alpha` is differentiated by the alpha_u launch
    torch.cuda.synchronize()
    assert bool((sevens == 7.0).all())
    assert _call(scene, d, film, dimage, -1, 0.01, g) == 0
    torch.cuda.synchronize()
    assert float(g.abs().max()) > 0.0
    g.zero_()
    refused(scene, d, ETA, b"cannot hold a differentiable texture")
    refused(scene, d, 3, b"cannot hold a differentiable texture")
    d.max_depth = -1
    refused(scene, d, ALPHA, b"max_depth <= 16")
    d.max_depth = 17
    refused(scene, d, ALPHA, b"max_depth <= 16")
    d.max_depth = 3
    blend = {"type": "blendbsdf", "weight": 0.3, "bsdf_1": {"type": "diffuse", "reflectance": [0.2, 0.5, 0.7]},
             "bsdf_0": dict(type="roughconductor", alpha={"type": "bitmap", "data": np.full((2, 2, 3), 0.2, F32)}, **CONDUCTOR_IOR)}
    p_b, scene_b = _box_scene(gpu, blend, max_depth=3)
    refused(scene_b, autodiff._desc(scene_b, scene_b.sensors()[0], scene_b.integrator(), None, p_b["seed"]), ALPHA, b"blendbsdf / mask")
    p_s, scene_s = _scene(gpu, scenes.cornell_box(), 32, 24, 8, 3, variant="spectral")
    refused(scene_s, autodiff._desc(scene_s, scene_s.sensors()[0], scene_s.integrator(), None, p_s["seed"]), ALPHA, b"RGB variant only")
    assert float(g.abs().max()) == 0.0                                      # no refused call wrote anything

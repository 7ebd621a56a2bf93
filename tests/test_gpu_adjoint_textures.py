"""Texel gradients in general RGB scenes (mtsamd_render_adjoint_textures, k_adjoint_tex): plastic / roughplastic / conductor BSDFs,
envmap and point lights.  Checked against the diffuse-only replay (mtsamd_render_adjoint) on diffuse scenes, against the constant-
parameter route (mtsamd_render_adjoint_param) on a uniform grey bitmap, against finite differences at common random numbers, and by a
small inversion in the style of invert_cbox.py."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from mitsuba2_amd import scenes

pytestmark = pytest.mark.gpu

NAMES = ["white", "red", "green", "light", "textured"]


def _sky(h=6, w=10, seed=7):
    img = np.random.RandomState(seed).uniform(0.3, 1.2, size=(h, w, 3)).astype(np.float32)
    return {"type": "envmap", "id": "sky", "data": img, "scale": 0.8, "to_world": scenes.look_at([0, 0, 0], [1, 0.2, 0.3], [0, 1, 0])}


def _open_box(tex, textured_bsdf=None, emitters=()):
    """Cornell box without its ceiling and area light (meshes 1 and 5): `tex` on the floor and the back wall (BSDF 4, replaced by
    `textured_bsdf` if given), a conductor on the tall box, lit by `emitters`"""
    sd = scenes.cornell_box(texture=tex)
    for b, n in zip(sd["bsdfs"], NAMES):
        b["id"] = n
    if textured_bsdf is not None:
        sd["bsdfs"][4] = dict(textured_bsdf, id="textured")
    sd["bsdfs"] = list(sd["bsdfs"]) + [{"type": "conductor", "id": "metal", "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14]}]
    sd["meshes"][7] = dict(sd["meshes"][7], bsdf=len(sd["bsdfs"]) - 1)
    sd["meshes"] = [m for i, m in enumerate(sd["meshes"]) if i not in (1, 5)]
    sd["emitters"] = list(emitters)
    return sd


def _scene(gpu, sd, w, h, spp, max_depth, seed=5, rfilter="box", variant="rgb"):
    p = scenes.cornell_box_sensor(w, h, spp, seed=seed, max_depth=max_depth, rfilter=rfilter)
    sensor = gpu.make_sensor(p)
    scene = gpu.Scene(sd, variant=variant, sensor=sensor, integrator=gpu.PathIntegrator(max_depth=max_depth))
    return p, scene


def _primal(scene, p):
    from mitsuba2_amd import autodiff
    d = autodiff._desc(scene, scene.sensors()[0], scene.integrator(), None, p["seed"])
    return d, autodiff._render_film(scene, d)


def _tex_floats(scene):
    return max(sum(h * w * 3 for (h, w, _) in scene._texture_shapes), 1)


def _grad_textures(scene, d, film, dimage):
    from mitsuba2_amd import _lib as L
    g = torch.zeros(_tex_floats(scene), device="cuda")
    L.check(L.lib().mtsamd_render_adjoint_textures(scene._handle, C.byref(d), C.c_void_p(dimage.data_ptr()), C.c_void_p(film.data_ptr()),
                                                   C.c_void_p(g.data_ptr()), None))
    torch.cuda.synchronize()
    return g.cpu().numpy()


def _grad_diffuse_route(scene, d, film, dimage):
    from mitsuba2_amd import _lib as L
    g = torch.zeros(_tex_floats(scene), device="cuda")
    L.check(L.lib().mtsamd_render_adjoint(scene._handle, C.byref(d), C.c_void_p(dimage.data_ptr()), C.c_void_p(film.data_ptr()),
                                          None, C.c_void_p(g.data_ptr()), None, None))
    torch.cuda.synchronize()
    return g.cpu().numpy()


def test_traverse_exposes_textured_reflectances_of_general_scenes(gpu):
    """textured diffuse floor + textured plastic + conductor box + envmap: the new keys, shaped (H, W, 3); a spectral copy has none"""
    from mitsuba2_amd import autodiff
    tex = np.full((4, 5, 3), 0.5, np.float32)
    sd = _open_box(tex, emitters=[_sky()])
    sd["bsdfs"].append({"type": "plastic", "id": "shiny", "diffuse_reflectance": {"type": "bitmap", "data": np.full((3, 2, 3), 0.4, np.float32)}})
    sd["bsdfs"].append({"type": "twosided", "id": "wrapped", "bsdf": {"type": "roughplastic", "alpha": 0.2,
                                                                       "diffuse_reflectance": {"type": "bitmap", "data": np.full((2, 2, 3), 0.3, np.float32)}}})
    sd["meshes"][1] = dict(sd["meshes"][1], bsdf=len(sd["bsdfs"]) - 2)         # back wall: textured plastic
    sd["meshes"][-2] = dict(sd["meshes"][-2], bsdf=len(sd["bsdfs"]) - 1)       # short box
    _, scene = _scene(gpu, sd, 16, 16, 4, 4)
    params = autodiff.traverse(scene)
    shapes = {k: tuple(v.shape) for k, v in params.items() if k.endswith(".data")}
    assert shapes == {"textured.reflectance.data": (4, 5, 3), "shiny.diffuse_reflectance.data": (3, 2, 3),
                      "wrapped.brdf_0.diffuse_reflectance.data": (2, 2, 3), "sky.data": (6, 10, 3)}
    assert np.allclose(params["shiny.diffuse_reflectance.data"].cpu().numpy(), 0.4)
    # the constant parameters of general scenes are still there
    assert "white.reflectance.value" in params and "metal.specular_reflectance.value" in params
    sd_s = copy.deepcopy(sd)
    sd_s["bsdfs"][5] = {"type": "conductor", "id": "metal", "eta": 0.5, "k": 3.0}      # the spectral variant needs uniform eta / k
    _, spectral = _scene(gpu, sd_s, 16, 16, 4, 4, variant="spectral")
    assert not any(k.endswith("reflectance.data") for k in autodiff.traverse(spectral).keys())


def _agree(g, ref, what):
    scale = np.abs(ref).max()
    err = np.abs(g - ref)
    assert scale > 1e-3, what
    bad = np.argwhere(err > 1e-4 * scale)
    assert len(bad) == 0, (what, len(bad), err.max() / scale, bad[:8].tolist())


@pytest.mark.parametrize("max_depth", [3, 7])
@pytest.mark.parametrize("twosided", [False, True])
def test_matches_diffuse_replay(gpu, max_depth, twosided):
    """On the textured diffuse Cornell box (a diffuse scene) the general replay reduces to k_adjoint: same paths, same sweep.  Depth 7
    is past rr_depth = 5, so the Russian-roulette term is covered."""
    rng = np.random.RandomState(1)
    tex = (0.3 + 0.5 * rng.rand(4, 5, 3)).astype(np.float32)
    sd = scenes.cornell_box(texture=tex)
    if twosided:
        sd["bsdfs"][4] = {"type": "twosided", "bsdf": sd["bsdfs"][4]}
    p, scene = _scene(gpu, sd, 24, 20, 4, max_depth)
    d, film = _primal(scene, p)
    dimage = torch.from_numpy(np.random.RandomState(2).randn(20, 24, 3).astype(np.float32)).cuda()
    g = _grad_textures(scene, d, film, dimage)
    ref = _grad_diffuse_route(scene, d, film, dimage)
    _agree(g, ref, (max_depth, twosided))


@pytest.mark.parametrize("model", ["plastic", "roughplastic"])
@pytest.mark.parametrize("nonlinear", [False, True])
def test_matches_constant_parameter_route(gpu, model, nonlinear):
    """A uniform grey bitmap (texture mean = the constant, so plastic's sampling weight kr matches): per channel the sum of the texel
    gradients is the gradient of the constant diffuse_reflectance (mtsamd_render_adjoint_param, O(h^2) central difference).
    max_depth 4 <= rr_depth: no Russian roulette."""
    from mitsuba2_amd import _lib as L
    grey = 0.5
    bsdf = {"type": model, "int_ior": 1.6, "nonlinear": nonlinear}
    if model == "roughplastic":
        bsdf.update(alpha=0.25, distribution="ggx")
    tex = np.full((3, 4, 3), grey, np.float32)
    sd_t = _open_box(tex, dict(bsdf, diffuse_reflectance={"type": "bitmap", "data": tex}), emitters=[_sky()])
    sd_c = _open_box(tex, dict(bsdf, diffuse_reflectance=[grey] * 3), emitters=[_sky()])
    dimage = torch.from_numpy(np.random.RandomState(3).uniform(0.0, 1.0, (24, 28, 3)).astype(np.float32)).cuda()
    p, scene_t = _scene(gpu, sd_t, 28, 24, 16, 4, seed=11)
    d, film = _primal(scene_t, p)
    g = _grad_textures(scene_t, d, film, dimage).reshape(-1, 3).sum(0)
    p, scene_c = _scene(gpu, sd_c, 28, 24, 16, 4, seed=11)
    d_c, film_c = _primal(scene_c, p)
    for c in range(3):
        want = torch.zeros(1, device="cuda")
        L.check(L.lib().mtsamd_render_adjoint_param(scene_c._handle, C.byref(d_c), C.c_void_p(dimage.data_ptr()), C.c_void_p(film_c.data_ptr()),
                                                    4, 0, c, 0.0, C.c_void_p(want.data_ptr()), None))
        torch.cuda.synchronize()
        want = float(want.item())
        assert abs(want) > 1e-2
        assert abs(float(g[c]) - want) <= 2e-3 * abs(want), (model, nonlinear, c, float(g[c]), want)


def test_finite_differences_and_autograd(gpu):
    """Textured diffuse floor under an envmap and a point light, a conductor in the room: the sampled directions do not depend on the
    texels and max_depth <= rr_depth, so with common random numbers (a fixed call counter) the image is a polynomial in a texel and
    central differences of the primal render check the replay.  The envmap key kept beside it runs its own replay."""
    from mitsuba2_amd import autodiff
    rng = np.random.RandomState(3)
    tex = (0.3 + 0.5 * rng.rand(6, 6, 3)).astype(np.float32)
    sd = _open_box(tex, emitters=[_sky(), {"type": "point", "position": [278, 450, 279], "intensity": [2e5, 2e5, 3e5]}])
    p, scene = _scene(gpu, sd, 32, 32, 8, 4, rfilter="gaussian")
    params = autodiff.traverse(scene)
    key = "textured.reflectance.data"
    params.keep([key, "sky.data"])
    for v in params.properties.values():
        v.requires_grad_(True)
    target = torch.from_numpy(np.random.RandomState(4).rand(32 * 32 * 3).astype(np.float32)).cuda()

    def loss_at():
        autodiff._render_counter[id(scene)] = 7
        img = autodiff.render(scene, params=params)
        return ((img - target) ** 2).sum() / img.numel()

    loss = loss_at()
    loss.backward()
    g = params[key].grad.clone()
    assert g.shape == (6, 6, 3) and float(g.abs().max()) > 0
    assert float(params["sky.data"].grad.abs().max()) > 0
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
            assert abs(fd - got) <= 3e-2 * max(abs(fd), abs(got)) + 1e-6, (idx, fd, got)
            checked += abs(fd) > 1e-5
    assert checked >= 3
    # unbiased mode and an unbounded depth
    img_u = autodiff.render(scene, params=params, unbiased=True, spp=(4, 2))
    img_u.sum().backward()
    _, deep = _scene(gpu, _open_box(tex, emitters=[_sky()]), 16, 16, 2, -1)
    pd = autodiff.traverse(deep)
    pd.keep([key])
    pd[key].requires_grad_(True)
    with pytest.raises(RuntimeError, match="max_depth <= 16"):
        autodiff.render(deep, params=pd).sum().backward()


def test_invert_roughplastic_texture(gpu):
    """invert_cbox.py on a textured roughplastic floor and back wall under an envmap: a 16 x 16 texture recovered from a uniform grey"""
    from mitsuba2_amd import autodiff
    yy, xx = np.meshgrid(np.linspace(0, 1, 16, dtype=np.float32), np.linspace(0, 1, 16, dtype=np.float32), indexing="ij")
    tex = np.stack([0.5 + 0.35 * np.sin(6 * xx) * np.cos(5 * yy), 0.45 + 0.3 * np.cos(4 * xx + 3 * yy), 0.4 + 0.3 * np.sin(7 * yy)], -1).astype(np.float32)
    sd = _open_box(tex, {"type": "roughplastic", "alpha": 0.2, "distribution": "ggx", "diffuse_reflectance": {"type": "bitmap", "data": tex}},
                   emitters=[_sky(8, 16)])
    p, scene = _scene(gpu, sd, 64, 64, 8, 3, seed=2)
    autodiff._render_counter.pop(id(scene), None)
    params = autodiff.traverse(scene)
    key = "textured.diffuse_reflectance.data"
    params.keep([key])
    ref = params[key].clone()
    image_ref = autodiff.render(scene, spp=64).detach()          # render call 0

    def image_loss():
        """the loss at the random numbers of the reference image: zero at the true texels, free of Monte Carlo noise"""
        call = autodiff._render_counter[id(scene)]
        autodiff._render_counter[id(scene)] = 0
        with torch.no_grad():
            out = float(((autodiff.render(scene, spp=64) - image_ref) ** 2).mean().item())
        autodiff._render_counter[id(scene)] = call
        return out

    params[key] = torch.full_like(ref, 0.5)
    params.update()
    loss0 = image_loss()
    opt = autodiff.Adam(params, lr=0.03)
    errs = [((ref - params[key].detach()) ** 2).mean().item()]
    for it in range(100):
        image = autodiff.render(scene, optimizer=opt, unbiased=True, spp=8)
        (((image - image_ref) ** 2).sum() / image.numel()).backward()
        opt.step()
        errs.append(((ref - params[key].detach()) ** 2).mean().item())
    loss1 = image_loss()
    assert loss1 < 0.3 * loss0, (loss0, loss1)
    assert errs[-1] < 0.5 * errs[0], errs[::10]

"""The adjoint kernels on hierarchy scenes: every one of k_adjoint, k_adjoint_tex, k_adjoint_param and k_adjoint_env has a `<false>`
instantiation (more than 64 primitives: BVH4 walk, the traversal stack of all 256 lanes in dynamic LDS) that the Cornell-box tests of
test_gpu_autodiff.py and test_gpu_adjoint_textures.py never launch.  Here they run on the displaced sphere over a textured ground
quad, at two sizes (tests/test_bvh_depth_cpu.py pins the classes): "shallow", a stack of at most 48 KiB, and "deep", the 261 k-triangle
mesh of the benchmark's config 3 whose stack is far above 64 KiB.  Each kernel is compared with the CPU oracle's restatement of the same
replay on the same scene dictionary and seed; both sides replay bit-identical paths, so only the order of the fp32 additions differs and
the tolerances are those of the flat-path tests of the same kernel, unchanged.

Worst deviations observed on an MI355X, shallow / deep (each test prints its own; run with -s):

    comparison                                              bound                                   shallow     deep
    k_adjoint: radiance, texels, constant reflectances      rtol 2e-2, atol 2e-3 max|oracle|        5.8e-5      3.5e-4    of the bound
                                                            (largest |error| / max|oracle|)         1.0e-6      1.4e-6
    k_adjoint_tex: texels against the oracle                rtol 2e-2, atol 2e-3 max|oracle|        5.6e-5      4.8e-5    of the bound
    k_adjoint_tex against k_adjoint                         1e-4 max|reference| per element         1.6e-7      2.3e-7
    k_adjoint_tex: texel sum against the constant           2e-3 |constant|                         1.2e-6      9.0e-7
    k_adjoint_param against the oracle (all 13 values)      2e-3 |oracle| + 1e-5                    3.3e-7      3.8e-7
    k_adjoint_env: texels                                   rtol 5e-2, atol 2e-2 max|oracle|        2.3e-5      1.8e-5    of the bound
    k_adjoint_env: sum of the texels                        1e-2 sum|oracle|                        1.6e-7      2.1e-7
    autograd against central differences (shallow only)     3e-2 max(|fd|, |gradient|) + 1e-6       3.0e-3 (a texel; the others below 1e-4)

The deep launches ask for well over 64 KiB of dynamic LDS besides the kernels' own static arrays and run as they are.  A library whose
fused walk drops one deferred child of every BVH4 node (hits are missed, nothing else changes) was tried once against the shallow cases:
all eight oracle comparisons fail, by 46 to 80 times the bound for k_adjoint, k_adjoint_tex and k_adjoint_env and by 22 % to 92 % of
the value for k_adjoint_param.  The texel sum and the constant-parameter gradient, both computed on the GPU, stay equal under that
change -- which is why test_texture_adjoint_matches_constant_parameter_route also holds the constant against the oracle.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_bvh_depth_cpu import hierarchy_scene, hierarchy_sensor, hierarchy_texture

pytestmark = pytest.mark.gpu

SIZES = ["shallow", "deep"]
W, H, SPP = 24, 20, 4


def _gpu_scene(gpu, sd, p):
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=p["max_depth"], rr_depth=p["rr_depth"]))
    info = (C.c_uint32 * 6)()
    from mitsuba2_amd import _lib as L
    L.check(L.lib().mtsamd_scene_info(scene._handle, info))
    assert info[0] > 64, "the scene must be a hierarchy scene: %d primitives" % info[0]      # otherwise the <true> kernels would run
    return scene


def _primal(scene, p, spp=None):
    from mitsuba2_amd import autodiff
    d = autodiff._desc(scene, scene.sensors()[0], scene.integrator(), spp, p["seed"])
    return d, autodiff._render_film(scene, d)


def _oracle(oracle, sd, p, size):
    desc = oracle.make_desc(p, analytic=True, film_rgb=True)
    S = oracle.OracleScene(sd, naive=size == "shallow")      # deep: the oracle's own BVH (bit-identical to its brute force, far faster)
    _, film_o = S.render_image(desc)
    return S, desc, film_o


def _check_primal(film, film_o):
    """the primal film against the oracle's, as test_adjoint_matches_oracle has it"""
    f = film.cpu().numpy()
    assert np.allclose(f[..., 4], film_o[..., 4], rtol=1e-5, atol=1e-6)
    relmse = float(np.mean((f[..., :3] - film_o[..., :3]) ** 2 / (film_o[..., :3] ** 2 + 1e-2)))
    assert relmse < 1e-5, relmse


def _worst(got, want, rtol, atol):
    """largest |got - want| / (atol + rtol |want|): np.allclose passes iff this is <= 1"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want))))


def _close(what, got, want, rtol, atol):
    worst = _worst(got, want, rtol, atol)
    rel = float(np.max(np.abs(np.asarray(got, np.float64) - want) / max(float(np.abs(want).max()), 1e-30)))
    print("%s: worst deviation %.3g of the bound (%.3g of max|oracle|)" % (what, worst, rel))
    assert np.allclose(got, want, rtol=rtol, atol=atol), "%s: worst deviation %.3g x the bound, %.3g of max|oracle|" % (what, worst, rel)


def _adjoint(scene, d, film, dimage, n_bsdfs, tex_floats, n_emitters):
    from mitsuba2_amd import _lib as L
    g_bsdf = torch.zeros((n_bsdfs, 3), device="cuda")
    g_tex = torch.zeros(tex_floats, device="cuda")
    g_em = torch.zeros((n_emitters, 3), device="cuda")
    L.check(L.lib().mtsamd_render_adjoint(scene._handle, C.byref(d), C.c_void_p(dimage.data_ptr()), C.c_void_p(film.data_ptr()),
                                          C.c_void_p(g_bsdf.data_ptr()), C.c_void_p(g_tex.data_ptr()), C.c_void_p(g_em.data_ptr()), None))
    torch.cuda.synchronize()
    return g_bsdf.cpu().numpy(), g_tex.cpu().numpy(), g_em.cpu().numpy()


def _adjoint_textures(scene, d, film, dimage, tex_floats):
    from mitsuba2_amd import _lib as L
    g = torch.zeros(tex_floats, device="cuda")
    L.check(L.lib().mtsamd_render_adjoint_textures(scene._handle, C.byref(d), C.c_void_p(dimage.data_ptr()), C.c_void_p(film.data_ptr()),
                                                   C.c_void_p(g.data_ptr()), None))
    torch.cuda.synchronize()
    return g.cpu().numpy()


def _adjoint_param(scene, d, film, dimage, bsdf, kind, comp, step):
    from mitsuba2_amd import _lib as L
    g = torch.zeros(1, device="cuda")
    L.check(L.lib().mtsamd_render_adjoint_param(scene._handle, C.byref(d), C.c_void_p(dimage.data_ptr()), C.c_void_p(film.data_ptr()), bsdf, kind, comp,
                                                step, C.c_void_p(g.data_ptr()), None))
    torch.cuda.synchronize()
    return float(g.item())


@pytest.mark.parametrize("rfilter,max_depth", [("box", 3), ("gaussian", 6)])
@pytest.mark.parametrize("size", SIZES)
def test_adjoint_matches_oracle(gpu, oracle, size, rfilter, max_depth):
    """k_adjoint<false>: constant reflectances, texels and the lamp's radiance.  Depth 6 is past rr_depth = 5."""
    sd, tex = hierarchy_scene(size)
    p = hierarchy_sensor(W, H, SPP, max_depth, rfilter)
    scene = _gpu_scene(gpu, sd, p)
    d, film = _primal(scene, p)
    S, desc, film_o = _oracle(oracle, sd, p, size)
    _check_primal(film, film_o)
    dimage = np.random.RandomState(2).randn(H, W, 3).astype(np.float32)
    gs_o, gt_o, ge_o = S.render_adjoint(desc, dimage, film_o, len(sd["meshes"]), tex.size, n_emitters=len(sd["emitters"]))
    gb, gt, ge = _adjoint(scene, d, film, torch.from_numpy(dimage).cuda(), len(sd["bsdfs"]), tex.size, len(sd["emitters"]))
    assert np.abs(ge_o).min() > 1e-3
    _close("emitter radiance", ge, ge_o, 2e-2, 2e-3 * np.abs(ge_o).max())
    assert np.abs(gt_o).max() > 1e-3
    _close("texels", gt, gt_o, 2e-2, 2e-3 * np.abs(gt_o).max())
    gb_o = np.zeros((len(sd["bsdfs"]), 3), np.float32)      # per-BSDF gradient = sum over the shapes that share it
    for si, m in enumerate(sd["meshes"]):
        gb_o[m["bsdf"]] += gs_o[si]
    assert np.abs(gb_o[0]).max() > 1e-3                      # the sphere
    _close("constant reflectances", gb, gb_o, 2e-2, 2e-3 * np.abs(gb_o).max())
    assert (gb[1] == 0).all()                                # the textured BSDF has no constant-reflectance gradient


def _agree(g, ref, what):
    """test_gpu_adjoint_textures._agree"""
    scale = np.abs(ref).max()
    err = np.abs(g - ref)
    assert scale > 1e-3, what
    print("%s: worst deviation %.3g of max|reference| (bound 1e-4)" % (what, err.max() / scale))
    bad = np.argwhere(err > 1e-4 * scale)
    assert len(bad) == 0, (what, len(bad), err.max() / scale, bad[:8].tolist())


@pytest.mark.parametrize("size", SIZES)
def test_texture_adjoint_matches_oracle_and_diffuse_replay(gpu, oracle, size):
    """k_adjoint_tex<false> on the diffuse scene: the oracle's texel gradient, and k_adjoint<false>'s (same paths, same sweep)"""
    sd, tex = hierarchy_scene(size)
    p = hierarchy_sensor(W, H, SPP, 6)
    scene = _gpu_scene(gpu, sd, p)
    d, film = _primal(scene, p)
    S, desc, film_o = _oracle(oracle, sd, p, size)
    _check_primal(film, film_o)
    dimage = np.random.RandomState(2).randn(H, W, 3).astype(np.float32)
    di = torch.from_numpy(dimage).cuda()
    _, gt_o = S.render_adjoint(desc, dimage, film_o, len(sd["meshes"]), tex.size)
    g = _adjoint_textures(scene, d, film, di, tex.size)
    assert np.abs(gt_o).max() > 1e-3
    _close("texels (k_adjoint_tex)", g, gt_o, 2e-2, 2e-3 * np.abs(gt_o).max())
    _, ref, _ = _adjoint(scene, d, film, di, len(sd["bsdfs"]), tex.size, len(sd["emitters"]))
    _agree(g, ref, "k_adjoint_tex against k_adjoint")


@pytest.mark.parametrize("size", SIZES)
def test_texture_adjoint_matches_constant_parameter_route(gpu, oracle, size):
    """k_adjoint_tex<false> through plastic / roughplastic: a `roughplastic` sphere over a `plastic` ground whose diffuse_reflectance is a
    uniform grey bitmap (texture mean = the constant, so the sampling weight matches).  Per channel the sum of the texel gradients is the
    gradient of the constant (mtsamd_render_adjoint_param, k_adjoint_param<false>), as in test_matches_constant_parameter_route; that
    constant-parameter gradient is itself checked against the oracle here.  max_depth 4 <= rr_depth: no Russian roulette."""
    grey, step = 0.5, 0.005
    sphere = {"type": "roughplastic", "alpha": 0.25, "distribution": "ggx", "int_ior": 1.6, "diffuse_reflectance": [0.6, 0.3, 0.2]}
    plastic = {"type": "plastic", "int_ior": 1.6}
    tex = hierarchy_texture(grey)
    sd_t, _ = hierarchy_scene(size, sphere=sphere, ground=dict(plastic, diffuse_reflectance={"type": "bitmap", "data": tex}), tex=tex)
    sd_c, _ = hierarchy_scene(size, sphere=sphere, ground=dict(plastic, diffuse_reflectance=[grey] * 3), tex=tex)
    p = hierarchy_sensor(W, H, 8, 4, seed=11)
    dimage = np.random.RandomState(3).uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
    di = torch.from_numpy(dimage).cuda()
    scene_t = _gpu_scene(gpu, sd_t, p)
    d, film = _primal(scene_t, p)
    g = _adjoint_textures(scene_t, d, film, di, tex.size).reshape(-1, 3).sum(0)
    scene_c = _gpu_scene(gpu, sd_c, p)
    d_c, film_c = _primal(scene_c, p)
    S, desc, film_o = _oracle(oracle, sd_c, p, size)
    _check_primal(film_c, film_o)
    for c in range(3):
        want = _adjoint_param(scene_c, d_c, film_c, di, 1, 0, c, step)
        assert abs(want) > 1e-2
        print("channel %d: texel sum %.6g, constant %.6g, deviation %.3g (bound 2e-3)" % (c, float(g[c]), want, abs(float(g[c]) - want) / abs(want)))
        assert abs(float(g[c]) - want) <= 2e-3 * abs(want), (size, c, float(g[c]), want, abs(float(g[c]) - want) / abs(want))
        want_o = S.render_adjoint_param(desc, dimage, film_o, [1], 0, c, step)
        print("channel %d: constant %.6g, oracle %.6g, deviation %.3g (bound 2e-3)" % (c, want, want_o, abs(want - want_o) / abs(want_o)))
        assert abs(want - want_o) < 2e-3 * abs(want_o) + 1e-5, (size, c, want, want_o, abs(want - want_o) / abs(want_o))


ROUGH = {"type": "roughconductor", "alpha": 0.3, "distribution": "ggx", "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14], "specular_reflectance": [0.9, 0.8, 0.7]}
PLASTIC = {"type": "plastic", "diffuse_reflectance": [0.2, 0.5, 0.3], "int_ior": 1.6}


@pytest.mark.parametrize("material,params", [(ROUGH, (("alpha", 4, 0.003), ("k", 3, 0.03), ("specular_reflectance", 1, 0.01))),
                                             (PLASTIC, (("diffuse_reflectance", 0, 0.005),))], ids=["roughconductor", "plastic"])
@pytest.mark.parametrize("size", SIZES)
def test_bsdf_parameter_adjoint_matches_oracle(gpu, oracle, size, material, params):
    """k_adjoint_param<false>: the parameters of the sphere's BSDF model, with the kinds and steps of the Cornell-box test of the same
    name in test_gpu_autodiff.py"""
    sd, _ = hierarchy_scene(size, sphere=material)
    p = hierarchy_sensor(W, H, 16, 5, seed=77)
    scene = _gpu_scene(gpu, sd, p)
    d, film = _primal(scene, p)
    S, desc, film_o = _oracle(oracle, sd, p, size)
    _check_primal(film, film_o)
    dimage = np.random.RandomState(4).uniform(-1.0, 1.0, (H, W, 3)).astype(np.float32)
    di = torch.from_numpy(dimage).cuda()
    for name, kind, step in params:
        for comp in range(1 if kind == 4 else 3):
            got = _adjoint_param(scene, d, film, di, 0, kind, comp, step)
            want = S.render_adjoint_param(desc, dimage, film_o, [0], kind, comp, step)
            assert abs(want) > 1e-3, (name, comp, want)
            print("%s[%d]: %.6g, oracle %.6g, deviation %.3g (bound 2e-3)" % (name, comp, got, want, abs(got - want) / abs(want)))
            assert abs(got - want) < 2e-3 * abs(want) + 1e-5, (size, name, comp, got, want, abs(got - want) / abs(want))


@pytest.mark.parametrize("with_area,rfilter,max_depth", [(False, "box", 4), (True, "gaussian", 6)])
@pytest.mark.parametrize("size", SIZES)
def test_envmap_adjoint_matches_oracle(gpu, oracle, size, with_area, rfilter, max_depth):
    """k_adjoint_env<false>: an 8 x 16 envmap over the scene, alone and beside the area light (emitter selection)"""
    from mitsuba2_amd import _lib as L
    img = np.random.RandomState(7).uniform(0.2, 1.0, size=(8, 16, 3)).astype(np.float32)
    sd, _ = hierarchy_scene(size, envmap=img, area=with_area)
    p = hierarchy_sensor(W, H, 8, max_depth, rfilter, seed=9)
    scene = _gpu_scene(gpu, sd, p)
    d, film = _primal(scene, p)
    S, desc, film_o = _oracle(oracle, sd, p, size)
    _check_primal(film, film_o)
    dimage = np.random.RandomState(2).randn(H, W, 3).astype(np.float32)
    g_o = S.render_adjoint_envmap(desc, dimage, film_o, img.shape)
    g = torch.zeros(img.shape, device="cuda")
    di = torch.from_numpy(dimage).cuda()
    L.check(L.lib().mtsamd_render_adjoint_envmap(scene._handle, C.byref(d), C.c_void_p(di.data_ptr()), C.c_void_p(film.data_ptr()),
                                                 C.c_void_p(g.data_ptr()), None))
    torch.cuda.synchronize()
    g = g.cpu().numpy()
    assert np.abs(g_o).max() > 1e-2
    _close("envmap texels", g, g_o, 5e-2, 2e-2 * np.abs(g_o).max())
    dev = abs(g.sum() - g_o.sum()) / np.abs(g_o).sum()
    print("envmap texels: sum deviates by %.3g of sum|oracle| (bound 1e-2)" % dev)
    assert abs(g.sum() - g_o.sum()) < 1e-2 * np.abs(g_o).sum(), dev


def test_autograd_and_finite_differences_on_a_hierarchy_scene(gpu):
    """The public surface on the shallow scene: traverse() names the parameters, render().backward() fills their gradients, and these
    agree with central differences of the GPU forward render at a fixed seed (steps and acceptance of test_autograd_and_finite_differences)."""
    from mitsuba2_amd import autodiff
    sd, tex = hierarchy_scene("shallow")
    p = hierarchy_sensor(32, 32, 8, 4, "gaussian")
    scene = _gpu_scene(gpu, sd, p)
    params = autodiff.traverse(scene)
    assert set(params.keys()) == {"sphere.reflectance.value", "ground.reflectance.data", "light.reflectance.value", "lamp.emitter.radiance.value"}
    params.keep(["sphere.reflectance.value", "ground.reflectance.data", "lamp.emitter.radiance.value"])
    for k in list(params.keys()):
        params[k].requires_grad_(True)
    target = torch.from_numpy(np.random.RandomState(4).rand(32 * 32 * 3).astype(np.float32)).cuda()

    def loss_at(seed_call):
        autodiff._render_counter[id(scene)] = seed_call          # same random numbers for every evaluation
        img = autodiff.render(scene, params=params)
        return ((img - target) ** 2).sum() / img.numel(), img

    loss, img = loss_at(7)
    assert img.shape == (32 * 32 * 3,) and img.requires_grad
    loss.backward()
    g_sphere = params["sphere.reflectance.value"].grad.clone()
    g_tex = params["ground.reflectance.data"].grad.clone()
    g_lamp = params["lamp.emitter.radiance.value"].grad.clone()
    assert g_tex.shape == tex.shape and g_tex.abs().max() > 0 and g_sphere.abs().max() > 0 and g_lamp.abs().min() > 0
    eps = 2e-2
    with torch.no_grad():
        for key, idx, g in (("sphere.reflectance.value", (0,), g_sphere), ("sphere.reflectance.value", (2,), g_sphere),
                            ("lamp.emitter.radiance.value", (0,), g_lamp), ("lamp.emitter.radiance.value", (2,), g_lamp),
                            ("ground.reflectance.data", (2, 3, 1), g_tex), ("ground.reflectance.data", (1, 1, 0), g_tex)):
            base = params[key].detach().clone()
            vp, vm = base.clone(), base.clone()
            h = 0.5 if "radiance" in key else eps          # the loss is quadratic in the radiance: central differences are exact
            vp[idx] += h; vm[idx] -= h
            params[key] = vp; lp, _ = loss_at(7)
            params[key] = vm; lm, _ = loss_at(7)
            params[key] = base
            fd = (lp.item() - lm.item()) / (2 * h)
            dev = abs(fd - g[idx].item()) / max(abs(fd), abs(g[idx].item()), 1e-30)
            print("%s%s: gradient %.6g, central difference %.6g, deviation %.3g (bound 3e-2)" % (key, idx, g[idx].item(), fd, dev))
            assert abs(fd - g[idx].item()) <= 3e-2 * max(abs(fd), abs(g[idx].item())) + 1e-6, (key, idx, fd, g[idx].item(), dev)

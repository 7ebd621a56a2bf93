"""The emitter family of the spectral path replay (mtsamd_render_adjoint_spectral_emitters: k_adjoint_spectral_emitters +
k_emitter_grad_to_rgb), mtsamd_scene_update_envmap on spectral scenes, and the emitter keys of ``traverse(scene, replay=True)``.

References.  (a) `escaped`: central differences of the ORACLE's spectral render (same seed, analytic filter, film_rgb) of a fresh
OracleScene per perturbed texel, dotted with a fixed random dLoss/dImage in float64.  Every BSDF there is a `conductor`: emitter
sampling is skipped for such BSDFs and consumes no random numbers, so the fresh scene replays the same directions although its sampling
hierarchy differs.  (b) `sampled`: central differences of the GPU's own primal film through update_envmap(rebuild_distribution=False):
unchanged render kernels, and the update is pinned by test_update_equals_a_fresh_scene.  (c) homogeneity: the image is homogeneous of
degree one in the emitters' colours, so sum rgb . grad = dimage . image, an exact reference from the primal film.  (d) the
central-difference route of autodiff (_spectral_gradient, unchanged code) for constant radiances.

Preconditions of a central difference in a colour, asserted on the host for every perturbed colour (`_same_cell`): the maximum stays
strict and in its channel, the normalised colour rgb / (2 max) stays in one cell of the coefficient table, every component stays > 0.

Bound: rtol |fd| + atol max |fd| with rtol = atol = 4 t, t = the worst disagreement of the reference's central differences at H and at
H / 2, |fd_H - fd_H/2| / (|fd_H/2| + max |fd_H/2|) over the components of a case (the rule of tests/test_gpu_adjoint_spectral.py).
MEASURED_T holds t per case: `flat` and `tree` measured on the host with `_oracle_fd`, `sampled` measured on the MI355X with
`_primal_fd` (the sentinel None makes a test fail rather than pass); the scalar identities of (c) use 4 t |reference| with t of `sampled`,
they are there to catch a missing factor, a missing scale term or a wrong maximal channel, all O(1) errors.  Measured: flat 3.660e-4,
tree 2.009e-4, sampled 2.349e-3 (bounds 1.46e-3, 8.04e-4, 9.40e-3).  Observed on the MI355X, worst deviation in units of the bound:
flat 0.160, tree 0.191, sampled 0.244; constants lamp 0.005, point 0.013; homogeneity |lhs - rhs| / |rhs| odd 2.0e-8, stride 8.2e-6,
crop 6.7e-8, deep 4.9e-7 against the 9.40e-3 allowed.  Figures: profiles/r10_adjoint_spectral_emitters.txt.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from mitsuba2_amd import scenes

pytestmark = pytest.mark.gpu

H = 2e-3                      # step of the central differences in the normalised colour; a texel moves by H * sc (sc = 2 max rgb)
MEASURED_T = {"flat": 3.660e-4, "tree": 2.009e-4, "sampled": 2.349e-3}


# ---- colours whose normalised colour sits in the middle of a cell of the res-64 coefficient table ----------------------------------
def _res(gpu):
    return int(np.frombuffer(open(gpu.srgb_coeff_path(), "rb").read()[4:8], np.uint32)[0])


def _centre(gpu, m, xi, yi, peak):
    """strict maximum `peak` in channel m; n = rgb / (2 peak) in the middle of cell (xi, yi) of the table's z = 0.5 plane"""
    res = _res(gpu)
    rgb = np.zeros(3)
    rgb[m], rgb[(m + 1) % 3], rgb[(m + 2) % 3] = peak, (xi + 0.5) / (res - 1) * peak, (yi + 0.5) / (res - 1) * peak
    return rgb.astype(np.float32)


def _cell(gpu, rgb):
    res = _res(gpu)
    rgb = np.asarray(rgb, np.float32)
    n = (rgb / (np.float32(2.0) * rgb.max())).astype(np.float64)
    m = int(np.argmax(rgb))
    return m, min(int(n[(m + 1) % 3] * (res - 1) / 0.5), res - 2), min(int(n[(m + 2) % 3] * (res - 1) / 0.5), res - 2)


def _step(rgb):
    """the step of a colour's central difference: H in its normalised colour"""
    return np.float32(H * 2.0 * float(np.max(rgb)))


def _same_cell(gpu, rgb, h):
    rgb = np.asarray(rgb, np.float32)
    for c in range(3):
        for sgn in (-1.0, 1.0):
            v = rgb.copy()
            v[c] += np.float32(sgn * h)
            assert v.min() > 0.0 and np.sum(v == v.max()) == 1, (rgb.tolist(), c, sgn)
            assert _cell(gpu, v) == _cell(gpu, rgb), (rgb.tolist(), c, sgn, _cell(gpu, v), _cell(gpu, rgb))


def _sky(gpu, seed=3, peak=(0.3, 0.9)):
    """8 x 4 texels, each with a strict maximum in a random channel and in mid-cell"""
    rng = np.random.RandomState(seed)
    img = np.zeros((4, 8, 3), np.float32)
    for i in range(4):
        for j in range(8):
            img[i, j] = _centre(gpu, rng.randint(3), rng.randint(8, 55), rng.randint(8, 55), rng.uniform(*peak))
    return img


ROT = scenes.look_at([0, 0, 0], [1, 0.2, 0.3], [0, 1, 0])


def _env(img, scale=0.7):
    return {"type": "envmap", "id": "my_envmap", "data": img, "scale": scale, "to_world": ROT}


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def _open_box(img, with_area, bsdfs=None, closed=False):
    """the Cornell box without ceiling and back wall (closed: with them; its front is open either way) under the envmap `img`
    (emitter 0), optionally keeping the area light (emitter 1)"""
    cb = scenes.cornell_box()
    keep = [i for i, m in enumerate(cb["meshes"]) if (closed or i not in (1, 2)) and (with_area or m.get("emitter", -1) < 0)]
    cb["meshes"] = [dict(cb["meshes"][i]) for i in keep]
    for b, n in zip(cb["bsdfs"], ["white", "red", "green", "light"]):
        b["id"] = n
    if bsdfs is not None:
        cb["bsdfs"] = bsdfs(cb["bsdfs"])
    cb["emitters"] = [_env(img)] + (list(cb["emitters"]) if with_area else [])
    for m in cb["meshes"]:
        if m.get("emitter", -1) >= 0:
            m["emitter"], m["id"] = 1, "lamp"
    return cb


def _all_conductor(bsdfs):
    return [{"type": "conductor", "id": b["id"], "eta": 0.2 + 0.1 * i, "k": 3.0} for i, b in enumerate(bsdfs)]


def _flat(img):
    return _open_box(img, False, _all_conductor)


def _tree(img):
    """bumpy_sphere(8, 16): more than 64 primitives, a hierarchy scene (k_adjoint_spectral_emitters<false>); all conductor, envmap only"""
    sd = scenes.bumpy_sphere(n_theta=8, n_phi=16)
    sd["meshes"] = [m for m in sd["meshes"] if m.get("emitter", -1) < 0]
    sd["bsdfs"] = [{"type": "conductor", "id": n, "eta": eta, "k": 3.0} for n, eta in (("ball", 0.2), ("ground", 0.4))]
    sd["emitters"] = [_env(img, scale=1.0)]
    return sd


def _lit_block(img, closed=False):
    """a diffuse floor and walls, a roughplastic short block, the envmap plus the area light: emitter samples on two emitters"""
    def bsdfs(b):
        return list(b) + [{"type": "roughplastic", "id": "block", "alpha": 0.25, "distribution": "ggx", "int_ior": 1.6,
                           "diffuse_reflectance": [0.5, 0.35, 0.3]}]
    cb = _open_box(img, True, bsdfs, closed)
    cb["meshes"][-2]["bsdf"] = len(cb["bsdfs"]) - 1
    return cb


CASES = {
    # name: (scene builder, sensor parameters, checked texels)
    "flat": (_flat, lambda: scenes.cornell_box_sensor(20, 16, 16, seed=3, max_depth=3, rfilter="box"), [(1, 5), (2, 5), (1, 4), (2, 2)]),
    "tree": (_tree, lambda: dict(scenes.bumpy_sphere_sensor(24, 16, 8, seed=4, max_depth=4)), [(1, 5), (2, 4), (1, 2), (0, 1)]),
    "sampled": (_lit_block, lambda: scenes.cornell_box_sensor(24, 20, 16, seed=5, max_depth=6, rr_depth=2, rfilter="box"), [(0, 2), (1, 6), (2, 1), (3, 5)]),
}


def _dimage(p, seed=7):
    return np.random.RandomState(seed).randn(p["height"] * p["width"] * 3)


def _perturbed(img, checked, h_of):
    """(texel, channel, map+, map-) for the checked components"""
    for (i, j) in checked:
        for c in range(3):
            tp, tm = img.copy(), img.copy()
            h = h_of(img[i, j])
            tp[i, j, c] += h; tm[i, j, c] -= h
            yield (i, j, c), tp, tm


def _oracle_fd(gpu, oracle, name, scale, seed):
    """reference (a): central differences of the oracle's render, one fresh OracleScene per perturbed map; step `scale` * _step(texel)"""
    build, sensor, checked = CASES[name]
    img, p = _sky(gpu), sensor()
    desc = oracle.make_desc(dict(p, seed=seed), analytic=True, film_rgb=True)
    di = _dimage(p)

    def image(data):
        return oracle.OracleScene(build(np.asarray(data, np.float32)), naive=True, spectral_path=gpu.srgb_coeff_path()).render_image(desc)[0].reshape(-1).astype(np.float64)

    return np.array([float(di @ (image(tp) - image(tm))) / (float(tp[idx]) - float(tm[idx]))
                     for idx, tp, tm in _perturbed(img, checked, lambda rgb: np.float32(scale) * _step(rgb))])


def _primal_fd(scene, d, img, checked, dimage, scale):
    """reference (b): central differences of the GPU's primal film; the sampling hierarchy stays that of `img`"""
    from mitsuba2_amd import autodiff
    di = dimage.double()
    fd = []
    try:
        for idx, tp, tm in _perturbed(img, checked, lambda rgb: np.float32(scale) * _step(rgb)):
            images = []
            for data in (tp, tm):
                scene.update_envmap(data, rebuild_distribution=False)
                images.append(autodiff._image_of(autodiff._render_film(scene, d)).double())
            fd.append(float(torch.dot(di, images[0] - images[1])) / (float(tp[idx]) - float(tm[idx])))
    finally:
        scene.update_envmap(img, rebuild_distribution=False)
    return np.array(fd)


@pytest.fixture(autouse=True)
def _own_render_counters():
    """autodiff keeps a per-scene call counter under id(scene); the tests below pin it, and drop what they added when they end"""
    from mitsuba2_amd import autodiff
    before = set(autodiff._render_counter)
    yield
    for k in set(autodiff._render_counter) - before:
        autodiff._render_counter.pop(k, None)


def _scene(gpu, sd, p):
    sensor = gpu.make_sensor(p)
    return sensor, gpu.Scene(sd, variant="spectral", sensor=sensor, integrator=gpu.PathIntegrator(max_depth=p["max_depth"], rr_depth=p["rr_depth"]))


def _replay(scene, d, dimage, want_em=True, want_env=True):
    """one mtsamd_render_adjoint_spectral_emitters call -> (primal film, grad_emitters (n, 3), grad_envmap (h, w, 3) or None), float64"""
    from mitsuba2_amd import _lib as L, autodiff
    film = autodiff._render_film(scene, d)
    ems = scene._dict["emitters"]
    g_em = torch.zeros((len(ems), 3), device="cuda")
    env = next((e for e in ems if e.get("type", "area") == "envmap"), None)
    g_env = torch.zeros(np.asarray(env["data"]).shape, device="cuda") if env is not None and want_env else None
    L.check(L.lib().mtsamd_render_adjoint_spectral_emitters(scene._handle, C.byref(d), C.c_void_p(dimage.data_ptr()), C.c_void_p(film.data_ptr()),
                                                            C.c_void_p(g_em.data_ptr()) if want_em else None,
                                                            C.c_void_p(g_env.data_ptr()) if g_env is not None else None, None))
    torch.cuda.synchronize()
    return film, g_em.cpu().numpy().astype(np.float64), (g_env.cpu().numpy().astype(np.float64) if g_env is not None else None)


def _check(name, got, fd, t, floor=1e-3):
    print(name, "worst deviation relative to |fd| + max |fd|: %.3e" % float(np.max(np.abs(got - fd) / (np.abs(fd) + np.abs(fd).max()))), "got", got.tolist(), "fd", fd.tolist())
    assert t is not None, "the H-versus-H/2 disagreement of this case has not been measured"
    tol = 4.0 * t
    bound = tol * np.abs(fd) + tol * np.abs(fd).max()
    print(name, "worst deviation in units of the bound: %.3f" % float(np.max(np.abs(got - fd) / bound)))
    assert np.abs(fd).max() > floor
    assert np.all(np.abs(got - fd) <= bound), (name, (np.abs(got - fd) / bound).tolist())


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_area", [False, True])
def test_update_equals_a_fresh_scene(gpu, with_area):
    from mitsuba2_amd import autodiff
    old, new = _sky(gpu, 3), _sky(gpu, 12, peak=(0.2, 2.5))
    new[1, 2] = 0.0                                                # a black texel: sentinel coefficients
    p = scenes.cornell_box_sensor(24, 20, 8, seed=2, max_depth=5, rfilter="box")
    sensor, scene = _scene(gpu, _open_box(old.copy(), with_area), p)
    _, fresh = _scene(gpu, _open_box(new.copy(), with_area), p)
    d = autodiff._desc(scene, sensor, scene.integrator(), None, 2)
    film0 = autodiff._render_film(scene, d)
    scene.update_envmap(old, rebuild_distribution=False)           # the texels make the round trip, the hierarchy stays
    assert torch.equal(autodiff._render_film(scene, d), film0)
    scene.update_envmap(torch.from_numpy(new).cuda())
    film1 = autodiff._render_film(scene, d)
    assert torch.equal(film1, autodiff._render_film(fresh, d)) and not torch.equal(film1, film0)
    assert np.array_equal(scene._dict["emitters"][0]["data"], new)          # the description follows the device


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["flat", "tree"])
def test_escaped_rays_against_oracle_differences(gpu, oracle, name):
    """open Cornell box (flat scene, k_adjoint_spectral_emitters<true>) and the displaced sphere (hierarchy, <false>), all conductor:
    the texel gradients of one replay against the oracle's central differences"""
    from mitsuba2_amd import autodiff
    build, sensor_params, checked = CASES[name]
    img, p = _sky(gpu), sensor_params()
    for (i, j) in checked:
        _same_cell(gpu, img[i, j], _step(img[i, j]))
    sensor, scene = _scene(gpu, build(img.copy()), p)
    d = autodiff._desc(scene, sensor, scene.integrator(), None, sensor.sampler().seed_value())
    dimage = torch.from_numpy(_dimage(p).astype(np.float32)).cuda()
    _, g_em, g_env = _replay(scene, d, dimage)
    got = np.array([g_env[i, j, c] for (i, j) in checked for c in range(3)])
    fd = _oracle_fd(gpu, oracle, name, 1.0, sensor.sampler().seed_value())
    _check(name, got, fd, MEASURED_T[name])
    assert np.isfinite(g_env).all() and not g_em.any()              # the envmap emitter's own row stays untouched


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------
def test_emitter_samples_against_primal_differences(gpu):
    """diffuse floor, roughplastic block, envmap + area light (two emitters: the r2 factor), roulette from the second vertex on"""
    from mitsuba2_amd import autodiff
    build, sensor_params, checked = CASES["sampled"]
    img, p = _sky(gpu), sensor_params()
    for (i, j) in checked:
        _same_cell(gpu, img[i, j], _step(img[i, j]))
    sensor, scene = _scene(gpu, build(img.copy()), p)
    d = autodiff._desc(scene, sensor, scene.integrator(), None, sensor.sampler().seed_value())
    dimage = torch.from_numpy(_dimage(p).astype(np.float32)).cuda()
    _, _, g_env = _replay(scene, d, dimage, want_em=False)
    got = np.array([g_env[i, j, c] for (i, j) in checked for c in range(3)])
    fd, fd_half = (_primal_fd(scene, d, img, checked, dimage, s) for s in (1.0, 0.5))
    print("sampled: H-versus-H/2 disagreement t = %.3e" % float(np.max(np.abs(fd - fd_half) / (np.abs(fd_half) + np.abs(fd_half).max()))))
    _check("sampled", got, fd, MEASURED_T["sampled"])


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------
EDGES = {           # those of tests/test_gpu_adjoint_spectral.py
    "odd": dict(width=19, height=13, spp=3, max_depth=4),
    "stride": dict(width=64, height=64, spp=129, max_depth=4),
    "crop": dict(width=40, height=32, spp=4, max_depth=4, crop=(7, 5, 21, 14)),
    "deep": dict(width=16, height=12, spp=8, max_depth=16),
}


def _special_sky(gpu):
    img = _sky(gpu, 5, peak=(0.3, 1.4))
    img[1, 3] = 0.4                  # grey: a tie of all three channels
    img[2, 5] = 0.0                  # black: no gradient
    img[1, 6] = [0.7, 0.7, 0.2]      # a tie of two
    img[0, 2] = [2.5, 1.1, 3.75]     # > 1
    return img


@pytest.mark.parametrize("edge", list(EDGES))
def test_homogeneity_at_the_launch_edges(gpu, edge):
    """sum_texels rgb . g_env + sum_emitters radiance . g_em = dimage . image, the sums in float64 on the host"""
    from mitsuba2_amd import autodiff
    e = EDGES[edge]
    img = _special_sky(gpu)
    sd = _lit_block(img.copy(), closed=edge == "deep")       # deep: only the front is open, so that paths live long
    p = scenes.cornell_box_sensor(e["width"], e["height"], e["spp"], seed=5, max_depth=e["max_depth"], rr_depth=17 if edge == "deep" else 2, rfilter="box")
    if "crop" in e:
        p["crop"] = e["crop"]
    sensor, scene = _scene(gpu, sd, p)
    d = autodiff._desc(scene, sensor, scene.integrator(), None, 5)
    if edge == "deep":       # some path does reach the 16th vertex: cutting the paths one vertex earlier changes the film
        _, shallow = _scene(gpu, sd, dict(p, max_depth=15))
        assert not torch.equal(autodiff._render_film(scene, d), autodiff._render_film(shallow, autodiff._desc(shallow, sensor, shallow.integrator(), None, 5)))
    cw, ch = p["crop"][2], p["crop"][3]
    dimage = torch.from_numpy(np.random.RandomState(8).uniform(0.0, 1.0, ch * cw * 3).astype(np.float32)).cuda()
    film, g_em, g_env = _replay(scene, d, dimage)
    assert np.isfinite(g_env).all() and np.isfinite(g_em).all()
    assert not g_env[2, 5].any() and np.abs(g_env[1, 3]).max() > 0 and np.abs(g_env[0, 2]).max() > 0
    rhs = float(torch.dot(dimage.double(), autodiff._image_of(film).double()))
    radiance = np.asarray(sd["emitters"][1]["radiance"], np.float64)
    lhs = float((img.astype(np.float64) * g_env).sum() + radiance @ g_em[1])
    print(edge, "lhs", lhs, "rhs", rhs, "relative deviation: %.3e" % (abs(lhs - rhs) / abs(rhs)), "share of the lamp: %.3f" % (radiance @ g_em[1] / rhs))
    assert MEASURED_T["sampled"] is not None
    assert rhs > 1.0 and abs(radiance @ g_em[1]) > 1e-3 * rhs
    assert abs(lhs - rhs) <= 4.0 * MEASURED_T["sampled"] * abs(rhs), (lhs, rhs)
    # a gradient nobody asked for is not computed, and does not change the other
    _, g_em2, none = _replay(scene, d, dimage, want_env=False)
    assert none is None and np.allclose(g_em2, g_em, rtol=1e-4, atol=0)


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lamp", "point"])
def test_constant_radiances_against_the_central_difference_route(gpu, monkeypatch, kind):
    """'lamp.emitter.radiance.value' of the (diffuse) Cornell box through traverse(scene, replay=True) and through the default
    traverse(scene); a `point` intensity next to the lamp: the default map has no key for a shapeless emitter, so its central differences
    are taken by the same unchanged function, _spectral_gradient, called on the replay map.  Same fd_step, same pinned call counter."""
    from mitsuba2_amd import autodiff, _lib as L
    sd = scenes.cornell_box()
    sd["meshes"][5]["id"] = "lamp"
    sd["emitters"][0] = dict(sd["emitters"][0], radiance=_centre(gpu, 0, 40, 21, 18.0))
    key, index = "lamp.emitter.radiance.value", 0
    if kind == "point":
        sd["emitters"] = list(sd["emitters"]) + [{"type": "point", "id": "bulb", "position": [278, 300, 150], "intensity": _centre(gpu, 2, 30, 44, 3e5)}]
        key, index = "bulb.intensity.value", 1
    value = np.asarray(sd["emitters"][index]["radiance" if kind == "lamp" else "intensity"], np.float32)
    _same_cell(gpu, value, _step(value))
    p = scenes.cornell_box_sensor(24, 20, 8, seed=5, max_depth=5, rr_depth=2, rfilter="box")
    sensor, scene = _scene(gpu, sd, p)
    dimage = torch.from_numpy(_dimage(p, 8).astype(np.float32)).cuda()
    params = autodiff.traverse(scene, replay=True)
    assert key in params and np.array_equal(params[key].cpu().numpy(), value)
    params.keep([key])
    params.fd_step = float(_step(value))
    params[key].requires_grad_(True)
    autodiff._render_counter[id(scene)] = 0
    renders = []
    render_film = autodiff._render_film
    with monkeypatch.context() as m:
        m.setattr(autodiff, "_render_film", lambda *a: (renders.append(1), render_film(*a))[1])
        (autodiff.render(scene, params=params) * dimage).sum().backward()
    assert len(renders) == 1                                      # the replay route makes exactly one primal render
    got = params[key].grad.cpu().numpy().astype(np.float64)
    if kind == "lamp":
        plain = autodiff.traverse(scene)
        plain.keep([key])
        plain.fd_step = params.fd_step
        plain[key].requires_grad_(True)
        autodiff._render_counter[id(scene)] = 0
        with monkeypatch.context() as m:
            m.setattr(L.lib(), "mtsamd_render_adjoint_spectral_emitters", lambda *a: pytest.fail("the default traverse() must not replay"))
            (autodiff.render(scene, params=plain) * dimage).sum().backward()
        fd = plain[key].grad.cpu().numpy().astype(np.float64)
    else:
        d = autodiff._desc(scene, sensor, scene.integrator(), None, sensor.sampler().seed_value())      # call 0 of autodiff.render
        fd = autodiff._spectral_gradient(scene, d, params, key, dimage).cpu().numpy().astype(np.float64)
    # the reference does not vanish: 1e-3 for a colour of order 1, so 1e-3 / max for a radiance (18) or an intensity (3e5)
    _check(kind, got, fd, MEASURED_T["sampled"], floor=1e-3 / float(value.max()))


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------
def test_envmap_workflow(gpu):
    """traverse(scene, replay=True) -> keep 'my_envmap.data' -> autograd gradient = the direct call; the default map raises; thirty Adam
    steps recover the lighting (docs/examples/10_inverse_rendering/invert_bunny.py on a small scene)"""
    from mitsuba2_amd import autodiff
    yy, xx = np.meshgrid(np.linspace(0, 1, 4, dtype=np.float32), np.linspace(0, 1, 8, dtype=np.float32), indexing="ij")
    truth = np.stack([0.9 + 0.7 * np.sin(5 * xx + 1), 0.8 + 0.6 * np.cos(4 * xx + 3 * yy), 1.0 + 0.7 * np.sin(6 * yy + 2 * xx)], -1).astype(np.float32)
    p = scenes.cornell_box_sensor(32, 32, 16, seed=6, max_depth=4, rfilter="box")
    sensor, scene = _scene(gpu, _open_box(truth.copy(), False), p)
    key = "my_envmap.data"
    # the default map: the key is there, its backward pass raises and names the switch
    plain = autodiff.traverse(scene)
    plain.keep([key])
    plain[key].requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"replay=True"):
        autodiff.render(scene, params=plain).sum().backward()
    # the autograd gradient is the direct call's
    params = autodiff.traverse(scene, replay=True)
    assert key in params and tuple(params[key].shape) == (4, 8, 3)
    params.keep([key])
    params[key].requires_grad_(True)
    dimage = torch.from_numpy(_dimage(p, 9).astype(np.float32)).cuda()
    autodiff._render_counter[id(scene)] = 0
    (autodiff.render(scene, params=params) * dimage).sum().backward()
    d = autodiff._desc(scene, sensor, scene.integrator(), None, sensor.sampler().seed_value())
    _, _, direct = _replay(scene, d, dimage, want_em=False)
    got = params[key].grad.cpu().numpy().astype(np.float64)
    # the same kernel on the same inputs: the two differ by the order of the float32 atomic sums only.  A texel's sum has N <= 16 384 samples
    # x 5 uses terms of either sign; two random orders differ by about 2 sqrt(N) 2^-24 = 3.4e-5 of the largest partial sum: 1e-4 of the
    # largest component is allowed
    print("autograd against the direct call: %.3e of the largest component" % (np.abs(got - direct).max() / np.abs(direct).max()))
    assert np.abs(direct).max() > 1e-3 and np.abs(got - direct).max() <= 1e-4 * np.abs(direct).max()
    # inversion
    autodiff._render_counter[id(scene)] = 0
    with torch.no_grad():
        target = autodiff.render(scene, spp=64).clone()
    params[key] = torch.full((4, 8, 3), 1.0)
    params.update()
    assert np.array_equal(scene._dict["emitters"][0]["data"], np.full((4, 8, 3), 1.0, np.float32))

    def image_loss():
        """the loss at the random numbers of the target image (call 0, 64 spp): zero at the true texels and free of Monte Carlo noise"""
        call = autodiff._render_counter[id(scene)]
        autodiff._render_counter[id(scene)] = 0
        with torch.no_grad():
            out = float(((autodiff.render(scene, spp=64, params=params) - target) ** 2).mean().item())
        autodiff._render_counter[id(scene)] = call
        return out

    autodiff._render_counter[id(scene)] = 1
    first = image_loss()
    opt = autodiff.Adam(params, lr=0.05)
    for it in range(30):
        img = autodiff.render(scene, spp=16, optimizer=opt)
        ((img - target) ** 2).mean().backward()
        opt.step()
    last = image_loss()
    print("inversion", first, last, float(params[key].min()))
    assert last < 0.2 * first, (first, last)
    assert float(params[key].min()) >= 0.0

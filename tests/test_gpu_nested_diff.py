"""Forward and reverse renders in scenes with blendbsdf / mask records (MTSAMD_FORWARD_NESTED / MTSAMD_REVERSE_NESTED; k_forward_nested,
k_reverse_nested; autodiff.render_forward / render(backward="fused") with nested=True).  The oracle's adjoints do not know nested
records, so every check rests on the primal code or on the existing derivative kernels:

 B. reduction: blendbsdf(weight = 0, A, B) and mask(opacity = 1, A) are A -- forward films and reverse gradients against the plain
    kernels on the scene with A, 48 blocks x 3 channels, rtol 2e-2 / atol 2e-3 of the maximum;
 C. child constants against central differences of the primal render, rr_depth > max_depth, 1e-2 |fd| + 1e-5 on block sums;
 D. the weight in a box lit by a point light (no MIS; the expected image is multilinear in the weights): D1 per sample at max_depth 2,
    D2 in expectation at max_depth 3 (|mean d| <= 4 SE(d), SE(d) <= 0.1 |mean forward|), D3 a mask at opacity 1 against the one-sided
    three-point stencil;
 E. the transpose identity <dimage, J t> = <J^T dimage, t>, 2e-3 |g| + 1e-5;
 F. launch edges; G. the Python surface.

Every GPU entry point used here with bit 4 is refused on the parent.  Every check prints its worst deviation in units of its bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from mitsuba2_amd import scenes
from test_bvh_depth_cpu import hierarchy_scene, hierarchy_sensor
from test_gpu_adjoint_textures import _scene, _tex_floats
from test_gpu_autodiff import _assert_close
from test_gpu_forward import PLASTIC, ROUGH, _block_sums, _desc, _forward_film, _image, _primal_film, _vp
from test_gpu_reverse import _dot, _random_dimage, _within

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID, UNSUPPORTED = -1, -5
REFLECTANCE, SPECULAR_REFLECTANCE, ETA, K, ALPHA, SPECULAR_TRANSMITTANCE = range(6)
DETACH, NESTED = 1, 4
LUM = np.array([0.212671, 0.715160, 0.072169])
SCALARS = {"roughconductor": [(SPECULAR_REFLECTANCE, c) for c in range(3)] + [(ETA, c) for c in range(3)] + [(K, c) for c in range(3)] + [(ALPHA, 0)],
           "plastic": [(REFLECTANCE, c) for c in range(3)] + [(SPECULAR_REFLECTANCE, c) for c in range(3)]}


def _n_flat(scene):
    from mitsuba2_amd import bsdfs as B
    return len(B.flatten(scene._bsdf_records))


def _tangent(scene, bsdf=None, emitters=None, tex=None, env=None, h=0.0, flags=0):
    """test_gpu_forward._tangent over the FLATTENED table (the children of nested records follow the top-level records)"""
    from mitsuba2_amd import _lib as L
    td, keep = L.TangentDesc(), []
    if bsdf is not None:
        a = np.zeros((_n_flat(scene), 18), F32)
        for (b, kind, comp), v in bsdf.items():
            a[b, 3 * kind + comp] = v
        keep.append(a)
        td.bsdf_tangents = a.ctypes.data_as(L.f32p)
    if emitters is not None:
        a = np.ascontiguousarray(emitters, F32)
        keep.append(a)
        td.emitter_tangents = a.ctypes.data_as(L.f32p)
    for name, t in (("texture_tangents_dev", tex), ("envmap_tangent_dev", env)):
        if t is not None:
            t = torch.as_tensor(np.ascontiguousarray(t, F32)).cuda().contiguous()
            keep.append(t)
            setattr(td, name, t.data_ptr())
    td.h, td.flags = float(h), int(flags)
    return td, keep


def _reverse(scene, d, dimage, film, wanted=(), emitters=False, tex_floats=0, env_shape=None, h=0.0, flags=0, into=None, expect=0):
    """test_gpu_reverse._reverse over the flattened table"""
    from mitsuba2_amd import _lib as L
    n_bsdf = _n_flat(scene)
    gd = L.GradientDesc()
    buf = dict(into or {})
    mask = np.zeros((n_bsdf, 18), np.uint8)
    if wanted:
        for (b, kind, c) in wanted:
            mask[b, 3 * kind + c] = 1
        buf.setdefault("bsdf", torch.zeros((n_bsdf, 18), device="cuda"))
        gd.bsdf_wanted = mask.ctypes.data_as(C.POINTER(C.c_uint8))
        gd.grad_bsdf_dev = buf["bsdf"].data_ptr()
    if emitters:
        buf.setdefault("emitters", torch.zeros((max(len(scene._dict.get("emitters", [])), 1), 3), device="cuda"))
        gd.grad_emitters_dev = buf["emitters"].data_ptr()
    if tex_floats:
        buf.setdefault("tex", torch.zeros(tex_floats, device="cuda"))
        gd.grad_textures_dev = buf["tex"].data_ptr()
    if env_shape is not None:
        buf.setdefault("env", torch.zeros(tuple(env_shape), device="cuda"))
        gd.grad_envmap_dev = buf["env"].data_ptr()
    gd.h, gd.flags = float(h), int(flags)
    di = dimage if isinstance(dimage, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dimage, F32)).cuda()
    rc = L.lib().mtsamd_render_reverse(scene._handle, C.byref(d), _vp(di), _vp(film), C.byref(gd), None)
    if expect:
        assert rc == expect, (rc, L.lib().mtsamd_last_error())
        return L.lib().mtsamd_last_error().decode()
    L.check(rc)
    torch.cuda.synchronize()
    if into is not None:
        return buf
    return {k: v.cpu().numpy().astype(np.float64) for k, v in buf.items()}


def _tex_info(scene, idx):
    from mitsuba2_amd import _lib as L
    off, w, h = C.c_uint64(), C.c_int32(), C.c_int32()
    L.check(L.lib().mtsamd_scene_texture_info(scene._handle, int(idx), C.byref(w), C.byref(h), C.byref(off)))
    return off.value, w.value, h.value


def _samples(scene, d, n, td=None):
    """per-sample (n, 4): the radiance of mtsamd_sample_radiance, or the derivative of mtsamd_sample_forward"""
    from mitsuba2_amd import _lib as L
    out = torch.zeros((n, 4), device="cuda")
    if td is None:
        L.check(L.lib().mtsamd_sample_radiance(scene._handle, C.byref(d), 0, n, _vp(out), None, None))
    else:
        L.check(L.lib().mtsamd_sample_forward(scene._handle, C.byref(d), C.byref(td[0]), 0, n, _vp(out), None, None))
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64)


TEX_A = np.random.RandomState(3).uniform(0.2, 0.8, (3, 4, 3)).astype(F32)
MODELS = {"roughconductor": ROUGH, "plastic": PLASTIC, "textured": {"type": "diffuse", "reflectance": {"type": "bitmap", "data": TEX_A}}}
OTHER = {"type": "diffuse", "reflectance": [0.2, 0.6, 0.4]}


def _box_with(gpu, mat, max_depth=7, rr_depth=None, w=32, h=24, spp=8, seed=21, hierarchy=False, **fields):
    """The Cornell box whose tall box carries `mat` (random texcoords on it), 32 x 24 x 8 spp; or the 70-triangle sphere scene with `mat` on
    the sphere, 25 x 19 x 3 spp.  Returns (scene, desc, index of mat's record)."""
    if hierarchy:
        sd, _ = hierarchy_scene("shallow", sphere=mat, area=True)
        n_uv = len(np.asarray(sd["meshes"][0]["positions"]).reshape(-1, 3))
        sd["meshes"][0]["texcoords"] = np.random.default_rng(4).uniform(0, 1, size=(n_uv, 2)).astype(F32)
        p = hierarchy_sensor(25, 19, 3, max_depth, seed=seed)
        scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=max_depth))
        top = 0
    else:
        cb = scenes.cornell_box()
        box = dict(cb["meshes"][7], texcoords=np.random.default_rng(4).uniform(0, 1, size=(24, 2)).astype(F32), bsdf=len(cb["bsdfs"]))
        sd = dict(cb, bsdfs=list(cb["bsdfs"]) + [mat], meshes=cb["meshes"][:7] + [box])
        p, scene = _scene(gpu, sd, w, h, spp, max_depth, seed=seed)
        top = len(sd["bsdfs"]) - 1
    if rr_depth is not None:
        fields["rr_depth"] = rr_depth
    return scene, _desc(scene, p, **fields), top


def _child(scene, top, k=0):
    from mitsuba2_amd import bsdfs as B
    B.flatten(scene._bsdf_records)
    return scene._bsdf_records[top]["nested"][k]


# ---- B. reduction to the plain scene ---------------------------------------------------------------------------------------------------------
REDUCTIONS = [("blend", "roughconductor", False, False), ("mask", "roughconductor", False, False), ("blend", "plastic", False, False),
              ("mask", "plastic", False, False), ("blend", "textured", False, False), ("mask", "textured", False, False),
              ("blend", "roughconductor", True, False), ("mask", "plastic", False, True)]


@pytest.mark.parametrize("nest,model,twosided,hierarchy", REDUCTIONS, ids=["%s-%s%s%s" % (n, m, "-twosided" if t else "", "-hierarchy" if hh else "") for n, m, t, hh in REDUCTIONS])
def test_a_nest_that_is_its_child_gives_the_plain_scene(gpu, nest, model, twosided, hierarchy):
    """blendbsdf(weight 0, A, B) and mask(opacity 1, A) sample and evaluate exactly as A does: forward films of one-hot tangents on each of
    A's scalars (a random texel tangent for the textured diffuse) and the reverse gradients of all of them, against the NEST = false kernels
    on the scene with plain A.  Attached roulette, rr_depth 2."""
    A = MODELS[model]
    mat = {"type": "blendbsdf", "weight": 0.0, "bsdf_0": A, "bsdf_1": OTHER} if nest == "blend" else {"type": "mask", "opacity": 1.0, "nested": A}
    plain = A
    if twosided:
        mat, plain = {"type": "twosided", "bsdf": mat}, {"type": "twosided", "bsdf": A}
    mine, dm, top = _box_with(gpu, mat, rr_depth=2, hierarchy=hierarchy)
    theirs, dt, top_t = _box_with(gpu, plain, rr_depth=2, hierarchy=hierarchy)
    child = _child(mine, top)
    film_m, film_t = _primal_film(mine, dm), _primal_film(theirs, dt)
    assert np.allclose(film_m.cpu().numpy(), film_t.cpu().numpy(), rtol=2e-5, atol=1e-6)      # the same render
    H, W = dm.crop_height, dm.crop_width
    dimage = _random_dimage(H, W)
    size = 4 if not hierarchy else 8
    if model == "textured":
        t_m, t_t = mine.texture_index(child), theirs.texture_index(top_t)
        assert t_m is not None and t_t is not None and _tex_floats(mine) == _tex_floats(theirs)
        tt = np.random.RandomState(2).uniform(-1.0, 1.0, _tex_floats(mine)).astype(F32)
        got = _block_sums(_image(_forward_film(mine, dm, _tangent(mine, tex=tt, flags=NESTED))), size)
        want = _block_sums(_image(_forward_film(theirs, dt, _tangent(theirs, tex=tt))), size)
        assert np.abs(want).max() > 1e-3
        _assert_close("%s(%s): forward film of a random texel tangent, %d blocks" % (nest, model, len(want)), got, want)
        g_m = _reverse(mine, dm, dimage, film_m, tex_floats=_tex_floats(mine), flags=NESTED)["tex"]
        g_t = _reverse(theirs, dt, dimage, film_t, tex_floats=_tex_floats(theirs))["tex"]
        assert np.abs(g_t).max() > 1e-3
        _assert_close("%s(%s): reverse texel gradients" % (nest, model), g_m, g_t)
        return
    worst = 0.0
    for (kind, comp) in SCALARS[model]:
        got = _block_sums(_image(_forward_film(mine, dm, _tangent(mine, bsdf={(child, kind, comp): 1.0}, flags=NESTED))), size)
        want = _block_sums(_image(_forward_film(theirs, dt, _tangent(theirs, bsdf={(top_t, kind, comp): 1.0}))), size)
        assert np.abs(want).max() > 1e-4, (kind, comp)
        worst = max(worst, float(np.max(np.abs(got - want) / (2e-3 * np.abs(want).max() + 2e-2 * np.abs(want)))))
        assert np.allclose(got, want, rtol=2e-2, atol=2e-3 * np.abs(want).max()), (nest, model, kind, comp)
    print("%s(%s)%s: forward films of %d one-hot tangents, %d blocks: worst deviation %.3g of the bound" % (
        nest, model, " twosided" if twosided else "", len(SCALARS[model]), got.shape[0], worst))
    g_m = _reverse(mine, dm, dimage, film_m, wanted=[(child, k, c) for k, c in SCALARS[model]], flags=NESTED)["bsdf"]
    g_t = _reverse(theirs, dt, dimage, film_t, wanted=[(top_t, k, c) for k, c in SCALARS[model]])["bsdf"]
    _assert_close("%s(%s): reverse gradients of the child's scalars" % (nest, model), g_m[child], g_t[top_t])
    assert not np.delete(g_m, child, 0).any()


# ---- C. child constants against central differences of the primal ----------------------------------------------------------------------------
@pytest.mark.parametrize("nest", ["blend", "mask"])
def test_child_reflectance_against_central_differences_of_the_primal(gpu, nest):
    """A diffuse child's reflectance inside a blend (weight 0.4) and behind a mask (opacity 0.6): with rr_depth > max_depth the image is a
    polynomial in it, so a central difference of the primal film at the same seed is exact to O(h^2)."""
    from mitsuba2_amd import autodiff
    refl = np.array([0.5, 0.3, 0.6])
    A = {"type": "diffuse", "reflectance": refl.tolist()}
    mat = {"type": "blendbsdf", "weight": 0.4, "bsdf_0": ROUGH, "bsdf_1": A} if nest == "blend" else {"type": "mask", "opacity": 0.6, "nested": A}
    scene, d, top = _box_with(gpu, mat, max_depth=7, rr_depth=9)
    child = _child(scene, top, 1 if nest == "blend" else 0)
    t = np.array([1.0, 0.5, -0.75])
    got = _block_sums(_image(_forward_film(scene, d, _tangent(scene, bsdf={(child, REFLECTANCE, c): t[c] for c in range(3)}, flags=NESTED))))
    h, images = 0.02, []
    for sign in (1.0, -1.0):
        scene.set_bsdf_reflectance(child, (refl + sign * h * t).tolist())
        images.append(_block_sums(_image(autodiff._render_film(scene, d).cpu().numpy())))
    scene.set_bsdf_reflectance(child, refl.tolist())
    fd = (images[0] - images[1]) / (2 * h)
    dev = np.abs(got - fd) / (1e-2 * np.abs(fd) + 1e-5)
    print("%s: child reflectance against central differences, %d block sums: worst deviation %.3g of the bound" % (nest, fd.size, float(dev.max())))
    assert np.abs(fd).max() > 1e-3 and (dev < 1).all(), (got[dev >= 1], fd[dev >= 1])


# ---- D. the weight -----------------------------------------------------------------------------------------------------------------------------
def _point_box(gpu, nest, w, max_depth, res=16, spp=512, seed=31):
    """the Cornell box without its lamp, lit by a point light; every surface carries the same nest at weight / opacity w"""
    cb = scenes.cornell_box()
    if nest == "blend":
        mat = {"type": "blendbsdf", "id": "nest", "weight": float(w), "bsdf_0": {"type": "diffuse", "reflectance": [0.05] * 3},
               "bsdf_1": {"type": "diffuse", "reflectance": [0.9] * 3}}
    else:
        mat = {"type": "mask", "id": "nest", "opacity": float(w), "nested": {"type": "diffuse", "reflectance": [0.7, 0.5, 0.8]}}
    sd = dict(bsdfs=[mat], meshes=[dict(m, bsdf=0, emitter=-1) for i, m in enumerate(cb["meshes"]) if i != 5],
              emitters=[{"type": "point", "position": [278, 400, 280], "intensity": [3e5, 2e5, 2.5e5]}])
    p, scene = _scene(gpu, sd, res, res, spp, max_depth, seed=seed)
    return scene, _desc(scene, p, rr_depth=max_depth + 2)


@pytest.mark.parametrize("nest", ["blend", "mask"])
def test_weight_per_sample_at_depth_two(gpu, nest):
    """D1.  max_depth 2: the radiance of each sample is the emitter sample of the first hit, linear in w, and the child choice reaches nothing
    that contributes: mtsamd_sample_forward against (R(w + h) - R(w - h)) / 2h of mtsamd_sample_radiance in fresh scenes, h = 0.25, sample
    by sample within 1e-5 (|R+| + |R-|) / 2h.  No sample is left out."""
    n, h = 16 * 16 * 16, 0.25
    scene, d = _point_box(gpu, nest, 0.5, 2, spp=16)
    fwd = _samples(scene, d, n, _tangent(scene, bsdf={(0, REFLECTANCE, 0): 1.0}, flags=NESTED))[:, :3]
    rp, rm = (_samples(*_point_box(gpu, nest, 0.5 + s * h, 2, spp=16), n)[:, :3] for s in (1.0, -1.0))
    fd = (rp - rm) / (2 * h)
    bound = 1e-5 * (np.abs(rp) + np.abs(rm)) / (2 * h)
    assert (np.abs(fd) > 0).mean() > 0.3
    lit = bound > 0
    print("%s: weight derivative per sample, %d samples (%d lit): worst deviation %.3g of the bound" % (
        nest, n, int(lit.any(1).sum()), float((np.abs(fwd - fd)[lit] / bound[lit]).max())))
    assert (np.abs(fwd - fd) <= bound).all()


def _expectation(what, fwd, fd):
    """the acceptance rule of D2 / D3 on per-sample derivatives (n, 3): for the whole-film sum of each channel |mean d| <= 4 SE(d), and
    SE(d) <= 0.1 |mean forward| so that noise cannot pass it"""
    dd = fwd - fd
    n = dd.shape[0]
    mean_d, se = dd.mean(0), dd.std(0, ddof=1) / np.sqrt(n)
    mean_f = fwd.mean(0)
    print("%s: mean forward %s, mean d %s, SE(d) %s: |mean d| / SE %s, SE / |mean forward| %s" % (
        what, mean_f, mean_d, se, np.abs(mean_d) / se, se / np.abs(mean_f)))
    assert (se <= 0.1 * np.abs(mean_f)).all(), (se, mean_f)
    assert (np.abs(mean_d) <= 4 * se).all(), (mean_d, se)


@pytest.mark.parametrize("nest", ["blend", "mask"])
def test_weight_in_expectation_at_depth_three(gpu, nest):
    """D2.  max_depth 3: the expected image is at most quadratic in w, so the central difference at h = 0.25 is exact in expectation; the
    samples share their random streams with the forward render.  The derivative of the child-selection probability (the s term) is what
    makes the forward render the derivative of the EXPECTED image: without it this test fails."""
    n, h = 16 * 16 * 512, 0.25
    scene, d = _point_box(gpu, nest, 0.5, 3)
    fwd = _samples(scene, d, n, _tangent(scene, bsdf={(0, REFLECTANCE, 0): 1.0}, flags=NESTED))[:, :3]
    rp, rm = (_samples(*_point_box(gpu, nest, 0.5 + s * h, 3), n)[:, :3] for s in (1.0, -1.0))
    _expectation("%s at 0.5, central difference" % nest, fwd, (rp - rm) / (2 * h))


def test_opacity_one_against_the_one_sided_stencil(gpu):
    """D3.  A mask at opacity 1, where an optimisation of the opacity starts: the raw value lies on the closed end of [0, 1], so the tangent
    passes; (3 I(1) - 4 I(1 - h) + I(1 - 2h)) / 2h is exact for quadratics."""
    n, h = 16 * 16 * 512, 0.25
    scene, d = _point_box(gpu, "mask", 1.0, 3)
    fwd = _samples(scene, d, n, _tangent(scene, bsdf={(0, REFLECTANCE, 0): 1.0}, flags=NESTED))[:, :3]
    r0 = _samples(scene, d, n)[:, :3]
    r1, r2 = (_samples(*_point_box(gpu, "mask", 1.0 - k * h, 3), n)[:, :3] for k in (1, 2))
    _expectation("mask at opacity 1, one-sided stencil", fwd, (3 * r0 - 4 * r1 + r2) / (2 * h))


# ---- E. the transpose identity ------------------------------------------------------------------------------------------------------------------
def _identity_box(gpu, which, max_depth=7, weight_map=None, hierarchy=False, envmap=False):
    """The area-lit Cornell box (bitmap on floor and back wall) with one blend wall -- the right wall: roughconductor + textured diffuse,
    weight 0.3 (or the bitmap `weight_map`) -- or with one masked box (the tall box: a bitmap opacity 8 x 8 over a plastic)"""
    rng = np.random.RandomState(11)
    if which == "blend":
        mat = {"type": "blendbsdf", "id": "nest", "weight": 0.3 if weight_map is None else {"type": "bitmap", "data": weight_map}, "bsdf_0": ROUGH,
               "bsdf_1": {"type": "diffuse", "reflectance": {"type": "bitmap", "data": rng.uniform(0.2, 0.8, (4, 3, 3)).astype(F32)}}}
    else:
        mat = {"type": "mask", "id": "nest", "opacity": {"type": "bitmap", "data": rng.uniform(0.3, 0.9, (8, 8, 3)).astype(F32)}, "nested": PLASTIC}
    if hierarchy:
        return _box_with(gpu, mat, max_depth=max_depth, rr_depth=2, hierarchy=True) + (None,)
    cb = scenes.cornell_box(texture=rng.uniform(0.2, 0.8, (5, 4, 3)).astype(F32))
    meshes = list(cb["meshes"])
    if which == "blend":
        meshes[3] = dict(meshes[3], bsdf=len(cb["bsdfs"]))
    else:
        meshes[7] = dict(meshes[7], texcoords=np.random.default_rng(4).uniform(0, 1, size=(24, 2)).astype(F32), bsdf=len(cb["bsdfs"]))
    sd = dict(cb, bsdfs=list(cb["bsdfs"]) + [mat], meshes=meshes)
    env = None
    if envmap:      # a sky behind the open front of the box: emitter 0; the lamp becomes emitter 1
        env = np.random.RandomState(7).uniform(0.3, 1.2, size=(6, 10, 3)).astype(F32)
        sd["emitters"] = [{"type": "envmap", "id": "sky", "data": env, "scale": 0.8, "to_world": scenes.look_at([0, 0, 0], [1, 0.2, 0.3], [0, 1, 0])}] + list(sd["emitters"])
        sd["meshes"] = [dict(m, emitter=1) if m.get("emitter", -1) >= 0 else m for m in meshes]
    p, scene = _scene(gpu, sd, 32, 24, 8, max_depth, seed=21)
    return scene, _desc(scene, p, rr_depth=2), len(sd["bsdfs"]) - 1, env


def _linear_entries(scene, top):
    """(record, kind, component) of every scalar the image is linear in along a path: colour constants of the plain records, of the children,
    and the weight where it is a constant"""
    from mitsuba2_amd import bsdfs as B
    flat = B.flatten(scene._bsdf_records)
    out = []
    for b, rec in enumerate(flat):
        if rec["type"] in (B.BLEND, B.MASK):
            if not isinstance(rec["reflectance"], dict):
                out.append((b, REFLECTANCE, 0))
        elif rec["type"] in (B.DIFFUSE, B.PLASTIC) and not isinstance(rec["reflectance"], dict):
            out += [(b, REFLECTANCE, c) for c in range(3)]
        if rec["type"] in (B.ROUGHCONDUCTOR, B.PLASTIC):
            out += [(b, SPECULAR_REFLECTANCE, c) for c in range(3)]
    return out


@pytest.mark.parametrize("which", ["blend", "mask"])
@pytest.mark.parametrize("detach", [True, False], ids=["detached", "attached"])
def test_transpose_identity(gpu, which, detach):
    """ONE random tangent over the children's colour constants, the weight, the opacity texels, the child's reflectance texels, the walls'
    texels and the lamp: <dimage, J t> of the forward render against <J^T dimage, t> of the reverse render, rr_depth 2.  alpha, eta and k of
    the roughconductor child are nonlinear: one-hot, so both sides take the same step.  The weight alone, one-hot, as well."""
    scene, d, top, _ = _identity_box(gpu, which)
    film = _primal_film(scene, d)
    dimage = _random_dimage(24, 32)
    flags = NESTED | (DETACH if detach else 0)
    linear = _linear_entries(scene, top)
    nonlinear = [(_child(scene, top, 0), kind, c) for kind, c in SCALARS["roughconductor"] if kind in (ETA, K, ALPHA)] if which == "blend" else []
    n_tex = _tex_floats(scene)
    g = _reverse(scene, d, dimage, film, wanted=linear + nonlinear, emitters=True, tex_floats=n_tex, flags=flags)
    rng = np.random.RandomState(6)
    t_bsdf = {w: float(rng.uniform(0.5, 1.0)) for w in linear}
    t_em = rng.uniform(0.5, 2.0, (len(scene._dict["emitters"]), 3)).astype(F32)
    t_tex = rng.uniform(-1.0, 1.0, n_tex).astype(F32)
    fwd = _dot(_forward_film(scene, d, _tangent(scene, bsdf=t_bsdf, emitters=t_em, tex=t_tex, flags=flags)), dimage)
    parts = {"constants": sum(g["bsdf"][b, 3 * kind + c] * t for (b, kind, c), t in t_bsdf.items()), "lamp": float((g["emitters"] * t_em).sum()),
             "texels": float((g["tex"] * t_tex.astype(np.float64)).sum())}
    print("%s %s: parts of <J^T dimage, t>: %s" % (which, "detached" if detach else "attached", parts))
    assert all(abs(v) > 1e-3 for v in parts.values()), parts
    _within("%s, one random tangent over every family" % which, sum(parts.values()), fwd, floor=1)
    # every texture of the scene received a gradient: the walls', the child's reflectance or the opacity map
    for idx in range(len(scene._texture_shapes)):
        off, w, h = _tex_info(scene, idx)
        assert np.abs(g["tex"][off: off + 3 * w * h]).max() > 1e-4, idx
    if which == "blend":
        got = [g["bsdf"][b, 3 * kind + c] for (b, kind, c) in nonlinear + [(top, REFLECTANCE, 0)]]
        want = [_dot(_forward_film(scene, d, _tangent(scene, bsdf={w: 1.0}, flags=flags)), dimage) for w in nonlinear + [(top, REFLECTANCE, 0)]]
        _within("blend: alpha, eta, k of the child and the weight, one-hot", got, want, floor=4)
    else:       # the opacity map alone, and its channel shares: the opacity is the luminance of the texel
        off, w, h = _tex_info(scene, scene.texture_index(top))
        only = np.zeros(n_tex, F32)
        only[off: off + 3 * w * h] = t_tex[off: off + 3 * w * h]
        _within("mask: the opacity texels alone", float((g["tex"] * only.astype(np.float64)).sum()),
                _dot(_forward_film(scene, d, _tangent(scene, tex=only, flags=flags)), dimage), floor=1)
        ch = g["tex"][off: off + 3 * w * h].reshape(h, w, 3).sum((0, 1))
        assert np.allclose(ch / ch.sum(), LUM, rtol=1e-4), ch / ch.sum()


def test_transpose_identity_on_the_hierarchy_scene(gpu):
    scene, d, top, _ = _identity_box(gpu, "blend", hierarchy=True)
    from mitsuba2_amd import _lib as L
    info = (C.c_uint32 * 6)()
    L.check(L.lib().mtsamd_scene_info(scene._handle, info))
    assert info[0] > 64            # a hierarchy scene: k_forward_nested<false>, k_reverse_nested<false, true>
    film = _primal_film(scene, d)
    dimage = _random_dimage(19, 25)
    linear = _linear_entries(scene, top)
    n_tex = _tex_floats(scene)
    g = _reverse(scene, d, dimage, film, wanted=linear, emitters=True, tex_floats=n_tex, flags=NESTED)
    rng = np.random.RandomState(6)
    t_bsdf = {w: float(rng.uniform(0.5, 1.0)) for w in linear}
    t_em = rng.uniform(0.5, 2.0, (len(scene._dict["emitters"]), 3)).astype(F32)
    t_tex = rng.uniform(-1.0, 1.0, n_tex).astype(F32)
    fwd = _dot(_forward_film(scene, d, _tangent(scene, bsdf=t_bsdf, emitters=t_em, tex=t_tex, flags=NESTED)), dimage)
    rev = sum(g["bsdf"][b, 3 * kind + c] * t for (b, kind, c), t in t_bsdf.items()) + float((g["emitters"] * t_em).sum()) + float((g["tex"] * t_tex.astype(np.float64)).sum())
    _within("hierarchy scene, blend on the sphere: one random tangent", rev, fwd, floor=1)
    w1 = g["bsdf"][top, 0]
    _within("... the weight one-hot", w1, _dot(_forward_film(scene, d, _tangent(scene, bsdf={(top, REFLECTANCE, 0): 1.0}, flags=NESTED)), dimage), floor=1)


def test_emitter_and_envmap_gradients_alone_run_at_any_depth(gpu):
    """RECORD = false: lamp and envmap only, max_depth 20; with a BSDF scalar or a texel wanted the same call is refused by its depth"""
    scene, d, top, env = _identity_box(gpu, "blend", max_depth=20, envmap=True)
    film = _primal_film(scene, d)
    dimage = _random_dimage(24, 32)
    g = _reverse(scene, d, dimage, film, emitters=True, env_shape=env.shape, flags=NESTED)
    rng = np.random.RandomState(9)
    t_em = rng.uniform(0.5, 2.0, (len(scene._dict["emitters"]), 3)).astype(F32)
    t_env = rng.uniform(0.0, 1.0, env.shape).astype(F32)
    fwd_em = _dot(_forward_film(scene, d, _tangent(scene, emitters=t_em, flags=NESTED)), dimage)
    fwd_env = _dot(_forward_film(scene, d, _tangent(scene, env=t_env, flags=NESTED)), dimage)
    _within("max_depth 20: lamp", float((g["emitters"] * t_em).sum()), fwd_em, floor=1)
    _within("max_depth 20: envmap", float((g["env"] * t_env.astype(np.float64)).sum()), fwd_env, floor=1)
    assert "max_depth <= 16" in _reverse(scene, d, dimage, film, wanted=[(top, REFLECTANCE, 0)], flags=NESTED, expect=UNSUPPORTED)
    assert "max_depth <= 16" in _reverse(scene, d, dimage, film, tex_floats=_tex_floats(scene), flags=NESTED, expect=UNSUPPORTED)


def test_a_constant_bitmap_weight_is_the_constant_weight(gpu):
    """The textured-weight path against the constant-weight path: a 3 x 2 bitmap of 0.3 everywhere.  The forward film of the all-ones texel
    tangent is that of the constant's tangent 1 (the luminance weights sum to 1), and the texel gradients add up to the constant's."""
    const, dc, top, _ = _identity_box(gpu, "blend")
    tex, dt, top_t, _ = _identity_box(gpu, "blend", weight_map=np.full((2, 3, 3), 0.3, F32))
    dimage = _random_dimage(24, 32)
    film_c, film_t = _primal_film(const, dc), _primal_film(tex, dt)
    want = _dot(_forward_film(const, dc, _tangent(const, bsdf={(top, REFLECTANCE, 0): 1.0}, flags=NESTED)), dimage)
    off, w, h = _tex_info(tex, tex.texture_index(top_t))
    ones = np.zeros(_tex_floats(tex), F32)
    ones[off: off + 3 * w * h] = 1.0
    got_f = _dot(_forward_film(tex, dt, _tangent(tex, tex=ones, flags=NESTED)), dimage)
    got_r = float(_reverse(tex, dt, dimage, film_t, tex_floats=_tex_floats(tex), flags=NESTED)["tex"][off: off + 3 * w * h].sum())
    g_c = _reverse(const, dc, dimage, film_c, wanted=[(top, REFLECTANCE, 0)], flags=NESTED)["bsdf"][top, 0]
    _within("bitmap weight against constant weight: forward / reverse / constant reverse", [got_f, got_r, g_c], [want, want, want], floor=3)
    # a tangent or a wanted flag on the weight that holds a texture is refused by name
    from mitsuba2_amd import _lib as L
    out = torch.zeros((dt.crop_height, dt.crop_width, 5), device="cuda")
    td = _tangent(tex, bsdf={(top_t, REFLECTANCE, 0): 1.0}, flags=NESTED)
    assert L.lib().mtsamd_render_forward(tex._handle, C.byref(dt), C.byref(td[0]), _vp(out), None) == UNSUPPORTED
    assert ("bsdf %d: weight holds a texture" % top_t) in L.lib().mtsamd_last_error().decode()
    assert ("bsdf %d: weight holds a texture" % top_t) in _reverse(tex, dt, dimage, film_t, wanted=[(top_t, REFLECTANCE, 0)], flags=NESTED, expect=UNSUPPORTED)


# ---- F. launch edges ----------------------------------------------------------------------------------------------------------------------------
def test_launch_edges(gpu):
    """45 samples; a forward film in several passes equals the one-pass film bit for bit; reverse gradients accumulate into a pre-filled
    buffer and unwanted entries keep their bits."""
    mat = {"type": "blendbsdf", "weight": 0.4, "bsdf_0": ROUGH, "bsdf_1": {"type": "diffuse", "reflectance": [0.5, 0.3, 0.6]}}
    scene, d, top = _box_with(gpu, mat, w=5, h=3, spp=3, rr_depth=2)
    c0, c1 = _child(scene, top, 0), _child(scene, top, 1)
    film = _primal_film(scene, d)
    dimage = _random_dimage(3, 5)
    wanted = [(top, REFLECTANCE, 0), (c0, ALPHA, 0), (c1, REFLECTANCE, 1)]
    g = _reverse(scene, d, dimage, film, wanted=wanted, emitters=True, flags=NESTED)
    want = [_dot(_forward_film(scene, d, _tangent(scene, bsdf={w: 1.0}, flags=NESTED)), dimage) for w in wanted]
    _within("45 samples: weight, child alpha, child reflectance", [g["bsdf"][b, 3 * k + c] for (b, k, c) in wanted], want, floor=2)
    # several passes
    big, db, top_b = _box_with(gpu, mat, w=48, h=32, spp=4, rr_depth=2)
    td = _tangent(big, bsdf={(top_b, REFLECTANCE, 0): 1.0, (_child(big, top_b, 0), ALPHA, 0): 0.5}, emitters=np.ones((1, 3), F32), flags=NESTED)
    one = _forward_film(big, db, td)
    same, ds, _ = _box_with(gpu, mat, w=48, h=32, spp=4, rr_depth=2, max_pass_log2=10)
    several = _forward_film(same, ds, _tangent(same, bsdf={(top_b, REFLECTANCE, 0): 1.0, (_child(same, top_b, 0), ALPHA, 0): 0.5}, emitters=np.ones((1, 3), F32), flags=NESTED))
    assert np.array_equal(one.view(np.uint32), several.view(np.uint32)) and np.abs(one[..., :3]).max() > 1e-2
    # accumulation
    pre = {"bsdf": torch.full((_n_flat(scene), 18), 3.0, device="cuda"), "emitters": torch.full((1, 3), -2.0, device="cuda")}
    before = pre["bsdf"].cpu().numpy().copy()
    acc = _reverse(scene, d, dimage, film, wanted=wanted, emitters=True, flags=NESTED, into=pre)
    got = acc["bsdf"].cpu().numpy()
    mask = np.zeros(got.shape, bool)
    for (b, k, c) in wanted:
        mask[b, 3 * k + c] = True
    assert np.array_equal(got[~mask].view(np.uint32), before[~mask].view(np.uint32))
    assert np.allclose(got[mask] - 3.0, g["bsdf"][mask], rtol=1e-4, atol=1e-6)
    assert np.allclose(acc["emitters"].cpu().numpy() + 2.0, g["emitters"], rtol=1e-4, atol=1e-5)


def test_a_clamped_weight_has_no_derivative_and_its_children_do(gpu):
    """raw weight 1.3: the clamp is flat there, so the weight's tangent contributes nothing and its gradient is 0; the children's
    derivatives are finite (bsdf_1 at weight 1) and the never-sampled child's are 0"""
    mat = {"type": "blendbsdf", "weight": 1.3, "bsdf_0": ROUGH, "bsdf_1": {"type": "diffuse", "reflectance": [0.5, 0.3, 0.6]}}
    scene, d, top = _box_with(gpu, mat, rr_depth=2)
    c0, c1 = _child(scene, top, 0), _child(scene, top, 1)
    film = _primal_film(scene, d)
    dimage = _random_dimage(24, 32)
    assert not _forward_film(scene, d, _tangent(scene, bsdf={(top, REFLECTANCE, 0): 1.0}, flags=NESTED))[..., :3].any()
    wanted = [(top, REFLECTANCE, 0), (c0, ALPHA, 0)] + [(c1, REFLECTANCE, c) for c in range(3)]
    g = _reverse(scene, d, dimage, film, wanted=wanted, flags=NESTED)["bsdf"]
    assert g[top, 0] == 0.0 and g[c0, 3 * ALPHA] == 0.0 and np.isfinite(g).all()
    fwd = [_dot(_forward_film(scene, d, _tangent(scene, bsdf={(c1, REFLECTANCE, c): 1.0}, flags=NESTED)), dimage) for c in range(3)]
    assert np.isfinite(fwd).all()
    _within("clamped weight: the child at weight 1", g[c1, :3], fwd, floor=2)


# ---- opt-in --------------------------------------------------------------------------------------------------------------------------------------
def test_opt_in_and_refusals(gpu):
    """Without bit 4 the scene is refused as before; the per-family adjoints keep refusing it; bit 4 in a scene without nested records is the
    unknown bit; other entries of a nested row are refused by name."""
    from mitsuba2_amd import _lib as L
    lib = L.lib()
    mat = {"type": "mask", "opacity": 0.6, "nested": PLASTIC}
    scene, d, top = _box_with(gpu, mat)
    film = _primal_film(scene, d)
    dimage = _random_dimage(24, 32)
    out = torch.zeros((24, 32, 5), device="cuda")

    def forward_refused(sc, td, code, text):
        assert lib.mtsamd_render_forward(sc._handle, C.byref(d), C.byref(td[0]), _vp(out), None) == code, lib.mtsamd_last_error()
        assert text in lib.mtsamd_last_error().decode(), lib.mtsamd_last_error()
        assert lib.mtsamd_sample_forward(sc._handle, C.byref(d), C.byref(td[0]), 0, 8, _vp(out), None, None) == code
    for flags in (0, DETACH):
        forward_refused(scene, _tangent(scene, emitters=np.ones((1, 3), F32), flags=flags), UNSUPPORTED, "blendbsdf / mask")
        assert "blendbsdf / mask" in _reverse(scene, d, dimage, film, emitters=True, flags=flags, expect=UNSUPPORTED)
    forward_refused(scene, _tangent(scene, emitters=np.ones((1, 3), F32), flags=2), INVALID, "unknown flag bits")
    forward_refused(scene, _tangent(scene, bsdf={(top, REFLECTANCE, 1): 1.0}, flags=NESTED), UNSUPPORTED, "a mask record has one differentiable scalar, its opacity")
    assert "kind 4, component 0 is wanted" in _reverse(scene, d, dimage, film, wanted=[(top, ALPHA, 0)], flags=NESTED, expect=UNSUPPORTED)
    g = torch.zeros(1, device="cuda")
    assert lib.mtsamd_render_adjoint_param(scene._handle, C.byref(d), _vp(torch.from_numpy(dimage).cuda()), _vp(film), _child(scene, top), 0, 0, 0.0, _vp(g), None) == UNSUPPORTED
    assert b"blendbsdf / mask" in lib.mtsamd_last_error()
    plain, dp, _ = _box_with(gpu, PLASTIC)
    td = _tangent(plain, emitters=np.ones((1, 3), F32), flags=NESTED)
    assert lib.mtsamd_render_forward(plain._handle, C.byref(dp), C.byref(td[0]), _vp(out), None) == INVALID and b"unknown flag bits" in lib.mtsamd_last_error()
    assert "unknown flag bits" in _reverse(plain, dp, dimage, _primal_film(plain, dp), emitters=True, flags=NESTED, expect=INVALID)
    assert lib.mtsamd_abi_version() == 6


# ---- G. Python -------------------------------------------------------------------------------------------------------------------------------------
def test_traverse_render_forward_and_the_fused_backward_pass(gpu):
    from mitsuba2_amd import autodiff
    scene, d, top, _ = _identity_box(gpu, "blend")
    params = autodiff.traverse(scene, emitters=True)
    keys = set(params.keys())
    assert {"nest.weight.value", "nest.bsdf_0.alpha.value", "nest.bsdf_0.eta.value", "nest.bsdf_0.k.value", "nest.bsdf_0.specular_reflectance.value",
            "nest.bsdf_1.reflectance.data"} <= keys, keys
    lamp = [k for k in keys if k.endswith(".emitter.radiance.value")][0]
    masked, dm, top_m, _ = _identity_box(gpu, "mask")
    mkeys = set(autodiff.traverse(masked).keys())
    assert {"nest.opacity.data", "nest.nested_bsdf.diffuse_reflectance.value", "nest.nested_bsdf.specular_reflectance.value"} <= mkeys, mkeys
    # the keys are settable: the weight moves the render
    base = autodiff._render_film(scene, d).cpu().numpy()
    params["nest.weight.value"] = torch.tensor([0.8])
    params.update()
    moved = autodiff._render_film(scene, d).cpu().numpy()
    assert not np.array_equal(base, moved)
    params["nest.weight.value"] = torch.tensor([0.3])
    params.update()
    assert np.array_equal(autodiff._render_film(scene, d).cpu().numpy(), base)
    # render_forward(nested=True) is the C call
    tangents = {"nest.weight.value": torch.tensor([1.0]), "nest.bsdf_0.alpha.value": torch.tensor([0.5]), lamp: torch.tensor([1.0, 2.0, 0.5])}
    autodiff._render_counter[id(scene)] = 0
    image = autodiff.render_forward(scene, params, tangents, nested=True).cpu().numpy().astype(np.float64)
    seed = scene.sensors()[0].sampler().seed_value()
    dd = autodiff._desc(scene, scene.sensors()[0], scene.integrator(), None, seed)
    c0 = _child(scene, top, 0)
    want = _image(_forward_film(scene, dd, _tangent(scene, bsdf={(top, REFLECTANCE, 0): 1.0, (c0, ALPHA, 0): 0.5}, emitters=np.array([[1.0, 2.0, 0.5]], F32), flags=NESTED)))
    assert np.abs(want).max() > 1e-2 and np.allclose(image.reshape(want.shape), want, rtol=1e-5, atol=1e-7)
    with pytest.raises(RuntimeError, match="nested=True"):
        autodiff.render_forward(scene, params, tangents)
    # backward="fused", nested=True: the gradients of a mixed key set are those of the C call
    mixed = ["nest.weight.value", "nest.bsdf_0.alpha.value", lamp]
    params.keep(mixed)
    for k in mixed:
        params[k].requires_grad_(True)
    with pytest.raises(RuntimeError, match="nested=True"):
        autodiff.render(scene, params=params, backward="fused")
    params[lamp].requires_grad_(False)         # (the default pass names render_forward for a lamp in a general scene, as before)
    with pytest.raises(RuntimeError, match="nested=True"):
        autodiff.render(scene, params=params)
    params[lamp].requires_grad_(True)
    autodiff._render_counter[id(scene)] = 0
    weights = torch.from_numpy(_random_dimage(24, 32).reshape(-1)).cuda()
    img = autodiff.render_torch(scene, params=params, backward="fused", nested=True)
    (img * weights).sum().backward()
    film = _primal_film(scene, dd)
    g = _reverse(scene, dd, weights.reshape(24, 32, 3), film, wanted=[(top, REFLECTANCE, 0), (c0, ALPHA, 0)], emitters=True, flags=NESTED)
    got = np.concatenate([params[k].grad.cpu().numpy().reshape(-1) for k in mixed])
    want = np.concatenate([[g["bsdf"][top, 0]], [g["bsdf"][c0, 3 * ALPHA]], g["emitters"][0]])
    assert np.abs(want).min() > 1e-4
    _assert_close("fused backward pass with nested=True against the C call", got, want)
    # the keyword is inert in a scene without nested records
    plain, dp, _ = _box_with(gpu, PLASTIC)
    pp = autodiff.traverse(plain)
    assert not [k for k in pp.keys() if "weight" in k or "opacity" in k]
    k0 = sorted(pp.keys())[0]
    autodiff._render_counter[id(plain)] = 0
    a = autodiff.render_forward(plain, pp, {k0: torch.ones_like(pp[k0])}, nested=True)
    autodiff._render_counter[id(plain)] = 0
    b = autodiff.render_forward(plain, pp, {k0: torch.ones_like(pp[k0])})
    assert torch.equal(a, b)


def test_opacity_inversion_on_the_point_lit_box(gpu):
    """Adam on opacity.value from 0.9 towards the image rendered at 0.4: 60 steps at lr 0.02, 16 x 16 x 64 spp; the final distance to 0.4 is
    below a fifth of the initial one."""
    from mitsuba2_amd import autodiff
    target_scene, dt = _point_box(gpu, "mask", 0.4, 3, spp=64)
    target = autodiff._image_of(autodiff._render_film(target_scene, dt)).detach()
    scene, _ = _point_box(gpu, "mask", 0.9, 3, spp=64)
    params = autodiff.traverse(scene)
    params.keep(["nest.opacity.value"])
    opt = autodiff.Adam(params, lr=0.02)
    for step in range(60):
        img = autodiff.render(scene, optimizer=opt, backward="fused", nested=True)
        loss = ((img - target) ** 2).mean()
        loss.backward()
        opt.step()
        with torch.no_grad():      # the projection an opacity optimisation applies: the closed interval on which it has a derivative
            params.properties["nest.opacity.value"].clamp_(0.0, 1.0)
    final = float(params["nest.opacity.value"].item())
    print("opacity inversion: 0.9 -> %.4f after 60 Adam steps at lr 0.02 (target 0.4)" % final)
    assert abs(final - 0.4) < 0.2 * abs(0.9 - 0.4), final

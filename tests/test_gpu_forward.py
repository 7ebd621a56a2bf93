"""The forward-mode derivative render (mtsamd_render_forward / mtsamd_sample_forward, k_forward; autodiff.render_forward): the image of
d(image)/d(t) along one tangent over BSDF constants, reflectance texels, emitter colours and envmap texels
(docs/examples/10_inverse_rendering/forward_diff.py).

1. Homogeneity: radiance is linear in all emitter colours jointly, so with the current colours (and envmap texels) as the tangent the
   derivative IS the radiance.  The bound is derived, not measured: every term is a product of the same <= 12 non-negative factors,
   possibly associated differently (<= 24 * 2^-24), and at most 34 non-negative terms are summed in the same order at max_depth <= 16:
   under 4e-6, asserted at rtol 1e-5; zeros stay zero; positions, alpha and the A / W channels of the films are equal bit for bit.
2. Linearity in one emitter: a one-hot colour tangent gives the film of a primal render lit by that emitter alone.
3. BSDF constants with the roulette factor held fixed: block sums of the image against the oracle's forward-mode replay (block
   indicators as dLoss/dImage) and <dimage, image> against mtsamd_render_adjoint_param, at that replay's bound 2e-3 |want| + 1e-5.
4. The attached roulette factor on the textured Cornell box: block sums against <gradient, tangent> of the oracle's adjoint and of
   mtsamd_render_adjoint, all families at once and one at a time, at that adjoint's bound (rtol 2e-2, atol 2e-3 max|want|).
5. A general scene: texel and envmap tangents against mtsamd_render_adjoint_textures / mtsamd_render_adjoint_envmap.
6. The reference scenario through autodiff.render_forward against a central difference of autodiff.render at the same seed.
7. Refusals, and the emitter keys of traverse(scene, emitters=True).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mitsuba2_amd import scenes
from test_bvh_depth_cpu import hierarchy_scene, hierarchy_sensor
from test_gpu_autodiff import _assert_close, _material_scene

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
ROUGH = {"type": "roughconductor", "alpha": 0.3, "distribution": "ggx", "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14], "specular_reflectance": [0.9, 0.8, 0.7]}
PLASTIC = {"type": "plastic", "diffuse_reflectance": [0.2, 0.5, 0.3], "int_ior": 1.6}
NAMES = ["white", "red", "green", "light", "textured"]


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _tangent(scene, bsdf=None, emitters=None, tex=None, env=None, h=0.0, flags=0):
    """(mtsamd_tangent_desc, what has to stay alive with it); bsdf: {(record, kind, component): value}"""
    from mitsuba2_amd import _lib as L
    td, keep = L.TangentDesc(), []
    if bsdf is not None:
        a = np.zeros((len(scene._bsdf_records), 18), np.float32)
        for (b, kind, comp), v in bsdf.items():
            a[b, 3 * kind + comp] = v
        keep.append(a)
        td.bsdf_tangents = a.ctypes.data_as(L.f32p)
    if emitters is not None:
        a = np.ascontiguousarray(emitters, np.float32)
        keep.append(a)
        td.emitter_tangents = a.ctypes.data_as(L.f32p)
    for name, t in (("texture_tangents_dev", tex), ("envmap_tangent_dev", env)):
        if t is not None:
            t = torch.as_tensor(np.ascontiguousarray(t, np.float32)).cuda().contiguous() if not isinstance(t, torch.Tensor) else t
            keep.append(t)
            setattr(td, name, t.data_ptr())
    td.h, td.flags = float(h), int(flags)
    return td, keep


def _desc(scene, p, **fields):
    from mitsuba2_amd import autodiff
    d = autodiff._desc(scene, scene.sensors()[0], scene.integrator(), None, p["seed"])
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def _forward_film(scene, d, td):
    from mitsuba2_amd import _lib as L
    film = torch.zeros((d.crop_height, d.crop_width, 5), device="cuda")
    L.check(L.lib().mtsamd_render_forward(scene._handle, C.byref(d), C.byref(td[0]), _vp(film), None))
    torch.cuda.synchronize()
    return film.cpu().numpy()


def _primal_film(scene, d):
    from mitsuba2_amd import autodiff
    film = autodiff._render_film(scene, d)
    torch.cuda.synchronize()
    return film


def _image(film):
    """autodiff._image_of in float64"""
    film = np.asarray(film, np.float64)
    return film[..., :3] / (film[..., 4:5].astype(np.float32).astype(np.float64) + np.float64(np.float32(1e-8)))


def _emitter_colours(sd):
    from mitsuba2_amd import emitters as E
    rows = np.zeros((max(len(sd["emitters"]), 1), 3), np.float32)
    for e, em in enumerate(sd["emitters"]):
        if em.get("type", "area") != "envmap":
            rows[e] = np.broadcast_to(np.asarray(E.normalize(em)["radiance"], np.float32), (3,))
    return rows


def _blocks(h, w, size=8):
    return [(y, x) for y in range(0, h, size) for x in range(0, w, size)]


def _block_sums(image, size=8):
    h, w, _ = image.shape
    return np.array([[image[y:y + size, x:x + size, c].sum() for c in range(3)] for (y, x) in _blocks(h, w, size)])


def _indicator(h, w, y, x, c=None, size=8):
    d = np.zeros((h, w, 3), np.float32)
    if c is None:
        d[y:y + size, x:x + size, :] = 1.0
    else:
        d[y:y + size, x:x + size, c] = 1.0
    return d


# ---------------------------------------------------------------------------------------------
# 1. homogeneity

def _lit_box():
    """the Cornell box lit by its area light, a point, a spot and a directional light under a constant environment"""
    sd = scenes.cornell_box()
    spot_tw = scenes.look_at([278, 500, 200], [300, 0, 320], [0, 0, 1])
    area = list(sd["emitters"])
    sd["emitters"] = [{"type": "constant", "radiance": [0.4, 0.6, 1.0]}] + area + [
        {"type": "point", "position": [100, 300, 100], "intensity": [2e5, 2e5, 3e5]},
        {"type": "spot", "to_world": spot_tw, "intensity": [5e5, 3e5, 3e5], "cutoff_angle": 35.0, "beam_width": 20.0},
        {"type": "directional", "direction": [0.3, -1.0, 0.4], "irradiance": [1.0, 1.5, 0.5]}]
    sd["meshes"] = [dict(m, emitter=1) if m.get("emitter", -1) >= 0 else m for m in sd["meshes"] if m is not sd["meshes"][1]]      # no ceiling: the sky is seen
    return sd


def _homogeneity_scene(gpu, which, w, h, spp):
    env = None
    if which == "cbox":
        sd = scenes.cornell_box()
        p = scenes.cornell_box_sensor(w, h, spp, seed=3, max_depth=6, rfilter="gaussian")
    elif which == "lights":
        sd = _lit_box()
        p = scenes.cornell_box_sensor(w, h, spp, seed=4, max_depth=8, rfilter="box")
    else:
        env = np.random.RandomState(7).uniform(0.2, 1.0, size=(8, 16, 3)).astype(np.float32)
        sd, _ = hierarchy_scene("shallow", sphere=ROUGH, envmap=env, area=True)
        p = dict(hierarchy_sensor(w, h, spp, 7, "gaussian", seed=9), aperture_radius=0.05, focus_distance=5.5)
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=p["max_depth"]))
    return sd, p, scene, env


@pytest.mark.parametrize("w,h,spp,pass_log2", [(5, 3, 3, 0), (96, 64, 96, 0), (48, 32, 4, 10)], ids=["45_samples", "two_trips", "several_passes"])
@pytest.mark.parametrize("which", ["cbox", "sphere_envmap_thinlens", "lights"])
def test_homogeneity_in_the_emitter_colours(gpu, which, w, h, spp, pass_log2):
    from mitsuba2_amd import _lib as L
    sd, p, scene, env = _homogeneity_scene(gpu, which, w, h, spp)
    d = _desc(scene, p, max_pass_log2=pass_log2)
    n = w * h * spp
    if spp == 96:
        assert n > 2048 * 256          # the threads of k_forward make a second trip
    if which == "sphere_envmap_thinlens":
        info = (C.c_uint32 * 6)()
        L.check(L.lib().mtsamd_scene_info(scene._handle, info))
        assert info[0] > 64            # a hierarchy scene: k_forward<false>
    td = _tangent(scene, emitters=_emitter_colours(sd), env=env)
    rad, pos = torch.zeros((n, 4), device="cuda"), torch.zeros((n, 2), device="cuda")
    fwd, fpos = torch.full((n, 4), -7.0, device="cuda"), torch.full((n, 2), -7.0, device="cuda")
    L.check(L.lib().mtsamd_sample_radiance(scene._handle, C.byref(d), 0, n, _vp(rad), _vp(pos), None))
    L.check(L.lib().mtsamd_sample_forward(scene._handle, C.byref(d), C.byref(td[0]), 0, n, _vp(fwd), _vp(fpos), None))
    torch.cuda.synchronize()
    rad, pos, fwd, fpos = (t.cpu().numpy() for t in (rad, pos, fwd, fpos))
    assert np.array_equal(pos.view(np.uint32), fpos.view(np.uint32)) and np.array_equal(rad[:, 3].view(np.uint32), fwd[:, 3].view(np.uint32))
    assert np.isfinite(rad).all() and (rad[:, :3] > 0).mean() > 0.3
    err = np.abs(fwd[:, :3].astype(np.float64) - rad[:, :3]) / np.maximum(np.abs(rad[:, :3].astype(np.float64)), 1e-300)
    print("%s %dx%d@%d: largest relative deviation of a sample %.3g (bound 1e-5)" % (which, w, h, spp, float(err[rad[:, :3] != 0].max())))
    assert (fwd[:, :3][rad[:, :3] == 0] == 0).all()
    assert (np.abs(fwd[:, :3].astype(np.float64) - rad[:, :3]) <= 1e-5 * np.abs(rad[:, :3])).all()
    # a window of the samples, starting inside a pixel
    if n > 40:
        part = torch.full((20, 4), -7.0, device="cuda")
        L.check(L.lib().mtsamd_sample_forward(scene._handle, C.byref(d), C.byref(td[0]), 17, 20, _vp(part), None, None))
        assert np.array_equal(part.cpu().numpy().view(np.uint32), fwd[17:37].view(np.uint32))
    # the films: RGB within the same bound, A and W bit for bit
    film = _primal_film(scene, d).cpu().numpy()
    dfilm = _forward_film(scene, d, td)
    assert np.array_equal(film[..., 3:].view(np.uint32), dfilm[..., 3:].view(np.uint32))
    # a pixel's sum holds the same non-negative terms in the same order on both sides
    assert (np.abs(dfilm[..., :3].astype(np.float64) - film[..., :3]) <= 1e-5 * np.abs(film[..., :3])).all()


# ---------------------------------------------------------------------------------------------
# 2. linearity in one emitter

def test_one_hot_emitter_tangent_is_the_render_lit_by_that_emitter(gpu):
    sd = scenes.cornell_box()
    sd["emitters"].append(dict(type="area", radiance=np.array([2.0, 4.0, 8.0], np.float32)))         # test_gpu_parity.test_two_emitters
    quad = np.array([[130, 165.5, 65], [82, 165.5, 225], [240, 165.5, 272], [290, 165.5, 114]], np.float32)
    sd["meshes"].append(dict(positions=quad, faces=np.array([[0, 1, 2], [0, 2, 3]], np.uint32), normals=None, texcoords=None, bsdf=0, emitter=1))
    p = scenes.cornell_box_sensor(48, 48, 8, seed=2, max_depth=6)
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=6))
    d = _desc(scene, p)
    colour = np.array([1.5, 0.5, 2.5], np.float32)
    films = []
    for e in range(2):
        rows = np.zeros((2, 3), np.float32)
        rows[e] = colour
        films.append(_forward_film(scene, d, _tangent(scene, emitters=rows)))
    for e in range(2):
        for k in range(2):
            scene.set_emitter_radiance(k, colour if k == e else [0.0, 0.0, 0.0])
        want = _primal_film(scene, d).cpu().numpy()
        assert want[..., :3].max() > 0.1
        assert np.array_equal(want[..., 3:].view(np.uint32), films[e][..., 3:].view(np.uint32))
        dev = np.abs(films[e][..., :3].astype(np.float64) - want[..., :3])
        print("emitter %d: largest deviation %.3g of the value (bound 1e-5)" % (e, float((dev / np.maximum(np.abs(want[..., :3]), 1e-30))[want[..., :3] != 0].max())))
        assert (dev <= 1e-5 * np.abs(want[..., :3])).all()


# ---------------------------------------------------------------------------------------------
# 3. BSDF constants, roulette factor held fixed

MATERIAL_CASES = [("tall.alpha.value", 4, 0.003), ("tall.k.value", 3, 0.03), ("tall.specular_reflectance.value", 1, 0.01), ("small.diffuse_reflectance.value", 0, 0.005)]


@functools.lru_cache(maxsize=None)
def _material_oracle():
    import oracle_binding as ob
    sd = scenes.cornell_box()
    sd["bsdfs"] = list(sd["bsdfs"]) + [dict(ROUGH, id="tall"), dict(PLASTIC, id="small")]
    sd["meshes"][6] = dict(sd["meshes"][6], bsdf=len(sd["bsdfs"]) - 2)
    sd["meshes"][7] = dict(sd["meshes"][7], bsdf=len(sd["bsdfs"]) - 1)
    p = scenes.cornell_box_sensor(40, 32, 16, seed=77, max_depth=5, rfilter="box")
    S = ob.OracleScene(sd)
    desc = ob.make_desc(p, analytic=True, film_rgb=True)
    _, film_o = S.render_image(desc)
    return S, desc, film_o


@pytest.mark.parametrize("key,kind,step", MATERIAL_CASES)
def test_bsdf_constants_match_the_oracle_block_by_block(gpu, oracle, key, kind, step):
    """60 values per parameter (20 blocks of 8 x 8 pixels x 3 channels), none left out.  On the oracle's side alone: 57 of the 60 values
    of alpha exceed 1e-3; for the three colour parameters exactly the 20 red-channel values are non-zero, all >= 2.4e-3."""
    from mitsuba2_amd import _lib as L
    sd, p, scene = _material_scene(gpu, (ROUGH, PLASTIC), w=40, h=32, spp=16, max_depth=5)
    d = _desc(scene, dict(p, seed=77))
    bsdf_index = len(sd["bsdfs"]) - (2 if key.startswith("tall") else 1)
    shapes = [i for i, m in enumerate(sd["meshes"]) if m["bsdf"] == bsdf_index]
    S, desc, film_o = _material_oracle()
    td = _tangent(scene, bsdf={(bsdf_index, kind, 0): 1.0}, h=step, flags=L.FORWARD_DETACH_ROULETTE)
    dfilm = _forward_film(scene, d, td)
    film = _primal_film(scene, d)
    assert np.array_equal(film.cpu().numpy()[..., 3:].view(np.uint32), dfilm[..., 3:].view(np.uint32))
    got = _block_sums(_image(dfilm))
    want = np.array([[S.render_adjoint_param(desc, _indicator(32, 40, y, x, c), film_o, shapes, kind, 0, step) for c in range(3)] for (y, x) in _blocks(32, 40)])
    assert got.shape == want.shape == (20, 3)
    assert (np.abs(want) > 1e-3).sum() >= 20, np.abs(want)
    dev = np.abs(got - want) / (2e-3 * np.abs(want) + 1e-5)
    print("%s: worst deviation of a block %.3g of the bound; %d of 60 oracle values above 1e-3" % (key, float(dev.max()), int((np.abs(want) > 1e-3).sum())))
    assert (dev < 1).all(), (key, float(dev.max()), got[dev >= 1], want[dev >= 1])
    # against the reverse replay on the GPU: <dimage, J t> = <J^T dimage, t>
    dimage = np.random.RandomState(4).uniform(-1.0, 1.0, (32, 40, 3)).astype(np.float32)
    di = torch.from_numpy(dimage).cuda()
    g = torch.zeros(1, device="cuda")
    L.check(L.lib().mtsamd_render_adjoint_param(scene._handle, C.byref(d), _vp(di), _vp(film), bsdf_index, kind, 0, step, _vp(g), None))
    torch.cuda.synchronize()
    rev, fwd = float(g.item()), float((_image(dfilm) * dimage.astype(np.float64)).sum())
    print("%s: <dimage, forward image> %.6g, reverse %.6g, deviation %.3g (bound 2e-3)" % (key, fwd, rev, abs(fwd - rev) / abs(rev)))
    assert abs(rev) > 1e-3 and abs(fwd - rev) < 2e-3 * abs(rev) + 1e-5


def test_bsdf_constants_on_a_hierarchy_scene(gpu, oracle):
    """k_forward<false>: the roughness of a roughconductor sphere under an envmap, six blocks against the oracle, the whole image against
    mtsamd_render_adjoint_param"""
    from mitsuba2_amd import _lib as L
    W, H, step = 24, 16, 0.003
    env = np.random.RandomState(7).uniform(0.2, 1.0, size=(8, 16, 3)).astype(np.float32)
    sd, _ = hierarchy_scene("shallow", sphere=ROUGH, envmap=env, area=True)
    p = hierarchy_sensor(W, H, 8, 5, seed=77)
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=5))
    d = _desc(scene, p)
    film = _primal_film(scene, d)
    S = oracle.OracleScene(sd, naive=True)
    desc = oracle.make_desc(p, analytic=True, film_rgb=True)
    _, film_o = S.render_image(desc)
    dfilm = _forward_film(scene, d, _tangent(scene, bsdf={(0, 4, 0): 1.0}, h=step, flags=L.FORWARD_DETACH_ROULETTE))
    image = _image(dfilm)
    got = _block_sums(image).sum(1)
    want = np.array([S.render_adjoint_param(desc, _indicator(H, W, y, x), film_o, [0], 4, 0, step) for (y, x) in _blocks(H, W)])
    assert got.shape == want.shape == (6,) and (np.abs(want) > 1e-3).sum() >= 3, want
    dev = np.abs(got - want) / (2e-3 * np.abs(want) + 1e-5)
    print("sphere alpha: worst deviation of a block %.3g of the bound" % float(dev.max()))
    assert (dev < 1).all(), (got, want)
    dimage = np.random.RandomState(4).uniform(-1.0, 1.0, (H, W, 3)).astype(np.float32)
    g = torch.zeros(1, device="cuda")
    L.check(L.lib().mtsamd_render_adjoint_param(scene._handle, C.byref(d), _vp(torch.from_numpy(dimage).cuda()), _vp(film), 0, 4, 0, step, _vp(g), None))
    torch.cuda.synchronize()
    rev, fwd = float(g.item()), float((image * dimage.astype(np.float64)).sum())
    assert abs(rev) > 1e-3 and abs(fwd - rev) < 2e-3 * abs(rev) + 1e-5, (fwd, rev)


# ---------------------------------------------------------------------------------------------
# 4. attached roulette, diffuse scene

def _textured_box(gpu, max_depth, rr_depth, w=32, h=32, spp=16):
    tex = (0.3 + 0.5 * np.random.RandomState(1).rand(4, 5, 3)).astype(np.float32)
    sd = scenes.cornell_box(texture=tex)
    for b, n in zip(sd["bsdfs"], NAMES):
        b["id"] = n
    p = scenes.cornell_box_sensor(w, h, spp, seed=5, max_depth=max_depth, rr_depth=rr_depth, rfilter="box")
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=max_depth, rr_depth=rr_depth))
    return sd, tex, p, scene


def test_attached_roulette_matches_the_adjoints_of_the_diffuse_scene(gpu, oracle):
    """Textured Cornell box, rr_depth 2, max_depth 6: random non-negative tangents on every constant reflectance, the texels and the
    lamp's radiance, all at once and one family at a time; 16 blocks x 3 channels against <g, t> of the oracle's adjoint and of
    mtsamd_render_adjoint.  The worst deviation in units of the bound is printed."""
    from mitsuba2_amd import _lib as L
    W = H = 32
    sd, tex, p, scene = _textured_box(gpu, 6, 2)
    d = _desc(scene, p)
    film = _primal_film(scene, d)
    S = oracle.OracleScene(sd, naive=True)
    desc = oracle.make_desc(p, analytic=True, film_rgb=True)
    _, film_o = S.render_image(desc)
    rng = np.random.RandomState(11)
    t_bsdf = rng.uniform(0.0, 1.0, (len(sd["bsdfs"]), 3))
    t_bsdf[4] = 0.0                                           # the textured record has no constant
    t_tex, t_em = rng.uniform(0.0, 1.0, tex.size), rng.uniform(0.0, 4.0, (1, 3))
    families = {"all": (t_bsdf, t_tex, t_em), "constants": (t_bsdf, None, None), "texels": (None, t_tex, None), "radiance": (None, None, t_em)}
    # the reverse side once per block and channel: the oracle's and the GPU's gradients
    rev_o, rev_g = [], []
    for (y, x) in _blocks(H, W):
        for c in range(3):
            dimage = _indicator(H, W, y, x, c)
            gs_o, gt_o, ge_o = S.render_adjoint(desc, dimage, film_o, len(sd["meshes"]), tex.size, n_emitters=1)
            gb_o = np.zeros((len(sd["bsdfs"]), 3))
            for si, m in enumerate(sd["meshes"]):
                gb_o[m["bsdf"]] += gs_o[si]
            rev_o.append((gb_o, gt_o.astype(np.float64), ge_o.astype(np.float64)))
            g_bsdf, g_tex, g_em = torch.zeros((len(sd["bsdfs"]), 3), device="cuda"), torch.zeros(tex.size, device="cuda"), torch.zeros((1, 3), device="cuda")
            L.check(L.lib().mtsamd_render_adjoint(scene._handle, C.byref(d), _vp(torch.from_numpy(dimage).cuda()), _vp(film), _vp(g_bsdf), _vp(g_tex), _vp(g_em), None))
            torch.cuda.synchronize()
            rev_g.append((g_bsdf.cpu().numpy().astype(np.float64), g_tex.cpu().numpy().astype(np.float64), g_em.cpu().numpy().astype(np.float64)))
    for name, (tb, tt, te) in families.items():
        bsdf = {(b, 0, c): tb[b, c] for b in range(len(sd["bsdfs"])) for c in range(3) if tb[b, c] != 0} if tb is not None else None
        dfilm = _forward_film(scene, d, _tangent(scene, bsdf=bsdf, emitters=te, tex=tt))
        assert np.array_equal(film.cpu().numpy()[..., 3:].view(np.uint32), dfilm[..., 3:].view(np.uint32))
        got = _block_sums(_image(dfilm)).reshape(-1)
        for side, rev in (("oracle", rev_o), ("mtsamd_render_adjoint", rev_g)):
            want = np.array([(0.0 if tb is None else (gb * tb).sum()) + (0.0 if tt is None else (gt * tt).sum()) + (0.0 if te is None else (ge * te).sum())
                             for (gb, gt, ge) in rev])
            assert (np.abs(want) > 1e-3 * np.abs(want).max()).sum() >= len(want) // 2, (name, side, want)
            _assert_close("%s against %s" % (name, side), got, want)


def test_the_roulette_flag(gpu):
    from mitsuba2_amd import _lib as L
    films = {}
    for rr_depth in (9, 2):
        sd, tex, p, scene = _textured_box(gpu, 6, rr_depth, 24, 24, 8)
        d = _desc(scene, p)
        t = {(1, 0, 0): 1.0, (1, 0, 1): 0.5, (0, 0, 2): 0.25}
        films[rr_depth] = [_forward_film(scene, d, _tangent(scene, bsdf=t, flags=f)) for f in (0, L.FORWARD_DETACH_ROULETTE)]
        assert np.abs(films[rr_depth][0][..., :3]).max() > 1e-2
    assert np.array_equal(films[9][0].view(np.uint32), films[9][1].view(np.uint32))          # no roulette on any path: nothing to detach
    assert (films[2][0][..., :3] != films[2][1][..., :3]).any()
    assert np.array_equal(films[2][0][..., 3:].view(np.uint32), films[2][1][..., 3:].view(np.uint32))


# ---------------------------------------------------------------------------------------------
# 5. a general scene

def test_texel_and_envmap_tangents_in_a_general_scene(gpu):
    """an open box with a textured plastic floor and back wall, a conductor box and an envmap: <dimage, J t> for three random dimage
    against <g, t> of mtsamd_render_adjoint_textures and of mtsamd_render_adjoint_envmap (max_depth 7: past rr_depth = 5)"""
    from mitsuba2_amd import _lib as L
    from test_gpu_adjoint_textures import _open_box, _sky
    tex = (0.3 + 0.5 * np.random.RandomState(1).rand(4, 5, 3)).astype(np.float32)
    sky = _sky()
    sd = _open_box(tex, textured_bsdf={"type": "plastic", "int_ior": 1.6, "diffuse_reflectance": {"type": "bitmap", "data": tex}}, emitters=[sky])
    W, H = 28, 24
    p = scenes.cornell_box_sensor(W, H, 8, seed=5, max_depth=7, rfilter="gaussian")
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=7))
    d = _desc(scene, p)
    film = _primal_film(scene, d)
    rng = np.random.RandomState(3)
    t_tex, t_env = rng.uniform(0.0, 1.0, tex.size).astype(np.float32), rng.uniform(0.0, 1.0, sky["data"].shape).astype(np.float32)
    image_tex = _image(_forward_film(scene, d, _tangent(scene, tex=t_tex)))
    image_env = _image(_forward_film(scene, d, _tangent(scene, env=t_env)))
    image_both = _image(_forward_film(scene, d, _tangent(scene, tex=t_tex, env=t_env)))
    assert np.allclose(image_both, image_tex + image_env, rtol=1e-4, atol=1e-5 * np.abs(image_both).max())       # the families add up
    got, want = {"texels": [], "envmap": []}, {"texels": [], "envmap": []}
    for seed in (2, 3, 4):
        dimage = np.random.RandomState(seed).uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
        di = torch.from_numpy(dimage).cuda()
        g_tex, g_env = torch.zeros(tex.size, device="cuda"), torch.zeros(sky["data"].shape, device="cuda")
        L.check(L.lib().mtsamd_render_adjoint_textures(scene._handle, C.byref(d), _vp(di), _vp(film), _vp(g_tex), None))
        L.check(L.lib().mtsamd_render_adjoint_envmap(scene._handle, C.byref(d), _vp(di), _vp(film), _vp(g_env), None))
        torch.cuda.synchronize()
        want["texels"].append(float((g_tex.cpu().numpy().astype(np.float64) * t_tex).sum()))
        want["envmap"].append(float((g_env.cpu().numpy().astype(np.float64) * t_env).sum()))
        got["texels"].append(float((image_tex * dimage).sum()))
        got["envmap"].append(float((image_env * dimage).sum()))
    for k in got:
        assert min(np.abs(want[k])) > 1e-2
        _assert_close(k, np.array(got[k]), np.array(want[k]))


# ---------------------------------------------------------------------------------------------
# 6. the reference scenario

def test_forward_diff_scenario_against_central_differences(gpu):
    """forward_diff.py: the tangent [1, 1, 1] on the red wall's reflectance.  With rr_depth > max_depth the image is a polynomial in the
    reflectance (no roulette probability depends on it), so a central difference of render() at the same seed is exact to O(h^2)."""
    from mitsuba2_amd import autodiff
    sd = scenes.cornell_box()
    for b, n in zip(sd["bsdfs"], NAMES):
        b["id"] = n
    p = scenes.cornell_box_sensor(48, 48, 16, seed=1, max_depth=4, rfilter="gaussian")
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=4))
    params = autodiff.traverse(scene)
    key = "red.reflectance.value"
    params.keep([key])
    base = params[key].detach().clone()
    weights = torch.from_numpy(np.random.RandomState(5).uniform(0.0, 1.0, 48 * 48 * 3).astype(np.float32)).cuda() / (48 * 48)
    autodiff._render_counter[id(scene)] = 0
    image = autodiff.render_forward(scene, params, {key: torch.ones(3)})
    assert image.shape == (48 * 48 * 3,) and float(image.abs().max()) > 1e-2
    got = float((image.double() * weights.double()).sum().item())
    losses = []
    for sign in (1.0, -1.0):
        autodiff._render_counter[id(scene)] = 0
        params[key] = base + sign * 0.02
        with torch.no_grad():
            losses.append(float((autodiff.render(scene, params=params).double() * weights.double()).sum().item()))
    params[key] = base
    params.update()
    fd = (losses[0] - losses[1]) / 0.04
    print("forward %.6g, central difference %.6g, deviation %.3g (bound 1e-2)" % (got, fd, abs(got - fd) / abs(fd)))
    assert abs(got - fd) < 1e-2 * abs(fd) + 1e-5, (got, fd)


# ---------------------------------------------------------------------------------------------
# 7. refusals and the emitter keys

def test_refusals(gpu):
    from mitsuba2_amd import autodiff, _lib as L
    lib = L.lib()
    sd, tex, p, scene = _textured_box(gpu, 4, 5, 8, 8, 2)
    out = torch.zeros((8, 8, 5), device="cuda")
    rows = _emitter_colours(sd)

    def film_call(sc, d, td):
        return lib.mtsamd_render_forward(sc._handle, C.byref(d), C.byref(td[0]), _vp(out), None), lib.mtsamd_last_error().decode()

    def sample_call(sc, d, td):
        return lib.mtsamd_sample_forward(sc._handle, C.byref(d), C.byref(td[0]), 0, 4, _vp(out), None, None), lib.mtsamd_last_error().decode()

    def refused(sc, d, td, code, text, film_only=False):
        for call in (film_call,) if film_only else (film_call, sample_call):
            rc, msg = call(sc, d, td)
            assert rc == code and text in msg, (rc, msg, text)

    ok = _tangent(scene, emitters=rows)
    assert film_call(scene, _desc(scene, p), ok)[0] == 0 and sample_call(scene, _desc(scene, p), ok)[0] == 0
    refused(scene, _desc(scene, p), _tangent(scene), INVALID, "the tangent is empty")
    refused(scene, _desc(scene, p), _tangent(scene, emitters=rows, flags=2), INVALID, "unknown flag bits")
    refused(scene, _desc(scene, p, integrator=1), ok, UNSUPPORTED, "path integrator")
    refused(scene, _desc(scene, p, row_begin=2), ok, UNSUPPORTED, "whole crop window")
    refused(scene, _desc(scene, p, part_count=2, part_tile_rows=4), ok, UNSUPPORTED, "whole crop window")
    refused(scene, _desc(scene, p, moment=1), ok, UNSUPPORTED, "moment", film_only=True)
    refused(scene, _desc(scene, p, film_rgb=0), ok, UNSUPPORTED, "film_rgb", film_only=True)
    refused(scene, _desc(scene, p, rfilter=5, rfilter_param=5.0), ok, UNSUPPORTED, "too wide", film_only=True)       # lanczos, 5 lobes: 10 taps
    refused(scene, _desc(scene, p), _tangent(scene, env=np.zeros((2, 2, 3), np.float32)), UNSUPPORTED, "no envmap emitter")
    refused(scene, _desc(scene, p), _tangent(scene, bsdf={(4, 0, 0): 1.0}), UNSUPPORTED, "bsdf 4 (type 0) has no differentiable parameter of kind 0")
    refused(scene, _desc(scene, p), _tangent(scene, bsdf={(1, 4, 0): 1.0}), UNSUPPORTED, "bsdf 1 (type 0) has no differentiable parameter of kind 4")
    refused(scene, _desc(scene, p), _tangent(scene, bsdf={(1, 0, 0): float("nan")}), INVALID, "not finite")
    refused(scene, _desc(scene, p), _tangent(scene, emitters=rows * np.float32("inf")), INVALID, "not finite")
    rc, msg = lib.mtsamd_sample_forward(scene._handle, C.byref(_desc(scene, p)), C.byref(ok[0]), 120, 10, _vp(out), None, None), lib.mtsamd_last_error()
    assert rc == INVALID and b"sample range" in msg
    # scenes the replay does not cover
    plain = gpu.Scene(scenes.cornell_box(), sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=4))
    refused(plain, _desc(plain, p), _tangent(plain, tex=np.zeros(4, np.float32)), UNSUPPORTED, "no bitmap textures")
    spectral = gpu.Scene(scenes.cornell_box(), variant="spectral", sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=4))
    refused(spectral, _desc(spectral, p), ok, UNSUPPORTED, "RGB variant")
    sd_b = scenes.cornell_box()
    sd_b["bsdfs"] = list(sd_b["bsdfs"]) + [{"type": "blendbsdf", "weight": 0.5, "bsdf_0": {"type": "diffuse"}, "bsdf_1": {"type": "conductor"}}]
    sd_b["meshes"][6] = dict(sd_b["meshes"][6], bsdf=len(sd_b["bsdfs"]) - 1)
    blend = gpu.Scene(sd_b, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=4))
    refused(blend, _desc(blend, p), ok, UNSUPPORTED, "blendbsdf / mask")
    sd_t = scenes.cornell_box()
    sd_t["bsdfs"] = list(sd_t["bsdfs"]) + [{"type": "roughconductor", "id": "tall", "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14], "alpha":{"type": "bitmap", "data": np.full((2, 2, 3), 0.2, np.float32)}}]
    sd_t["meshes"][6] = dict(sd_t["meshes"][6], bsdf=len(sd_t["bsdfs"]) - 1)
    textured = gpu.Scene(sd_t, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=4))
    refused(textured, _desc(textured, p), ok, UNSUPPORTED, "textured BSDF parameters")
    # the Python surface: keys without a forward derivative raise, as do unknown keys and spectral scenes
    params = autodiff.traverse(textured, geometry=True)
    pkey = next(k for k in params.keys() if k.endswith(".alpha.data"))
    vkey = next(k for k in params.keys() if k.endswith(".vertex_positions_buf"))
    for k in (pkey, vkey):
        with pytest.raises(RuntimeError, match="no forward-mode derivative"):
            autodiff.render_forward(textured, params, {k: torch.zeros_like(params[k])})
    with pytest.raises(KeyError):
        autodiff.render_forward(textured, params, {"nope.value": torch.zeros(3)})
    with pytest.raises(RuntimeError, match="RGB variant"):
        autodiff.render_forward(spectral, autodiff.traverse(spectral), {})


def test_traverse_emitters_adds_settable_colours_to_any_scene(gpu):
    from mitsuba2_amd import autodiff
    sd = _lit_box()
    sd["bsdfs"] = list(sd["bsdfs"]) + [dict(ROUGH, id="tall")]
    sd["meshes"][5] = dict(sd["meshes"][5], bsdf=len(sd["bsdfs"]) - 1)
    lamp = next(i for i, m in enumerate(sd["meshes"]) if m.get("emitter", -1) >= 0)
    sd["meshes"][lamp] = dict(sd["meshes"][lamp], id="lamp")
    for e, name in enumerate(["sky", "area", "bulb", "torch", "sun"]):
        sd["emitters"][e] = dict(sd["emitters"][e], id=name)
    p = scenes.cornell_box_sensor(16, 16, 4, seed=4, max_depth=5, rfilter="box")
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=5))
    before = set(autodiff.traverse(scene).keys())
    params = autodiff.traverse(scene, emitters=True)
    new = {"lamp.emitter.radiance.value", "sky.radiance.value", "bulb.intensity.value", "torch.intensity.value", "sun.irradiance.value"}
    assert set(params.keys()) == before | new and not before & new
    assert np.allclose(params["bulb.intensity.value"].cpu().numpy(), [2e5, 2e5, 3e5])
    # they round-trip through update(): the forward derivative along the new colours reproduces the render with them
    params["sky.radiance.value"] = [0.8, 0.2, 0.4]
    params["sun.irradiance.value"] = [2.0, 1.0, 3.0]
    autodiff._render_counter[id(scene)] = 0
    image = autodiff.render_forward(scene, params, {k: params[k] for k in new})
    autodiff._render_counter[id(scene)] = 0
    primal = autodiff.render(scene, params=params)
    assert float(primal.max()) > 0.1 and torch.allclose(image, primal, rtol=1e-5, atol=0)
    fresh = gpu.Scene(dict(sd, emitters=[dict(sd["emitters"][0], radiance=[0.8, 0.2, 0.4])] + sd["emitters"][1:4] + [dict(sd["emitters"][4], irradiance=[2.0, 1.0, 3.0])]),
                      sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=5))
    autodiff._render_counter[id(fresh)] = 0
    assert torch.equal(autodiff.render(fresh), primal)
    # no reverse-mode gradient outside diffuse area-lit scenes: render() says where the derivative is
    params["sun.irradiance.value"].requires_grad_(True)
    with pytest.raises(RuntimeError, match="render_forward"):
        autodiff.render(scene, params=params)

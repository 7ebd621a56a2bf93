"""Forward and reverse renders in scenes with textured BSDF parameters (MTSAMD_FORWARD_PARAM_TEXTURES / MTSAMD_REVERSE_PARAM_TEXTURES;
k_forward<FLAT, true>, k_reverse<FLAT, RECORD, true>; autodiff.render_forward / render(backward="fused") with param_maps=True).

The oracle knows constant parameters only, so the yardstick is the split construction of param_texel_scenes.py: a 2 x 9 map whose lookups
interpolate equal texels makes the textured scene `mine` the same render as the constant scene `theirs`.

 1. forward films of one-hot cell tangents, contracted with dimage, against the oracle's parameter adjoint (2e-3 |want| + 1e-5);
 2. the reverse render's map gradient: cell sums against the oracle at that bound, column 0 exactly 0, texel by texel against
    mtsamd_render_adjoint_param_textures (rtol 2e-2, atol 2e-3 max|g|), the luminance shares of an alpha map (1e-5);
 3. constants beside a map (eta, k of the mapped record, the floor's reflectance) against the oracle, from the reverse call and from
    one-hot forward films;
 4. the transpose identity <dimage, J t> = <J^T dimage, t> in a scene with non-uniform maps, roulette attached and detached;
 5. the attached roulette factor of the map texels against the plain k_forward on the constant scene (48 blocks: rtol 2e-2, atol 2e-3 max);
 6. the hierarchy instantiation at a launch edge against mtsamd_render_adjoint_param(ALPHA), and RECORD = false at max_depth 20;
 7. anisotropy (maps on alpha_u and alpha_v) and the pair rule (one map on alpha);
 8. a forward image against central differences of autodiff.render;
 9. opt-in and refusals, accumulation;
10. the Python surface.

Every check prints its worst deviation in units of its bound."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import param_texel_scenes as pts
from test_gpu_adjoint_param_textures import _box_scene, _constant_route, _grad, _sphere_scene
from test_gpu_adjoint_textures import _open_box, _primal, _scene, _sky, _tex_floats
from test_gpu_autodiff import _assert_close
from test_gpu_forward import _block_sums, _desc, _forward_film, _image, _primal_film, _tangent, _vp
from test_gpu_reverse import _dot, _random_dimage, _reverse, _within
from test_gpu_textured_params import CONDUCTOR_IOR

pytestmark = pytest.mark.gpu
F32 = np.float32
LUM = np.array([0.212671, 0.715160, 0.072169])
INVALID, UNSUPPORTED = -1, -5
REFLECTANCE, SPECULAR_REFLECTANCE, ETA, K, ALPHA, SPECULAR_TRANSMITTANCE = range(6)
DETACH, MAPS = 1, 2                  # MTSAMD_*_DETACH_ROULETTE, MTSAMD_*_PARAM_TEXTURES


def _tex_info(scene, idx):
    from mitsuba2_amd import _lib as L
    off, w, h = C.c_uint64(), C.c_int32(), C.c_int32()
    L.check(L.lib().mtsamd_scene_texture_info(scene._handle, int(idx), C.byref(w), C.byref(h), C.byref(off)))
    return off.value, w.value, h.value


def _texels(scene, flat, idx):
    off, w, h = _tex_info(scene, idx)
    return np.asarray(flat, np.float64)[off: off + 3 * w * h].reshape(h, w, 3)


def _tex_tangent(scene, entries):
    """the texture buffer (layout of grad_textures) holding the given (h, w, 3) tangents at their textures' slices, zero elsewhere"""
    flat = np.zeros(_tex_floats(scene), F32)
    for idx, t in entries.items():
        off, w, h = _tex_info(scene, idx)
        flat[off: off + 3 * w * h] = np.asarray(t, F32).reshape(h, w, 3).reshape(-1)
    return flat


def _cell_tangent(cell, comp):
    """1 on the columns of the cell, in channel comp (None: all three -- a roughness is the luminance of its texel, whose weights sum to 1)"""
    t = np.zeros((2, 9, 3), F32)
    if comp is None:
        t[:, pts.CELL_COLUMNS[cell]] = 1.0
    else:
        t[:, pts.CELL_COLUMNS[cell], comp] = 1.0
    return t


def _components(pname):
    return [(0, None)] if pname == "alpha" else [(c, c) for c in range(3)]


@functools.lru_cache(maxsize=None)
def _split(case):
    """the textured scene of a split case with its desc, primal film, record index and the textures of its maps; built once per case"""
    from mitsuba2_amd import autodiff, render as gpu
    mine, theirs, params = pts.split_scenes(case)
    p = pts.sensor_params()
    sensor = gpu.make_sensor(p)
    integ = gpu.PathIntegrator(max_depth=pts.MAX_DEPTH)
    scene = gpu.Scene(mine, sensor=sensor, integrator=integ)
    d = autodiff._desc(scene, sensor, integ, 8, pts.SEED)
    film = autodiff._render_film(scene, d)
    torch.cuda.synchronize()
    bsdf = len(mine["bsdfs"]) - 1
    textures = {pname: scene.texture_index(bsdf, pname) for pname in params}
    assert all(t is not None for t in textures.values())
    return dict(mine=mine, theirs=theirs, params=params, p=p, scene=scene, d=d, film=film, bsdf=bsdf, textures=textures)


@functools.lru_cache(maxsize=None)
def _split_reverse(case):
    """the whole texture-gradient buffer of ONE detached reverse call with the bit (every map of the case at once)"""
    s = _split(case)
    return _reverse(s["scene"], s["d"], pts.dimage(), s["film"], tex_floats=_tex_floats(s["scene"]), h=pts.H_STEP, flags=DETACH | MAPS)["tex"]


# ---- 1. forward against the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pts.SPLIT_CASES)
def test_forward_cell_tangents_match_the_oracle(gpu, oracle, case):
    """For every (parameter, cell, component) the forward film for the tangent that is 1 on that cell's columns, contracted with dimage
    through the film normalisation, is the oracle's derivative with respect to the constant of that cell: the same paths on both sides
    (the primal films agree first), two sums of the same terms -- 2e-3 |want| + 1e-5.  Roulette detached on both sides, h = H_STEP."""
    s = _split(case)
    film_o, wants = pts.oracle_wants(case)
    assert np.allclose(s["film"].cpu().numpy(), film_o, rtol=2e-5, atol=1e-6)
    got, want = [], []
    for pname in s["params"]:
        for cell in (0, 1):
            for comp, channel in _components(pname):
                tex = _tex_tangent(s["scene"], {s["textures"][pname]: _cell_tangent(cell, channel)})
                dfilm = _forward_film(s["scene"], s["d"], _tangent(s["scene"], tex=tex, h=pts.H_STEP, flags=DETACH | MAPS))
                got.append(_dot(dfilm, pts.dimage()))
                want.append(wants[(pname, cell, comp)])
    _within("%s: forward films of the cell tangents against the oracle" % case, got, want, floor=len(want))


# ---- 2. reverse against the oracle and the existing entry point ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", pts.SPLIT_CASES)
def test_reverse_map_gradient_matches_the_oracle_and_the_slot_replays(gpu, oracle, case):
    s = _split(case)
    _, wants = pts.oracle_wants(case)
    g = _split_reverse(case)
    every = _grad(s["scene"], s["d"], s["film"], torch.from_numpy(pts.dimage()).cuda(), -1, pts.H_STEP).cpu().numpy().astype(np.float64)
    got, want = [], []
    for pname in s["params"]:
        gt = _texels(s["scene"], g, s["textures"][pname])
        assert gt.shape == (2, 9, 3)
        assert np.all(gt[:, 0] == 0.0), (case, pname, gt[:, 0])            # no lookup touches column 0
        for cell, cols in enumerate(pts.CELL_COLUMNS):
            for comp, channel in _components(pname):
                got.append(float(gt[:, cols].sum() if channel is None else gt[:, cols, channel].sum()))
                want.append(wants[(pname, cell, comp)])
        _assert_close("%s %s: texel by texel against mtsamd_render_adjoint_param_textures" % (case, pname), gt, _texels(s["scene"], every, s["textures"][pname]))
        if pname == "alpha":      # the roughness is the luminance of the texel: the channels share the gradient in that ratio
            ch = gt.sum((0, 1))
            dev = np.abs(ch / ch.sum() - LUM) / (1e-5 * LUM)
            print("%s alpha channel shares: worst deviation %.3g of the bound" % (case, float(dev.max())))
            assert (dev <= 1).all(), (case, (ch / ch.sum()).tolist())
    _within("%s: cell sums of the reverse map gradient against the oracle" % case, got, want, floor=len(want))
    # the buffer outside the maps' slices holds the reflectance family only: nothing here (no bitmap reflectance in these scenes)
    mask = np.ones(g.size, bool)
    for t in s["textures"].values():
        off, w, h = _tex_info(s["scene"], t)
        mask[off: off + 3 * w * h] = False
    assert not g[mask].any()


# ---- 3. constants beside a map ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rough_ggx_alpha", "conductor_colour"])
def test_constants_beside_a_map_match_the_oracle(gpu, oracle, case):
    """eta and k of the mapped record (the oracle moves them on both halves of the box, meshes 7 and 8 together) and the floor's
    reflectance: from the reverse call with the bit, and from one-hot forward films contracted with dimage."""
    s = _split(case)
    scene, d, film = s["scene"], s["d"], s["film"]
    S = oracle.OracleScene(s["theirs"])
    desc = oracle.make_desc(pts.sensor_params(), analytic=True, film_rgb=True)
    film_o, _ = pts.oracle_wants(case)
    di = pts.dimage()
    tall, floor = s["bsdf"], s["bsdf"] - 1
    wanted = [(tall, kind, c) for kind in (ETA, K) for c in range(3)] + [(floor, REFLECTANCE, c) for c in range(3)]
    want = [S.render_adjoint_param(desc, di, film_o, [7, 8] if b == tall else [0], kind, c, pts.H_STEP) for (b, kind, c) in wanted]
    assert all(abs(w) > 1e-3 for w in want), want
    g = _reverse(scene, d, di, film, wanted=wanted, h=pts.H_STEP, flags=DETACH | MAPS)["bsdf"]
    _within("%s: reverse, constants beside the map" % case, [g[b, 3 * kind + c] for (b, kind, c) in wanted], want, floor=len(want))
    fwd = [_dot(_forward_film(scene, d, _tangent(scene, bsdf={w: 1.0}, h=pts.H_STEP, flags=DETACH | MAPS)), di) for w in wanted]
    _within("%s: forward, constants beside the map" % case, fwd, want, floor=len(want))


# ---- 4. transpose identity with non-uniform maps --------------------------------------------------------------------------------------------
def _mapped_box(gpu, mat, w=32, h=24, spp=8, max_depth=7, seed=21):
    """Cornell box with a bitmap reflectance on the floor and the back wall, whose tall box carries `mat` and random texcoords"""
    from mitsuba2_amd import scenes
    rng = np.random.RandomState(11)
    cb = scenes.cornell_box(texture=rng.uniform(0.2, 0.8, (5, 4, 3)).astype(F32))
    box = dict(cb["meshes"][7], texcoords=np.random.default_rng(4).uniform(0, 1, size=(24, 2)).astype(F32), bsdf=len(cb["bsdfs"]))
    sd = dict(cb, bsdfs=list(cb["bsdfs"]) + [mat], meshes=cb["meshes"][:7] + [box])
    p, scene = _scene(gpu, sd, w, h, spp, max_depth, seed=seed)
    return sd, p, scene


@pytest.mark.parametrize("detach", [True, False], ids=["detached", "attached"])
def test_transpose_identity_with_random_maps(gpu, detach):
    """An alpha map and a specular_reflectance map of random texels on the tall box (random texcoords), a bitmap reflectance on the floor
    and the back wall, the lamp; rr_depth 2.  ONE random tangent over all map texels, reflectance texels, colour constants and the lamp:
    <dimage, J t> against <J^T dimage, t>.  eta and k of the mapped record are nonlinear: one-hot, so both sides take the same step."""
    from mitsuba2_amd import bsdfs as B
    rng = np.random.RandomState(6)
    mat = dict(type="roughconductor", distribution="ggx", id="tall", alpha={"type": "bitmap", "data": rng.uniform(0.15, 0.4, (3, 4, 3)).astype(F32)},
               specular_reflectance={"type": "bitmap", "data": rng.uniform(0.3, 0.9, (2, 5, 3)).astype(F32)}, **CONDUCTOR_IOR)
    sd, p, scene = _mapped_box(gpu, mat)
    tall = len(sd["bsdfs"]) - 1
    assert scene.texture_index(tall, "alpha") is not None and scene.texture_index(tall, "specular_reflectance") is not None
    d = _desc(scene, p, rr_depth=2)
    film = _primal_film(scene, d)
    dimage = _random_dimage(24, 32)
    flags = MAPS | (DETACH if detach else 0)
    h = 0.01
    linear = [(b, REFLECTANCE, c) for b, rec in enumerate(scene._bsdf_records) if rec["type"] == B.DIFFUSE and not isinstance(rec["reflectance"], dict)
              for c in range(3)]
    nonlinear = [(tall, kind, c) for kind in (ETA, K) for c in range(3)]
    n_tex = _tex_floats(scene)
    g = _reverse(scene, d, dimage, film, wanted=linear + nonlinear, emitters=True, tex_floats=n_tex, h=h, flags=flags)
    t_bsdf = {w: float(rng.uniform(0.5, 1.0)) for w in linear}
    t_em = rng.uniform(0.5, 2.0, (len(sd["emitters"]), 3)).astype(F32)
    t_tex = rng.uniform(-1.0, 1.0, n_tex).astype(F32)
    fwd = _dot(_forward_film(scene, d, _tangent(scene, bsdf=t_bsdf, emitters=t_em, tex=t_tex, h=h, flags=flags)), dimage)
    parts = {"constants": sum(g["bsdf"][b, 3 * kind + c] * t for (b, kind, c), t in t_bsdf.items()), "lamp": float((g["emitters"] * t_em).sum()),
             "texels": float((g["tex"] * t_tex.astype(np.float64)).sum())}
    print("parts of <J^T dimage, t>: %s" % parts)
    assert all(abs(v) > 1e-3 for v in parts.values()), parts
    for name in ("alpha", "specular_reflectance"):
        assert np.abs(_texels(scene, g["tex"], scene.texture_index(tall, name))).max() > 1e-3
    _within("one tangent over map texels, reflectance texels, constants and the lamp (%s)" % ("detached" if detach else "attached"),
            sum(parts.values()), fwd, floor=1)
    got = [g["bsdf"][b, 3 * kind + c] for (b, kind, c) in nonlinear]
    want = [_dot(_forward_film(scene, d, _tangent(scene, bsdf={w: 1.0}, h=h, flags=flags)), dimage) for w in nonlinear]
    _within("eta and k of the mapped record, one-hot", got, want, floor=3)


# ---- 5. attached roulette against the plain kernels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pts.SPLIT_CASES)
def test_attached_roulette_matches_the_plain_forward_render_of_the_constant_scene(gpu, case):
    """rr_depth 2, roulette attached: the forward film of `mine` for a one-hot cell tangent against the forward film of `theirs` from
    today's plain k_forward, with the one-hot constant on that cell's record and the same h.  48 blocks of 4 x 4 pixels."""
    s = _split(case)
    p = s["p"]
    theirs = gpu.Scene(s["theirs"], sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=pts.MAX_DEPTH))
    d_m, d_t = _desc(s["scene"], p, rr_depth=2, sample_count=8), _desc(theirs, p, rr_depth=2, sample_count=8)
    assert len(_block_sums(np.zeros((24, 32, 3)), size=4)) == 48
    for pname in s["params"]:
        for cell in (0, 1):
            for comp, channel in _components(pname):
                tex = _tex_tangent(s["scene"], {s["textures"][pname]: _cell_tangent(cell, channel)})
                mine = _forward_film(s["scene"], d_m, _tangent(s["scene"], tex=tex, h=pts.H_STEP, flags=MAPS))
                want = _forward_film(theirs, d_t, _tangent(theirs, bsdf={(s["bsdf"] + cell, pts.KIND[pname], comp): 1.0}, h=pts.H_STEP))
                want_b = _block_sums(_image(want), size=4)
                assert np.abs(want_b).max() > 1e-3
                _assert_close("%s %s cell %d comp %d: attached forward films, 48 blocks" % (case, pname, cell, comp), _block_sums(_image(mine), size=4), want_b)


# ---- 6. hierarchy scenes, a launch edge -----------------------------------------------------------------------------------------------------
def test_hierarchy_scene_uniform_map_matches_the_constant_route(gpu):
    """k_forward<false, true> and k_reverse<false, true, true> on a film whose sample count is no multiple of the wavefront: the reverse
    map gradient of a uniform grey 3 x 4 roughness map sums to, and <dimage, forward film> of the all-ones tangent equals, the derivative
    with respect to the constant (mtsamd_render_adjoint_param, same h, same paths): 2e-3 |want|.  max_depth 7 > rr_depth."""
    grey, h = 0.25, 0.01
    p, scene_t = _sphere_scene(gpu, {"type": "bitmap", "data": np.full((3, 4, 3), grey, F32)})
    d, film = _primal(scene_t, p)
    di = np.random.RandomState(3).uniform(0.0, 1.0, (19, 25, 3)).astype(F32)
    p, scene_c = _sphere_scene(gpu, grey)
    d_c, film_c = _primal(scene_c, p)
    want = _constant_route(scene_c, d_c, film_c, torch.from_numpy(di).cuda(), 0, ALPHA, 0, h)
    assert abs(want) > 1e-2
    g = _reverse(scene_t, d, di, film, tex_floats=_tex_floats(scene_t), h=h, flags=DETACH | MAPS)["tex"]
    got_r = float(g.sum())
    got_f = _dot(_forward_film(scene_t, d, _tangent(scene_t, tex=np.ones(_tex_floats(scene_t), F32), h=h, flags=DETACH | MAPS)), di)
    for what, got in (("reverse", got_r), ("forward", got_f)):
        print("hierarchy, %s: got %.7g want %.7g, %.3g of the bound" % (what, got, want, abs(got - want) / (2e-3 * abs(want))))
        assert abs(got - want) <= 2e-3 * abs(want), (what, got, want)


def test_emitter_and_envmap_gradients_alone_run_at_any_depth(gpu):
    """RECORD = false, NEST = true: the lamp and the texels of an envmap at max_depth 20 in a scene with a roughness map, against the
    forward render along a random tangent; a texel gradient at that depth is refused."""
    from mitsuba2_amd import scenes
    sd = scenes.bumpy_sphere(4, 11)
    sphere = dict(sd["meshes"][0], texcoords=np.random.default_rng(8).uniform(0.0, 1.0, size=(sd["meshes"][0]["positions"].shape[0], 2)).astype(F32))
    mat = dict(type="roughconductor", distribution="ggx", alpha={"type": "bitmap", "data": np.random.RandomState(2).uniform(0.1, 0.4, (3, 4, 3)).astype(F32)},
               **CONDUCTOR_IOR)
    sd = dict(sd, meshes=[sphere] + sd["meshes"][1:], bsdfs=[mat] + sd["bsdfs"][1:], emitters=list(sd["emitters"]) + [_sky()])
    p = scenes.bumpy_sphere_sensor(25, 19, spp=3, seed=5, max_depth=20)
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=20))
    assert scene.info()["primitives"] > 64
    d = _desc(scene, p, rr_depth=3)
    film = _primal_film(scene, d)
    di = _random_dimage(19, 25)
    g = _reverse(scene, d, di, film, emitters=True, env_shape=(6, 10, 3), flags=MAPS)
    rng = np.random.RandomState(9)
    t_em, t_env = rng.uniform(0.5, 2.0, (2, 3)).astype(F32), rng.uniform(0.5, 2.0, (6, 10, 3)).astype(F32)
    fwd = _dot(_forward_film(scene, d, _tangent(scene, emitters=t_em, env=t_env, flags=MAPS)), di)
    rev = float((g["emitters"] * t_em).sum() + (g["env"] * t_env).sum())
    assert np.abs(g["emitters"][0]).max() > 1e-3 and np.abs(g["env"]).max() > 1e-3 and not g["emitters"][1].any()
    _within("lamp and envmap texels at max_depth 20 (RECORD = false)", rev, fwd, floor=1)
    assert "max_depth <= 16" in _reverse(scene, d, di, film, tex_floats=_tex_floats(scene), flags=MAPS, expect=UNSUPPORTED)


# ---- 7. anisotropy and the pair rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["separate", "pair"])
def test_anisotropic_maps_and_the_pair_rule(gpu, which):
    """Maps of random texels on alpha_u and alpha_v (separate), or one on alpha (one parameter: both roughnesses move together): the
    reverse texel gradients against mtsamd_render_adjoint_param_textures, and the forward / reverse transpose identity."""
    rng = np.random.RandomState(12)
    base = dict(type="roughconductor", distribution="ggx", id="tall", **CONDUCTOR_IOR)
    if which == "separate":
        mat = dict(base, alpha_u={"type": "bitmap", "data": rng.uniform(0.2, 0.4, (3, 4, 3)).astype(F32)},
                   alpha_v={"type": "bitmap", "data": rng.uniform(0.2, 0.4, (2, 5, 3)).astype(F32)})
        names = ("alpha_u", "alpha_v")
    else:
        mat = dict(base, alpha={"type": "bitmap", "data": rng.uniform(0.2, 0.4, (3, 4, 3)).astype(F32)})
        names = ("alpha",)
    p, scene = _box_scene(gpu, mat)
    index = len(scene._bsdf_records) - 1
    d, film = _primal(scene, p)
    di = np.random.RandomState(3).uniform(0.0, 1.0, (24, 32, 3)).astype(F32)
    h, n_tex = 0.003, _tex_floats(scene)
    g = _reverse(scene, d, di, film, tex_floats=n_tex, h=h, flags=DETACH | MAPS)["tex"]
    every = _grad(scene, d, film, torch.from_numpy(di).cuda(), -1, h).cpu().numpy().astype(np.float64)
    for name in names:
        t = scene.texture_index(index, name)
        assert np.abs(_texels(scene, every, t)).max() > 1e-3
        _assert_close("%s: texel by texel against mtsamd_render_adjoint_param_textures" % name, _texels(scene, g, t), _texels(scene, every, t))
    t_tex = rng.uniform(-1.0, 1.0, n_tex).astype(F32)
    fwd = _dot(_forward_film(scene, d, _tangent(scene, tex=t_tex, h=h, flags=DETACH | MAPS)), di)
    _within("%s: transpose identity" % which, float((g * t_tex.astype(np.float64)).sum()), fwd, floor=1)


# ---- 8. finite differences ------------------------------------------------------------------------------------------------------------------
def test_forward_image_against_central_differences(gpu):
    """A conductor floor (and back wall) with a 6 x 6 specular_reflectance bitmap under an envmap and a point light, max_depth 4 below
    rr_depth: with common random numbers the image is a polynomial in the texels, and the central difference of autodiff.render after
    Scene.update_texture(+- 0.02 t) checks the forward image for the random tangent t: 1e-2 |fd| + 1e-5."""
    from mitsuba2_amd import autodiff
    rng = np.random.RandomState(3)
    tex = (0.3 + 0.5 * rng.rand(6, 6, 3)).astype(F32)
    floor = dict(type="conductor", specular_reflectance={"type": "bitmap", "data": tex}, **CONDUCTOR_IOR)
    sd = _open_box(tex, floor, emitters=[_sky(), {"type": "point", "position": [278, 450, 279], "intensity": [2e5, 2e5, 3e5]}])
    p, scene = _scene(gpu, sd, 32, 32, 8, 4, rfilter="gaussian")
    params = autodiff.traverse(scene)
    key = "textured.specular_reflectance.data"
    assert key in params
    texture = params._kind[key][1]
    t = rng.uniform(-1.0, 1.0, (6, 6, 3)).astype(F32)
    weights = torch.from_numpy(np.random.RandomState(5).uniform(0.0, 1.0, 32 * 32 * 3).astype(F32)).cuda() / (32 * 32)
    autodiff._render_counter[id(scene)] = 7
    image = autodiff.render_forward(scene, params, {key: torch.from_numpy(t)}, param_maps=True)
    assert image.shape == (32 * 32 * 3,) and float(image.abs().max()) > 1e-2
    got = float((image.double() * weights.double()).sum().item())
    losses = []
    for sign in (1.0, -1.0):
        scene.update_texture(texture, tex + F32(sign * 0.02) * t)
        autodiff._render_counter[id(scene)] = 7
        with torch.no_grad():
            losses.append(float((autodiff.render(scene).double() * weights.double()).sum().item()))
    scene.update_texture(texture, tex)
    fd = (losses[0] - losses[1]) / 0.04
    print("forward %.6g, central difference %.6g, %.3g of the bound" % (got, fd, abs(got - fd) / (1e-2 * abs(fd) + 1e-5)))
    assert abs(fd) > 1e-3
    assert abs(got - fd) <= 1e-2 * abs(fd) + 1e-5, (got, fd)


# ---- 9. opt-in and refusals -----------------------------------------------------------------------------------------------------------------
def test_opt_in_refusals_and_accumulation(gpu):
    from mitsuba2_amd import _lib as L, scenes
    lib = L.lib()
    assert (L.FORWARD_PARAM_TEXTURES, L.REVERSE_PARAM_TEXTURES) == (MAPS, MAPS)
    amap = {"type": "bitmap", "data": np.full((2, 2, 3), 0.2, F32)}
    cmap = {"type": "bitmap", "data": np.full((2, 3, 3), 0.8, F32)}
    p, scene = _box_scene(gpu, dict(type="roughconductor", alpha=amap, specular_reflectance=cmap, **CONDUCTOR_IOR), max_depth=3)
    tall = len(scene._bsdf_records) - 1
    d, film = _primal(scene, p)
    di = _random_dimage(24, 32)
    n_tex = _tex_floats(scene)
    out = torch.zeros((24, 32, 5), device="cuda")
    ones = np.ones(n_tex, F32)

    def forward_refused(sc, d_, td, code, text):
        for rc in (lib.mtsamd_render_forward(sc._handle, C.byref(d_), C.byref(td[0]), _vp(out), None),
                   lib.mtsamd_sample_forward(sc._handle, C.byref(d_), C.byref(td[0]), 0, 4, _vp(out), None, None)):
            assert rc == code and text in lib.mtsamd_last_error().decode(), (rc, lib.mtsamd_last_error(), text)

    # without the bit: today's refusal; an unknown bit beside it: refused
    for flags in (0, DETACH):
        forward_refused(scene, d, _tangent(scene, tex=ones, flags=flags), UNSUPPORTED, "does not handle textured BSDF parameters")
        assert "does not handle textured BSDF parameters" in _reverse(scene, d, di, film, tex_floats=n_tex, flags=flags, expect=UNSUPPORTED)
    forward_refused(scene, d, _tangent(scene, tex=ones, flags=MAPS | 4), INVALID, "unknown flag bits")
    assert "unknown flag bits" in _reverse(scene, d, di, film, tex_floats=n_tex, flags=MAPS | 4, expect=INVALID)
    # a tangent / wanted flag on a parameter the record reads from a texture: refused by name
    for kind, name in ((ALPHA, "alpha"), (SPECULAR_REFLECTANCE, "specular_reflectance")):
        text = "bsdf %d: %s holds a texture" % (tall, name)
        forward_refused(scene, d, _tangent(scene, bsdf={(tall, kind, 0): 1.0}, flags=MAPS), UNSUPPORTED, text)
        assert text in _reverse(scene, d, di, film, wanted=[(tall, kind, 0)], flags=MAPS, expect=UNSUPPORTED)
    for binding, kind, name in (("alpha_u", ALPHA, "alpha_u"), ("alpha_v", ALPHA, "alpha_v"), ("specular_transmittance", SPECULAR_TRANSMITTANCE, "specular_transmittance")):
        mat = dict(type="roughdielectric", alpha=0.2, **{binding: cmap if kind != ALPHA else amap})
        if kind == ALPHA:
            mat.pop("alpha")
            mat["alpha_v" if binding == "alpha_u" else "alpha_u"] = 0.2
        p_b, scene_b = _box_scene(gpu, mat, max_depth=3)
        d_b, film_b = _primal(scene_b, p_b)
        text = "bsdf %d: %s holds a texture" % (tall, name)
        forward_refused(scene_b, d_b, _tangent(scene_b, bsdf={(tall, kind, 0): 1.0}, flags=MAPS), UNSUPPORTED, text)
        assert text in _reverse(scene_b, d_b, di, film_b, wanted=[(tall, kind, 0)], flags=MAPS, expect=UNSUPPORTED)
    # blend and spectral scenes stay refused with the bit
    blend = {"type": "blendbsdf", "weight": 0.3, "bsdf_1": {"type": "diffuse", "reflectance": [0.2, 0.5, 0.7]}, "bsdf_0": dict(type="roughconductor", alpha=amap, **CONDUCTOR_IOR)}
    p_b, scene_b = _box_scene(gpu, blend, max_depth=3)
    d_b, film_b = _primal(scene_b, p_b)
    forward_refused(scene_b, d_b, _tangent(scene_b, tex=np.ones(_tex_floats(scene_b), F32), flags=MAPS), UNSUPPORTED, "blendbsdf / mask")
    assert "blendbsdf / mask" in _reverse(scene_b, d_b, di, film_b, tex_floats=_tex_floats(scene_b), flags=MAPS, expect=UNSUPPORTED)
    # (a spectral scene cannot hold a textured parameter -- its creation refuses the binding -- so the bit is the unknown bit there)
    p_s, scene_s = _scene(gpu, scenes.cornell_box(), 32, 24, 8, 3, variant="spectral")
    d_s = _desc(scene_s, p_s)
    forward_refused(scene_s, d_s, _tangent(scene_s, emitters=np.ones((1, 3), F32), flags=MAPS), INVALID, "unknown flag bits")
    forward_refused(scene_s, d_s, _tangent(scene_s, emitters=np.ones((1, 3), F32)), UNSUPPORTED, "RGB variant only")
    assert "unknown flag bits" in _reverse(scene_s, d_s, di, film, emitters=True, flags=MAPS, expect=INVALID)
    assert "RGB variant only" in _reverse(scene_s, d_s, di, film, emitters=True, expect=UNSUPPORTED)
    # a scene without textured parameters: the bit has no meaning there and stays the unknown bit it is today (test_gpu_forward.py and
    # test_gpu_reverse.py pin that), so nothing such a scene computes can depend on it
    p_p, plain = _scene(gpu, scenes.cornell_box(), 32, 24, 8, 3)
    d_p, film_p = _primal(plain, p_p)
    forward_refused(plain, d_p, _tangent(plain, emitters=np.ones((1, 3), F32), flags=MAPS), INVALID, "unknown flag bits")
    assert "unknown flag bits" in _reverse(plain, d_p, di, film_p, emitters=True, flags=MAPS, expect=INVALID)
    # two reverse calls accumulate to twice one call
    wanted = [(tall, ETA, 0), (tall, K, 1)]
    one = _reverse(scene, d, di, film, wanted=wanted, emitters=True, tex_floats=n_tex, h=0.01, flags=MAPS)
    buf = _reverse(scene, d, di, film, wanted=wanted, emitters=True, tex_floats=n_tex, h=0.01, flags=MAPS, into={})
    buf = _reverse(scene, d, di, film, wanted=wanted, emitters=True, tex_floats=n_tex, h=0.01, flags=MAPS, into=buf)
    for k, v in one.items():
        assert np.abs(v).max() > 0 and np.allclose(buf[k].cpu().numpy(), 2 * v, rtol=1e-5, atol=1e-5 * np.abs(v).max()), k


# ---- 10. Python -------------------------------------------------------------------------------------------------------------------------------
def test_python_surface(gpu):
    from mitsuba2_amd import autodiff
    case = "rough_ggx_alpha"
    s = _split(case)
    scene = s["scene"]
    params = autodiff.traverse(scene, emitters=True)
    params.fd_step = pts.H_STEP
    akey, ekey = "tall.alpha.data", "tall.eta.value"
    lkey = next(k for k in params.keys() if params._kind[k][0] == "emitter")
    assert akey in params and ekey in params
    # render_forward: refused without the keyword, the film of test 1 with it
    with pytest.raises(RuntimeError, match="no forward-mode derivative"):
        autodiff.render_forward(scene, params, {akey: torch.zeros(2, 9, 3)})
    t = _cell_tangent(1, None)
    autodiff._render_counter[id(scene)] = 0
    image = autodiff.render_forward(scene, params, {akey: torch.from_numpy(t)}, detach_roulette=True, param_maps=True).cpu().numpy().reshape(24, 32, 3)
    want = _image(_forward_film(scene, s["d"], _tangent(scene, tex=_tex_tangent(scene, {s["textures"]["alpha"]: t}), h=pts.H_STEP, flags=DETACH | MAPS)))
    assert np.abs(want).max() > 1e-3 and np.allclose(image, want, rtol=1e-5, atol=1e-6 * np.abs(want).max())
    # fused backward with the keyword against the families on the map's texels
    di = torch.from_numpy(pts.dimage()).cuda().reshape(-1)

    def grads(keys, **kwargs):
        for k, v in params.items():
            v.requires_grad_(k in keys)
            v.grad = None
        autodiff._render_counter[id(scene)] = 0
        (autodiff.render(scene, params=params, **kwargs) * di).sum().backward()
        return {k: params[k].grad.detach().cpu().numpy().astype(np.float64) for k in keys}

    fam = grads([akey])
    fused = grads([akey], backward="fused", detach_roulette=True, param_maps=True)
    _assert_close("alpha.data: fused with param_maps against the families", fused[akey], fam[akey])
    # a mixed key set in one call: finite, non-zero, and what the C-level calls of tests 2 and 3 give
    with pytest.raises(RuntimeError, match="textured BSDF parameters"):
        grads([akey, ekey, lkey], backward="fused", detach_roulette=True)
    mixed = grads([akey, ekey, lkey], backward="fused", detach_roulette=True, param_maps=True)
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in mixed.values())
    ref = _reverse(scene, s["d"], pts.dimage(), s["film"], wanted=[(s["bsdf"], ETA, c) for c in range(3)], emitters=True, tex_floats=_tex_floats(scene),
                   h=pts.H_STEP, flags=DETACH | MAPS)
    _assert_close("mixed keys: alpha.data", mixed[akey], _texels(scene, ref["tex"], s["textures"]["alpha"]))
    _assert_close("mixed keys: eta", mixed[ekey], ref["bsdf"][s["bsdf"], 3 * ETA: 3 * ETA + 3])
    _assert_close("mixed keys: the lamp", mixed[lkey], ref["emitters"][params._kind[lkey][1]])
    for v in params.properties.values():
        v.requires_grad_(False)
    # in a scene without textured parameters the keyword is inert: the same film, bit for bit
    plain = gpu.Scene(s["theirs"], sensor=gpu.make_sensor(s["p"]), integrator=gpu.PathIntegrator(max_depth=pts.MAX_DEPTH))
    pp = autodiff.traverse(plain)
    key = next(k for k in pp.keys() if k.endswith(".eta.value"))
    films = []
    for maps in (False, True):
        autodiff._render_counter[id(plain)] = 0
        films.append(autodiff.render_forward(plain, pp, {key: torch.ones(3)}, param_maps=maps))
    assert float(films[0].abs().max()) > 0 and torch.equal(films[0], films[1])

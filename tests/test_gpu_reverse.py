"""The reverse-mode render (mtsamd_render_reverse, k_reverse; autodiff.render(backward="fused")): one path replay and one dLoss/dImage
give the gradient of every parameter the forward-mode render takes a tangent for.

The checker is the forward mode itself: for any dimage and tangent t, <dimage, J t> of mtsamd_render_forward equals <J^T dimage, t> of
the new call, at the project's bound for forward against mtsamd_render_adjoint_param, 2e-3 |want| + 1e-5.  Beside it stand the existing
adjoints of the same convention, the oracle, and -- for emitter colours -- plain primal renders lit by one emitter, which involve no
derivative code at all (_assert_close of test_gpu_autodiff.py: rtol 2e-2, atol 2e-3 max|want|).  Every test prints its worst deviation in
units of its bound.

1. transpose identity with the roulette factor held fixed and differentiated;   2. the existing adjoints and the oracle;
3. emitter colours against primal renders;   4. RECORD = false at any depth, and the depth limit of RECORD = true;   5. launch edges;
6. both sides of the two LDS bin capacities;   7. delta lobes;   8. accumulation;   9. autodiff.render(backward="fused").
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import flat_limits
from mitsuba2_amd import scenes
from test_bvh_depth_cpu import hierarchy_scene, hierarchy_sensor
from test_gpu_autodiff import _assert_close, _material_scene
from test_gpu_forward import (PLASTIC, ROUGH, _block_sums, _blocks, _desc, _emitter_colours, _forward_film, _image, _indicator, _lit_box, _primal_film,
                              _tangent, _textured_box, _vp)

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
REFLECTANCE, SPECULAR_REFLECTANCE, ETA, K, ALPHA, SPECULAR_TRANSMITTANCE = range(6)
CONDUCTOR = {"type": "conductor", "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14], "specular_reflectance": [0.9, 0.8, 0.7]}
DIELECTRIC = {"type": "dielectric", "int_ior": 1.5, "specular_reflectance": [0.9, 0.8, 0.7], "specular_transmittance": [0.7, 0.9, 0.8]}
SLOT_BINS = int(re.search(r"kReverseSlotBins = (\d+)u", open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mitsuba2_amd", "csrc", "kernels.h")).read()).group(1))


def _accepted(scene):
    """every (record, kind, component) mtsamd_render_adjoint_param accepts in this scene, from the types of its records"""
    from mitsuba2_amd import bsdfs as B
    kinds = {B.DIFFUSE: (REFLECTANCE,), B.PLASTIC: (REFLECTANCE, SPECULAR_REFLECTANCE), B.ROUGHPLASTIC: (REFLECTANCE, SPECULAR_REFLECTANCE),
             B.CONDUCTOR: (SPECULAR_REFLECTANCE, ETA, K), B.ROUGHCONDUCTOR: (SPECULAR_REFLECTANCE, ETA, K, ALPHA),
             B.DIELECTRIC: (SPECULAR_REFLECTANCE, SPECULAR_TRANSMITTANCE), B.ROUGHDIELECTRIC: (SPECULAR_REFLECTANCE, SPECULAR_TRANSMITTANCE, ALPHA),
             B.THINDIELECTRIC: (SPECULAR_REFLECTANCE, SPECULAR_TRANSMITTANCE)}
    out = []
    for b, rec in enumerate(scene._bsdf_records):
        for kind in kinds[rec["type"]]:
            if kind == REFLECTANCE and isinstance(rec["reflectance"], dict):
                continue
            out += [(b, kind, c) for c in range(1 if kind == ALPHA else 3)]
    return out


def _reverse(scene, d, dimage, film, wanted=(), emitters=False, tex_floats=0, env_shape=None, h=0.0, flags=0, into=None, expect=0):
    """one mtsamd_render_reverse call; returns {"bsdf": (n, 18), "emitters": (n, 3), "tex": flat, "env": (h, w, 3)} of what was asked for
    (float64 numpy), or the error text if `expect` is an error code.  `into`: device buffers of an earlier call, accumulated into."""
    from mitsuba2_amd import _lib as L
    n_bsdf = len(scene._bsdf_records)
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
    di = dimage if isinstance(dimage, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dimage, np.float32)).cuda()
    rc = L.lib().mtsamd_render_reverse(scene._handle, C.byref(d), _vp(di), _vp(film), C.byref(gd), None)
    if expect:
        assert rc == expect, (rc, L.lib().mtsamd_last_error())
        return L.lib().mtsamd_last_error().decode()
    L.check(rc)
    torch.cuda.synchronize()
    if into is not None:
        return buf
    return {k: v.cpu().numpy().astype(np.float64) for k, v in buf.items()}


def _dot(dfilm, dimage):
    return float((_image(dfilm) * np.asarray(dimage, np.float64)).sum())


def _within(what, got, want, floor=0):
    """|got - want| <= 2e-3 |want| + 1e-5 entry by entry: the bound of forward against mtsamd_render_adjoint_param"""
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    dev = np.abs(got - want) / (2e-3 * np.abs(want) + 1e-5)
    print("%s: worst deviation %.3g of the bound over %d entries, %d of them above 1e-3" % (what, float(dev.max()), want.size, int((np.abs(want) > 1e-3).sum())))
    assert (dev < 1).all(), (what, float(dev.max()), got[dev >= 1], want[dev >= 1])
    assert (np.abs(want) > 1e-3).sum() >= floor, (what, want)


def _random_dimage(h, w, seed=4):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, (h, w, 3)).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# 1. transpose identity

@pytest.mark.parametrize("detach", [True, False], ids=["detached", "attached"])
def test_transpose_identity_of_the_forward_render(gpu, detach):
    """Every accepted scalar of every record and the lamp, wanted at once.  The seven nonlinear scalars (alpha, eta, k of the
    roughconductor) against one-hot forward renders with the same step and flag; the colour constants and the lamp against ONE forward
    render along a random tangent.  At least half of the values compared exceed 1e-3 (on the oracle's side, render_adjoint_param with
    this dimage and seed, the seven nonlinear values range from 5.7e-3 to 0.27 in magnitude and all 21 colour values exceed 0.05)."""
    from mitsuba2_amd import _lib as L
    W, H = 40, 32
    sd, p, scene = _material_scene(gpu, (ROUGH, PLASTIC), w=W, h=H, spp=16, max_depth=5)
    d = _desc(scene, p, rr_depth=2)
    film = _primal_film(scene, d)
    dimage = _random_dimage(H, W)
    flag = L.REVERSE_DETACH_ROULETTE if detach else 0
    assert L.REVERSE_DETACH_ROULETTE == L.FORWARD_DETACH_ROULETTE
    wanted = _accepted(scene)
    tall = len(sd["bsdfs"]) - 2
    nonlinear = [(tall, ALPHA, 0)] + [(tall, kind, c) for kind in (ETA, K) for c in range(3)]
    linear = [w for w in wanted if w not in nonlinear]
    assert len(wanted) == 3 * (len(sd["bsdfs"]) - 2) + 10 + 6 and all(w in wanted for w in nonlinear)
    g = _reverse(scene, d, dimage, film, wanted=wanted, emitters=True, flags=flag)
    got = [g["bsdf"][b, 3 * kind + c] for (b, kind, c) in nonlinear]
    want = [_dot(_forward_film(scene, d, _tangent(scene, bsdf={w: 1.0}, flags=flag)), dimage) for w in nonlinear]
    _within("nonlinear scalars, %s" % ("detached" if detach else "attached"), got, want, floor=4)
    rng = np.random.RandomState(8)
    t_bsdf = {w: float(rng.uniform(0.5, 1.0)) for w in linear}
    t_em = rng.uniform(0.5, 2.0, (len(sd["emitters"]), 3)).astype(np.float32)
    fwd = _dot(_forward_film(scene, d, _tangent(scene, bsdf=t_bsdf, emitters=t_em, flags=flag)), dimage)
    rev = sum(g["bsdf"][b, 3 * kind + c] * t for (b, kind, c), t in t_bsdf.items()) + float((g["emitters"] * t_em).sum())
    _within("colour constants and the lamp along one tangent", rev, fwd, floor=1)
    lin = np.array([g["bsdf"][b, 3 * kind + c] for (b, kind, c) in linear] + list(g["emitters"].reshape(-1)))
    assert (np.abs(lin) > 1e-3).sum() >= lin.size // 2, lin
    # the entries nobody wanted stay zero
    unwanted = np.ones_like(g["bsdf"], bool)
    for (b, kind, c) in wanted:
        unwanted[b, 3 * kind + c] = False
    assert not g["bsdf"][unwanted].any()


def test_transpose_identity_where_the_throughput_has_zero_channels(gpu):
    """Cornell box with walls of reflectance (r, 0, 0) and (0, g, 0); only the three components of the first are wanted, no emitter
    gradient.  Behind that wall the throughput is 0 in green and blue, so the emitter sample at the next surface contributes nothing to
    the radiance -- but d radiance / d (green component of the wall) is exactly that sample's mis bv spec: the replay has to trace its
    shadow ray and record Nc there, as k_forward (dthr != 0) and GeneralRecorder (nc != 0) do."""
    W, H = 32, 32
    sd = scenes.cornell_box()
    sd["bsdfs"][1] = dict(sd["bsdfs"][1], reflectance=np.array([0.6, 0.0, 0.0], np.float32))
    sd["bsdfs"][2] = dict(sd["bsdfs"][2], reflectance=np.array([0.0, 0.5, 0.0], np.float32))
    p = scenes.cornell_box_sensor(W, H, 16, seed=21, max_depth=5, rfilter="box")
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=5))
    for rr_depth in (9, 2):
        d = _desc(scene, p, rr_depth=rr_depth)
        film = _primal_film(scene, d)
        dimage = _random_dimage(H, W)
        dimage[..., 1] = np.abs(dimage[..., 1])          # the green channel carries the terms in question: no cancellation there
        wanted = [(1, REFLECTANCE, c) for c in range(3)]
        g = _reverse(scene, d, dimage, film, wanted=wanted, h=0.01)
        want = [_dot(_forward_film(scene, d, _tangent(scene, bsdf={w: 1.0}, h=0.01)), dimage) for w in wanted]
        _within("wall (0.6, 0, 0), rr_depth %d" % rr_depth, g["bsdf"][1, :3], want, floor=3)


# ---------------------------------------------------------------------------------------------
# 2. the existing adjoints of the same convention

def test_detached_matches_the_parameter_adjoint_entry_by_entry(gpu):
    from mitsuba2_amd import _lib as L
    W, H = 40, 32
    sd, p, scene = _material_scene(gpu, (ROUGH, PLASTIC), w=W, h=H, spp=16, max_depth=5)
    d = _desc(scene, p, rr_depth=2)
    film = _primal_film(scene, d)
    di = torch.from_numpy(_random_dimage(H, W)).cuda()
    wanted = _accepted(scene)
    for step in (0.0, 0.003):
        g = _reverse(scene, d, di, film, wanted=wanted, h=step, flags=L.REVERSE_DETACH_ROULETTE)
        want = []
        for (b, kind, c) in wanted:
            g1 = torch.zeros(1, device="cuda")
            L.check(L.lib().mtsamd_render_adjoint_param(scene._handle, C.byref(d), _vp(di), _vp(film), b, kind, c, step, _vp(g1), None))
            want.append(float(g1.item()))
        _within("h = %g against mtsamd_render_adjoint_param" % step, [g["bsdf"][b, 3 * kind + c] for (b, kind, c) in wanted], want, floor=len(wanted) // 2)


def test_attached_matches_the_diffuse_adjoint_and_the_oracle(gpu, oracle):
    """textured Cornell box, rr_depth 2: constants, texels and the lamp for four block indicators against mtsamd_render_adjoint and the
    oracle's adjoint"""
    from mitsuba2_amd import _lib as L
    W = H = 32
    sd, tex, p, scene = _textured_box(gpu, 6, 2)
    d = _desc(scene, p)
    film = _primal_film(scene, d)
    S = oracle.OracleScene(sd, naive=True)
    desc = oracle.make_desc(p, analytic=True, film_rgb=True)
    _, film_o = S.render_image(desc)
    wanted = _accepted(scene)
    assert len(wanted) == 12          # four constant reflectances; the textured record has none
    got, dev, orc = [], [], []
    for (y, x) in _blocks(H, W)[1::4]:
        dimage = _indicator(H, W, y, x)
        g = _reverse(scene, d, dimage, film, wanted=wanted, emitters=True, tex_floats=tex.size)
        got.append((g["bsdf"][:, :3], g["tex"], g["emitters"]))
        g_bsdf, g_tex, g_em = torch.zeros((len(sd["bsdfs"]), 3), device="cuda"), torch.zeros(tex.size, device="cuda"), torch.zeros((1, 3), device="cuda")
        L.check(L.lib().mtsamd_render_adjoint(scene._handle, C.byref(d), _vp(torch.from_numpy(dimage).cuda()), _vp(film), _vp(g_bsdf), _vp(g_tex), _vp(g_em), None))
        torch.cuda.synchronize()
        dev.append((g_bsdf.cpu().numpy(), g_tex.cpu().numpy(), g_em.cpu().numpy()))
        gs_o, gt_o, ge_o = S.render_adjoint(desc, dimage, film_o, len(sd["meshes"]), tex.size, n_emitters=1)
        gb_o = np.zeros((len(sd["bsdfs"]), 3))
        for si, m in enumerate(sd["meshes"]):
            gb_o[m["bsdf"]] += gs_o[si]
        orc.append((gb_o, gt_o, ge_o))
    assert len(got) == 4
    for f, family in enumerate(("constants", "texels", "the lamp")):
        mine = np.concatenate([np.asarray(x[f], np.float64).reshape(-1) for x in got])
        for side, other in (("mtsamd_render_adjoint", dev), ("the oracle", orc)):
            want = np.concatenate([np.asarray(x[f], np.float64).reshape(-1) for x in other])
            assert (np.abs(want) > 1e-3 * np.abs(want).max()).sum() >= want.size // 4, (family, side, want)
            _assert_close("%s against %s" % (family, side), mine, want)


def test_attached_matches_the_texel_and_envmap_adjoints(gpu):
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
    di = torch.from_numpy(_random_dimage(H, W, seed=2)).cuda()
    g = _reverse(scene, d, di, film, tex_floats=tex.size, env_shape=sky["data"].shape)
    g_tex, g_env = torch.zeros(tex.size, device="cuda"), torch.zeros(sky["data"].shape, device="cuda")
    L.check(L.lib().mtsamd_render_adjoint_textures(scene._handle, C.byref(d), _vp(di), _vp(film), _vp(g_tex), None))
    L.check(L.lib().mtsamd_render_adjoint_envmap(scene._handle, C.byref(d), _vp(di), _vp(film), _vp(g_env), None))
    torch.cuda.synchronize()
    assert float(g_tex.abs().max()) > 1e-2 and float(g_env.abs().max()) > 1e-2
    _assert_close("texels against mtsamd_render_adjoint_textures", g["tex"], g_tex.cpu().numpy())
    _assert_close("envmap against mtsamd_render_adjoint_envmap", g["env"], g_env.cpu().numpy())
    # each family alone is the same gradient: one replay serves them all
    alone = _reverse(scene, d, di, film, env_shape=sky["data"].shape)
    _assert_close("envmap alone (no vertex record)", alone["env"], g_env.cpu().numpy())


# ---------------------------------------------------------------------------------------------
# 3. emitter colours against primal renders

def test_emitter_colours_are_the_renders_lit_by_one_emitter(gpu, oracle):
    """grad_emitters[e, c] for a block indicator = the block sum of channel c of the image lit by emitter e alone at colour (1, 1, 1):
    area, point, spot and directional lights under a constant environment.  No derivative code on the other side."""
    W, H = 32, 32
    sd = _lit_box()
    p = scenes.cornell_box_sensor(W, H, 8, seed=4, max_depth=8, rfilter="box")
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=8))
    d = _desc(scene, p)
    film = _primal_film(scene, d)
    n_em = len(sd["emitters"])
    assert [e.get("type", "area") for e in sd["emitters"]] == ["constant", "area", "point", "spot", "directional"]
    blocks = _blocks(H, W)[::5]
    assert len(blocks) == 4
    got = np.array([_reverse(scene, d, _indicator(H, W, y, x), film, emitters=True)["emitters"] for (y, x) in blocks])      # (block, emitter, channel)
    picked = [_blocks(H, W).index(b) for b in blocks]
    colours = _emitter_colours(sd)
    for e in range(n_em):
        for k in range(n_em):
            scene.set_emitter_radiance(k, [1.0, 1.0, 1.0] if k == e else [0.0, 0.0, 0.0])
        lit = _primal_film(scene, d).cpu().numpy()
        assert np.array_equal(lit[..., 4].view(np.uint32), film.cpu().numpy()[..., 4].view(np.uint32))
        want = _block_sums(_image(lit))[picked]
        assert np.abs(want).max() > 0
        _assert_close("emitter %d (%s) against the render it lights alone" % (e, sd["emitters"][e].get("type", "area")), got[:, e, :], want)
    for k in range(n_em):
        scene.set_emitter_radiance(k, colours[k])
    # once from the oracle: the spot alone
    from mitsuba2_amd import emitters as E
    sd_o = dict(sd, emitters=[dict(em, **{E._VALUE_KEY[em.get("type", "area")]: [1.0, 1.0, 1.0] if k == 3 else [0.0, 0.0, 0.0]}) for k, em in enumerate(sd["emitters"])])
    assert sd["emitters"][3]["type"] == "spot" and "intensity" in sd["emitters"][3]
    image_o, _ = oracle.OracleScene(sd_o, naive=True).render_image(oracle.make_desc(p, analytic=True, film_rgb=True))
    _assert_close("the spot against the oracle's render", got[:, 3, :], _block_sums(image_o.astype(np.float64))[picked])


# ---------------------------------------------------------------------------------------------
# 4. RECORD = false at any depth

@pytest.mark.parametrize("max_depth", [20, -1])
def test_emitter_and_envmap_gradients_at_any_depth(gpu, max_depth):
    W, H = 24, 16
    env = np.random.RandomState(7).uniform(0.2, 1.0, size=(8, 16, 3)).astype(np.float32)
    sd, _ = hierarchy_scene("shallow", sphere=ROUGH, envmap=env, area=True)
    p = hierarchy_sensor(W, H, 8, max_depth, seed=77)
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=max_depth))
    d = _desc(scene, p)
    film = _primal_film(scene, d)
    dimage = _random_dimage(H, W)
    g = _reverse(scene, d, dimage, film, emitters=True, env_shape=env.shape)
    rng = np.random.RandomState(3)
    t_em, t_env = rng.uniform(0.5, 2.0, (len(sd["emitters"]), 3)).astype(np.float32), rng.uniform(0.0, 1.0, env.shape).astype(np.float32)
    env_row = next(e for e, em in enumerate(sd["emitters"]) if em.get("type", "area") == "envmap")
    assert not g["emitters"][env_row].any()          # the row of the envmap is not touched
    for name, td, rev in (("emitters", _tangent(scene, emitters=t_em), float((g["emitters"] * t_em).sum())),
                          ("envmap", _tangent(scene, env=t_env), float((g["env"] * t_env).sum()))):
        _within("%s at max_depth %d against the forward render" % (name, max_depth), rev, _dot(_forward_film(scene, d, td), dimage), floor=1)
    # BSDF scalars and texels record their vertices: a finite depth of at most 16
    msg = _reverse(scene, d, dimage, film, wanted=[(0, ALPHA, 0)], emitters=True, expect=UNSUPPORTED)
    assert "max_depth <= 16" in msg and str(max_depth) in msg
    ok = _reverse(scene, _desc(scene, p, max_depth=16), dimage, film, wanted=[(0, ALPHA, 0)])
    assert np.isfinite(ok["bsdf"]).all() and ok["bsdf"][0, 3 * ALPHA] != 0
    assert "max_depth <= 16" in _reverse(scene, _desc(scene, p, max_depth=17), dimage, film, wanted=[(0, ALPHA, 0)], expect=UNSUPPORTED)


# ---------------------------------------------------------------------------------------------
# 5. launch edges

@pytest.mark.parametrize("case", ["45_samples", "two_trips", "hierarchy"])
def test_launch_edges(gpu, case):
    """under one wave; more than one grid-stride trip of the 2048 workgroups; k_reverse<false, true> on a hierarchy scene: the transpose
    identity with the lamp and one alpha"""
    from mitsuba2_amd import _lib as L
    if case == "hierarchy":
        W, H, spp = 24, 16, 8
        env = np.random.RandomState(7).uniform(0.2, 1.0, size=(8, 16, 3)).astype(np.float32)
        sd, _ = hierarchy_scene("shallow", sphere=ROUGH, envmap=env, area=True)
        p = hierarchy_sensor(W, H, spp, 5, seed=77)
        scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=5))
        info = (C.c_uint32 * 6)()
        L.check(L.lib().mtsamd_scene_info(scene._handle, info))
        assert info[0] > 64            # a hierarchy scene
        alpha = (0, ALPHA, 0)
    else:
        W, H, spp = (5, 3, 3) if case == "45_samples" else (96, 64, 96)
        sd, p, scene = _material_scene(gpu, (ROUGH, PLASTIC), w=W, h=H, spp=spp, max_depth=5)
        alpha = (len(sd["bsdfs"]) - 2, ALPHA, 0)
    if case == "two_trips":
        assert W * H * spp > 2048 * 256
    d = _desc(scene, p)
    film = _primal_film(scene, d)
    dimage = _random_dimage(H, W)
    lamp = next(e for e, em in enumerate(sd["emitters"]) if em.get("type", "area") == "area")
    t_em = np.zeros((len(sd["emitters"]), 3), np.float32)
    t_em[lamp] = [1.0, 2.0, 0.5]
    g = _reverse(scene, d, dimage, film, wanted=[alpha], emitters=True)
    _within("%s: alpha" % case, g["bsdf"][alpha[0], 3 * ALPHA], _dot(_forward_film(scene, d, _tangent(scene, bsdf={alpha: 1.0})), dimage))
    _within("%s: the lamp" % case, float((g["emitters"] * t_em).sum()), _dot(_forward_film(scene, d, _tangent(scene, emitters=t_em)), dimage))
    assert case == "45_samples" or (g["bsdf"][alpha[0], 3 * ALPHA] != 0 and g["emitters"][lamp].all())


# ---------------------------------------------------------------------------------------------
# 6. both sides of the bin capacity

def test_slot_counts_around_the_bin_capacity(gpu):
    """24 one-triangle shapes with a diffuse record each (72 scalars); the backdrop, which every camera ray can reach, carries record 21,
    so that the slots SLOT_BINS - 1 and SLOT_BINS (its red and green channels) are hit for certain.  1, SLOT_BINS and
    SLOT_BINS + 1 wanted slots against the same gradient computed in chunks of at most 16 slots per call."""
    assert SLOT_BINS == 64
    W, H = 24, 24
    sd = flat_limits.diffuse(flat_limits.soup(24, "per_triangle", 1))
    meshes = list(sd["meshes"])
    meshes[0], meshes[21] = dict(meshes[0], bsdf=21), dict(meshes[21], bsdf=0)
    sd = dict(sd, meshes=meshes)
    p = flat_limits.soup_sensor(W, H, 8, max_depth=5)
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=5))
    d = _desc(scene, p)
    film = _primal_film(scene, d)
    dimage = np.ones((H, W, 3), np.float32)
    every = _accepted(scene)
    assert len(every) == 72 and every[SLOT_BINS] == (21, REFLECTANCE, 1)
    chunks = np.zeros((24, 18))
    for k in range(0, SLOT_BINS + 1, 16):
        part = every[k:min(k + 16, SLOT_BINS + 1)]
        assert 1 <= len(part) <= 16
        chunks += _reverse(scene, d, dimage, film, wanted=part)["bsdf"]
    assert chunks[21, :2].all() and (chunks != 0).sum() >= 20          # record 21: slots SLOT_BINS - 1 and SLOT_BINS
    for n in (1, SLOT_BINS, SLOT_BINS + 1):
        wanted = every[:n] if n > 1 else [every[SLOT_BINS - 1]]
        g = _reverse(scene, d, dimage, film, wanted=wanted)["bsdf"]
        mask = np.zeros((24, 18), bool)
        for (b, kind, c) in wanted:
            mask[b, 3 * kind + c] = True
        assert not g[~mask].any()
        _assert_close("%d wanted slots against chunks of 16" % n, g[mask], chunks[mask])


def test_emitter_counts_around_the_bin_capacity(gpu):
    """the Cornell box's lamp and 32 point lights: emitter 31 is the last with an LDS bin, emitter 32 goes straight to global atomics.
    Each of the two against a one-hot forward render, and all 33 along one random tangent."""
    em_bins = int(re.search(r"kReverseEmitterBins = (\d+)u", open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mitsuba2_amd", "csrc", "kernels.h")).read()).group(1))
    assert em_bins == 32
    W, H = 24, 24
    sd = flat_limits.many_lights(scenes.cornell_box(), em_bins, 0, 0)
    assert len(sd["emitters"]) == em_bins + 1
    p = scenes.cornell_box_sensor(W, H, 8, seed=6, max_depth=4, rfilter="box")
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=4))
    d = _desc(scene, p)
    film = _primal_film(scene, d)
    dimage = np.abs(_random_dimage(H, W))
    g = _reverse(scene, d, dimage, film, emitters=True)["emitters"]
    # (a few of the random lights sit inside the two blocks and light nothing; the two at the capacity are in the open)
    assert g.shape == (em_bins + 1, 3) and g[em_bins - 1:].all() and (g != 0).all(1).sum() >= em_bins - 6
    for e in (em_bins - 1, em_bins):
        for c in range(3):
            t = np.zeros((em_bins + 1, 3), np.float32)
            t[e, c] = 1.0
            _within("emitter %d of %d, channel %d" % (e, em_bins + 1, c), g[e, c], _dot(_forward_film(scene, d, _tangent(scene, emitters=t)), dimage))
    t = _emitter_colours(sd) * np.random.RandomState(2).uniform(0.5, 1.5, (em_bins + 1, 3)).astype(np.float32)
    _within("all %d emitters along one tangent" % (em_bins + 1), float((g * t).sum()), _dot(_forward_film(scene, d, _tangent(scene, emitters=t)), dimage), floor=1)


# ---------------------------------------------------------------------------------------------
# 7. delta lobes

def test_delta_lobes(gpu):
    """a conductor and a dielectric: the discrete lobes are re-sampled with the perturbed records and the same numbers"""
    W, H = 32, 24
    sd, p, scene = _material_scene(gpu, (CONDUCTOR, DIELECTRIC), w=W, h=H, spp=16, max_depth=6)
    d = _desc(scene, p)
    film = _primal_film(scene, d)
    dimage = _random_dimage(H, W)
    tall, small = len(sd["bsdfs"]) - 2, len(sd["bsdfs"]) - 1
    wanted = [(tall, kind, c) for kind in (SPECULAR_REFLECTANCE, ETA) for c in range(3)] + \
             [(small, kind, c) for kind in (SPECULAR_REFLECTANCE, SPECULAR_TRANSMITTANCE) for c in range(3)]
    g = _reverse(scene, d, dimage, film, wanted=wanted, h=0.004)
    want = [_dot(_forward_film(scene, d, _tangent(scene, bsdf={w: 1.0}, h=0.004)), dimage) for w in wanted]
    _within("specular_reflectance / eta of the conductor, specular_reflectance / specular_transmittance of the dielectric",
            [g["bsdf"][b, 3 * kind + c] for (b, kind, c) in wanted], want, floor=6)


# ---------------------------------------------------------------------------------------------
# 8. accumulation

def test_gradients_are_accumulated_and_unwanted_entries_keep_their_bits(gpu):
    from test_gpu_adjoint_textures import _open_box, _sky
    tex = (0.3 + 0.5 * np.random.RandomState(1).rand(4, 5, 3)).astype(np.float32)
    sky = _sky()
    sd = _open_box(tex, textured_bsdf={"type": "plastic", "int_ior": 1.6, "diffuse_reflectance": {"type": "bitmap", "data": tex}},
                   emitters=[sky, {"type": "point", "position": [278, 400, 200], "intensity": [2e5, 2e5, 3e5]}])
    W, H = 24, 20
    p = scenes.cornell_box_sensor(W, H, 8, seed=5, max_depth=5, rfilter="box")
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=5))
    d = _desc(scene, p)
    film = _primal_film(scene, d)
    dimage = np.ones((H, W, 3), np.float32)
    wanted = [w for w in _accepted(scene) if w[1] in (REFLECTANCE, SPECULAR_REFLECTANCE)]
    assert len(wanted) >= 9
    sentinel = np.float32(-123.456)
    start = torch.full((len(sd["bsdfs"]), 18), float(sentinel), device="cuda")
    for (b, kind, c) in wanted:
        start[b, 3 * kind + c] = 0.0
    args = dict(wanted=wanted, emitters=True, tex_floats=tex.size, env_shape=sky["data"].shape)
    once = _reverse(scene, d, dimage, film, into={"bsdf": start.clone()}, **args)
    twice = _reverse(scene, d, dimage, film, into=_reverse(scene, d, dimage, film, into={"bsdf": start.clone()}, **args), **args)
    untouched = start.cpu().numpy() == sentinel
    for buf in (once, twice):
        assert np.array_equal(buf["bsdf"].cpu().numpy()[untouched].view(np.uint32), np.full(int(untouched.sum()), sentinel).view(np.uint32))
    assert not once["emitters"].cpu().numpy()[0].any() and once["emitters"].cpu().numpy()[1].all()      # the envmap's row; the point light
    for name in ("bsdf", "emitters", "tex", "env"):
        a, b = once[name].cpu().numpy().astype(np.float64), twice[name].cpu().numpy().astype(np.float64)
        if name == "bsdf":
            a, b = a[~untouched], b[~untouched]
        assert np.abs(a).max() > 1e-4          # (the intensity of the point light is 2e5: its gradient is of the order of 3e-4)
        nz = a != 0
        print("%s: two calls against twice one call, worst deviation %.3g of the bound (rtol 1e-5)" % (name, float(np.max(np.abs(b[nz] - 2 * a[nz]) / (1e-5 * np.abs(2 * a[nz]))))))
        assert np.allclose(b, 2 * a, rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------------------
# 9. autodiff.render(backward="fused")

def test_fused_backward_pass(gpu):
    from mitsuba2_amd import autodiff
    from test_gpu_adjoint_textures import _open_box, _sky
    tex = (0.3 + 0.5 * np.random.RandomState(1).rand(4, 5, 3)).astype(np.float32)
    sd = _open_box(tex, textured_bsdf={"type": "plastic", "int_ior": 1.6, "diffuse_reflectance": {"type": "bitmap", "data": tex}},
                   emitters=[_sky(), {"type": "point", "id": "bulb", "position": [278, 400, 200], "intensity": [2e5, 2e5, 3e5]}])
    W, H = 24, 20
    p = scenes.cornell_box_sensor(W, H, 8, seed=5, max_depth=4, rfilter="box")
    scene = gpu.Scene(sd, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=4))       # rr_depth 5 > max_depth: one convention
    params = autodiff.traverse(scene, emitters=True, geometry=True)
    shared = ["metal.eta.value", "textured.diffuse_reflectance.data", "sky.data"]
    bulb = "bulb.intensity.value"
    vkey = next(k for k in params.keys() if k.endswith(".vertex_positions_buf"))
    assert all(k in params for k in shared + [bulb])
    assert [params._kind[k][0] for k in shared + [bulb]] == ["bsdf_param", "texture", "envmap", "emitter"]
    weights = torch.from_numpy(np.random.RandomState(5).uniform(0.0, 1.0, W * H * 3).astype(np.float32)).cuda()

    def grads(keys, **kw):
        for k in keys:
            params[k].requires_grad_(True)
        autodiff._render_counter[id(scene)] = 0
        try:
            (autodiff.render_torch(scene, params=params, **kw) * weights).sum().backward()
            return {k: params[k].grad.detach().cpu().numpy().astype(np.float64) for k in keys}
        finally:
            for k in keys:
                params[k].grad = None
                params[k].requires_grad_(False)

    families = grads(shared)
    fused = grads(shared + [bulb], backward="fused")
    for k in shared:
        assert np.abs(families[k]).max() > 1e-3
        _assert_close("fused against families: %s" % k, fused[k], families[k])
    detached = grads(shared + [bulb], backward="fused", detach_roulette=True)
    for k in shared + [bulb]:      # no roulette on any path: nothing to detach
        assert np.array_equal(detached[k], fused[k]) or np.allclose(detached[k], fused[k], rtol=1e-5, atol=1e-5 * np.abs(fused[k]).max())
    # the bulb: radiance is linear in its intensity, so a central difference of primal renders at the same seed is the render it lights alone
    base = params[bulb].detach().clone()
    want = np.zeros(3)
    for c in range(3):
        images = []
        for sign in (1.0, -1.0):
            value = base.clone()
            value[c] = base[c] * (1.0 + sign)
            params[bulb] = value
            autodiff._render_counter[id(scene)] = 0
            with torch.no_grad():
                images.append(autodiff.render(scene, params=params).double())
        want[c] = float(((images[0] - images[1]) * weights.double()).sum().item()) / (2.0 * float(base[c]))
    params[bulb] = base
    params.update()
    assert np.abs(want).min() > 0
    _assert_close("the bulb against primal renders", fused[bulb], want)
    # the default backward pass is what it was; vertices and spectral scenes raise
    params[bulb].requires_grad_(True)
    with pytest.raises(RuntimeError, match="render_forward"):
        autodiff.render(scene, params=params)
    params[bulb].requires_grad_(False)
    params[vkey].requires_grad_(True)
    with pytest.raises(RuntimeError, match="settable, not differentiable"):
        autodiff.render(scene, params=params, backward="fused")
    params[vkey].requires_grad_(False)
    with pytest.raises(RuntimeError, match="backward"):
        autodiff.render(scene, params=params, backward="both")
    spectral = gpu.Scene(scenes.cornell_box(), variant="spectral", sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=4))
    with pytest.raises(RuntimeError, match="RGB variant"):
        autodiff.render(spectral, params=autodiff.traverse(spectral), backward="fused")


def test_refusals(gpu):
    from mitsuba2_amd import _lib as L
    sd, tex, p, scene = _textured_box(gpu, 4, 5, 8, 8, 2)
    d = _desc(scene, p)
    film = _primal_film(scene, d)
    dimage = np.ones((8, 8, 3), np.float32)
    assert _reverse(scene, d, dimage, film, emitters=True)["emitters"].all()
    assert "unknown flag bits" in _reverse(scene, d, dimage, film, emitters=True, flags=2, expect=INVALID)
    assert "path integrator" in _reverse(scene, _desc(scene, p, integrator=1), dimage, film, emitters=True, expect=UNSUPPORTED)
    assert "whole crop window" in _reverse(scene, _desc(scene, p, row_begin=2), dimage, film, emitters=True, expect=UNSUPPORTED)
    assert "film_rgb" in _reverse(scene, _desc(scene, p, film_rgb=0), dimage, film, emitters=True, expect=UNSUPPORTED)
    assert "no envmap emitter" in _reverse(scene, d, dimage, film, env_shape=(2, 2, 3), expect=UNSUPPORTED)
    assert "bsdf 4 (type 0) has no differentiable parameter of kind 0" in _reverse(scene, d, dimage, film, wanted=[(4, 0, 0)], expect=UNSUPPORTED)
    assert "bsdf 1 (type 0) has no differentiable parameter of kind 4" in _reverse(scene, d, dimage, film, wanted=[(1, ALPHA, 0)], expect=UNSUPPORTED)
    plain = gpu.Scene(scenes.cornell_box(), sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=4))
    assert "no bitmap textures" in _reverse(plain, _desc(plain, p), dimage, film, tex_floats=4, expect=UNSUPPORTED)
    spectral = gpu.Scene(scenes.cornell_box(), variant="spectral", sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=4))
    assert "RGB variant" in _reverse(spectral, _desc(spectral, p), dimage, film, emitters=True, expect=UNSUPPORTED)
    sd_b = scenes.cornell_box()
    sd_b["bsdfs"] = list(sd_b["bsdfs"]) + [{"type": "blendbsdf", "weight": 0.5, "bsdf_0": {"type": "diffuse"}, "bsdf_1": {"type": "conductor"}}]
    sd_b["meshes"][6] = dict(sd_b["meshes"][6], bsdf=len(sd_b["bsdfs"]) - 1)
    blend = gpu.Scene(sd_b, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=4))
    assert "blendbsdf / mask" in _reverse(blend, _desc(blend, p), dimage, film, emitters=True, expect=UNSUPPORTED)
    sd_t = scenes.cornell_box()
    sd_t["bsdfs"] = list(sd_t["bsdfs"]) + [{"type": "roughconductor", "id": "tall", "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14], "alpha": {"type": "bitmap", "data": np.full((2, 2, 3), 0.2, np.float32)}}]
    sd_t["meshes"][6] = dict(sd_t["meshes"][6], bsdf=len(sd_t["bsdfs"]) - 1)
    textured = gpu.Scene(sd_t, sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=4))
    assert "textured BSDF parameters" in _reverse(textured, _desc(textured, p), dimage, film, emitters=True, expect=UNSUPPORTED)

"""Every consumer of a scene after its geometry was edited, against a fresh scene of the edited description.

The method is that of test_gpu_vertex_update.py: create the live scene, run the consumer once so that the device holds the old state,
apply the edit, run the consumer again, and compare with a fresh gpu.Scene of the description the edit leads to -- by torch.equal, since
a hit (t, primitive, u, v) does not depend on the accelerator and everything downstream is the same arithmetic.  Where the sibling test
of a consumer compares with the oracle, a fresh OracleScene of that description is compared too, by that test's own comparison.  The
edits, scenes, inputs and consumers are in live_scene.py.

Edits (live_scene.EDITS).  Hierarchy scene (vm.sphere_scene() and material variants), moves squash + light: "refit", "rebuild",
"rebuild-sah"; "recompute-*": the same three with normals="recompute" on the mesh that has normals, the flag words 1, 3 and 11 of
mtsamd_scene_update_vertices; "moves-then-sah": both moves refitted, then rebuild_accel(builder="sah").  Flat scene (the Cornell box with
vertex normals on its short box), moves short-box + light: "refit" and "recompute-refit"; a rebuild is a no-op there.  After every edit
accel_info() has to report the rebuilds and the builder the edit implies: the tree really was swapped.

Which test covers what:

* test_consumers_on_the_hierarchy_scene / _on_the_flat_scene, consumer x edit:
  direct, depth (k_direct and the depth integrator, sample streams, + oracle); moment (film); aov-all (all nine channel types in one
  stream, + oracle), aov-<type> (each type alone), aov-nested (the film of the aov integrator round a path integrator, and its nested
  stream); ray-intersect-si (4 096 rays, the 26 SurfaceInteraction planes, + OracleScene.fill_si), ray-test (+ oracle);
  sample-emitter (1 000 reference points, visibility test on), pdf-emitter (of hand-made direction samples and of the scene's own),
  emitter-eval (rays aimed at the lamp).
* test_spectral_streams: PathIntegrator.sample on variant="spectral" with constant colours and with a tabulated spectrum bound
  (k_bounce_spectral / k_bounce_spectra), + the oracle's spectral path.
* test_forward_mode: mtsamd_render_forward on the rough-conductor / textured-ground / envmap / area-light variant, one tangent each on
  the roughness, the texels and the lamp's colour; the film stage is atomic-free: equal bits.
* test_reverse_mode_and_adjoints: mtsamd_render_reverse (all four gradient families at once), mtsamd_render_adjoint_param,
  mtsamd_render_adjoint_textures, mtsamd_render_adjoint_envmap on that variant; test_diffuse_adjoint_on_the_flat_scene:
  mtsamd_render_adjoint on the textured Cornell box.  These sum with float atomics: the bound is the project's own for two orders of the
  same fp32 sum (test_gpu_reverse.py, fused against detached: equal bits, or rtol 1e-5, atol 1e-5 max|want|).  Two fresh scenes are
  held against each other in the same test; their spread is printed in units of the bound and has to stay within 0.25 of it.
* test_product_path: autodiff.traverse(live, geometry=True, accel=a), vertex_positions_buf set to the squash, params.update();
  autodiff.render(backward="fused") and autodiff.render_forward give the fresh scene's image bit for bit and its gradients in the bound.
* test_sequences: three seeds, ten steps of moves (sphere, floor, light; three accel values; normals given, recomputed on the host, or
  "recompute"), rebuilds of either builder and the other setters; after steps 3, 6 and 10 the path stream, an AOV stream and the
  forward-mode film equal a fresh scene's of the description tracked in Python, and accel_info()["rebuilds"] counts the rebuilds made.

No case passes vacuously: each asserts that the consumer's output before and after the edit -- a fresh scene of the old description and
one of the new -- differs in at least MOVED_MIN = 5 % of its rows; for gradients, by more than ten times the bound in at least 5 % of the
non-zero entries.  test_live_scene_cpu.py establishes the same with the oracle wherever it has a counterpart.  The two aov channel types
that are zero in the reference too are asserted to be zero instead; dp_dv alone is not run on the flat scene (live_scene.FLAT_WITHOUT_FLOOR)."""
import copy
import ctypes as C

import numpy as np
import parity_util
import pytest
import torch

import live_scene as ls
import vertex_moves as vm
from test_gpu_forward import _desc, _forward_film, _primal_film, _tangent, _vp
from test_gpu_reverse import _accepted, _reverse

pytestmark = pytest.mark.gpu
F32 = np.float32
_ORACLE = {}


def _once(key, make):
    if key not in _ORACLE:
        _ORACLE[key] = make()
    return _ORACLE[key]


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _assert_tree(live, edit, moves, flat=False):
    info = live.accel_info()
    assert (info["rebuilds"], info["builder"]) == ls.rebuilds_of(edit, moves, flat), (edit, info)


def _against_the_oracle(oracle, consumer, kind, edit, new, p, got):
    """the comparison of the consumer's own test, with a fresh OracleScene of the edited description (computed once per description)"""
    key = (consumer, kind, ls.EDITS[edit][0])
    if consumer in ("direct", "depth"):
        want, wpos = _once(key, lambda: ls.oracle_stream(oracle, new, p, consumer))
        rgb, mask, pos = (x.cpu().numpy() for x in got)
        assert np.array_equal(pos, wpos) and np.array_equal(mask, want[:, 3] > 0.5)
        if consumer == "depth":
            assert np.array_equal(rgb, want[:, :3])
        else:
            parity_util.check("%s %s %s" % (consumer, kind, edit), rgb, want[:, :3])
    elif consumer == "aov-all":
        wpos, want = _once(key, lambda: ls.oracle_aovs(oracle, new, p))
        assert np.array_equal(got[1].cpu().numpy(), wpos) and np.array_equal(got[0].cpu().numpy(), want)
    elif consumer in ("ray-intersect-si", "ray-test"):
        ref, hit, planes = _once(("queries", kind, ls.EDITS[edit][0]), lambda: ls.oracle_queries(oracle, new, ls.fixed_inputs(kind)[0]))
        if consumer == "ray-test":
            assert np.array_equal(got[0].cpu().numpy(), hit)
            return
        fields, t, prim, shape = (x.cpu().numpy() for x in got)
        valid = np.isfinite(ref[0])
        assert np.array_equal(t, ref[0]) and np.array_equal(prim.astype(np.uint32)[valid], ref[1][valid]) and np.array_equal(shape.astype(np.uint32)[valid], ref[2][valid])
        assert fields.shape[1] == 26 and np.array_equal(fields[valid], planes[valid])


def _run_case(gpu, oracle, kind, consumer, edit):
    old, p = ls.sphere_scene() if kind == "sphere" else ls.cbox_scene()
    moves = ls.SPHERE_MOVES if kind == "sphere" else ls.CBOX_MOVES
    run = ls.CONSUMERS[consumer]
    live = gpu.Scene(copy.deepcopy(old))
    before = run(gpu, live, p)                                         # the device holds the old state
    new = ls.apply(live, old, edit, moves)
    _assert_tree(live, edit, moves, flat=kind == "cbox")
    got = run(gpu, live, p)
    want = run(gpu, gpu.Scene(copy.deepcopy(new)), p)
    assert _equal(got, want), (consumer, edit, [bool(torch.equal(x, y)) for x, y in zip(got, want)])
    if consumer in ls.ALWAYS_ZERO:
        assert not bool(want[0].any())
    else:
        moved = ls.share(before[0].cpu().numpy(), want[0].cpu().numpy())
        print("%s %s %s: the edit changes %.1f %% of the output" % (kind, consumer, edit, 100.0 * moved))
        assert moved >= ls.MOVED_MIN, (consumer, edit, moved)
    _against_the_oracle(oracle, consumer, kind, edit, new, p, got)


@pytest.mark.parametrize("edit", ls.HIERARCHY_EDITS)
@pytest.mark.parametrize("consumer", sorted(ls.CONSUMERS))
def test_consumers_on_the_hierarchy_scene(gpu, oracle, consumer, edit):
    _run_case(gpu, oracle, "sphere", consumer, edit)


@pytest.mark.parametrize("edit", ls.FLAT_EDITS)
@pytest.mark.parametrize("consumer", sorted(set(ls.CONSUMERS) - set(ls.FLAT_WITHOUT_FLOOR)))
def test_consumers_on_the_flat_scene(gpu, oracle, consumer, edit):
    _run_case(gpu, oracle, "cbox", consumer, edit)


# ---- the spectral variant ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edit", ls.HIERARCHY_EDITS)
@pytest.mark.parametrize("tabulated", [False, True], ids=["colours", "table"])
def test_spectral_streams(gpu, oracle, tabulated, edit):
    old, old_oracle, p = ls.spectral_scene(tabulated)
    live = gpu.Scene(copy.deepcopy(old), variant="spectral")
    assert live._n_spectra == (1 if tabulated else 0)
    before = ls.SPECTRAL_CONSUMER(gpu, live, p)
    new = ls.apply(live, old, edit, ls.SPHERE_MOVES)
    _assert_tree(live, edit, ls.SPHERE_MOVES)
    got = ls.SPECTRAL_CONSUMER(gpu, live, p)
    want = ls.SPECTRAL_CONSUMER(gpu, gpu.Scene(copy.deepcopy(new), variant="spectral"), p)
    assert _equal(got, want)
    assert ls.share(before[0].cpu().numpy(), want[0].cpu().numpy()) >= ls.MOVED_MIN
    new_oracle = dict(new, bsdfs=old_oracle["bsdfs"])
    ref, rpos = _once(("spectral", tabulated, ls.EDITS[edit][0]), lambda: ls.oracle_stream(oracle, new_oracle, p, spectral_path=gpu.srgb_coeff_path()))
    assert np.array_equal(got[2].cpu().numpy(), rpos) and np.array_equal(got[1].cpu().numpy(), ref[:, 3] > 0.5)
    parity_util.check("spectral %s %s" % ("table" if tabulated else "colours", edit), got[0].cpu().numpy(), ref[:, :3])


# ---- derivative renders --------------------------------------------------------------------------------------------------------------------------
def _derivative_scene(gpu, sd, p):
    return gpu.Scene(copy.deepcopy(sd), sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=p["max_depth"]))


def _tangents(scene):
    lamp = np.zeros((2, 3), F32)
    lamp[1] = [1.0, 2.0, 0.5]
    texels = np.random.RandomState(3).uniform(0.0, 1.0, ls.texture().size).astype(F32)
    return [_tangent(scene, bsdf={(0, ls.ALPHA, 0): 1.0}, h=0.003), _tangent(scene, tex=texels), _tangent(scene, emitters=lamp)]


def _forward_films(scene, p):
    d = _desc(scene, p)
    return [_primal_film(scene, d).cpu().numpy()] + [_forward_film(scene, d, td) for td in _tangents(scene)]


@pytest.mark.parametrize("edit", ls.HIERARCHY_EDITS)
def test_forward_mode(gpu, edit):
    old, p = ls.derivative_scene()
    live = _derivative_scene(gpu, old, p)
    before = _forward_films(live, p)
    new = ls.apply(live, old, edit, ls.SPHERE_MOVES)
    _assert_tree(live, edit, ls.SPHERE_MOVES)
    got, want = _forward_films(live, p), _forward_films(_derivative_scene(gpu, new, p), p)
    for name, b, g, w in zip(("primal", "roughness", "texels", "lamp"), before, got, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (name, edit)
        moved = ls.share(b.reshape(-1, 5), w.reshape(-1, 5))
        print("forward %s %s: the edit changes %.1f %% of the pixels" % (name, edit, 100.0 * moved))
        assert moved >= ls.MOVED_MIN and np.abs(w[..., :3]).max() > 1e-3, (name, edit, moved)


def _assert_gradients(what, before, got, want, again):
    """got (the live scene) against want (a fresh scene) in the bound; `again`: a second fresh scene, the reference's own spread"""
    for name in sorted(want):
        spread, dev = ls.in_bound(again[name], want[name]), ls.in_bound(got[name], want[name])
        moved = ls.gradient_share(before[name], want[name])
        print("%s %s: the live scene deviates by %.3g of the bound, two fresh scenes by %.3g; the edit moves %.1f %% of the non-zero entries by more than ten bounds"
              % (what, name, dev, spread, 100.0 * moved))
        assert np.abs(want[name]).max() > 1e-4, (what, name)
        assert spread <= 0.25, (what, name, spread)
        assert dev <= 1.0, (what, name, dev)
        assert moved >= ls.MOVED_MIN, (what, name, moved)


def _derivative_gradients(scene, p):
    """{family: float64 array}: the four families of mtsamd_render_reverse at once, then the three adjoint entry points"""
    from mitsuba2_amd import _lib as L
    d = _desc(scene, p)
    film = _primal_film(scene, d)
    dimage = torch.from_numpy(ls.dimage_of(p)).cuda()
    tex_floats, env_shape = ls.texture().size, ls.envmap().shape
    out = {"reverse-" + k: v for k, v in _reverse(scene, d, dimage, film, wanted=_accepted(scene), emitters=True, tex_floats=tex_floats, env_shape=env_shape).items()}
    scalars = [(0, ls.ALPHA, 0)] + [(0, kind, c) for kind in (ls.SPECULAR_REFLECTANCE, ls.ETA, ls.K) for c in range(3)]
    param = []
    for (b, kind, c) in scalars:
        g = torch.zeros(1, device="cuda")
        L.check(L.lib().mtsamd_render_adjoint_param(scene._handle, C.byref(d), _vp(dimage), _vp(film), b, kind, c, 0.003, _vp(g), None))
        param.append(float(g.item()))
    g_tex, g_env = torch.zeros(tex_floats, device="cuda"), torch.zeros(env_shape, device="cuda")
    L.check(L.lib().mtsamd_render_adjoint_textures(scene._handle, C.byref(d), _vp(dimage), _vp(film), _vp(g_tex), None))
    L.check(L.lib().mtsamd_render_adjoint_envmap(scene._handle, C.byref(d), _vp(dimage), _vp(film), _vp(g_env), None))
    torch.cuda.synchronize()
    out.update({"adjoint_param": np.array(param), "adjoint_textures": g_tex.cpu().numpy().astype(np.float64), "adjoint_envmap": g_env.cpu().numpy().astype(np.float64)})
    return out, film


@pytest.mark.parametrize("edit", ls.HIERARCHY_EDITS)
def test_reverse_mode_and_adjoints(gpu, edit):
    old, p = ls.derivative_scene()
    live = _derivative_scene(gpu, old, p)
    before, _ = _derivative_gradients(live, p)
    new = ls.apply(live, old, edit, ls.SPHERE_MOVES)
    _assert_tree(live, edit, ls.SPHERE_MOVES)
    got, film = _derivative_gradients(live, p)
    want, wfilm = _derivative_gradients(_derivative_scene(gpu, new, p), p)
    again, _ = _derivative_gradients(_derivative_scene(gpu, new, p), p)
    assert torch.equal(film, wfilm)
    _assert_gradients(edit, before, got, want, again)


def _diffuse_gradients(scene, sd, p, tex):
    from mitsuba2_amd import _lib as L
    d = _desc(scene, p)
    film = _primal_film(scene, d)
    g_bsdf, g_tex, g_em = torch.zeros((len(sd["bsdfs"]), 3), device="cuda"), torch.zeros(tex.size, device="cuda"), torch.zeros((1, 3), device="cuda")
    L.check(L.lib().mtsamd_render_adjoint(scene._handle, C.byref(d), _vp(torch.from_numpy(ls.dimage_of(p)).cuda()), _vp(film), _vp(g_bsdf), _vp(g_tex), _vp(g_em), None))
    torch.cuda.synchronize()
    return {"reflectances": g_bsdf.cpu().numpy().astype(np.float64), "texels": g_tex.cpu().numpy().astype(np.float64), "lamp": g_em.cpu().numpy().astype(np.float64)}, film


@pytest.mark.parametrize("edit", ls.FLAT_EDITS)
def test_diffuse_adjoint_on_the_flat_scene(gpu, edit):
    tex = ls.texture()
    old, p = ls.cbox_scene(tex)
    live = _derivative_scene(gpu, old, p)
    before, _ = _diffuse_gradients(live, old, p, tex)
    new = ls.apply(live, old, edit, ls.CBOX_MOVES)
    _assert_tree(live, edit, ls.CBOX_MOVES, flat=True)
    got, film = _diffuse_gradients(live, old, p, tex)
    want, wfilm = _diffuse_gradients(_derivative_scene(gpu, new, p), old, p, tex)
    again, _ = _diffuse_gradients(_derivative_scene(gpu, new, p), old, p, tex)
    assert torch.equal(film, wfilm)
    _assert_gradients("mtsamd_render_adjoint " + edit, before, got, want, again)


# ---- the product path ----------------------------------------------------------------------------------------------------------------------------
def _product(scene, params, weights):
    """(image, forward-mode image along the roughness, {key: gradient}) of autodiff.render(backward="fused") at a fixed seed"""
    from mitsuba2_amd import autodiff
    keys = {}
    for k in params.keys():
        kind = params._kind[k]
        if kind[0] in ("texture", "envmap", "emitter") or (kind[0] == "bsdf_param" and kind[2] == ls.ALPHA):
            keys[kind[0]] = k
    assert sorted(keys) == ["bsdf_param", "emitter", "envmap", "texture"], list(params.keys())
    for k in keys.values():
        params[k].requires_grad_(True)
    autodiff._render_counter[id(scene)] = 0
    try:
        image = autodiff.render(scene, params=params, backward="fused")
        (image * weights).sum().backward()
        grads = {kind: params[k].grad.detach().cpu().numpy().astype(np.float64) for kind, k in keys.items()}
    finally:
        for k in keys.values():
            params[k].grad = None
            params[k].requires_grad_(False)
    autodiff._render_counter[id(scene)] = 0
    forward = autodiff.render_forward(scene, params, {keys["bsdf_param"]: torch.ones(1)})
    return image.detach().clone(), forward.clone(), grads


@pytest.mark.parametrize("accel", ls.ACCELS)
def test_product_path(gpu, accel):
    from mitsuba2_amd import autodiff
    old, p = ls.derivative_scene()
    new = vm.moved(old, vm.SPHERE_MOVES["squash"])
    weights = torch.from_numpy(np.random.RandomState(5).uniform(0.0, 1.0, p["width"] * p["height"] * 3).astype(F32)).cuda()
    live = _derivative_scene(gpu, old, p)
    params = autodiff.traverse(live, geometry=True, emitters=True, accel=accel)
    image0, forward0, grads0 = _product(live, params, weights)
    params["ball.vertex_positions_buf"] = vm.SPHERE_MOVES["squash"](old)[1].reshape(-1)
    params.update()
    _assert_tree(live, accel, [vm.SPHERE_MOVES["squash"]])          # the edit of that name
    image, forward, grads = _product(live, params, weights)
    fresh = [_derivative_scene(gpu, new, p) for _ in range(2)]
    (wimage, wforward, wgrads), (_, _, again) = [_product(s, autodiff.traverse(s, emitters=True), weights) for s in fresh]
    assert torch.equal(image, wimage) and torch.equal(forward, wforward)
    for what, b, w in (("image", image0, wimage), ("forward image", forward0, wforward)):
        moved = ls.share(b.cpu().numpy().reshape(-1, 3), w.cpu().numpy().reshape(-1, 3))
        print("product path %s %s: the squash changes %.1f %% of the pixels" % (accel, what, 100.0 * moved))
        assert moved >= ls.MOVED_MIN
    _assert_gradients("product path " + accel, grads0, grads, wgrads, again)


# ---- sequences -------------------------------------------------------------------------------------------------------------------------------------
def _sequence_outputs(gpu, scene, p):
    d = _desc(scene, p)
    return (ls._stream(lambda g: g.PathIntegrator(max_depth=6))(gpu, scene, p) + ls._aov_stream("p:position n:sh_normal")(gpu, scene, p) +
            tuple(torch.from_numpy(_forward_film(scene, d, td)) for td in _tangents(scene)[::2]))


@pytest.mark.parametrize("seed", ls.SEQUENCE_SEEDS)
def test_sequences(gpu, seed):
    sd, p = ls.derivative_scene()
    live = _derivative_scene(gpu, sd, p)
    first = _sequence_outputs(gpu, live, p)
    rebuilds = 0
    for i, step in enumerate(ls.sequence(seed), 1):
        sd, made = ls.sequence_step(live, sd, step)
        rebuilds += made
        if i in ls.SEQUENCE_CHECKS:
            got, want = _sequence_outputs(gpu, live, p), _sequence_outputs(gpu, _derivative_scene(gpu, sd, p), p)
            assert _equal(got, want), (seed, i, step, [bool(torch.equal(x, y)) for x, y in zip(got, want)])
            assert ls.share(first[0].cpu().numpy(), want[0].cpu().numpy()) >= ls.MOVED_MIN
            assert live.accel_info()["rebuilds"] == rebuilds, (seed, i)
    assert rebuilds >= 2

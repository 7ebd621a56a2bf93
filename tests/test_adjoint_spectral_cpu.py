"""CPU-side checks of the spectral path replay (mtsamd_render_adjoint_spectral): the Jacobian of srgb_model_fetch against central
differences of the lookup itself, the two new entry points (declared, bound, exported, refusing null arguments without a device),
and the parameter names of ``traverse(scene, replay=True)``.

Jacobian bound.  Inside a table cell the lookup is trilinear in (x, y, z1) with x = rgb[i + 1] (res - 1) / z: a rational function
of the maximal component, so a central difference has a truncation error.  The bound is measured, not chosen: central differences
in float64 arithmetic over the float32 lookup at h = 2e-4 and at h / 2 = 1e-4 disagree by at most 3.36e-4 of the largest entry
of a colour's Jacobian over the 210 colours below (the float32 rounding of the lookup divided by 2 h, about 1e-7 * |coeff| / 1e-4,
is what they differ by: the disagreement grows when h shrinks).  The test allows 4 x that, 1.35e-3 of the largest entry; the analytic
Jacobian is observed at 3.39e-4, 0.25 of the bound."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from mitsuba2_amd import bsdfs as B, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEFF = os.path.join(ROOT, "tests", "golden", "rgb2spec_opt_res16.coeff").encode()
RES = 16
JAC_BOUND = 1.35e-3          # of the largest entry of the colour's Jacobian: 4 x the measured h-versus-h/2 disagreement (module docstring)


def _fetch(rgb):
    from mitsuba2_amd import _lib as L
    out = (C.c_float * 3)()
    assert L.lib().mtsamd_srgb_model_fetch(COEFF, (C.c_float * 3)(*[float(x) for x in rgb]), out) == 0
    return np.array(out[:], np.float64)


def _jacobian(rgb):
    """rows: the rgb component; columns: the coefficient"""
    from mitsuba2_amd import _lib as L
    out = (C.c_float * 9)()
    assert L.lib().mtsamd_srgb_model_fetch_jacobian(COEFF, (C.c_float * 3)(*[float(x) for x in rgb]), out) == 0
    return np.array(out[:], np.float64).reshape(3, 3)


def _central(rgb, h):
    rgb = np.asarray(rgb, np.float32)
    fd = np.zeros((3, 3))
    for c in range(3):
        hi, lo = rgb.copy(), rgb.copy()
        hi[c] += np.float32(h); lo[c] -= np.float32(h)
        fd[c] = (_fetch(hi) - _fetch(lo)) / (float(hi[c]) - float(lo[c]))
    return fd


def _cell_colours(n_per_branch=70, seed=5):
    """colours in the middle of a table cell (so that rgb +- h stays inside it), for each of the three maximal-component branches"""
    scale = np.frombuffer(open(COEFF.decode(), "rb").read()[8:8 + 4 * RES], np.float32).astype(np.float64)
    rng = np.random.RandomState(seed)
    out = []
    for branch in range(3):
        while len(out) < (branch + 1) * n_per_branch:
            zi = rng.randint(3, RES - 1)
            z = scale[zi] + (scale[zi + 1] - scale[zi]) * rng.uniform(0.3, 0.7)
            xi, yi = rng.randint(0, RES - 2, 2)
            x, y = (xi + rng.uniform(0.3, 0.7)) / (RES - 1), (yi + rng.uniform(0.3, 0.7)) / (RES - 1)
            if scale[zi + 1] - scale[zi] < 4e-3 or z < 0.05:
                continue
            rgb = np.zeros(3)
            rgb[branch], rgb[(branch + 1) % 3], rgb[(branch + 2) % 3] = z, x * z, y * z
            out.append(rgb.astype(np.float32))
    return out


def _cell(rgb):
    """(maximal component, xi, yi, zi) of rgb2spec_fetch in the res-16 table"""
    scale = np.frombuffer(open(COEFF.decode(), "rb").read()[8:8 + 4 * RES], np.float32).astype(np.float64)
    rgb = np.asarray(rgb, np.float64)
    i = 0
    for j in (1, 2):
        if rgb[j] >= rgb[i]:
            i = j
    x, y = rgb[(i + 1) % 3] * (RES - 1) / rgb[i], rgb[(i + 2) % 3] * (RES - 1) / rgb[i]
    return i, min(int(x), RES - 2), min(int(y), RES - 2), min(int(np.searchsorted(scale, rgb[i], side="right")) - 1, RES - 2)


def test_jacobian_matches_central_differences_inside_a_cell():
    worst_fd, worst = 0.0, 0.0
    colours = _cell_colours()
    assert len(colours) == 210
    for rgb in colours:
        jac = _jacobian(rgb)
        # the precondition of the comparison: every perturbed lookup lands in the cell of the colour itself
        for c in range(3):
            for step in (-2e-4, 2e-4):
                v = rgb.copy()
                v[c] += np.float32(step)
                assert _cell(v) == _cell(rgb), (rgb.tolist(), c, step)
        fd1, fd2 = _central(rgb, 2e-4), _central(rgb, 1e-4)
        scale = np.abs(fd2).max()
        worst_fd = max(worst_fd, np.abs(fd1 - fd2).max() / scale)
        err = np.abs(jac - fd2).max() / scale
        worst = max(worst, err)
        assert err <= JAC_BOUND, (rgb.tolist(), err, jac.tolist(), fd2.tolist())
    print("h-vs-h/2 disagreement %.3e, analytic-vs-fd %.3e (bound %.1e)" % (worst_fd, worst, JAC_BOUND))
    assert worst_fd <= JAC_BOUND / 4 * 1.0001          # the bound is 4 x the measured disagreement: keep the two figures together


def test_jacobian_sentinels_and_clamped_components():
    assert not _jacobian([0.0, 0.0, 0.0]).any()          # black and white are sentinels (c2 = -+inf): no derivative
    assert not _jacobian([1.0, 1.0, 1.0]).any()
    inside = _jacobian([0.4, 0.7, 0.2])
    assert np.abs(inside).min(axis=1).max() > 0 and np.isfinite(inside).all()
    for rgb, rows in (([1.3, 0.7, 0.2], [0]), ([0.4, 0.7, -0.1], [2]), ([0.4, 1.2, -0.5], [1, 2])):
        jac = _jacobian(rgb)
        for c in range(3):
            assert (not jac[c].any()) == (c in rows), (rgb, jac.tolist())
        # the other rows are those of the clamped colour
        clamped = np.clip(np.asarray(rgb, np.float32), 0, 1)
        keep = [c for c in range(3) if c not in rows]
        assert np.array_equal(jac[keep], _jacobian(clamped)[keep])


def test_symbols_are_declared_bound_and_exported():
    from mitsuba2_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtsamd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("mtsamd_render_adjoint_spectral", "mtsamd_srgb_model_fetch_jacobian"):
        assert re.search(r"\b%s\s*\(" % name, text)
        assert name in L.SYMBOLS
        assert any(ln.split()[-1] == name and ln.split()[1] == "T" for ln in out.splitlines() if len(ln.split()) == 3)
    assert L.SYMBOLS["mtsamd_render_adjoint_spectral"][1][-3:] == [C.c_void_p] * 3       # grad_bsdf_dev, grad_textures_dev, stream
    assert L.lib().mtsamd_abi_version() == 6                                                # an additive change


def test_argument_validation_without_gpu():
    from mitsuba2_amd import _lib as L
    lib = L.lib()
    d = L.RenderDesc()
    buf = (C.c_float * 16)()
    for args in ((None, C.byref(d), buf, buf, buf, buf, None), (None, C.byref(d), None, buf, buf, buf, None), (None, C.byref(d), buf, None, buf, buf, None)):
        assert lib.mtsamd_render_adjoint_spectral(*args) < 0
        assert b"null" in lib.mtsamd_last_error()
    rgb, jac = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 9)()
    for args in ((None, rgb, jac), (COEFF, None, jac), (COEFF, rgb, None)):
        assert lib.mtsamd_srgb_model_fetch_jacobian(*args) < 0
        assert b"null" in lib.mtsamd_last_error()
    assert lib.mtsamd_srgb_model_fetch_jacobian(b"/nonexistent/srgb.coeff", rgb, jac) < 0
    assert b"Could not load" in lib.mtsamd_last_error()


class _StubScene:
    """what ParameterMap reads of a Scene, without a device: records, variant, texture indices"""

    def __init__(self, sd, variant):
        self._dict, self._variant, self._device_index = sd, variant, 0
        self._bsdf_records = [B.normalize(b) for b in sd["bsdfs"]]
        self._tex = {i: n for n, i in enumerate(i for i, b in enumerate(self._bsdf_records) if isinstance(b["reflectance"], dict))}

    def texture_index(self, i):
        return self._tex.get(i)


def _keys(sd, variant, monkeypatch, **kw):
    import torch
    from mitsuba2_amd import autodiff
    monkeypatch.setattr(torch, "device", lambda *a: "cpu")          # the parameter tensors live on the scene's GPU; here: on the host
    return autodiff.ParameterMap(_StubScene(sd, variant), **kw)


def _bitmap(h, w, v=0.5):
    return dict(type="bitmap", data=np.full((h, w, 3), v, np.float32))


def test_parameter_keys_with_and_without_replay(monkeypatch):
    diffuse = scenes.cornell_box(texture=np.full((2, 2, 3), 0.5, np.float32))
    for b, n in zip(diffuse["bsdfs"], ["white", "red", "green", "light", "textured"]):
        b["id"] = n
    diffuse["meshes"][5]["id"] = "lamp"
    general = dict(diffuse, bsdfs=list(diffuse["bsdfs"]) + [
        {"type": "plastic", "id": "shiny", "diffuse_reflectance": _bitmap(3, 2), "specular_reflectance": [0.9, 0.8, 0.7]},
        {"type": "twosided", "id": "wrapped", "bsdf": {"type": "roughplastic", "alpha": 0.2, "diffuse_reflectance": _bitmap(2, 2)}},
        {"type": "plastic", "id": "checks", "diffuse_reflectance": {"type": "checkerboard"}},
        {"type": "conductor", "id": "metal", "eta": 0.5, "k": 3.0}])
    constants = {"white.reflectance.value", "red.reflectance.value", "green.reflectance.value", "light.reflectance.value"}
    # diffuse spectral scene: today's keys exactly, and the texels beside them with replay
    today = set(_keys(diffuse, "spectral", monkeypatch).keys())
    assert today == constants | {"lamp.emitter.radiance.value"}
    assert set(_keys(diffuse, "spectral", monkeypatch, replay=False).keys()) == today
    pm = _keys(diffuse, "spectral", monkeypatch, replay=True)
    assert set(pm.keys()) == today | {"textured.reflectance.data"}
    assert tuple(pm["textured.reflectance.data"].shape) == (2, 2, 3) and pm._kind["textured.reflectance.data"] == ("texture", 0, 4)
    # general spectral scene
    today_g = set(_keys(general, "spectral", monkeypatch).keys())
    assert not any(k.endswith(".data") for k in today_g)
    pm = _keys(general, "spectral", monkeypatch, replay=True)
    assert set(pm.keys()) == today_g | {"textured.reflectance.data", "shiny.diffuse_reflectance.data", "wrapped.brdf_0.diffuse_reflectance.data"}
    # which keys the replay differentiates: the reflectance family; specular colours keep the central-difference route
    from mitsuba2_amd import autodiff
    routed = {k for k in pm.keys() if autodiff._replayed(pm, k)}
    assert routed == constants | {"textured.reflectance.data", "shiny.diffuse_reflectance.data", "wrapped.brdf_0.diffuse_reflectance.data"}
    assert "shiny.specular_reflectance.value" in pm
    assert not any(autodiff._replayed(_keys(general, "spectral", monkeypatch), k) for k in today_g)
    # the flag is ignored for RGB scenes
    assert set(_keys(general, "rgb", monkeypatch, replay=True).keys()) == set(_keys(general, "rgb", monkeypatch).keys())
    assert set(_keys(diffuse, "rgb", monkeypatch, replay=True).keys()) == set(_keys(diffuse, "rgb", monkeypatch).keys())

"""CPU-side checks of the emitter family of the spectral path replay (mtsamd_render_adjoint_spectral_emitters): the host lookup
mtsamd_srgb_emitter_fetch_jacobian -- (c0, c1, c2, sc) of an emitter colour and the composed Jacobian Jn = d c / d rgb -- against
float64 central differences of the existing host fetch of (c, sc); the new symbols; the parameter names of ``traverse(scene, replay=True)``.

An emitter colour is stored as sc = 2 max(r, g, b), n = rgb / max(1e-8, sc), c = srgb_model_fetch(n).  n of the maximal channel m is the
constant 0.5, so every lookup sits on the z = 0.5 plane of the table and c is bilinear in the other two components of n: a central
difference in a channel other than m is exact up to rounding, one in channel m (n_j = rgb_j / (2 rgb_m), a rational function) has a
truncation error.  The precondition of the comparison is asserted per colour: the normalised colour of every perturbed colour lies in
the table cell of the colour's own n, the maximum stays strict and in its channel, every component stays > 0.

Bound (the rule of MEASURED_T in tests/test_gpu_adjoint_spectral.py): t = the worst disagreement of the central differences at H = 2e-3
and at H / 2, |fd_H - fd_H/2| / (|fd_H/2| + max |fd_H/2|) over the entries of a colour's Jacobian and over the colours below; the
analytic Jn may differ from fd_H/2 by 4 t |fd| + 4 t max |fd|, per coefficient (the columns have different units: c0 multiplies
nm^2).  Measured here on the CPU: t = 3.135e-4, set by the brightest colour (peak 8.5: the float32 rounding of the lookup divided by
2 H weighs most where the colour is large; the ordinary colours disagree by 6e-7 ... 3e-5), so the bound is 1.25e-3; the analytic Jn is
observed at 2.56e-4, 0.20 of the bound.  d sc / d rgb (2 in channel m) is compared the same way and agrees exactly.  The figures are
also in profiles/r10_adjoint_spectral_emitters.txt."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from mitsuba2_amd import bsdfs as B, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEFF = os.path.join(ROOT, "tests", "golden", "rgb2spec_opt_res16.coeff").encode()
RES = 16
H = 2e-3
MEASURED_T = 3.135e-4        # worst H-versus-H/2 disagreement of the central differences over _colours() (module docstring); bound = 4 x


def _fetch_c_sc(rgb):
    """the reference: (c0, c1, c2, sc) from the existing host fetch, the normalisation done here in float32 as the scene does it"""
    from mitsuba2_amd import _lib as L
    rgb = np.asarray(rgb, np.float32)
    sc = np.float32(max(max(rgb[0], rgb[1]), rgb[2]) * np.float32(2.0))
    n = rgb / max(np.float32(1e-8), sc)
    out = (C.c_float * 3)()
    assert L.lib().mtsamd_srgb_model_fetch(COEFF, (C.c_float * 3)(*[float(x) for x in n]), out) == 0
    return np.array(list(out[:]) + [float(sc)], np.float64)


def _lookup(rgb):
    """(c0, c1, c2, sc), Jn with rows = the rgb component, columns = the coefficient"""
    from mitsuba2_amd import _lib as L
    out4, jac = (C.c_float * 4)(), (C.c_float * 9)()
    assert L.lib().mtsamd_srgb_emitter_fetch_jacobian(COEFF, (C.c_float * 3)(*[float(x) for x in rgb]), out4, jac) == 0
    return np.array(out4[:], np.float64), np.array(jac[:], np.float64).reshape(3, 3)


def _central(rgb, h):
    rgb = np.asarray(rgb, np.float32)
    fd = np.zeros((3, 4))
    for c in range(3):
        hi, lo = rgb.copy(), rgb.copy()
        hi[c] += np.float32(h); lo[c] -= np.float32(h)
        fd[c] = (_fetch_c_sc(hi) - _fetch_c_sc(lo)) / (float(hi[c]) - float(lo[c]))
    return fd


def _scale_axis():
    return np.frombuffer(open(COEFF.decode(), "rb").read()[8:8 + 4 * RES], np.float32).astype(np.float64)


def _cell_of_normalised(rgb):
    """(maximal component, xi, yi, zi) of rgb2spec_fetch at n = rgb / (2 max rgb), as tests/test_gpu_adjoint_spectral.py::_cell"""
    rgb = np.asarray(rgb, np.float32)
    n = (rgb / (np.float32(2.0) * rgb.max())).astype(np.float64)
    i = 0
    for j in (1, 2):
        if n[j] >= n[i]:
            i = j
    x, y = n[(i + 1) % 3] * (RES - 1) / n[i], n[(i + 2) % 3] * (RES - 1) / n[i]
    return i, min(int(x), RES - 2), min(int(y), RES - 2), min(int(np.searchsorted(_scale_axis(), n[i], side="right")) - 1, RES - 2)


def _centre(m, xi, yi, peak):
    """a colour with its strict maximum `peak` in channel m whose normalised colour lies in the middle of cell (xi, yi) of the z = 0.5 plane"""
    rgb = np.zeros(3)
    rgb[m], rgb[(m + 1) % 3], rgb[(m + 2) % 3] = peak, (xi + 0.5) / (RES - 1) * peak, (yi + 0.5) / (RES - 1) * peak
    return rgb.astype(np.float32)


def _same_cell(rgb, h):
    rgb = np.asarray(rgb, np.float32)
    m = int(np.argmax(rgb))
    for c in range(3):
        for sgn in (-1.0, 1.0):
            v = rgb.copy()
            v[c] += np.float32(sgn * h)
            assert v.min() > 0.0 and int(np.argmax(v)) == m and np.sum(v == v.max()) == 1, (rgb.tolist(), c, sgn)
            assert _cell_of_normalised(v) == _cell_of_normalised(rgb), (rgb.tolist(), c, sgn)


def _colours():
    """a strict maximum in each of the three channels, in mid-cell, dim and ordinary peaks; and bright colours with sc > 2"""
    out = []
    for m in range(3):
        for (xi, yi, peak) in ((3, 9, 0.5), (11, 2, 0.31), (7, 7, 0.85), (1, 12, 0.6)):
            out.append(_centre(m, xi, yi, peak))
    out += [_centre(0, 5, 10, 3.0), _centre(1, 12, 4, 8.5), _centre(2, 2, 6, 1.7)]
    return out


def test_composed_jacobian_matches_central_differences():
    worst_t, worst = 0.0, 0.0
    colours = _colours()
    assert sum(2.0 * float(c.max()) > 2.0 for c in colours) >= 3 and {int(np.argmax(c)) for c in colours} == {0, 1, 2}
    for rgb in colours:
        _same_cell(rgb, H)
        value, jn = _lookup(rgb)
        assert np.array_equal(value, _fetch_c_sc(rgb)), (rgb.tolist(), value.tolist())
        m = int(np.argmax(rgb))
        full = np.concatenate([jn, np.array([[2.0 if c == m else 0.0] for c in range(3)])], axis=1)      # d sc / d rgb beside d c / d rgb
        fd1, fd2 = _central(rgb, H), _central(rgb, H / 2)
        # columns have different units (c0 multiplies nm^2): the rule is applied per coefficient
        for j in range(4):
            scale = np.abs(fd2[:, j]).max()
            t = float(np.max(np.abs(fd1[:, j] - fd2[:, j]) / (np.abs(fd2[:, j]) + scale)))
            worst_t = max(worst_t, t)
            bound = 4.0 * MEASURED_T * (np.abs(fd2[:, j]) + scale)
            dev = np.abs(full[:, j] - fd2[:, j])
            worst = max(worst, float(np.max(dev / bound)))
            assert np.all(dev <= bound), (rgb.tolist(), j, full[:, j].tolist(), fd2[:, j].tolist())
    print("H-versus-H/2 disagreement t = %.3e (MEASURED_T %.3e); analytic against fd: %.3f of the bound" % (worst_t, MEASURED_T, worst))
    assert worst_t <= MEASURED_T * 1.0001          # the bound is 4 x the measured disagreement: keep the two figures together


def test_row_sums_vanish():
    """c depends on rgb through n only, which is homogeneous of degree 0: sum_ch rgb_ch Jn[ch][j] = 0, to the rounding of that sum"""
    for rgb in _colours() + [np.float32([0.4, 0.4, 0.4]), np.float32([0.7, 0.7, 0.2])]:
        _, jn = _lookup(rgb)
        terms = np.asarray(rgb, np.float64)[:, None] * jn
        assert np.all(np.abs(terms.sum(0)) <= 16.0 * 2.0 ** -24 * np.abs(terms).sum(0)), (rgb.tolist(), terms.sum(0).tolist(), np.abs(terms).sum(0).tolist())
        assert np.abs(terms).sum(0).min() > 0.0


def test_tie_and_black():
    from mitsuba2_amd import _lib as L
    # grey: a tie of all three channels.  Jn is finite, and m is the LOWEST channel that attains the maximum (the value
    # max(max(r, g), b) returns): rows 1 and 2 are those of the fetch at n divided by sc, row 0 carries -(n_1 J_1 + n_2 J_2) / rgb_0
    grey = np.float32([0.4, 0.4, 0.4])
    value, jn = _lookup(grey)
    assert np.isfinite(jn).all() and np.isfinite(value).all() and value[3] == np.float32(0.8)
    jf = (C.c_float * 9)()
    assert L.lib().mtsamd_srgb_model_fetch_jacobian(COEFF, (C.c_float * 3)(0.5, 0.5, 0.5), jf) == 0
    jf = np.array(jf[:], np.float64).reshape(3, 3)
    sc = float(np.float32(0.8))
    assert np.allclose(jn[1], jf[1] / sc, rtol=1e-6, atol=0) and np.allclose(jn[2], jf[2] / sc, rtol=1e-6, atol=0)
    assert np.allclose(jn[0], -(0.5 * jf[1] + 0.5 * jf[2]) / 0.4, rtol=1e-6, atol=0) and np.abs(jn[0]).max() > 0
    # a tie of two: channel 0 again
    _, jn2 = _lookup(np.float32([0.7, 0.7, 0.2]))
    assert L.lib().mtsamd_srgb_model_fetch_jacobian(COEFF, (C.c_float * 3)(0.5, 0.5, float(np.float32(0.2) / np.float32(1.4))), (jf2 := (C.c_float * 9)())) == 0
    jf2 = np.array(jf2[:], np.float64).reshape(3, 3)
    assert np.allclose(jn2[1], jf2[1] / float(np.float32(1.4)), rtol=1e-6, atol=0)
    # black: not differentiable (n = 0 / 0): the sentinel coefficients, scale 0, Jn all zero
    value, jn = _lookup(np.float32([0.0, 0.0, 0.0]))
    assert value[0] == 0 and value[1] == 0 and value[2] == -np.inf and value[3] == 0 and not jn.any()


def test_symbols_are_declared_bound_and_exported():
    from mitsuba2_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtsamd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("mtsamd_render_adjoint_spectral_emitters", "mtsamd_srgb_emitter_fetch_jacobian"):
        assert re.search(r"\b%s\s*\(" % name, text)
        assert name in L.SYMBOLS
        assert any(ln.split()[-1] == name and ln.split()[1] == "T" for ln in out.splitlines() if len(ln.split()) == 3)
    assert L.SYMBOLS["mtsamd_render_adjoint_spectral_emitters"][1][-3:] == [C.c_void_p] * 3      # grad_emitters_dev, grad_envmap_dev, stream
    assert L.lib().mtsamd_abi_version() == 6                                                       # an additive change


def test_argument_validation_without_gpu():
    from mitsuba2_amd import _lib as L
    lib = L.lib()
    d = L.RenderDesc()
    buf = (C.c_float * 16)()
    for args in ((None, C.byref(d), buf, buf, buf, buf, None), (None, C.byref(d), None, buf, buf, buf, None), (None, C.byref(d), buf, None, buf, buf, None)):
        assert lib.mtsamd_render_adjoint_spectral_emitters(*args) < 0
        assert b"null" in lib.mtsamd_last_error()
    rgb, out4, jac = (C.c_float * 3)(0.5, 0.4, 0.3), (C.c_float * 4)(), (C.c_float * 9)()
    for args in ((None, rgb, out4, jac), (COEFF, None, out4, jac), (COEFF, rgb, None, jac), (COEFF, rgb, out4, None)):
        assert lib.mtsamd_srgb_emitter_fetch_jacobian(*args) < 0
        assert b"null" in lib.mtsamd_last_error()
    assert lib.mtsamd_srgb_emitter_fetch_jacobian(b"/nonexistent/srgb.coeff", rgb, out4, jac) < 0
    assert b"Could not load" in lib.mtsamd_last_error()


class _StubScene:
    """what ParameterMap reads of a Scene, without a device (as tests/test_adjoint_spectral_cpu.py)"""

    def __init__(self, sd, variant):
        self._dict, self._variant, self._device_index = sd, variant, 0
        self._bsdf_records = [B.normalize(b) for b in sd["bsdfs"]]

    def texture_index(self, i):
        return None


def _map(sd, variant, monkeypatch, **kw):
    import torch
    from mitsuba2_amd import autodiff
    monkeypatch.setattr(torch, "device", lambda *a: "cpu")
    return autodiff.ParameterMap(_StubScene(sd, variant), **kw)


def test_emitter_keys_and_routes(monkeypatch):
    from mitsuba2_amd import autodiff
    sd = scenes.cornell_box()
    sd["meshes"][5]["id"] = "lamp"
    sky = {"type": "envmap", "id": "my_envmap", "data": np.full((4, 8, 3), 0.5, np.float32)}
    extra = [sky, {"type": "point", "id": "bulb", "position": [1, 2, 3], "intensity": [5.0, 6.0, 7.0]},
             {"type": "spot", "intensity": 2.0}, {"type": "directional", "id": "sun", "direction": [0, -1, 0], "irradiance": [3.0, 2.0, 1.0]}]
    lit = dict(sd, emitters=list(sd["emitters"]) + extra)
    # the default map is what it was: the envmap key (its backward pass raises), no key for a shapeless emitter, nothing replayed
    plain = _map(lit, "spectral", monkeypatch)
    assert "my_envmap.data" in plain and not any(k.endswith(("intensity.value", "irradiance.value")) for k in plain.keys())
    assert not any(autodiff._replayed(plain, k) for k in plain.keys())
    pm = _map(lit, "spectral", monkeypatch, replay=True)
    new = {"bulb.intensity.value", "emitter_3.intensity.value", "sun.irradiance.value"}
    assert set(pm.keys()) == set(plain.keys()) | new
    assert pm["bulb.intensity.value"].tolist() == [5.0, 6.0, 7.0] and pm["emitter_3.intensity.value"].tolist() == [2.0, 2.0, 2.0]
    assert pm._kind["sun.irradiance.value"] == ("emitter", 4, 4) and pm._kind["my_envmap.data"][0] == "envmap"
    assert {k for k in pm.keys() if autodiff._replayed(pm, k) == "emitter"} == new | {"my_envmap.data"}
    # a diffuse scene under area lights: the lamp's key exists either way and moves to the replay
    both = [_map(sd, "spectral", monkeypatch, replay=r) for r in (False, True)]
    assert set(both[0].keys()) == set(both[1].keys()) and "lamp.emitter.radiance.value" in both[0]
    assert autodiff._replayed(both[1], "lamp.emitter.radiance.value") == "emitter" and not autodiff._replayed(both[0], "lamp.emitter.radiance.value")
    # RGB scenes ignore the flag
    assert set(_map(lit, "rgb", monkeypatch, replay=True).keys()) == set(_map(lit, "rgb", monkeypatch).keys())
    # the message of the default route names the switch
    with np.testing.assert_raises_regex(RuntimeError, r"replay=True"):
        autodiff._spectral_gradient(None, None, plain, "my_envmap.data", None)

"""CPU-side checks of the texel gradients of general RGB scenes (mtsamd_render_adjoint_textures): the entry point is declared, bound
and exported, it refuses bad arguments without touching a device, and the ParameterMap names the textured parameters as the
reference's traverse() does."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from mitsuba2_amd import bsdfs as B, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mtsamd_render_adjoint_textures"


def test_symbol_is_declared_bound_and_exported():
    from mitsuba2_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtsamd.h")).read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert NAME in L.SYMBOLS
    assert L.SYMBOLS[NAME][1][-2:] == [C.c_void_p, C.c_void_p]           # grad_textures_dev, stream
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == NAME and ln.split()[1] == "T" for ln in out.splitlines() if len(ln.split()) == 3)
    assert L.lib().mtsamd_abi_version() == 6                               # an additive change


def test_argument_validation_without_gpu():
    from mitsuba2_amd import _lib as L
    lib = L.lib()
    d = L.RenderDesc()
    buf = (C.c_float * 16)()
    # a null scene, dLoss/dImage or film is refused before any device work, with the wording of the sibling entry points
    assert lib.mtsamd_render_adjoint_textures(None, C.byref(d), buf, buf, buf, None) < 0
    assert b"null" in lib.mtsamd_last_error()
    assert lib.mtsamd_render_adjoint_textures(None, C.byref(d), None, buf, buf, None) < 0
    assert b"null" in lib.mtsamd_last_error()
    assert lib.mtsamd_render_adjoint_textures(None, C.byref(d), buf, None, buf, None) < 0
    assert b"null" in lib.mtsamd_last_error()


def _bitmap(h, w, v=0.5):
    return dict(type="bitmap", data=np.full((h, w, 3), v, np.float32))


def _general_scene_dict():
    """textured diffuse floor + back wall, textured plastic, a textured roughplastic inside `twosided`, a checkerboard plastic, a blend
    with a textured child, a conductor and an envmap"""
    sd = scenes.cornell_box(texture=np.full((4, 5, 3), 0.5, np.float32))
    names = ["white", "red", "green", "light", "textured"]
    for b, n in zip(sd["bsdfs"], names):
        b["id"] = n
    sd["bsdfs"] = list(sd["bsdfs"]) + [
        {"type": "plastic", "id": "shiny", "diffuse_reflectance": _bitmap(3, 2)},
        {"type": "twosided", "id": "wrapped", "bsdf": {"type": "roughplastic", "alpha": 0.2, "diffuse_reflectance": _bitmap(2, 2)}},
        {"type": "twosided", "id": "wrapped_diffuse", "bsdf": {"type": "diffuse", "reflectance": _bitmap(2, 3)}},
        {"type": "plastic", "id": "checks", "diffuse_reflectance": {"type": "checkerboard"}},
        {"type": "blendbsdf", "id": "blend", "weight": 0.5, "bsdf_0": {"type": "diffuse", "reflectance": _bitmap(2, 2)},
         "bsdf_1": {"type": "conductor"}},
        {"type": "conductor", "id": "metal"},
    ]
    sd["emitters"] = list(sd["emitters"]) + [{"type": "envmap", "id": "sky", "data": np.ones((4, 8, 3), np.float32)}]
    return sd


def test_texture_keys_of_a_general_scene():
    from mitsuba2_amd.autodiff import _texture_parameters
    sd = _general_scene_dict()
    records = [B.normalize(b) for b in sd["bsdfs"]]
    got = {key: (i, np.asarray(data).shape) for key, i, data in _texture_parameters(records)}
    assert got == {
        "textured.reflectance.data": (4, (4, 5, 3)),
        "shiny.diffuse_reflectance.data": (5, (3, 2, 3)),
        # TwoSidedBRDF::traverse exposes its nested BSDF as "brdf_0" (twosided.cpp:183-186)
        "wrapped.brdf_0.diffuse_reflectance.data": (6, (2, 2, 3)),
        "wrapped_diffuse.brdf_0.reflectance.data": (7, (2, 3, 3)),
    }
    # every new key passes the suffix convention of the existing parameter names
    assert all(k.split(".")[-2] in ("reflectance", "diffuse_reflectance") for k in got)
    # records without an id are named by their index
    records[5].pop("id")
    assert "bsdf_5.diffuse_reflectance.data" in {k for k, _, _ in _texture_parameters(records)}

"""Scenes shared by test_gpu_adjoint_param_textures.py and test_adjoint_param_textures_cpu.py: the split construction of
test_gpu_textured_params.py with bitmaps in place of checkerboards.

The tall box of the Cornell box carries per-face texcoords inside u in [0.125, 0.375] (faces 0-2) and [0.625, 0.875] (faces 3-5), v in
[0.125, 0.375].  A textured parameter reads a 2 x 9 bitmap whose rows are equal, columns 0-4 holding the value of cell 0 and columns 5-8
the value of cell 1: u * 8 lies in [1, 3] or [5, 7], so every lookup interpolates equal texels and the parameter is one of two constants
on every face.  The oracle, which knows constant parameters only, renders the same triangles as two meshes with two constant materials;
its parameter adjoint over one of those meshes is what the texel gradients of that cell must sum to."""
import functools

import numpy as np

import oracle_binding as ob
from test_gpu_textured_params import CASES, _box_texcoords

F32 = np.float32
SPLIT_CASES = ["rough_ggx_alpha", "rough_beckmann_alpha_colour", "frosted_alpha_transmittance", "glass_colours", "conductor_colour",
               "twosided_rough_alpha"]
KIND = {"alpha": 4, "specular_reflectance": 1, "specular_transmittance": 5}       # mtsamd_bsdf_param
CELL_COLUMNS = (slice(0, 5), slice(5, 9))
H_STEP = 0.01
MAX_DEPTH = 7                      # past rr_depth = 5: the roulette factor is part of the path
SEED = 21


def split_map(v0, v1):
    """2 x 9 texels, rows equal: columns 0-4 = v0, columns 5-8 = v1 (a scalar is a grey texel)"""
    m = np.empty((2, 9, 3), F32)
    m[:, :5] = np.asarray(v0, F32)
    m[:, 5:] = np.asarray(v1, F32)
    return m


def split_scenes(case):
    """(scene with the bitmap-textured material on the tall box, the oracle's scene: the box as two meshes (7: cell 0, 8: cell 1) with
    constant materials, {parameter: (v0, v1)})"""
    from mitsuba2_amd import scenes
    base, params, wrap = CASES[case]
    textured = wrap(dict(base, id="tall", **{p: {"type": "bitmap", "data": split_map(v0, v1)} for p, (v0, v1) in params.items()}))
    if "id" not in textured:
        textured["id"] = "tall"
    constants = [wrap(dict(base, **{p: v[k] for p, v in params.items()})) for k in (0, 1)]
    cb = scenes.cornell_box()
    floor = {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": [0.7, 0.7, 0.7]}}
    assert len(cb["meshes"]) == 8 and cb["meshes"][7]["faces"].shape == (12, 3)
    box = dict(cb["meshes"][7], texcoords=_box_texcoords())
    n = len(cb["bsdfs"])
    others = [dict(cb["meshes"][0], bsdf=n)] + cb["meshes"][1:7]
    mine = dict(cb, bsdfs=list(cb["bsdfs"]) + [floor, textured], meshes=others + [dict(box, bsdf=n + 1)])
    theirs = dict(cb, bsdfs=list(cb["bsdfs"]) + [floor] + constants,
                  meshes=others + [dict(box, faces=np.ascontiguousarray(box["faces"][:6]), bsdf=n + 1),
                                   dict(box, faces=np.ascontiguousarray(box["faces"][6:]), bsdf=n + 2)])
    return mine, theirs, params


def sensor_params():
    from mitsuba2_amd import scenes
    return dict(scenes.cornell_box_sensor(32, 24, spp=8, seed=SEED), max_depth=MAX_DEPTH)


def dimage():
    return np.random.RandomState(4).uniform(-1, 1, (24, 32, 3)).astype(F32)


@functools.lru_cache(maxsize=None)
def oracle_wants(case):
    """(the oracle's primal film, {(parameter, cell, component): d loss / d component of the constant on that cell}); alpha has the one
    component 0.  Computed once per case and shared."""
    _, theirs, params = split_scenes(case)
    S = ob.OracleScene(theirs)
    desc = ob.make_desc(sensor_params(), analytic=True, film_rgb=True)
    _, film = S.render_image(desc)
    film.setflags(write=False)
    di = dimage()
    wants = {}
    for pname in params:
        for cell in (0, 1):
            for comp in range(1 if pname == "alpha" else 3):
                wants[(pname, cell, comp)] = S.render_adjoint_param(desc, di, film, [7 + cell], KIND[pname], comp, H_STEP)
    return film, wants

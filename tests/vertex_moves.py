"""Scenes, vertex moves and the host driver shared by tests/test_vertex_update_cpu.py and tests/test_gpu_vertex_update.py.

A move is a function of a scene description that returns (shape, new positions, new normals or None); `moved(sd, move)` is the
description after it.  Normals of a mesh that has them are recomputed with loaders.compute_vertex_normals, as Scene.update_vertices
recomputes them, so the description, the live scene and the host driver all hold the same arrays.

tests/refit_driver.cpp is the host half of mtsamd_scene_set_vertex_positions as a stand-alone program: `Driver.run(sd, commands)` writes
the description and the commands, runs it and returns {label.key: uint32 words}."""
import copy
import os
import shutil
import subprocess

import numpy as np

import flat_limits
from mitsuba2_amd import emitters as E
from mitsuba2_amd import loaders, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mitsuba2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
F32 = np.float32
SPHERE, FLOOR, LIGHT = 0, 1, 2                 # meshes of scenes.bumpy_sphere
CBOX_LIGHT, CBOX_SHORT_BOX = 5, 6              # meshes of scenes.cornell_box
SPHERE_CENTRE = np.array([0.0, 1.2, 0.0])


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def sphere_scene():
    return scenes.bumpy_sphere(8, 16), dict(scenes.bumpy_sphere_sensor(24, 16, 8, seed=21), max_depth=6)


def cbox_scene():
    return scenes.cornell_box(), dict(scenes.cornell_box_sensor(48, 48, spp=4, seed=21), max_depth=6)


def soup_scene(n):
    """flat_limits.soup: 64 triangles is the largest LDS-resident scene, 65 the smallest hierarchy"""
    return copy.deepcopy(flat_limits.diffuse(flat_limits.soup(n, "mixed", 1))), flat_limits.soup_sensor(24, 24, 4, max_depth=6)


def leaf_root_scene():
    """One triangle, yet a hierarchy scene: the emitter table of its 2400 delta lights exceeds the LDS cap.  The root of its BVH is a
    leaf: there is no node at all."""
    base = flat_limits.diffuse(flat_limits.soup(1, "one_shape", 1))
    return copy.deepcopy(flat_limits.many_lights(base, 2400, 0, 0)), flat_limits.soup_sensor(16, 16, 2, max_depth=3)


# ---- moves -------------------------------------------------------------------------------------------------------------------------------
def _positions(sd, shape):
    return np.asarray(sd["meshes"][shape]["positions"], np.float64).reshape(-1, 3)


def _result(sd, shape, pos):
    pos = np.ascontiguousarray(pos, F32)
    m = sd["meshes"][shape]
    nrm = None
    if m.get("normals") is not None:
        nrm = np.ascontiguousarray(loaders.compute_vertex_normals(pos, m["faces"]), F32)
    return shape, pos, nrm


def translate(shape, d):
    return lambda sd: _result(sd, shape, _positions(sd, shape) + np.asarray(d, np.float64))


def scale_about(shape, s, centre=None, shift=(0, 0, 0)):
    def move(sd):
        p = _positions(sd, shape)
        c = p.mean(0) if centre is None else np.asarray(centre, np.float64)
        return _result(sd, shape, (p - c) * np.asarray(s, np.float64) + c + np.asarray(shift, np.float64))
    return move


def jitter(shape, amplitude, seed=5):
    return lambda sd: _result(sd, shape, _positions(sd, shape) + np.random.RandomState(seed).uniform(-amplitude, amplitude, _positions(sd, shape).shape))


def squash(shape, y):
    def move(sd):
        p = _positions(sd, shape).copy()
        p[:, 1] = y
        return _result(sd, shape, p)
    return move


def collapse(shape, first, count):
    """vertices [first, first + count) all go to the place of vertex `first`: every triangle among them has zero area"""
    def move(sd):
        p = _positions(sd, shape).copy()
        p[first:first + count] = p[first]
        return _result(sd, shape, p)
    return move


SPHERE_MOVES = {
    "translate-out": translate(SPHERE, (9, 0.5, 0)),
    "translate-small": translate(SPHERE, (0.3, 0.1, 0)),
    "shrink": scale_about(SPHERE, 0.5, SPHERE_CENTRE),
    "jitter": jitter(SPHERE, 0.05),
    "squash": squash(SPHERE, 1.2),
    "floor": scale_about(FLOOR, (3, 1, 3), (0, 0, 0)),
    "light": scale_about(LIGHT, 1.5, shift=(0.5, -0.5, 0)),
    "collapse": collapse(SPHERE, 16, 64),
}
CBOX_MOVES = {
    "short-box": lambda sd: translate(CBOX_SHORT_BOX, np.array([0.1, 0, -0.1]) * np.ptp(_positions(sd, CBOX_SHORT_BOX), axis=0)[[0, 0, 2]])(sd),
    "light": scale_about(CBOX_LIGHT, 0.5),
}
EDGE_MOVES = {          # one shape of each edge scene, moved far enough to change what the camera sees
    "soup65": (lambda: soup_scene(65), scale_about(1, 2.5, shift=(0.4, 0.3, -0.5))),
    "soup64": (lambda: soup_scene(64), scale_about(1, 2.5, shift=(0.4, 0.3, -0.5))),
    "leaf-root": (leaf_root_scene, scale_about(0, 0.6, shift=(0.5, 0.4, 0.0))),
}


def moved(sd, *moves):
    """the description after the moves, each applied to the result of the one before"""
    new = dict(sd, meshes=[dict(m) for m in sd["meshes"]])
    for move in moves:
        shape, pos, nrm = move(new)
        new["meshes"][shape] = dict(new["meshes"][shape], positions=pos, normals=nrm)
    return new


# ---- the host driver ---------------------------------------------------------------------------------------------------------------------
def _hex(a):
    return " ".join("%08x" % w for w in np.ascontiguousarray(a, F32).reshape(-1).view(np.uint32))


def description_text(sd):
    lines = ["bsdfs %d" % max(len(sd["bsdfs"]), 1)]
    for e in sd.get("emitters", []):
        n = E.normalize(e)
        lines.append("emitter %d %r %r %s" % (n["type"], float(n["cutoff_angle"]), float(n["beam_width"]), _hex(n["to_world"])))
    for m in sd["meshes"]:
        pos, faces = np.asarray(m["positions"], F32).reshape(-1, 3), np.asarray(m["faces"], np.uint32).reshape(-1, 3)
        has = m.get("normals") is not None
        lines.append("mesh %d %d %d %d %d" % (m["bsdf"] % max(len(sd["bsdfs"]), 1), m.get("emitter", -1), len(pos), len(faces), has))
        lines += ["P " + _hex(pos), "F " + " ".join(str(int(x)) for x in faces.reshape(-1))]
        if has:
            lines.append("N " + _hex(m["normals"]))
    return lines + ["build"]


def move_text(label, shape, pos, nrm):
    return ["move %d %d %s" % (shape, nrm is not None, label), "P " + _hex(pos)] + (["N " + _hex(nrm)] if nrm is not None else [])


class Driver:
    """tests/refit_driver.cpp compiled with the host builder; `flags`: extra compiler flags (a sanitizer build)"""

    def __init__(self, directory, flags=()):
        self.directory = str(directory)
        self.exe = os.path.join(self.directory, "refit_driver")
        subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, "-o", self.exe] + list(flags) +
                              ["-x", "hip", "--cuda-host-only", os.path.join(HERE, "refit_driver.cpp"), os.path.join(CSRC, "scene_build.cpp"), "-x", "c++"] +
                              [os.path.join(CSRC, f) for f in ("bvh.cpp", "envmap.cpp", "spectral_upsampling.cpp")], stderr=subprocess.DEVNULL)

    def run(self, sd, commands, name="scene"):
        path = os.path.join(self.directory, name + ".txt")
        with open(path, "w") as f:
            f.write("\n".join(description_text(sd) + list(commands)) + "\n")
        out = {}
        for line in subprocess.check_output([self.exe, path], text=True).splitlines():
            key, _, rest = line.partition(" ")
            if key.endswith(".rc"):
                out[key] = int(rest)
            elif key.endswith(".message"):
                out[key] = rest
            else:
                out[key] = np.array([int(w, 16) for w in rest.split()], np.uint32)
        return out


ARRAYS = ("nodes", "qnodes", "wnodes", "wnodes_h", "wnodes_p", "tris", "bbox", "grid", "counts")
RECORDS = ("tri_pos", "tri_nrm", "area_pmf", "area_cdf", "emitters", "flat_recs", "pair_recs")

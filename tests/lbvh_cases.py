"""Inputs and the host driver shared by tests/test_lbvh_cpu.py and tests/test_gpu_rebuild.py.

tests/lbvh_driver.cpp is the host specification of the accelerator rebuild (build_lbvh) as a stand-alone program: `Driver.run(sd, commands)`
writes a scene description (or none: `raw` commands carry their own triangles) and the commands, runs it and returns {label.key: uint32
words}.  The triangle sets below are the ones a Morton-ordered radix tree can get wrong: equal codes, an axis without extent, a chain."""
import os
import subprocess

import numpy as np

import deep_walk
import flat_limits
import vertex_moves as vm

F32 = np.float32
MAX_LEAF = 4                     # BuildOptions::max_leaf


def copies(n=65):
    """n copies of one triangle: every Morton code is equal, the tree splits on the sorted position alone"""
    tri = np.array([[0.1, 0.2, 0.3], [0.9, 0.3, 0.2], [0.4, 0.8, 0.5]], F32)
    return np.repeat(tri[None], n, 0)


def coplanar(n=65, seed=3):
    """a soup in the plane y = 0.5: the scene box has no extent along y"""
    rng = np.random.RandomState(seed)
    c = rng.uniform(-1, 1, (n, 1, 3))
    tri = c + rng.uniform(-0.2, 0.2, (n, 3, 3))
    tri[:, :, 1] = 0.5
    return tri.astype(F32)


def one_bit():
    """30 small triangles whose centres lie in the cells with one bit set on one axis, between two points that pin the scene box to
    [0, 1024]^3 (codes 0 and 2^30 - 1): 32 codes of which 30 have one bit, the radix tree a chain"""
    tri = [np.zeros((3, 3)), np.full((3, 3), 1024.0)]
    off = np.array([[-0.1, -0.1, -0.1], [0.1, -0.1, 0.1], [0.0, 0.1, 0.0]])
    for axis in range(3):
        for bit in range(10):
            c = np.full(3, 0.5)
            c[axis] = (1 << bit) + 0.5
            tri.append(c + off)
    return np.array(tri, F32)


def soup_triangles(n):
    return deep_walk.triangles(flat_limits.soup(n, "mixed", 1))


def triangle_scene(tri):
    """a triangle set as a one-mesh scene (ray queries and array comparisons: no emitter)"""
    return dict(meshes=[deep_walk._mesh(tri, 0)], bsdfs=[dict(type="diffuse", reflectance=np.array([0.6, 0.5, 0.4], F32))], emitters=[])


def raw_text(label, tri):
    return ["raw " + label, "P " + vm._hex(np.ascontiguousarray(tri, F32))]


def morton_codes(tri):
    """the 30-bit codes of build_lbvh, recomputed in numpy (float64 from the float32 boxes, as the specification)"""
    tri = np.asarray(tri, F32).reshape(-1, 3, 3)
    lo, hi = tri.min(1), tri.max(1)
    slo, shi = lo.min(0), hi.max(0)
    c = (F32(0.5) * (lo + hi)).astype(F32)
    ext = (shi - slo).astype(F32)
    codes = np.zeros(len(tri), np.uint64)
    for k in range(3):
        if not ext[k] > 0:
            continue
        x = np.floor((c[:, k].astype(np.float64) - np.float64(slo[k])) / np.float64(ext[k]) * 1024.0)
        cell = np.clip(x, 0, 1023).astype(np.uint64)
        for b in range(10):
            codes |= ((cell >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - k)
    return codes


class Driver:
    """tests/lbvh_driver.cpp compiled with the host builder; `flags`: extra compiler flags (a sanitizer build)"""

    def __init__(self, directory, flags=()):
        self.directory = str(directory)
        self.exe = os.path.join(self.directory, "lbvh_driver")
        subprocess.check_call([vm.HIPCC, "-std=c++17", "-O1", "-ffp-contract=off", "-I", vm.CSRC, "-o", self.exe] + list(flags) +
                              ["-x", "hip", "--cuda-host-only", os.path.join(vm.HERE, "lbvh_driver.cpp"), os.path.join(vm.CSRC, "scene_build.cpp"), "-x", "c++"] +
                              [os.path.join(vm.CSRC, f) for f in ("bvh.cpp", "envmap.cpp", "spectral_upsampling.cpp")], stderr=subprocess.DEVNULL)

    def run(self, sd, commands, name="scene"):
        path = os.path.join(self.directory, name + ".txt")
        with open(path, "w") as f:
            f.write("\n".join((vm.description_text(sd) if sd is not None else []) + list(commands)) + "\n")
        out = {}
        for line in subprocess.check_output([self.exe, path], text=True).splitlines():
            key, _, rest = line.partition(" ")
            if key.endswith(".rc"):
                out[key] = int(rest)
            elif key.endswith(".message"):
                out[key] = rest
            else:
                out[key] = hex_words(rest)
        return out


def hex_words(text):
    """the words of one dumped line: every word is printed as %08x, so the digits without the blanks are the big-endian bytes (a
    32 769-triangle dump holds millions of words: int(w, 16) word by word takes seconds)"""
    return np.frombuffer(bytes.fromhex(text.replace(" ", "")), dtype=">u4").astype(np.uint32)


COUNTS = ("root", "wroot", "wdepth", "n_nodes", "n_wnodes", "n_slots", "depth", "stack_depth")
NODE_ARRAYS = ("nodes", "qnodes", "wnodes", "wnodes_h", "wnodes_p", "tris", "grid")
TABLE_ARRAYS = ("kids", "order", "node_child", "wide_child", "boxes", "slot_prim")


def counts(out, label):
    return dict(zip(COUNTS, (int(x) for x in out[label + ".counts"])))


def sah(out, label):
    return float(out[label + ".sah"].view(np.float64)[0])

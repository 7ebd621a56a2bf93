"""Meshes, the host specification and the host driver shared by tests/test_vertex_normals_cpu.py and tests/test_gpu_vertex_normals.py.

`spec(positions, faces)` is mtsamd_compute_vertex_normals, the library's fp32 restatement of recompute_vertex_normals: it needs no scene
and no GPU.  tests/normals_driver.cpp is the same code as a stand-alone program (`Driver`, compiled as vertex_moves.Driver compiles
its own), which also runs the device's gather on the host and which a sanitizer build can run.

The edge meshes.  Small integers and binary fractions where a sum has to cancel exactly:
* fan: an apex with 300 incident faces on a bumpy rim;
* an isolated vertex, in no face;
* two coincident faces of opposite winding: normals and angles are exact, so each of their three vertices sums to exactly zero;
* strip257: a triangle strip of 257 vertices (one more than a block of the device's kernels);
* tiny_huge: one face with edges of 1e-30 and 1e10, whose cross product is a positive denormal while one squared edge length is 0;
* overflowing: one face whose edges overflow fp32."""
import ctypes as C
import os
import subprocess

import numpy as np

import vertex_moves as vm

F32 = np.float32
FAN_FACES = 300


def spec(positions, faces):
    from mitsuba2_amd import _lib as L
    pos = np.ascontiguousarray(positions, F32).reshape(-1, 3)
    fcs = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    out = np.full(pos.shape, np.nan, F32)
    L.check(L.lib().mtsamd_compute_vertex_normals(len(pos), pos.ctypes.data_as(C.c_void_p), len(fcs), fcs.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def bits(a):
    return np.ascontiguousarray(a, F32).reshape(-1).view(np.uint32)


# ---- meshes: (positions (N, 3) float32, faces (M, 3) uint32) -----------------------------------------------------------------------------
def fan(n=FAN_FACES):
    t = 2.0 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(t), 0.1 * np.sin(5.0 * t), np.sin(t)], 1)
    pos = np.concatenate([[[0.0, 0.4, 0.0]], rim]).astype(F32)
    i = np.arange(n)
    return pos, np.stack([np.zeros(n, np.int64), 1 + (i + 1) % n, 1 + i], 1).astype(np.uint32)        # the apex normal points up


def cancelling():
    return np.array([[3, 0, 0], [4, 0, 0], [3, 1, 0]], F32), np.array([[0, 1, 2], [0, 2, 1]], np.uint32)


def strip257():
    i = np.arange(257)
    pos = np.stack([0.01 * i, 0.1 * (i % 2), 0.02 * np.sin(0.37 * i)], 1).astype(F32)
    f = np.arange(255)
    faces = np.where((f % 2 == 0)[:, None], np.stack([f, f + 1, f + 2], 1), np.stack([f + 1, f, f + 2], 1))
    return pos, faces.astype(np.uint32)


def tiny_huge():
    return np.array([[0, 0, 0], [1e-30, 0, 0], [0, 1e10, 0]], F32), np.array([[0, 1, 2]], np.uint32)


def overflowing():
    return np.array([[-3e38, 0, 0], [3e38, 0, 0], [0, 3e38, 0]], F32), np.array([[0, 1, 2]], np.uint32)


def join(*meshes):
    """one mesh of several: the vertices one after another, the face indices shifted"""
    pos, faces, base = [], [], 0
    for p, f in meshes:
        pos.append(np.asarray(p, F32).reshape(-1, 3)); faces.append(np.asarray(f, np.uint32).reshape(-1, 3) + np.uint32(base))
        base += len(pos[-1])
    return np.concatenate(pos), np.concatenate(faces)


ISOLATED = (np.array([[5.0, 5.0, 5.0]], F32), np.zeros((0, 3), np.uint32))
# vertex ranges of edge_mesh(): the apex is vertex 0, the isolated vertex follows the rim, the cancelling faces' vertices come last
EDGE_APEX, EDGE_ISOLATED, EDGE_CANCELLING = 0, FAN_FACES + 1, slice(FAN_FACES + 2, FAN_FACES + 5)


def edge_mesh():
    return join(fan(), ISOLATED, cancelling())


# ---- the host driver ---------------------------------------------------------------------------------------------------------------------
class Driver:
    """tests/normals_driver.cpp compiled with the host builder; `flags`: extra compiler flags (a sanitizer build)"""

    def __init__(self, directory, flags=()):
        self.directory = str(directory)
        self.exe = os.path.join(self.directory, "normals_driver")
        subprocess.check_call([vm.HIPCC, "-std=c++17", "-O1", "-ffp-contract=off", "-I", vm.CSRC, "-o", self.exe] + list(flags) +
                              ["-x", "hip", "--cuda-host-only", os.path.join(vm.HERE, "normals_driver.cpp"), os.path.join(vm.CSRC, "scene_build.cpp"), "-x", "c++"] +
                              [os.path.join(vm.CSRC, f) for f in ("bvh.cpp", "envmap.cpp", "spectral_upsampling.cpp")], stderr=subprocess.DEVNULL)

    def run(self, meshes, name="meshes"):
        """meshes: {label: (positions, faces)} -> {label.normals / label.gathered: (N, 3) float32, label.skipped: int}"""
        path = os.path.join(self.directory, name + ".txt")
        with open(path, "w") as f:
            for label, (pos, faces) in meshes.items():
                pos, faces = np.ascontiguousarray(pos, F32).reshape(-1, 3), np.asarray(faces, np.uint32).reshape(-1, 3)
                f.write("mesh %s %d %d\nP %s\nF %s\n" % (label, len(pos), len(faces), vm._hex(pos), " ".join(str(int(x)) for x in faces.reshape(-1))))
        out = {}
        for line in subprocess.check_output([self.exe, path], text=True).splitlines():
            key, _, rest = line.partition(" ")
            if key.endswith(".skipped"):
                out[key] = int(rest)
            else:
                out[key] = np.array([int(w, 16) for w in rest.split()], np.uint32).view(F32).reshape(-1, 3)
        return out

"""The two scene sizes of tests/test_gpu_adjoint_hierarchy.py, and what they mean for a hierarchy-scene launch.  The fused kernels
(k_bounce, k_direct, the four adjoint kernels) keep the whole traversal stack of their 256 lanes in dynamic LDS:
8 B x (3 * wdepth + 2) x 256 (mitsuba2_amd/csrc/api.cpp, bounce_lds_bytes).  The GPU tests call their sizes "shallow" (at most 48 KiB,
what every launch may ask for without more ado) and "deep" (above 64 KiB, the size of the benchmark's mesh); here bvh.cpp is compiled
for the host and that claim is checked on the scenes' own triangles, with the shipped builder options.  The classes are asserted, not
the depths: a builder change that moves a scene out of its class asks for another size in HIERARCHY_SIZES."""
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from mitsuba2_amd import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mitsuba2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

HIERARCHY_SIZES = {"shallow": (12, 24), "deep": (256, 512)}      # bumpy_sphere(n_theta, n_phi)
TEX_SHAPE = (4, 5, 3)


@functools.lru_cache(maxsize=None)
def _base(n_theta, n_phi):
    return scenes.bumpy_sphere(n_theta, n_phi)


def hierarchy_texture(value=None):
    """the ground's bitmap: 4 x 5 texels in 0.3 .. 0.8, or uniform"""
    if value is not None:
        return np.full(TEX_SHAPE, value, np.float32)
    return (0.3 + 0.5 * np.random.RandomState(1).rand(*TEX_SHAPE)).astype(np.float32)


def hierarchy_scene(size, sphere=None, ground=None, tex=None, envmap=None, area=True):
    """bumpy_sphere of the given size class: BSDF ids 'sphere', 'ground', 'light', the lamp's shape 'lamp', texcoords on the ground quad and
    a bitmap `diffuse` on it.  `sphere` / `ground` replace those BSDFs (the id is kept); `envmap` = texels of an envmap emitter
    'sky' (emitter 0; the area light, if kept, becomes emitter 1); area=False drops the lamp.  Returns (scene dict, texels)."""
    base = _base(*HIERARCHY_SIZES[size])
    tex = hierarchy_texture() if tex is None else tex
    meshes = [dict(m) for m in base["meshes"]]
    meshes[1]["texcoords"] = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    meshes[2]["id"] = "lamp"
    bsdfs = [dict(base["bsdfs"][0]) if sphere is None else dict(sphere),
             dict(type="diffuse", reflectance=dict(type="bitmap", data=tex)) if ground is None else dict(ground), dict(base["bsdfs"][2])]
    for b, n in zip(bsdfs, ("sphere", "ground", "light")):
        b["id"] = n
    emitters = [dict(e) for e in base["emitters"]]
    if not area:
        meshes, emitters = meshes[:2], []
    if envmap is not None:
        emitters = [{"type": "envmap", "id": "sky", "data": envmap, "scale": 0.8, "to_world": scenes.look_at([0, 0, 0], [1, 0.2, 0.3], [0, 1, 0])}] + emitters
        for m in meshes:
            if m.get("emitter", -1) >= 0:
                m["emitter"] = 1
    return dict(meshes=meshes, bsdfs=bsdfs, emitters=emitters), tex


def hierarchy_sensor(w, h, spp, max_depth, rfilter="box", seed=5):
    return dict(scenes.bumpy_sphere_sensor(w, h, spp, seed=seed, max_depth=max_depth), rfilter=rfilter, rfilter_param=0.5)


PROGRAM = r"""
#include "bvh.h"
#include <cstdio>
#include <vector>
using namespace mtsamd;
int main(int argc, char **argv) {
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<float> tri;
    float buf[9 * 1024];
    for (size_t n; (n = std::fread(buf, sizeof(float), 9 * 1024, f)) > 0;) tri.insert(tri.end(), buf, buf + n);
    std::fclose(f);
    if (tri.empty() || tri.size() % 9) return 3;
    BvhOutput out;
    build_bvh(tri.data(), (uint32_t) (tri.size() / 9), 4u, out);        // max_leaf and options as mtsamd_scene_create has them
    std::printf("%u %u\n", (uint32_t) (tri.size() / 9), out.wdepth);
    return 0;
}
"""


def _triangles(sd):
    """9 floats per primitive in mesh order, as mtsamd_scene_create hands them to the builder"""
    return np.concatenate([np.asarray(m["positions"], np.float32).reshape(-1, 3)[np.asarray(m["faces"]).reshape(-1, 3)].reshape(-1, 9)
                           for m in sd["meshes"]])


@pytest.fixture(scope="module")
def bvh_driver():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "t.cpp"), os.path.join(tmp, "t")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.check_call([HIPCC, "-std=c++17", "-O2", "-I", CSRC, "-o", exe, src, os.path.join(CSRC, "bvh.cpp")],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

        def run(sd):
            path = os.path.join(tmp, "tri.bin")
            _triangles(sd).tofile(path)
            n, wdepth = (int(x) for x in subprocess.check_output([exe, path]).split())
            return n, wdepth
        yield run


@pytest.mark.parametrize("size", ["shallow", "deep"])
def test_traversal_stack_class_of_the_hierarchy_scenes(bvh_driver, size):
    sd, _ = hierarchy_scene(size)
    n, wdepth = bvh_driver(sd)
    assert n == sum(len(m["faces"]) for m in sd["meshes"]) and n > 64          # a hierarchy scene (kFlatMaxPrims = 64)
    lds = 8 * 256 * (3 * wdepth + 2)
    if size == "shallow":
        assert lds <= 48 * 1024, (n, wdepth, lds)
    else:
        assert 64 * 1024 < lds <= 150 * 1024, (n, wdepth, lds)              # 150 KiB: the limit mtsamd_scene_create enforces

"""The "cannot reach a light" test of fated paths (mitsuba2_amd/csrc/fated.h), compiled here for the host with the records of the host builder
(tests/fated_box_driver.cpp: emitter_exact_box + set_emitter_boxes of scene_build.cpp): it is conservative.  No ray for which the scalar
restatement of the pair test accepts an EMISSIVE triangle within [mint, maxt] is ever called "cannot reach" -- with the reciprocals exact,
an ulp off either way (v_rcp_f32) and with denormal direction components read as zero -- on the Cornell box, on the box scaled by 1e-3 and
1e3 and moved 1e3 of its size off the origin, and on a dozen random soups with random emissive subsets (1-4 emitters; five: the list is
empty and the elision off).  The rays are those of test_flat_cull_cpu.py (50 000 per scene: stress_rays.py plus interior rays, zero / -0 /
denormal direction components, finite maxt, far origins) and 10 000 aimed at, and just beside, the emissive triangles.  The padded boxes
contain the exact boxes plus the cluster boxes' pad; an invalidated record is reached by every ray whose segment is not empty; the test is not vacuous (on the
Cornell box most interior rays do NOT reach the luminaire's box).
The roulette peek: fated_peek_f32 returns what the oracle's mo_pcg32_next_f32 returns next, bit for bit, and fated_decide agrees with the
depth test and the roulette of the step written out with that generator."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import flat_limits as fl
from mitsuba2_amd import scenes
from stress_rays import tris, unit
from test_flat_cull_cpu import all_rays, moved

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "mitsuba2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
F32 = np.float32


def emissive_soup(n_tris, n_emitters, seed):
    """n_tris random triangles, one mesh each; a random subset of them emits, dealt to n_emitters emitters (each gets at least one)"""
    rng = np.random.RandomState(seed)
    tri = fl.soup_triangles(n_tris, seed)
    n_lit = int(rng.randint(n_emitters, max(n_emitters, n_tris // 3) + 1))
    lit = rng.permutation(n_tris)[:n_lit]
    owner = np.full(n_tris, -1, np.int32)
    owner[lit] = np.concatenate([np.arange(n_emitters), rng.randint(0, n_emitters, n_lit - n_emitters)]).astype(np.int32)
    meshes = [dict(fl._mesh(tri[k:k + 1], 0), emitter=int(owner[k])) for k in range(n_tris)]
    return dict(meshes=meshes, bsdfs=[dict(type="diffuse", reflectance=np.full(3, 0.5, F32))],
                emitters=[dict(type="area", radiance=np.ones(3, F32)) for _ in range(n_emitters)])


def aimed_rays(sd, prim_emitter, seed, n=10000):
    """rays towards points of the emissive triangles: inside, on the edges and vertices, and just outside; from inside the scene's box and
    from other surfaces (mint as the shading code sets it), infinite and finite maxt (ending on, before and behind the target)"""
    rng = np.random.RandomState(seed)
    tri = tris(sd)
    allp = tri.reshape(-1, 3)
    lo, hi = allp.min(0), allp.max(0)
    lit = np.nonzero(prim_emitter >= 0)[0]
    k = lit[rng.randint(0, len(lit), n)]
    b = rng.rand(n, 2)
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    b = np.where(rng.rand(n, 1) < 0.3, np.round(b), b)                         # vertices and edges
    b = b + np.where(rng.rand(n, 1) < 0.3, 1e-3 * rng.randn(n, 2), 0.0)        # just beside
    tgt = (tri[k, 0] + b[:, :1] * (tri[k, 1] - tri[k, 0]) + b[:, 1:] * (tri[k, 2] - tri[k, 0])).astype(F32)
    j = rng.randint(0, len(tri), n)
    c = rng.rand(n, 2) * 0.5
    on_surface = tri[j, 0] + c[:, :1] * (tri[j, 1] - tri[j, 0]) + c[:, 1:] * (tri[j, 2] - tri[j, 0])
    o = np.where(rng.rand(n, 1) < 0.5, lo + (hi - lo) * rng.rand(n, 3), on_surface).astype(F32)
    dist = np.linalg.norm(tgt.astype(np.float64) - o, axis=1)
    keep = dist > 0
    d = unit(np.where(keep[:, None], tgt - o, 1.0))
    factor = np.array([1.0, 1.0 - 1e-4, 1.0 + 1e-4, 3.0], F32)[rng.randint(0, 4, n)]
    maxt = np.where(rng.rand(n) < 0.5, np.inf, dist * factor).astype(F32)
    mint = np.where(np.arange(n) % 2 == 0, 0.0, 1e-4 * (1 + np.abs(o).max(1))).astype(F32)
    return np.ascontiguousarray(np.concatenate([o, d, mint[:, None], maxt[:, None]], 1)[keep], F32)


def fated_scenes():
    cb = scenes.cornell_box()
    size = 559.2
    out = {"cornell": cb, "cornell_1e-3": moved(cb, 1e-3), "cornell_1e3": moved(cb, 1e3), "cornell_far": moved(cb, 1.0, 1e3 * size)}
    rng = np.random.RandomState(17)
    shapes = [(4, 1), (9, 2), (64, 4), (64, 1), (33, 3), (12, 4), (20, 5)] + [(int(rng.randint(6, 65)), int(rng.randint(1, 5))) for _ in range(5)]
    for n_tris, n_emitters in shapes:
        out["soup_%d_%d_%d" % (n_tris, n_emitters, len(out))] = emissive_soup(n_tris, n_emitters, 40 + len(out))
    return out


def write_input(path, named):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(named)))
        for i, (name, sd) in enumerate(named.items()):
            tri = tris(sd)
            prim_emitter = np.concatenate([np.full(len(np.asarray(m["faces"]).reshape(-1, 3)), m["emitter"], np.int32) for m in sd["meshes"]])
            rays, _ = all_rays(sd, 5 + i)
            rays = np.ascontiguousarray(np.concatenate([rays, aimed_rays(sd, prim_emitter, 70 + i)]), F32)
            assert len(rays) >= 50000
            f.write(struct.pack("<I", len(name)) + name.encode())
            f.write(struct.pack("<II", len(tri), len(sd["emitters"])) + prim_emitter.tobytes() + np.ascontiguousarray(tri, F32).tobytes())
            f.write(struct.pack("<I", len(rays)) + rays.tobytes())


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    tmp = tmp_path_factory.mktemp("fated_box")
    exe = str(tmp / "driver")
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, "-I", os.path.join(ROOT, "oracle"), "-o", exe, "-x", "hip", "--cuda-host-only",
                           os.path.join(HERE, "fated_box_driver.cpp"), os.path.join(CSRC, "scene_build.cpp"), "-x", "c++"] +
                          [os.path.join(CSRC, f) for f in ("bvh.cpp", "envmap.cpp", "spectral_upsampling.cpp")], stderr=subprocess.DEVNULL)
    return exe, tmp


@pytest.fixture(scope="module")
def report(driver):
    exe, tmp = driver
    path = str(tmp / "input.bin")
    named = fated_scenes()
    write_input(path, named)
    out = {}
    for line in subprocess.check_output([exe, "boxes", path], text=True).splitlines():
        print(line)
        w = line.split()
        assert w[0] == "scene", line
        out[w[1]] = {k: int(v) for k, v in zip(w[2::2], w[3::2])}
    assert set(out) == set(named)
    return out


def test_no_ray_that_meets_an_emissive_triangle_is_called_unreachable(report):
    for name, r in report.items():
        assert r["violations"] == 0 and r["bad_records"] == 0 and r["invalid_missed"] == 0, (name, r)
        if r["emitters"] <= 4:
            assert r["list"] != 0 and r["need"] > 2000 and r["reached"] >= r["need"], (name, r)      # the aimed rays do meet the lights
        else:
            assert r["list"] == 0, (name, r)                                                           # over the cap: off


def test_the_box_test_is_not_vacuous_on_the_cornell_box(report):
    for name in ("cornell", "cornell_1e-3", "cornell_1e3", "cornell_far"):
        r = report[name]
        assert r["emitters"] == 1 and 2 * r["reached"] < r["rays"], (name, r)      # the luminaire is a small part of the ceiling


def test_roulette_peek_and_decision(driver):
    exe, _ = driver
    line = subprocess.check_output([exe, "peek"], text=True).strip()
    print(line)
    w = line.split()
    r = {k: int(v) for k, v in zip(w[1::2], w[2::2])}
    assert r["n"] == 4096 * 64 and r["peek_mismatch"] == 0 and r["decide_mismatch"] == 0
    assert r["n"] // 10 < r["fated"] < r["n"] - r["n"] // 10          # both outcomes occur

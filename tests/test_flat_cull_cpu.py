"""The cluster cull in front of every flat-scene ray query (mitsuba2_amd/csrc/flat_cull.h), compiled here for the host with the records of
the host builder (tests/flat_cull_driver.cpp): the cull is conservative.  For every ray, every triangle that a scalar restatement of the
pair test accepts within [mint, maxt] has its pair's bit set by the reach predicate -- in both of its forms, the work lists' and the
clustered loops'; with the reciprocals exact, an ulp off either way
(v_rcp_f32) and with denormal direction components read as zero -- on the Cornell box, on random soups of 1-64 triangles in 1-8 shapes, on
the box scaled by 1e-3 and 1e3 and on the box moved 1e3 of its size off the origin; with the rays of stress_rays.py (origins on surfaces
with mint = eps (1 + |p|), axis-parallel and grazing directions, exact ties, segments that end on a surface), interior rays, direction
components of 0, -0 and denormals, finite and infinite maxt, and origins 100 extents away.  The centre / half-extent boxes contain the
padded boxes they encode, the counts and pair masks are right, and the new form flags at most 1 % more (ray, cluster) tests than the lo /
hi form on the Cornell set: outward rounding widens a box by ulps, more would be a loose box."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import flat_limits as fl
from mitsuba2_amd import scenes
from stress_rays import stress_rays, tris, unit

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mitsuba2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
F32 = np.float32
INTERIOR = 1


def moved(sd, scale=1.0, shift=0.0):
    """the scene with every vertex at (p * scale + shift), rounded to float32 once"""
    return dict(sd, meshes=[dict(m, positions=(np.asarray(m["positions"], np.float64) * scale + shift).astype(F32)) for m in sd["meshes"]])


def soup(n_tris, n_shapes, seed):
    """n_tris random triangles (flat_limits.soup_triangles) cut into n_shapes runs of random lengths"""
    rng = np.random.RandomState(seed)
    tri = fl.soup_triangles(n_tris, seed)
    n_shapes = min(n_shapes, n_tris)
    cuts = np.sort(rng.choice(np.arange(1, n_tris), n_shapes - 1, replace=False)) if n_shapes > 1 else np.array([], int)
    return dict(meshes=[fl._mesh(t, 0) for t in np.split(tri, cuts)], bsdfs=[dict(type="diffuse", reflectance=np.full(3, 0.5, F32))], emitters=[])


def extra_rays(sd, seed):
    """(o, d, mint, maxt, kind) beyond stress_rays: interior rays, zero / -0 / denormal direction components, finite maxt, far origins"""
    rng = np.random.RandomState(seed)
    tri = tris(sd)
    allp = tri.reshape(-1, 3)
    lo, hi = allp.min(0), allp.max(0)
    size = float(np.abs(hi - lo).max())
    groups = []
    inf = lambda n: np.full(n, np.inf, F32)
    # interior rays: origins inside the bounding box, directions all over the sphere
    n = 4000
    o = (lo + (hi - lo) * rng.rand(n, 3)).astype(F32)
    groups.append((o, unit(rng.randn(n, 3)), np.zeros(n, F32), inf(n), np.full(n, INTERIOR, np.uint32)))
    # one or two direction components drawn from 0, -0, denormals and the smallest normals; origins inside the box and on surfaces.  (Not on
    # vertices: an axis-parallel ray from a vertex of one of the two boxes runs inside the planes of their upright faces, where Moeller-Trumbore
    # is ill-posed -- det is the rounding error of a product, u = v = 0 and t is noise -- and once the coordinates are inexact (the box
    # scaled by 1e-3) such a triangle can be accepted at a t that lies nowhere near it.  No box is conservative against that: the lo / hi
    # form misses the same triangle.  The vertex origins of stress_rays, axis-parallel ones included, stay as they are.)
    n = 6000
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754942e-38, -1.1754942e-38, 1.1754944e-38, -1.1754944e-38, 1e-30, -1e-30], F32)
    d = unit(rng.randn(n, 3))
    for k in range(n):
        axes = rng.permutation(3)[:1 + (k % 2)]
        d[k, axes] = tiny[rng.randint(0, len(tiny), len(axes))]
    k = rng.randint(0, len(tri), n)
    b = rng.rand(n, 2).astype(F32) * 0.5
    on_surface = tri[k, 0] + b[:, :1] * (tri[k, 1] - tri[k, 0]) + b[:, 1:] * (tri[k, 2] - tri[k, 0])
    o = np.where(rng.rand(n, 1) < 0.5, lo + (hi - lo) * rng.rand(n, 3), on_surface).astype(F32)
    mint = np.where(np.arange(n) % 2 == 0, 0.0, 1e-4 * (1 + np.abs(o).max(1))).astype(F32)
    groups.append((o, d, mint, inf(n), np.zeros(n, np.uint32)))
    # segments: maxt finite, ending on, just before and just behind a point of a surface (shadow rays), and random lengths
    n = 6000
    k = rng.randint(0, len(tri), n)
    b = rng.rand(n, 2).astype(F32) * 0.5
    tgt = (tri[k, 0] + b[:, :1] * (tri[k, 1] - tri[k, 0]) + b[:, 1:] * (tri[k, 2] - tri[k, 0])).astype(F32)
    o = (lo + (hi - lo) * rng.rand(n, 3)).astype(F32)
    dist = np.linalg.norm(tgt - o, axis=1)
    factor = np.array([1.0, 1.0 - 1e-4, 1.0 + 1e-4, 0.5, 3.0], F32)[rng.randint(0, 5, n)]
    maxt = np.where(rng.rand(n) < 0.2, size * rng.rand(n), dist * factor).astype(F32)
    mint = np.where(np.arange(n) % 2 == 0, 0.0, 1e-4 * (1 + np.abs(o).max(1))).astype(F32)
    groups.append((o, unit(tgt - o), mint, maxt, np.zeros(n, np.uint32)))
    # origins 100 extents away, aimed at points of the surfaces and of the bounding box, half of them axis-parallel
    n = 4000
    tgt = np.where(rng.rand(n, 1) < 0.5, tgt[:n], lo + (hi - lo) * rng.rand(n, 3))
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    d = np.where(rng.rand(n, 1) < 0.5, axes[rng.randint(0, 6, n)], unit(rng.randn(n, 3))).astype(F32)
    o = (tgt - 100.0 * size * d).astype(F32)
    maxt = np.where(rng.rand(n) < 0.3, 100.0 * size, np.inf).astype(F32)
    groups.append((o, d, np.zeros(n, F32), maxt, np.zeros(n, np.uint32)))
    return tuple(np.concatenate([g[i] for g in groups]) for i in range(5))


def all_rays(sd, seed):
    o, d, mint, maxt = stress_rays(sd, seed)
    xo, xd, xmint, xmaxt, kind = extra_rays(sd, seed + 100)
    rays = np.concatenate([np.concatenate([o, xo]), np.concatenate([d, xd]), np.concatenate([mint, xmint])[:, None], np.concatenate([maxt, xmaxt])[:, None]], 1)
    return np.ascontiguousarray(rays, F32), np.concatenate([np.zeros(len(o), np.uint32), kind])


def cull_scenes():
    cb = scenes.cornell_box()
    size = 559.2
    out = {"cornell": cb, "cornell_1e-3": moved(cb, 1e-3), "cornell_1e3": moved(cb, 1e3), "cornell_far": moved(cb, 1.0, 1e3 * size)}
    rng = np.random.RandomState(11)
    for n_tris, n_shapes in [(1, 1), (2, 2), (3, 2), (5, 1), (64, 8), (64, 1), (63, 7)] + [(int(rng.randint(4, 65)), int(rng.randint(1, 9))) for _ in range(5)]:
        out["soup_%d_%d_%d" % (n_tris, n_shapes, len(out))] = soup(n_tris, n_shapes, 20 + len(out))
    return out


def write_input(path, named):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(named)))
        for i, (name, sd) in enumerate(named.items()):
            tri = tris(sd)
            prim_shape = np.concatenate([np.full(len(np.asarray(m["faces"]).reshape(-1, 3)), s, np.uint32) for s, m in enumerate(sd["meshes"])])
            rays, kind = all_rays(sd, 5 + i)
            f.write(struct.pack("<I", len(name)) + name.encode())
            f.write(struct.pack("<I", len(tri)) + prim_shape.tobytes() + np.ascontiguousarray(tri, F32).tobytes())
            f.write(struct.pack("<I", len(rays)) + rays.tobytes() + kind.tobytes())


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    tmp = tmp_path_factory.mktemp("flat_cull")
    exe, path = str(tmp / "driver"), str(tmp / "input.bin")
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, "-o", exe, "-x", "hip", "--cuda-host-only",
                           os.path.join(HERE, "flat_cull_driver.cpp"), os.path.join(CSRC, "scene_build.cpp"), "-x", "c++"] +
                          [os.path.join(CSRC, f) for f in ("bvh.cpp", "envmap.cpp", "spectral_upsampling.cpp")], stderr=subprocess.DEVNULL)
    named = cull_scenes()
    write_input(path, named)
    out = {}
    for line in subprocess.check_output([exe, path], text=True).splitlines():
        print(line)
        w = line.split()
        assert w[0] == "scene" and "not_flat" not in w, line
        out[w[1]] = {k: int(v) for k, v in zip(w[2::2], w[3::2])}
    assert set(out) == set(named)
    return out


def test_cull_never_rejects_an_accepted_triangle(report):
    for name, r in report.items():
        assert r["form"] == 1, "the library's default is the new form"
        assert r["violations"] == 0 and r["violations_lean"] == 0, (name, r)      # the work lists' query and the clustered loops' 
        assert r["bad_records"] == 0, (name, r)
        assert r["rays_hit"] > r["rays"] // 4, (name, r)               # every scene's rays do meet triangles


def test_cull_is_not_vacuous_on_the_cornell_box(report):
    r = report["cornell"]
    assert r["clusters"] == 8 and r["interior"] >= 4000
    assert 2 * r["interior_hit"] >= r["interior"], r                  # the box is closed on five sides


def test_cull_is_as_tight_as_the_lo_hi_form(report):
    r = report["cornell"]
    print("cornell: (ray, cluster) tests flagged: new form %d (work lists) / %d (clustered loops), lo / hi form %d, of %d" %
          (r["flagged"], r["flagged_lean"], r["flagged_form0"], r["rays"] * r["clusters"]))
    assert r["flagged_form0"] < r["rays"] * r["clusters"]             # the cull does cull
    assert r["flagged"] <= 1.01 * r["flagged_form0"] and r["flagged_lean"] <= 1.01 * r["flagged_form0"], r

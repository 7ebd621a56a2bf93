"""The scenes and ray sets of tests/test_gpu_deep_walk.py really force deep walks: checked on the host, with the shipped builder.

tests/deep_walk.py holds a stand-alone program that links bvh.cpp and prints, for every ray that misses every triangle, the
order-independent minimum peak P of an exhaustive depth-first walk over the BVH4 (a lower bound on the device's peak stack height
whatever its child order and box padding; the argument is next to the program).  A ray "reaches the spill" of a kernel that keeps
LDS_DEPTH entries in LDS when P > LDS_DEPTH; the ray sets must do so by a margin: P >= LDS_DEPTH + 4 (spill rows 0 .. 3 written and
read back) for the sets on 4096 slivers, P >= LDS_DEPTH + 1 for the smaller scene of the long stream.  The classes are asserted, not
the figures: a builder change that moves a scene out of its class asks for another scene (or seed) in deep_walk.py.

Measured with the builder as shipped (python -m pytest tests/test_deep_walk_cpu.py -s prints the histograms):
  slivers(4096), 8000 through rays:   wdepth 8, bound 26; 97.4 % miss everything, each with P = 12; nearest-first replay peaks at 18
  slivers(1024), 4096 through rays:   wdepth 6, bound 20; 97.4 % miss everything, each with P = 9;  replay 16
  render scene, 4096 primary rays:    wdepth 9, bound 29; 84.1 % certified, each with P = 12 (the others hit one of the four blades,
                                      in the middle of such a walk);                          replay 20 .. 22
  existing scenes (certified maximum of P over rays that miss): sphere_small 2, sphere_large 3, hierarchy shallow 2, deep 3"""
import os
import re

import numpy as np
import pytest

import deep_walk as dw
from deep_walk import LDS_DEPTH
from mitsuba2_amd import scenes
from test_bvh_depth_cpu import HIERARCHY_SIZES

ROOT = os.path.dirname(dw.HERE)


@pytest.fixture(scope="module")
def cert():
    if not os.path.exists(dw.HIPCC):
        pytest.skip("hipcc not installed")
    with dw.make_certificate() as c:
        yield c


def _report(name, r):
    P, ok = r["P"], r["P"] >= 0
    line = ("%s: %d triangles, wdepth %d, stack bound %d, longest path %d; %d rays, %.1f %% miss every triangle; certified P histogram %s; "
            "nearest-first replay histogram %s" % (name, r["n"], r["wdepth"], 3 * r["wdepth"] + 2, r["longest"], len(P), 100.0 * ok.mean(),
                                                   dict(zip(*(x.tolist() for x in np.unique(P[ok], return_counts=True)))),
                                                   dict(zip(*(x.tolist() for x in np.unique(r["replay"][ok], return_counts=True))))))
    print(line)
    return line


def check_class(name, r, need, share):
    """at least `share` of the rays miss every triangle and are certified at P >= need; the stack bound holds and fits the LDS limit"""
    line = _report(name, r)
    bound = 3 * r["wdepth"] + 2
    assert r["longest"] <= bound, line                              # sum(children - 1) + 2 along the longest root-to-leaf path
    assert need < bound, line
    assert 8 * 256 * bound < 150 * 1024, line                       # what mtsamd_scene_create accepts (bounce_lds_bytes)
    got = float((r["P"] >= need).mean())
    assert got >= share, "%.1f %% of the rays are certified at P >= %d, %.0f %% are needed\n%s" % (100.0 * got, need, 100.0 * share, line)


def _oracle_misses(oracle, sd, rays, certified):
    """the certified rays miss in the arithmetic of the kernels too (the oracle's brute force is their reference): `best` never drops"""
    t = oracle.OracleScene(sd).ray_intersect(*rays, naive=True)[0]
    assert np.isinf(t[certified]).all(), int(np.isfinite(t[certified]).sum())


def test_lds_depth_is_what_the_kernels_share():
    """LDS_DEPTH and RAY_CHUNK restate constants of the sources (the library does not export them); a change there asks for another
    margin here.  The patterns only look for the name and the first BVH4 number after it, whatever the layout of the line."""
    api = open(os.path.join(dw.CSRC, "api.cpp")).read()
    hip = open(os.path.join(dw.CSRC, "kernels.hip")).read()

    def number(text, pattern):
        m = re.search(pattern, text, re.S)
        assert m, pattern
        return int(m.group(1))
    assert number(api, r"walk_lds_depth\s*=[^;]*?MTS_BVH4\s*\?\s*(\d+)") == LDS_DEPTH
    assert number(hip, r"kFinishLdsDepth\s*=\s*(\d+)") == LDS_DEPTH
    assert number(hip, r"define\s+MTS_TRACE_LDS_DEPTH[^\n]*?:\s*(\d+)\s*\)") == LDS_DEPTH          # the 256-thread workgroup's value
    assert number(hip, r"kRayChunk\s*=\s*(\d+)u?\s*\*\s*kBlock") * number(hip, r"kBlock\s*=\s*(\d+)") == dw.RAY_CHUNK


def test_query_rays_reach_the_spill(cert, oracle):
    sd = dw.slivers(dw.QUERY_K)
    rays = dw.query_rays()
    through, aimed = tuple(x[:dw.QUERY_THROUGH] for x in rays), tuple(x[dw.QUERY_THROUGH:] for x in rays)
    r = cert(dw.triangles(sd), through)
    check_class("slivers(%d), through rays" % dw.QUERY_K, r, LDS_DEPTH + 4, 0.8)
    _oracle_misses(oracle, sd, through, r["P"] >= 0)
    # the aimed rays are there for real hits: two thirds are unbounded and pass through a point well inside a sliver
    t = oracle.OracleScene(sd).ray_intersect(*aimed, naive=True)[0]
    assert np.isfinite(t).sum() >= dw.QUERY_AIMED // 2, np.isfinite(t).sum()
    _report("slivers(%d), aimed rays (%d hit)" % (dw.QUERY_K, np.isfinite(t).sum()), cert(dw.triangles(sd), aimed))


def test_stream_rays_reach_the_spill(cert, oracle):
    sd = dw.slivers(dw.STREAM_K)
    rays = dw.stream_tile()
    r = cert(dw.triangles(sd), rays)
    check_class("slivers(%d), stream tile" % dw.STREAM_K, r, LDS_DEPTH + 1, 0.8)
    _oracle_misses(oracle, sd, rays, r["P"] >= 0)
    idx = dw.stream_index(3 * dw.STREAM_TILE + 5)
    assert all(sorted(idx[k:k + dw.STREAM_TILE].tolist()) == list(range(dw.STREAM_TILE)) for k in (0, dw.STREAM_TILE))      # whole tiles: permutations
    assert not np.array_equal(idx[:dw.STREAM_TILE], idx[dw.STREAM_TILE:2 * dw.STREAM_TILE])


def test_render_scene_walks_deep_and_is_lit(cert, oracle):
    sd = dw.deep_render_scene()
    rays = dw.primary_rays(oracle)
    r = cert(dw.triangles(sd), rays)
    check_class("render scene, primary rays up to y = 0.3", r, LDS_DEPTH + 4, 0.5)
    _oracle_misses(oracle, sd, rays, r["P"] >= 0)
    p = dw.deep_render_sensor()
    n = p["width"] * p["height"] * p["sample_count"]
    assert n <= 8192
    for desc in (p, dict(p, integrator="direct", emitter_samples=1, bsdf_samples=1)):
        rgba, _ = oracle.OracleScene(sd, naive=True).sample_radiance(oracle.make_desc(desc), 0, n)
        lit = float((rgba[:, :3].max(1) > 0).mean())
        print("render scene, %s: %.1f %% of %d samples have a non-zero oracle radiance" % (desc.get("integrator", "path"), 100.0 * lit, n))
        assert lit >= 0.02, lit                                     # the GPU comparison is not one of zeros


def test_existing_scenes_stay_in_lds(cert):
    """on record: the scenes the suite had before do not reach the spill area (certified maxima, rays drawn as their tests draw them)"""
    for name, sd, n in (("sphere_small", scenes.bumpy_sphere(12, 24), 4000), ("sphere_large", scenes.bumpy_sphere(96, 192), 4000),
                        ("hierarchy shallow", scenes.bumpy_sphere(*HIERARCHY_SIZES["shallow"]), 4000),
                        ("hierarchy deep", scenes.bumpy_sphere(*HIERARCHY_SIZES["deep"]), 1000)):
        r = cert(dw.triangles(sd), dw.box_rays(sd, n, 11))
        _report(name, r)
        print("%s: certified maximum %d of a bound of %d, nearest-first replay maximum %d (LDS part: %d)"
              % (name, r["P"].max(), 3 * r["wdepth"] + 2, r["replay"].max(), LDS_DEPTH))
        assert r["longest"] <= 3 * r["wdepth"] + 2


def test_certificate_under_sanitizers(cert):
    """the program is stand-alone, so AddressSanitizer and UBSan can watch the builder on these inputs: the slivers (nearly equal boxes),
    and K triangles that share both far vertices exactly -- all centroids equal, the binned SAH has no axis to split"""
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1")
    if not dw.compiler_has_runtime(flags[:1]):
        pytest.skip("the compiler's sanitizer runtime is not installed")
    with dw.make_certificate(flags) as san:              # a failure of this build is a failure, with the compiler's output
        equal = dw.sliver_triangles(300)
        equal[:, 0], equal[:, 1] = 0.0, 1.0
        for tri, rays in ((dw.triangles(dw.slivers(dw.STREAM_K)), tuple(x[:64] for x in dw.stream_tile())),
                          (equal.reshape(-1, 9), dw.through_rays(64, 3)), (equal[:1].reshape(-1, 9), dw.through_rays(4, 3))):
            a, b = san(tri, rays), cert(tri, rays)
            assert all(np.array_equal(a[k], b[k]) for k in a)
            assert a["longest"] <= 3 * a["wdepth"] + 2

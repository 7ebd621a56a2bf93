"""The host specification of recompute_vertex_normals without a GPU: compute_vertex_normals (scene_build.cpp, built from
vertex_normals.h) through the export mtsamd_compute_vertex_normals and through tests/normals_driver.cpp, the stand-alone program that
vertex_normals_util.Driver compiles.

* the reference's own known answer, test_mesh.py::test04_normal_weighting_scheme, to its own tolerance;
* against loaders.compute_vertex_normals, float64 numpy, on the meshes of scenes.bumpy_sphere(8, 16) that carry normals, as built and
  after vm.jitter(SPHERE, 0.05);
* the edge meshes of vertex_normals_util.py: a unit vector or exactly (1, 0, 0), never a non-finite value;
* the device's order of work (a record per face, zeros for a skipped one, then a gather per vertex through the corner table) run on the
  host gives the bits of the sequential loop;
* the export refuses what it can; the library and the driver, compiled apart at different optimisation levels, agree to the bit;
* the driver built with -fsanitize=address,undefined runs the same inputs clean (a stand-alone program: nothing is preloaded)."""
import ctypes as C
import os

import numpy as np
import pytest

import vertex_moves as vm
import vertex_normals_util as vn
from mitsuba2_amd import loaders

F32 = np.float32
INVALID = -1          # MTSAMD_ERR_INVALID
# Largest absolute difference between the fp32 specification and float64 numpy over the sphere as built and jittered, measured here on
# the CPU: 6.332993507385254e-08 (about one unit in the last place of a component near 1; 5.960464477539063e-08 as built).  The bound is
# 4 x that, since the value depends on the jitter's seed.
MEASURED_MAX_DIFFERENCE = 6.332993507385254e-08
# The reference's own tolerance for this computation (test04_normal_weighting_scheme), for meshes with small angles: acos(dot) near
# dot = 1 turns an error e of the dot product into e / sin(angle) of the angle, in fp32 and in the reference alike.  The fan's apex
# angles are 2 pi / 300 = 0.021: three units in the last place of the dot product (1.8e-7) become 9e-6 per corner, at most 300 x that
# over the apex's sum, whose length is about 5: 5e-4.
REFERENCE_TOLERANCE = 5e-4


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(vm.HIPCC):
        pytest.skip("hipcc not installed")
    return vn.Driver(tmp_path_factory.mktemp("normals"))


def _sphere_meshes():
    """every mesh of the sphere scene that carries normals, as built and after the jitter"""
    sd = vm.sphere_scene()[0]
    out = {}
    for label, d in (("built", sd), ("jittered", vm.moved(sd, vm.jitter(vm.SPHERE, 0.05)))):
        for i, m in enumerate(d["meshes"]):
            if m.get("normals") is not None:
                out["%s%d" % (label, i)] = (np.asarray(m["positions"], F32).reshape(-1, 3), np.asarray(m["faces"], np.uint32).reshape(-1, 3))
    return out


def edge_meshes():
    sd = vm.sphere_scene()[0]
    _, collapsed, _ = vm.collapse(vm.SPHERE, 16, 64)(sd)
    return {
        "edge": vn.edge_mesh(), "strip257": vn.strip257(), "tiny_huge": vn.tiny_huge(), "overflowing": vn.overflowing(),
        "collapsed": (collapsed, np.asarray(sd["meshes"][vm.SPHERE]["faces"], np.uint32).reshape(-1, 3)),
    }


def _unit_or_bogus(n):
    """each row a unit vector (|len - 1| <= 1e-6) or exactly (1, 0, 0); returns the mask of the rows that are exactly (1, 0, 0)"""
    assert np.isfinite(n).all()
    bogus = (vn.bits(n).reshape(-1, 3) == vn.bits([1.0, 0.0, 0.0])).all(1)
    length = np.sqrt((n.astype(np.float64) ** 2).sum(1))
    assert (np.abs(length - 1.0) <= 1e-6).all(), float(np.abs(length - 1.0).max())
    return bogus


def test_reference_known_answer():
    """test_mesh.py::test04_normal_weighting_scheme: 5 vertices, faces [0, 1, 2] and [0, 3, 4]; ek.allclose(normals, closed form, 5e-4),
    i.e. |a - b| <= |b| * 5e-4 + 1e-8"""
    a, b = 1.0, 0.5
    pos = np.array([0, 0, 0, -a, 1, 0, a, 1, 0, -b, 0, 1, b, 0, 1], F32).reshape(-1, 3)
    faces = np.array([[0, 1, 2], [0, 3, 4]], np.uint32)
    n0, n1 = np.array([0.0, 0.0, -1.0]), np.array([0.0, 1.0, 0.0])
    n2 = n0 * (np.pi / 2.0) + n1 * np.arccos(3.0 / 5.0)
    n2 /= np.linalg.norm(n2)
    want = np.stack([n2, n0, n0, n1, n1])
    got = vn.spec(pos, faces)
    assert (np.abs(got - want) <= np.abs(want) * 5e-4 + 1e-8).all(), (got, want)


def test_host_spec_against_float64_numpy():
    """Largest absolute difference measured here on the CPU: 6.332993507385254e-08 (MEASURED_MAX_DIFFERENCE); allowed: 4 x that."""
    meshes = _sphere_meshes()
    assert sorted(meshes) == ["built0", "jittered0"]          # the sphere is the mesh with normals
    worst = 0.0
    for label, (pos, faces) in meshes.items():
        got, want = vn.spec(pos, faces), loaders.compute_vertex_normals(pos, faces)
        d = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        print("%s: %d vertices, largest |fp32 spec - float64 numpy| = %r" % (label, len(pos), d))
        worst = max(worst, d)
    print("largest absolute difference: %r" % worst)
    assert worst <= 4.0 * MEASURED_MAX_DIFFERENCE, worst


def test_edge_cases():
    """each output is a unit vector or exactly (1, 0, 0), and never non-finite"""
    got = {k: vn.spec(*m) for k, m in edge_meshes().items()}
    bogus = {k: _unit_or_bogus(n) for k, n in got.items()}
    e = bogus["edge"]
    assert e[vn.EDGE_ISOLATED] and e[vn.EDGE_CANCELLING].all()            # no face; two faces whose sum is exactly zero
    assert not e[:vn.FAN_FACES + 1].any()                                  # the fan: apex and rim
    apex = got["edge"][vn.EDGE_APEX].astype(np.float64)
    want = loaders.compute_vertex_normals(*vn.fan())[0].astype(np.float64)
    assert apex[1] > 0.9 and np.abs(apex - want).max() <= REFERENCE_TOLERANCE         # 300 incident faces, summed in face order
    assert not bogus["strip257"].any()
    assert np.abs(got["strip257"].astype(np.float64) - loaders.compute_vertex_normals(*vn.strip257())).max() <= REFERENCE_TOLERANCE
    assert bogus["tiny_huge"].all() and bogus["overflowing"].all()        # the only face of these vertices is skipped
    # vm.collapse: vertices 16 .. 79 of the sphere coincide.  Those whose every face lies among them have zero-area faces only
    pos, faces = edge_meshes()["collapsed"]
    inside = (faces >= 16) & (faces < 80)
    only_degenerate = np.ones(len(pos), bool)
    only_degenerate[np.unique(faces[inside.sum(1) < 2])] = False          # a face with two collapsed corners is degenerate too
    assert only_degenerate[16:80].any() and bogus["collapsed"][only_degenerate].all()
    # rings of 16: the pole ring 0 .. 15 is one point, whose faces reach into the collapsed ring 16 .. 31; ring 64 .. 79 is collapsed too
    # but keeps its faces towards ring 80 .. 95
    assert np.array_equal(np.nonzero(bogus["collapsed"])[0], np.arange(64))


def test_the_gather_reproduces_the_sequential_sum(driver):
    """normals_driver.cpp: `gathered` is the device's order of work on the host.  A skipped face's zero record adds +0 to a sum that is
    never -0, so the bits are those of the loop that skips it; the driver (-O1) and the library (-O3) agree too."""
    meshes = dict(edge_meshes(), **_sphere_meshes())
    out = driver.run(meshes)
    for label, (pos, faces) in meshes.items():
        assert np.array_equal(vn.bits(out[label + ".normals"]), vn.bits(out[label + ".gathered"])), label
        assert np.array_equal(vn.bits(out[label + ".normals"]), vn.bits(vn.spec(pos, faces))), label
    assert out["tiny_huge.skipped"] == 1 and out["overflowing.skipped"] == 1 and out["edge.skipped"] == 0 and out["strip257.skipped"] == 0
    assert out["collapsed.skipped"] > 0 and out["built0.skipped"] == 0


def test_the_export_needs_no_scene_and_refuses_bad_arrays():
    from mitsuba2_amd import _lib as L
    lib = L.lib()
    pos, faces = vn.cancelling()
    out = np.zeros_like(pos)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mtsamd_compute_vertex_normals(3, p(pos), 2, p(faces), p(out)) == 0
    assert np.array_equal(out, np.array([[1, 0, 0]] * 3, F32))
    assert lib.mtsamd_compute_vertex_normals(3, None, 2, p(faces), p(out)) == INVALID and lib.mtsamd_last_error() == b"null argument"
    assert lib.mtsamd_compute_vertex_normals(3, p(pos), 2, None, p(out)) == INVALID and lib.mtsamd_last_error() == b"null argument"
    bad = faces.copy(); bad[1, 2] = 3
    assert lib.mtsamd_compute_vertex_normals(3, p(pos), 2, p(bad), p(out)) == INVALID
    assert lib.mtsamd_last_error() == b"face 1: vertex index 3 out of range (3 vertices)"
    assert lib.mtsamd_compute_vertex_normals(0, None, 0, None, None) == 0
    # the flags of mtsamd_scene_update_vertices are looked at once there is a scene; without one the call is refused like the old one
    assert lib.mtsamd_scene_update_vertices(None, 0, p(pos), None, 1, None, None) == INVALID and lib.mtsamd_last_error() == b"null scene"


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path):
    if not os.path.exists(vm.HIPCC):
        pytest.skip("hipcc not installed")
    san = vn.Driver(tmp_path, flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    meshes = dict(edge_meshes(), **_sphere_meshes())
    out = san.run(meshes, "sanitized")
    for label, (pos, faces) in meshes.items():
        assert np.array_equal(vn.bits(out[label + ".normals"]), vn.bits(vn.spec(pos, faces))), label

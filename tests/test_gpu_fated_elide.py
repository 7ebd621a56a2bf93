"""Fated paths (mitsuba2_amd/csrc/fated.h): a path whose end at the next step is decided when its ray is spawned -- max_depth, or a
Russian roulette whose inputs are all known by then -- skips that step's ray query unless the ray can reach the padded box of an area
emitter, and the RGB shadow ring finishes a path that dies with its shadow ray pending instead of keeping it a launch as a zombie.  Neither
changes a sample: per-sample radiance is held bit for bit to the oracle's wavefront stream with the same seeds, in every schedule.

Counters.  The oracle reports (closest-hit rays, any-hit rays, samples).  An elided query is still counted, so closest_hit_rays and
segments must EQUAL the oracle's closest-hit count and samples its sample count.  any_hit_rays cannot equal the oracle's: the library has
never traced a shadow ray whose contribution is zero (test_gpu_parity.py holds it to <=); it must not exceed it and must be the same number
in every schedule.

Cases: the Cornell box 64 x 64 @ 32 spp with max_depth in {-1, 2, 3, 7} x rr_depth in {1, 5} through pipelines 0-4 (pipeline 0 is k_mega at
this size), a pass that ends in k_finish and one that drains by gathering; a light that covers the ceiling (the keep branch); a light of one
thin triangle (box reached, triangle missed); two area lights and a point light (general kernels); five area lights (over the cap: off);
an area light and a constant environment (off); the smallest bumpy_sphere that is not flat, RGB and spectral; the film render, autodiff.render
and the raw stream (the three store_xyz modes of store_result, which the ring's drain now calls); a vertex update that moves the light,
flat and hierarchy, against a fresh scene.  With max_depth = 2 nearly every path dies with a shadow ray pending: the test of the ring."""
import copy

import numpy as np
import pytest
import torch

from mitsuba2_amd import scenes

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H, SPP = 64, 64, 32
LIGHT = 5                                    # mesh index of the Cornell box's luminaire

# (pipeline, finish_kernel): 0 automatic (k_mega for a pass this small), 1 fused k_bounce, 2 split k_trace / k_shade, 3 queued shadow rays,
# 4 shadow ring; finish_kernel 2: k_finish as soon as the cursors are dry, 1: never (the rounds gather the pool and run it dry)
SCHEDULES = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (4, 2), (4, 1)]
_ORACLE = {}


def _quad_mesh(corners, bsdf, emitter, towards):
    p, f = scenes._quad(corners)
    return dict(positions=p, faces=scenes._orient(p, f, towards=towards), normals=None, texcoords=None, bsdf=bsdf, emitter=emitter)


def _cbox(kind):
    sd = scenes.cornell_box()
    centre = [278.0, 274.4, 279.6]
    rad = sd["emitters"][0]["radiance"]
    if kind == "ceiling_light":
        sd["meshes"][LIGHT] = _quad_mesh([[556, 548.3, 0], [556, 548.3, 559.2], [0, 548.3, 559.2], [0, 548.3, 0]], 3, 0, centre)
        sd["emitters"][0]["radiance"] = (rad * F32(0.05)).astype(F32)
    elif kind == "sliver_light":             # its box is the luminaire's rectangle, its area a hundredth of it
        p = np.array([[213, 548.3, 227], [343, 548.3, 332], [345, 548.3, 330]], F32)
        f = scenes._orient(p, np.array([[0, 1, 2]], np.uint32), towards=centre)
        sd["meshes"][LIGHT] = dict(positions=p, faces=f, normals=None, texcoords=None, bsdf=3, emitter=0)
        sd["emitters"][0]["radiance"] = (rad * F32(50.0)).astype(F32)
    elif kind in ("two_lights_and_point", "five_lights"):
        spots = [(60, 60), (420, 60), (60, 430), (420, 430)][:1 if kind == "two_lights_and_point" else 4]
        for k, (x, z) in enumerate(spots):
            sd["meshes"].append(_quad_mesh([[x + 70, 548.3, z], [x + 70, 548.3, z + 70], [x, 548.3, z + 70], [x, 548.3, z]], 3, 1 + k, centre))
            sd["emitters"].append(dict(type="area", radiance=(rad * F32(0.5 + 0.25 * k)).astype(F32)))
        if kind == "two_lights_and_point":
            sd["emitters"].append(dict(type="point", position=np.array([278, 300, 150], F32), intensity=np.array([2e5, 1.5e5, 1e5], F32)))
    elif kind == "environment":
        sd["emitters"].append(dict(type="constant", radiance=np.array([0.3, 0.4, 0.5], F32)))
    else:
        assert kind == "cornell"
    return sd


def _reference(oracle, gpu, key, sd, p, variant="rgb"):
    """per-sample stream, positions and counters of the oracle's wavefront mode: computed once per case, never modified"""
    k = (key, p["width"], p["height"], p["sample_count"], p["seed"], p["max_depth"], p["rr_depth"], variant)
    if k not in _ORACLE:
        S = oracle.OracleScene(sd, naive=True, spectral_path=gpu.srgb_coeff_path() if variant == "spectral" else None)
        desc = oracle.make_desc(p)
        n = p["width"] * p["height"] * p["sample_count"]
        ref, pos = S.sample_radiance(desc, 0, n)
        film, stats = S.render(desc, mode=1)
        for a in (ref, pos, film):
            a.setflags(write=False)
        _ORACLE[k] = (ref, pos, film, [int(x) for x in stats])
    return _ORACLE[k]


def _check(gpu, oracle, key, sd, p, schedules, variant="rgb"):
    ref, ref_pos, ref_film, (o_closest, o_any, o_samples) = _reference(oracle, gpu, key, sd, p, variant)
    n = len(ref)
    assert (ref[:, :3] > 0).any(1).mean() > 0.25, "the case is lit"
    scene, sensor = gpu.Scene(sd, variant=variant), gpu.make_sensor(p)
    any_hit, films, iters = set(), [], {}
    for pipeline, fk in schedules:
        integ = gpu.PathIntegrator(max_depth=p["max_depth"], rr_depth=p["rr_depth"], pipeline=pipeline)
        integ.finish_kernel = fk
        rgb, mask, pos = integ.sample(scene, sensor, 0, n)
        rgb = rgb.cpu().numpy()
        exact = (rgb == ref[:, :3]).all(1)
        assert exact.all(), (key, pipeline, fk, int((~exact).sum()), np.nonzero(~exact)[0][:8], rgb[~exact][:4], ref[~exact][:4, :3])
        assert (pos.cpu().numpy() == ref_pos).all() and (mask.cpu().numpy() == (ref[:, 3] > 0.5)).all(), (key, pipeline, fk)
        assert integ.render(scene, sensor)
        st = integ.stats
        print("%s depth %d rr %d %s pipeline %d/%d: closest %d (oracle %d) any %d (oracle %d) segments %d samples %d iterations %d" %
              (key, p["max_depth"], p["rr_depth"], variant, pipeline, fk, st["closest_hit_rays"], o_closest, st["any_hit_rays"], o_any, st["segments"],
               st["samples"], st["iterations"]))
        assert st["samples"] == o_samples == n and st["closest_hit_rays"] == o_closest and st["segments"] == o_closest, (key, pipeline, fk, st)
        assert st["any_hit_rays"] <= o_any
        any_hit.add(st["any_hit_rays"])
        films.append(sensor.film().bitmap(raw=True).clone())
        iters[(pipeline, fk)] = st["iterations"]
    assert len(any_hit) == 1, (key, any_hit)
    for f in films[1:]:
        assert torch.equal(f, films[0]), key                     # store_xyz = 1 through every schedule's way of ending a path
    if variant == "rgb":                                          # test_gpu_parity.py's bounds: the order of a pixel's splats is all that differs
        film = films[0].cpu().numpy()
        assert np.allclose(film[..., 3:], ref_film[..., 3:], rtol=1e-5, atol=1e-5)
        assert np.allclose(film[..., :3], ref_film[..., :3], rtol=2e-5, atol=1e-6)
    return iters


@pytest.mark.parametrize("rr_depth", [1, 5])
@pytest.mark.parametrize("max_depth", [-1, 2, 3, 7])
def test_cornell_box_every_schedule(gpu, oracle, max_depth, rr_depth):
    p = scenes.cornell_box_sensor(W, H, SPP, seed=7, max_depth=max_depth, rr_depth=rr_depth)
    iters = _check(gpu, oracle, "cornell", _cbox("cornell"), p, SCHEDULES)
    if max_depth in (-1, 7):                                      # (a path of two or three segments leaves little to drain)
        assert iters[(4, 1)] > iters[(4, 2)], iters              # the rounds really drained the pool where k_finish would have taken over


@pytest.mark.parametrize("kind", ["ceiling_light", "sliver_light", "two_lights_and_point", "five_lights", "environment"])
@pytest.mark.parametrize("max_depth", [-1, 3])
def test_other_lights(gpu, oracle, kind, max_depth):
    p = scenes.cornell_box_sensor(W, H, SPP, seed=11, max_depth=max_depth, rr_depth=2)
    _check(gpu, oracle, kind, _cbox(kind), p, [(0, 0), (1, 0), (3, 0), (4, 0), (4, 1)])


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
@pytest.mark.parametrize("max_depth", [-1, 3])
def test_hierarchy_scene(gpu, oracle, variant, max_depth):
    sd = scenes.bumpy_sphere(6, 8)
    assert sum(len(m["faces"]) for m in sd["meshes"]) > 64       # not LDS-resident; (5, 8) and (6, 6) are
    p = scenes.bumpy_sphere_sensor(48, 32, 16, seed=3, max_depth=max_depth, rr_depth=2)
    _check(gpu, oracle, "bumpy", sd, p, [(0, 0), (1, 0), (2, 0)], variant)


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
def test_flat_spectral_and_rgb_rings(gpu, oracle, variant):
    """the spectral ring keeps its zombies and loses only speed; max_depth 2: nearly every path dies with a shadow ray pending"""
    p = scenes.cornell_box_sensor(W, H, SPP, seed=5, max_depth=2, rr_depth=5)
    _check(gpu, oracle, "cornell", _cbox("cornell"), p, [(1, 0), (3, 0), (4, 0), (4, 1)], variant)


@pytest.mark.parametrize("max_depth", [2, -1])
def test_autodiff_render_through_the_ring(gpu, max_depth):
    """store_xyz = 2 (the linear RGB film of autodiff.render): the ring schedule against the fused kernel, which has no ring"""
    from mitsuba2_amd import autodiff
    p = scenes.cornell_box_sensor(W, H, SPP, seed=9, max_depth=max_depth, rr_depth=2)
    images = []
    for pipeline in (1, 4):
        scene = gpu.Scene(_cbox("cornell"), sensor=gpu.make_sensor(p), integrator=gpu.PathIntegrator(max_depth=max_depth, rr_depth=2, pipeline=pipeline))
        images.append(autodiff.render(scene).clone())            # the first call of a scene: the sampler's own seed
    assert torch.equal(images[0], images[1])
    assert torch.isfinite(images[0]).all() and images[0].max() > 0


def test_the_device_really_elides_and_the_ring_really_finishes(gpu):
    """Results and counters are designed not to show the elision, so these two figures do.
    Hierarchy scenes: tri_tests is real work (the triangles k_trace tests), and an elided path never reaches k_trace.  The parent
    commit's figures for these two renders, recorded on an MI355X with a -DMTS_FATED_ELIDE=0 library (the tree and the paths are
    deterministic), are 123838 and 126757; with the elision 114928 and 120163.  A kernel that reads an empty list gives the parent's.
    Ring: with rr_depth 1 the pool drains slowly and the number of launch rounds is set by the last paths to end.  The queued
    pipeline (3) keeps a path that dies with a shadow ray pending one more round as a zombie, the ring (4) finishes it in the round it
    dies in: fewer rounds (25 against 29 when recorded; the parent needs 29 in both)."""
    def stats(sd, p, pipeline, fk):
        integ = gpu.PathIntegrator(max_depth=p["max_depth"], rr_depth=p["rr_depth"], pipeline=pipeline)
        integ.finish_kernel = fk
        assert integ.render(gpu.Scene(sd), gpu.make_sensor(p))
        return integ.stats
    for max_depth, parent in ((3, 123838), (-1, 126757)):
        st = stats(scenes.bumpy_sphere(6, 8), scenes.bumpy_sphere_sensor(48, 32, 16, seed=3, max_depth=max_depth, rr_depth=2), 2, 0)
        print("hierarchy max_depth %d: tri_tests %d (parent %d)" % (max_depth, st["tri_tests"], parent))
        assert 0 < st["tri_tests"] < parent
    p = scenes.cornell_box_sensor(W, H, SPP, seed=7, max_depth=-1, rr_depth=1)
    queued, ring = stats(_cbox("cornell"), p, 3, 1)["iterations"], stats(_cbox("cornell"), p, 4, 1)["iterations"]
    print("rounds: queued shadow rays %d, shadow ring %d" % (queued, ring))
    assert ring < queued


@pytest.mark.parametrize("which", ["flat", "hierarchy"])
def test_vertex_update_moves_the_light(gpu, which):
    """the light leaves its box: boxes kept from creation would end fated paths that now reach it"""
    if which == "flat":
        sd, light, shift = _cbox("cornell"), LIGHT, [-180.0, -150.0, 160.0]
        p = scenes.cornell_box_sensor(W, H, 16, seed=21, max_depth=3, rr_depth=2)
    else:
        sd, light, shift = scenes.bumpy_sphere(6, 8), 2, [2.5, -1.0, -2.0]
        p = scenes.bumpy_sphere_sensor(48, 32, 16, seed=21, max_depth=3, rr_depth=2)
    new = copy.deepcopy(sd)
    new["meshes"][light]["positions"] = (np.asarray(sd["meshes"][light]["positions"], np.float64) + shift).astype(F32)

    def films(g):
        out = []
        for pipeline in (1, 4) if which == "flat" else (1, 2):
            sensor = gpu.make_sensor(p)
            assert gpu.PathIntegrator(max_depth=3, rr_depth=2, pipeline=pipeline).render(g, sensor)
            out.append(sensor.film().bitmap(raw=True).clone())
        assert torch.equal(out[0], out[1])
        return out[0]

    live = gpu.Scene(copy.deepcopy(sd))
    before = films(live)
    live.update_vertices(light, new["meshes"][light]["positions"])
    after, fresh = films(live), films(gpu.Scene(new))
    assert torch.equal(after, fresh)
    assert not torch.equal(after, before) and after[..., :3].max() > 0

"""The cluster cull of the flat-scene ray queries (flat_cull.h: centre / half-extent boxes, host-built pair masks, v_rcp_f32) only culls:
every answer stays what the brute force gives, bit for bit.

  queries   k_ray_intersect / k_ray_test on the rays of test_flat_cull_cpu.py (the families of stress_rays.py plus interior rays, direction
            components of 0, -0 and denormals, finite maxt, origins 100 extents away) against the oracle's brute force
            (ray_intersect_naive): the Cornell box, the box scaled by 1e-3 and 1e3 and moved 1e3 of its size off the origin, and soups of
            one cluster (no cull at all), two clusters, and 64 triangles in eight shapes.  Left out, whatever the cull: the rays for which
            some triangle's det is a nonzero subnormal -- rcp_nr2 starts from v_rcp_f32, which reads it as zero and rejects the triangle,
            while the oracle divides by it; the pair test is specified for normal-range det (the host test covers the flushed reciprocal)
  radiance  per-sample radiance of the Cornell box at 32 x 32 @ 16 spp in every pipeline (0-4), RGB and spectral, against the oracle's
            wavefront stream with the same seeds (camera-ray waves take the clustered loops, all other queries the work lists)
  update    a flat scene after update_vertices (the records are rebuilt by creation's code) against a freshly created scene"""
import copy

import numpy as np
import pytest
import torch

from mitsuba2_amd import scenes
from stress_rays import stress_rays, tris
from test_flat_cull_cpu import all_rays, moved, soup

pytestmark = pytest.mark.gpu

SIZE = 559.2
QUERY_SCENES = {
    "cornell": lambda: scenes.cornell_box(),
    "cornell_1e-3": lambda: moved(scenes.cornell_box(), 1e-3),
    "cornell_1e3": lambda: moved(scenes.cornell_box(), 1e3),
    "cornell_far": lambda: moved(scenes.cornell_box(), 1.0, 1e3 * SIZE),
    "one_cluster": lambda: soup(5, 1, 27),
    "two_clusters": lambda: soup(3, 2, 26),
    "eight_shapes": lambda: soup(64, 8, 28),
}
CLUSTERS = {"cornell": 8, "cornell_1e-3": 8, "cornell_1e3": 8, "cornell_far": 8, "one_cluster": 1, "two_clusters": 2, "eight_shapes": 7}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _gpu_ray(gpu, o, d, mint, maxt):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return gpu.Ray3f(o=t(o), d=t(d), mint=t(mint), maxt=t(maxt))


def _subnormal_det(sd, o, d):
    """rays for which det = dot(e1, cross(d, e2)) of some triangle, in the pair test's operations (fma emulated in float64, with a
    margin of two binades for its double rounding), is neither zero nor of normal range"""
    f32, f64 = np.float32, np.float64
    fma = lambda a, b, c: (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)
    tri = tris(sd)
    e1, e2 = (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]                 # [1, n_tris, 3]
    dx, dy, dz = (d[:, None, k] for k in range(3))
    with np.errstate(under="ignore"):
        pvx = fma(dy, e2[..., 2], -(dz * e2[..., 1]))
        pvy = fma(dz, e2[..., 0], -(dx * e2[..., 2]))
        pvz = fma(dx, e2[..., 1], -(dy * e2[..., 0]))
        det = np.abs(fma(e1[..., 2], pvz, fma(e1[..., 1], pvy, e1[..., 0] * pvx)))
    return ((det > 0) & (det < 4 * np.finfo(f32).tiny)).any(1)


def _clusters(sd):
    prim_shape = [s for s, m in enumerate(sd["meshes"]) for _ in range(len(m["faces"]))]
    return sum(1 for k in range((len(prim_shape) + 1) // 2) if k == 0 or prim_shape[2 * k] != prim_shape[2 * (k - 1)])


@pytest.mark.parametrize("name", list(QUERY_SCENES))
def test_queries_equal_the_brute_force(gpu, oracle, name):
    sd = QUERY_SCENES[name]()
    assert _clusters(sd) == CLUSTERS[name]
    rays, _ = all_rays(sd, 5 + list(QUERY_SCENES).index(name))
    skip = _subnormal_det(sd, rays[:, 0:3], rays[:, 3:6])
    tiny_d = ((np.abs(rays[:, 3:6]) < np.finfo(np.float32).tiny) & (rays[:, 3:6] != 0)).any(1)
    print("%s: %d rays with a subnormal det left out; %d rays with a denormal direction component kept" % (name, skip.sum(), (tiny_d & ~skip).sum()))
    # det of a triangle whose normal lies along the denormal component is (component x twice its area): subnormal unless the area is large.
    # On the box scaled by 1e-3 (walls of area 0.3) that takes every such ray out; the other scenes keep thousands (of 6000 drawn)
    assert name == "cornell_1e-3" or (tiny_d & ~skip).sum() > 1000
    rays = rays[~skip]
    n = (len(rays) // 64) * 64 - 27                        # the last wave is partial
    o, d, mint, maxt = (np.ascontiguousarray(a) for a in (rays[:n, 0:3], rays[:n, 3:6], rays[:n, 6], rays[:n, 7]))
    S = oracle.OracleScene(sd)
    t_o, prim_o, _, u_o, v_o = S.ray_intersect(o, d, mint, maxt, naive=True)
    hit_o = S.ray_test(o, d, mint, maxt, naive=True)
    print("%s: %d rays, %d hit, %d occluded" % (name, n, np.isfinite(t_o).sum(), hit_o.sum()))
    assert np.isfinite(t_o).sum() > n // 4
    scene = gpu.Scene(sd)
    assert scene.info()["primitives"] == sum(len(m["faces"]) for m in sd["meshes"]) <= 64      # LDS-resident (test_flat_cull_cpu.py: the builder says flat)
    ray = _gpu_ray(gpu, o, d, mint, maxt)
    res = scene.ray_intersect(ray, full=False)
    t_g, prim_g, uv_g = res.t.cpu().numpy(), res.prim_index.cpu().numpy().astype(np.uint32), res.prim_uv.cpu().numpy()
    found = np.isfinite(t_o)
    mism = (_bits(t_g) != _bits(t_o)) | (prim_g != prim_o.astype(np.uint32)) | (found & ((_bits(uv_g[:, 0]) != _bits(u_o)) | (_bits(uv_g[:, 1]) != _bits(v_o))))
    assert mism.sum() == 0, "mismatches: %d of %d: %s" % (mism.sum(), n, [(int(i), o[i].tolist(), d[i].tolist(), float(mint[i]), float(maxt[i]), float(t_g[i]), int(prim_g[i]), float(t_o[i]), int(prim_o[i])) for i in np.nonzero(mism)[0][:6]])
    hit_g = scene.ray_test(ray).cpu().numpy()
    bad = np.nonzero(hit_g != hit_o)[0]
    assert bad.size == 0, "ray_test mismatches: %d: %s" % (bad.size, [(int(i), o[i].tolist(), d[i].tolist(), float(mint[i]), float(maxt[i]), bool(hit_g[i])) for i in bad[:6]])


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
def test_per_sample_radiance(gpu, oracle, variant):
    sd = scenes.cornell_box()
    p = scenes.cornell_box_sensor(32, 32, 16, seed=3)
    n = 32 * 32 * 16
    S = oracle.OracleScene(sd, naive=True, spectral_path=gpu.srgb_coeff_path() if variant == "spectral" else None)
    ref, ref_pos = S.sample_radiance(oracle.make_desc(p), 0, n)
    assert (ref[:, :3] > 0).any(1).mean() > 0.5                   # most samples carry light
    g, sensor = gpu.Scene(sd, variant=variant), gpu.make_sensor(p)
    for pipeline in (0, 1, 2, 3, 4):
        rgb, mask, pos = gpu.PathIntegrator(max_depth=-1, rr_depth=5, pipeline=pipeline).sample(g, sensor, 0, n)
        rgb = rgb.cpu().numpy()
        exact = (rgb == ref[:, :3]).all(1)
        assert exact.all(), (pipeline, int((~exact).sum()), np.nonzero(~exact)[0][:8], rgb[~exact][:4], ref[~exact][:4, :3])
        assert (pos.cpu().numpy() == ref_pos).all() and (mask.cpu().numpy() == (ref[:, 3] > 0.5)).all(), pipeline


def test_update_vertices_rebuilds_the_cluster_records(gpu):
    """the short box leaves its cluster box (lifted, shifted and stretched) and the light moves: records kept from creation would cull hits"""
    sd = scenes.cornell_box()
    short, light = 6, 5
    new = copy.deepcopy(sd)
    new["meshes"][short]["positions"] = (np.asarray(sd["meshes"][short]["positions"], np.float64) * [1.0, 1.8, 1.0] + [150.0, 120.0, 180.0]).astype(np.float32)
    new["meshes"][light]["positions"] = (np.asarray(sd["meshes"][light]["positions"], np.float64) + [-60.0, -40.0, 35.0]).astype(np.float32)
    o, d, mint, maxt = stress_rays(new, 12)
    ray = _gpu_ray(gpu, o, d, mint, maxt)
    p = scenes.cornell_box_sensor(32, 32, 4, seed=21)

    def answers(g):
        res = g.ray_intersect(ray, full=False)
        sensor = gpu.make_sensor(p)
        assert gpu.PathIntegrator().render(g, sensor)
        return res.t.clone(), res.prim_index.clone(), res.prim_uv.clone(), g.ray_test(ray).clone(), sensor.film().bitmap(raw=True).clone()

    live = gpu.Scene(copy.deepcopy(sd))
    before = answers(live)
    for shape in (short, light):
        live.update_vertices(shape, new["meshes"][shape]["positions"])
    after, fresh = answers(live), answers(gpu.Scene(new))
    for a, f in zip(after, fresh):
        assert torch.equal(a, f)
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[4], before[4])

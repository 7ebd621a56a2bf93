"""Walks that leave the LDS part of the traversal stack: ray queries and render schedules on the scenes of tests/deep_walk.py.

k_ray_walk, k_trace and k_finish / k_mega keep 8 stack entries per lane in LDS and the rest in a global spill area; the scenes the other
tests use never certifiably go beyond 3 entries (tests/test_deep_walk_cpu.py), so a wrong spill stride, a wrong workgroup offset, a
slice spoilt between the chunks of a persistent workgroup or a slip at the hand-over row sp == 8 would pass them all.  Here 84 .. 97 %
of the rays need at least 12 entries whatever the order of their walk (at least 9 in the long stream), and the nearest-first order the
kernels use takes them to 16 .. 22 of a bound of 20 .. 29: the same walks also drive the kernels that keep the whole stack in LDS
(k_ray_intersect with the SurfaceInteraction fill, k_bounce, k_direct) near its end.
Not caught, here or elsewhere: an area sized one row short, or a row index shifted by one in push and pop alike.  Both show only in the
last row of a slice.  The bound 3 * wdepth + 2 carries two entries that no walk can take (a walk defers at most 3 * wdepth subtrees),
so the last two rows are out of reach of any ray; of the 10 / 16 / 19 reachable rows these walks use the first 8 / 10 / 14 (long
stream / slivers(4096) / render scene).
Which test covers what:
  walk_spill of k_ray_walk<false / true>: test_deep_walks_every_query, test_launch_edges_of_the_ray_fetch, test_stream_longer_than_the_persistent_grid
  trace_spill, k_trace slices (closest-hit and any-hit): test_per_sample_radiance pipeline 2, test_finish_kernel_on_deep_walks
  trace_spill, 64-lane slices of k_finish and k_mega: test_finish_kernel_on_deep_walks, test_per_sample_radiance pipeline 0
Every comparison is exact: the reference is the oracle's brute force, which knows nothing of the hierarchy."""
import numpy as np
import pytest
import torch

import deep_walk as dw
from test_gpu_lifecycle import _film, _knobs

pytestmark = pytest.mark.gpu


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def _gpu_ray(render, rays, sel=slice(None)):
    o, d, mint, maxt = (torch.from_numpy(np.ascontiguousarray(a[sel])).cuda() for a in rays)
    return render.Ray3f(o=o, d=d, mint=mint, maxt=maxt)


@pytest.fixture(scope="module")
def deep(gpu, oracle):
    """slivers(4096), its ray set and the oracle's brute-force answers, computed once"""
    sd = dw.slivers(dw.QUERY_K)
    rays = dw.query_rays()
    S = oracle.OracleScene(sd)
    ref = _frozen(*S.ray_intersect(*rays, naive=True))
    hit, = _frozen(S.ray_test(*rays, naive=True))
    assert np.isfinite(ref[0][dw.QUERY_THROUGH:]).sum() >= dw.QUERY_AIMED // 2        # real hits among the aimed rays
    order, = _frozen(np.random.RandomState(5).permutation(len(hit)))                   # both kinds of ray in every prefix
    return dict(sd=sd, scene=gpu.Scene(sd), S=S, rays=rays, ref=ref, hit=hit, order=order)


def _same_hits(res, ref, what):
    t, prim, shape, u, v = ref
    assert (res.t.cpu().numpy() == t).all(), what
    assert (res.prim_index.cpu().numpy().astype(np.uint32) == prim).all(), what
    assert (res.shape_index.cpu().numpy().astype(np.uint32) == shape).all(), what
    if res.prim_uv is not None:
        assert (res.prim_uv.cpu().numpy() == np.stack([u, v], 1)).all(), what


def test_deep_walks_every_query(gpu, deep):
    scene, rays, ref, hit = deep["scene"], deep["rays"], deep["ref"], deep["hit"]
    info = scene.info()
    assert info["primitives"] == dw.QUERY_K and info["bvh_nodes"] > 0                  # a hierarchy scene
    ray = _gpu_ray(gpu, rays)
    _same_hits(scene.ray_intersect(ray, full=False), ref, "k_ray_walk<false>")
    got = scene.ray_test(ray).cpu().numpy()
    assert (got == hit).all() and (got == np.isfinite(ref[0])).all(), "k_ray_walk<true>"
    _same_hits(scene.ray_intersect_naive(ray), ref, "brute force")
    si = scene.ray_intersect(ray)                                                       # whole stack in LDS, SurfaceInteraction fill
    assert (si.t.cpu().numpy() == ref[0]).all() and (si.prim_index.cpu().numpy().astype(np.uint32) == ref[1]).all()
    assert (si.shape_index.cpu().numpy().astype(np.uint32) == ref[2]).all()
    valid = np.isfinite(ref[0])
    want = deep["S"].fill_si(rays[1], ref[1], ref[3], ref[4])
    fields = np.concatenate([x.cpu().numpy() for x in (si.p, si.n, si.uv, si.sh_frame_s, si.sh_frame_t, si.sh_frame_n, si.dp_du, si.dp_dv, si.wi)], axis=1)
    assert (fields[valid] == want[valid]).all()
    assert (si.wi.cpu().numpy()[~valid] == -rays[1][~valid]).all()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, dw.RAY_CHUNK - 1, dw.RAY_CHUNK, dw.RAY_CHUNK + 1, 2 * dw.RAY_CHUNK + 1])
def test_launch_edges_of_the_ray_fetch(gpu, deep, n, masked):
    """stream lengths round the wave and the chunk of the dynamic ray fetch, with and without every third ray masked off"""
    scene, sel = deep["scene"], deep["order"][:n]
    ray = _gpu_ray(gpu, deep["rays"], sel)
    ref = tuple(a[sel] for a in deep["ref"])
    plain = scene.ray_intersect(ray, full=False)
    plain_hit = scene.ray_test(ray)
    _same_hits(plain, ref, n)
    assert (plain_hit.cpu().numpy() == deep["hit"][sel]).all()
    if not masked:
        return
    on = np.arange(n) % 3 != 0
    active = torch.from_numpy(on).cuda()
    res, res_hit = scene.ray_intersect(ray, active=active, full=False), scene.ray_test(ray, active=active)
    t, prim, shape, uv = (x.cpu().numpy() for x in (res.t, res.prim_index, res.shape_index, res.prim_uv))
    assert np.isposinf(t[~on]).all() and (prim[~on] == -1).all() and (shape[~on] == -1).all() and (uv[~on] == 0).all()
    assert not res_hit.cpu().numpy()[~on].any()
    # active rays: what the unmasked run gave (which is the oracle's answer)
    for a, b in ((res.t, plain.t), (res.prim_index, plain.prim_index), (res.shape_index, plain.shape_index), (res.prim_uv, plain.prim_uv),
                 (res_hit, plain_hit)):
        assert torch.equal(a[active], b[active])


@pytest.mark.parametrize("rounds", [1, 2])
def test_stream_longer_than_the_persistent_grid(gpu, oracle, rounds):
    """k_ray_walk runs 8 * CUs persistent workgroups; workgroup b takes the chunks b, b + 8 * CUs, ... of 4096 rays each.  A stream of
    rounds * 8 * CUs whole chunks, one more whole chunk and one ray: with rounds = 1 only workgroups 0 and 1 come back for a second
    chunk (the second one of a single ray); with rounds = 2 every workgroup takes a second chunk on the spill slice it has just used,
    workgroup 0 a third and workgroup 1 the one-ray chunk.  The whole stream is compared with the device's brute-force kernel, every
    997th ray with the oracle."""
    sd = dw.slivers(dw.STREAM_K)
    scene, S = gpu.Scene(sd), oracle.OracleScene(sd)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = rounds * 8 * cus * dw.RAY_CHUNK + dw.RAY_CHUNK + 1
    print("%d CUs: %d persistent workgroups, a stream of %d rays = %d chunks" % (cus, 8 * cus, n, -(-n // dw.RAY_CHUNK)))
    need = 192 * n              # bytes: rays (32 B each) and their transposed copy, two sets of hit records, the comparisons' temporaries
    free = torch.cuda.mem_get_info()[0]
    assert free >= need, "a stream of %d rays needs %d MiB of device memory, %d MiB are free" % (n, need >> 20, free >> 20)
    idx = dw.stream_index(n)
    tile = dw.stream_tile()
    gidx = torch.from_numpy(idx).cuda()
    o, d, mint, maxt = (torch.from_numpy(a).cuda()[gidx] for a in tile)
    ray = gpu.Ray3f(o=o, d=d, mint=mint, maxt=maxt)
    fast, slow = scene.ray_intersect(ray, full=False), scene.ray_intersect_naive(ray)
    assert torch.equal(fast.t, slow.t) and torch.equal(fast.prim_index, slow.prim_index)
    assert torch.equal(fast.shape_index, slow.shape_index) and torch.equal(fast.prim_uv, slow.prim_uv)
    assert torch.equal(scene.ray_test(ray), torch.isfinite(slow.t))
    some = np.arange(0, n, 997)
    ref = S.ray_intersect(*(a[idx[some]] for a in tile), naive=True)
    gsome = torch.from_numpy(some).cuda()
    assert (fast.t[gsome].cpu().numpy() == ref[0]).all() and (fast.prim_index[gsome].cpu().numpy().astype(np.uint32) == ref[1]).all()
    assert (fast.prim_uv[gsome].cpu().numpy() == np.stack([ref[3], ref[4]], 1)).all()
    assert np.isinf(ref[0]).mean() > 0.8                                                # the certified rays miss


# ---------------------------------------------------------------------------------------------------------------- render schedules
@pytest.fixture(scope="module")
def lit(gpu):
    sd, p = dw.deep_render_scene(), dw.deep_render_sensor()
    n = p["width"] * p["height"] * p["sample_count"]
    assert n <= 8192 and p["max_depth"] == 4
    return dict(sd=sd, p=p, n=n, sensor=gpu.make_sensor(p))


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
def test_per_sample_radiance(gpu, oracle, lit, variant):
    """primary rays through the cube, shadow rays back up through it to the lamp, bounce rays of the ground: every sample of every
    schedule a hierarchy scene has.  1: k_bounce (whole stack in LDS), 2: k_trace<closest> / k_shade / k_trace<any>, 0: a pass this
    small is one launch of k_mega; 4, the in-kernel shadow ring, exists for LDS-resident scenes only and must say so."""
    sd, p, n, sensor = lit["sd"], lit["p"], lit["n"], lit["sensor"]
    scene = gpu.Scene(sd, variant=variant)
    assert scene.info()["primitives"] == dw.RENDER_K + 4
    S = oracle.OracleScene(sd, naive=True, spectral_path=gpu.srgb_coeff_path() if variant == "spectral" else None)
    want, wpos = S.sample_radiance(oracle.make_desc(p), 0, n)
    assert (want[:, :3].max(1) > 0).mean() >= 0.02
    for pipeline in ((1, 2, 0) if variant == "rgb" else (1, 2)):
        rgb, mask, pos = gpu.PathIntegrator(max_depth=p["max_depth"], rr_depth=p["rr_depth"], pipeline=pipeline).sample(scene, sensor, 0, n)
        assert (pos.cpu().numpy() == wpos).all(), pipeline
        bad = (rgb.cpu().numpy() != want[:, :3]).any(1)
        assert not bad.any(), (variant, pipeline, int(bad.sum()), np.nonzero(bad)[0][:8])
        assert (mask.cpu().numpy() == (want[:, 3] > 0.5)).all(), pipeline
    with pytest.raises(RuntimeError, match="LDS-resident scenes only"):
        gpu.PathIntegrator(max_depth=p["max_depth"], pipeline=4).sample(scene, sensor, 0, n)


def test_finish_kernel_on_deep_walks(gpu, lit):
    """as test_finish_kernel_leaves_the_film_unchanged (tests/test_gpu_lifecycle.py), on walks that spill: the launch rounds of the split
    pipeline (k_trace slices of the spill area) against k_finish taking the pool as early as it may (64-lane slices of the same area)"""
    scene = gpu.Scene(lit["sd"])
    p = dw.deep_render_sensor(spp=8, max_depth=8)
    integ = gpu.PathIntegrator(max_depth=8, pipeline=2)
    with _knobs(integ, finish_kernel=1):
        never, st0 = _film(gpu, integ, scene, p)
    with _knobs(integ, finish_kernel=2):
        early, st1 = _film(gpu, integ, scene, p)
    assert st1["iterations"] < st0["iterations"]                 # the fused launch really replaced launch rounds
    for k in ("samples", "segments", "closest_hit_rays", "any_hit_rays"):
        assert st0[k] == st1[k], (k, st0[k], st1[k])
    assert st0["samples"] == 64 * 64 * 8 and float(never[..., :3].abs().max()) > 0
    assert torch.equal(never, early)


def test_direct_integrator_per_sample(gpu, oracle, lit):
    sd, p, n, sensor = lit["sd"], lit["p"], lit["n"], lit["sensor"]
    scene = gpu.Scene(sd)
    integ = gpu.DirectIntegrator()
    rgb, mask, pos = integ.sample(scene, sensor, 0, n)
    op = dict(p, integrator="direct", emitter_samples=integ.emitter_samples, bsdf_samples=integ.bsdf_samples, hide_emitters=integ.hide_emitters)
    want, wpos = oracle.OracleScene(sd, naive=True).sample_radiance(oracle.make_desc(op), 0, n)
    assert (want[:, :3].max(1) > 0).mean() >= 0.02
    assert (pos.cpu().numpy() == wpos).all() and (mask.cpu().numpy() == (want[:, 3] > 0.5)).all()
    bad = (rgb.cpu().numpy() != want[:, :3]).any(1)
    assert not bad.any(), (int(bad.sum()), np.nonzero(bad)[0][:8])

"""Flat-scene ray queries of incoherent rays (per-(ray, pair) work lists, traverse_flat_worklist) on hard rays: origins on surfaces,
grazing and axis-parallel directions, mint = 0 with hits at +-0, exact ties between two triangles, partially active waves.  Every
closest hit (t, primitive, u, v) and every any-hit answer must equal the oracle's brute force (ray_intersect_naive) and the GPU's own
brute force (traverse_naive)."""
import numpy as np
import pytest
import torch

from mitsuba2_amd import scenes

pytestmark = pytest.mark.gpu


def _tris(sd):
    p = []
    for m in sd["meshes"]:
        p.append(m["positions"][m["faces"].astype(np.int64)])
    return np.concatenate(p).astype(np.float32)          # [n_tris, 3 vertices, 3]


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _stress_rays(sd, seed):
    rng = np.random.RandomState(seed)
    tri = _tris(sd)
    allp = tri.reshape(-1, 3)
    lo, hi = allp.min(0), allp.max(0)
    groups = []
    # 1. origins on surfaces (random barycentrics), directions all over the sphere, the shading code's mint and mint = 0
    n = 6000
    k = rng.randint(0, len(tri), n)
    b = rng.rand(n, 2).astype(np.float32)
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    o = tri[k, 0] + b[:, :1] * (tri[k, 1] - tri[k, 0]) + b[:, 1:] * (tri[k, 2] - tri[k, 0])
    d = _unit(rng.randn(n, 3))
    mint = np.where(np.arange(n) % 2 == 0, 0.0, 1e-4 * (1 + np.abs(o).max(1))).astype(np.float32)
    groups.append((o, d, mint, np.full(n, np.inf, np.float32)))
    # 2. axis-parallel directions from inside the box and from vertices; grazing directions in (and just off) a triangle's plane
    n = 6000
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
    o = np.where(rng.rand(n, 1) < 0.5, lo + (hi - lo) * rng.rand(n, 3), allp[rng.randint(0, len(allp), n)]).astype(np.float32)
    d = axes[rng.randint(0, 6, n)]
    groups.append((o, d, np.zeros(n, np.float32), np.full(n, np.inf, np.float32)))
    k = rng.randint(0, len(tri), n)
    e1, e2 = tri[k, 1] - tri[k, 0], tri[k, 2] - tri[k, 0]
    nrm = _unit(np.cross(e1, e2))
    tang = _unit(np.cross(nrm, rng.randn(n, 3)))
    eps = np.array([0.0, 1e-7, -1e-7, 1e-4, -1e-3], np.float32)[rng.randint(0, 5, n)][:, None]
    d = _unit(tang + eps * nrm)
    o = (tri[k, 0] + 0.3 * e1 + 0.3 * e2 - 2.0 * np.abs(hi - lo).max() * d).astype(np.float32)
    groups.append((o, d, np.zeros(n, np.float32), np.full(n, np.inf, np.float32)))
    # 3. mint = 0 and hits at t = +-0: origins exactly at vertices and on edges (shared by two triangles: exact ties), both sides
    n = 6000
    k = rng.randint(0, len(tri), n)
    w = np.array([0.0, 0.5, 1.0], np.float32)[rng.randint(0, 3, n)][:, None]
    o = (tri[k, 0] + w * (tri[k, 1] - tri[k, 0])).astype(np.float32)
    d = _unit(rng.randn(n, 3))
    groups.append((o, d, np.zeros(n, np.float32), np.full(n, np.inf, np.float32)))
    # 4. exact ties: rays aimed at the midpoint of an edge (the diagonal of a quad: both triangles at the same t) and at vertices
    n = 6000
    k = rng.randint(0, len(tri), n)
    tgt = np.where(rng.rand(n, 1) < 0.5, 0.5 * (tri[k, 1] + tri[k, 2]), tri[k, rng.randint(0, 3, n)]).astype(np.float32)
    o = (lo + (hi - lo) * rng.rand(n, 3)).astype(np.float32)
    d = _unit(tgt - o)
    maxt = np.where(rng.rand(n) < 0.3, np.linalg.norm(tgt - o, axis=1), np.inf).astype(np.float32)      # segments ending at the target
    groups.append((o, d, np.zeros(n, np.float32), maxt))
    o, d, mint, maxt = (np.concatenate([g[i] for g in groups]).astype(np.float32) for i in range(4))
    perm = rng.permutation(len(o))                         # mix the kinds within a wave
    return o[perm], d[perm], mint[perm], maxt[perm]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("partial", [False, True])
def test_flat_worklist_stress(gpu, oracle, partial):
    sd = scenes.cornell_box()
    scene = gpu.Scene(sd)
    S = oracle.OracleScene(sd)
    o, d, mint, maxt = _stress_rays(sd, 5)
    n = len(o) - 27                                        # the last wave is partial
    o, d, mint, maxt = o[:n], d[:n], mint[:n], maxt[:n]
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ray = gpu.Ray3f(o=t_(o), d=t_(d), mint=t_(mint), maxt=t_(maxt))
    act = (np.random.RandomState(9).rand(n) < 0.6) if partial else np.ones(n, bool)
    active = torch.from_numpy(act.astype(np.uint8)).cuda() if partial else True
    t_o, prim_o, _, u_o, v_o = S.ray_intersect(o, d, mint, maxt, naive=True)
    hit_o = S.ray_test(o, d, mint, maxt, naive=True)
    t_o = np.where(act, t_o, np.inf).astype(np.float32)
    prim_o = np.where(act, prim_o, np.uint32(0xffffffff)).astype(np.uint32)
    u_o, v_o = np.where(act, u_o, 0.0).astype(np.float32), np.where(act, v_o, 0.0).astype(np.float32)
    hit_o = hit_o & act
    assert np.isfinite(t_o).sum() > n // 4 and (act & (t_o == 0)).sum() > 0
    res = scene.ray_intersect(ray, active=active, full=False)
    t_g, prim_g = res.t.cpu().numpy(), res.prim_index.cpu().numpy().astype(np.uint32)
    uv_g = res.prim_uv.cpu().numpy()
    mism = (t_g != t_o) | (prim_g != prim_o) | (uv_g[:, 0] != u_o) | (uv_g[:, 1] != v_o)
    assert mism.sum() == 0, "mismatches: %d of %d: %s" % (mism.sum(), n, [(int(i), o[i].tolist(), d[i].tolist(), float(mint[i]), float(maxt[i]), float(t_g[i]), int(prim_g[i]), float(t_o[i]), int(prim_o[i])) for i in np.nonzero(mism)[0][:6]])
    rn = scene.ray_intersect_naive(ray, active=active)
    assert (_bits(rn.t.cpu().numpy()) == _bits(t_g)).all() and (rn.prim_index.cpu().numpy().astype(np.uint32) == prim_g).all()
    assert (_bits(rn.prim_uv.cpu().numpy()) == _bits(uv_g)).all()
    hit_g = scene.ray_test(ray, active=active).cpu().numpy()
    bad = np.nonzero(hit_g != hit_o)[0]
    assert bad.size == 0, "ray_test mismatches: %s" % [(int(i), o[i].tolist(), d[i].tolist(), float(mint[i]), float(maxt[i]), bool(hit_g[i])) for i in bad[:6]]


def test_flat_worklist_signed_zero_hits(gpu, oracle):
    """mint = 0 from points on the walls: t = +-0 hits keep the sign of the sequential loop's (== the brute force's) t."""
    sd = scenes.cornell_box()
    scene = gpu.Scene(sd)
    tri = _tris(sd)
    rng = np.random.RandomState(3)
    n = 20000
    k = rng.randint(0, len(tri), n)
    b = rng.rand(n, 2).astype(np.float32) * 0.5
    o = (tri[k, 0] + b[:, :1] * (tri[k, 1] - tri[k, 0]) + b[:, 1:] * (tri[k, 2] - tri[k, 0])).astype(np.float32)
    d = _unit(rng.randn(n, 3))
    z = np.zeros(n, np.float32)
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ray = gpu.Ray3f(o=t_(o), d=t_(d), mint=t_(z), maxt=t_(np.full(n, np.inf, np.float32)))
    res = scene.ray_intersect(ray, full=False)
    rn = scene.ray_intersect_naive(ray)
    t_g = res.t.cpu().numpy()
    assert (t_g == 0).sum() > n // 20
    assert (_bits(t_g) == _bits(rn.t.cpu().numpy())).all()
    assert (res.prim_index.cpu().numpy() == rn.prim_index.cpu().numpy()).all()
    assert (_bits(res.prim_uv.cpu().numpy()) == _bits(rn.prim_uv.cpu().numpy())).all()

"""Hard rays for flat-scene ray queries, shared by the GPU tests that compare the device's closest-hit and any-hit answers with brute
force: origins on surfaces, grazing and axis-parallel directions, mint = 0 with hits at +-0, exact ties between two triangles."""
import numpy as np


def tris(sd):
    p = []
    for m in sd["meshes"]:
        p.append(m["positions"][m["faces"].astype(np.int64)])
    return np.concatenate(p).astype(np.float32)          # [n_tris, 3 vertices, 3]


def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def stress_rays(sd, seed):
    rng = np.random.RandomState(seed)
    tri = tris(sd)
    allp = tri.reshape(-1, 3)
    lo, hi = allp.min(0), allp.max(0)
    groups = []
    # 1. origins on surfaces (random barycentrics), directions all over the sphere, the shading code's mint and mint = 0
    n = 6000
    k = rng.randint(0, len(tri), n)
    b = rng.rand(n, 2).astype(np.float32)
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    o = tri[k, 0] + b[:, :1] * (tri[k, 1] - tri[k, 0]) + b[:, 1:] * (tri[k, 2] - tri[k, 0])
    d = unit(rng.randn(n, 3))
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
    nrm = unit(np.cross(e1, e2))
    tang = unit(np.cross(nrm, rng.randn(n, 3)))
    eps = np.array([0.0, 1e-7, -1e-7, 1e-4, -1e-3], np.float32)[rng.randint(0, 5, n)][:, None]
    d = unit(tang + eps * nrm)
    o = (tri[k, 0] + 0.3 * e1 + 0.3 * e2 - 2.0 * np.abs(hi - lo).max() * d).astype(np.float32)
    groups.append((o, d, np.zeros(n, np.float32), np.full(n, np.inf, np.float32)))
    # 3. mint = 0 and hits at t = +-0: origins exactly at vertices and on edges (shared by two triangles: exact ties), both sides
    n = 6000
    k = rng.randint(0, len(tri), n)
    w = np.array([0.0, 0.5, 1.0], np.float32)[rng.randint(0, 3, n)][:, None]
    o = (tri[k, 0] + w * (tri[k, 1] - tri[k, 0])).astype(np.float32)
    d = unit(rng.randn(n, 3))
    groups.append((o, d, np.zeros(n, np.float32), np.full(n, np.inf, np.float32)))
    # 4. exact ties: rays aimed at the midpoint of an edge (the diagonal of a quad: both triangles at the same t) and at vertices
    n = 6000
    k = rng.randint(0, len(tri), n)
    tgt = np.where(rng.rand(n, 1) < 0.5, 0.5 * (tri[k, 1] + tri[k, 2]), tri[k, rng.randint(0, 3, n)]).astype(np.float32)
    o = (lo + (hi - lo) * rng.rand(n, 3)).astype(np.float32)
    d = unit(tgt - o)
    maxt = np.where(rng.rand(n) < 0.3, np.linalg.norm(tgt - o, axis=1), np.inf).astype(np.float32)      # segments ending at the target
    groups.append((o, d, np.zeros(n, np.float32), maxt))
    o, d, mint, maxt = (np.concatenate([g[i] for g in groups]).astype(np.float32) for i in range(4))
    perm = rng.permutation(len(o))                         # mix the kinds within a wave
    return o[perm], d[perm], mint[perm], maxt[perm]

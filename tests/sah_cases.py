"""Inputs, the host driver and the numpy replay shared by tests/test_sah_levels_cpu.py and tests/test_gpu_rebuild_sah.py.

tests/sah_levels_driver.cpp is the host specification of the SAH accelerator rebuild (build_sah_levels) as a stand-alone program, beside
build_bvh (creation's builder) and build_lbvh; `Driver.run` is lbvh_cases.Driver's.  `replay` restates the rules of build_sah_levels in
numpy float64, from the triangles alone: IEEE double in the expression order of csrc/sah_keys.h, so every decision can be held to it
exactly."""
import os
import subprocess

import numpy as np

import lbvh_cases as lc
import vertex_moves as vm

F32, F64, I32 = np.float32, np.float64, np.int32
BINS, INTERSECT, GUARD_DEPTH = 16, 1.5, 40
LEAF, SPLIT_BIN, SPLIT_MIDDLE = 0, 1, 2
WAVE_NODE, SHARE_LEVEL = 64, 8          # kSahWaveNode, kSahShareLevel of csrc/sah_build.h


class Driver(lc.Driver):
    """tests/sah_levels_driver.cpp compiled with the host builder; `flags`: extra compiler flags (a sanitizer build)"""

    def __init__(self, directory, flags=()):
        self.directory = str(directory)
        self.exe = os.path.join(self.directory, "sah_levels_driver")
        subprocess.check_call([vm.HIPCC, "-std=c++17", "-O1", "-ffp-contract=off", "-I", vm.CSRC, "-o", self.exe] + list(flags) +
                              ["-x", "hip", "--cuda-host-only", os.path.join(vm.HERE, "sah_levels_driver.cpp"), os.path.join(vm.CSRC, "scene_build.cpp"), "-x", "c++"] +
                              [os.path.join(vm.CSRC, f) for f in ("bvh.cpp", "envmap.cpp", "spectral_upsampling.cpp")], stderr=subprocess.DEVNULL)


def depth_guard_set():
    """30 thin triangles at (2^-4i, 0, 0), 30 at (0, 2^-4i, 0), 30 at (0, 0, 2^-4i), each with vertices p, p (1 + 1e-3), p (1 - 1e-3): the
    binned SAH peels one scale off per level, 45 levels deep, so the split in the middle of the order from depth 40 on is taken"""
    tri = []
    for axis in range(3):
        for i in range(30):
            p = np.zeros(3)
            p[axis] = 2.0 ** (-4 * i)
            tri.append([p, p * (1 + 1e-3), p * (1 - 1e-3)])
    return np.array(tri, F32)


def skewed(n_cluster=300, n_far=40, seed=9):
    """a dense cluster and a few triangles far away: levels of many nodes that still hold a node of more than WAVE_NODE primitives"""
    rng = np.random.RandomState(seed)
    c = np.concatenate([rng.uniform(0.0, 0.05, (n_cluster, 1, 3)), rng.uniform(-8.0, 8.0, (n_far, 1, 3))])
    return (c + rng.uniform(-0.01, 0.01, (len(c), 3, 3))).astype(F32)


def threshold_set(seed=13):
    """two clusters far apart, of WAVE_NODE and WAVE_NODE + 1 triangles: the root's children are the largest node one wave decides and
    the smallest a whole workgroup does"""
    rng = np.random.RandomState(seed)
    c = np.concatenate([rng.uniform(0.0, 1.0, (WAVE_NODE, 1, 3)), rng.uniform(0.0, 1.0, (WAVE_NODE + 1, 1, 3)) + np.array([100.0, 0.0, 0.0])])
    return (c + rng.uniform(-0.1, 0.1, (len(c), 3, 3))).astype(F32)


def _area(lo, hi):
    dx, dy, dz = hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]
    if dx < 0:
        return F64(0.0)
    return 2.0 * (dx * dy + dy * dz + dz * dx)


def node_bins(lo, hi, cen, ids, clo, chi):
    """per axis: None (no centroid extent), or (bin of every primitive, count per bin, box lo per bin, box hi per bin)"""
    out = []
    for a in range(3):
        ext = chi[a] - clo[a]
        if not ext > 0.0:
            out.append(None)
            continue
        scale = F64(BINS) / ext
        b = np.clip(((cen[ids, a] - clo[a]) * scale).astype(np.int64), 0, BINS - 1)
        cnt = np.bincount(b, minlength=BINS)
        blo = np.full((BINS, 3), np.inf)
        bhi = np.full((BINS, 3), -np.inf)
        for k in np.nonzero(cnt)[0]:
            blo[k], bhi[k] = lo[ids[b == k]].min(0), hi[ids[b == k]].max(0)
        out.append((b, cnt, blo, bhi))
    return out


def decide(lo, hi, cen, ids, depth, max_leaf):
    """-> mode, primitives of the left child, (axis, bin, cost) of the search, left mask (SPLIT_BIN only), bins"""
    count = len(ids)
    if count <= 1:
        return LEAF, 0, (-1, -1, np.finfo(F64).max), None, None
    clo, chi = cen[ids].min(0), cen[ids].max(0)
    parent = max(_area(lo[ids].min(0), hi[ids].max(0)), F64(1e-300))
    bins = node_bins(lo, hi, cen, ids, clo, chi)
    best, ba, bb = np.finfo(F64).max, -1, -1
    for a in range(3):
        if bins[a] is None:
            continue
        _, cnt, blo, bhi = bins[a]
        right_area, right_cnt = np.zeros(BINS), np.zeros(BINS, np.int64)
        alo, ahi, c = np.full(3, np.inf), np.full(3, -np.inf), 0
        for b in range(BINS - 1, 0, -1):
            if cnt[b]:
                alo, ahi = np.minimum(alo, blo[b]), np.maximum(ahi, bhi[b])
            c += cnt[b]
            right_area[b], right_cnt[b] = (_area(alo, ahi) if c else 0.0), c
        alo, ahi, c = np.full(3, np.inf), np.full(3, -np.inf), 0
        for b in range(BINS - 1):
            if cnt[b]:
                alo, ahi = np.minimum(alo, blo[b]), np.maximum(ahi, bhi[b])
            c += cnt[b]
            if c == 0 or right_cnt[b + 1] == 0:
                continue
            cost = 1.0 + INTERSECT * (_area(alo, ahi) * F64(c) + right_area[b + 1] * F64(right_cnt[b + 1])) / parent
            if cost < best:
                best, ba, bb = cost, a, b
    found = (ba, bb, best)
    if count <= max_leaf and (ba < 0 or INTERSECT * count <= best):
        return LEAF, 0, found, None, bins
    if ba < 0 or depth >= GUARD_DEPTH:
        return SPLIT_MIDDLE, count // 2, found, None, bins
    left = bins[ba][0] <= bb
    assert 0 < left.sum() < count
    return SPLIT_BIN, int(left.sum()), found, left, bins


def replay(tri, max_leaf=lc.MAX_LEAF, keep_bins=16):
    """the tree of build_sah_levels from the triangles: kids, node_child, slot_prim, per builder node (first, count, depth, mode, left,
    axis, bin, cost), and the bins of the first `keep_bins` nodes of more than one primitive"""
    tri = np.asarray(tri, F32).reshape(-1, 3, 3)
    lo, hi = tri.min(1).astype(F64), tri.max(1).astype(F64)
    cen = 0.5 * (lo + hi)
    n = len(tri)
    perm = np.arange(n)
    level, base, n_inner, n_slots, depth = [(0, n)], 0, 0, 0, 0
    kids, node_child, slot_prim, nodes, kept = [], [], np.zeros(n, np.uint32), [], []
    while level:
        next_base, nxt, new_perm, r = base + len(level), [], perm.copy(), 0
        for j, (first, count) in enumerate(level):
            ids = perm[first:first + count]
            mode, left, (axis, b, cost), mask, bins = decide(lo, hi, cen, ids, depth, max_leaf)
            nodes.append((first, count, depth, mode, left, axis, b, cost))
            if bins is not None and len(kept) < keep_bins:
                kept.append((base + j, bins))
            if mode == LEAF:
                kids.append((-1, int(np.uint32(0x80000000 | (count << 27) | n_slots).view(I32))))
                slot_prim[n_slots:n_slots + count] = ids
                n_slots += count
                continue
            l = next_base + 2 * r
            r += 1
            kids.append((l, l + 1))
            node_child.append((l, l + 1))
            nxt += [(first, left), (first + left, count - left)]
            if mode == SPLIT_BIN:
                new_perm[first:first + count] = np.concatenate([ids[mask], ids[~mask]])
        n_inner += r
        base, level, perm, depth = next_base, nxt, new_perm, depth + 1
    return dict(kids=np.array(kids, I32).reshape(-1, 2), node_child=np.array(node_child, I32).reshape(-1, 2), slot_prim=slot_prim, nodes=nodes,
                bins=kept, levels=depth)


def leaf_sets(kids, slot_prim, tris=None):
    """the leaves in slot order: [(first, sorted primitives, their slot records sorted by primitive)]"""
    refs = kids[kids[:, 0] < 0, 1].view(np.uint32)
    out = []
    for ref in sorted(refs, key=lambda x: int(x) & 0x07ffffff):
        first, count = int(ref) & 0x07ffffff, (int(ref) >> 27) & 15
        prims = slot_prim[first:first + count]
        o = np.argsort(prims, kind="stable")
        out.append((first, prims[o].tolist(), None if tris is None else tris.reshape(-1, 12)[first:first + count][o].tolist()))
    return out


def sah_terms(kids, boxes):
    """the terms of sah_cost_blocked per builder node, sorted: the two builders number the nodes differently, the multiset is the same"""
    d = boxes[:, 3:].astype(F64) - boxes[:, :3].astype(F64)
    area = 2.0 * (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0])
    return area, kids[:, 0] >= 0

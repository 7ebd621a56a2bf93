#!/usr/bin/env python3
"""What recomputing the vertex normals of a moved mesh costs, on the device and on the host, on scenes.matpreview() (a displaced sphere
of ~262 k triangles with normals, a ground plane, an area light, an envmap).  The positions live on the device, as an optimisation loop
holds them; every call moves every vertex (two position sets alternate).

* `recompute`: Scene.update_vertices(shape, positions, normals="recompute"), end to end: the clone the scene keeps, the output tensor,
  mtsamd_scene_update_vertices with MTSAMD_VERTICES_RECOMPUTE_NORMALS (k_normals_faces, k_normals_vertices, then the refit);
* `host-normals`: Scene.update_vertices(shape, positions) with normals=None on the same tensors, the path before this one: the
  positions go to the host, loaders.compute_vertex_normals runs in float64 numpy, the normals come back and the description is mirrored;
* `abi-recompute` / `abi-given`: the library call alone, with the flag and normals_out, and without the flag given device normals (the
  figure of scripts/bench_vertex_update.py) -- their difference is what the two normals kernels and the copy of the result add;
* `first-recompute`: the first call for a shape, which reads the face indices back, builds the vertex-to-corner table on the host and
  uploads it; once per shape and scene;
* `flush`: reading Scene._dict after a recompute, which copies the pending arrays to the host (what a loop pays only when it looks).

The per-kernel split comes from a kernel trace of this script (--abi-only), taken in a run of its own.  One JSON line per figure: the
median and the range of --rounds timings after --warmup.  No threshold: these are first measurements."""
import argparse
import copy
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mitsuba2_amd import _lib as L, render, scenes

SPHERE = 0


def report(name, times, **extra):
    print(json.dumps(dict(figure=name, median_ms=1e3 * statistics.median(times), min_ms=1e3 * min(times), max_ms=1e3 * max(times), rounds=len(times), **extra)), flush=True)


def timed(fn, rounds, warmup):
    out = []
    for k in range(warmup + rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(k)
        torch.cuda.synchronize()
        if k >= warmup:
            out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-rounds", type=int, default=5)
    ap.add_argument("--theta", type=int, default=256)
    ap.add_argument("--abi-only", action="store_true", help="the two library calls only (the run under the kernel trace)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    sd = scenes.matpreview(a.theta, 2 * a.theta)
    n_tris = sum(len(np.asarray(m["faces"]).reshape(-1, 3)) for m in sd["meshes"])
    mesh = sd["meshes"][SPHERE]
    pos = np.asarray(mesh["positions"], np.float64).reshape(-1, 3)
    moved = pos + np.random.RandomState(5).uniform(-0.02, 0.02, pos.shape)
    sets = [torch.from_numpy(np.ascontiguousarray(p, np.float32)).cuda() for p in (pos, moved)]
    scene = render.Scene(copy.deepcopy(sd))
    lib, stream = L.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty_like(sets[0])
    extra = dict(triangles=n_tris, vertices=len(pos))

    t0 = time.perf_counter()
    L.check(lib.mtsamd_scene_update_vertices(scene._handle, SPHERE, C.c_void_p(sets[1].data_ptr()), None, 1, C.c_void_p(out.data_ptr()), stream))
    report("first-recompute", [time.perf_counter() - t0], **extra)
    normals = [None, out.clone()]
    L.check(lib.mtsamd_scene_update_vertices(scene._handle, SPHERE, C.c_void_p(sets[0].data_ptr()), None, 1, C.c_void_p(out.data_ptr()), stream))
    normals[0] = out.clone()

    def abi_recompute(k):
        L.check(lib.mtsamd_scene_update_vertices(scene._handle, SPHERE, C.c_void_p(sets[(k + 1) % 2].data_ptr()), None, 1, C.c_void_p(out.data_ptr()), stream))
    report("abi-recompute", timed(abi_recompute, a.rounds, a.warmup), **extra)

    def abi_given(k):
        i = (k + 1) % 2
        L.check(lib.mtsamd_scene_set_vertex_positions(scene._handle, SPHERE, C.c_void_p(sets[i].data_ptr()), C.c_void_p(normals[i].data_ptr()), stream))
    report("abi-given", timed(abi_given, a.rounds, a.warmup), **extra)
    if a.abi_only:
        return

    report("recompute", timed(lambda k: scene.update_vertices(SPHERE, sets[(k + 1) % 2], normals="recompute"), a.rounds, a.warmup), **extra)

    def flush(k):
        scene.update_vertices(SPHERE, sets[(k + 1) % 2], normals="recompute")
        torch.cuda.synchronize()
        t = time.perf_counter()
        scene._dict
        flush.times.append(time.perf_counter() - t)
    flush.times = []
    timed(flush, a.host_rounds, 1)
    report("flush", flush.times[1:], **extra)

    report("host-normals", timed(lambda k: scene.update_vertices(SPHERE, sets[(k + 1) % 2]), a.host_rounds, 1), **extra)


if __name__ == "__main__":
    main()

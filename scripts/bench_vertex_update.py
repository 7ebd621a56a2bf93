#!/usr/bin/env python3
"""What a vertex update costs, and what the kept topology costs afterwards, on scenes.matpreview() (a displaced sphere of ~262 k
triangles, its normals, a ground plane, an area light, an envmap).

* `update`: mtsamd_scene_set_vertex_positions of the sphere with positions and normals that already live on the device, synchronised
  wall clock per call, alternating between two position sets so that every call moves every vertex;
* `create`: render.Scene(description) of the same scene -- the host SAH build, the uploads and the Python marshalling of the description.
  It is the only way to move a vertex without the update; run the script with --lib on a build of the parent commit to time it there
  (`--create-only` implied: that library lacks the update);
* per move (jitter, shrink, translate-out): triangle tests per closest-hit query (stats tri_tests / closest_hit_rays) and the time of
  one render of the refitted scene beside a fresh scene of the moved mesh.  Both run the same kernels on the same triangles; only the
  topology of the accelerator differs.

The split of an update by stage and the number of propagation launches come from a kernel trace of this script (the kernels are named
k_refit_check, k_refit_gather, k_refit_leaves, k_refit_level -- one launch per height class -- and k_refit_emit), taken in a run of its own.
One JSON line per figure: the median and the range of --rounds timings after --warmup.  No threshold: these are first measurements."""
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
from mitsuba2_amd import _lib as L, loaders, render, scenes

SPHERE = 0
CENTRE = np.array([0.0, 1.2, 0.0])


def moves(pos):
    rng = np.random.RandomState(5)
    return {"jitter": pos + rng.uniform(-0.02, 0.02, pos.shape), "shrink": (pos - CENTRE) * 0.5 + CENTRE, "translate-out": pos + np.array([9.0, 0.5, 0.0])}


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
    ap.add_argument("--create-rounds", type=int, default=3)
    ap.add_argument("--theta", type=int, default=256)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--lib", default=None, help="time scene creation with this libmtsamd.so (a build of another commit)")
    ap.add_argument("--create-only", action="store_true")
    ap.add_argument("--no-renders", action="store_true", help="stop after the update timings (the run under the kernel trace)")
    a = ap.parse_args()
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)
        for name in ("mtsamd_scene_set_vertex_positions", "mtsamd_scene_read_accel"):
            L.SYMBOLS.pop(name, None)
        a.create_only = True
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    sd = scenes.matpreview(a.theta, 2 * a.theta)
    n_tris = sum(len(np.asarray(m["faces"]).reshape(-1, 3)) for m in sd["meshes"])
    descriptions = [copy.deepcopy(sd) for _ in range(a.create_rounds + 1)]      # the copy is not part of the timing
    held = []

    def create(k):
        held[:] = [render.Scene(descriptions[k])]             # (the scene before it is destroyed here: part of what a user pays)
    report("create", timed(create, a.create_rounds, 1), triangles=n_tris, library=a.lib or "this build")
    held.clear()
    if a.create_only:
        return
    scene = render.Scene(copy.deepcopy(sd))
    mesh = sd["meshes"][SPHERE]
    pos = np.asarray(mesh["positions"], np.float64).reshape(-1, 3)
    sets = []
    for p in (pos, moves(pos)["jitter"]):
        p32 = np.ascontiguousarray(p, np.float32)
        sets.append((torch.from_numpy(p32).cuda(), torch.from_numpy(np.ascontiguousarray(loaders.compute_vertex_normals(p32, mesh["faces"]), np.float32)).cuda()))
    lib, stream = L.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def update(k):
        p, n = sets[(k + 1) % 2]
        L.check(lib.mtsamd_scene_set_vertex_positions(scene._handle, SPHERE, C.c_void_p(p.data_ptr()), C.c_void_p(n.data_ptr()), stream))
    report("update", timed(update, a.rounds, a.warmup), triangles=n_tris, vertices=len(pos), info=scene.info())

    if a.no_renders:
        return
    sp = scenes.bumpy_sphere_sensor(a.width, a.width * 3 // 4, a.spp, seed=1, max_depth=6)
    for name, p in moves(pos).items():
        p32 = np.ascontiguousarray(p, np.float32)
        refitted = render.Scene(copy.deepcopy(sd))
        refitted.update_vertices(SPHERE, torch.from_numpy(p32).cuda())
        new = copy.deepcopy(sd)
        new["meshes"][SPHERE] = dict(new["meshes"][SPHERE], positions=p32, normals=np.ascontiguousarray(loaders.compute_vertex_normals(p32, mesh["faces"]), np.float32))
        fresh = render.Scene(new)
        films = {}
        for label, s in (("refitted", refitted), ("fresh", fresh)):
            integ, sensor = render.PathIntegrator(max_depth=6), render.make_sensor(sp)
            times = timed(lambda k: integ.render(s, sensor), max(a.rounds // 4, 3), 1)
            films[label] = sensor.film().bitmap(raw=True).clone()
            st = integ.stats
            report("render-after-%s-%s" % (name, label), times, tri_tests_per_closest_hit=st["tri_tests"] / max(st["closest_hit_rays"], 1),
                   closest_hit_rays=st["closest_hit_rays"], any_hit_rays=st["any_hit_rays"])
        print(json.dumps(dict(figure="films-equal-after-%s" % name, equal=bool(torch.equal(films["refitted"], films["fresh"])))), flush=True)


if __name__ == "__main__":
    main()

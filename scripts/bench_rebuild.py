#!/usr/bin/env python3
"""What an accelerator rebuild costs and what the rebuilt tree is worth, on scenes.matpreview() (a displaced sphere of ~262 k triangles,
a ground plane, an area light, an envmap).

(a) `rebuild`: Scene.rebuild_accel(builder=...) end to end per --builder (`lbvh`, `sah` or `both`; the figure carries the builder),
    synchronised wall clock per call, and for the SAH builder the host's wall time per level of the last build; beside it `refit` (mtsamd_scene_set_vertex_positions
    with arrays on the device) and `create` (render.Scene of the same description: the only alternative without the rebuild).  Run the
    script with --lib on a build of the parent commit to time creation there (--create-only implied).  The split by stage comes from a
    kernel trace of `--no-renders`, taken in a run of its own.
(b) tree quality: triangle tests per closest-hit query, the time of one 256x192x16 render and accel_info's SAH cost for four trees --
    the SAH tree of a fresh scene, that tree refitted, the LBVH of a rebuild, the SAH tree of a rebuild -- without a move, after each of bench_vertex_update.py's
    three moves, and after one large deformation (squash to a tenth of the height plus a jitter of 0.2).
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
    squashed = pos.copy()
    squashed[:, 1] = CENTRE[1] + 0.1 * (pos[:, 1] - CENTRE[1])
    return {"none": pos, "jitter": pos + rng.uniform(-0.02, 0.02, pos.shape), "shrink": (pos - CENTRE) * 0.5 + CENTRE,
            "translate-out": pos + np.array([9.0, 0.5, 0.0]), "squash-jitter": squashed + np.random.RandomState(6).uniform(-0.2, 0.2, pos.shape)}


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
    ap.add_argument("--builder", choices=("lbvh", "sah", "both"), default="both", help="the builder(s) of the rebuilds that are timed and rendered")
    ap.add_argument("--moves", default=None, help="comma-separated subset of the deformations of (b)")
    ap.add_argument("--lib", default=None, help="time scene creation with this libmtsamd.so (a build of another commit)")
    ap.add_argument("--create-only", action="store_true")
    ap.add_argument("--no-renders", action="store_true", help="stop after the timings of (a) (the run under the kernel trace)")
    a = ap.parse_args()
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)
        for name in ("mtsamd_scene_rebuild_accel", "mtsamd_scene_accel_info", "mtsamd_scene_rebuild_accel_with", "mtsamd_scene_rebuild_levels"):
            L.SYMBOLS.pop(name, None)
        a.create_only = True
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    sd = scenes.matpreview(a.theta, 2 * a.theta)
    n_tris = sum(len(np.asarray(m["faces"]).reshape(-1, 3)) for m in sd["meshes"])
    descriptions = [copy.deepcopy(sd) for _ in range(a.create_rounds + 1)]
    held = []

    def create(k):
        held[:] = [render.Scene(descriptions[k])]
    report("create", timed(create, a.create_rounds, 1), triangles=n_tris, library=a.lib or "this build")
    held.clear()
    if a.create_only:
        return
    scene = render.Scene(copy.deepcopy(sd))
    mesh = sd["meshes"][SPHERE]
    pos = np.asarray(mesh["positions"], np.float64).reshape(-1, 3)
    normals = lambda p32: np.ascontiguousarray(loaders.compute_vertex_normals(p32, mesh["faces"]), np.float32)
    sets = []
    for p in (pos, moves(pos)["jitter"]):
        p32 = np.ascontiguousarray(p, np.float32)
        sets.append((torch.from_numpy(p32).cuda(), torch.from_numpy(normals(p32)).cuda()))
    lib, stream = L.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refit(k):
        p, n = sets[(k + 1) % 2]
        L.check(lib.mtsamd_scene_set_vertex_positions(scene._handle, SPHERE, C.c_void_p(p.data_ptr()), C.c_void_p(n.data_ptr()), stream))
    report("refit", timed(refit, a.rounds, a.warmup), triangles=n_tris)
    builders = ("lbvh", "sah") if a.builder == "both" else (a.builder,)
    for builder in builders:
        report("rebuild", timed(lambda k: scene.rebuild_accel(builder=builder), a.rounds, a.warmup), builder=builder, triangles=n_tris,
               info=scene.accel_info(sah_cost=True))
        if builder == "sah":
            levels = scene.rebuild_levels()
            print(json.dumps(dict(figure="rebuild-levels", builder=builder, levels=len(levels), total_ms=sum(ms for _, ms in levels),
                                  nodes=[m for m, _ in levels], ms=[round(ms, 4) for _, ms in levels])), flush=True)

        def both(k):
            p, n = sets[(k + 1) % 2]
            L.check(lib.mtsamd_scene_update_vertices(scene._handle, SPHERE, C.c_void_p(p.data_ptr()), C.c_void_p(n.data_ptr()), 2 | (8 if builder == "sah" else 0),
                                                     None, stream))
        report("update-and-rebuild", timed(both, a.rounds, a.warmup), builder=builder, triangles=n_tris)
    if a.no_renders:
        return

    sp = scenes.bumpy_sphere_sensor(a.width, a.width * 3 // 4, a.spp, seed=1, max_depth=6)
    for name, p in moves(pos).items():
        if a.moves and name not in a.moves.split(","):
            continue
        p32 = np.ascontiguousarray(p, np.float32)
        new = copy.deepcopy(sd)
        new["meshes"][SPHERE] = dict(new["meshes"][SPHERE], positions=p32, normals=normals(p32))
        trees = {"fresh-sah": render.Scene(new)}
        if name != "none":
            trees["refitted-sah"] = render.Scene(copy.deepcopy(sd))
            trees["refitted-sah"].update_vertices(SPHERE, torch.from_numpy(p32).cuda())
        for builder in builders:
            trees["rebuilt-" + builder] = render.Scene(copy.deepcopy(sd))
            trees["rebuilt-" + builder].update_vertices(SPHERE, torch.from_numpy(p32).cuda(), accel="rebuild" if builder == "lbvh" else "rebuild-sah")
        films = {}
        for label, s in trees.items():
            integ, sensor = render.PathIntegrator(max_depth=6), render.make_sensor(sp)
            times = timed(lambda k: integ.render(s, sensor), max(a.rounds // 4, 3), 1)
            films[label] = sensor.film().bitmap(raw=True).clone()
            st = integ.stats
            report("render-after-%s-%s" % (name, label), times, tri_tests_per_closest_hit=st["tri_tests"] / max(st["closest_hit_rays"], 1),
                   accel=s.accel_info(sah_cost=True))
        print(json.dumps(dict(figure="films-equal-after-%s" % name, equal=all(bool(torch.equal(f, films["fresh-sah"])) for f in films.values()))), flush=True)


if __name__ == "__main__":
    main()

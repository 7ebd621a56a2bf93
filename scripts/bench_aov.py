#!/usr/bin/env python3
"""Cost of the `aov` integrator (src/integrators/aov.cpp) beside a path-traced render: the Cornell box at 512 x 512 x 64 spp and the
261 k-triangle displaced sphere at 640 x 360 x 16 spp, each as plain `path`, as `aov` (depth + sh_normal + position) around `path`, and
as `aov` alone.  The three variants are run in turn, round after round, so that drift of the device hits them alike; the median and the
range of the wall-clock times are printed with the device times of the trace / AOV kernels (stats[5]) and of the film splats (stats[6])."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mitsuba2_amd import render, scenes

AOVS = "depth:depth n:sh_normal p:position"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="scales both film sizes (quick runs)")
    args = ap.parse_args()
    s = args.scale
    cases = [("cbox 512x512x64", scenes.cornell_box(), scenes.cornell_box_sensor(int(512 * s), int(512 * s), 64)),
             ("mesh261k 640x360x16", scenes.bumpy_sphere(256, 512), scenes.bumpy_sphere_sensor(int(640 * s), int(360 * s), 16))]
    for name, sd, sp in cases:
        scene, sensor = render.Scene(sd), render.make_sensor(sp)
        variants = [("path", render.PathIntegrator()), ("aov(path)", render.AOVIntegrator(AOVS, render.PathIntegrator(), name="img")),
                    ("aov alone", render.AOVIntegrator(AOVS))]
        times = {k: [] for k, _ in variants}
        dev = {k: [] for k, _ in variants}
        for r in range(args.warmup + args.rounds):
            for k, integ in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                assert integ.render(scene, sensor)
                torch.cuda.synchronize()
                if r >= args.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
                    dev[k].append((integ.stats["bounce_ns"] * 1e-6, integ.stats["film_ns"] * 1e-6))
        for k, _ in variants:
            t, d = np.array(times[k]), np.array(dev[k])
            print(json.dumps(dict(case=name, variant=k, rounds=args.rounds, wall_ms_median=round(float(np.median(t)), 3),
                                  wall_ms_range=[round(float(t.min()), 3), round(float(t.max()), 3)],
                                  trace_ms_median=round(float(np.median(d[:, 0])), 3), trace_ms_range=[round(float(d[:, 0].min()), 3), round(float(d[:, 0].max()), 3)],
                                  film_ms_median=round(float(np.median(d[:, 1])), 3), film_ms_range=[round(float(d[:, 1].min()), 3), round(float(d[:, 1].max()), 3)])))


if __name__ == "__main__":
    main()

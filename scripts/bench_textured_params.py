#!/usr/bin/env python3
"""Cost of textured BSDF parameters (alpha, specular colours) on the Cornell box at 512 x 512 x 64 spp, tall box = the material:

* `blend`     the `blend_rough_diffuse` material of tests/test_gpu_bsdfs.py: the scene that already ran the nested (general == 2) kernels
              before they learned to resolve textured parameters.  Run this script on the parent commit and on this one: the median of
              the new build may exceed the parent's by no more than the parent's own run-to-run range;
* `constant`  a constant roughconductor: the general == 1 kernels;
* `map`       the same roughconductor with a checkerboard alpha of two equal colours: general == 2 plus a lookup per hit.  map / constant is
              the price of a roughness map (a build without textured parameters reports `map` as unavailable).

The variants are rendered in turn, round after round, so that drift of the device hits them alike; after `--warmup` rounds the median
and the range of `--rounds` wall-clock times (synchronised) are printed with the device time of the trace kernels, one JSON line each."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mitsuba2_amd import render, scenes

IOR = {"eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14]}
ROUGH = dict(type="roughconductor", alpha=0.2, distribution="ggx", **IOR)
MATERIALS = {
    "blend": {"type": "blendbsdf", "weight": 0.3, "bsdf_0": ROUGH, "bsdf_1": {"type": "diffuse", "reflectance": [0.2, 0.5, 0.7]}},
    "constant": ROUGH,
    "map": dict(ROUGH, alpha={"type": "checkerboard", "color0": 0.2, "color1": 0.2}),
}


def box_scene(material):
    cb = scenes.cornell_box()
    tall = len(cb["meshes"]) - 1
    uv = np.tile(np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32), (6, 1))       # every variant carries the same texcoords
    cb["bsdfs"] = list(cb["bsdfs"]) + [material]
    cb["meshes"][tall] = dict(cb["meshes"][tall], bsdf=len(cb["bsdfs"]) - 1, texcoords=uv)
    return cb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sensor = render.make_sensor(scenes.cornell_box_sensor(args.size, args.size, args.spp))
    variants = []
    for name, material in MATERIALS.items():
        try:
            variants.append((name, render.Scene(box_scene(material)), render.PathIntegrator()))
        except (RuntimeError, TypeError) as e:
            print(json.dumps(dict(label=args.label, variant=name, unavailable=str(e)[:120])))
    times, dev = {k: [] for k, _, _ in variants}, {k: [] for k, _, _ in variants}
    for r in range(args.warmup + args.rounds):
        for k, scene, integ in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert integ.render(scene, sensor)
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
                dev[k].append(integ.stats["bounce_ns"] * 1e-6)
    for k, _, _ in variants:
        t, d = np.array(times[k]), np.array(dev[k])
        print(json.dumps(dict(label=args.label, variant=k, film="%dx%dx%d" % (args.size, args.size, args.spp), rounds=args.rounds,
                              wall_ms_median=round(float(np.median(t)), 3), wall_ms_range=[round(float(t.min()), 3), round(float(t.max()), 3)],
                              trace_ms_median=round(float(np.median(d)), 3), trace_ms_range=[round(float(d.min()), 3), round(float(d.max()), 3)])))
    if "map" in times and "constant" in times:
        print(json.dumps(dict(label=args.label, map_over_constant_wall=round(float(np.median(times["map"]) / np.median(times["constant"])), 4),
                              map_over_constant_trace=round(float(np.median(dev["map"]) / np.median(dev["constant"])), 4))))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Sample rate of the Cornell box (36 triangles, LDS-resident) in the RGB or the spectral variant: bench.py's headline film, timed the same
way (unprofiled renders between device synchronisations), for the variant bench.py does not time on this scene.  One JSON line with the
median and the range over the rounds; compare lines of one job only."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mitsuba2_amd import render, scenes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="spectral", choices=["rgb", "spectral"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    args = ap.parse_args()
    scene = render.Scene(scenes.cornell_box(), variant=args.variant)
    sensor = render.make_sensor(scenes.cornell_box_sensor(args.res, args.res, args.spp))
    integ = render.PathIntegrator()
    rates = []
    for r in range(args.warmup + args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert integ.render(scene, sensor)
        torch.cuda.synchronize()
        if r >= args.warmup:
            rates.append(integ.stats["samples"] / (time.perf_counter() - t0) * 1e-6)
    a = np.array(rates)
    print(json.dumps(dict(scene="cbox", variant=args.variant, film=[args.res, args.res, args.spp], rounds=args.rounds,
                          msample_per_s_median=round(float(np.median(a)), 1), msample_per_s_range=[round(float(a.min()), 1), round(float(a.max()), 1)])))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of tabulated spectra in the render kernels: the spectral mesh configuration (261 k-triangle displaced sphere, 1920 x 1080) with a
`roughconductor` object, rendered twice on the same build -- with uniform eta / k (k_shade<PathStateS, general>), and with 56-node
irregular eta / k tables (k_shade<PathStateT, general>, which evaluates the spectrum pool: a binary search and one interpolation per
wavelength and parameter).  The two variants are run in turn, round after round, so that drift of the device hits them alike; printed are
the median and range of the sample rate and the per-launch device time of the k_shade instantiation each variant uses.  The renders run
with profile=True (HIP events around every trace / shade launch, which is where the per-launch time comes from): the two rates compare
with each other, not with bench.py's, which times unprofiled renders at 1024 spp."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mitsuba2_amd import render, scenes

ETA, K = 0.2, 3.9


def table(mean, n=56, seed=0):
    """an irregular table of n nodes with unequal gaps over 360..830 nm whose values wobble around `mean`"""
    rng = np.random.default_rng(seed)
    nodes = np.cumsum(rng.uniform(0.5, 1.5, n))
    nodes = 360.0 + (nodes - nodes[0]) * (470.0 / (nodes[-1] - nodes[0]))
    return {"type": "irregular", "wavelengths": nodes.astype(np.float32), "values": (mean * (1.0 + 0.2 * np.sin(nodes / 40.0))).astype(np.float32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--scale", type=float, default=1.0, help="scales the film size (quick runs)")
    args = ap.parse_args()
    w, h = int(1920 * args.scale), int(1080 * args.scale)
    sp = scenes.bumpy_sphere_sensor(w, h, args.spp)
    variants = []
    for name, eta, k in (("uniform eta / k", ETA, K), ("56-node irregular eta / k", table(ETA, seed=1), table(K, seed=2))):
        sd = scenes.bumpy_sphere(256, 512)
        sd["bsdfs"] = [{"type": "roughconductor", "alpha": 0.2, "distribution": "ggx", "eta": eta, "k": k}] + list(sd["bsdfs"][1:])
        variants.append((name, render.Scene(sd, variant="spectral"), render.make_sensor(sp), render.PathIntegrator(profile=True)))
    rate = {v[0]: [] for v in variants}
    shade = {v[0]: [] for v in variants}
    for r in range(args.warmup + args.rounds):
        for name, scene, sensor, integ in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert integ.render(scene, sensor)
            torch.cuda.synchronize()
            if r >= args.warmup:
                rate[name].append(integ.stats["samples"] / (time.perf_counter() - t0) * 1e-6)
                shade[name].append(integ.stats["shade_ns"] / max(integ.stats["shade_launches"], 1) * 1e-3)
    for name, scene, _, _ in variants:
        a, b = np.array(rate[name]), np.array(shade[name])
        print(json.dumps(dict(variant=name, spectra=scene._n_spectra, film=[w, h, args.spp], rounds=args.rounds,
                              msample_per_s_median=round(float(np.median(a)), 3), msample_per_s_range=[round(float(a.min()), 3), round(float(a.max()), 3)],
                              k_shade_us_per_launch_median=round(float(np.median(b)), 2),
                              k_shade_us_per_launch_range=[round(float(b.min()), 2), round(float(b.max()), 2)])))


if __name__ == "__main__":
    main()

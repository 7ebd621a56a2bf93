#!/usr/bin/env python3
"""Cost of one replay of mtsamd_render_adjoint_param_textures per parameter slot, on the Cornell box at 256 x 256 x 16 spp with 64 x 64
maps on the tall box, beside mtsamd_render_adjoint_textures on the same box with a 64 x 64 diffuse reflectance map:

* `diffuse_texels`           tall box = diffuse, reflectance bitmap: mtsamd_render_adjoint_textures (k_adjoint_tex).  This figure exists on
                             the parent commit too: run the script there with --baseline-only to compare the two builds;
* `alpha`                    roughconductor, one map behind alpha_u and alpha_v: param = ALPHA (one launch: the pair is alpha_u's);
* `alpha_u`, `alpha_v`       roughconductor with a map of its own on each roughness (and one on specular_reflectance): one slot each;
* `specular_reflectance`     that roughconductor's colour map; `conductor_reflectance`: the same slot on a smooth conductor (discrete lobe);
* `specular_transmittance`   dielectric with maps on both colours: the transmittance slot; `glass_reflectance`: its reflectance slot.

The variants run in turn, round after round; after --warmup rounds the median and the range of --rounds synchronised wall-clock times
are printed, one JSON line each.  No threshold: this is a first measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mitsuba2_amd import _lib as L, autodiff, render, scenes

IOR = {"eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14]}
ALPHA, ALPHA_U, ALPHA_V, SPEC, TRANS = 4, 6, 7, 1, 5


def bitmap(lo, hi, seed):
    return {"type": "bitmap", "data": np.random.RandomState(seed).uniform(lo, hi, size=(64, 64, 3)).astype(np.float32)}


def box_scene(material):
    cb = scenes.cornell_box()
    tall = len(cb["meshes"]) - 1
    uv = np.tile(np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32), (6, 1))
    cb["bsdfs"] = list(cb["bsdfs"]) + [material]
    cb["meshes"][tall] = dict(cb["meshes"][tall], bsdf=len(cb["bsdfs"]) - 1, texcoords=uv)
    return cb


def variants(baseline_only):
    out = [("diffuse_texels", {"type": "diffuse", "reflectance": bitmap(0.2, 0.8, 1)}, None)]
    if baseline_only:
        return out
    rough = dict(type="roughconductor", distribution="ggx", **IOR)
    aniso = dict(rough, alpha_u=bitmap(0.1, 0.4, 2), alpha_v=bitmap(0.1, 0.4, 3), specular_reflectance=bitmap(0.5, 1.0, 4))
    glass = dict(type="dielectric", int_ior="bk7", specular_reflectance=bitmap(0.5, 1.0, 5), specular_transmittance=bitmap(0.5, 1.0, 6))
    return out + [("alpha", dict(rough, alpha=bitmap(0.1, 0.4, 2)), ALPHA), ("alpha_u", aniso, ALPHA_U), ("alpha_v", aniso, ALPHA_V),
                  ("specular_reflectance", aniso, SPEC),
                  ("conductor_reflectance", dict(type="conductor", specular_reflectance=bitmap(0.5, 1.0, 4), **IOR), SPEC),
                  ("specular_transmittance", glass, TRANS), ("glass_reflectance", glass, SPEC)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--label", default="")
    ap.add_argument("--baseline-only", action="store_true", help="mtsamd_render_adjoint_textures alone (a build without the new entry point)")
    args = ap.parse_args()
    p = scenes.cornell_box_sensor(args.size, args.size, args.spp, seed=3, max_depth=args.max_depth)
    dimage = torch.from_numpy(np.random.RandomState(0).uniform(-1, 1, (args.size, args.size, 3)).astype(np.float32)).cuda()
    runs = []
    for name, material, param in variants(args.baseline_only):
        sensor = render.make_sensor(p)
        integ = render.PathIntegrator(max_depth=args.max_depth)
        scene = render.Scene(box_scene(material), sensor=sensor, integrator=integ)
        d = autodiff._desc(scene, sensor, integ, None, p["seed"])
        film = autodiff._render_film(scene, d)
        g = torch.zeros(max(sum(h * w * 3 for (h, w, _) in scene._texture_shapes), 1), device="cuda")
        args_ = (scene._handle, C.byref(d), C.c_void_p(dimage.data_ptr()), C.c_void_p(film.data_ptr()))
        if param is None:
            call = lambda a=args_, g=g: L.check(L.lib().mtsamd_render_adjoint_textures(*a, C.c_void_p(g.data_ptr()), None))
        else:
            call = lambda a=args_, g=g, q=param: L.check(L.lib().mtsamd_render_adjoint_param_textures(*a, q, 0.0, C.c_void_p(g.data_ptr()), None))
        runs.append((name, call, (scene, d, film, g)))
    times = {name: [] for name, _, _ in runs}
    for r in range(args.warmup + args.rounds):
        for name, call, _ in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    for name, _, keep in runs:
        t = np.array(times[name])
        print(json.dumps(dict(label=args.label, variant=name, film="%dx%dx%d" % (args.size, args.size, args.spp), max_depth=args.max_depth,
                              rounds=args.rounds, ms_median=round(float(np.median(t)), 4), ms_range=[round(float(t.min()), 4), round(float(t.max()), 4)],
                              grad_abs_sum=float(keep[3].abs().sum().item()))))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the forward-mode derivative render (mtsamd_render_forward) beside what it replaces.  Per scene -- the Cornell box with a
roughconductor and a plastic box at 256 x 256 x 16 spp, and scenes.matpreview() -- and per K in 1, 4, 16 (as many constant BSDF scalars as
the scene has):

* `primal`    one mtsamd_render(film_rgb = 1) of the same descriptor;
* `forward`   ONE mtsamd_render_forward with a tangent of 1 on K scalars;
* `adjoint`   K calls of mtsamd_render_adjoint_param, one per scalar (what autodiff.render's backward pass pays for them).

The three are run in turn, round after round, so that drift of the device hits them alike; after `--warmup` rounds the median and the
range of `--rounds` synchronised wall-clock times are printed, one JSON line per (scene, K)."""
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

ROUGH = {"type": "roughconductor", "alpha": 0.3, "distribution": "ggx", "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14], "specular_reflectance": [0.9, 0.8, 0.7]}
PLASTIC = {"type": "plastic", "diffuse_reflectance": [0.2, 0.5, 0.3], "int_ior": 1.6}


def build(which, size, spp):
    if which == "cbox":
        sd = scenes.cornell_box()
        sd["bsdfs"] = list(sd["bsdfs"]) + [dict(ROUGH, id="tall"), dict(PLASTIC, id="small")]
        sd["meshes"][6] = dict(sd["meshes"][6], bsdf=len(sd["bsdfs"]) - 2)
        sd["meshes"][7] = dict(sd["meshes"][7], bsdf=len(sd["bsdfs"]) - 1)
        p = scenes.cornell_box_sensor(size, size, spp, seed=1, max_depth=8)
    else:
        sd = scenes.matpreview()
        p = scenes.bumpy_sphere_sensor(size, size * 3 // 4, spp, seed=1, max_depth=8)
    sensor = render.make_sensor(p)
    return render.Scene(sd, sensor=sensor, integrator=render.PathIntegrator(max_depth=8)), sensor, p


def scalars(scene):
    """(record, mtsamd_bsdf_param, component) of every constant BSDF scalar traverse() names"""
    params = autodiff.traverse(scene)
    out = []
    for k, v in params.items():
        kind, idx, extra = params._kind[k]
        if kind in ("bsdf", "bsdf_param"):
            out += [(idx, 0 if kind == "bsdf" else int(extra), c) for c in range(v.numel())]
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--scenes", default="cbox,matpreview")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    lib = L.lib()
    for which in args.scenes.split(","):
        scene, sensor, p = build(which, args.size, args.spp)
        d = autodiff._desc(scene, sensor, scene.integrator(), None, p["seed"])
        every = scalars(scene)
        n_records = len(scene._bsdf_records)
        film = autodiff._render_film(scene, d)
        dimage = torch.rand((d.crop_height, d.crop_width, 3), device="cuda")
        out = torch.zeros_like(film)
        g = torch.zeros(1, device="cuda")
        ptr = lambda t: C.c_void_p(t.data_ptr())
        for K in (1, 4, 16):
            chosen = every[:: max(len(every) // K, 1)][:K]
            tangent = np.zeros((n_records, L.BSDF_TANGENT_FLOATS), np.float32)
            for (b, kind, comp) in chosen:
                tangent[b, 3 * kind + comp] = 1.0
            td = L.TangentDesc()
            td.bsdf_tangents = tangent.ctypes.data_as(L.f32p)
            td.flags = L.FORWARD_DETACH_ROULETTE

            def primal():
                L.check(lib.mtsamd_render(scene._handle, C.byref(d), ptr(out), None, None))

            def forward():
                L.check(lib.mtsamd_render_forward(scene._handle, C.byref(d), C.byref(td), ptr(out), None))

            def adjoint():
                for (b, kind, comp) in chosen:
                    L.check(lib.mtsamd_render_adjoint_param(scene._handle, C.byref(d), ptr(dimage), ptr(film), b, kind, comp, 0.0, ptr(g), None))

            runs = {"primal": primal, "forward": forward, "adjoint": adjoint}
            times = {k: [] for k in runs}
            for r in range(args.warmup + args.rounds):
                for k, fn in runs.items():
                    t = timed(fn)
                    if r >= args.warmup:
                        times[k].append(t)
            row = dict(label=args.label, scene=which, film="%dx%dx%d" % (d.crop_width, d.crop_height, d.sample_count), K=len(chosen), rounds=args.rounds)
            for k, t in times.items():
                t = np.array(t)
                row[k + "_ms_median"] = round(float(np.median(t)), 3)
                row[k + "_ms_range"] = [round(float(t.min()), 3), round(float(t.max()), 3)]
            row["forward_over_primal"] = round(row["forward_ms_median"] / row["primal_ms_median"], 3)
            row["adjoint_over_forward"] = round(row["adjoint_ms_median"] / row["forward_ms_median"], 3)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

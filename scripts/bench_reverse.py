#!/usr/bin/env python3
"""Cost of the reverse-mode render (mtsamd_render_reverse) beside what it replaces, on the two scenes of bench_forward.py -- the Cornell
box with a roughconductor and a plastic box at 256 x 256 x 16 spp, and scenes.matpreview() at 256 x 192 x 16 spp -- per K in 1, 4, 16 (as
many constant BSDF scalars as the scene has):

* `primal`    one mtsamd_render(film_rgb = 1) of the same descriptor;
* `fused`     ONE mtsamd_render_reverse with K wanted scalars and MTSAMD_REVERSE_DETACH_ROULETTE, so that it computes what ...
* `adjoint`   ... the K calls of mtsamd_render_adjoint_param compute, one per scalar (autodiff.render's default backward pass).

The three are run in turn, round after round, so that drift of the device hits them alike; after `--warmup` rounds the median and the
range of `--rounds` synchronised wall-clock times are printed, one JSON line per (scene, K), with the largest deviation between the two
gradients relative to the largest entry."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_forward import build, scalars, timed
from mitsuba2_amd import _lib as L, autodiff


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
        ptr = lambda t: C.c_void_p(t.data_ptr())
        for K in (1, 4, 16):
            chosen = every[:: max(len(every) // K, 1)][:K]
            wanted = np.zeros((n_records, L.BSDF_TANGENT_FLOATS), np.uint8)
            for (b, kind, comp) in chosen:
                wanted[b, 3 * kind + comp] = 1
            g_fused = torch.zeros((n_records, L.BSDF_TANGENT_FLOATS), device="cuda")
            g_adjoint = torch.zeros(len(chosen), device="cuda")
            gd = L.GradientDesc()
            gd.bsdf_wanted = wanted.ctypes.data_as(C.POINTER(C.c_uint8))
            gd.grad_bsdf_dev = g_fused.data_ptr()
            gd.flags = L.REVERSE_DETACH_ROULETTE

            def primal():
                L.check(lib.mtsamd_render(scene._handle, C.byref(d), ptr(out), None, None))

            def fused():
                g_fused.zero_()
                L.check(lib.mtsamd_render_reverse(scene._handle, C.byref(d), ptr(dimage), ptr(film), C.byref(gd), None))

            def adjoint():
                g_adjoint.zero_()
                for i, (b, kind, comp) in enumerate(chosen):
                    L.check(lib.mtsamd_render_adjoint_param(scene._handle, C.byref(d), ptr(dimage), ptr(film), b, kind, comp, 0.0, ptr(g_adjoint[i:i + 1]), None))

            runs = {"primal": primal, "fused": fused, "adjoint": adjoint}
            times = {k: [] for k in runs}
            for r in range(args.warmup + args.rounds):
                for k, fn in runs.items():
                    t = timed(fn)
                    if r >= args.warmup:
                        times[k].append(t)
            a = g_adjoint.cpu().numpy().astype(np.float64)
            f = np.array([g_fused[b, 3 * kind + comp].item() for (b, kind, comp) in chosen], np.float64)
            row = dict(label=args.label, scene=which, film="%dx%dx%d" % (d.crop_width, d.crop_height, d.sample_count), K=len(chosen), rounds=args.rounds)
            for k, t in times.items():
                t = np.array(t)
                row[k + "_ms_median"] = round(float(np.median(t)), 3)
                row[k + "_ms_range"] = [round(float(t.min()), 3), round(float(t.max()), 3)]
            row["fused_over_primal"] = round(row["fused_ms_median"] / row["primal_ms_median"], 3)
            row["adjoint_over_fused"] = round(row["adjoint_ms_median"] / row["fused_ms_median"], 3)
            row["largest_deviation_over_largest_entry"] = float(np.abs(f - a).max() / max(np.abs(a).max(), 1e-30))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

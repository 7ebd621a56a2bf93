#!/usr/bin/env python3
"""Cost of the forward and reverse renders in scenes with textured BSDF parameters (MTSAMD_FORWARD_PARAM_TEXTURES /
MTSAMD_REVERSE_PARAM_TEXTURES) beside what they stand next to.  Two scenes: the Cornell box whose tall box is a roughconductor with an
`alpha` map and a `specular_reflectance` map (16 x 16 random texels, random texcoords) at 256 x 256 x 16 spp, and scenes.matpreview()
with the same material on the sphere at 256 x 192 x 16 spp; max_depth 8, Russian roulette detached on both sides.

* `primal`    one mtsamd_render(film_rgb = 1) of the same descriptor;
* `forward`   one mtsamd_render_forward with a tangent on the texels of both maps;
* `fused`     ONE mtsamd_render_reverse with the bit: both maps' texels and K = 0 / 4 further constants (eta / k of the mapped record
              and the colours of other records), beside
* `replays`   the two slot replays of mtsamd_render_adjoint_param_textures it replaces (alpha, specular_reflectance; the K constants
              are not in them: they have no gradient in such a scene without the bit).

The four are run in turn, round after round, so that drift of the device hits them alike; after `--warmup` rounds the median and the
range of `--rounds` synchronised wall-clock times are printed, one JSON line per (scene, K), with the largest deviation between the two
texel gradients relative to the largest entry."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_forward import scalars, timed
from mitsuba2_amd import _lib as L, autodiff, render, scenes

F32 = np.float32


def build(which, size, spp):
    rng = np.random.RandomState(1)
    mat = dict(type="roughconductor", distribution="ggx", id="mapped", eta=[0.2, 0.92, 1.1], k=[3.9, 2.45, 2.14],
               alpha={"type": "bitmap", "data": rng.uniform(0.1, 0.4, (16, 16, 3)).astype(F32)},
               specular_reflectance={"type": "bitmap", "data": rng.uniform(0.3, 0.9, (16, 16, 3)).astype(F32)})
    if which == "cbox":
        sd = scenes.cornell_box()
        sd["bsdfs"] = list(sd["bsdfs"]) + [mat]
        sd["meshes"][7] = dict(sd["meshes"][7], bsdf=len(sd["bsdfs"]) - 1, texcoords=rng.uniform(0, 1, size=(24, 2)).astype(F32))
        p = scenes.cornell_box_sensor(size, size, spp, seed=1, max_depth=8)
        mapped = len(sd["bsdfs"]) - 1
    else:
        sd = scenes.matpreview()
        sd["bsdfs"][0] = mat
        sd["meshes"][0] = dict(sd["meshes"][0], texcoords=rng.uniform(0, 1, size=(sd["meshes"][0]["positions"].shape[0], 2)).astype(F32))
        p = scenes.bumpy_sphere_sensor(size, size * 3 // 4, spp, seed=1, max_depth=8)
        mapped = 0
    sensor = render.make_sensor(p)
    return render.Scene(sd, sensor=sensor, integrator=render.PathIntegrator(max_depth=8)), sensor, p, mapped


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
        scene, sensor, p, mapped = build(which, args.size, args.spp)
        d = autodiff._desc(scene, sensor, scene.integrator(), None, p["seed"])
        n_records = len(scene._bsdf_records)
        n_tex = max(sum(h * w * 3 for (h, w, _) in scene._texture_shapes), 1)
        film = autodiff._render_film(scene, d)
        dimage = torch.rand((d.crop_height, d.crop_width, 3), device="cuda")
        out = torch.zeros_like(film)
        dfilm = torch.zeros_like(film)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        t_tex = torch.rand(n_tex, device="cuda")
        td = L.TangentDesc()
        td.texture_tangents_dev = t_tex.data_ptr()
        td.h, td.flags = 0.01, L.FORWARD_DETACH_ROULETTE | L.FORWARD_PARAM_TEXTURES
        others = [s for s in scalars(scene) if s[0] != mapped]
        for K in (0, 4):
            chosen = ([(mapped, 2, 0), (mapped, 3, 1)] + others[:2])[:K]          # eta.r and k.g of the mapped record, two colours elsewhere
            wanted = np.zeros((n_records, L.BSDF_TANGENT_FLOATS), np.uint8)
            for (b, kind, comp) in chosen:
                wanted[b, 3 * kind + comp] = 1
            g_bsdf = torch.zeros((n_records, L.BSDF_TANGENT_FLOATS), device="cuda")
            g_fused, g_replays = torch.zeros(n_tex, device="cuda"), torch.zeros(n_tex, device="cuda")
            gd = L.GradientDesc()
            if chosen:
                gd.bsdf_wanted = wanted.ctypes.data_as(C.POINTER(C.c_uint8))
                gd.grad_bsdf_dev = g_bsdf.data_ptr()
            gd.grad_textures_dev = g_fused.data_ptr()
            gd.h, gd.flags = 0.01, L.REVERSE_DETACH_ROULETTE | L.REVERSE_PARAM_TEXTURES

            def primal():
                L.check(lib.mtsamd_render(scene._handle, C.byref(d), ptr(out), None, None))

            def forward():
                L.check(lib.mtsamd_render_forward(scene._handle, C.byref(d), C.byref(td), ptr(dfilm), None))

            def fused():
                g_fused.zero_(); g_bsdf.zero_()
                L.check(lib.mtsamd_render_reverse(scene._handle, C.byref(d), ptr(dimage), ptr(film), C.byref(gd), None))

            def replays():
                g_replays.zero_()
                for param in (4, 1):          # MTSAMD_PARAM_ALPHA (its alpha_u launch; the alpha_v slot launches nothing), SPECULAR_REFLECTANCE
                    L.check(lib.mtsamd_render_adjoint_param_textures(scene._handle, C.byref(d), ptr(dimage), ptr(film), param, 0.01, ptr(g_replays), None))

            runs = {"primal": primal, "forward": forward, "fused": fused, "replays": replays}
            times = {k: [] for k in runs}
            for r in range(args.warmup + args.rounds):
                for k, fn in runs.items():
                    t = timed(fn)
                    if r >= args.warmup:
                        times[k].append(t)
            a, f = g_replays.cpu().numpy().astype(np.float64), g_fused.cpu().numpy().astype(np.float64)
            row = dict(label=args.label, scene=which, film="%dx%dx%d" % (d.crop_width, d.crop_height, d.sample_count), K=len(chosen), rounds=args.rounds)
            for k, t in times.items():
                t = np.array(t)
                row[k + "_ms_median"] = round(float(np.median(t)), 3)
                row[k + "_ms_range"] = [round(float(t.min()), 3), round(float(t.max()), 3)]
            row["forward_over_primal"] = round(row["forward_ms_median"] / row["primal_ms_median"], 3)
            row["replays_over_fused"] = round(row["replays_ms_median"] / row["fused_ms_median"], 3)
            row["largest_deviation_over_largest_entry"] = float(np.abs(f - a).max() / max(np.abs(a).max(), 1e-30))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the forward and reverse renders in scenes with blendbsdf / mask records (MTSAMD_FORWARD_NESTED / MTSAMD_REVERSE_NESTED) beside
the primal render of the same descriptor.  Two scenes: the Cornell box with a blend wall (the right wall: roughconductor + diffuse,
weight 0.3) and a masked tall box (a 16 x 16 opacity map over a plastic, random texcoords) at 256 x 256 x 16 spp, and scenes.matpreview()
with a blended material on the sphere (roughconductor + plastic, weight 0.4) at 256 x 192 x 16 spp; max_depth 8, Russian roulette
detached.

* `primal`    one mtsamd_render(film_rgb = 1);
* `forward`   one mtsamd_render_forward with a tangent on every weight, on the roughness of the roughconductor child and, where there is
              one, on the texels of the opacity map;
* `reverse`   ONE mtsamd_render_reverse for the same parameters: the weights, that roughness, the texels.

The three are run in turn, round after round, so that drift of the device hits them alike; after `--warmup` rounds the median and the
range of `--rounds` synchronised wall-clock times are printed, one JSON line per scene, with <dimage, J t> of the forward render beside
<J^T dimage, t> of the reverse render.  Nothing is asserted on the times."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_forward import timed
from mitsuba2_amd import _lib as L, autodiff, bsdfs as B, render, scenes

F32 = np.float32
ROUGH = dict(type="roughconductor", distribution="ggx", alpha=0.25, eta=[0.2, 0.92, 1.1], k=[3.9, 2.45, 2.14])


def build(which, size, spp):
    rng = np.random.RandomState(1)
    if which == "cbox":
        sd = scenes.cornell_box()
        n = len(sd["bsdfs"])
        sd["bsdfs"] = list(sd["bsdfs"]) + [
            dict(type="blendbsdf", id="wall", weight=0.3, bsdf_0=ROUGH, bsdf_1=dict(type="diffuse", reflectance=[0.14, 0.45, 0.091])),
            dict(type="mask", id="box", opacity={"type": "bitmap", "data": rng.uniform(0.3, 0.9, (16, 16, 3)).astype(F32)},
                 nested=dict(type="plastic", diffuse_reflectance=[0.2, 0.5, 0.3], int_ior=1.6))]
        sd["meshes"][3] = dict(sd["meshes"][3], bsdf=n)
        sd["meshes"][7] = dict(sd["meshes"][7], bsdf=n + 1, texcoords=rng.uniform(0, 1, size=(24, 2)).astype(F32))
        p = scenes.cornell_box_sensor(size, size, spp, seed=1, max_depth=8)
    else:
        sd = scenes.matpreview()
        sd["bsdfs"][0] = dict(type="blendbsdf", id="blended", weight=0.4, bsdf_0=ROUGH, bsdf_1=dict(type="plastic", diffuse_reflectance=[0.2, 0.5, 0.3], int_ior=1.6))
        p = scenes.bumpy_sphere_sensor(size, size * 3 // 4, spp, seed=1, max_depth=8)
    sensor = render.make_sensor(p)
    return render.Scene(sd, sensor=sensor, integrator=render.PathIntegrator(max_depth=8)), sensor, p


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
        flat = B.flatten(scene._bsdf_records)
        n_tex = max(sum(h * w * 3 for (h, w, _) in scene._texture_shapes), 1)
        has_tex = any(h * w for (h, w, _) in scene._texture_shapes)
        film = autodiff._render_film(scene, d)
        dimage = torch.rand((d.crop_height, d.crop_width, 3), device="cuda")
        out, dfilm = torch.zeros_like(film), torch.zeros_like(film)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        # the weights that are constants, and the roughness of every roughconductor child
        entries = [(b, 0) for b, r in enumerate(flat) if r["type"] in (B.BLEND, B.MASK) and not isinstance(r["reflectance"], dict)] + \
                  [(b, 3 * 4) for b, r in enumerate(flat) if r["type"] == B.ROUGHCONDUCTOR]
        t_bsdf = np.zeros((len(flat), L.BSDF_TANGENT_FLOATS), F32)
        wanted = np.zeros((len(flat), L.BSDF_TANGENT_FLOATS), np.uint8)
        for (b, i) in entries:
            t_bsdf[b, i], wanted[b, i] = 1.0, 1
        t_tex = torch.rand(n_tex, device="cuda")
        td = L.TangentDesc()
        td.bsdf_tangents = t_bsdf.ctypes.data_as(L.f32p)
        if has_tex:
            td.texture_tangents_dev = t_tex.data_ptr()
        td.h, td.flags = 0.01, L.FORWARD_DETACH_ROULETTE | L.FORWARD_NESTED
        g_bsdf = torch.zeros((len(flat), L.BSDF_TANGENT_FLOATS), device="cuda")
        g_tex = torch.zeros(n_tex, device="cuda")
        gd = L.GradientDesc()
        gd.bsdf_wanted = wanted.ctypes.data_as(C.POINTER(C.c_uint8))
        gd.grad_bsdf_dev = g_bsdf.data_ptr()
        if has_tex:
            gd.grad_textures_dev = g_tex.data_ptr()
        gd.h, gd.flags = 0.01, L.REVERSE_DETACH_ROULETTE | L.REVERSE_NESTED

        def primal():
            L.check(lib.mtsamd_render(scene._handle, C.byref(d), ptr(out), None, None))

        def forward():
            dfilm.zero_()
            L.check(lib.mtsamd_render_forward(scene._handle, C.byref(d), C.byref(td), ptr(dfilm), None))

        def reverse():
            g_bsdf.zero_(); g_tex.zero_()
            L.check(lib.mtsamd_render_reverse(scene._handle, C.byref(d), ptr(dimage), ptr(film), C.byref(gd), None))

        runs = {"primal": primal, "forward": forward, "reverse": reverse}
        times = {k: [] for k in runs}
        for r in range(args.warmup + args.rounds):
            for k, fn in runs.items():
                t = timed(fn)
                if r >= args.warmup:
                    times[k].append(t)
        image = (dfilm[..., :3] / (dfilm[..., 4:5] + 1e-8)).double()
        fwd = float((image * dimage.double()).sum().item())
        rev = float((g_bsdf.double().cpu().numpy() * t_bsdf).sum() + (float((g_tex.double() * t_tex.double()).sum().item()) if has_tex else 0.0))
        row = dict(label=args.label, scene=which, film="%dx%dx%d" % (d.crop_width, d.crop_height, d.sample_count), scalars=len(entries),
                   texels=n_tex if has_tex else 0, rounds=args.rounds)
        for k, t in times.items():
            t = np.array(t)
            row[k + "_ms_median"] = round(float(np.median(t)), 3)
            row[k + "_ms_range"] = [round(float(t.min()), 3), round(float(t.max()), 3)]
        row["forward_over_primal"] = round(row["forward_ms_median"] / row["primal_ms_median"], 3)
        row["reverse_over_primal"] = round(row["reverse_ms_median"] / row["primal_ms_median"], 3)
        row["forward_dot"], row["reverse_dot"] = fwd, rev
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""SHA-256 digests of the forward films and reverse gradients of scenes with textured BSDF parameters and no nested record
(MTSAMD_FORWARD_PARAM_TEXTURES / MTSAMD_REVERSE_PARAM_TEXTURES), to show that a change leaves their bits alone: run it with the library
of the parent commit and with the library of the change (`--lib`), and compare the lines.

Scenes: the Cornell box whose tall box is a roughconductor with an `alpha` map and a `specular_reflectance` map (flat scene), 32 x 24 x 8
spp, and the 261 k-triangle scenes.matpreview() with that material (hierarchy scene), 32 x 24 x 4 spp; max_depth 7, rr_depth 2, roulette
attached and detached.  Digested: the forward film of a random tangent over both maps, eta / k and the lamp; the BSDF, emitter and texel
gradients of one reverse call (RECORD = true); the emitter gradient of a reverse call that wants nothing else (RECORD = false).  The
reverse gradients are sums of float atomics, whose order is not fixed: a digest that differs between two runs of ONE library says so
(`--repeat`), and then the largest difference is what to compare."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mitsuba2_amd import _lib as L

F32 = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="path of the libmtsamd.so to load instead of the built one")
    ap.add_argument("--label", default="")
    ap.add_argument("--repeat", type=int, default=2)
    args = ap.parse_args()
    if args.lib:
        L.LIB_PATH = os.path.abspath(args.lib)
    from bench_fused_param_maps import build
    from mitsuba2_amd import autodiff
    lib = L.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    sha = lambda t: hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()[:16]
    for which, size, spp in (("cbox", 32, 8), ("matpreview", 32, 4)):
        scene, sensor, p, mapped = build(which, size, spp)
        d = autodiff._desc(scene, sensor, scene.integrator(), None, p["seed"])
        d.max_depth, d.rr_depth = 7, 2
        n_records = len(scene._bsdf_records)
        n_tex = max(sum(h * w * 3 for (h, w, _) in scene._texture_shapes), 1)
        n_em = max(len(scene._dict.get("emitters", [])), 1)
        film = autodiff._render_film(scene, d)
        rng = np.random.RandomState(5)
        dimage = torch.from_numpy(rng.uniform(-1, 1, (d.crop_height, d.crop_width, 3)).astype(F32)).cuda()
        t_tex = torch.from_numpy(rng.uniform(-1, 1, n_tex).astype(F32)).cuda()
        t_bsdf = np.zeros((n_records, L.BSDF_TANGENT_FLOATS), F32)
        t_bsdf[mapped, 6:12] = rng.uniform(0.5, 1.0, 6)
        t_em = rng.uniform(0.5, 2.0, (n_em, 3)).astype(F32)
        wanted = (t_bsdf != 0).astype(np.uint8)
        for detach in (0, 1):
            for rep in range(args.repeat):
                td = L.TangentDesc()
                td.bsdf_tangents, td.emitter_tangents = t_bsdf.ctypes.data_as(L.f32p), t_em.ctypes.data_as(L.f32p)
                td.texture_tangents_dev = t_tex.data_ptr()
                td.h, td.flags = 0.01, detach | L.FORWARD_PARAM_TEXTURES
                dfilm = torch.zeros_like(film)
                L.check(lib.mtsamd_render_forward(scene._handle, C.byref(d), C.byref(td), ptr(dfilm), None))
                g_bsdf, g_em, g_tex = torch.zeros((n_records, 18), device="cuda"), torch.zeros((n_em, 3), device="cuda"), torch.zeros(n_tex, device="cuda")
                gd = L.GradientDesc()
                gd.bsdf_wanted, gd.grad_bsdf_dev = wanted.ctypes.data_as(C.POINTER(C.c_uint8)), g_bsdf.data_ptr()
                gd.grad_emitters_dev, gd.grad_textures_dev = g_em.data_ptr(), g_tex.data_ptr()
                gd.h, gd.flags = 0.01, detach | L.REVERSE_PARAM_TEXTURES
                L.check(lib.mtsamd_render_reverse(scene._handle, C.byref(d), ptr(dimage), ptr(film), C.byref(gd), None))
                g_only = torch.zeros((n_em, 3), device="cuda")
                go = L.GradientDesc()
                go.grad_emitters_dev, go.h, go.flags = g_only.data_ptr(), 0.01, detach | L.REVERSE_PARAM_TEXTURES
                L.check(lib.mtsamd_render_reverse(scene._handle, C.byref(d), ptr(dimage), ptr(film), C.byref(go), None))
                torch.cuda.synchronize()
                print(json.dumps(dict(label=args.label, scene=which, detach=detach, run=rep, primal=sha(film), forward=sha(dfilm), grad_bsdf=sha(g_bsdf),
                                      grad_emitters=sha(g_em), grad_textures=sha(g_tex), grad_emitters_alone=sha(g_only),
                                      sums=[float(dfilm.double().sum()), float(g_bsdf.double().sum()), float(g_em.double().sum()), float(g_tex.double().sum())])), flush=True)


if __name__ == "__main__":
    main()

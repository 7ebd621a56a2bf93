#!/usr/bin/env python3
"""BASELINE config 4: one inverse-rendering iteration on the Cornell box (primal render + derivative render + adjoint +
Adam step), the setup of docs/examples/10_inverse_rendering/invert_cbox.py: path max_depth=3, box filter, spp=1,
unbiased=True, image writing disabled.  The reference quotes ~50 ms (unbiased) / ~27 ms (biased) per iteration on a
Titan RTX (docs/src/inverse_rendering/diff_render.rst:311-314), film resolution not stated; 256x256 is used here."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mitsuba2_amd import render, scenes, autodiff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--texture", type=int, default=0, help="optimise a texture of this resolution on floor + back wall instead of the red wall colour")
    ap.add_argument("--general", action="store_true", help="general scene: textured roughplastic floor + back wall under an envmap "
                    "(texels through mtsamd_render_adjoint_textures); times one biased iteration and the adjoint kernel alone")
    ap.add_argument("--spectral-replay", action="store_true", help="spectral Cornell box: one backward pass for the red wall's constant "
                    "colour through the path replay (mtsamd_render_adjoint_spectral) and through central differences (six renders)")
    ap.add_argument("--spectral-emitters", action="store_true", help="spectral scenes under an envmap: HIP-event time of one emitter replay "
                    "(mtsamd_render_adjoint_spectral_emitters, envmap texels + radiances) next to the primal render of the same description")
    args = ap.parse_args()
    if args.spectral_emitters:
        return bench_spectral_emitters(args)
    if args.general:
        return bench_general(args)
    if args.spectral_replay:
        return bench_spectral_replay(args)
    tex = None
    if args.texture:
        tex = np.full((args.texture, args.texture, 3), 0.5, np.float32)
    sd = scenes.cornell_box(texture=tex)
    for b, n in zip(sd["bsdfs"], ["white", "red", "green", "light", "textured"]):
        b["id"] = n
    p = scenes.cornell_box_sensor(args.res, args.res, args.spp, max_depth=3, rfilter="box")
    scene = render.Scene(sd, sensor=render.make_sensor(p), integrator=render.PathIntegrator(max_depth=3))
    params = autodiff.traverse(scene)
    key = "textured.reflectance.data" if args.texture else "red.reflectance.value"
    params.keep([key])
    ref = params[key].clone()
    image_ref = autodiff.render(scene, spp=8).detach()
    params[key] = torch.full_like(ref, 0.9)
    params.update()
    for unbiased in (True, False):
        opt = autodiff.Adam(params, lr=0.2 if not args.texture else 0.02)
        for it in range(5):          # warm-up
            img = autodiff.render(scene, optimizer=opt, unbiased=unbiased, spp=args.spp)
            (((img - image_ref) ** 2).sum() / img.numel()).backward()
            opt.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(args.iters):
            img = autodiff.render(scene, optimizer=opt, unbiased=unbiased, spp=args.spp)
            (((img - image_ref) ** 2).sum() / img.numel()).backward()
            opt.step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.iters
        err = ((ref - params[key].detach()) ** 2).mean().item()
        print("cbox %dx%d spp=%d max_depth=3 box filter, %s, unbiased=%s: %.2f ms per iteration (fwd+adjoint+Adam), param mse %.3g"
              % (args.res, args.res, args.spp, key, unbiased, ms, err))


def bench_general(args):
    """Cornell box without ceiling and area light, the floor and back wall a textured roughplastic (--texture, default 16), a conductor
    tall box, an envmap sky: one biased iteration (primal + texel adjoint + Adam) and the texel adjoint alone"""
    import ctypes as C
    from mitsuba2_amd import _lib as L
    from mitsuba2_amd.render import _ptr, _stream
    n = args.texture or 16
    tex = np.full((n, n, 3), 0.5, np.float32)
    sd = scenes.cornell_box(texture=tex)
    sd["bsdfs"][4] = {"type": "roughplastic", "id": "textured", "alpha": 0.2, "distribution": "ggx", "diffuse_reflectance": {"type": "bitmap", "data": tex}}
    sd["bsdfs"] = list(sd["bsdfs"]) + [{"type": "conductor", "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14]}]
    sd["meshes"][7] = dict(sd["meshes"][7], bsdf=len(sd["bsdfs"]) - 1)
    sd["meshes"] = [m for i, m in enumerate(sd["meshes"]) if i not in (1, 5)]
    sky = np.random.RandomState(7).uniform(0.3, 1.2, size=(32, 64, 3)).astype(np.float32)
    sd["emitters"] = [{"type": "envmap", "data": sky, "scale": 0.8}]
    p = scenes.cornell_box_sensor(args.res, args.res, args.spp, max_depth=3, rfilter="box")
    scene = render.Scene(sd, sensor=render.make_sensor(p), integrator=render.PathIntegrator(max_depth=3))
    params = autodiff.traverse(scene)
    key = "textured.diffuse_reflectance.data"
    params.keep([key])
    image_ref = autodiff.render(scene, spp=8).detach()
    params[key] = torch.full_like(params[key], 0.8)
    params.update()
    opt = autodiff.Adam(params, lr=0.02)

    def iteration():
        img = autodiff.render(scene, optimizer=opt, spp=args.spp)
        (((img - image_ref) ** 2).sum() / img.numel()).backward()
        opt.step()
    for it in range(5):
        iteration()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(args.iters):
        iteration()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.iters
    # the texel adjoint alone, for the film and dLoss/dImage of one render
    d = autodiff._desc(scene, scene.sensors()[0], scene.integrator(), args.spp, 1)
    film = autodiff._render_film(scene, d)
    dimage = torch.ones(args.res * args.res * 3, device="cuda")
    g = torch.zeros(n * n * 3, device="cuda")
    call = lambda: L.check(L.lib().mtsamd_render_adjoint_textures(scene._handle, C.byref(d), _ptr(dimage), _ptr(film), _ptr(g), _stream()))
    for it in range(3):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(args.iters):
        call()
    torch.cuda.synchronize()
    ms_adj = (time.perf_counter() - t0) * 1e3 / args.iters
    print("general scene %dx%d spp=%d max_depth=3: textured roughplastic (%dx%d) + conductor + envmap, %s, biased: %.2f ms per iteration "
          "(fwd+adjoint+Adam), texel adjoint alone %.2f ms" % (args.res, args.res, args.spp, n, n, key, ms, ms_adj))


def bench_spectral_replay(args):
    """One backward pass (no primal render, no optimiser step) of the spectral Cornell box for one constant colour, three components:
    the spectral path replay against the central-difference route (six renders), same scene, same spp, same dLoss/dImage"""
    sd = scenes.cornell_box()
    for b, n in zip(sd["bsdfs"], ["white", "red", "green", "light"]):
        b["id"] = n
    p = scenes.cornell_box_sensor(args.res, args.res, args.spp, max_depth=3, rfilter="box")
    scene = render.Scene(sd, variant="spectral", sensor=render.make_sensor(p), integrator=render.PathIntegrator(max_depth=3))
    dimage = torch.from_numpy(np.random.RandomState(1).randn(args.res * args.res * 3).astype(np.float32)).cuda()
    out = {}
    for replay in (True, False):
        params = autodiff.traverse(scene, replay=replay)
        params.keep(["red.reflectance.value"])
        params["red.reflectance.value"].requires_grad_(True)
        times = []
        for it in range(3 + args.iters):
            loss = (autodiff.render(scene, params=params, spp=args.spp) * dimage).sum()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss.backward()
            torch.cuda.synchronize()
            if it >= 3:          # three warm-up passes
                times.append((time.perf_counter() - t0) * 1e3)
        out[replay] = (float(np.median(times)), float(np.min(times)), float(np.max(times)), params["red.reflectance.value"].grad.cpu().numpy() / (3 + args.iters))
    for replay, name in ((True, "spectral path replay"), (False, "central differences (6 renders)")):
        ms, lo, hi, g = out[replay]
        print("spectral cbox %dx%d spp=%d max_depth=3 box filter, red.reflectance.value, backward pass through %s: median %.2f ms (min %.2f, max %.2f) over %d passes; "
              "mean gradient %s" % (args.res, args.res, args.spp, name, ms, lo, hi, args.iters, np.array2string(g, precision=4)))


def bench_spectral_emitters(args):
    """The emitter replay against the primal render of the same description, both timed with HIP events on the current stream: the open
    Cornell box (flat scene) with a roughplastic block under a 64 x 32 envmap and its area light, and the displaced sphere (hierarchy scene,
    256 x 512 segments as in the mesh benchmark) under the same map"""
    import ctypes as C
    from mitsuba2_amd import _lib as L
    from mitsuba2_amd.render import _ptr, _stream
    sky = np.random.RandomState(7).uniform(0.3, 1.2, size=(32, 64, 3)).astype(np.float32)
    env = {"type": "envmap", "id": "my_envmap", "data": sky, "scale": 0.8}
    cb = scenes.cornell_box()
    cb["meshes"] = [m for i, m in enumerate(cb["meshes"]) if i not in (1, 2)]
    cb["bsdfs"] = list(cb["bsdfs"]) + [{"type": "roughplastic", "alpha": 0.2, "distribution": "ggx", "diffuse_reflectance": [0.5, 0.35, 0.3]}]
    cb["meshes"][-2] = dict(cb["meshes"][-2], bsdf=len(cb["bsdfs"]) - 1)
    cb["emitters"] = list(cb["emitters"]) + [env]
    ball = scenes.bumpy_sphere(256, 512)
    ball["emitters"] = list(ball["emitters"]) + [env]
    for name, sd, p in (("open cbox + roughplastic block", cb, scenes.cornell_box_sensor(args.res, args.res, args.spp, max_depth=6, rfilter="box")),
                        ("bumpy_sphere(256, 512)", ball, dict(scenes.bumpy_sphere_sensor(96, 64, args.spp), max_depth=6))):
        sensor = render.make_sensor(p)
        scene = render.Scene(sd, variant="spectral", sensor=sensor, integrator=render.PathIntegrator(max_depth=6))
        d = autodiff._desc(scene, sensor, scene.integrator(), None, 1)
        film = autodiff._render_film(scene, d)
        dimage = torch.from_numpy(np.random.RandomState(1).randn(p["height"] * p["width"] * 3).astype(np.float32)).cuda()
        g_em = torch.zeros((len(sd["emitters"]), 3), device="cuda")
        g_env = torch.zeros(sky.shape, device="cuda")
        scratch = torch.zeros_like(film)
        calls = {"primal render": lambda: L.check(L.lib().mtsamd_render(scene._handle, C.byref(d), _ptr(scratch), None, _stream())),
                 "emitter replay": lambda: L.check(L.lib().mtsamd_render_adjoint_spectral_emitters(scene._handle, C.byref(d), _ptr(dimage), _ptr(film), _ptr(g_em), _ptr(g_env), _stream()))}
        for what, call in calls.items():
            times = []
            for it in range(3 + args.iters):
                scratch.zero_()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); call(); b.record()
                torch.cuda.synchronize()
                if it >= 3:
                    times.append(a.elapsed_time(b))
            print("spectral %s %dx%d spp=%d max_depth=6, 64x32 envmap + area light, %s: median %.3f ms (min %.3f, max %.3f) over %d runs"
                  % (name, p["width"], p["height"], args.spp, what, float(np.median(times)), float(np.min(times)), float(np.max(times)), args.iters))


if __name__ == "__main__":
    main()

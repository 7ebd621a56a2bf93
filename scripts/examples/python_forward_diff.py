#!/usr/bin/env python3
"""Forward-mode differentiation of a render: the scenario of docs/examples/10_inverse_rendering/forward_diff.py on the synthetic Cornell
box.  A tangent of [1, 1, 1] is put on the reflectance of the red wall and carried forward through the path tracer in one replay of the
camera samples (autodiff.render_forward, mtsamd_render_forward); the result is the image of d(image)/d(reflectance along the tangent),
written as an 8-bit PNG scaled to its largest value -- the wall itself lights up, and so does everything it bleeds colour onto.

    python scripts/examples/python_forward_diff.py --out cbox_forward_diff.png
    python scripts/examples/python_forward_diff.py --key lamp.emitter.radiance.value --emitters
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mitsuba2_amd import autodiff, bitmap, render as R, scenes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--key", default="red.reflectance.value", help="the parameter that carries the tangent (see --list)")
    ap.add_argument("--emitters", action="store_true", help="traverse(scene, emitters=True): emitter colours become parameters")
    ap.add_argument("--list", action="store_true", help="print the parameters and leave")
    ap.add_argument("--out", default="cbox_forward_diff.png")
    args = ap.parse_args()

    cb = scenes.cornell_box()
    for b, name in zip(cb["bsdfs"], ["white", "red", "green", "light"]):
        b["id"] = name
    cb["meshes"][5]["id"] = "lamp"
    sensor = R.make_sensor(scenes.cornell_box_sensor(args.res, args.res, spp=args.spp, seed=0, max_depth=args.max_depth))
    scene = R.Scene(cb, sensor=sensor, integrator=R.PathIntegrator(max_depth=args.max_depth))
    params = autodiff.traverse(scene, emitters=args.emitters)
    if args.list:
        for k, v in params.items():
            print("%-40s %s" % (k, tuple(v.shape)))
        return
    params.keep([args.key])

    # ek.set_gradient(param, [1, 1, 1]); ek.forward(param); ek.gradient(image)
    image_grad = autodiff.render_forward(scene, params, {args.key: torch.ones_like(params[args.key])}, spp=args.spp)
    grad = image_grad.reshape(args.res, args.res, 3).cpu().numpy()
    peak = float(np.abs(grad).max())
    print("d(image)/d(%s . [1, 1, 1]): min %.4g, max %.4g, mean %.4g" % (args.key, float(grad.min()), float(grad.max()), float(grad.mean())))
    bitmap.write_png(args.out, np.clip(np.abs(grad) / max(peak, 1e-30) * 255.0 + 0.5, 0, 255).astype(np.uint8))
    print("wrote", args.out)


if __name__ == "__main__":
    main()

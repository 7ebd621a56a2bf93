#!/usr/bin/env python3
"""One SHA-256 per raw film of a fixed list of small renders: every route through the film stage of mtsamd_render and mtsamd_render_aov
(api.cpp, FilmStage) -- one pass and several, the overlapped splat, the moment integrator's two films, a partitioned film, film_rgb, the
tiled and the gather kernels, the aov integrator with kept streams, splatted pass by pass and partitioned, a spectral mesh scene -- at the
sizes tests/test_gpu_lifecycle.py and tests/test_gpu_aov.py use.  The film kernels use no atomics, so a build that leaves the film stage
alone prints the same listing as its parent:

    python scripts/film_digest.py [--save films.npz] [--against films.npz]

--save keeps the films; --against compares with kept films instead of by digest: equal, or the largest difference and whether it is
within the tolerance of the lifecycle tests (rtol = atol = 2e-5), for a configuration whose digest does not reproduce."""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mitsuba2_amd import _lib as L, render as R, scenes

AOVS_NESTED = "d:depth p:position n:sh_normal"
AOVS_ALL = "dx:duv_dx dy:duv_dy d:depth p:position uv:uv gn:geo_normal sn:sh_normal du:dp_du dv:dp_dv"


def films():
    """yields (name, raw film, passes)"""
    def raw(integ, scene, sp, **kw):
        sensor = R.make_sensor(sp)
        assert integ.render(scene, sensor, **kw)
        return sensor.film().bitmap(raw=True).cpu().numpy(), integ.stats["passes"]

    def knobs(integ, log2):
        for t in [integ] + ([integ.nested] if getattr(integ, "nested", None) is not None else []):
            t.max_pass_log2 = log2
        return integ

    # tests/test_gpu_lifecycle.py: Cornell box 96 x 64 at 16 spp; max_pass_log2 = 13: passes of five rows
    cbox = R.Scene(scenes.cornell_box())
    sp = scenes.cornell_box_sensor(96, 64, 16, seed=4)
    wide = dict(sp, rfilter_param=1.0)          # gaussian of radius 4: the gather kernel
    yield ("path, one pass",) + raw(R.PathIntegrator(), cbox, sp)
    yield ("path, passes of five rows",) + raw(knobs(R.PathIntegrator(), 13), cbox, sp)
    yield ("moment, passes of five rows",) + raw(knobs(R.MomentIntegrator(R.PathIntegrator()), 13), cbox, sp)
    yield ("path, partition (1, 3, 8), passes of four rows",) + raw(knobs(R.PathIntegrator(), 13), cbox, sp, partition=(1, 3, 8))
    sensor = R.make_sensor(sp)
    d = knobs(R.PathIntegrator(), 13)._desc(sensor)
    d.film_rgb = 1
    rgb, stats = torch.zeros((64, 96, 5), dtype=torch.float32, device="cuda"), (C.c_uint64 * 16)()
    L.check(L.lib().mtsamd_render(cbox._handle, C.byref(d), R._ptr(rgb), stats, R._stream()))
    yield "path, film_rgb = 1, passes of five rows", rgb.cpu().numpy(), int(stats[14])
    yield ("path, gather filter, one pass",) + raw(R.PathIntegrator(), cbox, wide)
    yield ("path, gather filter, passes of five rows",) + raw(knobs(R.PathIntegrator(), 13), cbox, wide)
    # tests/test_gpu_aov.py: displaced sphere 32 x 24 at 4 spp; max_pass_log2 = 10: passes of eight rows
    ball = R.Scene(scenes.bumpy_sphere(12, 24, with_normals=True))
    sp = scenes.bumpy_sphere_sensor(32, 24, 4, seed=3)
    nested = lambda: knobs(R.AOVIntegrator(AOVS_NESTED, R.PathIntegrator(max_depth=3), name="img"), 10)
    yield ("aov(path), streams kept",) + raw(nested(), ball, sp)
    ball.set_aov_keep_limit(0)
    yield ("aov(path), pass by pass",) + raw(nested(), ball, sp)
    yield ("aov alone, pass by pass",) + raw(knobs(R.AOVIntegrator(AOVS_ALL), 10), ball, sp)
    yield ("aov alone, pass by pass, partition (0, 2, 4)",) + raw(knobs(R.AOVIntegrator(AOVS_ALL), 10), ball, sp, partition=(0, 2, 4))
    yield ("aov alone, pass by pass, gather filter",) + raw(knobs(R.AOVIntegrator(AOVS_ALL), 10), ball, dict(sp, rfilter_param=1.0))
    ball.set_aov_keep_limit(1 << 30)
    # tests/test_gpu_lifecycle.py: spectral mesh scene, 96 x 64 at 8 spp
    mesh = R.Scene(scenes.bumpy_sphere(48, 96), variant="spectral")
    yield ("spectral mesh, passes of ten rows",) + raw(knobs(R.PathIntegrator(), 13), mesh, scenes.bumpy_sphere_sensor(96, 64, 8))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--save", metavar="NPZ")
    ap.add_argument("--against", metavar="NPZ")
    args = ap.parse_args()
    kept = dict(np.load(args.against)) if args.against else {}
    out = {}
    for name, film, passes in films():
        out[name] = film
        line = "%s  %-52s %2d passes  %s" % (hashlib.sha256(np.ascontiguousarray(film).tobytes()).hexdigest(), name, passes, "x".join(map(str, film.shape)))
        if name in kept:
            diff = float(np.abs(film.astype(np.float64) - kept[name]).max())
            line += "  equal" if np.array_equal(film, kept[name]) else "  max |difference| %.3g, within rtol = atol = 2e-5: %s" % (diff, np.allclose(film, kept[name], rtol=2e-5, atol=2e-5))
        print(line, flush=True)
    if args.save:
        np.savez(args.save, **out)


if __name__ == "__main__":
    main()

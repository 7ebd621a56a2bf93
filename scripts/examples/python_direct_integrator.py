#!/usr/bin/env python3
"""A direct-lighting integrator written in Python over wavefronts, composed from the operator API of mitsuba2_amd.render: it renders
the Cornell box (tall box: rough copper, short box: plastic) into an ImageBlock, develops it through an HDRFilm and writes an EXR.

The structure is this project's own k_direct (csrc/kernels.hip): per camera sample one emitter sample and one BSDF sample, combined with
the power heuristic, in the kernel's order of operations.  Every lane of the wavefront is the PCG32 stream the built-in integrators give
the same global sample index, so `--check` can compare the result with DirectIntegrator sample by sample.  The integrator is not plugged
into render(): it drives its own loop, one pass of `--spp-per-pass` samples per pixel at a time.

    python scripts/examples/python_direct_integrator.py --out cbox_direct.exr
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mitsuba2_amd import render as R, scenes


def mis_weight(pdf_a, pdf_b):
    """power heuristic (direct.cpp:208-211)"""
    a, b = pdf_a * pdf_a, pdf_b * pdf_b
    return torch.where(a > 0, a / (a + b), torch.zeros_like(a))


def sample_direct(scene, sensor, sampler, index):
    """radiance of the camera samples with global indices `index` (pixel * spp + sample): (rgb (N,3), valid (N,), film position (N,2))"""
    film = sensor.film()
    (cw, ch), (cx, cy), spp = film.crop_size(), film.crop_offset(), sensor.sampler().sample_count()
    pixel = index // spp
    jitter = sampler.next_2d()
    pos = torch.stack([((pixel % cw).float() + float(cx)) + jitter[:, 0], ((pixel // cw).float() + float(cy)) + jitter[:, 1]], dim=1)
    aperture = sampler.next_2d() if sensor.needs_aperture_sample() else None
    sampler.next_1d()                                          # the wavelength sample: drawn in every variant, unused in RGB
    ray = sensor.sample_ray(torch.stack([(pos[:, 0] - float(cx)) / float(cw), (pos[:, 1] - float(cy)) / float(ch)], dim=1), aperture)
    si = scene.ray_intersect(ray)
    valid = si.is_valid()
    ctx = R.BSDFContext()
    bsdf = si.bsdf()

    # emitters seen directly; the environment on lanes that escaped
    result = si.emitter(scene).eval(si)

    # emitter sampling, on smooth BSDFs only
    smooth = valid & R.has_flag(bsdf.flags(), R.BSDFFlags.Smooth)
    ds, emitted = scene.sample_emitter_direction(si, sampler.next_2d(active=smooth), test_visibility=False, active=smooth)
    lit = smooth & (ds.pdf != 0)
    value, bsdf_pdf = bsdf.eval_pdf(ctx, si, si.to_local(ds.d), lit)
    mis = torch.where(ds.delta, torch.ones_like(bsdf_pdf), mis_weight(ds.pdf * 0.5, bsdf_pdf * 0.5))
    contrib = (mis.unsqueeze(1) * value) * emitted
    shadow = lit & (contrib != 0).any(dim=1)                  # the shadow ray is traced only where it can matter
    occluded = scene.ray_test(R.Ray3f(o=si.p, d=ds.d, mint=(1.0 + si.p.abs().amax(dim=1)) * R.RayEpsilon,
                                      maxt=ds.dist * (1.0 - R.ShadowEpsilon)), active=shadow)
    result = result + torch.where((shadow & ~occluded).unsqueeze(1), contrib, torch.zeros_like(contrib))

    # BSDF sampling
    bs, weight = bsdf.sample(ctx, si, sampler.next_1d(active=valid), sampler.next_2d(active=valid), valid)
    go = valid & (weight != 0).any(dim=1)
    si2 = scene.ray_intersect(si.spawn_ray(si.to_world(bs.wo)), active=go)
    emitter = si2.emitter(scene, active=go)
    radiance = emitter.eval(si2, go)
    ds2 = R.DirectionSample3f(si2, si)
    ds2.object, ds2.delta = emitter, R.has_flag(bs.sampled_type, R.BSDFFlags.Delta)
    mis = mis_weight(bs.pdf * 0.5, scene.pdf_emitter_direction(si, ds2, go) * 0.5)
    seen = go & (emitter._lanes >= 0)
    result = result + torch.where(seen.unsqueeze(1), (weight * radiance) * mis.unsqueeze(1), torch.zeros_like(radiance))
    return result, valid, pos


def srgb_to_xyz(rgb):
    """spectrum.h:220-227"""
    m = torch.tensor([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], device=rgb.device)
    return rgb @ m.t()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--spp-per-pass", type=int, default=4, help="samples per pixel in one wavefront")
    ap.add_argument("--out", default="cbox_direct.exr")
    ap.add_argument("--check", action="store_true", help="compare every sample with DirectIntegrator.sample")
    args = ap.parse_args()

    cb = scenes.cornell_box()
    cb["bsdfs"] = list(cb["bsdfs"]) + [{"type": "roughconductor", "alpha": 0.2, "distribution": "ggx", "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14]},
                                       {"type": "plastic", "diffuse_reflectance": [0.1, 0.27, 0.36], "int_ior": 1.9}]
    cb["meshes"][7] = dict(cb["meshes"][7], bsdf=len(cb["bsdfs"]) - 2)       # tall box
    cb["meshes"][6] = dict(cb["meshes"][6], bsdf=len(cb["bsdfs"]) - 1)       # short box
    scene = R.Scene(cb)
    sensor = R.make_sensor(scenes.cornell_box_sensor(args.res, args.res, spp=args.spp, seed=args.seed))
    film = sensor.film()
    block = R.ImageBlock(film.crop_size(), 5, filter=film.reconstruction_filter())
    block.set_offset(film.crop_offset())
    sampler = sensor.sampler()

    total = args.res * args.res * args.spp
    per_pass = args.res * args.res * max(1, min(args.spp_per_pass, args.spp))
    worst = 0.0
    for first in range(0, total, per_pass):
        count = min(per_pass, total - first)
        sampler.seed(args.seed, count, first)
        rgb, valid, pos = sample_direct(scene, sensor, sampler, torch.arange(first, first + count, device="cuda"))
        xyzaw = torch.cat([srgb_to_xyz(rgb), valid.float().unsqueeze(1), torch.ones((count, 1), device="cuda")], dim=1)
        block.put(pos, xyzaw)
        if args.check:
            want, want_valid, want_pos = R.DirectIntegrator(emitter_samples=1, bsdf_samples=1).sample(scene, sensor, first, count)
            assert torch.equal(pos, want_pos) and torch.equal(valid, want_valid)
            worst = max(worst, float(((rgb - want).abs() / torch.maximum(want.abs(), want.mean())).max()))
    film.prepare(device="cuda")
    film.put(block)
    film.set_destination_file(args.out)
    print("wrote", film.develop())
    if args.check:
        print("largest per-sample deviation from DirectIntegrator.sample: %.3e" % worst)


if __name__ == "__main__":
    main()

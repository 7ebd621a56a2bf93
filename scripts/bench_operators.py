#!/usr/bin/env python3
"""Throughput of the operator API (BSDF eval / pdf / sample, emitter sampling / pdf / eval, the wavefront sampler) at 2^22 rows on the
Cornell box (tables in LDS) and on the 261 k-triangle displaced sphere (hierarchy scene: tables in global memory).

Every operator is launched through its C entry point on planes prepared once, so the time is the kernel's and not the packing of the
Python surface.  Per operator: `--warmup` launches, then `--rounds` windows of `--launches` back-to-back launches between two device
events; the median and the range over the windows are printed as one JSON line with the rate in Mquery/s and the achieved bytes/s against
the bytes the algorithm has to move per row (inputs read + outputs written; the scene tables are not counted)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mitsuba2_amd import _lib as L, render, scenes

ROUGH = {"type": "roughconductor", "alpha": 0.2, "distribution": "ggx", "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14]}
PLASTIC = {"type": "plastic", "diffuse_reflectance": [0.1, 0.27, 0.36], "int_ior": 1.9}


def _cases():
    cb = scenes.cornell_box()
    cb["bsdfs"] = list(cb["bsdfs"]) + [ROUGH, PLASTIC]
    cb["meshes"][7] = dict(cb["meshes"][7], bsdf=len(cb["bsdfs"]) - 2)       # tall box
    cb["meshes"][6] = dict(cb["meshes"][6], bsdf=len(cb["bsdfs"]) - 1)       # short box
    mesh = scenes.bumpy_sphere(256, 512)
    mesh["bsdfs"] = [ROUGH] + list(mesh["bsdfs"][1:])
    return [("cbox", cb, ((10, 10, 10), (540, 540, 550))), ("mesh261k", mesh, ((-3, 0.1, -3), (3, 3.5, 3)))]


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    n, lib = args.rows, L.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator(device="cuda").manual_seed(1)
    unit = lambda: torch.nn.functional.normalize(torch.randn((n, 3), device="cuda", generator=gen), dim=1).t().contiguous()
    uniform = lambda k: torch.rand((k, n), device="cuda", generator=gen)
    for name, sd, (lo, hi) in _cases():
        scene = render.Scene(sd)
        h = scene._handle
        n_shapes, n_emitters = scene.shape_count(), len(sd["emitters"])
        shape = (torch.arange(n, device="cuda") % n_shapes).to(torch.int32)
        rough = torch.full((n,), 7 if name == "cbox" else 0, dtype=torch.int32, device="cuda")      # the shape that carries ROUGH
        wi, wo, uv, s3 = unit(), unit(), uniform(2), uniform(3)
        ref = (torch.tensor(lo, device="cuda") + uniform(3).t() * (torch.tensor(hi, device="cuda") - torch.tensor(lo, device="cuda"))).t().contiguous()
        out = torch.empty((16, n), dtype=torch.float32, device="cuda")
        index = torch.empty(n, dtype=torch.int32, device="cuda")
        state = torch.empty((2, n), dtype=torch.int64, device="cuda")

        def query(shapes):
            q = L.BsdfQuery()
            q.shape, q.wi_x, q.wi_y, q.wi_z, q.u, q.v = _ptr(shapes), _ptr(wi[0]), _ptr(wi[1]), _ptr(wi[2]), _ptr(uv[0]), _ptr(uv[1])
            q.wo_x, q.wo_y, q.wo_z = _ptr(wo[0]), _ptr(wo[1]), _ptr(wo[2])
            q.sample1, q.sample2_x, q.sample2_y = _ptr(s3[0]), _ptr(s3[1]), _ptr(s3[2])
            return q

        q_all, q_rough = query(shape), query(rough)
        # one emitter sample first: the pdf / eval operators run on its record
        L.check(lib.mtsamd_sample_emitter_direction(h, n, _ptr(ref), _ptr(s3), None, _ptr(out), _ptr(index), stream))
        ds = out[:15].clone()
        emitter = index.clone()
        L.check(lib.mtsamd_sampler_seed(n, 0, 0, _ptr(state[0]), _ptr(state[1]), stream))
        # (label, bytes read + written per row, launch)
        ops = [
            ("bsdf_eval_pdf (all shapes)", 4 + 12 + 8 + 12 + 16, lambda: lib.mtsamd_bsdf_eval_pdf(h, n, C.byref(q_all), _ptr(out), stream)),
            ("bsdf_eval_pdf (roughconductor)", 4 + 12 + 8 + 12 + 16, lambda: lib.mtsamd_bsdf_eval_pdf(h, n, C.byref(q_rough), _ptr(out), stream)),
            ("bsdf_sample (all shapes)", 4 + 12 + 8 + 12 + 40, lambda: lib.mtsamd_bsdf_sample(h, n, C.byref(q_all), _ptr(out), stream)),
            ("bsdf_sample (roughconductor)", 4 + 12 + 8 + 12 + 40, lambda: lib.mtsamd_bsdf_sample(h, n, C.byref(q_rough), _ptr(out), stream)),
            ("sample_emitter_direction", 12 + 8 + 60 + 4, lambda: lib.mtsamd_sample_emitter_direction(h, n, _ptr(ref), _ptr(s3), None, _ptr(out), _ptr(index), stream)),
            ("pdf_emitter_direction", 4 + 12 + 12 + 4 + 4, lambda: lib.mtsamd_pdf_emitter_direction(h, n, _ptr(emitter), _ptr(ds[6:9]), _ptr(ds[3:6]), _ptr(ds[9]), None, None, _ptr(out), stream)),
            ("emitter_eval", 4 + 12 + 12 + 12, lambda: lib.mtsamd_emitter_eval(h, n, _ptr(emitter), _ptr(wi), _ptr(ds[6:9]), None, _ptr(out), stream)),
            ("sampler_seed", 16, lambda: lib.mtsamd_sampler_seed(n, 0, 0, _ptr(state[0]), _ptr(state[1]), stream)),
            ("sampler_next_1d", 8 + 8 + 8 + 4, lambda: lib.mtsamd_sampler_next(n, 1, _ptr(state[0]), _ptr(state[1]), None, _ptr(out), stream)),
            ("sampler_next_2d", 8 + 8 + 8 + 8, lambda: lib.mtsamd_sampler_next(n, 2, _ptr(state[0]), _ptr(state[1]), None, _ptr(out), stream)),
        ]
        for label, row_bytes, launch in ops:
            for _ in range(args.warmup):
                L.check(launch())
            ms = []
            for _ in range(args.rounds):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.launches):
                    L.check(launch())
                t1.record()
                t1.synchronize()
                ms.append(t0.elapsed_time(t1) / args.launches)
            ms = np.array(ms)
            med = float(np.median(ms))
            print(json.dumps(dict(scene=name, operator=label, rows=n, emitters=n_emitters, ms_median=round(med, 4),
                                  ms_range=[round(float(ms.min()), 4), round(float(ms.max()), 4)], mquery_per_s=round(n / med * 1e-3, 1),
                                  bytes_per_row=row_bytes, gbyte_per_s=round(n * row_bytes / med * 1e-6, 1))), flush=True)


if __name__ == "__main__":
    main()

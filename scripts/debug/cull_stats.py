"""Diagnostic (libraries built with -DMTS_CULL_STATS=1 or 2, loaded through MTSAMD_LIB): triangles really tested per ray on the
Cornell box -- per closest-hit ray (MTS_CULL_STATS=1: the any-hit queries count nominally) or per shadow ray (MTS_CULL_STATS=2: the
closest-hit queries count nominally).  Pass the build's value as the first argument.  Builds with -DMTS_CULL_STATS=4 / 8 count, on top
of the nominal figures, the wave queries of the per-(ray, pair) work lists that fall back to the plain loop (4) or all of them (8):
the fallback share is the ratio of the two figures (the render, and with it the wave queries, is the same in both builds)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from mitsuba2_amd import render as R, scenes
mode = int(sys.argv[1]) if len(sys.argv) > 1 else 1
scene = R.Scene(scenes.cornell_box())
sensor = R.make_sensor(scenes.cornell_box_sensor(1024, 1024, 64))
integ = R.PathIntegrator()
integ.render(scene, sensor); torch.cuda.synchronize()
st = integ.stats
n_prims = 36.0
nominal = n_prims * (st["closest_hit_rays"] + st["any_hit_rays"])
if mode in (4, 8):
    extra = st["tri_tests"] - nominal
    print("work-list wave queries%s: %d  (closest-hit rays %.3e, shadow rays %.3e)" %
          (" taking the plain-loop fallback" if mode == 4 else "", int(round(extra)), st["closest_hit_rays"], st["any_hit_rays"]))
    sys.exit(0)
if mode == 1:
    kind, rays, real = "closest-hit", st["closest_hit_rays"], st["tri_tests"] - n_prims * st["any_hit_rays"]
else:
    kind, rays, real = "shadow", st["any_hit_rays"], st["tri_tests"] - n_prims * st["closest_hit_rays"]
print("tri tests %.3e nominal %.3e  %s rays %.3e  -> %.2f tests = %.2f pairs per %s ray (36 tests = no culling)" %
      (st["tri_tests"], nominal, kind, rays, real / rays, real / rays / 2.0, kind))

"""Diagnostic (a library built with -DMTS_FATED_STATS=1, loaded through MTSAMD_LIB): the share of closest-hit queries that the fated-path
rule elides (fated.h).  In that build an elided query is counted as a segment but NOT as a closest-hit ray, so the share is
1 - closest_hit_rays / segments.  Cornell box 1024 x 1024 @ 64 spp by default: `fated_stats.py [max_depth [rr_depth]]`."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from mitsuba2_amd import render as R, scenes
max_depth = int(sys.argv[1]) if len(sys.argv) > 1 else -1
rr_depth = int(sys.argv[2]) if len(sys.argv) > 2 else 5
scene = R.Scene(scenes.cornell_box())
sensor = R.make_sensor(scenes.cornell_box_sensor(1024, 1024, 64))
integ = R.PathIntegrator(max_depth=max_depth, rr_depth=rr_depth)
integ.render(scene, sensor); torch.cuda.synchronize()
st = integ.stats
seg, cl = st["segments"], st["closest_hit_rays"]
print("max_depth %d rr_depth %d: segments %.4e per sample %.3f, closest-hit queries run %.4e, elided %.4e = %.2f %% of the queries" %
      (max_depth, rr_depth, seg, seg / st["samples"], cl, seg - cl, 100.0 * (seg - cl) / seg))

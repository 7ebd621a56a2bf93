"""Pool drain of the shadow-ring schedule (kernels.hip, k_shade with gather_w > 4): once the sample cursors are dry and the pool
has shrunk, one workgroup takes the paths of gather_w scheduling waves; their prefix sums live in dynamic LDS after the shadow rings
and only these launches reserve them.  With k_finish switched off (finish_kernel = 1) the launch rounds run the pool dry and pass
through every gathering width; with finish_kernel = 2 the pass ends in k_finish as soon as the cursors are dry, before any gathering,
and the queued-shadow-ray schedule (pipeline 3) never gathers.  A path performs the same floating-point operations in the same order
in every schedule, so the Cornell-box films must be equal bit for bit."""
import pytest
import torch

from mitsuba2_amd import scenes

pytestmark = pytest.mark.gpu


def _film(variant, pipeline, finish_kernel, p):
    from mitsuba2_amd import render as R
    scene = R.Scene(scenes.cornell_box(), variant=variant)
    integ = R.PathIntegrator(pipeline=pipeline)
    integ.finish_kernel = finish_kernel
    sensor = R.make_sensor(p)
    assert integ.render(scene, sensor)
    return sensor.film().bitmap(raw=True).clone(), dict(integ.stats)


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
def test_gathering_drain_equals_plain_schedules(variant):
    p = scenes.cornell_box_sensor(256, 256, 64, seed=5)
    gathered, sg = _film(variant, 4, 1, p)
    no_gather, sn = _film(variant, 4, 2, p)
    queued, sq = _film(variant, 3, 0, p)
    assert sg["iterations"] > sn["iterations"]                   # the launch rounds really drained the pool
    for k in ("samples", "segments", "closest_hit_rays", "any_hit_rays"):
        assert sg[k] == sn[k] == sq[k], (k, sg[k], sn[k], sq[k])
    assert torch.equal(gathered, no_gather)
    assert torch.equal(gathered, queued)
    assert torch.isfinite(gathered).all() and gathered[..., :3].max() > 0

"""autodiff.render() folds a per-scene call counter into the seed and keeps it under id(scene).  CPython reuses ids, so the entry has to
go when the scene dies: a new scene that receives a dead scene's id must start at call 0, whatever renders or tests ran before.  No GPU:
the stand-in scene lets render() get as far as the counter and fails when the description is built."""
import gc

import pytest

from mitsuba2_amd import autodiff


class _Sampler:
    def seed_value(self):
        return 3


class _Sensor:
    def sampler(self):
        return _Sampler()


class _Scene:
    def sensors(self):
        return [_Sensor()]

    def integrator(self):
        return object()


def _render_once(scene):
    with pytest.raises(Exception):
        autodiff.render(scene, spp=1)


def test_counter_entry_dies_with_its_scene():
    scene = _Scene()
    key = id(scene)
    _render_once(scene)
    _render_once(scene)
    assert autodiff._render_counter[key] == 2
    autodiff._render_counter[key] = 11                      # what tests do to pin the random numbers
    del scene
    gc.collect()
    assert key not in autodiff._render_counter and key not in autodiff._render_tracked
    # a scene at a recycled address starts at call 0
    for _ in range(64):
        fresh = _Scene()
        assert autodiff._render_counter.get(id(fresh), 0) == 0
        _render_once(fresh)
        assert autodiff._render_counter[id(fresh)] == 1
        del fresh

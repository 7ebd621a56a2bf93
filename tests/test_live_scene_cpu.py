"""What tests/test_gpu_live_scene.py and tests/test_gpu_rebuild_sizes.py rest on, established without a GPU.

1. No case of test_gpu_live_scene.py passes vacuously: for every consumer the oracle implements, the oracle's output on the old and on
   the moved description (live_scene.SPHERE_MOVES on the hierarchy scene, live_scene.CBOX_MOVES on the flat one) differs in at least
   MOVED_MIN = 5 % of its entries -- radiance, direct, depth, the aov channels, fill_si, sample_emitter -- and the gradients of
   render_adjoint, render_adjoint_param and render_adjoint_envmap differ by more than ten times the comparison bound of the GPU test in at
   least 5 % of their non-zero entries.  The measured shares are SHARES_MEASURED, percent; each is printed and asserted.
2. The three sequences of test_gpu_live_scene.py each hold a rebuild of either builder followed later by a refit, and a
   normals="recompute" update after a rebuild.
3. The inputs of test_gpu_rebuild_sizes.py: build_sah_levels equals build_bvh byte for byte at 4 097 and 32 769 triangles; build_lbvh's
   slot_prim for copies(2049) is 0..2048; nb > 1 024 builder nodes for the 4 097 soup under both builders; the widest level of the SAH
   build at 32 769 exceeds one block of the 64-bit scan."""
import os

import numpy as np
import pytest

import lbvh_cases as lc
import live_scene as ls
import sah_cases as sc
import vertex_moves as vm
from test_sah_levels_cpu import assert_same_tree_as_creation

F32 = np.float32
# percent of entries (rows) the moves change, measured with the CPU oracle
SHARES_MEASURED = {
    "sphere-path": 57.6, "sphere-direct": 53.2, "sphere-depth": 30.5, "sphere-aov": 30.5, "sphere-fill_si": 51.5, "sphere-ray_test": 27.0,
    "sphere-sample_emitter": 100.0, "spectral-colours": 57.6, "spectral-table": 57.6,
    "cbox-path": 79.9, "cbox-direct": 62.5, "cbox-depth": 9.5, "cbox-aov": 9.9, "cbox-fill_si": 45.9, "cbox-ray_test": 30.6, "cbox-sample_emitter": 100.0,
    "render_adjoint": 100.0, "render_adjoint_param": 100.0, "render_adjoint_envmap": 95.9,
}


def _report(name, value):
    print("%s: the moves change %.1f %% (recorded %.1f)" % (name, 100.0 * value, SHARES_MEASURED.get(name, float("nan"))))
    assert value >= ls.MOVED_MIN, (name, value)
    assert abs(100.0 * value - SHARES_MEASURED[name]) < 0.05, (name, 100.0 * value)


def _scenes(kind):
    old, p = ls.sphere_scene() if kind == "sphere" else ls.cbox_scene()
    return old, vm.moved(old, *(ls.SPHERE_MOVES if kind == "sphere" else ls.CBOX_MOVES)), p


@pytest.mark.parametrize("kind", ["sphere", "cbox"])
@pytest.mark.parametrize("integrator", ["path", "direct", "depth"])
def test_streams_move(oracle, kind, integrator):
    old, new, p = _scenes(kind)
    before, _ = ls.oracle_stream(oracle, old, p, integrator)
    after, _ = ls.oracle_stream(oracle, new, p, integrator)
    _report("%s-%s" % (kind, integrator), ls.share(before, after))


@pytest.mark.parametrize("tabulated", [False, True], ids=["colours", "table"])
def test_spectral_streams_move(oracle, tabulated):
    from mitsuba2_amd import render
    _, old, p = ls.spectral_scene(tabulated)
    new = vm.moved(old, *ls.SPHERE_MOVES)
    path = render.srgb_coeff_path()
    before, _ = ls.oracle_stream(oracle, old, p, spectral_path=path)
    after, _ = ls.oracle_stream(oracle, new, p, spectral_path=path)
    _report("spectral-%s" % ("table" if tabulated else "colours"), ls.share(before, after))


@pytest.mark.parametrize("kind", ["sphere", "cbox"])
def test_aov_channels_move(oracle, kind):
    old, new, p = _scenes(kind)
    _, before = ls.oracle_aovs(oracle, old, p)
    _, after = ls.oracle_aovs(oracle, new, p)
    _report("%s-aov" % kind, ls.share(before, after))
    groups = {"depth": [4], "position": [5, 6, 7], "uv": [8, 9], "geo_normal": [10, 11, 12], "sh_normal": [13, 14, 15], "dp_du": [16, 17, 18], "dp_dv": [19, 20, 21]}
    for name, cols in groups.items():          # every channel type alone keeps the floor, but for the two that are always zero
        alone = ls.share(before[:, cols], after[:, cols])
        print("%s %s alone: %.1f %%" % (kind, name, 100.0 * alone))
        assert alone >= ls.MOVED_MIN or (kind == "cbox" and "aov-" + name in ls.FLAT_WITHOUT_FLOOR), (kind, name, alone)
    assert not before[:, :4].any() and not after[:, :4].any()


@pytest.mark.parametrize("kind", ["sphere", "cbox"])
def test_queries_move(oracle, kind):
    old, new, _ = _scenes(kind)
    rays = ls.fixed_inputs(kind)[0]
    (ref0, hit0, si0), (ref1, hit1, si1) = ls.oracle_queries(oracle, old, rays), ls.oracle_queries(oracle, new, rays)
    v0, v1 = np.isfinite(ref0[0]), np.isfinite(ref1[0])
    rows0 = np.where(v0[:, None], np.concatenate([ref0[0][:, None], si0], 1), 0)
    rows1 = np.where(v1[:, None], np.concatenate([ref1[0][:, None], si1], 1), 0)
    _report("%s-fill_si" % kind, ls.share(rows0, rows1))
    _report("%s-ray_test" % kind, ls.share(hit0, hit1))


@pytest.mark.parametrize("kind", ["sphere", "cbox"])
def test_emitter_samples_move(oracle, kind):
    old, new, _ = _scenes(kind)
    _, points, samples = ls.fixed_inputs(kind)
    _report("%s-sample_emitter" % kind, ls.share(ls.oracle_emitter_samples(oracle, old, points, samples), ls.oracle_emitter_samples(oracle, new, points, samples)))


def test_derivative_gradients_move(oracle):
    old, p = ls.derivative_scene()
    new = vm.moved(old, *ls.SPHERE_MOVES)
    (param0, env0), (param1, env1) = ls.oracle_derivative_gradients(oracle, old, p), ls.oracle_derivative_gradients(oracle, new, p)
    _report("render_adjoint_param", ls.gradient_share(param0, param1))
    _report("render_adjoint_envmap", ls.gradient_share(env0, env1))


def test_diffuse_gradients_move(oracle):
    tex = ls.texture()
    old, p = ls.cbox_scene(tex)
    new = vm.moved(old, *ls.CBOX_MOVES)
    _report("render_adjoint", ls.gradient_share(ls.oracle_diffuse_gradients(oracle, old, p, tex.size), ls.oracle_diffuse_gradients(oracle, new, p, tex.size)))


# ---- 2. the sequences ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ls.SEQUENCE_SEEDS)
def test_sequences_hold_what_they_are_for(seed):
    steps = ls.sequence(seed)
    assert len(steps) == ls.SEQUENCE_STEPS and steps == ls.sequence(seed)
    refit_after, recompute_after = ls.sequence_facts(steps)
    assert refit_after == {"lbvh", "sah"} and recompute_after, steps
    sd = ls.derivative_scene()[0]
    for step in steps:                       # the tracked description advances without a device
        sd, made = ls.sequence_step(None, sd, step)
        assert made in (0, 1)


# ---- 3. the inputs of test_gpu_rebuild_sizes.py ------------------------------------------------------------------------------------------------
SCAN_BLOCK_U64 = 256 * 15          # the larger of the two one-block limits of rocprim::exclusive_scan on unsigned long long (see the GPU file)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(vm.HIPCC):
        pytest.skip("hipcc not installed")
    return sc.Driver(tmp_path_factory.mktemp("live_sizes"))


@pytest.mark.parametrize("n", [4097, 32769])
def test_sah_levels_is_creations_builder_at_the_large_sizes(driver, n):
    name = "n%d" % n
    raw = driver.run(None, lc.raw_text(name, lc.soup_triangles(n)), name)
    assert_same_tree_as_creation(raw, name, name + "b")
    nb = len(raw[name + ".order"])
    assert nb == len(raw[name + ".kids"]) // 2 and nb > 1024
    widest = int(np.bincount(raw[name + ".t_depth"]).max())
    print("%s: %d builder nodes, widest level %d" % (name, nb, widest))
    if n == 32769:
        assert widest + 1 > SCAN_BLOCK_U64 and 2 * n > 65537


def test_lbvh_of_the_large_inputs(driver):
    out = driver.run(lc.triangle_scene(lc.copies(2049)), ["lbvh l"], "copies2049")
    assert np.array_equal(out["l.slot_prim"], np.arange(2049, dtype=np.uint32))
    assert len(set(lc.morton_codes(lc.copies(2049)).tolist())) == 1
    out = driver.run(lc.triangle_scene(lc.soup_triangles(4097)), ["lbvh l"], "n4097")
    assert len(out["l.order"]) > 1024 and len(out["l.order"]) == len(out["l.kids"]) // 2

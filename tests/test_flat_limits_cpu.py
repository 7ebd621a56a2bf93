"""LDS-resident scenes at their table limits, without a GPU.  The byte counts of every flat-scene launch (device_scene.h lds_bytes,
kernels.h shade_ring_lds_bytes and flat_launch_lds_max) are held against their restatement in tests/flat_limits.py; the builder
(scene_build.cpp) keeps a scene flat exactly while its largest launch fits the cap, and builds it as a hierarchy scene with a walkable
BVH4 beyond; and the scenes the GPU tests render satisfy the conditions that make a radiance comparison worth something (oracle only)."""
import numpy as np
import pytest

import flat_limits as fl
import oracle_binding as ob
from mitsuba2_amd import bsdfs as B, emitters as E, scenes
from test_scene_build_cpu import SPECTRAL, bsdf, driver, emitter, flags, mesh  # noqa: F401  (driver: the compiled builder, a module fixture)

LIMITS = ("mega", "block", "ring_rgb_steady", "ring_spectral_gather", "max_rgb", "max_spectral", "cap", "n_wnodes", "wdepth")


def records(sd, spectral=False):
    """A scene dictionary as records of the builder driver (spectral: built as a scene of the spectral variant).  The driver lays out triangles of its own; every figure tested here depends
    on the counts alone: triangles per mesh in mesh order, the flattened BSDF table with its nesting, the emitters and who owns them."""
    out = [SPECTRAL] if spectral else []
    out += [mesh(len(np.asarray(m["faces"]).reshape(-1, 3)), int(m["bsdf"]), int(m.get("emitter", -1))) for m in sd["meshes"]]
    for n in B.flatten([B.normalize(b) for b in sd["bsdfs"]]):
        out.append(bsdf(n["type"], twosided=int(n["twosided"]), nested=n.get("nested", [-1, -1]), reflectance=[0.5, 0.5, 0.5]))
    for e in sd.get("emitters", []):
        n = E.normalize(e)
        out.append(emitter(n["type"], radiance=n["radiance"], to_world=n["to_world"].reshape(-1), cutoff_angle=n["cutoff_angle"], beam_width=n["beam_width"]))
    return out


def limits(scene):
    return dict(zip(LIMITS, (int(x) for x in scene["limits"])))


def expected(c):
    return dict(mega=fl.lds_bytes(c, 64), block=fl.lds_bytes(c, 256), ring_rgb_steady=fl.ring_bytes(c, False, 4),
                ring_spectral_gather=fl.ring_bytes(c, True, 1024), max_rgb=fl.launch_max(c, False), max_spectral=fl.launch_max(c, True), cap=fl.CAP)


def built(driver, named, spectral=False):
    out = driver({k: records(sd, spectral) for k, sd in named.items()})
    assert all(s["rc"] == 0 for s in out.values()), {n: s["message"] for n, s in out.items() if s["rc"]}
    return out


def test_byte_counts_match_the_restated_formulas(driver):
    """the four scenes whose demands the project documents (prims / shapes / BSDF records / emitters): the Cornell box 36 / 8 / 4 / 1,
    64 / 64 / 64 / 1, 64 / 64 / 64 / 64 and -- every facet behind a `mask` -- 64 / 64 / 128 / 64; then soups of every size and partition"""
    masked = fl.soup(64, "per_triangle", 64)
    masked = dict(masked, bsdfs=[dict(type="mask", opacity=0.7, bsdf=b) if b["type"] != "twosided" else dict(type="mask", opacity=0.7, bsdf=b["bsdf"]) for b in masked["bsdfs"]])
    named = {"cbox": scenes.cornell_box(), "one_emitter": fl.soup(64, "per_triangle", 1), "all_emitters": fl.soup(64, "per_triangle", 64), "masked": masked}
    assert [fl.counts(named[k])[:1] + fl.counts(named[k])[3:] for k in named] == [(36, 8, 4, 1), (64, 64, 64, 1), (64, 64, 64, 64), (64, 64, 128, 64)]
    named.update({"soup_%d_%s" % (n, p): fl.soup(n, p, 64) for n in fl.SOUP_SIZES for p in fl.PARTITIONS if n <= fl.FLAT_MAX})
    out = built(driver, named)
    for name, sd in named.items():
        c, f, got = fl.counts(sd), flags(out[name]), limits(out[name])
        assert (f["n_prims"], f["n_pairs"], f["n_clusters"], f["n_shapes"], len(out[name]["bsdfs"]) * 4 // fl.BSDF_BYTES, len(out[name]["emitters"]) * 4 // fl.EMITTER_BYTES) == c, name
        assert {k: got[k] for k in expected(c)} == expected(c), name
        assert f["flat"] == 1 and got["max_rgb"] <= got["max_spectral"] <= fl.CAP
    # the ring formulas are the largest; the 64-triangle scene with 64 one-triangle shapes has a full pair mask
    assert fl.counts(named["all_emitters"])[1] == 32 and fl.launch_max(fl.counts(named["cbox"]), True) == fl.ring_bytes(fl.counts(named["cbox"]), True, 1024)


@pytest.mark.parametrize("spectral", [False, True])
def test_flat_boundary_in_emitters_and_records(driver, spectral):
    """In either variant (the spectral ring entries are 4 bytes larger, so a spectral scene stops being flat 14 emitters or 16 records
    sooner), one emitter / one BSDF record decides: the last count that is flat and the first that is not, for the Cornell box under a grid of
    point lights and for 64 one-triangle shapes with a growing material library.  Over the cap the scene is a hierarchy scene with a
    BVH4 to walk (stack depth 3 * wdepth + 2 >= 2), not an error."""
    cb, soup = scenes.cornell_box(), fl.soup(64, "per_triangle", 64)
    n_e, n_r = fl.last_flat_extra(fl.counts(cb), spectral), fl.last_flat_records(fl.counts(soup), spectral)
    assert n_e > 500 and n_r > 500
    assert n_e == fl.last_flat_extra(fl.counts(cb), True) + (0 if spectral else 14) and n_r == fl.last_flat_records(fl.counts(soup), True) + (0 if spectral else 16)
    key = "max_spectral" if spectral else "max_rgb"
    named = {"lights_last": fl.many_lights(cb, n_e - n_e // 3, n_e // 3, 0), "lights_first": fl.many_lights(cb, n_e + 1 - n_e // 3, n_e // 3, 0),
             "records_last": fl.with_records(soup, n_r), "records_first": fl.with_records(soup, n_r + 1),
             "far_over": fl.many_lights(cb, 2000, 0, 0), "65": fl.soup(65, "per_triangle", 64)}
    out = built(driver, named, spectral)
    for name, sd in named.items():
        c, f, got = fl.counts(sd), flags(out[name]), limits(out[name])
        assert {k: got[k] for k in expected(c)} == expected(c), name
        assert f["spectral"] == int(spectral) and f["flat"] == int(fl.is_flat(c, spectral)), (name, c, got)
        if f["flat"]:
            assert got[key] <= fl.CAP
        else:
            assert f["n_pairs"] == 0 and f["n_clusters"] == 0 and len(out[name]["flat_recs"]) == 0
            assert got["n_wnodes"] > 0 and 3 * got["wdepth"] + 2 >= 2
    assert [flags(out[k])["flat"] for k in named] == [1, 0, 1, 0, 0, 0]
    assert limits(out["lights_last"])[key] <= fl.CAP < limits(out["lights_first"])[key] == limits(out["lights_last"])[key] + fl.EMITTER_BYTES
    assert limits(out["records_last"])[key] <= fl.CAP < limits(out["records_first"])[key] == limits(out["records_last"])[key] + fl.BSDF_BYTES


def test_bands_land_where_they_should():
    """many_lights counts for the GPU tests come from the arithmetic: each formula's `mid` count puts that launch in (48 KiB, 64 KiB), its
    `100k` count within one emitter record of 100 KiB, unless the scene stops being flat first"""
    c = fl.counts(scenes.cornell_box())
    b = fl.bands(c)
    for name, f in fl.FORMULAS.items():
        spectral = fl.VARIANT[name] == "spectral"
        last = fl.last_flat_extra(c, spectral)
        mid, big = f(fl._with_emitters(c, b[(name, "mid")])), f(fl._with_emitters(c, b[(name, "100k")]))
        assert 48 * 1024 < mid < 64 * 1024, (name, mid)
        assert (100 * 1024 <= big < 100 * 1024 + fl.EMITTER_BYTES) or b[(name, "100k")] == last, (name, big)
        assert fl.is_flat(fl._with_emitters(c, b[(name, "last_flat")]), spectral) and not fl.is_flat(fl._with_emitters(c, b[(name, "first_hier")]), spectral)


# ---- the scenes of the GPU radiance tests are worth comparing: oracle only ---------------------------------------------------------------
def _radiance(sd, sp):
    n = sp["width"] * sp["height"] * sp["sample_count"]
    return ob.OracleScene(sd).sample_radiance(ob.make_desc(sp), 0, n)[0]


@pytest.mark.parametrize("n_tris", fl.SOUP_SIZES)
@pytest.mark.parametrize("partition", fl.PARTITIONS)
def test_soups_are_hit_and_lit(n_tris, partition):
    want = _radiance(fl.soup(n_tris, partition, 64), fl.soup_sensor(32, 32, 8))
    assert np.isfinite(want).all()
    assert (want[:, 3] > 0.5).mean() >= 0.25 and (want[:, :3].max(1) > 0).mean() >= 0.10


def test_many_lights_change_the_picture():
    cb, sp = scenes.cornell_box(), scenes.cornell_box_sensor(32, 32, 8, seed=2)
    base = _radiance(cb, sp)
    b = fl.bands(fl.counts(cb))
    for n in sorted(set(b.values())):
        want = _radiance(fl.many_lights(cb, n - n // 3, n // 3, 0), sp)
        assert np.isfinite(want).all()
        assert (want[:, 3] > 0.5).mean() >= 0.25 and (want[:, :3].max(1) > 0).mean() >= 0.10
        assert (want[:, :3] != base[:, :3]).any(1).mean() >= 0.50, n

"""The host half of the flat scenes' shading records (mitsuba2_amd/csrc/scene_build.cpp, build_flat_records) without a GPU, through
tests/scene_build_driver.cpp.  The 64-byte record of primitive i is

    r0 = (p0.xyz, n.x)  r1 = (n.y, n.z, s.x, s.y)  r2 = (s.z, p1.xyz)  r3 = (p2.xyz, shape bits)

and the host writes zeros into the six frame words (n, s): k_flat_frames fills them on the device at scene creation
(tests/test_gpu_flat_frames.py).  This pins the words Geo<true>::tri_positions / prim_shape and the frame kernel agree on."""
import numpy as np

from test_scene_build_cpu import AREA, bsdf, driver, emitter, f32, flags, mesh  # noqa: F401  (driver: the fixture)

FRAME_WORDS = [3, 4, 5, 6, 7, 8]
POSITION_WORDS = [0, 1, 2, 9, 10, 11, 12, 13, 14]


def test_host_record_layout(driver):
    out = driver({
        "mixed": [mesh(3, 0), mesh(2, 1, uv=1), mesh(1, 0, normals=1), mesh(2, 1, 0, uv=1, normals=1), bsdf(), bsdf(), emitter(AREA)],
        "one_triangle": [mesh(1, 0), bsdf()],
        "last_flat": [mesh(60, 0), mesh(4, 0, uv=1), bsdf()],
        "first_hierarchy": [mesh(60, 0), mesh(5, 0, uv=1), bsdf()],
        "empty": [],
    })
    assert all(s["rc"] == 0 for s in out.values()), {n: s["message"] for n, s in out.items()}
    for name, n_prims in (("mixed", 8), ("one_triangle", 1), ("last_flat", 64)):
        s = out[name]
        assert flags(s)["flat"] == 1 and flags(s)["n_prims"] == n_prims
        words = s["flat_recs"].reshape(n_prims, 16)
        # positions in primitive order at r0.xyz, r2.yzw, r3.xyz -- the very words of tri_pos
        assert np.array_equal(words[:, POSITION_WORDS], s["tri_pos"].reshape(n_prims, 9)), name
        assert np.array_equal(words[:, 15], s["prim_shape"]), name                       # shape bits
        assert not words[:, FRAME_WORDS].any(), name                                     # +0.0 in every frame word: the device's to fill
    # the driver's geometry: triangle k of mesh i is (k, 0, i) (k + 1, 0, i) (k, 1, i)
    rec = f32(out["mixed"]["flat_recs"]).reshape(8, 16)
    assert np.array_equal(rec[4, POSITION_WORDS], np.float32([1, 0, 1, 2, 0, 1, 1, 1, 1]))
    assert list(out["mixed"]["prim_shape"]) == [0, 0, 0, 1, 1, 2, 3, 3]
    assert flags(out["first_hierarchy"])["flat"] == 0 and out["first_hierarchy"]["flat_recs"].size == 0      # 65 primitives: no records at all
    assert flags(out["empty"])["flat"] == 1 and out["empty"]["flat_recs"].size == 0

"""LDS-resident ("flat") scenes at their limits: the host arithmetic of their LDS demand, restated, and the scenes that sit on it.

A scene of at most FLAT_MAX triangles is staged whole in LDS by every kernel that touches it (device_scene.h, lds_stage<true>): shading
records, pair records, cluster boxes, the shape, BSDF and emitter tables, the area distributions and the per-wave work lists.  `lds_bytes`,
`ring_bytes` and `launch_max` restate lds_bytes(), shade_ring_lds_bytes() and flat_launch_lds_max() of device_scene.h / kernels.h;
tests/test_flat_limits_cpu.py holds them against the C++ byte for byte.  `soup` builds triangle soups at the primitive limits (1, 2, 3,
63, 64 triangles, and 65: the smallest hierarchy scene), `many_lights` adds delta emitters -- which own no triangle, so their count is
bounded by nothing but the LDS cap -- and `bands` picks the emitter counts at which each launch formula lands in a given place."""
import functools

import numpy as np

from mitsuba2_amd import bsdfs as B

F32 = np.float32
FLAT_MAX = 64                     # kFlatMaxPrims
CAP = 150 * 1024                  # kFlatLdsCap: a scene whose largest launch asks for more is built as a hierarchy scene
SHAPE_BYTES, BSDF_BYTES, EMITTER_BYTES = 16, 128, 144      # sizeof(DevShape), sizeof(DevBsdf), sizeof(DevEmitter)
WL_ROUNDS = 8                     # MTS_FLAT_WL_ROUNDS
WL_WORDS = 128 + 64 * WL_ROUNDS // 2                        # kWlWords
SHADOW_RING, SHADE_WAVES, GATHER_MAX = 128, 4, 1024         # kShadowRing, kShadeWaves, the widest gathering launch
PARTITIONS = ("one_shape", "per_triangle", "mixed")
SOUP_SIZES = (1, 2, 3, 63, 64, 65)


# ---------------------------------------------------------------------------------------------------------------- host arithmetic
def counts(sd):
    """(n_prims, n_pairs, n_clusters, n_shapes, n_bsdf_records, n_emitters) of a scene dictionary, as the builder counts them: a pair is
    two consecutive primitives, a cluster a run of pairs whose first primitives belong to one shape, the BSDF table holds the top-level
    records followed by the children of blendbsdf / mask records."""
    prim_shape = [i for i, m in enumerate(sd["meshes"]) for _ in range(len(np.asarray(m["faces"]).reshape(-1, 3)))]
    n_prims = len(prim_shape)
    n_pairs = (n_prims + 1) // 2
    n_clusters = sum(1 for k in range(n_pairs) if k == 0 or prim_shape[2 * k] != prim_shape[2 * (k - 1)])
    n_bsdfs = len(B.flatten([B.normalize(b) for b in sd["bsdfs"]]))
    return n_prims, n_pairs, n_clusters, len(sd["meshes"]), n_bsdfs, len(sd.get("emitters", []))


def lds_bytes(c, block):
    """dynamic LDS of a launch with `block` threads that stages the flat scene with counts c: the tables plus one work list per wave"""
    n_prims, n_pairs, n_clusters, n_shapes, n_bsdfs, n_emitters = c
    return (64 * n_prims + 80 * (n_pairs + 1) + 32 * n_clusters + SHAPE_BYTES * n_shapes + BSDF_BYTES * n_bsdfs + EMITTER_BYTES * n_emitters +
            8 * n_prims + 4 + 4 * WL_WORDS * (block // 64))


def ring_bytes(c, spectral, gather_w):
    """k_shade with the in-kernel shadow rings: the scene at 256 threads rounded up to 16 bytes, four rings of SHADOW_RING entries of 48
    (spectral: 52) bytes and, in a gathering launch, gather_w + 1 prefix sums"""
    base = (lds_bytes(c, 64 * SHADE_WAVES) + 15) // 16 * 16
    return base + SHADE_WAVES * SHADOW_RING * (52 if spectral else 48) + (4 * (gather_w + 1) if gather_w > 4 else 0)


def launch_max(c, spectral):
    """the largest dynamic LDS any launch asks for on a flat scene of the given variant"""
    return max(lds_bytes(c, 64), lds_bytes(c, 256), ring_bytes(c, spectral, GATHER_MAX))


def is_flat(c, spectral):
    return c[0] <= FLAT_MAX and launch_max(c, spectral) <= CAP


# the launch formulas a band is defined by: name -> bytes(counts)
FORMULAS = {
    "mega": lambda c: lds_bytes(c, 64),                       # k_mega, k_finish
    "block": lambda c: lds_bytes(c, 256),                     # k_bounce*, k_direct, k_aov, adjoints, ray queries, operators
    "ring_rgb": lambda c: ring_bytes(c, False, GATHER_MAX),   # the default schedule, rgb
    "ring_spectral": lambda c: ring_bytes(c, True, GATHER_MAX),
}


VARIANT = {"mega": "rgb", "block": "rgb", "ring_rgb": "rgb", "ring_spectral": "spectral"}      # the variant each formula is run in


def _with_emitters(c, n):
    return c[:5] + (c[5] + n,)


def last_flat_extra(c, spectral):
    """the largest number of emitters that can be added to a scene with counts c (itself flat) before it stops being flat"""
    assert is_flat(c, spectral)
    n = 0
    while is_flat(_with_emitters(c, n + 1), spectral):
        n += 1
    return n


def bands(c):
    """{(formula, place): added emitters} for the places `mid` (the demand of that launch lies in (48 KiB, 64 KiB): 56 KiB is aimed at),
    `100k` (nearest to 100 KiB), `last_flat` and `first_hier`.  The scene's variant decides where flat ends: `ring_spectral` is run on
    spectral scenes, the other three on rgb ones (VARIANT).  A formula whose demand does not reach a place while the scene is still flat
    gets the last flat count."""
    out = {}
    for name, f in FORMULAS.items():
        last = last_flat_extra(c, VARIANT[name] == "spectral")
        for place, target in (("mid", 56 * 1024), ("100k", 100 * 1024)):
            n = max(0, -(-(target - f(c)) // EMITTER_BYTES))
            out[(name, place)] = min(n, last)
        out[(name, "last_flat")] = last
        out[(name, "first_hier")] = last + 1
    return out


# ---------------------------------------------------------------------------------------------------------------- scenes
_BSDF_CYCLE = (
    lambda c: dict(type="diffuse", reflectance=c),
    lambda c: dict(type="twosided", bsdf=dict(type="diffuse", reflectance=c)),
    lambda c: dict(type="roughconductor", alpha=0.25, distribution="ggx", eta=0.0, k=1.0, specular_reflectance=c),
    lambda c: dict(type="plastic", diffuse_reflectance=c),
    lambda c: dict(type="dielectric"),
)


def _mesh(tri, bsdf, emitter=-1):
    tri = np.ascontiguousarray(tri, F32)
    return dict(positions=tri.reshape(-1, 3), faces=np.arange(3 * len(tri), dtype=np.uint32).reshape(-1, 3), normals=None, texcoords=None,
                bsdf=bsdf, emitter=emitter)


def soup_triangles(n_tris, seed):
    """(n_tris, 3, 3) float32.  Triangle 0 is a backdrop that fills the view of soup_sensor() (the 1- and 2-triangle scenes need it);
    triangles 1 and 2 are coplanar and share an edge (a quad: rays at the diagonal tie exactly); triangle 3 is a sliver (1e-3 wide); the
    rest are random triangles with edges of 0.4 to 1.2 in the box [-1.4, 1.4]^2 x [-1, 1] between the camera and the backdrop."""
    rng = np.random.RandomState(seed)
    tri = np.empty((n_tris, 3, 3))
    centre = np.concatenate([rng.uniform(-1.4, 1.4, (n_tris, 2)), rng.uniform(-1.0, 1.0, (n_tris, 1))], 1)
    for k in range(n_tris):
        tri[k] = centre[k] + rng.uniform(0.2, 0.6, (3, 1)) * rng.randn(3, 3) / np.sqrt(3.0) * 1.7
    tri[0] = [[8, -5, 1.5], [-8, -5, 1.5], [0, 10, 1.5]]                     # normal towards the camera (-z)
    if n_tris > 2:
        q = np.array([[-0.9, -0.6, 0.25], [0.1, -0.7, 0.5], [0.2, 0.4, 0.525], [-0.8, 0.5, 0.275]])       # z = 0.25 x + 0.475
        tri[1], tri[2] = q[[0, 1, 2]], q[[0, 2, 3]]
    if n_tris > 3:
        tri[3] = [[0.3, -0.9, -0.2], [0.301, -0.9, -0.2], [0.9, 0.8, 0.1]]
    return tri.astype(F32)


def _partition(n_tris, partition):
    if partition == "one_shape":
        return [n_tris]
    if partition == "per_triangle":
        return [1] * n_tris
    assert partition == "mixed", partition
    sizes, cycle, k = [], (1, 3, 7, 2, 5, 9), 0                              # odd sizes: pairs straddle shapes
    while sum(sizes) < n_tris:
        sizes.append(min(cycle[k % len(cycle)], n_tris - sum(sizes)))
        k += 1
    return sizes


@functools.lru_cache(maxsize=None)
def soup(n_tris, partition, n_area_emitters, seed=1):
    """A triangle soup cut into shapes by `partition`, every shape with a BSDF record of its own (the records cycle through diffuse,
    twosided diffuse, roughconductor, plastic and dielectric), the first n_area_emitters shapes (all of them if there are fewer) with an
    area emitter of their own.  Shape 0 holds the backdrop, so any n_area_emitters >= 1 lights the whole view."""
    rng = np.random.RandomState(seed + 1000)
    tri = soup_triangles(n_tris, seed)
    sizes = _partition(n_tris, partition)
    n_em = min(n_area_emitters, len(sizes))
    meshes, bsdfs, emitters, first = [], [], [], 0
    for s, size in enumerate(sizes):
        colour = (0.2 + 0.6 * rng.rand(3)).astype(F32)
        bsdfs.append(_BSDF_CYCLE[s % len(_BSDF_CYCLE)](colour))
        if s < n_em:
            scale = 0.6 if s == 0 else 6.0                                   # the backdrop is large: keep it dim
            emitters.append(dict(type="area", radiance=(scale * (0.3 + rng.rand(3))).astype(F32)))
        meshes.append(_mesh(tri[first:first + size], s, s if s < n_em else -1))
        first += size
    return dict(meshes=meshes, bsdfs=bsdfs, emitters=emitters)


def diffuse(sd, n_records=None):
    """the same scene with one-sided diffuse BSDF records (what the adjoint replay differentiates): one per record of `sd`, or
    n_records of them that the shapes use in turn"""
    rng = np.random.RandomState(7)
    n = len(sd["bsdfs"]) if n_records is None else n_records
    bsdfs = [dict(type="diffuse", reflectance=(0.2 + 0.6 * rng.rand(3)).astype(F32)) for _ in range(n)]
    return dict(sd, bsdfs=bsdfs, meshes=[dict(m, bsdf=m["bsdf"] % n) for m in sd["meshes"]])


def soup_sensor(width=32, height=32, spp=4, seed=3, max_depth=-1):
    from mitsuba2_amd import scenes
    return dict(to_world=scenes.look_at([0.0, 0.0, -4.5], [0.0, 0.0, 0.0], [0, 1, 0]), fov=40.0, near_clip=0.01, far_clip=100.0,
                width=width, height=height, crop=(0, 0, width, height), rfilter="box", rfilter_param=0.5,
                sample_count=spp, seed=seed, max_depth=max_depth, rr_depth=5)


def many_lights(base, n_point, n_spot, n_directional, seed=2):
    """`base` plus delta emitters inside its bounding box (margin: 10 % of the extent), appended behind its own emitters: point lights,
    spots aimed at random points of the box, directional lights.  Their intensities scale with the box so that each adds about as much
    light as a dim area light would."""
    rng = np.random.RandomState(seed)
    allp = np.concatenate([np.asarray(m["positions"], np.float64).reshape(-1, 3) for m in base["meshes"]])
    lo, hi = allp.min(0), allp.max(0)
    ext = float((hi - lo).max())
    inside = lambda: lo + (hi - lo) * (0.1 + 0.8 * rng.rand(3))
    n = n_point + n_spot + n_directional
    power = 4.0 * ext * ext / max(n, 1) ** 0.5
    emitters = list(base.get("emitters", []))
    from mitsuba2_amd import scenes
    for _ in range(n_point):
        emitters.append(dict(type="point", position=inside().astype(F32), intensity=(power * (0.2 + rng.rand(3))).astype(F32)))
    for _ in range(n_spot):
        o, t = inside(), inside()
        up = [0, 1, 0] if abs((t - o)[1]) < 0.9 * np.linalg.norm(t - o) else [1, 0, 0]
        emitters.append(dict(type="spot", to_world=scenes.look_at(o, t, up), cutoff_angle=float(25 + 30 * rng.rand()),
                             intensity=(4.0 * power * (0.2 + rng.rand(3))).astype(F32)))
    for _ in range(n_directional):
        d = rng.randn(3)
        emitters.append(dict(type="directional", direction=(d / np.linalg.norm(d)).astype(F32), irradiance=(0.5 * (0.2 + rng.rand(3)) / max(n, 1) ** 0.5).astype(F32)))
    return dict(base, emitters=emitters)


def with_records(sd, n_extra):
    """`sd` with n_extra more records in its BSDF table, as a material library that the shapes only partly use: blendbsdf entries (three
    records each: the blend and its two children), then one `mask` (two records) or one plain record to reach the count exactly"""
    c = lambda v: dict(type="diffuse", reflectance=np.array([v, 0.5, 0.4], F32))
    extra, left = [], n_extra
    while left >= 3:
        extra.append(dict(type="blendbsdf", weight=0.3, bsdf1=c(0.2), bsdf2=dict(type="roughconductor", alpha=0.2, distribution="ggx", eta=0.0, k=1.0)))
        left -= 3
    if left == 2:
        extra.append(dict(type="mask", opacity=0.6, bsdf=c(0.3)))
    elif left == 1:
        extra.append(c(0.7))
    return dict(sd, bsdfs=list(sd["bsdfs"]) + extra)


def last_flat_records(c, spectral):
    """the largest number of BSDF records that can be added to a scene with counts c (itself flat) before it stops being flat"""
    assert is_flat(c, spectral)
    n = 0
    while is_flat(c[:4] + (c[4] + n + 1,) + c[5:], spectral):
        n += 1
    return n

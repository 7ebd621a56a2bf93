"""Scenes that force deep BVH4 walks, and a host-side certificate of how deep a walk must go.

Every hierarchy-scene kernel walks the BVH4 with a per-lane stack of at most 3 * wdepth + 2 entries.  k_ray_walk, k_trace and k_finish /
k_mega keep the first LDS_DEPTH of them in LDS and the rest in a global spill area; ordinary scenes hardly ever leave the LDS part.
`slivers(K)` is a scene whose every node box is nearly the whole scene box, so that a ray through the middle enters every child of every
node; the certificate program proves, per ray and independently of the order in which a walk visits children, a lower bound on the peak
stack height.  tests/test_deep_walk_cpu.py asserts the bound for the ray sets below, tests/test_gpu_deep_walk.py runs them on the device."""
import contextlib
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from mitsuba2_amd import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mitsuba2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# Stack entries per lane that stay in LDS, shared by the three spilling walks of BVH4 builds: walk_lds_depth of k_ray_walk (api.cpp,
# where the scene view is filled), kTraceLdsDepth of k_trace (MTS_TRACE_LDS_DEPTH at the shipped 256-thread workgroup) and
# kFinishLdsDepth of k_finish / k_mega (both kernels.hip).  Entry number LDS_DEPTH (counting from 0) is the first one in the spill area.
LDS_DEPTH = 8
RAY_CHUNK = 4096            # kRayChunk of k_ray_walk (kernels.hip): rays a persistent workgroup takes at a time
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- scenes
def sliver_triangles(K, seed=24, wide=0):
    """(K, 3, 3) float32: thin triangles fanned round the body diagonal of the unit cube.  Two vertices lie within 0.02 of opposite corners,
    the third at the midpoint of the diagonal, displaced perpendicular to it by 0.3 / K at the angle 2 pi i / K.  The box of every
    triangle, and therefore of every node, is nearly the whole cube.  `wide` triangles, evenly spaced round the fan, are displaced by
    0.1 instead: blades that rays really hit, in the middle of a deep walk.  Their third vertex stays inside the box of the other two, so
    the boxes, and with them the hierarchy, are those of the thin fan."""
    rng = np.random.RandomState(seed)
    axis = np.ones(3) / np.sqrt(3.0)
    e0 = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
    e1 = np.cross(axis, e0)
    ang = 2.0 * np.pi * np.arange(K) / K
    perp = np.cos(ang)[:, None] * e0 + np.sin(ang)[:, None] * e1
    width = np.full(K, 0.3 / K)
    if wide:
        width[::K // wide][:wide] = 0.1
    tri = np.empty((K, 3, 3))
    tri[:, 0] = 0.02 / np.sqrt(3.0) * rng.rand(K, 3)
    tri[:, 1] = 1.0 - 0.02 / np.sqrt(3.0) * rng.rand(K, 3)
    tri[:, 2] = 0.5 + width[:, None] * perp
    return tri.astype(F32)


def _mesh(tri, bsdf, emitter=-1):
    tri = np.ascontiguousarray(tri, F32)
    return dict(positions=tri.reshape(-1, 3), faces=np.arange(3 * len(tri), dtype=np.uint32).reshape(-1, 3), normals=None, texcoords=None,
                bsdf=bsdf, emitter=emitter)


@functools.lru_cache(maxsize=None)
def slivers(K):
    """`sliver_triangles(K)` as a one-mesh scene with a diffuse BSDF (ray queries only: no emitter)"""
    return dict(meshes=[_mesh(sliver_triangles(K), 0)], bsdfs=[dict(type="diffuse", reflectance=np.array([0.6, 0.5, 0.4], F32))], emitters=[])


RENDER_K, RENDER_WIDE = 4096, 4
CUBE_ORIGIN = np.array([-0.5, 0.7, -0.5], F32)          # the unit cube of the slivers sits above the ground, centred on (0, 1.2, 0)


@functools.lru_cache(maxsize=None)
def deep_render_scene():
    """slivers(RENDER_K) with RENDER_WIDE blades, diffuse, over a ground quad and under a small area light, laid out as scenes.bumpy_sphere: the camera of
    deep_render_sensor() looks down through the middle of the cube at the ground, the shadow rays of what it sees climb back through the
    cube to the light and the bounce rays of the ground leave upwards through it."""
    quad = lambda a, b, c, d: np.array([[a, b, c], [a, c, d]], F32)
    ground = quad([-6, 0, -6], [-6, 0, 6], [6, 0, 6], [6, 0, -6])              # normal +y
    lamp = quad([-0.5, 4, -0.5], [0.5, 4, -0.5], [0.5, 4, 0.5], [-0.5, 4, 0.5])     # normal -y
    meshes = [_mesh(sliver_triangles(RENDER_K, wide=RENDER_WIDE) + CUBE_ORIGIN, 0), _mesh(ground, 1), _mesh(lamp, 2, emitter=0)]
    bsdfs = [dict(type="diffuse", reflectance=np.array(c, F32)) for c in ([0.7, 0.4, 0.3], [0.5, 0.5, 0.5], [0, 0, 0])]
    return dict(meshes=meshes, bsdfs=bsdfs, emitters=[dict(type="area", radiance=np.array([20.0, 20.0, 20.0], F32))])


def deep_render_sensor(width=64, height=64, spp=2, seed=4, max_depth=4):
    """8192 samples; the cube fills most of the frame"""
    return dict(to_world=scenes.look_at([0.3, 3.6, -0.9], [0.0, 1.2, 0.0], [0, 1, 0]), fov=18.0, near_clip=0.01, far_clip=1e4,
                width=width, height=height, crop=(0, 0, width, height), rfilter="box", rfilter_param=0.5,
                sample_count=spp, seed=seed, max_depth=max_depth, rr_depth=5)


def triangles(sd):
    """9 floats per primitive in mesh order, as mtsamd_scene_create hands them to the builder"""
    return np.concatenate([np.asarray(m["positions"], F32).reshape(-1, 3)[np.asarray(m["faces"]).reshape(-1, 3)].reshape(-1, 9)
                           for m in sd["meshes"]])


# ---------------------------------------------------------------------------------------------------------------- ray sets
def through_rays(n, seed):
    """rays through the middle of the unit cube: origins in [0.3, 0.7]^3, uniform directions, unbounded.  They miss nearly every sliver."""
    rng = np.random.RandomState(seed)
    o = (0.3 + 0.4 * rng.rand(n, 3)).astype(F32)
    d = rng.randn(n, 3)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    return o, d, np.full(n, 1e-4, F32), np.full(n, np.inf, F32)


def aimed_rays(K, n, seed):
    """rays aimed at points inside slivers, so that real hits occur; a third of them with a finite maxt around the hit distance"""
    rng = np.random.RandomState(seed)
    tri = sliver_triangles(K).astype(np.float64)[rng.randint(0, K, n)]
    b = rng.dirichlet([1.0, 1.0, 1.0], n)
    target = (b[:, :, None] * tri).sum(1)
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    d = normal * np.where(rng.rand(n, 1) < 0.5, -1.0, 1.0) + 0.4 * rng.randn(n, 3)      # steep enough to meet a thin triangle
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = 0.05 + 0.5 * rng.rand(n)
    o = target - d * dist[:, None]
    maxt = np.where(rng.rand(n) < 1.0 / 3.0, dist * (0.5 + rng.rand(n)), np.inf)
    return o.astype(F32), d.astype(F32), np.full(n, 1e-4, F32), maxt.astype(F32)


def box_rays(sd, n, seed):
    """rays as the ray-query tests of the older scenes draw them (tests/test_gpu_parity.py, _rays): origins in the scene box, uniform
    directions, three in ten with a finite maxt up to the box diagonal"""
    rng = np.random.RandomState(seed)
    allp = np.concatenate([m["positions"] for m in sd["meshes"]])
    lo, hi = allp.min(0), allp.max(0)
    o = (lo + (hi - lo) * rng.rand(n, 3)).astype(F32)
    d = rng.randn(n, 3)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    mint = np.full(n, 1e-4, F32)
    maxt = np.where(rng.rand(n) < 0.3, rng.rand(n) * np.linalg.norm(hi - lo), np.inf).astype(F32)
    return o, d, mint, maxt


QUERY_K, QUERY_THROUGH, QUERY_AIMED = 4096, 8000, 2000
STREAM_K, STREAM_TILE = 1024, 4096


@functools.lru_cache(maxsize=None)
def query_rays():
    """the ray set of the deep-walk query tests on slivers(QUERY_K): QUERY_THROUGH rays of through_rays, then QUERY_AIMED aimed ones"""
    a, b = through_rays(QUERY_THROUGH, 21), aimed_rays(QUERY_K, QUERY_AIMED, 22)
    return tuple(np.concatenate([x, y]) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def stream_tile():
    """the rays a long stream on slivers(STREAM_K) is tiled from"""
    return through_rays(STREAM_TILE, 23)


def stream_index(n):
    """ray i of a stream of n is ray stream_index(n)[i] of stream_tile(): a fixed permutation, so that neighbouring lanes walk different rays"""
    i = np.arange(n, dtype=np.int64)
    return ((i * 2654435761 + (i // STREAM_TILE) * 40503) % STREAM_TILE).astype(np.int64)


def primary_rays(ob, n=4096, seed=31):
    """camera rays of deep_render_sensor() at uniform film positions (ob: the oracle binding), cut off at the plane y = 0.3 between the
    cube and the ground.  Every primary ray ends on the ground, so none misses every triangle; but until a walk has found that hit at
    t_ground it culls nothing nearer, and afterwards only what starts beyond t_ground: every child box that the segment up to y = 0.3
    pierces is entered either way.  A segment that misses every triangle thus certifies the walk of the whole ray."""
    s = np.random.RandomState(seed).rand(n, 2).astype(F32)
    o, d, mint, maxt = ob.camera_rays(ob.make_desc(deep_render_sensor()), s[:, 0].copy(), s[:, 1].copy())
    assert (d[:, 1] < 0).all() and (o[:, 1] > 0.3).all()
    return o, d, mint, np.minimum(maxt, (o[:, 1] - F32(0.3)) / -d[:, 1]).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- certificate
# Stand-alone host program.  Input: a file of [n_tri, n_ray as uint32][n_tri x 9 floats][n_ray x 8 floats: o, d, mint, maxt].
# Output: "n_tri wdepth longest n_wnodes", then one line "P replay" per ray, or "-1 -1" for a ray that does not provably miss every triangle.
#   longest: max over root-to-leaf paths of sum(children - 1), + 2 -- the trivial side of the stack bound 3 * wdepth + 2
#   P:       order-independent minimum peak stack height of an exhaustive depth-first walk.  A child counts as entered only if the ray
#            segment pierces its box on the 16-bit grid (BvhOutput::wnodes) shrunk by one cell on every side; the boxes the device tests
#            (fp16 or 15-bit planes rounded outward from that grid, slab intervals padded for rounding) contain it, so the device enters a
#            superset of these children.  For a node with entered children of minimum peaks p_1 .. p_h,
#            P(node) = min over visiting orders of max_k((h - 1 - k) + p_order[k]), leaves 0: while child k is walked, the h - 1 - k
#            later ones wait on the stack.  A ray that misses every triangle never shortens its segment, so its walk is exhaustive in any
#            order and its peak stack height is at least P, whatever the sort network does.
#   replay:  peak of a nearest-first walk over the unshrunk grid boxes (what the closest-hit walk does, up to padding): an estimate
# Misses are decided by brute force in double precision with a margin (barycentrics within 1e-3, t within 1e-3 relative) that counts
# grazing rays as hits.
PROGRAM = r"""
#include "bvh.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
using namespace mtsamd;

static const double kInf = std::numeric_limits<double>::infinity();
static BvhOutput g_bvh;
struct Ray { double o[3], d[3], mint, maxt; };

static bool may_hit(const float *tp, const Ray &r) {
    double p0[3], e1[3], e2[3], s[3], p[3], q[3];
    for (int k = 0; k < 3; ++k) { p0[k] = tp[k]; e1[k] = (double) tp[3 + k] - p0[k]; e2[k] = (double) tp[6 + k] - p0[k]; s[k] = r.o[k] - p0[k]; }
    auto cross = [](const double *a, const double *b, double *c) { c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0]; };
    auto dot = [](const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    cross(r.d, e2, p);
    const double det = dot(e1, p);
    if (std::fabs(det) <= 1e-9 * std::sqrt(dot(e1, e1) * dot(e2, e2) * dot(r.d, r.d))) return true;      // parallel: undecided, so not a miss
    const double eps = 1e-3, u = dot(s, p) / det;
    cross(s, e1, q);
    const double v = dot(r.d, q) / det, t = dot(e2, q) / det;
    if (u < -eps || v < -eps || u + v > 1.0 + eps) return false;
    return t >= r.mint - eps * std::fabs(t) - 1e-6 && t <= r.maxt + eps * std::fabs(t) + 1e-6;
}

// entry distance of the ray segment into child c of node `node` with its grid box shrunk by `shrink` cells, +inf if it misses
static double enter(uint32_t node, int c, const Ray &r, double shrink) {
    const uint32_t *w = g_bvh.wnodes.data() + 16 * (size_t) node + 4 * c;
    double tn = r.mint, tf = r.maxt;
    for (int k = 0; k < 3; ++k) {
        const double lo = (double) g_bvh.q_lo[k] + ((double) (w[k] & 0xffffu) + shrink) * (double) g_bvh.q_step[k];
        const double hi = (double) g_bvh.q_lo[k] + ((double) (w[k] >> 16) - shrink) * (double) g_bvh.q_step[k];
        if (!(lo <= hi)) return kInf;
        if (r.d[k] == 0.0) { if (r.o[k] < lo || r.o[k] > hi) return kInf; continue; }
        double a = (lo - r.o[k]) / r.d[k], b = (hi - r.o[k]) / r.d[k];
        if (a > b) std::swap(a, b);
        tn = std::max(tn, a); tf = std::min(tf, b);
    }
    return tn <= tf ? tn : kInf;
}
static bool is_leaf(uint32_t ref) { return (ref & 0x80000000u) != 0u; }
static const uint32_t kAbsent = 0x7fffffffu;

static int min_peak(uint32_t ref, const Ray &r) {
    if (is_leaf(ref)) return 0;
    int p[4], h = 0;
    for (int c = 0; c < 4; ++c) {
        const uint32_t child = g_bvh.wnodes[16 * (size_t) ref + 4 * c + 3];
        if (child != kAbsent && enter(ref, c, r, 1.0) < kInf) p[h++] = min_peak(child, r);
    }
    if (h == 0) return 0;
    int order[4] = { 0, 1, 2, 3 }, best = 1 << 30;
    do {
        int peak = 0;
        for (int k = 0; k < h; ++k) peak = std::max(peak, (h - 1 - k) + p[order[k]]);
        best = std::min(best, peak);
    } while (std::next_permutation(order, order + h));
    return best;
}

static void replay(uint32_t ref, const Ray &r, int sp, int &peak) {
    peak = std::max(peak, sp);
    if (is_leaf(ref)) return;
    std::pair<double, uint32_t> hit[4];
    int h = 0;
    for (int c = 0; c < 4; ++c) {
        const uint32_t child = g_bvh.wnodes[16 * (size_t) ref + 4 * c + 3];
        const double t = child != kAbsent ? enter(ref, c, r, 0.0) : kInf;
        if (t < kInf) hit[h++] = { t, child };
    }
    std::stable_sort(hit, hit + h, [](const std::pair<double, uint32_t> &a, const std::pair<double, uint32_t> &b) { return a.first < b.first; });
    for (int k = 0; k < h; ++k) replay(hit[k].second, r, sp + (h - 1 - k), peak);
}

static uint32_t longest(uint32_t ref) {
    if (is_leaf(ref)) return 0u;
    uint32_t n = 0u, deepest = 0u;
    for (int c = 0; c < 4; ++c) {
        const uint32_t child = g_bvh.wnodes[16 * (size_t) ref + 4 * c + 3];
        if (child != kAbsent) { ++n; deepest = std::max(deepest, longest(child)); }
    }
    return n - 1u + deepest;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t head[2];
    if (std::fread(head, sizeof(uint32_t), 2, f) != 2 || head[0] == 0u) return 3;
    std::vector<float> tri(9 * (size_t) head[0]), rays(8 * (size_t) head[1]);
    if (std::fread(tri.data(), sizeof(float), tri.size(), f) != tri.size()) return 3;
    if (std::fread(rays.data(), sizeof(float), rays.size(), f) != rays.size()) return 3;
    std::fclose(f);
    build_bvh(tri.data(), head[0], 4u, g_bvh);        // max_leaf and options as mtsamd_scene_create has them
    std::printf("%u %u %u %u\n", head[0], g_bvh.wdepth, longest(g_bvh.wroot) + 2u, g_bvh.n_wnodes);
    for (uint32_t i = 0; i < head[1]; ++i) {
        const float *p = rays.data() + 8 * (size_t) i;
        Ray r;
        for (int k = 0; k < 3; ++k) { r.o[k] = p[k]; r.d[k] = p[3 + k]; }
        r.mint = p[6]; r.maxt = p[7];
        bool miss = true;
        for (uint32_t t = 0; t < head[0] && miss; ++t) miss = !may_hit(tri.data() + 9 * (size_t) t, r);
        if (!miss) { std::printf("-1 -1\n"); continue; }
        int peak = 0;
        replay(g_bvh.wroot, r, 0, peak);
        std::printf("%d %d\n", min_peak(g_bvh.wroot, r), peak);
    }
    return 0;
}
"""


class Certificate:
    """builds PROGRAM once (hipcc as a host compiler, bvh.cpp linked in) and runs it: __call__(triangles (n, 9), rays) ->
    dict(n, wdepth, longest, n_wnodes, P (-1: the ray may hit a triangle), replay)"""

    def __init__(self, tmp, flags=()):
        self.tmp = tmp
        src, self.exe = os.path.join(tmp, "cert.cpp"), os.path.join(tmp, "cert")
        with open(src, "w") as f:
            f.write(PROGRAM)
        build = subprocess.run([HIPCC, "-std=c++17", "-O2", *flags, "-I", CSRC, "-o", self.exe, src, os.path.join(CSRC, "bvh.cpp")],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert build.returncode == 0, build.stdout

    def __call__(self, tri, rays=None):
        tri = np.ascontiguousarray(tri, F32).reshape(-1, 9)
        if rays is None:
            rays = (np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros(0, F32), np.zeros(0, F32))
        o, d, mint, maxt = rays
        packed = np.concatenate([o, d, mint[:, None], maxt[:, None]], axis=1).astype(F32)
        path = os.path.join(self.tmp, "in.bin")
        with open(path, "wb") as f:
            np.array([len(tri), len(packed)], np.uint32).tofile(f)
            tri.tofile(f)
            packed.tofile(f)
        out = subprocess.check_output([self.exe, path]).split()
        head, body = [int(x) for x in out[:4]], np.array(out[4:], dtype=np.int64).reshape(-1, 2)
        assert head[0] == len(tri) and len(body) == len(packed)
        return dict(n=head[0], wdepth=head[1], longest=head[2], n_wnodes=head[3], P=body[:, 0], replay=body[:, 1])


@contextlib.contextmanager
def make_certificate(flags=()):
    """a Certificate in a temporary directory"""
    with tempfile.TemporaryDirectory() as tmp:
        yield Certificate(tmp, flags)


def compiler_has_runtime(flags):
    """whether an empty program links with `flags` (the sanitizer runtimes are an optional part of the compiler's installation)"""
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "empty.cpp")
        with open(src, "w") as f:
            f.write("int main() { return 0; }\n")
        return subprocess.run([HIPCC, *flags, "-o", os.path.join(tmp, "empty"), src], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0

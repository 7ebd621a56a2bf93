"""Work-list helpers of the flat-scene queries (mitsuba2_amd/csrc/flat_worklist.h), compiled here for the host: the minimum of the
64-bit closest-hit keys picks what the sequential loop "t <= best" over the primitives picks (later primitives win ties, -0 == +0),
on random and adversarial (t, primitive) sequences; item encoding and the per-lane item lists are a bijection onto the (lane, pair)
pairs of the reach masks."""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mitsuba2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

PROGRAM = r"""
#include "flat_worklist.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
using namespace mtsamd;
static uint32_t bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }

// the sequential loop of traverse_flat: accepted candidates in primitive order, "t <= best" from best = maxt
static bool sequential(const std::vector<float> &t, const std::vector<bool> &ok, float maxt, float &bt, uint32_t &bp) {
    float best = maxt; uint32_t best_prim = ~0u;
    for (uint32_t p = 0; p < t.size(); ++p) if (ok[p] && t[p] <= best) { best = t[p]; best_prim = p; }
    bt = best; bp = best_prim;
    return best_prim != ~0u;
}

int main() {
    std::mt19937 rng(7);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float pool[] = { 0.0f, -0.0f, 1e-45f, -1e-45f, 1e-38f, 1e-4f, 0.5f, 0.5f, 1.0f, 1.0f, std::nextafter(1.0f, 2.0f),
                           std::nextafter(1.0f, 0.0f), 3.0e38f, inf, -1.0f, -0.5f, -inf, nan, 2.0f, 2.0f };
    const int n_pool = sizeof(pool) / sizeof(pool[0]);
    for (int trial = 0; trial < 200000; ++trial) {
        const uint32_t n = 1u + rng() % 64u;
        const int kind = trial % 3;
        std::vector<float> t(n); std::vector<bool> ok(n);
        for (uint32_t p = 0; p < n; ++p) {
            if (kind == 0) t[p] = pool[rng() % n_pool];                                         // adversarial: zeros, ties, extremes, NaN
            else if (kind == 1) t[p] = (float) (rng() % 4u) * 0.25f * ((rng() & 1u) ? 1.0f : -1.0f);   // many exact ties, +-0
            else t[p] = std::ldexp((float) (rng() % 1000u), (int) (rng() % 40u) - 20);
            ok[p] = (rng() % 4u) != 0u;
        }
        const float mint = (trial & 4) ? 0.0f : ((trial & 8) ? -1.0f : 1e-4f);
        const float maxt = (trial & 16) ? inf : pool[rng() % n_pool];
        // acceptance as tri_accept: t >= mint && t <= maxt (NaN fails)
        for (uint32_t p = 0; p < n; ++p) ok[p] = ok[p] && t[p] >= mint && t[p] <= maxt;
        float bt; uint32_t bp;
        const bool found = sequential(t, ok, maxt, bt, bp);
        // the minimum of the keys, in a shuffled order of the items, the two triangles of a pair reduced first as the kernel does
        std::vector<uint32_t> order(n);
        for (uint32_t p = 0; p < n; ++p) order[p] = p;
        std::shuffle(order.begin(), order.end(), rng);
        uint64_t key = kWlNoKey;
        for (uint32_t p : order) if (ok[p]) { const uint64_t k = wl_key(t[p], p); if (k < key) key = k; }
        if ((key != kWlNoKey) != found) { std::printf("found differs: trial %d\n", trial); return 1; }
        if (found) {
            const uint32_t prim = wl_key_prim(key);
            if (prim != bp || bits(t[prim]) != bits(bt)) { std::printf("trial %d: key -> %u (t %a), sequential -> %u (t %a)\n", trial, prim, t[prim], bp, bt); return 1; }
        }
    }
    // the order of wl_t_order agrees with the float order on every pair of a dense sample of floats
    std::vector<float> xs = { -inf, -3e38f, -1.0f, -1e-38f, -1e-45f, -0.0f, 0.0f, 1e-45f, 1e-38f, 1.0f, 3e38f, inf };
    for (int i = 0; i < 2000; ++i) { uint32_t b = rng(); float x; std::memcpy(&x, &b, 4); if (!std::isnan(x)) xs.push_back(x); }
    for (float a : xs) for (float b : xs)
        if ((a < b) != (wl_t_order(a) < wl_t_order(b)) || (a == b) != (wl_t_order(a) == wl_t_order(b))) { std::printf("order: %a %a\n", a, b); return 1; }
    // items: encode / decode, and the lists of all lanes (exclusive prefix of the counts) cover every (lane, pair) once
    for (uint32_t lane = 0; lane < 64u; ++lane)
        for (uint32_t pair = 0; pair <= 32u; ++pair) {
            const uint32_t it = wl_item(lane, pair);
            if (it > 0xffffu || wl_item_owner(it) != lane || wl_item_pair(it) != pair) { std::printf("item %u %u\n", lane, pair); return 1; }
        }
    for (int trial = 0; trial < 2000; ++trial) {
        const uint32_t n_lanes = 1u + rng() % 64u;
        std::vector<uint32_t> mask(n_lanes), pos(n_lanes);
        uint32_t total = 0;
        for (uint32_t l = 0; l < n_lanes; ++l) {
            mask[l] = (trial % 5 == 0) ? 0xffffffffu : rng() & rng();
            pos[l] = total; total += (uint32_t) __builtin_popcount(mask[l]);
        }
        std::vector<uint16_t> tbl(total + 1u, 0xbeefu);
        for (uint32_t l = 0; l < n_lanes; ++l) wl_push_items(tbl.data(), pos[l], mask[l], l);
        if (tbl[total] != 0xbeefu) { std::printf("list overrun\n"); return 1; }
        std::vector<uint32_t> seen(n_lanes, 0u);
        for (uint32_t j = 0; j < total; ++j) {
            const uint32_t l = wl_item_owner(tbl[j]), p = wl_item_pair(tbl[j]);
            if (l >= n_lanes || p >= 32u || !(mask[l] >> p & 1u) || (seen[l] >> p & 1u)) { std::printf("bad item %u\n", j); return 1; }
            if (j > pos[l] && wl_item_pair(tbl[j - 1]) >= p) { std::printf("pairs out of order\n"); return 1; }
            seen[l] |= 1u << p;
        }
        for (uint32_t l = 0; l < n_lanes; ++l) if (seen[l] != mask[l]) { std::printf("missing items of lane %u\n", l); return 1; }
    }
    std::printf("ok\n");
    return 0;
}
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_worklist_key_reproduces_sequential_loop():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "t.cpp"), os.path.join(tmp, "t")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-I", CSRC, "-o", exe, src],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        out = subprocess.check_output([exe]).decode()
        assert out.strip() == "ok", out

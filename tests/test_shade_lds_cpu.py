"""LDS and occupancy of the headline kernel, k_shade<PathState, false, true, true> (Cornell box, shadow-ring schedule), from the
compiler's resource remarks: its static LDS stays small (the gathering prefix sums live in dynamic LDS, added only to the launches
that gather), it keeps 4 waves per SIMD, and static plus the dynamic LDS the host computes for the Cornell box (kernels.h,
shade_ring_lds_bytes) fit 4 workgroups in the 160 KiB of a CU."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "mitsuba2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADLINE = "_ZN6mtsamd7k_shadeINS_9PathStateELb0ELb1ELb1EEEvNS_12RenderParamsE"
LDS_PER_CU = 160 * 1024

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")


def makefile_flags():
    """CXXFLAGS of the library's Makefile (without $(EXTRA)): the remarks must describe the code the library ships."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    line = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1)
    return [f for f in line.split() if not f.startswith("$(")]


@pytest.fixture(scope="module")
def headline_resources():
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-c", "-o", os.path.join(tmp, "kernels.o"),
               "-Rpass-analysis=kernel-resource-usage"] + makefile_flags() + [os.path.join(CSRC, "kernels.hip")]
        out = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert out.returncode == 0, out.stderr[-4000:]
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"remark:\s+([^:]+?): (\S+) \[-Rpass-analysis", line)
        if m and cur == HEADLINE:
            res[m.group(1)] = m.group(2)
    assert res, "no resource remarks for " + HEADLINE
    return res


def cbox_dynamic_lds():
    """shade_ring_lds_bytes() of the Cornell box as launch_bounce computes it (steady state: no gathering)."""
    sys.path.insert(0, ROOT)
    from mitsuba2_amd import scenes
    sd = scenes.cornell_box()
    prim_shape = [i for i, m in enumerate(sd["meshes"]) for _ in range(len(m["faces"]))]
    n_prims = len(prim_shape)
    n_pairs = (n_prims + 1) // 2
    n_clusters = sum(1 for k in range(n_pairs) if k == 0 or prim_shape[2 * k] != prim_shape[2 * (k - 1)])
    program = r"""
#include "kernels.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv) {
    mtsamd::SceneView sv = {};
    sv.flat = 1u;
    sv.n_prims = (uint32_t) atoi(argv[1]); sv.n_pairs = (uint32_t) atoi(argv[2]); sv.n_clusters = (uint32_t) atoi(argv[3]);
    sv.n_shapes = (uint32_t) atoi(argv[4]); sv.n_bsdfs = (uint32_t) atoi(argv[5]); sv.n_emitters = (uint32_t) atoi(argv[6]);
    printf("%zu %zu %zu\n", mtsamd::shade_ring_lds_bytes(sv, false, 4u), mtsamd::shade_ring_lds_bytes(sv, true, 4u),
           mtsamd::shade_ring_lds_bytes(sv, false, 1024u));
    return 0;
}
"""
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "lds.hip"), os.path.join(tmp, "lds")
        open(src, "w").write(program)
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                               "-o", exe, src])
        args = [str(x) for x in (n_prims, n_pairs, n_clusters, len(sd["meshes"]), len(sd["bsdfs"]), len(sd["emitters"]))]
        rgb, spectral, gather = (int(x) for x in subprocess.check_output([exe] + args, text=True).split())
    return rgb, spectral, gather


def test_headline_static_lds(headline_resources):
    assert int(headline_resources["LDS Size [bytes/block]"]) <= 512, headline_resources


def test_headline_occupancy(headline_resources):
    assert int(headline_resources["Occupancy [waves/SIMD]"]) == 4, headline_resources


def test_headline_four_workgroups_per_cu(headline_resources):
    static = int(headline_resources["LDS Size [bytes/block]"])
    rgb, spectral, gather = cbox_dynamic_lds()
    assert 4 * (static + rgb) <= LDS_PER_CU, (static, rgb)
    # the RGB ring entry is 4 bytes smaller than the spectral one; gathering launches add their gather_w + 1 prefix sums only
    assert spectral - rgb == 4 * 4 * 128
    assert gather - rgb == 4 * 1025

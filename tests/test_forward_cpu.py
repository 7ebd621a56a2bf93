"""The host half of the forward-mode derivative render without a GPU: build_tangent_records (mitsuba2_amd/csrc/scene_build.cpp) through
tests/forward_tangent_driver.cpp, a stand-alone program compiled with the host-only scene builder the way scene_build_driver.cpp is.

* a tangent that is 1 on one scalar and 0 elsewhere gives, bit for bit, the records and the 1 / (2 h) that mtsamd_render_adjoint_param
  builds for that scalar (the rule is written out here in float32, independently of the driver), for every (type, kind, component)
  bsdf_param_fields accepts, at the default step and at an explicit one; every other (type, kind, component) is refused by name;
* the step of a tangent over several scalars is the largest that moves no scalar beyond its limit;
* ALPHA and ETA stay above 1e-4, and a value that leaves no room is refused;
* non-finite tangents, ALPHA components 1 and 2, textured reflectances and blendbsdf records are refused with their messages;
* the driver built with -fsanitize=address,undefined runs the same cases clean (a stand-alone program: nothing is preloaded);
* the entry points of the library refuse null arguments before they touch a device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mitsuba2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
F32 = np.float32
INVALID, UNSUPPORTED = -1, -5
REFLECTANCE, SPECULAR_REFLECTANCE, ETA, K, ALPHA, SPECULAR_TRANSMITTANCE = range(6)
FIELDS = ("r", "g", "b", "sr", "sg", "sb", "er", "eg", "eb", "kr", "kg", "kb", "alpha_u", "alpha_v")
# type, texture, then FIELDS: one record per model (device_bsdf.h: 0 diffuse, 1 conductor, 2 roughconductor, 3 dielectric, 4 plastic,
# 5 roughplastic, 6 roughdielectric, 7 thindielectric), a textured diffuse, an anisotropic roughconductor, a blendbsdf
RECORDS = [
    (0, -1, .5, .25, .75, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (1, -1, 0, 0, 0, .9, .8, 1., .2, 1.1, 1.4, 3.9, 2.4, 2.2, 0, 0),
    (2, -1, 0, 0, 0, 1., .7, .01, .15, .0002, 1.3, 3.5, .002, 6.5, .15, .15),
    (3, -1, 0, 0, 0, 1., .9, .8, 1.5, 0, 0, .95, .9, 1., 0, 0),
    (4, -1, .1, .27, .36, 1., .6, .3, 1.49, .4, .03, .6, 0, 0, 0, 0),
    (5, -1, .02, .9, .36, .8, .8, .8, 1.49, .4, .03, .6, 0, 0, .1, .1),
    (6, -1, 0, 0, 0, 1., 1., 1., 1.5, 0, 0, 1., .5, .04, .3, .3),
    (7, -1, 0, 0, 0, 1., .5, .2, 1.5, 0, 0, .7, .8, .9, 0, 0),
    (0, 0, .5, .5, .5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (2, -1, 0, 0, 0, 1., 1., 1., .2, .9, 1.1, 3.9, 2.4, 2.2, .1, .2),
    (8, -1, .5, .5, .5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
]
STEPS = (0.0, 0.003)


def accepted(rec, kind, comp):
    """the parameters mtsamd_render_adjoint_param accepts, from its description in include/mtsamd.h: the fields they move, or None"""
    t, texture = rec[0], rec[1]
    conductor, dielectric = t in (1, 2), t in (3, 6, 7)
    if t >= 8:
        return None
    if kind == REFLECTANCE:
        return (comp,) if texture < 0 and t in (0, 4, 5) else None
    if kind == SPECULAR_REFLECTANCE:
        return (3 + comp,) if t != 0 else None
    if kind == ETA:
        return (6 + comp,) if conductor else None
    if kind in (K, SPECULAR_TRANSMITTANCE):
        return (9 + comp,) if (conductor if kind == K else dielectric) else None
    return (12, 13) if t in (2, 6) and rec[2 + 12] == rec[2 + 13] and comp == 0 else None


def adjoint_param_rule(theta, kind, h):
    """plus, minus and 1 / (2 h) of mtsamd_render_adjoint_param for one scalar, in float32"""
    theta, h = F32(theta), F32(h)
    if not h > 0:
        h = F32(0.01) * max(abs(theta), F32(0.05))
    if kind in (ALPHA, ETA) and theta - h <= F32(1e-4):
        h = F32(0.5) * (theta - F32(1e-4))
    return theta + h, theta - h, F32(1.0) / ((theta + h) - (theta - h))


def bits(x):
    return np.asarray(x, F32).view(np.uint32)


def _case_lines():
    """the case file and what each label is: (record, kind, comp, h) for the one-hot runs"""
    lines, one_hot = [], {}

    def table(records):
        lines.append("clear")
        for r in records:
            lines.append("record " + " ".join(repr(float(x)) if i >= 2 else str(x) for i, x in enumerate(r)))

    def tangent(b, entries):
        t = ["0"] * 18
        for (kind, comp), v in entries.items():
            t[3 * kind + comp] = v if isinstance(v, str) else repr(float(v))
        lines.append("tangent %d %s" % (b, " ".join(t)))

    table(RECORDS)
    for b, rec in enumerate(RECORDS):
        for kind in range(6):
            for comp in range(3):
                for si, h in enumerate(STEPS):
                    label = "hot_%d_%d_%d_%d" % (b, kind, comp, si)
                    tangent(b, {(kind, comp): 1.0})
                    lines.append("run %s %r" % (label, h))
                    one_hot[label] = (b, kind, comp, h)
                tangent(b, {})
    lines.append("null untouched 0.01")
    # a tangent over several scalars of the roughconductor (record 2): specular_reflectance.r 2, eta.r -0.5, alpha 4, k.b 1
    tangent(2, {(SPECULAR_REFLECTANCE, 0): 2.0, (ETA, 0): -0.5, (ALPHA, 0): 4.0, (K, 2): 1.0})
    lines.append("run several_h 0.01")
    lines.append("run several_default 0")
    tangent(2, {})
    # floors: alpha just above 1e-4; eta.g of record 2 is 0.0002; alpha at the floor leaves no room
    table([(2, -1, 0, 0, 0, 1., 1., 1., .2, .9, 1.1, 3.9, 2.4, 2.2, .0002, .0002), (1, -1, 0, 0, 0, 1., 1., 1., .00015, 1.1, 1.4, 3.9, 2.4, 2.2, 0, 0),
           (6, -1, 0, 0, 0, 1., 1., 1., 1.5, 0, 0, 1., 1., 1., .0001, .0001)])
    tangent(0, {(ALPHA, 0): 2.0, (K, 0): 1.0})
    tangent(1, {(ETA, 0): 1.0})
    lines.append("run floors 0.01")
    tangent(2, {(ALPHA, 0): 1.0})
    lines.append("run no_room 0.01")
    tangent(2, {})
    for name, value in (("nan", "nan"), ("inf", "inf"), ("minus_inf", "-inf")):
        tangent(1, {(K, 1): value})
        lines.append("run %s 0" % name)
    return lines, one_hot


def _build(directory, flags=()):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = os.path.join(str(directory), "forward_tangent_driver")
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, "-o", exe] + list(flags) +
                          ["-x", "hip", "--cuda-host-only", os.path.join(HERE, "forward_tangent_driver.cpp"), os.path.join(CSRC, "scene_build.cpp"), "-x", "c++"] +
                          [os.path.join(CSRC, f) for f in ("bvh.cpp", "envmap.cpp", "spectral_upsampling.cpp")], stderr=subprocess.DEVNULL)
    return exe


def _run(exe, directory):
    lines, one_hot = _case_lines()
    path = os.path.join(str(directory), "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = {}
    for line in subprocess.check_output([exe, path], text=True).splitlines():
        label, what, rest = (line.split(" ", 2) + [""])[:3]
        entry = out.setdefault(label, {"plus": {}, "minus": {}})
        if what == "rc":
            entry["rc"] = int(rest)
        elif what == "msg":
            entry["msg"] = rest
        elif what == "inv_2h":
            entry["inv_2h"] = np.array([int(w, 16) for w in rest.split()], np.uint32).view(F32)
        else:
            b, words = rest.split(" ", 1)
            entry[what][int(b)] = np.array([int(w, 16) for w in words.split()], np.uint32).view(F32)
    return out, one_hot


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("forward_tangent")
    return _run(_build(d), d)


def _check_one_hot(out, one_hot):
    n_accepted = 0
    for label, (b, kind, comp, h) in one_hot.items():
        rec, got = RECORDS[b], out[label]
        fields = accepted(rec, kind, comp)
        if fields is None:
            assert got["rc"] == UNSUPPORTED, (label, got)
            assert got["msg"].startswith("bsdf %d (type %d) has no differentiable parameter of kind %d" % (b, rec[0], kind)), got["msg"]
            continue
        n_accepted += 1
        assert got["rc"] == 0, (label, got)
        plus, minus, inv = adjoint_param_rule(rec[2 + fields[0]], kind, h)
        for other, row in enumerate(RECORDS):
            want_p, want_m = np.array(row[2:], F32), np.array(row[2:], F32)
            if other == b:
                want_p[list(fields)], want_m[list(fields)] = plus, minus
            assert np.array_equal(bits(got["plus"][other]), bits(want_p)) and np.array_equal(bits(got["minus"][other]), bits(want_m)), (label, other)
        want_inv = np.zeros(len(RECORDS), F32)
        want_inv[b] = inv
        assert np.array_equal(bits(got["inv_2h"]), bits(want_inv)), (label, got["inv_2h"], inv)
    return n_accepted


def test_one_hot_tangents_are_the_records_of_the_parameter_adjoint(results):
    out, one_hot = results
    # accepted (type, kind, component) triples per record of RECORDS, two steps each
    assert _check_one_hot(out, one_hot) == 2 * (3 + 9 + 10 + 6 + 6 + 6 + 7 + 6 + 0 + 9 + 0)
    got = out["untouched"]
    assert got["rc"] == 0 and not got["inv_2h"].any()
    for b, row in enumerate(RECORDS):
        assert np.array_equal(bits(got["plus"][b]), bits(row[2:])) and np.array_equal(bits(got["minus"][b]), bits(row[2:]))


def test_the_step_of_a_tangent_over_several_scalars(results):
    out, _ = results
    theta = np.array(RECORDS[2][2:], F32)
    t = np.zeros(14, np.float64)
    t[3], t[6], t[12], t[13], t[11] = 2.0, -0.5, 4.0, 4.0, 1.0
    for label, limits in (("several_h", np.full(14, 0.01)), ("several_default", 0.01 * np.maximum(np.abs(theta.astype(np.float64)), 0.05))):
        got = out[label]
        assert got["rc"] == 0, got
        eps = float(np.min(limits[t != 0] / np.abs(t[t != 0])))          # the largest step that moves no scalar beyond its limit
        moved_p = got["plus"][2].astype(np.float64) - theta, theta - got["minus"][2].astype(np.float64)
        for moved in moved_p:
            # theta + eps t in float32: half a unit in the last place of the largest value (6.5) is 2.4e-7
            assert np.abs(moved - eps * t).max() <= 5e-7, (label, moved, eps * t)
            assert (np.abs(moved) <= limits * (1 + 1e-6) + 5e-7).all()
            assert (moved[t == 0] == 0).all()
        # some scalar sits at its limit, and 1 / (2 eps) is taken from the scalar with the largest |t| (alpha)
        assert np.isclose(np.max(np.abs(eps * t) / limits), 1.0, rtol=1e-6)
        want = F32(4.0) / (got["plus"][2][12] - got["minus"][2][12])
        assert bits(got["inv_2h"][2]) == bits(want) and abs(float(want) * 2 * eps - 1) < 1e-4
        assert not got["inv_2h"][[0, 1] + list(range(3, len(RECORDS)))].any()
        for other in range(len(RECORDS)):
            if other != 2:
                assert np.array_equal(bits(got["plus"][other]), bits(RECORDS[other][2:]))


def test_alpha_and_eta_stay_above_their_floor(results):
    out, _ = results
    got = out["floors"]
    assert got["rc"] == 0, got
    # record 0: alpha 2e-4 with tangent 2 and k.r with tangent 1: eps = min(.01 / 2, .01) would take alpha below 1e-4;
    # the shrunk step is 0.5 (alpha - 1e-4) / 2
    eps = 0.5 * (float(F32(2e-4)) - float(F32(1e-4))) / 2
    assert 1e-4 < got["minus"][0][12] == got["minus"][0][13] and np.isclose(got["minus"][0][12], 2e-4 - 2 * eps, rtol=1e-5)
    assert np.isclose(got["plus"][0][12], 2e-4 + 2 * eps, rtol=1e-5) and np.isclose(got["plus"][0][9] - F32(3.9), eps, rtol=1e-2)
    # record 1: a one-hot on eta.r = 1.5e-4 is the rule of the parameter adjoint
    plus, minus, inv = adjoint_param_rule(.00015, ETA, 0.01)
    assert bits(got["plus"][1][6]) == bits(plus) and bits(got["minus"][1][6]) == bits(minus) and bits(got["inv_2h"][1]) == bits(inv)
    assert minus > F32(1e-4)
    assert got["inv_2h"][2] == 0
    bad = out["no_room"]
    assert bad["rc"] == INVALID and bad["msg"] == "bsdf 2: parameter value 0.0001 leaves no room for a central difference", bad


def test_refusals_and_their_messages(results):
    out, one_hot = results
    for name in ("nan", "inf", "minus_inf"):
        assert out[name]["rc"] == INVALID and out[name]["msg"] == "bsdf 1: the tangent of parameter kind 3 is not finite", out[name]
    # ALPHA takes component 0 only; a textured reflectance and a blendbsdf record have no constant to move
    for label, (b, kind, comp, h) in one_hot.items():
        if (kind == ALPHA and comp > 0) or b in (8, 10) and kind == REFLECTANCE:
            assert out[label]["rc"] == UNSUPPORTED and "bsdf %d (type %d)" % (b, RECORDS[b][0]) in out[label]["msg"] and "kind %d" % kind in out[label]["msg"]
    # the anisotropic roughconductor has no isotropic alpha
    assert out["hot_9_4_0_0"]["rc"] == UNSUPPORTED


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path):
    exe = _build(tmp_path, flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    out, one_hot = _run(exe, tmp_path)
    assert _check_one_hot(out, one_hot) > 0 and out["floors"]["rc"] == 0 and out["no_room"]["rc"] == INVALID


def test_null_arguments_are_refused_without_a_device():
    from mitsuba2_amd import _lib as L
    lib = L.lib()
    d, t = L.RenderDesc(), L.TangentDesc()
    out = (C.c_float * 4)()
    fake = C.c_void_p(C.addressof(out))        # never dereferenced: the null checks come first
    for args in ((None, C.byref(d), C.byref(t), fake), (fake, None, C.byref(t), fake), (fake, C.byref(d), None, fake), (fake, C.byref(d), C.byref(t), None)):
        assert lib.mtsamd_render_forward(*args, None) == INVALID and lib.mtsamd_last_error() == b"null argument"
        assert lib.mtsamd_sample_forward(args[0], args[1], args[2], 0, 1, args[3], None, None) == INVALID and lib.mtsamd_last_error() == b"null argument"
    assert L.BSDF_TANGENT_FLOATS == 18 and L.FORWARD_DETACH_ROULETTE == 1 and lib.mtsamd_abi_version() == 6

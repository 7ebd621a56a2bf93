"""The host half of the forward and reverse renders in scenes with textured BSDF parameters, without a GPU: build_tangent_records and
build_reverse_slots (mitsuba2_amd/csrc/scene_build.cpp) through tests/fused_param_maps_driver.cpp, a stand-alone program compiled with the
host-only scene builder the way forward_tangent_driver.cpp is.

* the pairs / slots of the untextured fields of a record with a map are, bit for bit, those of the same record without the map, one scalar
  at a time at the default step and at an explicit one;
* the eps rule of a tangent over several scalars ignores the fields a texture overwrites: placeholders that would shrink the step (an
  alpha at its floor, a huge colour) change nothing;
* a tangent and a wanted flag on each of the five bindable parameters (alpha, alpha_u, alpha_v, specular_reflectance,
  specular_transmittance) is refused by name -- ALPHA if either roughness is bound;
* the driver built with -fsanitize=address,undefined runs the same cases clean (a stand-alone program: nothing is preloaded)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mitsuba2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
UNSUPPORTED = -5
REFLECTANCE, SPECULAR_REFLECTANCE, ETA, K, ALPHA, SPECULAR_TRANSMITTANCE = range(6)
TEX_PARAMS, ALPHA_U_LUM, ALPHA_V_LUM = 512, 1024, 2048      # device_bsdf.h: kBsdfTexParams, kBsdfAlphaULum, kBsdfAlphaVLum
STEPS = (0.0, 0.003)


def bound(alpha_u=0, alpha_v=0, spec=0, trans=0):
    """(flags, nested0, nested1) of a record whose slots read texture `index` ("1 + texture index" per 16-bit field, 0 = the constant)"""
    return (TEX_PARAMS | (ALPHA_U_LUM if alpha_u else 0) | (ALPHA_V_LUM if alpha_v else 0), alpha_u | alpha_v << 16, spec | trans << 16)


# name: (type, the 14 floats from r on, the binding, the kinds the binding takes away, the name the refusal uses).  The placeholders of
# the textured fields are chosen to disturb a step rule that looked at them: an alpha at its floor, colours of 100
FLOATS_RC = (0, 0, 0, .9, .8, .7, .2, .92, 1.1, 3.9, 2.45, 2.14, .15, .15)
FLOATS_RD = (0, 0, 0, 1., .9, .8, 1.5, 0, 0, .95, .9, 1., .3, .3)
MAPPED = {
    "alpha": (2, FLOATS_RC[:12] + (.0001, .0001), bound(alpha_u=1, alpha_v=1), (ALPHA,), "alpha"),
    "alpha_u": (2, FLOATS_RC[:12] + (.0001, .15), bound(alpha_u=2), (ALPHA,), "alpha_u"),
    "alpha_v": (6, FLOATS_RD[:12] + (.3, .0001), bound(alpha_v=1), (ALPHA,), "alpha_v"),
    "specular_reflectance": (2, FLOATS_RC[:3] + (100., 100., 100.) + FLOATS_RC[6:], bound(spec=3), (SPECULAR_REFLECTANCE,), "specular_reflectance"),
    "specular_transmittance": (6, FLOATS_RD[:9] + (100., 100., 100.) + FLOATS_RD[12:], bound(trans=1), (SPECULAR_TRANSMITTANCE,), "specular_transmittance"),
    "both_colours": (3, FLOATS_RD[:3] + (100.,) * 3 + FLOATS_RD[6:9] + (100.,) * 3 + (0, 0), bound(spec=1, trans=1),
                     (SPECULAR_REFLECTANCE, SPECULAR_TRANSMITTANCE), None),
}
PLAIN_FLOATS = {"alpha": FLOATS_RC, "alpha_u": FLOATS_RC, "alpha_v": FLOATS_RD, "specular_reflectance": FLOATS_RC, "specular_transmittance": FLOATS_RD,
                "both_colours": FLOATS_RD[:12] + (0, 0)}
KINDS = {2: (SPECULAR_REFLECTANCE, ETA, K, ALPHA), 6: (SPECULAR_REFLECTANCE, SPECULAR_TRANSMITTANCE, ALPHA), 3: (SPECULAR_REFLECTANCE, SPECULAR_TRANSMITTANCE)}
FIELD = {SPECULAR_REFLECTANCE: 3, ETA: 6, K: 9, SPECULAR_TRANSMITTANCE: 9}


def _record(type_, floats, binding=(0, 0, 0)):
    return "record %d -1 %d %d %d %s" % ((type_,) + tuple(binding) + (" ".join(repr(float(x)) for x in floats),))


def _vector(op, b, entries):
    t = ["0"] * 18
    for (kind, comp), v in entries.items():
        t[3 * kind + comp] = str(v)
    return "%s %d %s" % (op, b, " ".join(t))


def _case_lines():
    """Record 0 is always the mapped record, record 1 the same record without the map (its textured fields hold ordinary constants)."""
    lines, hot, refused = [], [], []
    for name, (type_, floats, binding, taken, _) in MAPPED.items():
        lines += ["clear", _record(type_, floats, binding), _record(type_, PLAIN_FLOATS[name])]
        for kind in KINDS[type_]:
            for comp in range(1 if kind == ALPHA else 3):
                for b in (0, 1):
                    for si, h in enumerate(STEPS):
                        label = "%s_%d_%d_%d_%d" % (name, kind, comp, b, si)
                        for op, run, value in (("tangent", "forward", 1.0), ("wanted", "reverse", 1)):
                            lines += [_vector(op, b, {(kind, comp): value}), "%s %s_%s %r" % (run, label, run, h), _vector(op, b, {})]
                        (refused if b == 0 and kind in taken else hot).append((name, kind, comp, b, si))
        # a tangent over every untextured colour scalar at once, on either record
        several = {(kind, comp): 0.5 + 0.25 * comp + kind for kind in KINDS[type_] if kind not in taken and kind != ALPHA for comp in range(3)}
        for b in (0, 1):
            for si, h in enumerate(STEPS):
                lines += [_vector("tangent", b, several), "forward %s_several_%d_%d %r" % (name, b, si, h), _vector("tangent", b, {})]
    return lines, hot, refused


def _build(directory, flags=()):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = os.path.join(str(directory), "fused_param_maps_driver")
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, "-o", exe] + list(flags) +
                          ["-x", "hip", "--cuda-host-only", os.path.join(HERE, "fused_param_maps_driver.cpp"), os.path.join(CSRC, "scene_build.cpp"), "-x", "c++"] +
                          [os.path.join(CSRC, f) for f in ("bvh.cpp", "envmap.cpp", "spectral_upsampling.cpp")], stderr=subprocess.DEVNULL)
    return exe


def _run(exe, directory):
    lines, hot, refused = _case_lines()
    path = os.path.join(str(directory), "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = {}
    for line in subprocess.check_output([exe, path], text=True).splitlines():
        label, what, rest = (line.split(" ", 2) + [""])[:3]
        entry = out.setdefault(label, {"plus": {}, "minus": {}, "slot": []})
        if what == "rc":
            entry["rc"] = int(rest)
        elif what == "msg":
            entry["msg"] = rest
        elif what in ("inv_2h", "range"):
            entry[what] = rest.split()
        elif what == "slot":
            entry["slot"].append(rest.split())
        else:
            b, words = rest.split(" ", 1)
            entry[what][int(b)] = words.split()
    return out, hot, refused


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("fused_param_maps")
    return _run(_build(d), d)


def _moved(words, name, b):
    """hex words of a dumped record -> the words of the fields the tangent may move: everything but the textured fields of record 0"""
    type_, _, binding, taken, _ = MAPPED[name]
    skip = set()
    if b == 0:
        if binding[1] & 0xFFFF:
            skip.add(12)
        if binding[1] >> 16:
            skip.add(13)
        if binding[2] & 0xFFFF:
            skip |= {3, 4, 5}
        if binding[2] >> 16:
            skip |= {9, 10, 11}
    return [w for i, w in enumerate(words) if i not in skip], skip


def _check_untextured_fields(out, hot):
    n = 0
    for (name, kind, comp, b, si) in hot:
        if b != 0:
            continue
        label = "%s_%d_%d_%%d_%d" % (name, kind, comp, si)
        mine, plain = out[(label % 0) + "_forward"], out[(label % 1) + "_forward"]
        if plain["rc"] != 0:          # the model has no such parameter (an anisotropic alpha): refused on both sides, in the usual words
            assert mine["rc"] == plain["rc"] and "has no differentiable parameter" in mine["msg"], (label, mine, plain)
            continue
        assert mine["rc"] == 0, (label, mine)
        # the pair of the mapped record: the moved scalar and every untextured field as in the plain record, bit for bit; its textured
        # fields keep their placeholders (the device overwrites them with the lookup); 1 / (2 eps) as in the plain record
        for side in ("plus", "minus"):
            got, skip = _moved(mine[side][0], name, 0)
            want = [w for i, w in enumerate(plain[side][1]) if i not in skip]
            assert got == want, (label, side, got, want)
        assert mine["inv_2h"][0] == plain["inv_2h"][1] and int(mine["inv_2h"][0], 16) != 0 and int(mine["inv_2h"][1], 16) == 0, (label, mine["inv_2h"], plain["inv_2h"])
        # the slot of the reverse render: the same patch
        rm, rp = out[(label % 0) + "_reverse"], out[(label % 1) + "_reverse"]
        assert rm["rc"] == 0 and rp["rc"] == 0 and len(rm["slot"]) == 1 and len(rp["slot"]) == 1, (label, rm, rp)
        sm, sp = rm["slot"][0], rp["slot"][0]
        assert sm[1] == "0" and sp[1] == "1" and int(sp[2]) - int(sm[2]) == 18 and sm[3:] == sp[3:], (label, sm, sp)
        assert rm["range"] == ["0", "1", "1"] and rp["range"] == ["0", "0", "1"]
        n += 1
    return n


def test_untextured_fields_beside_a_map_are_those_of_the_plain_record(results):
    out, hot, _ = results
    # per mapped record the accepted scalars outside its binding, two steps each: roughconductor 9 (+ alpha 1), roughdielectric 6 (+ 1),
    # dielectric 6; minus what the binding takes away
    assert _check_untextured_fields(out, hot) == 2 * (9 + 9 + 6 + 7 + 4 + 0)


def test_the_eps_rule_ignores_textured_fields(results):
    out, _, _ = results
    n = 0
    for name, (type_, floats, binding, taken, _) in MAPPED.items():
        if name == "both_colours":
            continue          # nothing untextured is left to carry a tangent
        for si in range(len(STEPS)):
            mine, plain = out["%s_several_0_%d" % (name, si)], out["%s_several_1_%d" % (name, si)]
            assert mine["rc"] == 0 and plain["rc"] == 0, (name, mine, plain)
            for side in ("plus", "minus"):
                got, skip = _moved(mine[side][0], name, 0)
                assert got == [w for i, w in enumerate(plain[side][1]) if i not in skip], (name, side)
                # the textured fields are not moved: they hold their placeholders
                assert [w for i, w in enumerate(mine[side][0]) if i in skip] == \
                       ["%08x" % int(np.float32(floats[i]).view(np.uint32)) for i in sorted(skip)], (name, side)
            assert mine["inv_2h"][0] == plain["inv_2h"][1] and int(mine["inv_2h"][0], 16) != 0
            n += 1
    assert n == 10


def _check_refusals(out, refused):
    names = set()
    for (name, kind, comp, b, si) in refused:
        label = "%s_%d_%d_%d_%d" % (name, kind, comp, b, si)
        want = MAPPED[name][4] or {SPECULAR_REFLECTANCE: "specular_reflectance", SPECULAR_TRANSMITTANCE: "specular_transmittance"}[kind]
        for run in ("forward", "reverse"):
            got = out["%s_%s" % (label, run)]
            assert got["rc"] == UNSUPPORTED and got["msg"].startswith("bsdf 0: %s holds a texture" % want), (label, run, got)
        names.add(want)
    return names


def test_a_tangent_or_wanted_flag_on_a_textured_parameter_is_refused_by_name(results):
    out, _, refused = results
    assert _check_refusals(out, refused) == {"alpha", "alpha_u", "alpha_v", "specular_reflectance", "specular_transmittance"}
    assert len(refused) == 2 * (1 + 1 + 1 + 3 + 3 + 6)


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path):
    exe = _build(tmp_path, flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    out, hot, refused = _run(exe, tmp_path)
    assert _check_untextured_fields(out, hot) > 0 and len(_check_refusals(out, refused)) == 5

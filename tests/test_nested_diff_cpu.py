"""The host half of the forward and reverse renders in scenes with blendbsdf / mask records (MTSAMD_FORWARD_NESTED /
MTSAMD_REVERSE_NESTED), without a GPU: check_derivative_flags, split_nested_rows and add_weight_slots (mitsuba2_amd/csrc/scene_build.cpp)
through tests/nested_tangent_driver.cpp, a stand-alone program compiled with the host-only scene builder the way
forward_tangent_driver.cpp is.

* the rows of nested records are taken out -- entry 18 * b + 0 becomes the weight's tangent / wanted flag -- and the rows of every
  other record reach build_tangent_records / build_reverse_slots bit for bit: the tables equal those of the same tangent with the
  nested rows zeroed, handed to the old builders directly;
* a wanted weight is one slot without a pair (f0 = f1 = 0xffff, out = 18 * b) inside its record's range, in record order;
* every refusal returns its message: components 1 and 2 and every other kind on a nested record, a tangent / wanted flag on a textured
  weight, a tangent that is not finite;
* the flag rule per scene class: bit 4 is known only in an RGB scene with a nested record; without it every answer is the old one;
* the driver built with -fsanitize=address,undefined runs the same cases clean (a stand-alone program: nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mitsuba2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
INVALID, UNSUPPORTED = -1, -5
DIFFUSE, ROUGHCONDUCTOR, BLEND, MASK = 0, 2, 8, 9
TEX_PARAMS = 512      # device_bsdf.h: kBsdfTexParams

DIFF = (.5, .4, .3) + (1.,) * 3 + (0.,) * 3 + (1.,) * 3 + (.1, .1)
ROUGH = (0, 0, 0, .9, .8, .7, .2, .92, 1.1, 3.9, 2.45, 2.14, .15, .15)


def _record(type_, floats, texture=-1, flags=0, nested=(0, 0)):
    return "record %d %d %d %d %d %s" % (type_, texture, flags, nested[0], nested[1], " ".join(repr(float(x)) for x in floats))


def _nest(type_, w, children, texture=-1):
    return _record(type_, (w, w, w) + DIFF[3:], texture=texture, nested=children)


def _vector(op, b, entries):
    t = ["0"] * 18
    for i, v in entries.items():
        t[i] = str(v)
    return "%s %d %s" % (op, b, " ".join(t))


# record 0: blend(0.3; 2, 3), 1: mask(0.6; 4), 2: roughconductor, 3: diffuse, 4: diffuse, 5: blend with a textured weight, 6: a plain wall
TABLE = [_nest(BLEND, .3, (2, 3)), _nest(MASK, .6, (4, 4)), _record(ROUGHCONDUCTOR, ROUGH), _record(DIFFUSE, DIFF), _record(DIFFUSE, DIFF),
         _nest(BLEND, .5, (3, 4), texture=0), _record(DIFFUSE, DIFF)]
CHILD_ROWS = {2: {3: .5, 6: 1., 9: -2., 12: .25}, 3: {0: 1., 1: -.5, 2: 2.}, 4: {1: 1.}, 6: {0: .75}}
N = len(TABLE)


def _cases():
    lines = ["clear"] + TABLE
    # the split: weights 0.7 / -1.5 beside tangents on the children and the wall
    for b, row in CHILD_ROWS.items():
        lines.append(_vector("tangent", b, row))
    lines += ["plain without_weights 0.0", "plain without_weights_h 0.003"]
    lines += [_vector("tangent", 0, {0: .7}), _vector("tangent", 1, {0: -1.5}), "forward split 0.0", "forward split_h 0.003"]
    for b, row in CHILD_ROWS.items():
        lines.append(_vector("wanted", b, {i: 1 for i in row}))
    lines += [_vector("wanted", 0, {0: 1}), _vector("wanted", 1, {0: 1}), "reverse slots 0.0"]
    lines += [_vector("wanted", 0, {}), _vector("wanted", 1, {}), "reverse slots_plain 0.0"]
    for b in range(N):
        lines += [_vector("tangent", b, {}), _vector("wanted", b, {})]
    # refusals, one entry at a time on the blend (0), the mask (1) and the textured blend (5)
    for b in (0, 1):
        for i in range(1, 18):
            lines += [_vector("tangent", b, {i: 1.0}), "forward refuse_t_%d_%d 0.0" % (b, i), _vector("tangent", b, {}),
                      _vector("wanted", b, {i: 1}), "reverse refuse_w_%d_%d 0.0" % (b, i), _vector("wanted", b, {})]
    lines += [_vector("tangent", 5, {0: 1.0}), "forward refuse_t_tex 0.0", _vector("tangent", 5, {}),
              _vector("wanted", 5, {0: 1}), "reverse refuse_w_tex 0.0", _vector("wanted", 5, {}),
              _vector("tangent", 0, {0: "inf"}), "forward refuse_inf 0.0", _vector("tangent", 0, {}),
              _vector("tangent", 3, {3: 1.0}), "forward refuse_child 0.0", _vector("tangent", 3, {})]
    # the old builders still refuse a tangent on a nested record and keep no slot for it
    lines += [_vector("tangent", 0, {0: 1.0}), "plain old_refuses 0.0", _vector("tangent", 0, {})]
    # the flag rule per scene class
    for name, table, spectral in (("nested", TABLE, 0), ("plain", [_record(DIFFUSE, DIFF), _record(ROUGHCONDUCTOR, ROUGH)], 0),
                                  ("maps", [_record(ROUGHCONDUCTOR, ROUGH, flags=TEX_PARAMS, nested=(1, 0))], 0),
                                  ("both", [_nest(MASK, .6, (1, 1)), _record(ROUGHCONDUCTOR, ROUGH, flags=TEX_PARAMS, nested=(1, 0))], 0),
                                  ("spectral", [_nest(MASK, .6, (1, 1)), _record(DIFFUSE, DIFF)], 1)):
        lines += ["clear"] + table + ["spectral %d" % spectral]
        for bits in range(9):
            for reverse in (0, 1):
                lines.append("flags %s_%d_%d %d %d" % (name, bits, reverse, bits, reverse))
    return lines


def _build(directory, flags=()):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = os.path.join(str(directory), "nested_tangent_driver")
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, "-o", exe] + list(flags) +
                          ["-x", "hip", "--cuda-host-only", os.path.join(HERE, "nested_tangent_driver.cpp"), os.path.join(CSRC, "scene_build.cpp"), "-x", "c++"] +
                          [os.path.join(CSRC, f) for f in ("bvh.cpp", "envmap.cpp", "spectral_upsampling.cpp")], stderr=subprocess.DEVNULL)
    return exe


def _run(exe, directory):
    path = os.path.join(str(directory), "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(_cases()) + "\n")
    out = {}
    for line in subprocess.check_output([exe, path], text=True).splitlines():
        label, what, rest = (line.split(" ", 2) + [""])[:3]
        entry = out.setdefault(label, {"plus": {}, "minus": {}, "rest": {}, "slot": []})
        if what == "rc":
            entry["rc"] = int(rest)
        elif what == "nested":
            entry["nested"] = int(rest)
        elif what == "msg":
            entry["msg"] = rest
        elif what in ("inv_2h", "range", "weight"):
            entry[what] = rest.split()
        elif what == "slot":
            entry["slot"].append(rest.split())
        else:
            b, words = rest.split(" ", 1)
            entry[what][int(b)] = words.split()
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("nested_diff")
    return _run(_build(d), d)


def _hex(x):
    import numpy as np
    return "%08x" % int(np.float32(x).view(np.uint32))


def _check_split(out):
    for suffix in ("", "_h"):
        mine, old = out["split" + suffix], out["without_weights" + suffix]
        assert mine["rc"] == 0 and old["rc"] == 0, (mine, old)
        # the nested rows are zero in what is handed on, every other row is the caller's, bit for bit
        assert mine["rest"] == old["rest"]
        assert all(int(w, 16) == 0 for b in (0, 1, 5) for w in mine["rest"][b])
        assert mine["weight"] == [_hex(.7), _hex(-1.5)] + [_hex(0.)] * (N - 2)
        # ... and so are the tables the old builder makes of them
        assert mine["plus"] == old["plus"] and mine["minus"] == old["minus"] and mine["inv_2h"] == old["inv_2h"]
        assert [int(w, 16) != 0 for w in mine["inv_2h"]] == [False, False, True, True, True, False, True]
    return True


def test_nested_rows_are_taken_out_and_the_rest_reaches_the_old_builder_bit_for_bit(results):
    assert _check_split(results)


def test_a_wanted_weight_is_a_slot_without_a_pair_in_record_order(results):
    mine, old = results["slots"], results["slots_plain"]
    assert mine["rc"] == 0 and old["rc"] == 0
    assert mine["weight"] == ["1", "1", "0", "0", "0", "0", "0"] and old["weight"] == ["0"] * N
    n_child = {b: len(r) for b, r in CHILD_ROWS.items()}
    assert old["range"] == ["0", "0", "0", "4", "7", "8", "8", "9"] and len(old["slot"]) == sum(n_child.values())
    assert mine["range"] == ["0", "1", "2", "6", "9", "10", "10", "11"]
    # the two weight slots come first (records 0 and 1); the others are the old slots, moved by two
    assert [s[1:5] for s in mine["slot"][:2]] == [["0", "0", "65535", "65535"], ["1", "18", "65535", "65535"]]
    assert [s[1:] for s in mine["slot"][2:]] == [s[1:] for s in old["slot"]]
    assert [int(s[0]) for s in mine["slot"]] == list(range(11))


def _check_refusals(out):
    n = 0
    for b, kind_name, model in ((0, "weight", "blendbsdf"), (1, "opacity", "mask")):
        for i in range(1, 18):
            for run, tail in (("t", "of its tangent is not zero"), ("w", "is wanted")):
                got = out["refuse_%s_%d_%d" % (run, b, i)]
                assert got["rc"] == UNSUPPORTED, got
                assert got["msg"] == "bsdf %d: a %s record has one differentiable scalar, its %s (parameter kind 0, component 0); kind %d, component %d %s" % (
                    b, model, kind_name, i // 3, i % 3, tail), got
                n += 1
    assert out["refuse_t_tex"]["rc"] == UNSUPPORTED and out["refuse_t_tex"]["msg"].startswith("bsdf 5: weight holds a texture; its texels carry the tangent")
    assert out["refuse_w_tex"]["rc"] == UNSUPPORTED and out["refuse_w_tex"]["msg"].startswith("bsdf 5: weight holds a texture; its texels carry the gradient")
    assert out["refuse_inf"]["rc"] == INVALID and "bsdf 0: the tangent of parameter kind 0 is not finite" in out["refuse_inf"]["msg"]
    # a child is an ordinary record: its refusals are the old builder's (a diffuse has no specular_reflectance)
    assert out["refuse_child"]["rc"] == UNSUPPORTED and "bsdf 3 (type 0) has no differentiable parameter of kind 1" in out["refuse_child"]["msg"]
    assert out["old_refuses"]["rc"] == UNSUPPORTED and "bsdf 0 (type 8) has no differentiable parameter of kind 0" in out["old_refuses"]["msg"]
    return n


def test_every_refusal_returns_its_message(results):
    assert _check_refusals(results) == 2 * 17 * 2


def _check_flags(out):
    for reverse, mode, desc in ((0, "forward-mode", "tangent"), (1, "reverse-mode", "gradient")):
        def got(name, bits):
            return out["%s_%d_%d" % (name, bits, reverse)]
        unknown = lambda bits: "unknown flag bits 0x%x in the %s descriptor" % (bits, desc)
        blend = "the %s render does not handle blendbsdf / mask materials" % mode
        maps = "the %s render does not handle textured BSDF parameters (alpha, specular_reflectance, specular_transmittance)" % mode
        for bits in range(9):
            # an RGB scene with a nested record: bit 4 opens it; without it the old refusals (flags 2 there is still the unknown bit)
            g = got("nested", bits)
            if bits & ~5:
                assert (g["rc"], g["msg"]) == (INVALID, unknown(bits))
            elif bits & 4:
                assert (g["rc"], g["nested"]) == (0, 1)
            else:
                assert (g["rc"], g["msg"], g["nested"]) == (UNSUPPORTED, blend, 0)
            # no nested record: bit 4 stays unknown
            g = got("plain", bits)
            assert (g["rc"], g["nested"]) == (0, 0) if not bits & ~1 else (g["rc"], g["msg"]) == (INVALID, unknown(bits))
            g = got("maps", bits)
            if bits & ~3:
                assert (g["rc"], g["msg"]) == (INVALID, unknown(bits))
            elif bits & 2:
                assert (g["rc"], g["nested"]) == (0, 0)
            else:
                assert (g["rc"], g["msg"]) == (UNSUPPORTED, maps)
            # both features: refused with a message that names both once bit 4 is set; without it, the old answers
            g = got("both", bits)
            if bits & ~7:
                assert (g["rc"], g["msg"]) == (INVALID, unknown(bits))
            elif bits & 4:
                assert g["rc"] == UNSUPPORTED and "blendbsdf / mask materials together with textured BSDF parameters" in g["msg"], g
            elif bits & 2:
                assert (g["rc"], g["msg"]) == (UNSUPPORTED, blend)
            else:
                assert (g["rc"], g["msg"]) == (UNSUPPORTED, maps)
            # a spectral scene: bit 4 unknown, the old refusal otherwise
            g = got("spectral", bits)
            if bits & ~1:
                assert (g["rc"], g["msg"]) == (INVALID, unknown(bits))
            else:
                assert (g["rc"], g["msg"]) == (UNSUPPORTED, "the %s render is implemented for the RGB variant only" % mode)
    return True


def test_the_flag_rule_per_scene_class(results):
    assert _check_flags(results)


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path):
    exe = _build(tmp_path, flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    out = _run(exe, tmp_path)
    assert _check_split(out) and _check_refusals(out) == 68 and _check_flags(out)

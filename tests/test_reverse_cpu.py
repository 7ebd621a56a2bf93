"""The host half of the reverse-mode render without a GPU: build_reverse_slots (mitsuba2_amd/csrc/scene_build.cpp) through
tests/reverse_slots_driver.cpp, a stand-alone program compiled with the host-only scene builder the way forward_tangent_driver.cpp is.

* for every (type, kind, component) bsdf_param_fields accepts -- the 62 triples of test_forward_cpu.py -- at the default step and at an
  explicit one, the slot's patched pair and 1 / (2 h) are, bit for bit, what build_tangent_records gives for the one-hot tangent on that
  scalar (computed by the driver in the same run) AND what mtsamd_render_adjoint_param builds (the rule written out in float32 in
  test_forward_cpu.py); every other triple is refused by name;
* ALPHA and ETA stay above 1e-4, and a value that leaves no room is refused;
* the slot ranges of the records are contiguous, in record order, and cover exactly the wanted scalars;
* the driver built with -fsanitize=address,undefined runs the same cases clean (a stand-alone program: nothing is preloaded);
* the entry point of the library refuses null arguments and an empty gradient before it touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_forward_cpu import ALPHA, CSRC, ETA, F32, HERE, HIPCC, INVALID, K, RECORDS, STEPS, UNSUPPORTED, accepted, adjoint_param_rule, bits

FLOAT_OFFSET = (0, 1, 2, 8, 9, 10, 12, 13, 14, 16, 17, 18, 15, 19)      # of r .. alpha_v inside DevBsdf (device_bsdf.h), in floats
FLOOR_TABLE = [(2, -1, 0, 0, 0, 1., 1., 1., .2, .9, 1.1, 3.9, 2.4, 2.2, .0002, .0002), (1, -1, 0, 0, 0, 1., 1., 1., .00015, 1.1, 1.4, 3.9, 2.4, 2.2, 0, 0),
               (6, -1, 0, 0, 0, 1., 1., 1., 1.5, 0, 0, 1., 1., 1., .0001, .0001)]


def _case_lines():
    lines, one_hot = [], {}

    def table(records):
        lines.append("clear")
        for r in records:
            lines.append("record " + " ".join(repr(float(x)) if i >= 2 else str(x) for i, x in enumerate(r)))

    def wanted(b, entries, value="1"):
        w = ["0"] * 18
        for kind, comp in entries:
            w[3 * kind + comp] = value
        lines.append("wanted %d %s" % (b, " ".join(w)))

    table(RECORDS)
    for b, rec in enumerate(RECORDS):
        for kind in range(6):
            for comp in range(3):
                wanted(b, [(kind, comp)])
                for si, h in enumerate(STEPS):
                    label = "hot_%d_%d_%d_%d" % (b, kind, comp, si)
                    lines.append("run %s %r" % (label, h))
                    one_hot[label] = (b, kind, comp, h)
                wanted(b, [])
    lines.append("null untouched 0.01")
    lines.append("run none 0.01")
    # every accepted scalar of every record at once (any non-zero byte means wanted)
    every = []
    for b, rec in enumerate(RECORDS):
        here = [(kind, comp) for kind in range(6) for comp in range(3) if accepted(rec, kind, comp) is not None]
        every += [(b, kind, comp) for kind, comp in here]
        wanted(b, here, "252" if b == 2 else "1")
    for si, h in enumerate(STEPS):
        lines.append("run every_%d %r" % (si, h))
    table(FLOOR_TABLE)
    wanted(0, [(ALPHA, 0), (K, 0)])
    wanted(1, [(ETA, 0)])
    lines.append("run floors 0.01")
    wanted(2, [(ALPHA, 0)])
    lines.append("run no_room 0.01")
    return lines, one_hot, every


def _build(directory, flags=()):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = os.path.join(str(directory), "reverse_slots_driver")
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, "-o", exe] + list(flags) +
                          ["-x", "hip", "--cuda-host-only", os.path.join(HERE, "reverse_slots_driver.cpp"), os.path.join(CSRC, "scene_build.cpp"), "-x", "c++"] +
                          [os.path.join(CSRC, f) for f in ("bvh.cpp", "envmap.cpp", "spectral_upsampling.cpp")], stderr=subprocess.DEVNULL)
    return exe


def _run(exe, directory):
    lines, one_hot, every = _case_lines()
    path = os.path.join(str(directory), "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = {}
    for line in subprocess.check_output([exe, path], text=True).splitlines():
        label, what, rest = (line.split(" ", 2) + [""])[:3]
        entry = out.setdefault(label, {"slots": {}})
        if what == "rc":
            entry["rc"] = int(rest)
        elif what == "msg":
            entry["msg"] = rest
        elif what == "range":
            entry["range"] = [int(x) for x in rest.split()]
        else:
            j, words = (rest.split(" ", 1) + [""])[:2]
            slot = entry["slots"].setdefault(int(j), {})
            if what in ("slot", "ref_rc", "ref_others"):
                slot[what] = [int(x) for x in words.split()]
            else:
                slot[what] = np.array([int(w, 16) for w in words.split()], np.uint32).view(F32)
    return out, one_hot, every


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("reverse_slots")
    return _run(_build(d), d)


def _check_slot(table, slot, b, kind, comp, h, where):
    """one slot against the one-hot tangent records of the same run and against the rule of the parameter adjoint"""
    rec = table[b]
    fields = accepted(rec, kind, comp)
    assert slot["slot"][:2] == [b, 18 * b + 3 * kind + comp], (where, slot["slot"])
    assert slot["slot"][2] == FLOAT_OFFSET[fields[0]] and slot["slot"][3] == FLOAT_OFFSET[fields[-1]], (where, slot["slot"])
    assert slot["ref_rc"] == [0] and slot["ref_others"] == [1], where
    for mine, ref in (("plus", "ref_plus"), ("minus", "ref_minus"), ("inv", "ref_inv")):
        assert np.array_equal(bits(slot[mine]), bits(slot[ref])), (where, mine, slot[mine], slot[ref])
    plus, minus, inv = adjoint_param_rule(rec[2 + fields[0]], kind, h)
    want_p, want_m = np.array(rec[2:], F32), np.array(rec[2:], F32)
    want_p[list(fields)], want_m[list(fields)] = plus, minus
    assert np.array_equal(bits(slot["plus"]), bits(want_p)) and np.array_equal(bits(slot["minus"]), bits(want_m)), where
    assert bits(slot["inv"])[0] == bits(inv), (where, slot["inv"], inv)


def _check_one_hot(out, one_hot):
    n_accepted = 0
    for label, (b, kind, comp, h) in one_hot.items():
        rec, got = RECORDS[b], out[label]
        if accepted(rec, kind, comp) is None:
            assert got["rc"] == UNSUPPORTED, (label, got)
            assert got["msg"] == "bsdf %d (type %d) has no differentiable parameter of kind %d (component %d is wanted)" % (b, rec[0], kind, comp), got["msg"]
            continue
        n_accepted += 1
        assert got["rc"] == 0 and len(got["slots"]) == 1, (label, got)
        assert got["range"] == [0] * (b + 1) + [1] * (len(RECORDS) - b), (label, got["range"])
        _check_slot(RECORDS, got["slots"][0], b, kind, comp, h, label)
    return n_accepted


def test_every_slot_is_the_one_hot_tangent_record_bit_for_bit(results):
    out, one_hot, _ = results
    assert _check_one_hot(out, one_hot) == 2 * 62
    for label in ("untouched", "none"):
        assert out[label]["rc"] == 0 and not out[label]["slots"] and out[label]["range"] == [0] * (len(RECORDS) + 1), out[label]


def test_record_ranges_are_contiguous_and_cover_the_wanted_scalars(results):
    out, _, every = results
    assert len(every) == 62
    for si, h in enumerate(STEPS):
        got = out["every_%d" % si]
        assert got["rc"] == 0 and len(got["slots"]) == 62 and len(got["range"]) == len(RECORDS) + 1
        assert got["range"][0] == 0 and got["range"][-1] == 62 and got["range"] == sorted(got["range"])
        # slot j belongs to the record whose range holds j, and the slots are the wanted scalars in (record, kind, component) order
        for j, (b, kind, comp) in enumerate(every):
            assert got["range"][b] <= j < got["range"][b + 1], (j, b, got["range"])
            _check_slot(RECORDS, got["slots"][j], b, kind, comp, h, ("every", si, j))
        for b in (8, 10):      # the textured diffuse keeps no slot, the blendbsdf neither
            assert got["range"][b] == got["range"][b + 1]


def test_alpha_and_eta_stay_above_their_floor(results):
    out, _, _ = results
    got = out["floors"]
    assert got["rc"] == 0 and got["range"] == [0, 2, 3, 3], got
    # slots in kind order: k.r (3) of record 0, then its alpha (4); eta.r of record 1
    _check_slot(FLOOR_TABLE, got["slots"][0], 0, K, 0, 0.01, "floors k")
    _check_slot(FLOOR_TABLE, got["slots"][1], 0, ALPHA, 0, 0.01, "floors alpha")
    _check_slot(FLOOR_TABLE, got["slots"][2], 1, ETA, 0, 0.01, "floors eta")
    alpha_minus, eta_minus = got["slots"][1]["minus"], got["slots"][2]["minus"]
    assert F32(1e-4) < alpha_minus[12] == alpha_minus[13] < F32(2e-4) and F32(1e-4) < eta_minus[6] < F32(1.5e-4)
    bad = out["no_room"]
    assert bad["rc"] == INVALID and bad["msg"] == "bsdf 2: parameter value 0.0001 leaves no room for a central difference", bad


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path):
    exe = _build(tmp_path, flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    out, one_hot, _ = _run(exe, tmp_path)
    assert _check_one_hot(out, one_hot) == 2 * 62 and out["floors"]["rc"] == 0 and out["no_room"]["rc"] == INVALID and len(out["every_0"]["slots"]) == 62


def test_null_arguments_are_refused_without_a_device():
    from mitsuba2_amd import _lib as L
    lib = L.lib()
    d, g = L.RenderDesc(), L.GradientDesc()
    out = (C.c_float * 4)()
    fake = C.c_void_p(C.addressof(out))        # never dereferenced: the checks below come before any use
    g.grad_emitters_dev = fake
    for args in ((None, C.byref(d), fake, fake, C.byref(g)), (fake, None, fake, fake, C.byref(g)), (fake, C.byref(d), None, fake, C.byref(g)),
                 (fake, C.byref(d), fake, None, C.byref(g)), (fake, C.byref(d), fake, fake, None)):
        assert lib.mtsamd_render_reverse(*args, None) == INVALID and lib.mtsamd_last_error() == b"null argument"
    empty = L.GradientDesc()
    assert lib.mtsamd_render_reverse(fake, C.byref(d), fake, fake, C.byref(empty), None) == INVALID
    assert lib.mtsamd_last_error().startswith(b"the gradient is empty")
    half = L.GradientDesc()
    half.grad_bsdf_dev = fake
    assert lib.mtsamd_render_reverse(fake, C.byref(d), fake, fake, C.byref(half), None) == INVALID
    assert lib.mtsamd_last_error() == b"bsdf_wanted and grad_bsdf_dev go together: one of them is null"
    assert L.REVERSE_DETACH_ROULETTE == 1 and C.sizeof(L.GradientDesc) == 48 and lib.mtsamd_abi_version() == 6

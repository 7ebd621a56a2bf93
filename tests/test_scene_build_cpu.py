"""The host-only scene builder (mitsuba2_amd/csrc/scene_build.cpp) without a GPU.  tests/scene_build_driver.cpp is compiled with the
builder, bvh.cpp, envmap.cpp and spectral_upsampling.cpp into a plain host program that builds the scenes written here and dumps what the
host holds; every expectation is in this file:

* layout: primitive order, pair and cluster records, gradient offsets, area distributions, the empty scene's roots;
* setter round trip: creating with a value `v` gives the same bytes as creating with `u` and setting `v` -- the invariant that the
  conversions shared by creation and the setters exist to keep (KNOWN_STALE lists what the library has never kept in step);
* every error of creation that needs no device: its code and exact message, from the builder and from the built library's C ABI."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from mitsuba2_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mitsuba2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
MODEL = os.path.join(HERE, "golden", "rgb2spec_opt_res16.coeff")
F32 = np.float32

DIFFUSE, CONDUCTOR, ROUGHCONDUCTOR, DIELECTRIC, PLASTIC, ROUGHPLASTIC, ROUGHDIELECTRIC, THINDIELECTRIC, BLEND, MASK = range(10)
AREA, CONSTANT, ENVMAP, POINT, SPOT, DIRECTIONAL = range(6)
P_REFLECTANCE, P_SPECULAR, P_ETA, P_K, P_ALPHA, P_TRANSMITTANCE = range(6)
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]


# ---- scene descriptions: lists of (record, fields) -------------------------------------------------------------------------------------
def mesh(tris=1, bsdf=0, emitter=-1, **kw):
    return ("mesh", dict(tris=tris, bsdf=bsdf, emitter=emitter, **kw))


def bsdf(type=DIFFUSE, **kw):
    d = dict(type=type, reflectance=[0.5, 0.5, 0.5], texture=-1, specular_reflectance=[1, 1, 1], specular_transmittance=[1, 1, 1], eta=[0, 0, 0], k=[1, 1, 1],
             int_ior=1.5046, ext_ior=1.000277, alpha_u=0.1, alpha_v=0.1, sample_visible=1, nested=[-1, -1])
    d.update(kw)
    return ("bsdf", d)


def emitter(type=AREA, **kw):
    d = dict(type=type, radiance=[1, 1, 1], to_world=IDENTITY, cutoff_angle=20, beam_width=15, envmap_scale=1)
    d.update(kw)
    return ("emitter", d)


def bitmap(data):
    data = np.asarray(data, F32)
    return ("texture", dict(kind=0, width=data.shape[1], height=data.shape[0], data=data.ravel()))


def checkerboard(color0=(0.4, 0.4, 0.4), color1=(0.2, 0.2, 0.2)):
    return ("texture", dict(kind=1, color0=color0, color1=color1))


def envmap(data, **kw):
    data = np.asarray(data, F32)
    return emitter(ENVMAP, envmap_width=data.shape[1], envmap_height=data.shape[0], data=data.ravel(), **kw)


SPECTRAL = ("spectral", {})


def texels(seed, h=2, w=3):
    return (0.1 + 0.8 * np.random.RandomState(seed).rand(h, w, 3)).astype(F32)


def _text(v):
    return ",".join(repr(float(F32(x))) for x in np.atleast_1d(np.asarray(v, np.float64)))


def to_text(name, records):
    lines = ["scene " + name]
    lines += [" ".join([rec] + ["%s=%s" % (k, _text(v)) for k, v in fields.items()]) for rec, fields in records]
    return "\n".join(lines + ["end"]) + "\n"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    tmp = tmp_path_factory.mktemp("scene_build")
    exe = str(tmp / "driver")
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, "-o", exe, "-x", "hip", "--cuda-host-only",
                           os.path.join(HERE, "scene_build_driver.cpp"), os.path.join(CSRC, "scene_build.cpp"), "-x", "c++"] +
                          [os.path.join(CSRC, f) for f in ("bvh.cpp", "envmap.cpp", "spectral_upsampling.cpp")], stderr=subprocess.DEVNULL)

    def run(scenes):
        """{name: records} -> {name: {key: uint32 words | rc | message}}"""
        path = str(tmp / "scenes.txt")
        with open(path, "w") as f:
            f.write("".join(to_text(n, r) for n, r in scenes.items()))
        out, cur = {}, None
        for line in subprocess.check_output([exe, path, MODEL], text=True).splitlines():
            key, _, rest = line.partition(" ")
            if key == "scene":
                cur = out.setdefault(rest, {})
            elif key == "rc":
                cur["rc"] = int(rest)
            elif key == "message":
                cur["message"] = rest
            else:
                cur[key] = np.array([int(w, 16) for w in rest.split()], np.uint32)
        assert set(out) == set(scenes)
        return out
    return run


def f32(words):
    return np.asarray(words, np.uint32).view(F32)


# ---- layout ------------------------------------------------------------------------------------------------------------------------------
FLAGS = ("general", "nested", "non_diffuse", "delta", "spectral", "environment", "flat", "n_pairs", "n_clusters", "n_spectra", "n_prims", "n_shapes", "has_envmap")


def flags(scene):
    return dict(zip(FLAGS, (int(x) for x in scene["flags"])))


def cluster_rule(prim_shape):
    """a new cluster starts at every pair whose first primitive belongs to another shape than the pair before"""
    n_pairs = (len(prim_shape) + 1) // 2
    return sum(1 for k in range(n_pairs) if k == 0 or prim_shape[2 * k] != prim_shape[2 * (k - 1)])


def test_layout(driver):
    tex = texels(0)
    out = driver({
        "two_shapes": [mesh(2, 0), mesh(1, 1), bsdf(), bsdf()],
        "one_triangle": [mesh(1, 0), bsdf()],
        "three_shapes": [mesh(3, 0), mesh(4, 0), mesh(1, 0), bsdf()],
        "textures": [mesh(1, 0), bsdf(), bitmap(tex), checkerboard(), bitmap(texels(1, 4, 2))],
        "area": [mesh(4, 0, 0, degenerate=[0, 3]), bsdf(), emitter(AREA)],
        "empty": [],
    })
    assert all(s["rc"] == 0 for s in out.values()), {n: s["message"] for n, s in out.items()}
    s = out["two_shapes"]
    assert list(s["prim_shape"]) == [0, 0, 1]
    assert list(s["shapes"].reshape(-1, 4)[:, 3]) == [0, 2]                       # first_prim
    fl = flags(s)
    assert (fl["n_prims"], fl["n_pairs"], fl["flat"]) == (3, 2, 1) and fl["n_clusters"] == cluster_rule(s["prim_shape"]) == 2
    pairs = f32(s["pair_recs"]).reshape(-1, 4)
    assert len(pairs) == 5 * 2 + 2 * 2
    # pair 1 = (primitive 2, nothing): slot A is p0 / e1 / e2 of the triangle (2 tris of mesh 0, then triangle 0 of mesh 1 at z = 1)
    assert np.array_equal(pairs[5:10, [0, 2]].ravel()[:9], F32([0, 0, 1, 1, 0, 0, 0, 1, 0]))
    assert not pairs[5:10, [1, 3]].any() and not s["pair_recs"].reshape(-1, 4)[5:10, [1, 3]].any()      # slot B: zero words
    assert list(s["pair_recs"].reshape(-1, 4)[10::2, 3]) == [1, 1]                # pairs per cluster
    s = out["one_triangle"]
    fl = flags(s)
    assert list(s["prim_shape"]) == [0] and (fl["n_pairs"], fl["n_clusters"]) == (1, 1)
    assert not s["pair_recs"].reshape(-1, 4)[:5, [1, 3]].any()
    s = out["three_shapes"]                    # 8 primitives: the pair (2, 3) straddles two shapes and stays with the first, shape 2 starts no pair
    assert list(s["prim_shape"]) == [0, 0, 0, 1, 1, 1, 1, 2]
    assert flags(s)["n_clusters"] == cluster_rule(s["prim_shape"]) == 2
    assert list(s["pair_recs"].reshape(-1, 4)[20::2, 3]) == [2, 2]
    t = out["textures"]["textures"].reshape(3, -1)
    assert list(t[:, 4]) == [0, 18, 18] and list(t[:, 5]) == [0, 1, 0]           # grad_offset (a checkerboard has no texels), kind
    assert np.array_equal(f32(out["textures"]["texels0"]), tex.ravel())
    s = out["area"]
    pmf, cdf, e = f32(s["area_pmf"]), f32(s["area_cdf"]), s["emitters"].reshape(-1, 36)[0]
    assert np.array_equal(pmf, F32([0, 0.5, 0.5, 0])) and np.array_equal(cdf, F32([0, 0.5, 1, 1]))
    assert (e[4], e[5], e[8], e[9]) == (0, 4, 1, 2)                               # first_prim, n_prims, valid_lo, valid_hi
    assert np.array_equal(f32(e[6:8]), F32([1, 1]))                               # area_sum, area_norm
    s = out["empty"]
    assert list(s["bvh"]) == [0x80000000, 0x80000000, 1, 0, 0] and flags(s)["n_prims"] == 0 and flags(s)["flat"] == 1


# ---- setter round trip -------------------------------------------------------------------------------------------------------------------
U, V, W = [0.25, 0.5, 0.75], [0.625, 0.125, 0.375], [0.875, 0.75, 0.5]


def _material(type, variant, texture=None, **kw):
    recs = [SPECTRAL] if variant == "spectral" else []
    fields = dict(texture=-1 if texture is None else 0, specular_reflectance=[0.75, 0.5, 0.25])
    fields.update(kw)
    recs += [mesh(2, 0, uv=1), mesh(1, 1, 0), bsdf(type, **fields), bsdf(), emitter(AREA)]
    return recs + ([bitmap(texture)] if texture is not None else [])


def roundtrip_cases():
    """name -> (records created with v, records created with u + the setter call)"""
    cases = {}
    for variant in ("rgb", "spectral"):
        def add(name, make, op):
            cases["%s/%s" % (variant, name)] = (make(V), make(U) + [op])
        for type, tname in ((DIFFUSE, "diffuse"), (PLASTIC, "plastic"), (ROUGHPLASTIC, "roughplastic")):
            add("reflectance_" + tname, lambda x, type=type: _material(type, variant, reflectance=x), ("set_reflectance", dict(bsdf=0, value=V)))
            add("reflectance_param_" + tname, lambda x, type=type: _material(type, variant, reflectance=x), ("set_param", dict(bsdf=0, kind=P_REFLECTANCE, value=V)))
            add("texture_" + tname, lambda x, type=type: _material(type, variant, texture=texels(int(x[0] * 8))),
                ("set_texture", dict(texture=0, value=texels(int(V[0] * 8)).ravel())))
        for type, tname in ((CONDUCTOR, "conductor"), (DIELECTRIC, "dielectric"), (PLASTIC, "plastic"), (ROUGHPLASTIC, "roughplastic")):
            add("specular_reflectance_" + tname, lambda x, type=type: _material(type, variant, specular_reflectance=x),
                ("set_param", dict(bsdf=0, kind=P_SPECULAR, value=V)))
        add("specular_transmittance", lambda x: _material(DIELECTRIC, variant, specular_transmittance=x), ("set_param", dict(bsdf=0, kind=P_TRANSMITTANCE, value=V)))
        uniform = variant == "spectral"           # the spectral variant takes one value for eta and k
        eu, ev = ([0.25] * 3, [0.625] * 3) if uniform else (U, V)
        add("eta", lambda x: _material(CONDUCTOR, variant, eta=ev if x is V else eu, k=[2, 2, 2]), ("set_param", dict(bsdf=0, kind=P_ETA, value=ev)))
        add("k", lambda x: _material(ROUGHCONDUCTOR, variant, k=ev if x is V else eu), ("set_param", dict(bsdf=0, kind=P_K, value=ev)))
        add("alpha", lambda x: _material(ROUGHCONDUCTOR, variant, alpha_u=x[0], alpha_v=x[0]), ("set_param", dict(bsdf=0, kind=P_ALPHA, value=[V[0]])))
        head = [SPECTRAL] if variant == "spectral" else []
        add("radiance_area", lambda x: head + [mesh(1, 0, 0), bsdf(), emitter(AREA, radiance=[4 * c for c in x])], ("set_radiance", dict(emitter=0, value=[4 * c for c in V])))
        add("radiance_point", lambda x: head + [mesh(1, 0), bsdf(), emitter(POINT, radiance=[4 * c for c in x])], ("set_radiance", dict(emitter=0, value=[4 * c for c in V])))
        add("envmap", lambda x: head + [mesh(1, 0), bsdf(), envmap(2 * texels(int(x[0] * 8), 4, 8))], ("set_envmap", dict(value=2 * texels(int(V[0] * 8), 4, 8).ravel())))
        # sequences on a textured (rough)plastic: the lobe weight reads the texture's mean and the specular mean, whichever was set last
        ta, tb, tc = texels(2), texels(5), texels(7)
        spec = lambda x: ("set_param", dict(bsdf=0, kind=P_SPECULAR, value=x))
        tex = lambda t: ("set_texture", dict(texture=0, value=t.ravel()))
        for type, tname in ((PLASTIC, "plastic"), (ROUGHPLASTIC, "roughplastic")):
            for sname, start, ops in (("specular_texels", U, [spec(V), tex(tb)]), ("texels_specular", U, [tex(tb), spec(V)]),
                                      ("specular_texels_specular", U, [spec(W), tex(tb), spec(V)]), ("texels_texels", V, [tex(tc), tex(tb)])):
                cases["%s/sequence_%s_%s" % (variant, sname, tname)] = (_material(type, variant, texture=tb, specular_reflectance=V),
                                                                         _material(type, variant, texture=ta, specular_reflectance=start) + ops)
    return cases


# Pairs that differ on purpose: host values the library has never kept in step with a setter (the setters were moved, not changed).
# name -> (key, word indices within it, reason)
KNOWN_STALE = {
    # mtsamd_scene_update_texture recomputes Texture::mean() only for a bitmap that feeds a (rough)plastic lobe weight, its one reader; the
    # device copy of the record is never refreshed either
    "rgb/texture_diffuse": ("textures", [18], "mean of a bitmap no lobe weight reads"),
}


def test_setter_round_trip(driver):
    cases = roundtrip_cases()
    scenes = {}
    for name, (a, b) in cases.items():
        scenes[name + "#created"], scenes[name + "#set"] = a, b
    out = driver(scenes)
    assert len(cases) == 2 * (20 + 2 * 4)          # + four sequences on each of the two textured plastics
    for name in cases:
        a, b = out[name + "#created"], out[name + "#set"]
        assert a["rc"] == 0 and b["rc"] == 0, (name, a["message"], b["message"])
        b.pop("changed_bsdfs", None)
        assert set(a) == set(b)
        for key in a:
            if key in ("rc", "message"):
                continue
            wa, wb = a[key].copy(), b[key].copy()
            assert wa.shape == wb.shape, (name, key)
            if key == "textures":                   # word 19 of a record is padding
                wa.reshape(-1, 20)[:, 19] = wb.reshape(-1, 20)[:, 19] = 0
            if name in KNOWN_STALE and KNOWN_STALE[name][0] == key:
                idx = KNOWN_STALE[name][1]
                assert not np.array_equal(wa[idx], wb[idx]), (name, "no longer stale: drop the entry")
                wa[idx] = wb[idx] = 0
            assert np.array_equal(wa, wb), (name, key, np.flatnonzero(wa != wb)[:8])
    # the conversions ran: a spectral plastic's weight follows both means, and its Jacobian is not empty
    s = out["spectral/reflectance_plastic#set"]
    kr, dm, sm = f32(s["bsdfs"].reshape(-1, 32)[0, 16:17])[0], f32(s["diff_mean"])[0], f32(s["spec_mean"])[0]
    assert kr == sm / (dm + sm) and 0 < kr < 1 and s["jac_bsdf"].size == 18 and s["jac_bsdf"][:9].any()
    s = out["rgb/texture_plastic#set"]
    kr, tm, sm = f32(s["bsdfs"].reshape(-1, 32)[0, 16:17])[0], f32(s["textures"].reshape(1, -1)[0, 18:19])[0], f32(s["spec_mean"])[0]
    assert kr == sm / (tm + sm) and sm == (F32(0.75) + F32(0.5) + F32(0.25)) * (F32(1) / F32(3))


# ---- error paths -------------------------------------------------------------------------------------------------------------------------
INVALID, UNSUPPORTED = -1, -5
ONE = [mesh(1, 0), bsdf()]
ZERO16 = [0] * 16
IOR_DIFFER = "The interior and exterior indices of refraction must be positive and differ!"
NESTED = "Only materials without a transmission component can be nested!"
ERRORS = {
    "empty_mesh": ([mesh(1, 0, empty=1), bsdf()], INVALID, "mesh 0: empty mesh"),
    "bsdf_index": ([mesh(1, 3), bsdf()], INVALID, "mesh 0: invalid bsdf index 3"),
    "emitter_index": ([mesh(1, 0, 2), bsdf()], INVALID, "mesh 0: invalid emitter index 2"),
    "texture_index": ([mesh(1, 0), bsdf(texture=1)], INVALID, "bsdf 0: invalid texture index 1"),
    "face_index": ([mesh(2, 0, badface=1), bsdf()], INVALID, "mesh 0: face index out of range"),
    "two_shapes_one_emitter": ([mesh(1, 0, 0), mesh(1, 0, 0), bsdf(), emitter(AREA)], INVALID, "An area emitter can be only be attached to a single shape."),
    "area_without_shape": (ONE + [emitter(AREA)], INVALID, "emitter 0 is not attached to a shape"),
    "environment_on_shape": ([mesh(1, 0, 0), bsdf(), emitter(CONSTANT)], INVALID, "emitter 0: an environment emitter cannot be attached to a shape"),
    "point_on_shape": ([mesh(1, 0, 0), bsdf(), emitter(POINT)], INVALID, "emitter 0: a point / spot / directional emitter cannot be attached to a shape"),
    "two_environments": (ONE + [emitter(CONSTANT), emitter(CONSTANT)], INVALID, "Only one environment emitter can be specified per scene."),
    "envmap_too_small": (ONE + [envmap(np.ones((2, 1, 3)))], INVALID, "emitter 0: the environment map must be at least 2x2 pixels in size"),
    "spot_cutoff": (ONE + [emitter(SPOT, cutoff_angle=10, beam_width=20)], INVALID, "emitter 0: spot: cutoff_angle must not be smaller than beam_width"),
    "spot_singular": (ONE + [emitter(POINT), emitter(SPOT, to_world=ZERO16)], INVALID, "emitter 1: singular to_world transformation"),
    "envmap_singular": (ONE + [envmap(np.ones((2, 2, 3)), to_world=ZERO16)], INVALID, "envmap: singular to_world transformation"),
    "emitter_kind": (ONE + [emitter(9)], UNSUPPORTED, "emitter 0: unknown emitter type 9"),
    "bsdf_kind": ([mesh(1, 0), bsdf(12)], UNSUPPORTED, "bsdf 0: unknown BSDF type 12"),
    "texture_kind": (ONE + [("texture", dict(kind=3))], UNSUPPORTED, "texture 0: unknown texture kind 3"),
    "texture_too_small": (ONE + [bitmap(np.ones((2, 1, 3)))], INVALID, "texture 0: image must be at least 2x2 pixels in size"),
    "spectral_eta": ([SPECTRAL, mesh(1, 0), bsdf(CONDUCTOR, eta=[0.1, 0.2, 0.3])], UNSUPPORTED,
                     "bsdf 0: the spectral variant needs uniform (constant) eta and k spectra, or tabulated ones (mtsamd_scene_create_with_spectra)"),
    "spectral_k": ([SPECTRAL, mesh(1, 0), bsdf(ROUGHCONDUCTOR, k=[1, 1, 2])], UNSUPPORTED,
                   "bsdf 0: the spectral variant needs uniform (constant) eta and k spectra, or tabulated ones (mtsamd_scene_create_with_spectra)"),
    "texture_on_conductor": ([mesh(1, 0), bsdf(CONDUCTOR, texture=0), checkerboard()], UNSUPPORTED,
                             "bsdf 0: textures are implemented for diffuse.reflectance and (rough)plastic.diffuse_reflectance only"),
    "roughplastic_ior": ([mesh(1, 0), bsdf(ROUGHPLASTIC, int_ior=1.5, ext_ior=1.5)], INVALID, IOR_DIFFER),
    "roughplastic_anisotropic": ([mesh(1, 0), bsdf(ROUGHPLASTIC, alpha_u=0.1, alpha_v=0.2)], INVALID,
                                 "The 'roughplastic' plugin currently does not support anisotropic microfacet distributions!"),
    "roughdielectric_ior": ([mesh(1, 0), bsdf(ROUGHDIELECTRIC, int_ior=-1)], INVALID, IOR_DIFFER),
    "dielectric_ior": ([mesh(1, 0), bsdf(DIELECTRIC, ext_ior=0)], INVALID, "The interior and exterior indices of refraction must be positive!"),
    "plastic_ior": ([mesh(1, 0), bsdf(PLASTIC, int_ior=-1.5)], INVALID, "The interior and exterior indices of refraction must be positive!"),
    "twosided_dielectric": ([mesh(1, 0), bsdf(THINDIELECTRIC, twosided=1)], INVALID, NESTED),
    "twosided_mask": ([mesh(1, 1), bsdf(), bsdf(MASK, nested=[0, -1], twosided=1)], INVALID, NESTED),
    "nested_index": ([mesh(1, 1), bsdf(), bsdf(BLEND, nested=[0, 5])], INVALID, "bsdf 1: nested[1] must index a plain BSDF record"),
    "nested_nested": ([mesh(1, 1), bsdf(), bsdf(MASK, nested=[1, -1])], INVALID, "bsdf 1: nested[0] must index a plain BSDF record"),
    "nested_textured_child": ([SPECTRAL, mesh(1, 1), bsdf(texture=0), bsdf(MASK, nested=[0, -1]), bitmap(texels(0))], UNSUPPORTED,
                              "bsdf 1: textured children of a blendbsdf / mask are implemented for the RGB variant only"),
    "nested_textured_weight": ([SPECTRAL, mesh(1, 1), bsdf(), bsdf(BLEND, nested=[0, 0], texture=0), checkerboard()], UNSUPPORTED,
                               "eval_1(): a bitmap / checkerboard weight is converted into spectra in the spectral variant (bitmap.cpp:218-222); use a constant"),
    "srgb_range": ([SPECTRAL, mesh(1, 0), bsdf(reflectance=[1.5, 0.25, 0.25])], INVALID, "Invalid RGB reflectance value [1.5, 0.25, 0.25], must be in the range [0, 1]!"),
    "srgb_range_specular": ([SPECTRAL, mesh(1, 0), bsdf(CONDUCTOR, specular_reflectance=[0.5, -0.5, 0.5])], INVALID,
                            "Invalid RGB reflectance value [0.5, -0.5, 0.5], must be in the range [0, 1]!"),
    "srgb_range_checkerboard": ([SPECTRAL, mesh(1, 0), bsdf(texture=0), checkerboard(color1=(0.5, 0.5, 2))], INVALID,
                                "Invalid RGB reflectance value in checkerboard texture 0, must be in the range [0, 1]!"),
    "no_probability_mass": ([mesh(2, 0, 0, degenerate=[0, 1]), bsdf(), emitter(AREA)], INVALID, "DiscreteDistribution: no probability mass found!"),
    "no_model": ([("spectral", dict(no_model=1)), mesh(1, 0), bsdf()], INVALID,
                 "Could not load sRGB-to-spectrum upsampling model ('/nonexistent/model.coeff'); build it with mtsamd_rgb2spec_build"),
}


def test_error_paths_of_the_builder(driver):
    out = driver({name: case[0] for name, case in ERRORS.items()})
    for name, (_, code, message) in ERRORS.items():
        assert (out[name]["rc"], out[name]["message"]) == (code, message), name


def _abi_scene(records, keep):
    """the same records as ctypes descriptors; the geometry follows tests/scene_build_driver.cpp"""
    meshes, tables = [], {"bsdf": [], "emitter": [], "texture": []}
    spectral, model = 0, None
    for rec, fields in records:
        if rec == "spectral":
            spectral, model = 1, b"/nonexistent/model.coeff" if fields.get("no_model") else MODEL.encode()
        elif rec == "mesh":
            n, i = fields["tris"], len(meshes)
            pos = np.array([[[k, 0, i], [k + 1, 0, i], [k, 1, i]] for k in range(n)], F32)
            faces = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
            for d in fields.get("degenerate", []):
                faces[d, 1:] = faces[d, 0]
            if fields.get("badface"):
                faces[-1, -1] = 3 * n
            keep += [pos, faces]
            meshes.append(L.MeshDesc(3 * n, 0 if fields.get("empty") else n, pos.ctypes.data_as(L.f32p), None, None, faces.ctypes.data_as(L.u32p),
                                     fields["bsdf"], fields["emitter"]))
        else:
            d = {"bsdf": L.BsdfDesc, "emitter": L.EmitterDesc, "texture": L.TextureDesc}[rec]()
            for k, v in fields.items():
                if k == "data":
                    v = np.ascontiguousarray(v, F32)
                    keep.append(v)
                    setattr(d, "envmap_data" if rec == "emitter" else "data", v.ctypes.data_as(L.f32p))
                elif np.ndim(v):
                    setattr(d, k, type(getattr(d, k))(*v))
                else:
                    setattr(d, k, v)
            tables[rec].append(d)

    def array(cls, items):
        a = (cls * max(len(items), 1))(*items)
        keep.append(a)
        return a, len(items)
    return L.SceneDesc(*array(L.MeshDesc, meshes), *array(L.BsdfDesc, tables["bsdf"]), *array(L.EmitterDesc, tables["emitter"]),
                       *array(L.TextureDesc, tables["texture"]), spectral, model)


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_error_paths_through_the_abi(name):
    """the built library reports them before it asks for a device: no GPU is needed"""
    records, code, message = ERRORS[name]
    keep = []
    sd = _abi_scene(records, keep)
    handle = C.c_void_p()
    lib = L.lib()
    assert lib.mtsamd_scene_create(C.byref(sd), 0, C.byref(handle)) == code
    assert lib.mtsamd_last_error().decode() == message
    assert not handle.value

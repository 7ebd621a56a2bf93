"""The setters of the C ABI against fresh scenes: a live scene after a setter renders the sample stream of a scene created with the new
value, bit for bit.  Every stream case (`_check`) creates the live scene with the old values, renders once so that the device holds the
old state, applies the setter(s), samples with PathIntegrator(max_depth=6), and compares rgb, mask and pos by equality with (a) a fresh
OracleScene built from the description with the new values (the reference; parity_util.check, exact fraction 1.0) and (b) a fresh GPU
scene with the new values (torch.equal; it tells a wrong setter from a wrong kernel).  No case passes vacuously: each asserts that the
oracle's streams of the old and the new description differ in at least 5 % of the samples (MOVED_MIN).

Scene classes.  flat: scenes.cornell_box() with the material on mesh 6, 48 x 48 at 4 spp (8 spp for the sequences), seed 21; open: the
open box of the environment tests (test_gpu_integrators._open_scene); hierarchy: scenes.bumpy_sphere(8, 16) with the material on the
sphere (bvh_nodes > 0), bumpy_sphere_sensor(24, 16, 8).  Bitmaps are 4 x 6, the envmap 8 x 16.

Families (test, setter, kind, variant, scene class):
A  test_constants: set_bsdf_reflectance and set_bsdf_param on every (model, kind) bsdf_param_fields accepts -- (diffuse_)reflectance of
   diffuse / plastic / roughplastic through both setters; specular_reflectance of conductor, roughconductor, dielectric,
   roughdielectric, thindielectric, plastic, roughplastic; specular_transmittance of the three dielectrics; eta and k of the two
   conductors; alpha of roughconductor / roughdielectric.  RGB, flat, pipelines 1, 2, 4 and the automatic one on one case per model.
B  test_nesting: the same setters on the record inside `twosided` (pipelines 1, 2, 4) and on child records of blendbsdf / mask (child
   indices from bsdfs.flatten).  RGB, flat, pipeline 1; a nested scene runs the fused kernels whatever the pipeline (schedule.cpp), so
   pipelines 2 and 4 are asserted to return the stream of pipeline 1.
C  test_textures: update_texture on a textured diffuse, plastic, roughplastic and a textured roughplastic child of a blend, from a device
   tensor and from a host array, and once under a non-identity to_uv.  RGB, flat, pipelines 1 and 2.
D  test_sequences: specular -> texels, texels -> specular, specular -> texels -> specular, texels twice on a textured plastic and a
   textured roughplastic.  RGB and spectral, flat, pipelines 1 and 2.  (RGB specular -> texels: the stale lobe weight this file found.)
E  test_emitters: set_emitter_radiance on area (flat), constant, point, spot, directional (open); update_envmap with a rebuilt
   hierarchy against a fresh scene, and without against OracleScene.update_envmap(data, rebuild_warp=False) alone (a fresh GPU scene
   always builds the hierarchy of its own texels).  RGB, pipelines 1, 2, 4.
F  test_spectral: specular_transmittance of the three dielectrics, alpha of roughconductor / roughdielectric, the srgb_d65 colours of
   the constant, point, spot and directional emitters.  Spectral, flat / open, pipelines 1 and 2.
G  test_hierarchy: roughconductor alpha, texels of a textured plastic, area radiance.  RGB and spectral, hierarchy, pipelines 1 and 2;
   pipeline 4 is asserted to be refused there.
H  test_refused_setters_change_nothing: an out-of-range colour and a non-uniform eta in a spectral scene, alpha of a roughplastic and of
   an anisotropic roughconductor, a kind the model lacks, update_texture on a checkerboard: the library's message, the stream after the
   failed call equals the stream before it, and a following successful setter still gives the fresh scene's stream.
I  test_adjoint_after_a_setter: equality of gradient tensors between the live and a fresh scene -- RGB mtsamd_render_adjoint_param on a
   roughconductor's alpha after set_bsdf_param; spectral replay: the reflectance gradient after set_bsdf_reflectance (the device
   Jacobian behind jac_dirty) and the emitter gradient after set_emitter_radiance (ejac_dirty).  No existing test asserts these.  The
   gradients are sums of float atomics, which are equal between two runs only if the order of the terms is fixed: the RGB kernel adds
   one in-order total per workgroup, so its case has one workgroup (16 x 16 x 1 = 256 samples); the spectral kernels add per lane into
   LDS, so their cases have one wave (8 x 8 x 1 = 64 samples).  Each case also asserts that the setter moved the gradient.
J  test_product_path: autodiff.traverse on an RGB general scene with a textured plastic; new specular_reflectance.value and new texels,
   update(); the raw film equals the film of a fresh scene with both.

Share of samples the oracle moves between the old and the new description, measured on the host (the issue lists plastic specular
12.8 %, roughconductor alpha 13.3 %, dielectric transmittance 8.7 %, plastic texels 13.6 %); every other case, by family, least first:
A  dielectric-specular_reflectance 6.2, roughdielectric-specular_reflectance 7.3, thindielectric-specular_reflectance 7.5,
   dielectric-specular_transmittance 8.7, thindielectric-specular_transmittance 8.7, roughdielectric-specular_transmittance 9.0,
   conductor-eta 10.4, conductor-k 10.4, conductor-specular_reflectance 10.4, plastic-specular_reflectance 12.8,
   roughplastic-specular_reflectance 12.8, roughconductor-eta 13.4, roughconductor-k 13.4, roughconductor-specular_reflectance 13.4,
   diffuse-reflectance 13.7, diffuse-reflectance-set_reflectance 13.7, plastic-diffuse_reflectance 13.7,
   plastic-diffuse_reflectance-set_reflectance 13.7, roughplastic-diffuse_reflectance 13.7,
   roughplastic-diffuse_reflectance-set_reflectance 13.7, roughconductor-alpha 14.0, roughdielectric-alpha 15.2
B  mask-child-specular 9.6, blend-child1-reflectance 10.4, blend-child1-reflectance-param 10.4, mask-twosided-child-reflectance 12.4,
   blend-child0-alpha 12.5, twosided-diffuse-reflectance 13.7, twosided-roughconductor-alpha 14.0
C  blend-child-roughplastic-device 11.1, blend-child-roughplastic-host 11.1, diffuse-device 13.7, diffuse-host 13.7, plastic-device
   13.7, plastic-host 13.7, plastic-to_uv-device 13.7, roughplastic-device 13.7, roughplastic-host 13.7
D  rgb-plastic-texels_texels 13.7, rgb-roughplastic-specular_texels 13.7, rgb-roughplastic-specular_texels_specular 13.7,
   rgb-roughplastic-texels_specular 13.7, rgb-roughplastic-texels_texels 13.7, spectral-plastic-texels_texels 13.7,
   spectral-roughplastic-specular_texels 13.7, spectral-roughplastic-specular_texels_specular 13.7,
   spectral-roughplastic-texels_specular 13.7, spectral-roughplastic-texels_texels 13.7, rgb-plastic-specular_texels 13.8,
   rgb-plastic-specular_texels_specular 13.8, rgb-plastic-texels_specular 13.8, spectral-plastic-specular_texels 13.8,
   spectral-plastic-specular_texels_specular 13.8, spectral-plastic-texels_specular 13.8
E  spot 12.4, directional 22.1, point 28.0, area 78.2, constant 94.6, envmap_keep 95.2, envmap 96.1
F  dielectric-specular_transmittance 8.7, thindielectric-specular_transmittance 8.7, roughdielectric-specular_transmittance 9.0,
   emitter-spot 12.4, roughconductor_uniform-alpha 14.0, roughdielectric-alpha 15.3, emitter-directional 22.1, emitter-point 28.0,
   emitter-constant 94.6
G  rgb-roughconductor-alpha 19.1, spectral-plastic-texels 19.1, spectral-roughconductor-alpha 19.1, rgb-plastic-texels 19.2,
   rgb-area-radiance 44.6, spectral-area-radiance 44.6
H (the setter that follows the refusal)  checkerboard-texels 12.8, roughplastic-alpha 12.8, anisotropic-alpha 13.3, kind-the-model-lacks
   13.7, spectral-colour-out-of-range 13.7, spectral-nonuniform-eta 14.0, spectral-nonuniform-k 14.0
"""
import copy
import ctypes as C

import numpy as np
import parity_util
import pytest
import torch

from mitsuba2_amd import scenes

pytestmark = pytest.mark.gpu

MOVED_MIN = 0.05
KIND = {"reflectance": 0, "diffuse_reflectance": 0, "specular_reflectance": 1, "eta": 2, "k": 3, "alpha": 4, "specular_transmittance": 5}
U, V, W = [0.25, 0.5, 0.75], [0.625, 0.125, 0.375], [0.875, 0.75, 0.5]
GREY = [0.1, 0.27, 0.36]


def _texels(seed, shape=(4, 6, 3)):
    return np.random.default_rng(seed).uniform(0.1, 0.9, size=shape).astype(np.float32)


TEX_A, TEX_B, TEX_C = _texels(7), _texels(8), _texels(9)
TO_UV = [[3.0, 0, 0.25, 0], [0, 5.0, 0.1, 0], [0, 0, 1, 0], [0, 0, 0, 1]]      # the third column is the translation (Transform4f::extract)

MODELS = {
    "diffuse": {"type": "diffuse", "reflectance": U},
    "plastic": {"type": "plastic", "diffuse_reflectance": GREY, "specular_reflectance": U, "int_ior": 1.9},
    "roughplastic": {"type": "roughplastic", "alpha": 0.15, "diffuse_reflectance": GREY, "specular_reflectance": U},
    "conductor": {"type": "conductor", "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14], "specular_reflectance": [0.9, 0.8, 0.7]},
    "roughconductor": {"type": "roughconductor", "alpha": 0.2, "distribution": "ggx", "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14],
                       "specular_reflectance": [0.9, 0.8, 0.7]},
    "dielectric": {"type": "dielectric", "int_ior": "bk7", "specular_reflectance": [0.9, 0.8, 0.7], "specular_transmittance": [0.9, 0.95, 1.0]},
    "roughdielectric": {"type": "roughdielectric", "alpha": 0.2, "specular_reflectance": [0.9, 0.8, 0.7], "specular_transmittance": [0.9, 0.95, 1.0]},
    "thindielectric": {"type": "thindielectric", "specular_reflectance": [0.9, 0.8, 0.7], "specular_transmittance": [0.9, 0.95, 1.0]},
    # specular_reflectance of a smooth dielectric moves only the paths with a reflection event on it: 4.2 % / 3.1 % of the samples at
    # bk7's index, 6.2 % / 7.5 % at 6.0
    "dielectric_dense": {"type": "dielectric", "int_ior": 6.0, "specular_reflectance": [0.9, 0.8, 0.7], "specular_transmittance": [0.9, 0.95, 1.0]},
    "thindielectric_dense": {"type": "thindielectric", "int_ior": 6.0, "specular_reflectance": [0.9, 0.8, 0.7], "specular_transmittance": [0.9, 0.95, 1.0]},
    # uniform eta / k: what the spectral variant accepts
    "roughconductor_uniform": {"type": "roughconductor", "alpha": 0.2, "distribution": "ggx", "eta": 0.2, "k": 3.9, "specular_reflectance": [0.9, 0.8, 0.7]},
}


def _textured(model, to_uv=None, **kw):
    tex = {"type": "bitmap", "data": TEX_A.copy()}
    if to_uv is not None:
        tex["to_uv"] = to_uv
    if model == "diffuse":
        return {"type": "diffuse", "reflectance": tex}
    return dict(MODELS[model], diffuse_reflectance=tex, **kw)


# ---- scenes: (description, index of the record under test, sensor parameters) ----------------------------------------------------------
def _flat(material, spp=4):
    cb = scenes.cornell_box()
    cb["bsdfs"] = list(cb["bsdfs"]) + [copy.deepcopy(material)]
    cb["meshes"][6] = dict(cb["meshes"][6], bsdf=len(cb["bsdfs"]) - 1)
    return cb, len(cb["bsdfs"]) - 1, dict(scenes.cornell_box_sensor(48, 48, spp=spp, seed=21), max_depth=6)


def _hierarchy(material):
    sd = scenes.bumpy_sphere(8, 16)
    sd["bsdfs"][0] = copy.deepcopy(material)
    return sd, 0, dict(scenes.bumpy_sphere_sensor(24, 16, 8), max_depth=6)


def _envmap_image(seed, bright):
    img = np.random.default_rng(seed).uniform(0.05, 1.0, size=(8, 16, 3)).astype(np.float32)
    img[bright[0]:bright[0] + 2, bright[1]:bright[1] + 2] += 30.0              # a small bright region: the sampling hierarchy matters
    return img


def _open(emitter):
    """the open box under / next to `emitter` (index 0), with the area light kept (index 1)"""
    from test_gpu_integrators import _open_scene
    cb = _open_scene(True)
    cb["emitters"] = [copy.deepcopy(emitter)] + [e for e in cb["emitters"] if e.get("type", "area") == "area"]
    return cb, None, dict(scenes.cornell_box_sensor(48, 48, spp=4, seed=21), max_depth=6)


SPOT_TO_WORLD = scenes.look_at([278, 500, 200], [300, 0, 320], [0, 0, 1])
EMITTERS = {
    "constant": ({"type": "constant", "radiance": [0.4, 0.6, 1.0]}, "radiance", [0.9, 0.5, 0.3]),
    "point": ({"type": "point", "position": [278, 400, 279], "intensity": [4e5, 3e5, 2e5]}, "intensity", [2e5, 3e5, 5e5]),
    "spot": ({"type": "spot", "to_world": SPOT_TO_WORLD, "intensity": [9e5, 9e5, 6e5], "cutoff_angle": 35.0, "beam_width": 20.0}, "intensity", [5e5, 7e5, 9e5]),
    "directional": ({"type": "directional", "direction": [0.3, -1.0, 0.4], "irradiance": [3.0, 2.5, 2.0]}, "irradiance", [1.5, 2.0, 3.5]),
}


# ---- steps: (where, key, value[, via]) -- one setter call on the live scene, one edit of the description -----------------------------------
# where: ("bsdf", top-level index, *keys down to the plugin dictionary of the record) or ("emitter", index)
# key: a parameter name of KIND, "texels", the emitter's value key, "envmap" (hierarchy rebuilt) or "envmap_keep" (hierarchy kept)
def _leaf(sd, where):
    node = sd["bsdfs"][where[1]]
    for k in where[2:]:
        node = node[k]
    return node


def _texture_key(leaf):
    return "reflectance" if leaf["type"] == "diffuse" else "diffuse_reflectance"


def _flat_index(sd, where):
    """index of the record in the device's table: top-level records keep their place, children follow them (bsdfs.flatten)"""
    from mitsuba2_amd import bsdfs as B
    records = [B.normalize(b) for b in sd["bsdfs"]]
    B.flatten(records)
    top, rec = sd["bsdfs"][where[1]], records[where[1]]
    if rec["type"] not in (B.BLEND, B.MASK):
        return where[1]
    children = [k for k, v in top.items() if k not in ("type", "id", "weight", "opacity") and isinstance(v, dict)]
    return rec["nested"][children.index(where[2])]


def _edit(sd, step):
    where, key, value = step[:3]
    if where[0] == "emitter":
        sd["emitters"][where[1]]["data" if key.startswith("envmap") else key] = np.array(value, np.float32)
        return
    leaf = _leaf(sd, where)
    if key == "texels":
        leaf[_texture_key(leaf)] = dict(leaf[_texture_key(leaf)], data=np.array(value, np.float32))
    else:
        leaf[key] = float(value) if key == "alpha" else [float(x) for x in value]


def _push(scene, sd, step):
    where, key, value = step[:3]
    via = step[3] if len(step) > 3 else None
    if where[0] == "emitter":
        if key.startswith("envmap"):
            scene.update_envmap(np.array(value, np.float32), rebuild_distribution=key == "envmap")
        else:
            scene.set_emitter_radiance(where[1], value)
        return
    index = _flat_index(sd, where)
    if key == "texels":
        texture = scene.texture_index(index)
        assert texture is not None
        scene.update_texture(texture, np.array(value, np.float32) if via == "host" else torch.from_numpy(np.array(value, np.float32)).cuda())
    elif via == "reflectance":
        scene.set_bsdf_reflectance(index, value)
    else:
        scene.set_bsdf_param(index, KIND[key], [value] if key == "alpha" else value)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
def _case(scene, steps, pipelines, variant="rgb", nested=False):
    sd, index, p = scene
    steps = [((("bsdf", index) + s[0][1:]) if s[0][0] == "material" else s[0],) + tuple(s[1:]) for s in steps]
    return dict(old=sd, steps=steps, p=p, pipelines=pipelines, variant=variant, nested=nested)


M = ("material",)          # the record under test; ("material", key, ...) walks into its plugin dictionary


def _constants():
    out, seen = {}, set()
    rows = [(m, k, V, via) for m, k in (("diffuse", "reflectance"), ("plastic", "diffuse_reflectance"), ("roughplastic", "diffuse_reflectance"))
            for via in ("reflectance", "param")]
    rows += [(m, "specular_reflectance", V, "param") for m in ("conductor", "roughconductor", "dielectric_dense", "roughdielectric", "thindielectric_dense", "plastic", "roughplastic")]
    rows += [(m, "specular_transmittance", [0.5, 0.7, 0.6], "param") for m in ("dielectric", "roughdielectric", "thindielectric")]
    rows += [(m, k, v, "param") for m in ("conductor", "roughconductor") for k, v in (("eta", [0.3, 0.6, 1.4]), ("k", [3.0, 2.0, 2.5]))]
    rows += [(m, "alpha", 0.3, "param") for m in ("roughconductor", "roughdielectric")]
    for model, key, value, via in rows:
        name = model.replace("_dense", "")
        pipelines = (1, 2, 4) if name in seen else (0, 1, 2, 4)          # the automatic schedule on one case per model
        seen.add(name)
        out["%s-%s%s" % (name, key, "-set_reflectance" if via == "reflectance" else "")] = _case(_flat(MODELS[model]), [(M, key, value, via)], pipelines)
    return out


def _nesting():
    rough, diffuse = MODELS["roughconductor"], MODELS["diffuse"]
    blend = {"type": "blendbsdf", "weight": 0.3, "bsdf_0": rough, "bsdf_1": diffuse}
    return {
        "twosided-diffuse-reflectance": _case(_flat({"type": "twosided", "bsdf": diffuse}), [(M + ("bsdf",), "reflectance", V, "reflectance")], (1, 2, 4)),
        "twosided-roughconductor-alpha": _case(_flat({"type": "twosided", "bsdf": rough}), [(M + ("bsdf",), "alpha", 0.3)], (1, 2, 4)),
        "blend-child0-alpha": _case(_flat(blend), [(M + ("bsdf_0",), "alpha", 0.3)], (1,), nested=True),
        "blend-child1-reflectance": _case(_flat(blend), [(M + ("bsdf_1",), "reflectance", V, "reflectance")], (1,), nested=True),
        "blend-child1-reflectance-param": _case(_flat(blend), [(M + ("bsdf_1",), "reflectance", V)], (1,), nested=True),
        "mask-child-specular": _case(_flat({"type": "mask", "opacity": 0.6, "nested": MODELS["plastic"]}), [(M + ("nested",), "specular_reflectance", V)], (1,), nested=True),
        "mask-twosided-child-reflectance": _case(_flat({"type": "mask", "opacity": 0.6, "nested": {"type": "twosided", "bsdf": diffuse}}),
                                                 [(M + ("nested", "bsdf"), "reflectance", V, "reflectance")], (1,), nested=True),
    }


def _textures():
    out = {}
    for source in ("device", "host"):
        for model in ("diffuse", "plastic", "roughplastic"):
            out["%s-%s" % (model, source)] = _case(_flat(_textured(model)), [(M, "texels", TEX_B, source)], (1, 2))
        blend = {"type": "blendbsdf", "weight": 0.45, "bsdf_0": MODELS["diffuse"], "bsdf_1": _textured("roughplastic")}
        out["blend-child-roughplastic-%s" % source] = _case(_flat(blend), [(M + ("bsdf_1",), "texels", TEX_B, source)], (1,), nested=True)
    out["plastic-to_uv-device"] = _case(_flat(_textured("plastic", to_uv=TO_UV)), [(M, "texels", TEX_B, "device")], (1, 2))
    return out


SEQUENCES = {
    "specular_texels": [(M, "specular_reflectance", V), (M, "texels", TEX_B)],
    "texels_specular": [(M, "texels", TEX_B), (M, "specular_reflectance", V)],
    "specular_texels_specular": [(M, "specular_reflectance", W), (M, "texels", TEX_B), (M, "specular_reflectance", V)],
    "texels_texels": [(M, "texels", TEX_C), (M, "texels", TEX_B)],
}


def _sequences():
    return {"%s-%s-%s" % (variant, model, name): _case(_flat(_textured(model), spp=8), steps, (1, 2), variant)
            for variant in ("rgb", "spectral") for model in ("plastic", "roughplastic") for name, steps in SEQUENCES.items()}


def _emitters():
    out = {"area": _case(_flat(MODELS["roughconductor"]), [(("emitter", 0), "radiance", [10.0, 12.0, 15.0])], (1, 2, 4))}
    for name, (emitter, key, value) in EMITTERS.items():
        out[name] = _case(_open(emitter), [(("emitter", 0), key, value)], (1, 2, 4))
    env = {"type": "envmap", "data": _envmap_image(5, (2, 10)), "scale": 0.7, "to_world": scenes.look_at([0, 0, 0], [1, 0.2, 0.3], [0, 1, 0])}
    for key in ("envmap", "envmap_keep"):
        out[key] = _case(_open(env), [(("emitter", 0), key, _envmap_image(6, (4, 3)))], (1, 2, 4))
    return out


def _spectral():
    out = {"%s-specular_transmittance" % m: _case(_flat(MODELS[m]), [(M, "specular_transmittance", [0.5, 0.7, 0.6])], (1, 2), "spectral")
           for m in ("dielectric", "roughdielectric", "thindielectric")}
    for m in ("roughconductor_uniform", "roughdielectric"):
        out["%s-alpha" % m] = _case(_flat(MODELS[m]), [(M, "alpha", 0.3)], (1, 2), "spectral")
    for name, (emitter, key, value) in EMITTERS.items():
        out["emitter-" + name] = _case(_open(emitter), [(("emitter", 0), key, value)], (1, 2), "spectral")
    return out


def _hierarchies():
    out = {}
    for variant in ("rgb", "spectral"):
        out[variant + "-roughconductor-alpha"] = _case(_hierarchy(MODELS["roughconductor_uniform"]), [(M, "alpha", 0.3)], (1, 2), variant)
        out[variant + "-plastic-texels"] = _case(_hierarchy(_textured("plastic")), [(M, "texels", TEX_B)], (1, 2), variant)
        out[variant + "-area-radiance"] = _case(_hierarchy(MODELS["roughconductor_uniform"]), [(("emitter", 0), "radiance", [10.0, 12.0, 15.0])], (1, 2), variant)
    return out


FAMILIES = {"constants": _constants(), "nesting": _nesting(), "textures": _textures(), "sequences": _sequences(), "emitters": _emitters(),
            "spectral": _spectral(), "hierarchy": _hierarchies()}


# ---- the invariant ---------------------------------------------------------------------------------------------------------------------------
_REFERENCES = {}


def _described(old, steps):
    new = copy.deepcopy(old)
    for step in steps:
        _edit(new, step)
    return new


def _oracle_streams(oracle, key, case, spectral_path):
    """(stream of the old description, stream of the new one, positions), each from a fresh OracleScene; computed once per case"""
    if key not in _REFERENCES:
        p = case["p"]
        n = p["width"] * p["height"] * p["sample_count"]
        desc = oracle.make_desc(p)
        path = spectral_path if case["variant"] == "spectral" else None
        before, _ = oracle.OracleScene(copy.deepcopy(case["old"]), spectral_path=path).sample_radiance(desc, 0, n)
        if any(s[1] == "envmap_keep" for s in case["steps"]):           # the texels change, the sampling hierarchy stays the old one's
            kept = oracle.OracleScene(copy.deepcopy(case["old"]), spectral_path=path)
            kept.update_envmap(case["steps"][0][2], rebuild_warp=False)
            after, pos = kept.sample_radiance(desc, 0, n)
        else:
            after, pos = oracle.OracleScene(_described(case["old"], case["steps"]), spectral_path=path).sample_radiance(desc, 0, n)
        for a in (before, after, pos):
            a.setflags(write=False)
        _REFERENCES[key] = (before, after, pos)
    return _REFERENCES[key]


def moved_share(before, after):
    return float((before != after).any(1).mean())


def _sample(integ, scene, sensor, n):
    rgb, mask, pos = integ.sample(scene, sensor, 0, n)
    return rgb.clone(), mask.clone(), pos.clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _against_references(gpu, case, label, got, want, wpos, integ, sensor, n, fresh=True):
    """(a) the oracle's stream of the new description, (b) a fresh GPU scene with the new values"""
    rgb, mask, pos = got
    same_fresh = None
    if fresh:
        same_fresh = _same(got, _sample(integ, gpu.Scene(_described(case["old"], case["steps"]), variant=case["variant"]), sensor, n))
    try:
        assert np.array_equal(pos.cpu().numpy(), wpos) and np.array_equal(mask.cpu().numpy(), want[:, 3] > 0.5), (label, "positions / mask differ from the oracle's")
        parity_util.check(label, rgb.cpu().numpy(), want[:, :3])
    except AssertionError as e:
        raise AssertionError("%s [the live scene equals a fresh GPU scene: %s]" % (e, same_fresh)) from None
    assert same_fresh is not False, (label, "the oracle's stream, but not the stream of a fresh GPU scene")


def _check(gpu, oracle, family, name):
    case = FAMILIES[family][name]
    p, variant = case["p"], case["variant"]
    n = p["width"] * p["height"] * p["sample_count"]
    before, want, wpos = _oracle_streams(oracle, (family, name), case, gpu.srgb_coeff_path() if variant == "spectral" else None)
    moved = moved_share(before, want)
    print("%s/%s: the setter moves %.1f %% of the oracle's samples" % (family, name, 100.0 * moved))
    assert moved >= MOVED_MIN, (name, moved)
    keep = any(s[1] == "envmap_keep" for s in case["steps"])
    for pipeline in case["pipelines"]:
        integ, sensor = gpu.PathIntegrator(max_depth=6, pipeline=pipeline), gpu.make_sensor(p)
        live = gpu.Scene(copy.deepcopy(case["old"]), variant=variant)
        assert integ.render(live, sensor)                     # the device holds the old state: workspace, staged records, tables
        for step in case["steps"]:
            _push(live, case["old"], step)
        got = _sample(integ, live, sensor, n)
        _against_references(gpu, case, "%s/%s pipeline %d" % (family, name, pipeline), got, want, wpos, integ, sensor, n, fresh=not keep)
        if case["nested"]:           # blendbsdf / mask: only the fused kernels carry the nesting code, whatever pipeline is asked for
            for other in (2, 4):
                assert _same(got, _sample(gpu.PathIntegrator(max_depth=6, pipeline=other), live, sensor, n)), (name, other)
    return live


@pytest.mark.parametrize("name", sorted(FAMILIES["constants"]))
def test_constants(gpu, oracle, name):
    _check(gpu, oracle, "constants", name)


@pytest.mark.parametrize("name", sorted(FAMILIES["nesting"]))
def test_nesting(gpu, oracle, name):
    _check(gpu, oracle, "nesting", name)


@pytest.mark.parametrize("name", sorted(FAMILIES["textures"]))
def test_textures(gpu, oracle, name):
    _check(gpu, oracle, "textures", name)


@pytest.mark.parametrize("name", sorted(FAMILIES["sequences"]))
def test_sequences(gpu, oracle, name):
    _check(gpu, oracle, "sequences", name)


@pytest.mark.parametrize("name", sorted(FAMILIES["emitters"]))
def test_emitters(gpu, oracle, name):
    _check(gpu, oracle, "emitters", name)


@pytest.mark.parametrize("name", sorted(FAMILIES["spectral"]))
def test_spectral(gpu, oracle, name):
    _check(gpu, oracle, "spectral", name)


@pytest.mark.parametrize("name", sorted(FAMILIES["hierarchy"]))
def test_hierarchy(gpu, oracle, name):
    live = _check(gpu, oracle, "hierarchy", name)
    assert live.info()["bvh_nodes"] > 0 and live.info()["primitives"] > 64
    p = FAMILIES["hierarchy"][name]["p"]
    with pytest.raises(RuntimeError, match="LDS-resident scenes only"):
        gpu.PathIntegrator(max_depth=6, pipeline=4).sample(live, gpu.make_sensor(p), 0, 64)


# ---- H: refused setters ----------------------------------------------------------------------------------------------------------------------
def _checkerboard_update(scene, sd, where):
    """mtsamd_scene_update_texture itself: Scene.update_texture refuses a checkerboard before the library sees it (it has no texel shape)"""
    from mitsuba2_amd import _lib as L
    texels = np.zeros((2, 2, 3), np.float32)
    L.check(L.lib().mtsamd_scene_update_texture(scene._handle, scene.texture_index(_flat_index(sd, where)), texels.ctypes.data_as(C.c_void_p), None))


CHECKER = {"type": "checkerboard", "color0": [0.8, 0.2, 0.1], "color1": [0.1, 0.3, 0.7]}
REFUSED = {
    # name: (variant, material, the refused call (scene, description, where), the library's message, a setter that works)
    "spectral-colour-out-of-range": ("spectral", MODELS["diffuse"], lambda s, sd, w: s.set_bsdf_reflectance(_flat_index(sd, w), [1.2, 0.1, 0.1]),
                                     r"Invalid RGB reflectance value \[1\.2, 0\.1, 0\.1\], must be in the range \[0, 1\]!", (M, "reflectance", V, "reflectance")),
    "spectral-nonuniform-eta": ("spectral", MODELS["roughconductor_uniform"], lambda s, sd, w: s.set_bsdf_param(_flat_index(sd, w), KIND["eta"], [0.2, 0.9, 1.1]),
                                r"the spectral variant needs uniform \(constant\) eta and k spectra", (M, "alpha", 0.3)),
    "spectral-nonuniform-k": ("spectral", MODELS["roughconductor_uniform"], lambda s, sd, w: s.set_bsdf_param(_flat_index(sd, w), KIND["k"], [3.9, 2.4, 2.1]),
                              r"the spectral variant needs uniform \(constant\) eta and k spectra", (M, "alpha", 0.3)),
    "roughplastic-alpha": ("rgb", MODELS["roughplastic"], lambda s, sd, w: s.set_bsdf_param(_flat_index(sd, w), KIND["alpha"], [0.3]),
                           r"bsdf 4 \(type 5\) has no settable parameter of kind 4", (M, "specular_reflectance", V)),
    "anisotropic-alpha": ("rgb", dict({k: v for k, v in MODELS["roughconductor"].items() if k != "alpha"}, alpha_u=0.3, alpha_v=0.1), lambda s, sd, w: s.set_bsdf_param(_flat_index(sd, w), KIND["alpha"], [0.3]),
                          r"bsdf 4 \(type 2\) has no settable parameter of kind 4", (M, "specular_reflectance", V)),
    "kind-the-model-lacks": ("rgb", MODELS["diffuse"], lambda s, sd, w: s.set_bsdf_param(_flat_index(sd, w), KIND["specular_reflectance"], V),
                             r"bsdf 4 \(type 0\) has no settable parameter of kind 1", (M, "reflectance", V)),
    "checkerboard-texels": ("rgb", dict(MODELS["plastic"], diffuse_reflectance=CHECKER), _checkerboard_update, r"texture 0 is not a bitmap", (M, "specular_reflectance", V)),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_setters_change_nothing(gpu, oracle, name):
    variant, material, refused, message, good = REFUSED[name]
    case = _case(_flat(material), [good], (1,), variant)
    where, p = case["steps"][0][0], case["p"]
    n = p["width"] * p["height"] * p["sample_count"]
    before, want, wpos = _oracle_streams(oracle, ("refused", name), case, gpu.srgb_coeff_path() if variant == "spectral" else None)
    assert moved_share(before, want) >= MOVED_MIN
    integ, sensor = gpu.PathIntegrator(max_depth=6, pipeline=1), gpu.make_sensor(p)
    live = gpu.Scene(copy.deepcopy(case["old"]), variant=variant)
    assert integ.render(live, sensor)
    stream = _sample(integ, live, sensor, n)
    with pytest.raises(RuntimeError, match=message):
        refused(live, case["old"], where)
    assert _same(stream, _sample(integ, live, sensor, n))                       # the scene is as it was
    parity_util.check(name + " before", stream[0].cpu().numpy(), before[:, :3])
    _push(live, case["old"], case["steps"][0])
    _against_references(gpu, case, "refused/" + name, _sample(integ, live, sensor, n), want, wpos, integ, sensor, n)


# ---- I: the adjoint after a setter -----------------------------------------------------------------------------------------------------------
def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _param_gradient(scene, d, dimage, index):
    from mitsuba2_amd import _lib as L, autodiff
    film, g = autodiff._render_film(scene, d), torch.zeros(1, device="cuda")
    L.check(L.lib().mtsamd_render_adjoint_param(scene._handle, C.byref(d), _ptr(dimage), _ptr(film), index, KIND["alpha"], 0, 0.0, _ptr(g), None))
    torch.cuda.synchronize()
    return film, g


def _reflectance_gradient(scene, d, dimage, index):
    from mitsuba2_amd import _lib as L, autodiff
    film, g = autodiff._render_film(scene, d), torch.zeros((len(scene._dict["bsdfs"]), 3), device="cuda")
    L.check(L.lib().mtsamd_render_adjoint_spectral(scene._handle, C.byref(d), _ptr(dimage), _ptr(film), _ptr(g), None, None))
    torch.cuda.synchronize()
    return film, g


def _emitter_gradient(scene, d, dimage, index):
    from mitsuba2_amd import _lib as L, autodiff
    film, g = autodiff._render_film(scene, d), torch.zeros((len(scene._dict["emitters"]), 3), device="cuda")
    L.check(L.lib().mtsamd_render_adjoint_spectral_emitters(scene._handle, C.byref(d), _ptr(dimage), _ptr(film), _ptr(g), None, None))
    torch.cuda.synchronize()
    return film, g


ADJOINTS = {
    # name: (variant, scene, step, film size: one workgroup / one wave (module docstring), gradient)
    "rgb-alpha": ("rgb", lambda: _flat(MODELS["roughconductor"]), (M, "alpha", 0.3), 16, _param_gradient),
    "spectral-reflectance": ("spectral", lambda: (scenes.cornell_box(), 1, None), (M, "reflectance", [0.2, 0.5, 0.3], "reflectance"), 8, _reflectance_gradient),
    "spectral-emitter": ("spectral", lambda: (scenes.cornell_box(), 1, None), (("emitter", 0), "radiance", [10.0, 12.0, 15.0]), 8, _emitter_gradient),
}


@pytest.mark.parametrize("name", sorted(ADJOINTS))
def test_adjoint_after_a_setter(gpu, name):
    from mitsuba2_amd import autodiff
    variant, build, step, size, gradient = ADJOINTS[name]
    sd, index, _ = build()
    p = scenes.cornell_box_sensor(size, size, spp=1, seed=77, max_depth=5)
    case = _case((sd, index, p), [step], (1,), variant)
    sensor = gpu.make_sensor(p)
    dimage = torch.from_numpy(np.random.RandomState(4).uniform(-1.0, 1.0, (size, size, 3)).astype(np.float32)).cuda()
    live = gpu.Scene(copy.deepcopy(sd), variant=variant)
    d = autodiff._desc(live, sensor, gpu.PathIntegrator(max_depth=5), 1, 77)
    film_old, g_old = gradient(live, d, dimage, index)           # the device holds the old state, the Jacobians of the old colours included
    _push(live, sd, case["steps"][0])
    film, g = gradient(live, d, dimage, index)
    film_fresh, g_fresh = gradient(gpu.Scene(_described(sd, case["steps"]), variant=variant), d, dimage, index)
    print("%s: gradient before %s, after %s, fresh %s" % (name, g_old.flatten().tolist(), g.flatten().tolist(), g_fresh.flatten().tolist()))
    assert torch.isfinite(g).all() and bool((g != 0).any()) and not torch.equal(g, g_old) and not torch.equal(film, film_old)
    assert torch.equal(film, film_fresh)
    assert torch.equal(g, g_fresh), (name, g.flatten().tolist(), g_fresh.flatten().tolist())


# ---- J: the product path ---------------------------------------------------------------------------------------------------------------------
def test_product_path(gpu):
    """ParameterMap.update() pushes the constants before the texels (insertion order): the order that left the lobe weight stale"""
    from mitsuba2_amd import autodiff
    sd, index, p = _flat(dict(_textured("plastic"), id="box"))
    live, sensor = gpu.Scene(copy.deepcopy(sd)), gpu.make_sensor(p)
    integ = gpu.PathIntegrator(max_depth=6)
    assert integ.render(live, sensor)
    old_film = sensor.film().bitmap(raw=True).clone()
    params = autodiff.traverse(live)
    keys = list(params.keys())
    assert "box.specular_reflectance.value" in keys and "box.diffuse_reflectance.data" in keys
    assert keys.index("box.specular_reflectance.value") < keys.index("box.diffuse_reflectance.data")
    params["box.specular_reflectance.value"] = V
    params["box.diffuse_reflectance.data"] = TEX_B
    params.update()
    assert integ.render(live, sensor)
    film = sensor.film().bitmap(raw=True).clone()
    new = _described(sd, [(("bsdf", index), "specular_reflectance", V), (("bsdf", index), "texels", TEX_B)])
    sensor2 = gpu.make_sensor(p)
    assert integ.render(gpu.Scene(new), sensor2)
    assert not torch.equal(film, old_film)
    assert torch.equal(film, sensor2.film().bitmap(raw=True))

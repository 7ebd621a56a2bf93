"""Differentiable rendering: the counterpart of ``mitsuba.python.autodiff`` / ``mitsuba.python.util.traverse``
(``src/python/python/autodiff.py:6-91,121-194,200-377``, ``util.py:16-179``) for the parameters this backend supports --
diffuse reflectances, constant (``'<bsdf>.reflectance.value'``, ``src/spectra/srgb.cpp:59-61``) or bitmap
(``'<bsdf>.reflectance.data'``, ``src/textures/bitmap.cpp:295-299``).

The reference records the whole render in Enoki's autodiff graph and calls ``ek.backward``.  Here the forward pass is
the ordinary wavefront render into an R,G,B,A,W film, and the backward pass is ``mtsamd_render_adjoint``: every camera
sample is replayed with the same PCG32 stream and its vertices are swept backwards (``k_adjoint`` in
``csrc/kernels.hip``); outside diffuse scenes bitmap texels of diffuse / (rough)plastic reflectances go through
``mtsamd_render_adjoint_textures`` (``k_adjoint_tex``, the same sweep over the general path step), and the texels of bitmaps bound to
``alpha`` / ``alpha_u`` / ``alpha_v`` / ``specular_reflectance`` / ``specular_transmittance`` (``'<bsdf>.alpha.data'``, ...) through
``mtsamd_render_adjoint_param_textures`` (``k_adjoint_param_tex``: that sweep with a central difference of the model code, one replay per
parameter slot).  ``render(..., backward="fused")`` replaces these per-family replays of RGB scenes by ONE, ``mtsamd_render_reverse``
(``k_reverse``, the transpose of ``render_forward``), which also differentiates emitter colours in any scene.  PyTorch only provides the autograd plumbing (as ``render_torch`` does in the reference,
``autodiff.py:380-482``).
"""
import ctypes as C
import math
import weakref
from contextlib import contextmanager

import numpy as np
import torch

from . import bsdfs as B

from . import _lib as L
from .render import PathIntegrator, _ptr, _stream

_DERIV_SEED_OFFSET = 0x9E3779B97F4A7C15      # decorrelates the derivative pass from the primal pass (unbiased=True)


def _is_spectral(scene):
    return getattr(scene, "_variant", getattr(scene, "variant", "rgb")) == "spectral"


def _texture_parameters(records):
    """The bitmap texels mtsamd_render_adjoint_textures differentiates outside diffuse scenes: diffuse.reflectance and
    (rough)plastic.diffuse_reflectance of the top-level BSDF records, plain or inside `twosided` (whose nested BSDF is "brdf_0",
    twosided.cpp:183-186).  Returns (key, record index, texels) triples; children of blendbsdf / mask and procedural textures have none."""
    names = {B.DIFFUSE: "reflectance", B.PLASTIC: "diffuse_reflectance", B.ROUGHPLASTIC: "diffuse_reflectance"}
    out = []
    for i, b in enumerate(records):
        refl = b["reflectance"]
        if b["type"] not in names or not isinstance(refl, dict) or refl.get("type") != "bitmap":
            continue
        name = b.get("id", "bsdf_%d" % i) + (".brdf_0" if b.get("twosided") else "")
        out.append(("%s.%s.data" % (name, names[b["type"]]), i, refl["data"]))
    return out


def _parameter_texture_parameters(scene):
    """The bitmap texels mtsamd_render_adjoint_param_textures differentiates: bitmaps bound to alpha / alpha_u / alpha_v of the rough
    models and to specular_reflectance / specular_transmittance of the conductors and dielectrics, on top-level plain records (inside
    `twosided`: "brdf_0").  Returns (key, texture index, slots, texels): slots are the mtsamd_bsdf_param values whose replays add up to the
    gradient of the texture.  A texture that serves more than one binding gets no key -- its texels would have to collect the replays of
    every slot that reads it; the `alpha` pair is the exception ('<id>.alpha.data': alpha_u and alpha_v of ONE record sharing a texture,
    the sum of the two replays).  Checkerboards have no texels; a scene with a blendbsdf / mask record has no such keys (the entry
    point refuses it)."""
    records = scene._bsdf_records
    if any(b["type"] in (B.BLEND, B.MASK) for b in records):
        return []
    users = {}
    for (i, pname), t in getattr(scene, "_param_texture", {}).items():
        users.setdefault(t, []).append((i, pname))
    out = []
    for t, used in sorted(users.items()):
        i = used[0][0]
        names = sorted(p for _, p in used)
        if i >= len(records) or any(j != i for j, _ in used):
            continue
        spec = records[i]["textures"][names[0]]
        if spec.get("type") != "bitmap":
            continue
        if names == ["alpha_u", "alpha_v"]:
            pname, slots = "alpha", (B.TEXTURE_PARAMS["alpha_u"], B.TEXTURE_PARAMS["alpha_v"])
        elif len(names) == 1:
            pname, slots = names[0], (B.TEXTURE_PARAMS[names[0]],)
        else:
            continue
        name = records[i].get("id", "bsdf_%d" % i) + (".brdf_0" if records[i].get("twosided") else "")
        out.append(("%s.%s.data" % (name, pname), t, slots, spec["data"]))
    return out


class ParameterMap:
    """Dictionary-like view of the differentiable scene parameters (util.py:16-130): torch tensors on the scene's GPU.
    Writes take effect in the scene after :meth:`update` (``parameters_changed``)."""

    def __init__(self, scene, replay=False, geometry=False, normals=None, emitters=False, accel="refit"):
        self._scene = scene
        if accel not in ("refit", "rebuild", "rebuild-sah"):
            raise RuntimeError("accel: \"refit\", \"rebuild\" or \"rebuild-sah\", not %r" % (accel,))
        self._accel = accel                          # what update() does to the accelerator when it moves a mesh
        want_emitters = bool(emitters) and not _is_spectral(scene)      # RGB scenes: the emitter-colour keys below, in any scene
        if normals not in (None, "recompute"):
            raise RuntimeError("normals: None or \"recompute\", not %r" % (normals,))
        self._normals = normals                      # how update() gets the vertex normals of a moved mesh that has them
        # spectral variant only: differentiate the reflectance family (constant srgb colours and bitmap texels of diffuse.reflectance /
        # (rough)plastic.diffuse_reflectance) by the spectral path replay, mtsamd_render_adjoint_spectral, instead of central differences,
        # and the emitter family (envmap texels; radiance / intensity / irradiance of every other emitter) by
        # mtsamd_render_adjoint_spectral_emitters
        self._replay = bool(replay) and _is_spectral(scene)
        if self._replay and getattr(scene, "_n_spectra", 0):      # what mtsamd_render_adjoint_spectral* would answer at the first backward pass
            raise RuntimeError("the spectral adjoint does not replay scenes with tabulated spectra (%u bound here): node values are not "
                               "differentiated" % scene._n_spectra)
        self.rebuild_envmap_distribution = True      # what parameters_changed() does (envmap.cpp:220-253); False: tests of linearity
        self.fd_step = 0.0                           # BSDF-model parameters: step of the central difference of the model code (0: 1 % of the value)
        self.properties = {}
        self._kind = {}
        dev = torch.device("cuda", scene._device_index)
        emitters = scene._dict.get("emitters", [])
        from . import emitters as E
        # 'my_envmap.data' (envmap.cpp:214-218): differentiable in any scene (any BSDF).  Layout: (H, W, 3) linear RGB here; the
        # reference's traverse() exposes the flat H * W * 4 buffer of its bitmap (RGB + a padding channel that carries no parameter,
        # envmap.cpp:216): a script written like invert_bunny.py reshapes with .reshape(H, W, 4)[..., :3] ("parity unpinned": no
        # reference test fixes the layout)
        for e, em in enumerate(emitters):
            if em.get("type", "area") == "envmap":
                key = em.get("id", "emitter_%d" % e) + ".data"
                self.properties[key] = torch.as_tensor(np.ascontiguousarray(em["data"], np.float32), dtype=torch.float32, device=dev).clone()
                self._kind[key] = ("envmap", e, e)
        # reflectances and area-light radiances are differentiated by the diffuse path replay (mtsamd_render_adjoint): scenes of
        # diffuse BSDFs (plain or inside `twosided`) lit by area lights only
        diffuse_scene = all(b["type"] == 0 for b in scene._bsdf_records) and \
            all(em.get("type", "area") == "area" for em in emitters)
        self._diffuse_scene = diffuse_scene
        for i, b in enumerate(scene._bsdf_records if diffuse_scene else []):
            if b["type"] != 0:            # only diffuse reflectances are exposed (the adjoint pass covers those)
                continue
            name = b.get("id", "bsdf_%d" % i)
            if b["twosided"]:             # TwoSidedBRDF::traverse exposes its nested BSDF as "brdf_0" (twosided.cpp:183-186)
                name += ".brdf_0"
            refl = b["reflectance"]
            if isinstance(refl, dict) and refl.get("type") != "bitmap":
                continue                  # procedural textures have no differentiable texels
            if _is_spectral(scene) and (isinstance(refl, dict) or b.get("uniform_mask", 0) & 1 or 0 in b.get("spectra", {})):
                continue                  # spectral variant: constants that are srgb colours only (_spectral_gradient), no tabulated spectra
            if isinstance(refl, dict):
                key = name + ".reflectance.data"
                self.properties[key] = torch.as_tensor(refl["data"], dtype=torch.float32, device=dev).clone()
                self._kind[key] = ("texture", scene.texture_index(i), i)
            else:
                key = name + ".reflectance.value"
                self.properties[key] = torch.as_tensor([float(x) for x in refl], dtype=torch.float32, device=dev)
                self._kind[key] = ("bsdf", i, i)
        # parameters of the BSDF models beyond `diffuse` (what their traverse() exposes, e.g. roughconductor.cpp:393-404, plastic.cpp:299-307):
        # differentiated by mtsamd_render_adjoint_param in ANY scene (any emitter, any depth): constants only.  Spectral variant: the same
        # keys, differentiated by central differences of whole renders (_spectral_gradient); `uniform` spectra are not exposed
        for i, b in enumerate(scene._bsdf_records if not diffuse_scene else []):
            name = b.get("id", "bsdf_%d" % i) + (".brdf_0" if b.get("twosided") and b["type"] != B.DIFFUSE else "")
            flat_index = i                # top-level records keep their place in the table (bsdfs.flatten)
            for pname, kind, types in (("reflectance", 0, (B.DIFFUSE,)), ("diffuse_reflectance", 0, (B.PLASTIC, B.ROUGHPLASTIC)),
                                       ("specular_reflectance", 1, (B.CONDUCTOR, B.ROUGHCONDUCTOR, B.PLASTIC, B.ROUGHPLASTIC, B.DIELECTRIC, B.ROUGHDIELECTRIC, B.THINDIELECTRIC)),
                                       ("specular_transmittance", 5, (B.DIELECTRIC, B.ROUGHDIELECTRIC, B.THINDIELECTRIC)),
                                       ("eta", 2, (B.CONDUCTOR, B.ROUGHCONDUCTOR)), ("k", 3, (B.CONDUCTOR, B.ROUGHCONDUCTOR))):
                if b["type"] not in types:
                    continue
                src = b["reflectance"] if kind == 0 else b[pname]
                if isinstance(src, dict) or pname in b.get("textures", {}):
                    continue              # textured: no constant parameter (the setter refuses it; its texels have a '.data' key)
                if _is_spectral(scene) and (kind in (2, 3) or (b.get("uniform_mask", 0) >> {0: 0, 1: 1, 5: 2}[kind]) & 1 or kind in b.get("spectra", {})):
                    continue              # spectral variant: eta / k, `uniform` and tabulated spectra are not srgb colours
                key = "%s.%s.value" % (name, pname)
                self.properties[key] = torch.as_tensor([float(x) for x in src], dtype=torch.float32, device=dev)
                self._kind[key] = ("bsdf_param", flat_index, kind)
            if b["type"] in (B.ROUGHCONDUCTOR, B.ROUGHDIELECTRIC) and b["alpha_u"] == b["alpha_v"] and \
                    not {"alpha_u", "alpha_v"} & set(b.get("textures", {})):
                key = name + ".alpha.value"
                self.properties[key] = torch.as_tensor([float(b["alpha_u"])], dtype=torch.float32, device=dev)
                self._kind[key] = ("bsdf_param", flat_index, 4)
        # bitmap texels of diffuse reflectances in every other RGB scene: the general path replay (mtsamd_render_adjoint_textures)
        for key, i, data in (_texture_parameters(scene._bsdf_records) if not diffuse_scene and not _is_spectral(scene) else []):
            self.properties[key] = torch.as_tensor(np.ascontiguousarray(data, np.float32), dtype=torch.float32, device=dev).clone()
            self._kind[key] = ("texture", scene.texture_index(i), i)
        # bitmaps bound to alpha / specular colours (RGB scenes): one replay per slot, mtsamd_render_adjoint_param_textures
        for key, t, slots, data in (_parameter_texture_parameters(scene) if not _is_spectral(scene) else []):
            self.properties[key] = torch.as_tensor(np.ascontiguousarray(data, np.float32), dtype=torch.float32, device=dev).clone()
            self._kind[key] = ("param_texture", t, slots)
        # blendbsdf / mask records of RGB scenes, under the names of the reference's traverse() (blendbsdf.cpp:165-169, mask.cpp:167-170):
        # '<id>.weight.value|data' / '<id>.opacity.value|data' and the children's parameters under '<id>.bsdf_0.' / '.bsdf_1.' /
        # '.nested_bsdf.'.  Settable through the setters above; differentiable by render(backward="fused", nested=True) and render_forward(nested=True) only
        self._nested_scene = not _is_spectral(scene) and any(b["type"] in (B.BLEND, B.MASK) for b in scene._bsdf_records)
        for i, b in enumerate(scene._bsdf_records if self._nested_scene else []):
            if b["type"] not in (B.BLEND, B.MASK):
                continue
            name = b.get("id", "bsdf_%d" % i)
            wname = "weight" if b["type"] == B.BLEND else "opacity"
            w = b["reflectance"]
            if isinstance(w, dict):
                if w.get("type") == "bitmap":         # (a checkerboard weight renders but has no texels)
                    key = "%s.%s.data" % (name, wname)
                    self.properties[key] = torch.as_tensor(np.ascontiguousarray(w["data"], np.float32), dtype=torch.float32, device=dev).clone()
                    self._kind[key] = ("texture", scene.texture_index(i), i)
            else:
                key = "%s.%s.value" % (name, wname)
                self.properties[key] = torch.as_tensor([float(w[0])], dtype=torch.float32, device=dev)
                self._kind[key] = ("nest_weight", i, 0)
            for c, child in enumerate(b["children"]):
                self._add_child_keys(scene, child, name + (".bsdf_%d" % c if b["type"] == B.BLEND else ".nested_bsdf"), b["nested"][c], dev)
        # spectral variant with `replay`: the same texel keys, in diffuse and general scenes alike (mtsamd_render_adjoint_spectral)
        for key, i, data in (_texture_parameters(scene._bsdf_records) if self._replay else []):
            self.properties[key] = torch.as_tensor(np.ascontiguousarray(data, np.float32), dtype=torch.float32, device=dev).clone()
            self._kind[key] = ("texture", scene.texture_index(i), i)
        # 'shape.emitter.radiance.value' of area lights (docs/src/inverse_rendering/diff_render.rst:76)
        for i, m in enumerate(scene._dict["meshes"] if diffuse_scene else []):
            e = m.get("emitter", -1)
            if e is None or e < 0 or scene._dict["emitters"][e].get("type", "area") != "area":
                continue
            if _is_spectral(scene) and E.normalize(scene._dict["emitters"][e]).get("spectrum") is not None:
                continue                  # the radiance holds a tabulated spectrum: not an srgb_d65 colour, no key
            key = m.get("id", "shape_%d" % i) + ".emitter.radiance.value"
            rad = np.broadcast_to(np.asarray(E.normalize(scene._dict["emitters"][e])["radiance"], np.float32), (3,))      # (RGB variant: a spectrum plugin's pre-integrated colour)
            self.properties[key] = torch.as_tensor(rad.copy(), dtype=torch.float32, device=dev)
            self._kind[key] = ("emitter", e, i)
        # spectral variant with `replay`: the emitted colour of the emitters that have no shape -- `constant`, `point`, `spot`, `directional` --
        # under their own id ('<emitter>.radiance.value', '.intensity.value', '.irradiance.value').  Area lights keep the keys above
        for e, em in enumerate(emitters if self._replay else []):
            t = em.get("type", "area")
            if t in ("envmap", "area"):
                continue
            if E.normalize(em).get("spectrum") is not None:
                continue                  # (a scene with spectra refuses the replay above; kept for the day it does not)
            key = "%s.%s.value" % (em.get("id", "emitter_%d" % e), E._VALUE_KEY[t])
            self.properties[key] = torch.as_tensor(E.normalize(em)["radiance"], dtype=torch.float32, device=dev)
            self._kind[key] = ("emitter", e, e)

        # RGB variant with `emitters`: the same emitter-colour keys in ANY scene -- area lights under their shape, `constant`, `point`, `spot`
        # and `directional` under their own id.  Settable, and usable as tangents of render_forward (radiance is linear in them); the
        # default reverse pass covers them in diffuse area-lit scenes only (the keys above), so render() raises on one that requires a gradient
        # unless backward="fused"
        for i, m in enumerate(scene._dict["meshes"] if want_emitters and not diffuse_scene else []):
            e = m.get("emitter", -1)
            if e is None or e < 0 or scene._dict["emitters"][e].get("type", "area") != "area":
                continue
            key = m.get("id", "shape_%d" % i) + ".emitter.radiance.value"
            rad = np.broadcast_to(np.asarray(E.normalize(scene._dict["emitters"][e])["radiance"], np.float32), (3,))
            self.properties[key] = torch.as_tensor(rad.copy(), dtype=torch.float32, device=dev)
            self._kind[key] = ("emitter", e, i)
        for e, em in enumerate(emitters if want_emitters else []):
            t = em.get("type", "area")
            if t in ("envmap", "area"):
                continue
            key = "%s.%s.value" % (em.get("id", "emitter_%d" % e), E._VALUE_KEY[t])
            rad = np.broadcast_to(np.asarray(E.normalize(em)["radiance"], np.float32), (3,))
            self.properties[key] = torch.as_tensor(rad.copy(), dtype=torch.float32, device=dev)
            self._kind[key] = ("emitter", e, e)

        # '<shape id>.vertex_positions_buf' of every mesh (mesh.cpp:781-804): the flat 3N buffer.  Settable, not differentiable: there is
        # no reparameterised integrator behind it (render() refuses a tensor that requires a gradient)
        for i, m in enumerate(scene._dict["meshes"] if geometry else []):
            key = m.get("id", "shape_%d" % i) + ".vertex_positions_buf"
            self.properties[key] = torch.as_tensor(np.ascontiguousarray(m["positions"], np.float32).reshape(-1), dtype=torch.float32, device=dev).clone()
            self._kind[key] = ("vertices", i, m.get("normals") is not None)
            # the scene was created from these positions: update() pushes the buffer only once it holds something else
            self.__dict__.setdefault("_pushed", {})[key] = (self.properties[key], self.properties[key]._version)

    def _add_child_keys(self, scene, b, prefix, flat_index, dev):
        """The keys of a plain record that is a child of a blendbsdf / mask (record `flat_index` of the flattened table): what the loops
        over the top-level records of a general scene add, under `prefix`."""
        name = prefix + (".brdf_0" if b.get("twosided") and b["type"] != B.DIFFUSE else "")
        for pname, kind, types in (("reflectance", 0, (B.DIFFUSE,)), ("diffuse_reflectance", 0, (B.PLASTIC, B.ROUGHPLASTIC)),
                                   ("specular_reflectance", 1, (B.CONDUCTOR, B.ROUGHCONDUCTOR, B.PLASTIC, B.ROUGHPLASTIC, B.DIELECTRIC, B.ROUGHDIELECTRIC, B.THINDIELECTRIC)),
                                   ("specular_transmittance", 5, (B.DIELECTRIC, B.ROUGHDIELECTRIC, B.THINDIELECTRIC)),
                                   ("eta", 2, (B.CONDUCTOR, B.ROUGHCONDUCTOR)), ("k", 3, (B.CONDUCTOR, B.ROUGHCONDUCTOR))):
            if b["type"] not in types:
                continue
            src = b["reflectance"] if kind == 0 else b[pname]
            if pname in b.get("textures", {}):
                continue
            if isinstance(src, dict):
                if kind == 0 and src.get("type") == "bitmap":
                    key = "%s.%s.data" % (prefix + (".brdf_0" if b.get("twosided") else ""), pname)
                    self.properties[key] = torch.as_tensor(np.ascontiguousarray(src["data"], np.float32), dtype=torch.float32, device=dev).clone()
                    self._kind[key] = ("texture", scene.texture_index(flat_index), flat_index)
                continue
            key = "%s.%s.value" % (name, pname)
            self.properties[key] = torch.as_tensor([float(x) for x in src], dtype=torch.float32, device=dev)
            self._kind[key] = ("bsdf_param", flat_index, kind)
        if b["type"] in (B.ROUGHCONDUCTOR, B.ROUGHDIELECTRIC) and b["alpha_u"] == b["alpha_v"] and not {"alpha_u", "alpha_v"} & set(b.get("textures", {})):
            key = name + ".alpha.value"
            self.properties[key] = torch.as_tensor([float(b["alpha_u"])], dtype=torch.float32, device=dev)
            self._kind[key] = ("bsdf_param", flat_index, 4)

    def __getitem__(self, k): return self.properties[k]
    def __contains__(self, k): return k in self.properties
    def __len__(self): return len(self.properties)
    def keys(self): return self.properties.keys()
    def items(self): return self.properties.items()

    def __setitem__(self, k, value):
        if k not in self.properties:
            raise KeyError(k)
        old = self.properties[k]
        new = torch.as_tensor(value, dtype=torch.float32, device=old.device).reshape(old.shape).clone()
        new.requires_grad_(old.requires_grad)
        self.properties[k] = new

    def keep(self, keys):
        """util.py:120-129"""
        keys = set(keys)
        self.properties = {k: v for k, v in self.properties.items() if k in keys}

    def all_differentiable(self):
        return True

    def update(self):
        """util.py:103-118: push the current values into the scene (parameters_changed).  A value the scene has already seen -- the same
        tensor at the same version -- is not pushed again: render() calls this before every primal pass, and reading a constant back
        to the host costs a device synchronisation."""
        seen = self.__dict__.setdefault("_pushed", {})
        for k, v in self.properties.items():
            last = seen.get(k)
            if last is not None and last[0] is v and last[1] == v._version:      # (the tensor itself is kept: an id can be reused)
                continue
            kind, idx, _ = self._kind[k]
            if _is_spectral(self._scene) and (kind in ("bsdf", "texture") or (kind == "bsdf_param" and self._kind[k][2] != 4)):
                # spectral variant: an srgb colour lives in [0, 1]^3 (srgb.cpp:34-35); an optimiser step that leaves the box is projected
                # back onto it (the parameter tensor itself, so that the optimiser's state and the scene agree)
                with torch.no_grad():
                    v.clamp_(0.0, 1.0)
            if _is_spectral(self._scene) and kind == "envmap":
                # spectral variant: a texel is upsampled as a scale times a colour in [0, 1]^3 (envmap.cpp:96-109), so it is projected onto
                # >= 0, on the parameter tensor itself as above
                with torch.no_grad():
                    v.clamp_(min=0.0)
            seen[k] = (v, v._version)
            if kind == "vertices":
                self._scene.update_vertices(idx, v, normals=self._normals if self._kind[k][2] else None, accel=self._accel)
            elif kind in ("texture", "param_texture"):
                self._scene.update_texture(idx, v)
            elif kind == "emitter":
                self._scene.set_emitter_radiance(idx, v.detach().cpu().tolist())
            elif kind == "envmap":
                self._scene.update_envmap(v, rebuild_distribution=self.rebuild_envmap_distribution)
            elif kind == "bsdf_param":
                vals = [float(x) for x in v.detach().cpu().reshape(-1).tolist()]
                self._scene.set_bsdf_param(idx, self._kind[k][2], vals)
            elif kind == "nest_weight":      # the record keeps its weight / opacity in the reflectance field, all three components
                self._scene.set_bsdf_reflectance(idx, [float(v.detach().cpu().reshape(-1)[0])] * 3)
            else:
                self._scene.set_bsdf_reflectance(idx, v.detach().cpu().tolist())


def traverse(scene, replay=False, geometry=False, normals=None, emitters=False, accel="refit"):
    """mitsuba.python.util.traverse (util.py:132-179) for the supported parameters.  ``replay=True`` (spectral scenes; ignored for RGB
    ones) adds the bitmap texels of the reflectance family and the emitted colour of shapeless emitters, and differentiates the reflectance
    family and the emitter family (envmap texels included) with one spectral path replay each per backward pass.  ``geometry=True`` adds
    '<shape id>.vertex_positions_buf' of every mesh (the flat 3N buffer of mesh.cpp:781-804); update() pushes it through
    Scene.update_vertices; ``normals="recompute"`` makes it pass that on for every mesh with vertex normals, so that a moved mesh's
    normals are recomputed on the device and no vertex data visits the host; ``accel="rebuild"`` makes every such update rebuild the
    accelerator's topology instead of only refitting it, ``accel="rebuild-sah"`` with the SAH builder (Scene.update_vertices).  These keys are settable, not differentiable -- an optimiser marks every key of its map as requiring a gradient,
    which is why they have to be asked for: render() raises on one that requires a gradient.  ``emitters=True`` (RGB scenes; ignored for
    spectral ones) adds the emitter colours in any scene: '<shape id>.emitter.radiance.value' of area lights and
    '<emitter id>.radiance|intensity|irradiance.value' of `constant`, `point`, `spot` and `directional` emitters.  They are settable and
    serve as tangents of render_forward; outside diffuse area-lit scenes render() raises on one that requires a gradient unless it is
    called with backward="fused"."""
    return ParameterMap(scene, replay=replay, geometry=geometry, normals=normals, emitters=emitters, accel=accel)


def _replayed(pmap, key):
    """Which spectral path replay differentiates this key?  "reflectance": texels and the constant (diffuse_)reflectance colours
    (mtsamd_render_adjoint_spectral); "emitter": envmap texels and emitter radiances (mtsamd_render_adjoint_spectral_emitters); None:
    central differences."""
    kind, _, extra = pmap._kind[key]
    if not pmap._replay:
        return None
    if kind in ("texture", "bsdf") or (kind == "bsdf_param" and extra == 0):
        return "reflectance"
    return "emitter" if kind in ("envmap", "emitter") else None


def _texture_slice(scene, g_tex, idx):
    off, w, h = C.c_uint64(), C.c_int32(), C.c_int32()
    L.check(L.lib().mtsamd_scene_texture_info(scene._handle, idx, C.byref(w), C.byref(h), C.byref(off)))
    return g_tex[off.value: off.value + 3 * w.value * h.value].reshape(h.value, w.value, 3).clone()


def _desc(scene, sensor, integrator, spp, seed):
    d = integrator._desc(sensor)
    if spp is not None:
        d.sample_count = int(spp)
    d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    d.film_rgb = 1
    d.rfilter_analytic = 1          # CUDA variants evaluate the filter analytically (imageblock.cpp:131-132)
    return d


def _render_film(scene, d):
    dev = torch.device("cuda", scene._device_index)
    film = torch.zeros((d.crop_height, d.crop_width, 5), dtype=torch.float32, device=dev)
    L.check(L.lib().mtsamd_render(scene._handle, C.byref(d), _ptr(film), None, _stream()))
    return film


def _image_of(film):
    """autodiff.py:80-91: values / (weight + 1e-8), flattened RGB."""
    return (film[..., :3] / (film[..., 4:5] + 1e-8)).reshape(-1)


def _spectral_gradient(scene, d, pmap, key, gi):
    """Spectral variant: d(loss)/d(parameter) of a constant colour, radiance or roughness by central differences of the rendered
    image at fixed random numbers (the derivative pass's seed): two renders per scalar component.  The reference differentiates its
    spectral variants with Enoki's autodiff like the others; this backend has no spectral path replay, so the
    spectral ParameterMap is limited to a handful of constants -- texels and envmaps raise."""
    kind, idx, extra = pmap._kind[key]
    if kind in ("texture", "envmap"):
        raise RuntimeError("the spectral variant differentiates constant colours, radiances and roughnesses only (%s is a %s; texels and envmaps need traverse(scene, replay=True))" % (key, kind))
    value = [float(x) for x in pmap[key].detach().cpu().reshape(-1).tolist()]

    def push(vals):
        if kind == "emitter":
            scene.set_emitter_radiance(idx, vals)
        elif kind == "bsdf_param":
            scene.set_bsdf_param(idx, extra, vals)
        else:
            scene.set_bsdf_reflectance(idx, vals)

    grad = torch.zeros(len(value), dtype=torch.float32, device=gi.device)
    colour = kind != "emitter" and not (kind == "bsdf_param" and extra == 4)
    try:
        for c in range(len(value)):
            h = float(pmap.fd_step) if pmap.fd_step > 0 else 0.01 * max(abs(value[c]), 0.05)
            hi, lo = value[c] + h, value[c] - h
            if colour:
                hi, lo = min(hi, 1.0), max(lo, 0.0)                       # srgb colours live in [0, 1] (srgb.cpp:34-35)
            elif kind == "bsdf_param":
                lo = max(lo, 1e-4)                                        # roughness
            images = []
            for x in (hi, lo):
                push(value[:c] + [x] + value[c + 1:])
                images.append(_image_of(_render_film(scene, d)))
            grad[c] = torch.dot(gi, images[0] - images[1]) / (hi - lo)
    finally:
        push(value)               # an exception on the way leaves the scene at the parameter's value
    return grad.reshape(pmap[key].shape)


class _Render(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scene, d, pmap, keys, *values):
        pmap.update()                 # parameters_changed(): the scene sees the current values
        film = _render_film(scene, d)
        ctx.scene, ctx.d, ctx.pmap, ctx.keys = scene, d, pmap, keys
        ctx.save_for_backward(film)
        return _image_of(film)

    @staticmethod
    def backward(ctx, grad_image):
        (film,) = ctx.saved_tensors
        scene, d, pmap, keys = ctx.scene, ctx.d, ctx.pmap, ctx.keys
        dev = film.device
        n_bsdf = len(scene._dict["bsdfs"])
        tex_floats = sum(h * w * 3 for (h, w, _) in scene._texture_shapes)
        g_bsdf = torch.zeros((n_bsdf, 3), dtype=torch.float32, device=dev)
        g_tex = torch.zeros(max(tex_floats, 1), dtype=torch.float32, device=dev)
        g_em = torch.zeros((max(len(scene._dict.get("emitters", [])), 1), 3), dtype=torch.float32, device=dev)
        gi = grad_image.to(dev, torch.float32).contiguous()
        if _is_spectral(scene):
            grads = {}
            replayed = {pmap._kind[k][0] for k in keys if _replayed(pmap, k) == "reflectance"}
            if replayed:      # one replay for the whole reflectance family; a gradient nobody asked for is not computed (null)
                L.check(L.lib().mtsamd_render_adjoint_spectral(scene._handle, C.byref(d), _ptr(gi), _ptr(film), _ptr(g_bsdf) if replayed - {"texture"} else None,
                                                               _ptr(g_tex) if "texture" in replayed else None, _stream()))
            emitted = {pmap._kind[k][0] for k in keys if _replayed(pmap, k) == "emitter"}
            g_env = None
            if emitted:       # and one for the whole emitter family
                if "envmap" in emitted:
                    g_env = torch.zeros_like(next(pmap[k] for k in keys if pmap._kind[k][0] == "envmap"))
                L.check(L.lib().mtsamd_render_adjoint_spectral_emitters(scene._handle, C.byref(d), _ptr(gi), _ptr(film), _ptr(g_em) if "emitter" in emitted else None,
                                                                        _ptr(g_env) if g_env is not None else None, _stream()))
            for k in keys:
                kind, idx, _ = pmap._kind[k]
                if not _replayed(pmap, k):
                    grads[k] = _spectral_gradient(scene, d, pmap, k, gi.reshape(-1))
                elif kind == "envmap":
                    grads[k] = g_env
                elif kind == "emitter":
                    grads[k] = g_em[idx].clone().reshape(pmap[k].shape)
                elif kind == "texture":
                    grads[k] = _texture_slice(scene, g_tex, idx)
                else:
                    grads[k] = g_bsdf[idx].clone().reshape(pmap[k].shape)
            return (None, None, None, None) + tuple(grads[k] for k in keys)
        kinds = {pmap._kind[k][0] for k in keys}
        if pmap._diffuse_scene and kinds - {"envmap", "bsdf_param"}:
            L.check(L.lib().mtsamd_render_adjoint(scene._handle, C.byref(d), _ptr(gi), _ptr(film), _ptr(g_bsdf), _ptr(g_tex), _ptr(g_em), _stream()))
        elif "texture" in kinds:          # texels in any other scene: the replay through the general step
            L.check(L.lib().mtsamd_render_adjoint_textures(scene._handle, C.byref(d), _ptr(gi), _ptr(film), _ptr(g_tex), _stream()))
        g_env = None
        if "envmap" in kinds:
            g_env = torch.zeros_like(next(pmap[k] for k in keys if pmap._kind[k][0] == "envmap"))
            L.check(L.lib().mtsamd_render_adjoint_envmap(scene._handle, C.byref(d), _ptr(gi), _ptr(film), _ptr(g_env), _stream()))
        # texels behind alpha / specular colours: one replay per slot the kept keys need, each into a zeroed buffer of its own
        g_slot = {}
        for slot in sorted({s for k in keys if pmap._kind[k][0] == "param_texture" for s in pmap._kind[k][2]}):
            g_slot[slot] = torch.zeros_like(g_tex)
            L.check(L.lib().mtsamd_render_adjoint_param_textures(scene._handle, C.byref(d), _ptr(gi), _ptr(film), int(slot), float(pmap.fd_step),
                                                                 _ptr(g_slot[slot]), _stream()))
        grads = []
        for k in keys:
            kind, idx, _ = pmap._kind[k]
            if kind == "param_texture":
                grads.append(sum(_texture_slice(scene, g_slot[s], idx) for s in pmap._kind[k][2]))
                continue
            if kind == "bsdf_param":          # one replay per scalar component (forward-mode derivative carried beside the path)
                n = pmap[k].numel()
                g = torch.zeros(n, dtype=torch.float32, device=dev)
                for c in range(n):
                    L.check(L.lib().mtsamd_render_adjoint_param(scene._handle, C.byref(d), _ptr(gi), _ptr(film), int(idx), int(pmap._kind[k][2]), c,
                                                                float(pmap.fd_step), _ptr(g[c:c + 1]), _stream()))
                grads.append(g.reshape(pmap[k].shape))
                continue
            if kind == "envmap":
                grads.append(g_env)
            elif kind == "bsdf":
                grads.append(g_bsdf[idx].clone())
            elif kind == "emitter":
                grads.append(g_em[idx].clone())
            else:
                grads.append(_texture_slice(scene, g_tex, idx))
        return (None, None, None, None) + tuple(grads)


class _RenderFused(torch.autograd.Function):
    """render(backward="fused"): the primal pass of _Render, and ONE path replay (mtsamd_render_reverse, k_reverse) for every `bsdf`,
    `bsdf_param`, `texture`, `emitter` and `envmap` key of the backward pass -- one estimator with one Russian-roulette convention.
    `param_texture` keys keep their own replays (mtsamd_render_adjoint_param_textures) unless `param_maps` is set: then they come from
    that same call (MTSAMD_REVERSE_PARAM_TEXTURES), beside every other key of a scene with textured BSDF parameters."""

    @staticmethod
    def forward(ctx, scene, d, pmap, keys, flags, *values):
        detach_roulette, ctx.param_maps, ctx.nested = bool(flags & 1), bool(flags & 2), bool(flags & 4)
        pmap.update()
        film = _render_film(scene, d)
        ctx.scene, ctx.d, ctx.pmap, ctx.keys, ctx.detach_roulette = scene, d, pmap, keys, detach_roulette
        ctx.save_for_backward(film)
        return _image_of(film)

    @staticmethod
    def backward(ctx, grad_image):
        (film,) = ctx.saved_tensors
        scene, d, pmap, keys = ctx.scene, ctx.d, ctx.pmap, ctx.keys
        dev = film.device
        gi = grad_image.to(dev, torch.float32).contiguous()
        kinds = {pmap._kind[k][0] for k in keys}
        n_bsdf = max(len(B.flatten(scene._bsdf_records)), 1)
        wanted = np.zeros((n_bsdf, L.BSDF_TANGENT_FLOATS), np.uint8)
        for k in keys:
            kind, idx, extra = pmap._kind[k]
            if kind in ("bsdf", "bsdf_param", "nest_weight"):
                row = int(extra) if kind == "bsdf_param" else 0      # a weight / opacity: entry 18 * record + 0
                wanted[idx, 3 * row: 3 * row + pmap[k].numel()] = 1
        g_bsdf = torch.zeros((n_bsdf, L.BSDF_TANGENT_FLOATS), dtype=torch.float32, device=dev) if wanted.any() else None
        g_em = torch.zeros((max(len(scene._dict.get("emitters", [])), 1), 3), dtype=torch.float32, device=dev) if "emitter" in kinds else None
        tex_floats = sum(h * w * 3 for (h, w, _) in scene._texture_shapes)
        g_tex = torch.zeros(max(tex_floats, 1), dtype=torch.float32, device=dev) if kinds & {"texture", "param_texture"} else None
        g_env = torch.zeros_like(next(pmap[k] for k in keys if pmap._kind[k][0] == "envmap")) if "envmap" in kinds else None
        fused_kinds = kinds if ctx.param_maps else kinds - {"param_texture"}
        if fused_kinds:
            gd = L.GradientDesc()
            if g_bsdf is not None:
                gd.bsdf_wanted = wanted.ctypes.data_as(C.POINTER(C.c_uint8))
                gd.grad_bsdf_dev = _ptr(g_bsdf)
            gd.grad_emitters_dev = _ptr(g_em) if g_em is not None else None
            gd.grad_textures_dev = _ptr(g_tex) if fused_kinds & {"texture", "param_texture"} else None
            gd.grad_envmap_dev = _ptr(g_env) if g_env is not None else None
            gd.h = float(pmap.fd_step)
            gd.flags = (L.REVERSE_DETACH_ROULETTE if ctx.detach_roulette else 0) | \
                       (L.REVERSE_PARAM_TEXTURES if ctx.param_maps and getattr(scene, "_param_texture", None) else 0) | \
                       (L.REVERSE_NESTED if ctx.nested and _has_nested_records(scene) else 0)
            L.check(L.lib().mtsamd_render_reverse(scene._handle, C.byref(d), _ptr(gi), _ptr(film), C.byref(gd), _stream()))
        g_slot = {}
        for slot in sorted({s for k in keys if pmap._kind[k][0] == "param_texture" and not ctx.param_maps for s in pmap._kind[k][2]}):
            g_slot[slot] = torch.zeros_like(g_tex)
            L.check(L.lib().mtsamd_render_adjoint_param_textures(scene._handle, C.byref(d), _ptr(gi), _ptr(film), int(slot), float(pmap.fd_step),
                                                                 _ptr(g_slot[slot]), _stream()))
        grads = []
        for k in keys:
            kind, idx, extra = pmap._kind[k]
            if kind == "param_texture" and not ctx.param_maps:
                grads.append(sum(_texture_slice(scene, g_slot[s], idx) for s in extra))
            elif kind in ("bsdf", "bsdf_param", "nest_weight"):
                row = int(extra) if kind == "bsdf_param" else 0
                grads.append(g_bsdf[idx, 3 * row: 3 * row + pmap[k].numel()].clone().reshape(pmap[k].shape))
            elif kind == "envmap":
                grads.append(g_env)
            elif kind == "emitter":
                grads.append(g_em[idx].clone().reshape(pmap[k].shape))
            else:
                grads.append(_texture_slice(scene, g_tex, idx))
        return (None, None, None, None, None) + tuple(grads)


_render_counter = {}      # id(scene) -> number of render() calls so far
_render_tracked = set()   # ids whose entry is dropped when their scene dies: id() values are reused, and a new scene must start at call 0


def _forget_scene(key):
    _render_counter.pop(key, None)
    _render_tracked.discard(key)


def _next_seed(scene, sensor):
    """The seed of the next call for this scene: the call counter folded into the sampler's seed."""
    if id(scene) not in _render_tracked:
        _render_tracked.add(id(scene))
        weakref.finalize(scene, _forget_scene, id(scene))
    call = _render_counter.get(id(scene), 0)
    _render_counter[id(scene)] = call + 1
    return sensor.sampler().seed_value() + call * 0xD1B54A32D192ED03


def _has_nested_records(scene):
    return not _is_spectral(scene) and any(b["type"] in (B.BLEND, B.MASK) for b in scene._bsdf_records)


def render_forward(scene, params, tangents, spp=None, sensor_index=0, detach_roulette=False, param_maps=False, nested=False):
    """Forward-mode derivative render: the flat ``H*W*3`` image of d(image)/d(t) along the tangent ``tangents`` -- what
    ``ek.gradient(image)`` holds after ``ek.set_gradient(param, t); ek.forward(param)`` in
    ``docs/examples/10_inverse_rendering/forward_diff.py`` (``diff_render.rst:332-398``).  ``tangents`` maps keys of ``params`` to tensors of
    the parameters' shapes; the contributions of all keys add up in ONE replay (``mtsamd_render_forward``): BSDF constants, bitmap texels of
    the reflectance family, emitter colours (``traverse(scene, emitters=True)``) and envmap texels.  Texels of parameter maps
    (``'<bsdf>.alpha.data'``, ...) and vertex positions have no forward derivative here and raise.  ``params.update()`` runs first; the seed
    comes from the call counter exactly as in :func:`render`, so resetting ``_render_counter[id(scene)]`` gives common random numbers with
    it.  ``params.fd_step`` is the step of the central difference behind BSDF constants; ``detach_roulette=True`` holds the
    Russian-roulette factor fixed (the convention of ``mtsamd_render_adjoint_param``); by default it is differentiated as the reference does.
    ``param_maps=True`` (``MTSAMD_FORWARD_PARAM_TEXTURES``) opens scenes with textured BSDF parameters: every key above works there, and the
    texels of parameter maps (``'<bsdf>.alpha.data'``, ...) take tangents too, with the step ``params.fd_step`` of
    ``mtsamd_render_adjoint_param_textures``.  ``nested=True`` (``MTSAMD_FORWARD_NESTED``) opens scenes with blendbsdf / mask records: the
    children's keys, ``'<id>.weight.value'`` / ``'<id>.opacity.value'`` and the texels of a bitmap weight take tangents; the weight's
    derivative includes the derivative of the child-selection probability, so the image is the derivative of the expected image
    (``include/mtsamd.h``).  The keyword is inert in scenes without such records."""
    if _is_spectral(scene):
        raise RuntimeError("render_forward is implemented for the RGB variant only")
    if _has_nested_records(scene) and not nested:
        raise RuntimeError("this scene has blendbsdf / mask materials: render_forward differentiates it with nested=True only")
    sensor = scene.sensors()[sensor_index]
    integrator = scene.integrator() if scene.integrator() is not None else PathIntegrator()
    for k in tangents:
        if k not in params:
            raise KeyError(k)
        kind = params._kind[k][0]
        if kind == "vertices" or (kind == "param_texture" and not param_maps):
            raise RuntimeError("%s has no forward-mode derivative: %s" % (k, "texels of BSDF parameter maps are differentiated by the reverse pass only"
                                                                          if kind == "param_texture" else "there is no reparameterised integrator for vertex positions"))
    if not tangents:
        raise RuntimeError("render_forward needs a tangent on at least one parameter")
    params.update()
    d = _desc(scene, sensor, integrator, spp, _next_seed(scene, sensor))
    dev = torch.device("cuda", scene._device_index)
    n_bsdf = len(B.flatten(scene._bsdf_records))
    n_em = len(scene._dict.get("emitters", []))
    t_bsdf = np.zeros((max(n_bsdf, 1), L.BSDF_TANGENT_FLOATS), np.float32)
    t_em = np.zeros((max(n_em, 1), 3), np.float32)
    t_tex = t_env = None
    used = set()
    for k, t in tangents.items():
        kind, idx, extra = params._kind[k]
        t = torch.as_tensor(t, dtype=torch.float32)
        if t.numel() != params[k].numel():
            raise RuntimeError("the tangent of %s has %d elements, the parameter %d" % (k, t.numel(), params[k].numel()))
        used.add(kind)
        if kind in ("bsdf", "bsdf_param", "nest_weight"):
            row = int(extra) if kind == "bsdf_param" else 0      # a weight / opacity: entry 18 * record + 0
            v = t.detach().cpu().reshape(-1).numpy()
            t_bsdf[idx, 3 * row: 3 * row + len(v)] += v
        elif kind == "emitter":
            t_em[idx] += t.detach().cpu().reshape(3).numpy()
        elif kind == "envmap":
            t_env = t.detach().to(dev).reshape(params[k].shape).contiguous()
        else:       # texture, param_texture: the texture buffer at the bitmap's slice
            if t_tex is None:
                t_tex = torch.zeros(max(sum(h * w * 3 for (h, w, _) in scene._texture_shapes), 1), dtype=torch.float32, device=dev)
            off, w, h = C.c_uint64(), C.c_int32(), C.c_int32()
            L.check(L.lib().mtsamd_scene_texture_info(scene._handle, idx, C.byref(w), C.byref(h), C.byref(off)))
            t_tex[off.value: off.value + 3 * w.value * h.value] = t.detach().to(dev).reshape(-1)
    td = L.TangentDesc()
    if used & {"bsdf", "bsdf_param", "nest_weight"}:
        td.bsdf_tangents = t_bsdf.ctypes.data_as(L.f32p)
    if "emitter" in used:
        td.emitter_tangents = t_em.ctypes.data_as(L.f32p)
    td.texture_tangents_dev = _ptr(t_tex) if t_tex is not None else None
    td.envmap_tangent_dev = _ptr(t_env) if t_env is not None else None
    td.h = float(params.fd_step)
    # the C interface knows the bit in scenes with textured BSDF parameters only; in any other scene param_maps changes nothing
    td.flags = (L.FORWARD_DETACH_ROULETTE if detach_roulette else 0) | (L.FORWARD_PARAM_TEXTURES if param_maps and getattr(scene, "_param_texture", None) else 0) | \
               (L.FORWARD_NESTED if nested and _has_nested_records(scene) else 0)      # likewise: the bit exists in scenes with blend / mask records only
    film = torch.zeros((d.crop_height, d.crop_width, 5), dtype=torch.float32, device=dev)
    L.check(L.lib().mtsamd_render_forward(scene._handle, C.byref(d), C.byref(td), _ptr(film), _stream()))
    return _image_of(film)


def render(scene, spp=None, unbiased=False, optimizer=None, sensor_index=0, params=None, backward="families", detach_roulette=False,
           param_maps=False, nested=False):
    """mitsuba.python.autodiff.render (autodiff.py:121-194): differentiable render returning the flattened RGB image
    (``len == H*W*3``).  ``params`` (or ``optimizer.params``) is the :class:`ParameterMap` whose tensors with
    ``requires_grad`` receive gradients; without one the call is a plain render.  Every call draws new random numbers
    (the reference's sampler keeps advancing its streams between calls; here the call counter is folded into the seed).

    ``backward`` picks the backward pass.  ``"families"`` (the default) is one entry point per parameter family: one replay per scalar of
    a BSDF-model parameter, one for texels, one for the envmap; emitter colours only in diffuse area-lit scenes.  ``"fused"`` (RGB
    scenes) serves every ``bsdf``, ``bsdf_param``, ``texture``, ``emitter`` and ``envmap`` key with ONE replay, ``mtsamd_render_reverse``,
    the transpose of :func:`render_forward`: emitter keys of ``traverse(scene, emitters=True)`` are then differentiable in any scene, and
    the whole gradient is that of one estimator -- Russian roulette differentiated as the reference does, or held fixed with
    ``detach_roulette=True`` (the convention of ``mtsamd_render_adjoint_param``).  Texels of parameter maps keep their own replays, and
    no other key of a scene with such maps is differentiable, unless ``param_maps=True`` (``MTSAMD_REVERSE_PARAM_TEXTURES``): then that one
    ``mtsamd_render_reverse`` call serves the maps' texels and every other key of the scene alike, mixed key sets such as (``eta``,
    ``alpha.data``, a lamp colour) included.  ``backward="families"`` ignores ``param_maps``.  A scene with blendbsdf / mask materials is
    differentiable with ``backward="fused", nested=True`` only (``MTSAMD_REVERSE_NESTED``): the weight / opacity, the children's
    parameters, the texels of a bitmap weight and every other key of the scene come from that one call; without the keyword a key of such
    a scene that requires a gradient raises.  ``nested`` is inert in scenes without such materials.
    """
    if backward not in ("families", "fused"):
        raise RuntimeError("backward: \"families\" or \"fused\", not %r" % (backward,))
    if backward == "fused" and _is_spectral(scene):
        raise RuntimeError("backward=\"fused\" is implemented for the RGB variant only")
    sensor = scene.sensors()[sensor_index]
    integrator = scene.integrator() if scene.integrator() is not None else PathIntegrator()
    if optimizer is not None and params is None:
        params = optimizer.params
    if params is not None and not _is_spectral(scene) and not params._diffuse_scene and backward != "fused":
        for k, v in params.items():
            if v.requires_grad and params._kind[k][0] == "emitter":
                raise RuntimeError("%s has a reverse-mode gradient in diffuse scenes lit by area lights only; its derivative image in this "
                                   "scene comes from render_forward (clear requires_grad on it)" % k)
    if unbiased:
        if optimizer is None and params is None:
            raise Exception("render(): unbiased=True requires that an optimizer is specified!")
        if not isinstance(spp, tuple):
            spp = (spp, spp)
    elif isinstance(spp, tuple):
        raise Exception("render(): unbiased=False requires that spp is either an integer or None!")
    base = _next_seed(scene, sensor)

    def differentiable(spp_, seed):
        d = _desc(scene, sensor, integrator, spp_, seed)
        keys = [k for k, v in params.items() if v.requires_grad] if params is not None else []
        for k in keys:
            if params._kind[k][0] == "vertices":
                raise RuntimeError("%s is settable, not differentiable: there is no reparameterised integrator for vertex positions; "
                                   "clear requires_grad on it" % k)
        if not keys:
            if params is not None:
                params.update()
            return _image_of(_render_film(scene, d))
        if _has_nested_records(scene) and not (backward == "fused" and nested):
            raise RuntimeError("%s requires a gradient in a scene with blendbsdf / mask materials: such a scene is differentiated by "
                               "render(..., backward=\"fused\", nested=True) only" % keys[0])
        if backward == "fused":
            return _RenderFused.apply(scene, d, params, keys, (1 if detach_roulette else 0) | (2 if param_maps else 0) | (4 if nested else 0),
                                      *[params[k] for k in keys])
        return _Render.apply(scene, d, params, keys, *[params[k] for k in keys])

    if not unbiased:
        return differentiable(spp, base)
    with torch.no_grad():
        if params is not None:
            params.update()
        image = _image_of(_render_film(scene, _desc(scene, sensor, integrator, spp[0], base)))
    image_diff = differentiable(spp[1], base + _DERIV_SEED_OFFSET)
    return image_diff + (image - image_diff).detach()        # ek.reattach(image, image_diff), autodiff.py:185-187


def render_torch(scene, params=None, **kwargs):
    """autodiff.py:380-482: the image as a torch tensor whose autograd graph reaches ``params``."""
    return render(scene, params=params, **kwargs)


class Optimizer:
    """autodiff.py:200-243"""

    def __init__(self, params, lr):
        self.set_learning_rate(lr)
        self.params = params
        if not params.all_differentiable():
            raise Exception("Optimizer.__init__(): all parameters should be differentiable!")
        self.state = {}
        for k, p in self.params.items():
            p.requires_grad_(True)
            self._reset(k)

    def set_learning_rate(self, lr):
        self.lr = lr

    @contextmanager
    def disable_gradients(self):
        for _, p in self.params.items():
            p.requires_grad_(False)
        try:
            yield
        finally:
            for _, p in self.params.items():
                p.requires_grad_(True)

    def _replace(self, key, value):
        value = value.detach()           # a fresh tensor (the result of the update expression): no copy needed
        value.requires_grad_(True)
        self.params.properties[key] = value


class SGD(Optimizer):
    """autodiff.py:246-306: v <- mu v + g ; p <- p - lr v"""

    def __init__(self, params, lr, momentum=0):
        assert momentum >= 0 and momentum < 1
        assert lr > 0
        self.momentum = momentum
        super().__init__(params, lr)

    def step(self):
        for k, p in list(self.params.items()):
            g = p.grad
            if g is None:
                continue
            if self.momentum != 0:
                self.state[k] = self.momentum * self.state[k] + g
                value = p.detach() - self.lr * self.state[k]
            else:
                value = p.detach() - self.lr * g
            self._replace(k, value)
        self.params.update()

    def _reset(self, key):
        if self.momentum == 0:
            return
        self.state[key] = torch.zeros_like(self.params[key])

    def __repr__(self):
        return "SGD[\n  lr = %.2g,\n  momentum = %.2g\n]" % (self.lr, self.momentum)


class Adam(Optimizer):
    """autodiff.py:309-377"""

    def __init__(self, params, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-8):
        super().__init__(params, lr)
        assert 0 <= beta_1 < 1 and 0 <= beta_2 < 1 and lr > 0 and epsilon > 0
        self.beta_1, self.beta_2, self.epsilon = beta_1, beta_2, epsilon
        self.t = 0

    def step(self):
        self.t += 1
        lr_t = self.lr * math.sqrt(1 - self.beta_2 ** self.t) / (1 - self.beta_1 ** self.t)
        for k, p in list(self.params.items()):
            g = p.grad
            if g is None:
                continue
            m_t, v_t = self.state[k]                       # updated in place: m <- b1 m + (1 - b1) g, v <- b2 v + (1 - b2) g^2
            m_t.mul_(self.beta_1).add_(g, alpha=1 - self.beta_1)
            v_t.mul_(self.beta_2).addcmul_(g, g, value=1 - self.beta_2)
            self._replace(k, torch.addcdiv(p.detach(), m_t, torch.sqrt(v_t).add_(self.epsilon), value=-lr_t))
        self.params.update()      # the reference leaves this to the next render's parameters_changed(); explicit here

    def _reset(self, key):
        p = self.params[key]
        self.state[key] = (torch.zeros_like(p), torch.zeros_like(p))

    def __repr__(self):
        return "Adam[\n  lr = %g,\n  betas = (%g, %g),\n  eps = %g\n]" % (self.lr, self.beta_1, self.beta_2, self.epsilon)

"""Host side of the operator API (mitsuba2_amd.render: BSDFContext, BSDFFlags, DirectionSample3f, spawn_ray, a <bsdf> loaded on its own):
what needs no device."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _si(R, **kw):
    n = next(iter(kw.values())).shape[0]
    base = dict(t=torch.ones(n), prim_index=torch.zeros(n, dtype=torch.int32), shape_index=torch.zeros(n, dtype=torch.int32))
    base.update(kw)
    return R.SurfaceInteraction3f(**base)


def test_direction_sample_from_two_interactions():
    """DirectionSample(it, ref) (records.h:168-174): d and dist from it.p - ref.p, n = the shading normal of `it`, -it.wi where `it`
    is not valid"""
    from mitsuba2_amd import render as R
    it = _si(R, t=torch.tensor([2.0, float("inf"), 1.0]), p=torch.tensor([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [4.0, 0.0, 3.0]]),
             n=torch.tensor([[1.0, 0.0, 0.0]] * 3), sh_frame_n=torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]]),
             wi=torch.tensor([[0.0, 0.0, 1.0], [0.0, -0.6, 0.8], [0.0, 0.0, 1.0]]))
    ref = _si(R, p=torch.tensor([[1.0, 2.0, 1.0], [5.0, 5.0, 5.0], [0.0, 0.0, 0.0]]))
    ds = R.DirectionSample3f(it, ref)
    assert torch.equal(ds.dist[[0, 2]], torch.tensor([2.0, 5.0]))
    assert torch.equal(ds.d[0], torch.tensor([0.0, 0.0, 1.0]))
    want = torch.tensor([4.0, 0.0, 3.0]) * (torch.tensor(1.0) / torch.tensor(5.0))       # the kernels divide by multiplying with 1 / dist
    assert torch.equal(ds.d[2], want)
    assert torch.equal(ds.d[1], torch.tensor([-0.0, 0.6, -0.8]))                          # escaped lane: -it.wi
    assert torch.equal(ds.n, it.sh_frame_n) and torch.equal(ds.p, it.p)                  # the SHADING normal, not the geometric one
    assert ds.pdf.shape == (3,) and not ds.delta.any()
    # the element-by-element form stays
    e = R.DirectionSample3f(p=it.p, n=it.n, d=ds.d, dist=ds.dist, pdf=ds.pdf, delta=ds.delta, object=None)
    assert e.n is it.n and e.d is ds.d


def test_spawn_ray_epsilons():
    """Interaction::spawn_ray / spawn_ray_to (interaction.h:58-69): mint = RayEpsilon * (1 + max |p|), maxt = inf resp.
    dist * (1 - ShadowEpsilon)"""
    from mitsuba2_amd import render as R
    f32 = np.float32
    assert R.RayEpsilon == float(f32(np.finfo(f32).eps / 2 * 1500)) and R.ShadowEpsilon == float(f32(R.RayEpsilon) * f32(10))
    p = torch.tensor([[1.0, -7.5, 3.0], [0.0, 0.0, 0.0], [552.8, 0.25, -559.2]])
    si = _si(R, p=p)
    d = torch.tensor([[0.0, 0.0, 1.0]] * 3)
    ray = si.spawn_ray(d)
    want = ((f32(1.0) + np.abs(p.numpy()).max(axis=1)) * f32(R.RayEpsilon)).astype(f32)
    assert np.array_equal(ray.mint.numpy(), want) and ray.mint.dtype == torch.float32
    assert torch.isinf(ray.maxt).all() and (ray.maxt > 0).all()
    assert torch.equal(ray.o, p) and torch.equal(ray.d, d)
    target = p + torch.tensor([[0.0, 3.0, 4.0]] * 3)
    ray = si.spawn_ray_to(target)
    assert np.array_equal(ray.mint.numpy(), want)
    dist = np.sqrt(((target - p).numpy() ** 2).sum(axis=1)).astype(f32)
    assert np.allclose(ray.maxt.numpy(), dist * (f32(1.0) - f32(R.ShadowEpsilon)), rtol=1e-6, atol=0)
    assert (ray.maxt.numpy() < dist).all()
    assert np.allclose(ray.d.numpy(), [[0.0, 0.6, 0.8]] * 3, rtol=1e-6)


def test_to_local_and_to_world_are_inverse_on_an_orthonormal_frame():
    from mitsuba2_amd import render as R
    s, t, n = torch.tensor([[0.0, 1.0, 0.0]]), torch.tensor([[0.0, 0.0, 1.0]]), torch.tensor([[1.0, 0.0, 0.0]])
    si = _si(R, sh_frame_s=s, sh_frame_t=t, sh_frame_n=n)
    v = torch.tensor([[0.25, -0.5, 2.0]])
    assert torch.equal(si.to_local(v), torch.tensor([[-0.5, 2.0, 0.25]]))
    assert torch.equal(si.to_world(si.to_local(v)), v)


def test_bsdf_flags_and_has_flag():
    """BSDFFlags values and unions of bsdf.h:38-124; flags of the plugins as their constructors set them"""
    from mitsuba2_amd import render as R, bsdfs as B
    F = R.BSDFFlags
    assert int(F.Null) == 1 and int(F.DiffuseReflection) == 2 and int(F.GlossyReflection) == 8 and int(F.DeltaReflection) == 0x20
    assert int(F.DeltaTransmission) == 0x40 and int(F.FrontSide) == 0x8000 and int(F.BackSide) == 0x10000
    assert F.Smooth == F.DiffuseReflection | F.DiffuseTransmission | F.GlossyReflection | F.GlossyTransmission
    assert F.Delta == F.Null | F.DeltaReflection | F.DeltaTransmission and int(F.All) == 0x1FF
    assert R.has_flag(F.DeltaReflection, F.Delta) and not R.has_flag(F.DeltaReflection, F.Smooth)
    t = torch.tensor([int(F.Null), int(F.GlossyReflection), 0], dtype=torch.int32)
    assert R.has_flag(t, F.Delta).tolist() == [True, False, False] and R.has_flag(t, F.Smooth).tolist() == [False, True, False]
    flags = lambda d: R.bsdf_flags(B.normalize(d))
    assert flags({"type": "diffuse"}) == int(F.DiffuseReflection | F.FrontSide)
    assert flags({"type": "twosided", "bsdf": {"type": "diffuse"}}) == int(F.DiffuseReflection | F.FrontSide | F.BackSide)
    assert R.has_flag(flags({"type": "plastic"}), F.Smooth) and R.has_flag(flags({"type": "plastic"}), F.Delta)
    assert not R.has_flag(flags({"type": "dielectric"}), F.Smooth)
    assert R.has_flag(flags({"type": "roughconductor", "eta": 0.0, "alpha_u": 0.1, "alpha_v": 0.3}), F.Anisotropic)
    mask = flags({"type": "mask", "nested": {"type": "diffuse"}})
    assert R.has_flag(mask, F.Null) and R.has_flag(mask, F.Delta) and R.has_flag(mask, F.Smooth)      # the null lobe counts as delta
    # the kernels' own notion of Smooth (bsdf_is_smooth, mirrored in bsdfs.SMOOTH) agrees for every plain plugin
    for name, tid in B.TYPE_IDS.items():
        d = {"type": name, "eta": 0.0} if "conductor" in name else {"type": name}
        assert bool(R.has_flag(flags(d), F.Smooth)) == B.SMOOTH[tid], name


def test_bsdf_context_refuses_what_is_not_built():
    from mitsuba2_amd import render as R
    ctx = R.BSDFContext()
    assert ctx.mode == R.TransportMode.Radiance and ctx.type_mask == 0x1FF and ctx.component == 0xFFFFFFFF
    with pytest.raises(RuntimeError, match="component selection is not built"):
        R.BSDFContext(component=0)
    with pytest.raises(RuntimeError, match="component selection is not built"):
        R.BSDFContext(type_mask=int(R.BSDFFlags.Delta))
    with pytest.raises(RuntimeError, match="Importance"):
        R.BSDFContext(mode=R.TransportMode.Importance)
    ctx.component = 1                                         # set after construction: refused when the context is used
    with pytest.raises(RuntimeError, match="component selection is not built"):
        ctx._check()


BSDF_XML = ('<bsdf type="roughconductor" id="m"><float name="alpha" value="0.2"/><string name="distribution" value="ggx"/>'
            '<rgb name="eta" value="0.2, 0.92, 1.1"/><rgb name="k" value="3.9, 2.45, 2.14"/></bsdf>')


def test_standalone_bsdf_from_xml_and_dict():
    """a root <bsdf> / a BSDF plugin dictionary loads as a render.BSDF with the record of bsdfs.normalize -- without touching a device"""
    from mitsuba2_amd import render as R, xml as mxml, bsdfs as B
    plugin = {"type": "roughconductor", "id": "m", "alpha": 0.2, "distribution": "ggx", "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14]}
    b = mxml.load_string(BSDF_XML)
    assert isinstance(b, R.BSDF) and b.record() == B.normalize(plugin)
    assert b.flags() == R.bsdf_flags(B.normalize(plugin)) and R.has_flag(b.flags(), R.BSDFFlags.GlossyReflection)
    d = mxml.load_dict(plugin)
    assert isinstance(d, R.BSDF) and d.record() == B.normalize(plugin)
    nested = {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.6, 0.3, 0.2]}}}
    t = mxml.load_dict(nested)
    assert t.record() == B.normalize({"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": [0.6, 0.3, 0.2]}})
    blend = mxml.load_string('<bsdf type="blendbsdf"><float name="weight" value="0.3"/><bsdf type="diffuse"/><bsdf type="conductor"/></bsdf>')
    assert blend.record()["type"] == B.BLEND and [c["type"] for c in blend.record()["children"]] == [B.DIFFUSE, B.CONDUCTOR]
    # the loader's own errors stay
    with pytest.raises(mxml.XMLError, match='unexpected attribute "foo" in element "bsdf"'):
        mxml.load_string('<bsdf type="diffuse" foo="1"/>')
    with pytest.raises(mxml.XMLError, match="BSDF plugin 'hair' is not supported"):
        mxml.load_string('<bsdf type="hair"/>')
    with pytest.raises(mxml.XMLError, match='unreferenced property "shininess"'):
        mxml.load_string('<bsdf type="diffuse"><float name="shininess" value="2"/></bsdf>')


def test_root_elements():
    """a <bsdf> root no longer raises "must be a scene"; a property as root still raises what it raised"""
    from mitsuba2_amd import xml as mxml
    assert isinstance(mxml.parse_string('<bsdf type="diffuse"/>'), mxml.BSDFDescription)
    with pytest.raises(Exception, match='root element "integer" must be an object'):
        mxml.parse_string('<?xml version="1.0"?><integer name="a" value="10"></integer>')
    with pytest.raises(mxml.XMLError, match='root element "shape" must be a scene or a bsdf'):
        mxml.parse_string('<shape type="rectangle"/>')
    assert mxml.parse_string('<scene version="2.0.0"></scene>').scene_dict["meshes"] == []


def test_header_declares_every_operator_symbol():
    """include/mtsamd.h declares what _lib.py binds for the operator API, with the reference interfaces it stands for, and the ABI
    version stays 6 (an additive change)"""
    from mitsuba2_amd import _lib
    text = open(os.path.join(ROOT, "include", "mtsamd.h")).read()
    names = ("mtsamd_bsdf_eval_pdf", "mtsamd_bsdf_sample", "mtsamd_sample_emitter_direction", "mtsamd_pdf_emitter_direction",
             "mtsamd_emitter_eval", "mtsamd_sampler_seed", "mtsamd_sampler_next", "mtsamd_scene_shape_tables")
    for name in names:
        assert name in _lib.SYMBOLS, name
        assert re.search(r"MTSAMD_API int %s\(" % name, text), name
    for ref in ("bsdf.h", "scene.cpp:165-189", "scene.cpp:191-206", "emitter.h", "independent.cpp:62-72", "shape.h"):
        assert ref in text, ref
    lib = _lib.lib()
    assert lib.mtsamd_abi_version() == 6
    # arguments the host can check are refused before a device is touched
    assert lib.mtsamd_bsdf_eval_pdf(None, 4, None, None, None) < 0 and b"null scene" in lib.mtsamd_last_error()
    assert lib.mtsamd_sampler_next(4, 3, None, None, None, None, None) < 0 and b"dims" in lib.mtsamd_last_error()
    assert lib.mtsamd_sampler_seed(4, 0, 0, None, None, None) < 0
    assert lib.mtsamd_sampler_seed(0, 0, 0, None, None, None) == 0          # n == 0: OK, nothing launched

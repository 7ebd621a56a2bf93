"""Tabulated and analytic spectra of the spectral variant, the part that needs no GPU: ingestion of every XML / dictionary / file form
(src/libcore/xml.cpp:1084-1125, src/spectra/regular.cpp, irregular.cpp, d65.cpp, blackbody.cpp), the validation errors of the C ABI with
the reference's messages (include/mitsuba/core/distr_1d.h:293-345, 561-622), Texture::mean() (regular.cpp:99-101, irregular.cpp:111-113)
and the additive ABI."""
import ctypes as C

import numpy as np
import pytest

from mitsuba2_amd import _lib as L
from mitsuba2_amd import bsdfs as B
from mitsuba2_amd import emitters as E
from mitsuba2_amd import render as R
from mitsuba2_amd import spectrum as S
from mitsuba2_amd import xml as mxml

F32 = np.float32


# ---- ingestion -------------------------------------------------------------------------------------------------------------------
def test_plugin_dictionaries_parse_to_their_kind():
    reg = S.parse({"type": "regular", "lambda_min": 500, "lambda_max": 600, "values": "1, 2"})            # test_regular.py:10-16
    assert reg["kind"] == "regular" and reg["lambda_min"] == 500.0 and reg["lambda_max"] == 600.0
    assert reg["values"].dtype == F32 and reg["values"].tolist() == [1.0, 2.0]
    irr = S.parse({"type": "irregular", "wavelengths": "500, 600, 650", "values": "1, 2, .5"})            # test_irregular.py:10-15
    assert irr["kind"] == "irregular" and irr["wavelengths"].tolist() == [500.0, 600.0, 650.0] and irr["values"].tolist() == [1.0, 2.0, 0.5]
    seq = S.parse({"type": "irregular", "wavelengths": [400, 410, 500], "values": np.array([0.1, 0.2, 0.3])})
    assert seq["wavelengths"].tolist() == [400.0, 410.0, 500.0] and np.array_equal(seq["values"], np.array([0.1, 0.2, 0.3], F32))
    bb = S.parse({"type": "blackbody", "temperature": 6504})
    assert bb == {"kind": "blackbody", "temperature": 6504.0}


def test_d65_expands_to_the_reference_table():
    """d65.cpp:44-66: 95 entries over 360..830 nm, data[i] * (scale * (1 / 10568)) in float32"""
    d = S.parse({"type": "d65", "scale": 2.5})
    assert d["kind"] == "regular" and d["lambda_min"] == 360.0 and d["lambda_max"] == 830.0 and d["values"].size == 95
    scale = F32(2.5) * (F32(1.0) / F32(10568.0))
    assert np.array_equal(d["values"], S._cie()["d65"] * scale)
    assert S.parse({"type": "d65"})["values"][48] == S._cie()["d65"][48] * (F32(1.0) / F32(10568.0))       # 600 nm, default scale 1


def test_pairs_follow_the_loader():
    """xml.cpp:1087-1124: pairs inside an emitter are scaled by MTS_CIE_Y_NORMALIZATION, others are not; equal gaps (within
    math::Epsilon<float> of the first) make a `regular` spectrum, anything else an `irregular` one"""
    refl = S.from_pairs([400, 500, 600, 700], [0.04, 0.05, 0.55, 0.63], False)
    assert refl["kind"] == "regular" and refl["lambda_min"] == 400.0 and refl["lambda_max"] == 700.0
    assert np.array_equal(refl["values"], np.array([0.04, 0.05, 0.55, 0.63], F32))
    emit = S.from_pairs([400, 500, 600, 700], [0, 8, 15.6, 18.4], True)
    assert np.array_equal(emit["values"], np.array([0, 8, 15.6, 18.4], F32) * S.MTS_CIE_Y_NORMALIZATION)
    irr = S.from_pairs([400, 500, 650], [1, 2, 3], False)
    assert irr["kind"] == "irregular" and irr["wavelengths"].tolist() == [400.0, 500.0, 650.0]
    # the epsilon rule: a gap that differs from the first by one float32 step at 100 (7.6e-6 > 6e-8) is irregular ...
    assert S.from_pairs([400, 500, np.nextafter(F32(600), F32(700))], [1, 1, 1], False)["kind"] == "irregular"
    # ... gaps that are equal in float32 although the decimal inputs are not exactly representable stay regular
    assert S.from_pairs([360.5, 361.0, 361.5, 362.0], [1, 1, 1, 1], False)["kind"] == "regular"
    assert S.from_pairs([500, 600], [1, 2], False)["kind"] == "regular"           # a single gap is regular
    with pytest.raises(RuntimeError, match="increasing order"):
        S.from_pairs([500, 400], [1, 1], False)


XML = """<scene version="2.0.0">
    <bsdf type="diffuse" id="redish"><spectrum name="reflectance" value="400:0.04, 500:0.05, 600:0.55, 700:0.63"/></bsdf>
    <bsdf type="roughconductor" id="metal">
        <spectrum name="eta" value="400:1.4, 500:0.9, 650:0.2"/>
        <spectrum name="k" type="irregular"><string name="wavelengths" value="400, 500, 650"/><string name="values" value="1.9, 1.8, 3.4"/></spectrum>
    </bsdf>
    <shape type="rectangle"><ref id="redish"/></shape>
    <shape type="rectangle"><ref id="metal"/>
        <emitter type="area"><spectrum name="radiance" value="400:0, 500:8, 600:15.6, 700:18.4"/></emitter></shape>
    <emitter type="point"><spectrum name="intensity" type="blackbody"><float name="temperature" value="3000"/></spectrum></emitter>
</scene>"""


def test_xml_carries_the_spectrum_beside_the_rgb_value():
    d = mxml.parse_string(XML)
    assert d.uses_tabulated_spectra
    red, metal = d.scene_dict["bsdfs"][:2]
    # the RGB value is still there and is today's pre-integration
    assert red["reflectance"] == S.tabulated_to_rgb([400, 500, 600, 700], [0.04, 0.05, 0.55, 0.63], False, "reflectance")
    assert metal["eta"] == S.tabulated_to_rgb([400, 500, 650], [1.4, 0.9, 0.2], False, "eta")
    n_red, n_metal = B.normalize(red), B.normalize(metal)
    assert n_red["reflectance"] == red["reflectance"] and set(n_red["spectra"]) == {0}
    spec = S.parse(n_red["spectra"][0])
    assert spec["kind"] == "regular" and np.array_equal(spec["values"], np.array([0.04, 0.05, 0.55, 0.63], F32))       # not scaled
    assert set(n_metal["spectra"]) == {2, 3}                                   # MTSAMD_PARAM_ETA, MTSAMD_PARAM_K
    eta = S.parse(n_metal["spectra"][2])
    assert eta["kind"] == "irregular" and eta["wavelengths"].tolist() == [400.0, 500.0, 650.0]
    k = n_metal["spectra"][3]
    assert k["kind"] == "irregular" and np.array_equal(k["values"], np.array([1.9, 1.8, 3.4], F32))
    assert len(n_metal["k"]) == 3 and min(n_metal["k"]) > 1.0                 # the nested plugin's RGB value: unbounded pre-integration
    area, point = d.scene_dict["emitters"]
    assert area["radiance"] == S.tabulated_to_rgb([400, 500, 600, 700], [0, 8, 15.6, 18.4], True, "radiance")
    n_area = E.normalize(area)
    got = S.parse(n_area["spectrum"], within_emitter=True)
    assert np.array_equal(got["values"], np.array([0, 8, 15.6, 18.4], F32) * S.MTS_CIE_Y_NORMALIZATION)             # scaled inside emitters
    assert E.normalize(point)["spectrum"] == {"kind": "blackbody", "temperature": 3000.0}


def test_load_dict_and_file_forms(tmp_path):
    spd = tmp_path / "Au.eta.spd"
    spd.write_text("# wavelength value\n400 1.4\n500 0.9\n\n650 0.2\n")
    d = mxml.parse_dict({"type": "scene",
                         "metal": {"type": "conductor", "eta": {"type": "spectrum", "value": [(400, 1.4), (500, 0.9), (650, 0.2)]},
                                   "k": {"type": "regular", "lambda_min": 400, "lambda_max": 700, "values": [1.9, 1.8, 3.4, 4.0]}}})
    n = B.normalize(d.scene_dict["bsdfs"][0])
    assert S.parse(n["spectra"][2])["kind"] == "irregular" and n["spectra"][3]["kind"] == "regular" and n["spectra"][3]["values"].size == 4
    x = mxml.parse_string('<scene version="2.0.0"><bsdf type="conductor"><spectrum name="eta" filename="Au.eta.spd"/></bsdf></scene>',
                          base_dir=str(tmp_path))
    eta = S.parse(B.normalize(x.scene_dict["bsdfs"][0])["spectra"][2])
    assert eta["kind"] == "irregular" and eta["wavelengths"].tolist() == [400.0, 500.0, 650.0] and eta["values"].tolist() == [F32(1.4), F32(0.9), F32(0.2)]
    f = S.parse({"type": "spectrum", "filename": str(spd)})
    assert np.array_equal(f["values"], eta["values"])
    # the load_dict form with a file, relative to the base directory and absolute
    for fn in ("Au.eta.spd", str(spd)):
        y = mxml.parse_dict({"type": "scene", "metal": {"type": "conductor", "eta": {"type": "spectrum", "filename": fn}}}, base_dir=str(tmp_path))
        assert y.uses_tabulated_spectra and y.scene_dict["bsdfs"][0]["eta"] == S.tabulated_to_rgb([400, 500, 650], [1.4, 0.9, 0.2], False, "eta")
        got = S.parse(B.normalize(y.scene_dict["bsdfs"][0])["spectra"][2])
        assert got["kind"] == "irregular" and np.array_equal(got["wavelengths"], eta["wavelengths"]) and np.array_equal(got["values"], eta["values"])
    with pytest.raises(Exception, match="file does not exist"):
        mxml.parse_dict({"type": "scene", "metal": {"type": "conductor", "eta": {"type": "spectrum", "filename": "missing.spd"}}}, base_dir=str(tmp_path))
    with pytest.raises(Exception, match="2 entries"):
        mxml.parse_dict({"type": "scene", "metal": {"type": "conductor", "eta": {"type": "spectrum", "filename": fn, "value": 1.0}}})


def test_xml_nested_regular_and_d65_plugins():
    d = mxml.parse_string("""<scene version="2.0.0">
        <bsdf type="diffuse" id="tab"><spectrum name="reflectance" type="regular">
            <float name="lambda_min" value="400"/><float name="lambda_max" value="700"/><string name="values" value="0.1, 0.2 0.6,0.7"/></spectrum></bsdf>
        <shape type="rectangle"><ref id="tab"/><emitter type="area"><spectrum name="radiance" type="d65"><float name="scale" value="3"/></spectrum></emitter></shape>
        <emitter type="constant"><spectrum name="radiance" type="d65"/></emitter>
    </scene>""")
    n = B.normalize(d.scene_dict["bsdfs"][0])
    reg = n["spectra"][0]
    assert reg["kind"] == "regular" and (reg["lambda_min"], reg["lambda_max"]) == (400.0, 700.0) and np.array_equal(reg["values"], np.array([0.1, 0.2, 0.6, 0.7], F32))
    assert n["reflectance"] == S.to_rgb(reg, False, "reflectance") and max(n["reflectance"]) <= 1.0          # what the RGB variant renders
    area, const = (E.normalize(e) for e in d.scene_dict["emitters"])
    assert area["spectrum"]["kind"] == "regular" and np.array_equal(area["spectrum"]["values"], S._cie()["d65"] * (F32(3.0) * (F32(1.0) / F32(10568.0))))
    assert const["spectrum"]["values"].size == 95 and const["spectrum"]["lambda_min"] == 360.0 and const["spectrum"]["lambda_max"] == 830.0
    assert np.allclose(const["radiance"], [1.0, 1.0, 1.0], atol=2e-2)         # d65 at scale 1 integrates to white (d65.cpp:45-47)


def test_nest_weights_refuse_spectra():
    """blendbsdf weights / mask opacities are scalars (Texture::eval_1): a spectrum is refused by name, in every form it can arrive in"""
    kid = '<bsdf type="diffuse"/>'
    for xml in ('<bsdf type="blendbsdf"><spectrum name="weight" value="400:0.2, 700:0.8"/>%s%s</bsdf>' % (kid, kid),
                '<bsdf type="mask"><spectrum name="opacity" value="400:0.2, 700:0.8"/>%s</bsdf>' % kid):
        with pytest.raises(Exception, match="is a scalar .*not a spectrum"):
            mxml.parse_string('<scene version="2.0.0">%s</scene>' % xml)
    with pytest.raises(RuntimeError, match="is a scalar .*not a spectrum"):
        B.normalize({"type": "blendbsdf", "weight": {"type": "regular", "lambda_min": 400, "lambda_max": 700, "values": [0.2, 0.8]},
                     "a": {"type": "diffuse"}, "b": {"type": "diffuse"}})


def test_plugin_in_an_rgb_scene_is_pre_integrated():
    """a spectrum plugin given to an RGB scene: regular / irregular go through spectrum_to_rgb, blackbody raises as the reference does"""
    n = B.normalize({"type": "diffuse", "reflectance": {"type": "irregular", "wavelengths": [400, 500, 600, 700], "values": [0.04, 0.05, 0.55, 0.63]}})
    assert n["reflectance"] == S.tabulated_to_rgb([400, 500, 600, 700], [0.04, 0.05, 0.55, 0.63], False, "reflectance")
    assert n["uniform_mask"] == 0
    with pytest.raises(RuntimeError, match="[Nn]ot implemented for non-spectral"):
        S.to_rgb(S.parse({"type": "blackbody", "temperature": 3000}), True, "radiance")
    e = E.normalize({"type": "point", "intensity": {"type": "blackbody", "temperature": 3000}})
    assert e["spectrum"]["kind"] == "blackbody"          # render.Scene(variant="rgb") raises for it (test_gpu_spectra.py)
    with pytest.raises(RuntimeError, match="emission spectrum"):
        B.normalize({"type": "diffuse", "reflectance": {"type": "blackbody", "temperature": 3000}})
    with pytest.raises(RuntimeError, match="takes no spectrum"):
        B.normalize({"type": "dielectric", "int_ior": 1.5, "spectra": {"eta": {"type": "spectrum", "value": [(400, 1), (500, 2)]}}})


@pytest.mark.parametrize("plugin, message", [
    ({"type": "regular", "lambda_min": 400, "lambda_max": 700, "values": [1.0]}, "ContinuousDistribution: needs at least two entries!"),
    ({"type": "regular", "lambda_min": 700, "lambda_max": 700, "values": [1.0, 2.0]}, "ContinuousDistribution: invalid range!"),
    ({"type": "irregular", "wavelengths": [400], "values": [1.0]}, "IrregularContinuousDistribution: needs at least two entries!"),
    ({"type": "irregular", "wavelengths": [400, 500, 600], "values": [1.0, 2.0]}, "'pdf' and 'nodes' size mismatch!"),
    ({"type": "irregular", "wavelengths": [400, 600, 600], "values": [1.0, 2.0, 3.0]}, "node positions must be strictly increasing!"),
    ({"type": "regular", "lambda_min": 400, "lambda_max": 700, "values": "1, x"}, "Could not parse floating point value 'x'"),
])
def test_python_validation_uses_the_reference_messages(plugin, message):
    with pytest.raises(RuntimeError, match=message.replace("(", r"\(").replace(")", r"\)")):
        S.parse(plugin)


# ---- C ABI: validation, mean, additive layout ------------------------------------------------------------------------------------------
def _desc(kind, values=(), wavelengths=None, lambda_min=0.0, lambda_max=0.0, temperature=0.0, keep=None):
    d = L.SpectrumDesc()
    d.type, d.size, d.lambda_min, d.lambda_max, d.temperature = kind, len(values), lambda_min, lambda_max, temperature
    v = np.ascontiguousarray(values, F32)
    keep.append(v)
    d.values = v.ctypes.data_as(L.f32p)
    if wavelengths is not None:
        w = np.ascontiguousarray(wavelengths, F32)
        keep.append(w)
        d.wavelengths = w.ctypes.data_as(L.f32p)
    return d


def _mean(d):
    out = C.c_float()
    L.check(L.lib().mtsamd_spectrum_mean(C.byref(d), C.byref(out)))
    return F32(out.value)


def test_spectrum_mean_matches_the_reference_fixtures():
    keep = []
    # test_regular.py:10-16, :29: integral 150; test_irregular.py:10-15, :28: integral 212.5
    assert _mean(_desc(0, [1, 2], lambda_min=500, lambda_max=600, keep=keep)) == F32(150.0) / (F32(830.0) - F32(360.0))
    assert _mean(_desc(1, [1, 2, 0.5], [500, 600, 650], keep=keep)) == F32(212.5) / (F32(830.0) - F32(360.0))
    assert _mean(_desc(0, [0.5] * 95, lambda_min=360, lambda_max=830, keep=keep)) == F32(0.5)
    assert _mean(_desc(1, [0.5, 0.5, 0.5], [360, 500, 830], keep=keep)) == F32(0.5)
    assert R.spectrum_mean({"type": "regular", "lambda_min": 500, "lambda_max": 600, "values": "1, 2"}) == pytest.approx(150.0 / 470.0, rel=1e-7)


@pytest.mark.parametrize("make, message", [
    (lambda k: _desc(0, [1.0], lambda_min=400, lambda_max=700, keep=k), "ContinuousDistribution: needs at least two entries!"),
    (lambda k: _desc(1, [1.0], [400.0], keep=k), "IrregularContinuousDistribution: needs at least two entries!"),
    (lambda k: _desc(1, [1.0, 2.0, 3.0], [400, 600, 600], keep=k), "node positions must be strictly increasing!"),
    (lambda k: _desc(1, [1.0, 2.0, 3.0], [400, 600, 500], keep=k), "node positions must be strictly increasing!"),
    (lambda k: _desc(0, [1.0, 2.0], lambda_min=700, lambda_max=700, keep=k), "ContinuousDistribution: invalid range!"),
    (lambda k: _desc(0, [1.0, 2.0], lambda_min=700, lambda_max=400, keep=k), "ContinuousDistribution: invalid range!"),
    (lambda k: _desc(0, [1.0, -2.0], lambda_min=400, lambda_max=700, keep=k), "entries must be non-negative!"),
    (lambda k: _desc(0, [0.0, 0.0], lambda_min=400, lambda_max=700, keep=k), "no probability mass found!"),
])
def test_abi_validation_errors(make, message):
    """every spectrum error, through the host-only mean and through scene creation (which checks before it touches a device)"""
    keep = []
    d = make(keep)
    out = C.c_float()
    assert L.lib().mtsamd_spectrum_mean(C.byref(d), C.byref(out)) == -1
    assert message in L.lib().mtsamd_last_error().decode()
    sd = L.SceneDesc()
    sd.spectral = 1
    handle = C.c_void_p()
    with pytest.raises(RuntimeError, match=message.replace("(", r"\(").replace(")", r"\)")):
        L.check(L.lib().mtsamd_scene_create_with_spectra(C.byref(sd), C.byref(d), 1, None, 0, 0, C.byref(handle)))
    assert not handle.value


def test_abi_binding_errors():
    keep = []
    lib = L.lib()
    table, planck = _desc(0, [1.0, 2.0], lambda_min=400, lambda_max=700, keep=keep), _desc(2, temperature=3000.0, keep=keep)
    spectra = (L.SpectrumDesc * 2)(table, planck)
    bd = (L.BsdfDesc * 2)()
    bd[0].type, bd[0].texture, bd[1].type, bd[1].texture = B.DIFFUSE, -1, B.DIELECTRIC, -1
    ed = (L.EmitterDesc * 1)()
    ed[0].type = E.TYPE_IDS["envmap"]
    handle = C.c_void_p()

    def create(spectral, target, index, param, spectrum):
        sd = L.SceneDesc(None, 0, bd, 2, ed, 1, None, 0, spectral, None)
        bn = L.SpectrumBinding(target, index, param, spectrum)
        return lib.mtsamd_scene_create_with_spectra(C.byref(sd), spectra, 2, C.byref(bn), 1, 0, C.byref(handle)), lib.mtsamd_last_error().decode()

    rc, msg = create(0, 0, 0, 0, 0)                   # a spectrum on an RGB-variant scene
    assert rc == -5 and "spectral variant" in msg
    rc, msg = create(1, 0, 0, 0, 1)                   # blackbody on a BSDF
    assert rc == -1 and "blackbody" in msg
    rc, msg = create(1, 0, 1, 2, 0)                   # eta of a dielectric is an IOR, not a spectrum
    assert rc == -5 and "takes no spectrum" in msg
    rc, msg = create(1, 0, 0, 3, 0)                   # k of a diffuse BSDF
    assert rc == -5 and "takes no spectrum" in msg
    rc, msg = create(1, 1, 0, 0, 0)                   # an envmap
    assert rc == -5 and "envmap" in msg
    rc, msg = create(1, 0, 2, 0, 0)
    assert rc == -1 and "out of range" in msg
    rc, msg = create(1, 0, 0, 0, 2)
    assert rc == -1 and "out of range" in msg
    rc, msg = create(1, 7, 0, 0, 0)
    assert rc == -1 and "unknown target" in msg
    assert not handle.value


def test_abi_is_additive():
    """version 6, the three new symbols, and the layout of every existing descriptor unchanged (sizes on the LP64 ABI the library is built for)"""
    lib = L.lib()
    assert lib.mtsamd_abi_version() == 6
    for name in ("mtsamd_scene_create_with_spectra", "mtsamd_spectrum_eval", "mtsamd_spectrum_mean"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert (C.sizeof(L.MeshDesc), C.sizeof(L.BsdfDesc), C.sizeof(L.EmitterDesc), C.sizeof(L.TextureDesc), C.sizeof(L.SceneDesc), C.sizeof(L.RenderDesc)) == \
        (48, 112, 112, 72, 72, 216)
    assert C.sizeof(L.SpectrumDesc) == 40 and C.sizeof(L.SpectrumBinding) == 16
    assert lib.mtsamd_scene_create_with_spectra(None, None, 0, None, 0, 0, None) < 0 and b"null" in lib.mtsamd_last_error()

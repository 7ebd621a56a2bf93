"""The `aov` integrator (src/integrators/aov.cpp) without a GPU: the AOV string, the channel names and their order, the error messages,
XML / dict ingestion and the two entry points of the C ABI."""
import pytest

from mitsuba2_amd import render as R, xml as mxml

AOVS = "dd.y:depth, nn:sh_normal,p:position uvs:uv"
NAMES = ["dd.y", "nn.X", "nn.Y", "nn.Z", "p.X", "p.Y", "p.Z", "uvs.U", "uvs.V"]


def test_aov_string_gives_the_reference_names_in_order():
    """aov.cpp:88-134: split on commas and spaces; depth -> <name>, vectors -> .X .Y .Z, uv kinds -> .U .V"""
    integ = R.AOVIntegrator(AOVS)
    assert integ.aov_names() == NAMES
    assert integ.aov_channels() == ["X", "Y", "Z", "A", "W"] + NAMES
    every = R.AOVIntegrator("a:depth b:position c:uv d:geo_normal e:sh_normal f:dp_du g:dp_dv h:duv_dx i:duv_dy")
    assert every.aov_names() == ["a", "b.X", "b.Y", "b.Z", "c.U", "c.V", "d.X", "d.Y", "d.Z", "e.X", "e.Y", "e.Z", "f.X", "f.Y", "f.Z",
                                 "g.X", "g.Y", "g.Z", "h.U", "h.V", "i.U", "i.V"]
    assert every._types == list(range(9))          # mtsamd_aov_type


def test_nested_integrator_channels_come_last():
    """aov.cpp:136-151: <prop>.R/G/B/A after the string's AOVs"""
    integ = R.AOVIntegrator(AOVS, R.PathIntegrator(max_depth=5, pipeline=2, paths_per_wave=128), name="my_image")
    assert integ.aov_channels() == ["X", "Y", "Z", "A", "W"] + NAMES + ["my_image.R", "my_image.G", "my_image.B", "my_image.A"]
    assert integ.aov_channels()[-4:] == ["my_image." + c for c in "RGBA"]
    assert (integ.pipeline, integ.paths_per_wave) == (2, 128)          # scheduler knobs of the nested integrator
    assert R.AOVIntegrator("", R.DepthIntegrator()).aov_names() == ["integrator_0." + c for c in "RGBA"]


def test_error_messages():
    with pytest.raises(RuntimeError, match='Invalid AOV type "normal"'):
        R.AOVIntegrator("n:normal")
    for bad in ("depth", "a:b:depth", ":depth", "a:"):
        with pytest.raises(RuntimeError, match="Invalid AOV specification: require <name>:<type> pair"):
            R.AOVIntegrator(bad)
    with pytest.raises(RuntimeError, match="exactly one nested integrator"):
        R.AOVIntegrator("d:depth", [R.PathIntegrator(), R.DirectIntegrator()])
    for child in (R.MomentIntegrator(R.PathIntegrator()), R.AOVIntegrator("d:depth"), "path"):
        with pytest.raises(RuntimeError, match="must be a path, direct or depth integrator"):
            R.AOVIntegrator("d:depth", child)
    # Film::prepare refuses two channels of one name
    film = R.HDRFilm(8, 8)
    with pytest.raises(RuntimeError, match="duplicate channel name"):
        film.prepare(R.AOVIntegrator("a:depth,a:depth").aov_channels(), device="cpu")
    film.prepare(R.AOVIntegrator(AOVS).aov_channels(), device="cpu")
    assert film.channels() == ["X", "Y", "Z", "A", "W"] + NAMES


def _same(a, b):
    assert type(a) is type(b) and a.aov_channels() == b.aov_channels() and a._types == b._types and a.name == b.name
    assert type(a.nested) is type(b.nested)
    if a.nested is not None:
        assert (a.nested.max_depth, a.nested.rr_depth) == (b.nested.max_depth, b.nested.rr_depth)


def test_xml_and_dict_ingestion_agree():
    want = R.AOVIntegrator(AOVS, R.PathIntegrator(max_depth=5), name="my_image")
    x = mxml.parse_string("""<scene version="2.0.0"><integrator type="aov"><string name="aovs" value="%s"/>
        <integrator type="path" name="my_image"><integer name="max_depth" value="5"/></integrator></integrator></scene>""" % AOVS)
    d = mxml.parse_dict({"type": "scene", "integ": {"type": "aov", "aovs": AOVS, "my_image": {"type": "path", "max_depth": 5}}})
    assert x.integrator == d.integrator == dict(type="aov", aovs=AOVS, name="my_image", nested=dict(type="path", max_depth=5, rr_depth=5))
    _same(mxml._make_integrator(x.integrator), want)
    _same(mxml._make_integrator(d.integrator), want)
    # unnamed children get the names the moment branch uses; no child at all is allowed
    u = mxml.parse_string('<scene version="2.0.0"><integrator type="aov"><string name="aovs" value="d:depth"/><integrator type="depth"/></integrator></scene>')
    assert u.integrator["name"] == "integrator_0"
    _same(mxml._make_integrator(u.integrator), R.AOVIntegrator("d:depth", R.DepthIntegrator()))
    alone = mxml.parse_string('<scene version="2.0.0"><integrator type="aov"><string name="aovs" value="d:depth"/></integrator></scene>')
    _same(mxml._make_integrator(alone.integrator), R.AOVIntegrator("d:depth"))
    with pytest.raises(mxml.XMLError, match="exactly one nested integrator"):
        mxml.parse_string('<scene version="2.0.0"><integrator type="aov"><string name="aovs" value="d:depth"/><integrator type="depth"/>'
                          '<integrator type="path" name="b"/></integrator></scene>')
    with pytest.raises(mxml.XMLError, match='unreferenced property "aov"'):          # a stray scalar property is reported, not swallowed
        mxml.parse_string('<scene version="2.0.0"><integrator type="aov"><string name="aovs" value="d:depth"/><string name="aov" value="x:uv"/></integrator></scene>')
    with pytest.raises(mxml.XMLError, match=r"\(path, direct, depth, moment, aov\)"):
        mxml.parse_string('<scene version="2.0.0"><integrator type="volpath"/></scene>')


def test_abi_declares_the_entry_points():
    from mitsuba2_amd import _lib
    assert "mtsamd_render_aov" in _lib.SYMBOLS and "mtsamd_sample_aovs" in _lib.SYMBOLS
    lib = _lib.lib()
    assert lib.mtsamd_abi_version() == 6
    assert lib.mtsamd_render_aov.argtypes is not None and lib.mtsamd_sample_aovs.argtypes is not None
    assert lib.mtsamd_render_aov(None, None, None, 0, 0, None, None, None) == -1 and b"null" in lib.mtsamd_last_error()

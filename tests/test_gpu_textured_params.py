"""Textured alpha and specular colours of the conductor / dielectric BSDFs on the GPU, against the unchanged oracle (which knows
constant parameters only):

1. by splitting: the tall box of the Cornell box carries per-face texcoords strictly inside one checkerboard cell per face, so a
   checkerboard parameter takes one of two constants on every face; the oracle renders the same triangles as two meshes with two
   constant materials.  Per-sample radiance of `path` (pipelines 0 and 2) and `direct`, bit for bit;
2. the hierarchy instantiation: the displaced sphere at its smallest tessellation that is not LDS-resident, a checkerboard alpha whose
   two colours are equal against the constant;
3. a bitmap, exactly: BSDF.eval / pdf / sample of a roughconductor with bitmap alpha and bitmap specular_reflectance against the
   oracle's row-wise BSDF fed with the host restatement of the bilinear lookup (exactly rounded fused multiply-adds) and the luminance;
4. update_texture on the roughness map against a fresh scene built with the new map; the setter and adjoint refusals;
5. an XML scene with a <texture name="alpha"> child loads and renders."""
import functools
from fractions import Fraction

import numpy as np
import parity_util
import pytest
import torch

import oracle_binding as ob

pytestmark = pytest.mark.gpu
F32 = np.float32

CONDUCTOR_IOR = {"eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14]}
COLOURS = ([0.9, 0.8, 0.7], [0.2, 0.5, 0.6])
COLOURS_T = ([0.9, 0.95, 1.0], [0.5, 0.3, 0.8])


def _wrap_none(leaf):
    return leaf


def _wrap_twosided(leaf):
    return {"type": "twosided", "bsdf": leaf}


def _wrap_blend(leaf):
    return {"type": "blendbsdf", "weight": 0.3, "bsdf_0": leaf, "bsdf_1": {"type": "diffuse", "reflectance": [0.2, 0.5, 0.7]}}


# name -> (constant parameters of the leaf, {parameter: (value on the cell-0 faces, value on the cell-1 faces)}, wrapper)
CASES = {
    "rough_ggx_alpha": (dict(type="roughconductor", distribution="ggx", **CONDUCTOR_IOR), {"alpha": (0.1, 0.4)}, _wrap_none),
    "rough_beckmann_alpha_colour": (dict(type="roughconductor", distribution="beckmann", eta=0.0, k=1.0),
                                    {"alpha": (0.15, 0.3), "specular_reflectance": COLOURS}, _wrap_none),
    "rough_beckmann_aniso": (dict(type="roughconductor", distribution="beckmann", **CONDUCTOR_IOR), {"alpha_u": (0.3, 0.1), "alpha_v": (0.1, 0.35)}, _wrap_none),
    "rough_ggx_all_aniso_one_map": (dict(type="roughconductor", distribution="ggx", sample_visible=False, eta=0.0, k=1.0, alpha_v=0.2),
                                    {"alpha_u": (0.35, 0.12)}, _wrap_none),
    "frosted_alpha_transmittance": (dict(type="roughdielectric"), {"alpha": (0.1, 0.3), "specular_transmittance": COLOURS_T}, _wrap_none),
    "frosted_ggx_aniso_reflectance": (dict(type="roughdielectric", distribution="ggx", int_ior="diamond"),
                                      {"alpha_u": (0.3, 0.15), "alpha_v": (0.1, 0.25), "specular_reflectance": COLOURS}, _wrap_none),
    "conductor_colour": (dict(type="conductor", **CONDUCTOR_IOR), {"specular_reflectance": COLOURS}, _wrap_none),
    "glass_colours": (dict(type="dielectric", int_ior="bk7"), {"specular_reflectance": COLOURS, "specular_transmittance": COLOURS_T}, _wrap_none),
    "thin_glass_colours": (dict(type="thindielectric"), {"specular_reflectance": COLOURS, "specular_transmittance": COLOURS_T}, _wrap_none),
    "twosided_rough_alpha": (dict(type="roughconductor", distribution="ggx", eta=0.0, k=1.0), {"alpha": (0.1, 0.3)}, _wrap_twosided),
    "blend_child_alpha": (dict(type="roughconductor", distribution="ggx", **CONDUCTOR_IOR), {"alpha": (0.1, 0.4), "specular_reflectance": COLOURS}, _wrap_blend),
}


def _materials(case):
    """the textured plugin, and the two constant plugins it equals on the cell-0 / cell-1 faces"""
    base, params, wrap = CASES[case]
    textured = dict(base, **{p: {"type": "checkerboard", "color0": v0, "color1": v1} for p, (v0, v1) in params.items()})
    return wrap(textured), [wrap(dict(base, **{p: v[k] for p, v in params.items()})) for k in (0, 1)]


def _box_texcoords():
    """four uvs per face of the tall box, strictly inside checkerboard cell (0, 0) (colour 0) for the first three faces and inside cell
    (1, 0) (colour 1) for the last three: the cell-0 faces come first"""
    corner = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F32) * F32(0.25)
    return np.concatenate([corner + np.array([0.125 if face < 3 else 0.625, 0.125], F32) for face in range(6)]).astype(F32)


def _split_scenes(case):
    """(scene with the textured material on the tall box, the oracle's scene: the box as two meshes with constant materials).  The tall
    box is the last mesh, so the global primitive order and every other shape index are the same in both."""
    from mitsuba2_amd import scenes
    textured, constants = _materials(case)
    cb = scenes.cornell_box()
    floor = {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": [0.7, 0.7, 0.7]}}
    assert len(cb["meshes"]) == 8 and cb["meshes"][7]["faces"].shape == (12, 3)       # five walls, the light, the short box, the tall box
    box = dict(cb["meshes"][7], texcoords=_box_texcoords())
    n = len(cb["bsdfs"])
    others = [dict(cb["meshes"][0], bsdf=n)] + cb["meshes"][1:7]
    mine = dict(cb, bsdfs=list(cb["bsdfs"]) + [floor, textured], meshes=others + [dict(box, bsdf=n + 1)])
    theirs = dict(cb, bsdfs=list(cb["bsdfs"]) + [floor] + constants,
                  meshes=others + [dict(box, faces=np.ascontiguousarray(box["faces"][:6]), bsdf=n + 1),
                                   dict(box, faces=np.ascontiguousarray(box["faces"][6:]), bsdf=n + 2)])
    return mine, theirs


def _sensor(integrator):
    from mitsuba2_amd import scenes
    sp = dict(scenes.cornell_box_sensor(64, 64, spp=8, seed=21), max_depth=6)
    if integrator == "direct":
        sp.update(integrator="direct", emitter_samples=2, bsdf_samples=2)
    return sp


N = 64 * 64 * 8


@functools.lru_cache(maxsize=None)
def _oracle_samples(case, integrator):
    want, wpos = ob.OracleScene(_split_scenes(case)[1]).sample_radiance(ob.make_desc(_sensor(integrator)), 0, N)
    want.setflags(write=False), wpos.setflags(write=False)
    return want, wpos


def _check_samples(rgb, mask, pos, want, wpos):
    rgb, mask, pos = rgb.cpu().numpy(), mask.cpu().numpy(), pos.cpu().numpy()
    assert np.array_equal(pos, wpos) and np.array_equal(mask, want[:, 3] > 0.5)
    parity_util.check("per-sample radiance", rgb, want[:, :3])      # exact fraction 1.0


@pytest.mark.parametrize("pipeline", [0, 2])
@pytest.mark.parametrize("case", sorted(CASES))
def test_path_samples_match_split_oracle(case, pipeline):
    from mitsuba2_amd import render as R
    sp = _sensor("path")
    scene, sensor = R.Scene(_split_scenes(case)[0]), R.make_sensor(sp)
    _check_samples(*R.PathIntegrator(max_depth=6, pipeline=pipeline).sample(scene, sensor, 0, N), *_oracle_samples(case, "path"))


@pytest.mark.parametrize("case", sorted(CASES))
def test_direct_samples_match_split_oracle(case):
    from mitsuba2_amd import render as R
    scene, sensor = R.Scene(_split_scenes(case)[0]), R.make_sensor(_sensor("direct"))
    _check_samples(*R.DirectIntegrator(shading_samples=2).sample(scene, sensor, 0, N), *_oracle_samples(case, "direct"))


def test_the_two_cells_differ():
    """the split is not vacuous: the oracle's picture changes when the two constants are swapped"""
    want, _ = _oracle_samples("rough_ggx_alpha", "path")
    mine, theirs = _split_scenes("rough_ggx_alpha")
    n = len(theirs["bsdfs"])
    swapped = dict(theirs, meshes=theirs["meshes"][:7] + [dict(theirs["meshes"][7], bsdf=n - 1), dict(theirs["meshes"][8], bsdf=n - 2)])
    other, _ = ob.OracleScene(swapped).sample_radiance(ob.make_desc(_sensor("path")), 0, N)
    assert not np.array_equal(other[:, :3], want[:, :3])


# ---- 2. hierarchy scenes ----------------------------------------------------------------------------------------------------------------
def test_hierarchy_scene_equal_colours_match_constant():
    from mitsuba2_amd import render as R, scenes
    sd = scenes.bumpy_sphere(4, 11)        # 70 triangles: the smallest tessellation above the 64 primitives of an LDS-resident scene
    sphere = sd["meshes"][0]
    rng = np.random.default_rng(8)
    sphere = dict(sphere, texcoords=rng.uniform(0.0, 1.0, size=(sphere["positions"].shape[0], 2)).astype(F32))
    base = dict(type="roughconductor", distribution="ggx", **CONDUCTOR_IOR)
    to_uv = np.array([[7, 0, 0.3, 0], [0, 5, 0.1, 0], [0, 0, 1, 0], [0, 0, 0, 1]], F32)
    tex = dict(base, alpha={"type": "checkerboard", "color0": 0.2, "color1": 0.2, "to_uv": to_uv})
    mine = dict(sd, meshes=[sphere] + sd["meshes"][1:], bsdfs=[tex] + sd["bsdfs"][1:])
    theirs = dict(mine, bsdfs=[dict(base, alpha=0.2)] + sd["bsdfs"][1:])
    sp = dict(scenes.bumpy_sphere_sensor(64, 64, spp=8, seed=5), max_depth=5)
    scene, sensor = R.Scene(mine), R.make_sensor(sp)
    assert scene.info()["primitives"] > 64
    n = 64 * 64 * 8
    want, wpos = ob.OracleScene(theirs).sample_radiance(ob.make_desc(sp), 0, n)
    for pipeline in (0, 2):
        _check_samples(*R.PathIntegrator(max_depth=5, pipeline=pipeline).sample(scene, sensor, 0, n), want, wpos)


# ---- 3. a bitmap, exactly ---------------------------------------------------------------------------------------------------------------
def _round_f32(x):
    """the float32 nearest to the rational x, ties to even: one rounding, where float32(float(x)) rounds twice"""
    f = F32(float(x))
    best = None
    for c in (np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))):
        err = abs(Fraction(float(c)) - x)
        even = (int(np.asarray(c, F32).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, c)
    return F32(best[1])


def _fma(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _interpolate(data, u, v):
    """BitmapTexture::interpolate (bitmap.cpp:250-293) for an identity to_uv, bilinear / repeat, operation by operation in float32"""
    h, w = data.shape[:2]
    u, v = _fma(F32(1), u, _fma(F32(0), v, F32(0))), _fma(F32(0), u, _fma(F32(1), v, F32(0)))
    ux, uy = F32(u - np.floor(u)) * F32(w - 1), F32(v - np.floor(v)) * F32(h - 1)
    px, py = min(int(ux), w - 2), min(int(uy), h - 2)
    w1x, w1y = F32(ux - F32(px)), F32(uy - F32(py))
    w0x, w0y = F32(F32(1) - w1x), F32(F32(1) - w1y)
    out = []
    for c in range(3):
        v00, v10, v01, v11 = data[py, px, c], data[py, px + 1, c], data[py + 1, px, c], data[py + 1, px + 1, c]
        v0, v1 = _fma(w0x, v00, F32(w1x * v10)), _fma(w0x, v01, F32(w1x * v11))
        out.append(_fma(w0y, v0, F32(w1y * v1)))
    return out


def _luminance(c):
    """spectrum.h:239-241"""
    return _fma(F32(0.072169), c[2], _fma(F32(0.715160), c[1], F32(F32(0.212671) * c[0])))


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def test_bitmap_parameters_exactly():
    from mitsuba2_amd import render as R
    rng = np.random.default_rng(17)
    alpha_map = rng.uniform(0.05, 0.6, size=(3, 5, 3)).astype(F32)          # 5 x 3 texels, colour: eval_1 is the luminance
    spec_map = rng.uniform(0.1, 1.0, size=(3, 5, 3)).astype(F32)
    base = dict(type="roughconductor", distribution="ggx", **CONDUCTOR_IOR)
    bsdf = R.BSDF(plugin=dict(base, alpha={"type": "bitmap", "data": alpha_map}, specular_reflectance={"type": "bitmap", "data": spec_map}))
    nodes = np.array([[i / 4, j / 2] for j in range(3) for i in range(5)], F32)        # bilinear weights exactly 0 and 1
    n_rand = 256
    uv = np.concatenate([rng.uniform(0.0, 1.0, size=(n_rand, 2)).astype(F32), nodes])
    n = uv.shape[0]
    wi, wo = _unit(rng.normal(size=(n, 3))), _unit(rng.normal(size=(n, 3)))
    wi[: n // 2 + 64, 2] = np.abs(wi[: n // 2 + 64, 2])                    # mostly the reflecting side
    wo[: n // 2, 2] = np.abs(wo[: n // 2, 2])
    wi[n_rand:, 2], wo[n_rand:, 2] = np.abs(wi[n_rand:, 2]), np.abs(wo[n_rand:, 2])
    s = rng.uniform(size=(n, 3)).astype(F32)

    ctx = R.BSDFContext()
    si = R.SurfaceInteraction3f(t=torch.ones(n, device="cuda"), prim_index=None, shape_index=None, wi=torch.as_tensor(wi, device="cuda"),
                                uv=torch.as_tensor(uv, device="cuda"))
    value, pdf = bsdf.eval_pdf(ctx, si, torch.as_tensor(wo, device="cuda"))
    bs, weight = bsdf.sample(ctx, si, torch.as_tensor(s[:, 0], device="cuda"), torch.as_tensor(s[:, 1:3], device="cuda"))
    got = dict(eval=value, pdf=pdf, s_wo=bs.wo, s_pdf=bs.pdf, s_eta=bs.eta, s_delta=bs.delta, s_weight=weight, s_valid=bs.valid)
    got = {k: v.cpu().numpy() for k, v in got.items()}

    want = {k: [] for k in got}
    alphas = []
    for r in range(n):
        a = _luminance(_interpolate(alpha_map, uv[r, 0], uv[r, 1]))
        spec = _interpolate(spec_map, uv[r, 0], uv[r, 1])
        alphas.append(a)
        row = ob.bsdf_kat(dict(base, alpha=float(a), specular_reflectance=[float(x) for x in spec]), wi[r:r + 1], wo[r:r + 1], s[r:r + 1])
        for k in want:
            want[k].append(row[k][0])
    # the node rows read single texels: their roughness is the luminance of that texel
    for k, (j, i) in enumerate((j, i) for j in range(3) for i in range(5)):
        assert alphas[n_rand + k] == _luminance(alpha_map[0 if j == 2 else j, 0 if i == 4 else i])       # u = 1 or v = 1 wraps to texel 0
    assert np.asarray(want["s_valid"]).sum() > n // 2 and (np.asarray(want["pdf"]) > 0).sum() > n // 4
    for k in got:
        w = np.asarray(want[k])
        differing = np.nonzero(np.atleast_2d((got[k] != w).T).any(0) & ~np.atleast_2d((np.isnan(got[k].astype(F32)) & np.isnan(w.astype(F32))).T).all(0))[0]
        assert differing.size == 0, (k, "rows", differing[:8].tolist(), "node rows start at", n_rand)


# ---- 4. updates and refusals ----------------------------------------------------------------------------------------------------------
def _map_scene(texels):
    from mitsuba2_amd import scenes
    cb = scenes.cornell_box()
    box = dict(cb["meshes"][7], texcoords=np.random.default_rng(4).uniform(0, 1, size=(24, 2)).astype(F32))
    mat = dict(type="roughconductor", distribution="ggx", alpha={"type": "bitmap", "data": texels}, specular_reflectance=[0.9, 0.8, 0.7], **CONDUCTOR_IOR)
    return dict(cb, bsdfs=list(cb["bsdfs"]) + [mat], meshes=cb["meshes"][:7] + [dict(box, bsdf=len(cb["bsdfs"]))])


@pytest.mark.parametrize("via", ["host", "device"])
def test_update_texture_on_a_roughness_map(via):
    from mitsuba2_amd import render as R
    rng = np.random.default_rng(9)
    old, new = rng.uniform(0.05, 0.2, size=(4, 6, 3)).astype(F32), rng.uniform(0.2, 0.6, size=(4, 6, 3)).astype(F32)
    sp = _sensor("path")
    sensor = R.make_sensor(sp)
    scene = R.Scene(_map_scene(old))
    index = len(scene._bsdf_records) - 1
    texture = scene.texture_index(index, "alpha")
    assert texture is not None and scene.texture_index(index, "alpha_u") == texture == scene.texture_index(index, "alpha_v")
    assert scene.texture_index(index) is None and scene.texture_index(index, "specular_reflectance") is None
    integ = R.PathIntegrator(max_depth=6)
    before, _, _ = integ.sample(scene, sensor, 0, N)
    scene.update_texture(texture, new if via == "host" else torch.from_numpy(new).cuda())
    after, mask, pos = integ.sample(scene, sensor, 0, N)
    fresh, fmask, fpos = integ.sample(R.Scene(_map_scene(new)), sensor, 0, N)
    assert torch.equal(after, fresh) and torch.equal(mask, fmask) and torch.equal(pos, fpos)
    assert not torch.equal(before, after)


def test_setters_and_adjoints_refuse_textured_parameters():
    from mitsuba2_amd import render as R
    texels = np.full((2, 2, 3), 0.2, F32)
    scene = R.Scene(_map_scene(texels))
    index = len(scene._bsdf_records) - 1
    with pytest.raises(RuntimeError, match="alpha holds a texture"):
        scene.set_bsdf_param(index, 4, [0.3])
    scene.set_bsdf_param(index, 1, [0.5, 0.4, 0.3])          # the constant beside it stays settable
    import ctypes as C
    from mitsuba2_amd import _lib as L
    d = R.PathIntegrator(max_depth=3)._desc(R.make_sensor(_sensor("path")))
    n_px = d.film_width * d.film_height
    dimage, film, grad = np.zeros((n_px, 3), F32), np.zeros((n_px, 5), F32), np.zeros(12, F32)
    d.max_depth = 3
    rc = L.lib().mtsamd_render_adjoint_textures(scene._handle, C.byref(d), dimage.ctypes.data_as(C.c_void_p), film.ctypes.data_as(C.c_void_p),
                                                grad.ctypes.data_as(C.c_void_p), None)
    assert rc == -5 and b"textured BSDF parameters" in L.lib().mtsamd_last_error()
    spectral = _map_scene(texels)       # uniform eta / k, as the spectral variant needs them: the roughness map is what is refused
    spectral["bsdfs"][-1] = dict(type="roughconductor", eta=0.0, k=1.0, alpha={"type": "bitmap", "data": texels})
    with pytest.raises(RuntimeError, match=r"eval_1\(\): a bitmap / checkerboard alpha"):
        R.Scene(spectral, variant="spectral")
    spectral["bsdfs"][-1] = dict(type="conductor", eta=0.0, k=1.0, specular_reflectance={"type": "checkerboard"})
    with pytest.raises(RuntimeError, match="textured specular_reflectance is implemented for the RGB variant only"):
        R.Scene(spectral, variant="spectral")


# ---- 5. XML -------------------------------------------------------------------------------------------------------------------------------
def test_xml_scene_with_a_roughness_texture_loads_and_renders():
    from mitsuba2_amd import render as R, xml as mxml
    x = """<scene version="2.0.0">
      <sensor type="perspective"><float name="fov" value="40"/>
        <film type="hdrfilm"><integer name="width" value="32"/><integer name="height" value="32"/></film>
        <sampler type="independent"><integer name="sample_count" value="8"/></sampler></sensor>
      <shape type="rectangle"><transform name="to_world"><rotate y="1" angle="180"/><translate z="4"/></transform>
        <bsdf type="roughconductor"><spectrum name="eta" value="0"/><spectrum name="k" value="1"/>
          <texture name="alpha" type="checkerboard"><spectrum name="color0" value="0.05"/><spectrum name="color1" value="0.5"/>
            <transform name="to_uv"><scale x="4" y="4"/></transform></texture></bsdf></shape>
      <emitter type="constant"><rgb name="radiance" value="1, 0.8, 0.6"/></emitter>
      <shape type="rectangle"><emitter type="area"><rgb name="radiance" value="8,8,8"/></emitter>
        <transform name="to_world"><scale x="0.3" y="0.3"/><translate x="0.5" y="1.5" z="2"/></transform></shape></scene>"""
    scene = mxml.load_string(x)
    assert scene.texture_index(0, "alpha") == 0
    cam = scene.sensors()[0]
    assert R.PathIntegrator(max_depth=4).render(scene, cam)
    img = cam.film().bitmap().cpu().numpy()
    assert np.isfinite(img).all() and img[..., :3].max() > 0
    constant = mxml.load_string(x.replace('name="color1" value="0.5"', 'name="color1" value="0.05"'))
    cam2 = constant.sensors()[0]
    assert R.PathIntegrator(max_depth=4).render(constant, cam2)
    assert not np.array_equal(cam2.film().bitmap().cpu().numpy(), img)       # the second colour of the map is seen

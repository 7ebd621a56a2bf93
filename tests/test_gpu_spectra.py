"""Tabulated and analytic spectra (regular, irregular, d65, blackbody) as parameter values of the spectral variant, on the GPU.  The oracle
cannot evaluate a table, so every test pins the feature to something the oracle or the reference does fix: the reference's own KATs, a
float32 restatement of the cited operation sequence, constant tables against `uniform` constants (bit for bit), and 1 nm tabulations of the
upsampled colours against the oracle's srgb render (within the measured interpolation gap)."""
import ctypes as C

import numpy as np
import parity_util
import pytest

from mitsuba2_amd import scenes
from mitsuba2_amd import spectrum as S
from test_gpu_spectral import SPECTRAL_MATERIALS

pytestmark = pytest.mark.gpu
F32 = np.float32


def _eval(gpu, plugin, lam):
    import torch
    return gpu.spectrum_eval(plugin, torch.as_tensor(np.asarray(lam, F32), device="cuda")).cpu().numpy()


# ---- 1. the reference's KATs -----------------------------------------------------------------------------------------------------
REGULAR = {"type": "regular", "lambda_min": 500, "lambda_max": 600, "values": "1, 2"}                       # test_regular.py:10-16
IRREGULAR = {"type": "irregular", "wavelengths": "500, 600, 650", "values": "1, 2, .5"}                     # test_irregular.py:10-15


def test_reference_kats(gpu):
    lam = 450 + 50 * np.arange(6)
    got = _eval(gpu, REGULAR, lam[:5])
    assert np.allclose(got, [0, 1, 1.5, 2, 0], rtol=1e-5, atol=1e-8)          # test_regular.py:24-27 (ek.allclose defaults)
    assert got[0] == 0.0 and got[4] == 0.0 and got[1] == 1.0 and got[3] == 2.0  # exact 0 outside, exact node values
    got = _eval(gpu, IRREGULAR, lam)
    assert np.allclose(got, [0, 1, 1.5, 2, 0.5, 0], rtol=1e-5, atol=1e-8)     # test_irregular.py:23-26
    assert got[0] == 0.0 and got[5] == 0.0 and got[1] == 1.0 and got[3] == 2.0 and got[4] == 0.5
    assert (_eval(gpu, {"type": "blackbody", "temperature": 3000}, [359.9, 830.1, np.nan]) == 0.0).all()


# ---- 2. evaluation against a restatement ---------------------------------------------------------------------------------------------
def _fmaf(a, b, c):
    """fmaf of float32 operands: the product is exact in float64, the sum is rounded once more on the way to float32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _regular_restated(lambda_min, lambda_max, values, lam):
    """ContinuousDistribution::eval_pdf, distr_1d.h:378-393, with m_inv_interval_size of :314-344"""
    values, lam = np.asarray(values, F32), np.asarray(lam, F32)
    lo, hi = F32(lambda_min), F32(lambda_max)
    inv = F32(1.0 / ((float(hi) - float(lo)) / (values.size - 1)))
    active = (lam >= lo) & (lam <= hi)
    x = (np.where(active, lam, lo) - lo) * inv
    i = np.clip(x.astype(np.uint32), 0, values.size - 2)
    w1 = x - i.astype(F32)
    w0 = F32(1.0) - w1
    return np.where(active, _fmaf(w0, values[i], w1 * values[i + 1]), F32(0.0))


def _irregular_restated(nodes, values, lam):
    """IrregularContinuousDistribution::eval_pdf, distr_1d.h:655-677"""
    nodes, values, lam = np.asarray(nodes, F32), np.asarray(values, F32), np.asarray(lam, F32)
    active = (lam >= nodes[0]) & (lam <= nodes[-1])
    index = np.searchsorted(nodes, lam, side="left")                  # the first node that is not < lam
    index = np.maximum(np.minimum(index, nodes.size - 1), 1) - 1
    x0, x1, y0, y1 = nodes[index], nodes[index + 1], values[index], values[index + 1]
    with np.errstate(invalid="ignore"):
        t = (lam - x0) / (x1 - x0)
        return np.where(active, _fmaf(t, y1 - y0, y0), F32(0.0))


def _ulps(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), np.finfo(F32).tiny)).astype(np.float64)


def _wavelengths(extra):
    lam = np.linspace(340.0, 850.0, 4096).astype(F32)
    lam[100:100 + len(extra)] = np.asarray(extra, F32)               # each end node and an interior node: the binary search's `<` decides the side
    return lam


@pytest.mark.parametrize("case", ["regular95", "regular2", "irregular7", "irregular56"])
def test_table_evaluation_matches_the_restatement(gpu, case):
    rng = np.random.default_rng(7)
    if case == "regular95":
        lo, hi, values = 360.0, 830.0, S._cie()["d65"] * F32(1.0 / 10568.0)
        lam = _wavelengths([lo, hi, 600.0])
        got, want = _eval(gpu, {"type": "regular", "lambda_min": lo, "lambda_max": hi, "values": values}, lam), _regular_restated(lo, hi, values, lam)
    elif case == "regular2":
        lo, hi, values = 400.5, 700.25, np.array([0.2, 3.0], F32)
        lam = _wavelengths([lo, hi])
        got, want = _eval(gpu, {"type": "regular", "lambda_min": lo, "lambda_max": hi, "values": values}, lam), _regular_restated(lo, hi, values, lam)
    else:
        n = 7 if case == "irregular7" else 56
        nodes = np.cumsum(rng.uniform(0.3, 1.0, n) ** 3).astype(F32)                     # unequal gaps
        nodes = (F32(365.0) + (nodes - nodes[0]) * (F32(455.0) / (nodes[-1] - nodes[0]))).astype(F32)
        assert (np.diff(nodes) > 0).all()
        values = rng.uniform(0.0, 4.0, n).astype(F32)
        lam = _wavelengths([nodes[0], nodes[-1], nodes[n // 2], np.nextafter(nodes[n // 2], F32(0)), np.nextafter(nodes[n // 2], F32(1e3))])
        got, want = _eval(gpu, {"type": "irregular", "wavelengths": nodes, "values": values}, lam), _irregular_restated(nodes, values, lam)
        assert got[100] == values[0] and got[101] == values[-1] and got[102] == values[n // 2]      # node values at the nodes
    outside = want == 0.0
    assert (got[outside] == 0.0).all() and outside.sum() > 200
    worst = _ulps(got, want).max()
    print("%s: worst difference %.2f ulp over %d wavelengths" % (case, worst, lam.size))
    assert worst <= 1.0


@pytest.mark.parametrize("temperature", [1500.0, 3000.0, 6504.0, 10000.0])
def test_blackbody_matches_planck(gpu, temperature):
    """blackbody.cpp:46-83 against float64 Planck.  The bound: the exponent's argument a = c1 / (lambda T) carries a few float32 roundings
    (relative 2^-23 each), exp(a) turns them into a relative a * 2^-23 each, and the remaining products, the quotient and lm_exp add
    a few 2^-23 of their own: 8 * 2^-23 * (1 + a) per point."""
    lam = np.linspace(340.0, 850.0, 4096).astype(F32)
    got = _eval(gpu, {"type": "blackbody", "temperature": temperature}, lam).astype(np.float64)
    c, h, k = 2.99792458e+8, 6.62607004e-34, 1.38064852e-23
    l = lam.astype(np.float64) * 1e-9
    a = (h * c / k) / (l * temperature)
    want = np.where((lam >= 360) & (lam <= 830), 1e-9 * (2 * h * c * c) / (l ** 5 * np.expm1(a)), 0.0)
    inside = want > 0
    assert (got[~inside] == 0.0).all()
    rel = np.abs(got[inside] - want[inside]) / want[inside]
    bound = 8 * 2.0 ** -23 * (1 + a[inside])
    print("blackbody %g K: worst error / bound = %.3f" % (temperature, (rel / bound).max()))
    assert (rel <= bound).all()


# ---- 3. bit-exact plumbing against the oracle ------------------------------------------------------------------------------------------
def _const(c):
    """an irregular table that evaluates to exactly c: fmaf(t, 0, c) = c"""
    return {"type": "irregular", "wavelengths": [360.0, 500.0, 830.0], "values": [c, c, c]}


_KEYS = ("reflectance", "diffuse_reflectance", "specular_reflectance", "specular_transmittance", "eta", "k")


def _tabulated(material):
    """the plugin dictionary with every constant (`uniform`) spectral parameter replaced by a constant table"""
    out = {}
    for key, v in material.items():
        if isinstance(v, dict) and "type" in v and key not in _KEYS:
            out[key] = _tabulated(v)
        elif key in _KEYS and isinstance(v, (int, float)):
            out[key] = _const(float(v))
        else:
            out[key] = v
    return out


PLUMBING = {
    "conductor": dict(SPECTRAL_MATERIALS["conductor"]),                                                       # eta, k
    "rough_ggx": dict(SPECTRAL_MATERIALS["rough_ggx"], specular_reflectance=0.8),                             # eta, k, specular_reflectance
    "glass": dict(SPECTRAL_MATERIALS["glass"], specular_transmittance=0.9, specular_reflectance=0.7),         # both dielectric spectra
    "frosted_glass": dict(SPECTRAL_MATERIALS["frosted_glass"], specular_transmittance=0.95),
    "uniform_diffuse": dict(SPECTRAL_MATERIALS["uniform_diffuse"]),                                           # reflectance
    "plastic_uniform": dict(SPECTRAL_MATERIALS["plastic_uniform"], diffuse_reflectance=0.5, specular_reflectance=0.5),   # means exact
    "blend": {"type": "blendbsdf", "weight": 0.35, "bsdf_0": {"type": "diffuse", "reflectance": 0.4},
              "bsdf_1": {"type": "roughconductor", "alpha": 0.2, "eta": 0.2, "k": 3.9, "specular_reflectance": 0.8}},
    "twosided": {"type": "twosided", "bsdf": {"type": "plastic", "diffuse_reflectance": 0.5, "specular_reflectance": 0.5}},
}


def _scene_with(scene_name, material):
    if scene_name == "cbox":
        sd, p = scenes.cornell_box(), dict(scenes.cornell_box_sensor(48, 48, 8, seed=12), max_depth=6)
        sd["bsdfs"] = list(sd["bsdfs"]) + [material]
        sd["meshes"][6] = dict(sd["meshes"][6], bsdf=len(sd["bsdfs"]) - 1)
    else:
        sd, p = scenes.bumpy_sphere(48, 96), dict(scenes.bumpy_sphere_sensor(64, 48, 4), max_depth=6)
        sd["bsdfs"] = [material] + list(sd["bsdfs"][1:])
    return sd, p


@pytest.mark.parametrize("scene_name", ["cbox", "sphere"])
@pytest.mark.parametrize("material", sorted(PLUMBING))
def test_constant_tables_equal_uniform_constants(gpu, oracle, scene_name, material):
    path = gpu.srgb_coeff_path()
    uniform, p = _scene_with(scene_name, PLUMBING[material])
    tables, _ = _scene_with(scene_name, _tabulated(PLUMBING[material]))
    scene, sensor = gpu.Scene(tables, variant="spectral"), gpu.make_sensor(p)
    assert scene._n_spectra >= 1
    n = p["width"] * p["height"] * p["sample_count"]
    xyz, mask, pos = gpu.PathIntegrator(max_depth=6, pipeline=1).sample(scene, sensor, 0, n)
    for pipeline in (2, 0):
        other, _, _ = gpu.PathIntegrator(max_depth=6, pipeline=pipeline).sample(scene, sensor, 0, n)
        assert (xyz == other).all(), pipeline
    ref, ref_pos = oracle.OracleScene(uniform, spectral_path=path).sample_radiance(oracle.make_desc(p), 0, n)
    assert (pos.cpu().numpy() == ref_pos).all() and ((ref[:, 3] > 0.5) == mask.cpu().numpy()).all()
    parity_util.check("constant tables", xyz.cpu().numpy(), ref[:, :3])


# ---- 4. shape of the curve against the oracle --------------------------------------------------------------------------------------------
def _model(coeff, lam):
    """srgb_model_eval (include/mitsuba/render/srgb.h:8-24) in float64"""
    c0, c1, c2 = (float(x) for x in coeff)
    if np.isinf(c2):
        return np.full_like(lam, 1.0 if c2 > 0 else 0.0)
    v = (c0 * lam + c1) * lam + c2
    return np.maximum(0.0, 0.5 + 0.5 * v / np.sqrt(1.0 + v * v))


def _fetch(gpu, rgb):
    from mitsuba2_amd import _lib as L
    out = (C.c_float * 3)()
    L.check(L.lib().mtsamd_srgb_model_fetch(gpu.srgb_coeff_path().encode(), (C.c_float * 3)(*[float(x) for x in rgb]), out))
    return [float(x) for x in out]


def reflectance_curve(gpu, rgb):
    coeff = _fetch(gpu, rgb)
    return lambda lam: _model(coeff, lam)


def emitter_curve(gpu, rgb):
    """SRGBEmitterSpectrum (srgb_d65.cpp:27-63): D65 * scale / 10568 * model(rgb / scale), scale = 2 max(rgb), as scene creation computes it"""
    rgb = np.asarray(rgb, F32)
    scale = F32(max(rgb)) * F32(2.0)
    coeff = _fetch(gpu, rgb * (F32(1.0) / scale))
    d65 = (S._cie()["d65"] * (scale * F32(1.0 / 10568.0))).astype(np.float64)
    return lambda lam: np.interp(lam, 360.0 + 5.0 * np.arange(95), d65) * _model(coeff, lam)


def tabulate(curve, spacing=1.0):
    """(regular plugin over 360..830 nm, eps, spacing): eps = the largest relative gap between the table's interpolant and the curve on a
    0.01 nm grid, in float64.  The spacing starts at 1 nm (471 nodes) and is halved while eps misses 1e-4 (the bound stays)."""
    fine = np.linspace(360.0, 830.0, 47001)
    while True:
        n = int(round(470.0 / spacing)) + 1
        nodes = 360.0 + spacing * np.arange(n)
        values = curve(nodes).astype(F32)
        eps = float(np.max(np.abs(np.interp(fine, nodes, values.astype(np.float64)) - curve(fine)) / curve(fine)))
        if eps < 1e-4 or spacing <= 0.125:
            return {"type": "regular", "lambda_min": 360.0, "lambda_max": 830.0, "values": values}, eps, spacing
        spacing *= 0.5


POINT = {"type": "point", "position": [278, 400, 279], "intensity": [4e5, 3e5, 2e5]}


def _curve_case(gpu, case):
    """(scene with srgb colours, the same scene with the table in place of one of them, eps, node spacing of the table)"""
    sd = scenes.cornell_box()
    rgb_scene = dict(sd, bsdfs=list(sd["bsdfs"]), emitters=list(sd["emitters"]), meshes=list(sd["meshes"]))
    material = {"diffuse.reflectance": {"type": "diffuse", "reflectance": [0.5, 0.4, 0.3]},
                "conductor.specular_reflectance": dict(SPECTRAL_MATERIALS["conductor"]),
                "dielectric.specular_transmittance": dict(SPECTRAL_MATERIALS["glass"])}.get(case, {"type": "diffuse", "reflectance": [0.5, 0.4, 0.3]})
    rgb_scene["bsdfs"].append(material)
    rgb_scene["meshes"][6] = dict(rgb_scene["meshes"][6], bsdf=len(rgb_scene["bsdfs"]) - 1)
    if case == "point.intensity":
        rgb_scene["emitters"].append(dict(POINT))
    tab_scene = dict(rgb_scene, bsdfs=list(rgb_scene["bsdfs"]), emitters=list(rgb_scene["emitters"]))
    if case in ("area.radiance", "point.intensity"):
        e, key = (0, "radiance") if case == "area.radiance" else (1, "intensity")
        table, eps, spacing = tabulate(emitter_curve(gpu, rgb_scene["emitters"][e][key]))
        tab_scene["emitters"][e] = dict(rgb_scene["emitters"][e], **{key: table})
    else:
        key = case.split(".")[1]
        table, eps, spacing = tabulate(reflectance_curve(gpu, material[key]))
        tab_scene["bsdfs"][-1] = dict(material, **{key: table})
    return rgb_scene, tab_scene, eps, spacing


CURVE_CASES = ["diffuse.reflectance", "conductor.specular_reflectance", "dielectric.specular_transmittance", "area.radiance", "point.intensity"]


@pytest.mark.parametrize("case", CURVE_CASES)
def test_one_nm_tables_reproduce_the_upsampled_colours(gpu, oracle, case):
    """With rr_depth > max_depth no roulette decision depends on the throughput, so positions and masks equal the oracle's exactly and the
    per-sample XYZ -- a sum of non-negative terms, each with at most 6 reflectance factors and one emitter factor -- agrees within
    rtol = 4 * 6 * eps + 1e-5 (the 4 covers float32 accumulation)."""
    rgb_scene, tab_scene, eps, spacing = _curve_case(gpu, case)
    print("%s: eps = %.3e at %g nm" % (case, eps, spacing))
    assert eps < 1e-4
    p = dict(scenes.cornell_box_sensor(48, 48, 8, seed=12), max_depth=6, rr_depth=7)
    n = 48 * 48 * 8
    scene, sensor = gpu.Scene(tab_scene, variant="spectral"), gpu.make_sensor(p)
    assert scene._n_spectra == 1
    xyz, mask, pos = gpu.PathIntegrator(max_depth=6, rr_depth=7).sample(scene, sensor, 0, n)
    ref, ref_pos = oracle.OracleScene(rgb_scene, spectral_path=gpu.srgb_coeff_path()).sample_radiance(oracle.make_desc(p), 0, n)
    assert (pos.cpu().numpy() == ref_pos).all() and ((ref[:, 3] > 0.5) == mask.cpu().numpy()).all()
    got, want = xyz.cpu().numpy().astype(np.float64), ref[:, :3].astype(np.float64)
    rtol = 4 * 6 * eps + 1e-5
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    rel[(got == 0) & (want == 0)] = 0.0
    print("%s: worst relative difference %.3e (rtol %.3e), %d of %d samples non-zero" % (case, rel.max(), rtol, (want.max(1) > 0).sum(), n))
    assert (rel <= rtol).all()


# ---- 5. wavelength-dependent eta / k -----------------------------------------------------------------------------------------------------
# gold, n and k after Johnson and Christy (Phys. Rev. B 6, 4370, 1972), rounded: k is low in the blue, where gold absorbs
GOLD_NM = [360.0, 400.0, 450.0, 500.0, 550.0, 600.0, 650.0, 700.0, 750.0, 830.0]
GOLD_N = [1.66, 1.47, 1.38, 0.97, 0.43, 0.25, 0.17, 0.16, 0.15, 0.16]
GOLD_K = [1.96, 1.95, 1.92, 1.87, 2.46, 2.98, 3.45, 3.95, 4.45, 5.08]


def test_gold_like_conductor(gpu):
    gold = {"type": "roughconductor", "alpha": 0.2, "distribution": "ggx",
            "eta": {"type": "spectrum", "value": list(zip(GOLD_NM, GOLD_N))}, "k": {"type": "spectrum", "value": list(zip(GOLD_NM, GOLD_K))}}
    sd = scenes.bumpy_sphere(48, 96)
    sd["bsdfs"] = [gold] + list(sd["bsdfs"][1:])
    p = scenes.bumpy_sphere_sensor(64, 48, 64)
    out = {}
    for variant in ("rgb", "spectral"):
        scene, sensor = gpu.Scene(sd, variant=variant), gpu.make_sensor(p)
        assert scene._n_spectra == (2 if variant == "spectral" else 0)
        assert gpu.PathIntegrator().render(scene, sensor)
        out[variant] = sensor.film().bitmap().cpu().numpy()[..., :3]
    r, g, b = out["spectral"].reshape(-1, 3).mean(0)
    print("gold: spectral mean rgb %s, rgb-variant mean rgb %s" % ([r, g, b], out["rgb"].reshape(-1, 3).mean(0).tolist()))
    assert r > g > b
    assert abs(out["spectral"].mean() - out["rgb"].mean()) / out["rgb"].mean() < 0.1


# ---- 6. refusals and unchanged behaviour ---------------------------------------------------------------------------------------------------
def _tabulated_box():
    sd = scenes.cornell_box()
    sd["bsdfs"] = list(sd["bsdfs"]) + [{"type": "conductor", "id": "metal", "eta": _const(0.2), "k": _const(3.9), "specular_reflectance": [0.9, 0.7, 0.3]},
                                       {"type": "diffuse", "id": "tab", "reflectance": {"type": "regular", "lambda_min": 360, "lambda_max": 830, "values": [0.2, 0.6]}}]
    sd["meshes"][6] = dict(sd["meshes"][6], bsdf=len(sd["bsdfs"]) - 2)
    sd["meshes"][7] = dict(sd["meshes"][7], bsdf=len(sd["bsdfs"]) - 1)
    sd["emitters"] = [dict(sd["emitters"][0], radiance={"type": "d65", "scale": 15.0})]
    return sd


def test_setters_and_replay_refuse_spectra(gpu):
    from mitsuba2_amd import autodiff
    sd = _tabulated_box()
    scene = gpu.Scene(sd, variant="spectral")
    metal, tab = len(sd["bsdfs"]) - 2, len(sd["bsdfs"]) - 1
    with pytest.raises(RuntimeError, match="tabulated spectrum"):
        scene.set_bsdf_reflectance(tab, [0.5, 0.5, 0.5])
    with pytest.raises(RuntimeError, match="tabulated spectrum"):
        scene.set_bsdf_param(tab, 0, [0.5, 0.5, 0.5])
    with pytest.raises(RuntimeError, match="tabulated spectrum"):
        scene.set_bsdf_param(metal, 2, [0.3, 0.3, 0.3])
    with pytest.raises(RuntimeError, match="tabulated spectrum"):
        scene.set_bsdf_param(metal, 3, [3.0, 3.0, 3.0])
    with pytest.raises(RuntimeError, match="tabulated spectrum"):
        scene.set_emitter_radiance(0, [1.0, 1.0, 1.0])
    scene.set_bsdf_param(metal, 1, [0.8, 0.6, 0.2])                 # the srgb colour beside them stays settable
    scene.set_bsdf_reflectance(0, [0.5, 0.5, 0.5])
    with pytest.raises(RuntimeError, match="tabulated spectra"):
        autodiff.traverse(scene, replay=True)
    keys = set(autodiff.traverse(scene).keys())
    assert "metal.specular_reflectance.value" in keys and "bsdf_0.reflectance.value" in keys
    assert not any(k.startswith("tab.") or k in ("metal.eta.value", "metal.k.value") for k in keys)
    with pytest.raises(RuntimeError, match="[Nn]ot implemented for non-spectral"):
        sd2 = scenes.cornell_box()
        sd2["emitters"] = list(sd2["emitters"]) + [{"type": "point", "position": [278, 400, 279], "intensity": {"type": "blackbody", "temperature": 3000}}]
        gpu.Scene(sd2, variant="rgb")


@pytest.mark.parametrize("form", ["plugin", "loaded", "table_bsdf"])
def test_traverse_in_a_diffuse_scene_with_spectra(gpu, form):
    """the plain Cornell box (diffuse BSDFs, one area light: the scene class whose traverse() lists the light's radiance) with a spectrum on
    the light -- given as a plugin, or as a loaded XML scene carries it: beside the pre-integrated colour -- or on one reflectance: no key
    for the parameter that holds the spectrum, the others are listed and can still be updated; the RGB variant keeps the light's key"""
    import torch
    from mitsuba2_amd import autodiff
    sd = scenes.cornell_box()
    for i, m in enumerate(sd["meshes"]):
        m["id"] = "shape_%d" % i
    lamp = "shape_%d.emitter.radiance.value" % next(i for i, m in enumerate(sd["meshes"]) if m.get("emitter", -1) == 0)
    if form == "plugin":
        sd["emitters"] = [dict(sd["emitters"][0], radiance={"type": "d65", "scale": 15.0})]
    elif form == "loaded":
        pairs = [(400.0, 0.0), (500.0, 8.0), (600.0, 15.6), (700.0, 18.4)]
        sd["emitters"] = [dict(sd["emitters"][0], radiance=S.tabulated_to_rgb([p[0] for p in pairs], [p[1] for p in pairs], True, "radiance"),
                               spectra={"radiance": {"type": "spectrum", "value": pairs}})]
    else:
        sd["bsdfs"][1] = {"type": "diffuse", "reflectance": {"type": "regular", "lambda_min": 360, "lambda_max": 830, "values": [0.2, 0.6]}}
    scene = gpu.Scene(sd, variant="spectral")
    assert scene._n_spectra == 1
    params = autodiff.traverse(scene)
    keys = set(params.keys())
    if form == "table_bsdf":
        assert lamp in keys and "bsdf_1.reflectance.value" not in keys
    else:
        assert lamp not in keys and "bsdf_1.reflectance.value" in keys
    assert "bsdf_0.reflectance.value" in keys
    sensor = gpu.make_sensor(dict(scenes.cornell_box_sensor(16, 16, 4), max_depth=4))
    before, _, _ = gpu.PathIntegrator(max_depth=4).sample(scene, sensor, 0, 16 * 16 * 4)
    params["bsdf_0.reflectance.value"] = torch.tensor([0.2, 0.3, 0.9])
    if lamp in keys:
        params[lamp] = torch.tensor([5.0, 5.0, 5.0])
    params.update()                                               # every key that is offered can be pushed
    after, _, _ = gpu.PathIntegrator(max_depth=4).sample(scene, sensor, 0, 16 * 16 * 4)
    assert not (before == after).all()
    rgb = autodiff.traverse(gpu.Scene(sd, variant="rgb"))       # RGB variant: the pre-integrated colours, every key as before
    assert lamp in rgb.keys() and "bsdf_1.reflectance.value" in rgb.keys() and rgb[lamp].shape == (3,)
    rgb[lamp] = torch.tensor([5.0, 5.0, 5.0])
    rgb.update()


def test_adjoint_entry_points_refuse_spectra(gpu):
    import torch
    from mitsuba2_amd import _lib as L
    scene, sensor = gpu.Scene(_tabulated_box(), variant="spectral"), gpu.make_sensor(dict(scenes.cornell_box_sensor(16, 16, 2), max_depth=4))
    d = gpu.PathIntegrator(max_depth=4)._desc(sensor)
    dimage, film, grad = torch.ones(16 * 16 * 3, device="cuda"), torch.ones(16 * 16 * 5, device="cuda"), torch.zeros(64 * 3, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for fn in (L.lib().mtsamd_render_adjoint_spectral, L.lib().mtsamd_render_adjoint_spectral_emitters):
        assert fn(scene._handle, C.byref(d), ptr(dimage), ptr(film), ptr(grad), None, None) == -5
        assert b"tabulated spectra" in L.lib().mtsamd_last_error()


def test_rgb_variant_renders_the_pre_integrated_colour(gpu):
    sd = _tabulated_box()
    plain = _tabulated_box()
    for rec, ref in zip(sd["bsdfs"][-2:], plain["bsdfs"][-2:]):
        for key in ("eta", "k", "reflectance"):
            if isinstance(rec.get(key), dict):
                ref[key] = S.to_rgb(S.parse(rec[key]), False, key)
    plain["emitters"] = [dict(plain["emitters"][0], radiance=S.to_rgb(S.parse(sd["emitters"][0]["radiance"], within_emitter=True), True, "radiance"))]
    p = scenes.cornell_box_sensor(32, 32, 4, seed=3)
    films = []
    for desc in (sd, plain):
        scene, sensor = gpu.Scene(desc, variant="rgb"), gpu.make_sensor(p)
        assert scene._n_spectra == 0
        rgb, _, _ = gpu.PathIntegrator().sample(scene, sensor, 0, 32 * 32 * 4)
        films.append(rgb.cpu().numpy())
    assert (films[0] == films[1]).all() and films[0].max() > 0


def test_zero_spectra_is_scene_create(gpu, monkeypatch):
    """a scene without spectra gives the same samples through mtsamd_scene_create_with_spectra(..., 0 spectra) as through mtsamd_scene_create"""
    from mitsuba2_amd import _lib as L
    sd, p = _scene_with("cbox", SPECTRAL_MATERIALS["conductor"])
    sensor = gpu.make_sensor(p)
    a, _, _ = gpu.PathIntegrator(max_depth=6).sample(gpu.Scene(sd, variant="spectral"), sensor, 0, 48 * 48 * 8)
    lib = L.lib()
    calls = []

    class Via:
        def __getattr__(self, name):
            if name == "mtsamd_scene_create":
                def create(desc, device, out):
                    calls.append(1)
                    return lib.mtsamd_scene_create_with_spectra(desc, None, 0, None, 0, device, out)
                return create
            return getattr(lib, name)
    monkeypatch.setattr(L, "lib", lambda: Via())
    b, _, _ = gpu.PathIntegrator(max_depth=6).sample(gpu.Scene(sd, variant="spectral"), sensor, 0, 48 * 48 * 8)
    assert calls == [1] and (a == b).all()

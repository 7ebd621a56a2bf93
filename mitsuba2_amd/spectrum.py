"""Tabulated spectra on the host: what the reference's XML loader does with `<spectrum value="400:0.3, 500:0.7, ..."/>` or
`<spectrum filename=.../>` in the RGB variants -- pre-integration against the CIE 1931 observer and conversion to linear sRGB
(``src/libcore/xml.cpp:1084-1146``, ``src/libcore/spectrum.cpp:9-86``, ``include/mitsuba/core/spectrum.h:127-237``)."""
import os
import re

import numpy as np

F32 = np.float32
MTS_WAVELENGTH_MIN, MTS_WAVELENGTH_MAX = F32(360.0), F32(830.0)
MTS_CIE_Y_NORMALIZATION = F32(1.0 / 106.7502593994140625)          # spectrum.h:133

_tables = None


def _cie():
    """the CIE 1931 tables shipped with the HIP sources (csrc/cie_data.h: generated data)"""
    global _tables
    if _tables is None:
        text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "cie_data.h")).read()
        out = {}
        for key in ("x", "y", "z", "d65"):
            body = re.search(r"kCie_%s\[95\]\s*=\s*\{(.*?)\};" % key, text, re.S).group(1)
            out[key] = np.array([float(v) for v in re.findall(r"[-+]?\d*\.\d+(?:[eE][-+]?\d+)?", body)], dtype=F32)
            assert out[key].size == 95
        _tables = out
    return _tables


def cie1931_xyz(wavelength):
    """spectrum.h:150-176: linear interpolation in the 95-sample table, 0 outside [360, 830] nm"""
    t = _cie()
    w = np.asarray(wavelength, dtype=F32)
    tt = (w - F32(360.0)) * F32(94.0 / 470.0)
    i0 = np.clip(tt.astype(np.int32), 0, 93)
    w1 = tt - i0.astype(F32)
    w0 = F32(1.0) - w1
    ok = (w >= F32(360.0)) & (w <= F32(830.0))
    return np.stack([np.where(ok, w0 * t[k][i0] + w1 * t[k][i0 + 1], F32(0)) for k in "xyz"], axis=-1).astype(F32)


def xyz_to_srgb(xyz):
    m = np.array([[3.240479, -1.537150, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]], dtype=F32)
    return (np.asarray(xyz, dtype=F32) @ m.T).astype(F32)


def spectrum_to_rgb(wavelengths, values, bounded=True):
    """spectrum.cpp:41-86: Riemann sum over 1000 steps of the piecewise-linear spectrum times the colour matching functions"""
    wl, val = np.asarray(wavelengths, dtype=F32), np.asarray(values, dtype=F32)
    if wl.size < 2 or wl.size != val.size:
        raise RuntimeError("spectrum: at least two wavelength:value pairs are required")
    if (np.diff(wl) < 0).any():
        raise RuntimeError("Wavelengths must be specified in increasing order!")
    steps = 1000
    x = MTS_WAVELENGTH_MIN + (np.arange(steps, dtype=F32) / F32(steps - 1)) * (MTS_WAVELENGTH_MAX - MTS_WAVELENGTH_MIN)
    keep = (x >= wl[0]) & (x <= wl[-1])
    x = x[keep]
    idx = np.clip(np.searchsorted(wl, x, side="right") - 1, 0, wl.size - 2)       # math::find_interval
    x0, x1, y0, y1 = wl[idx], wl[idx + 1], val[idx], val[idx + 1]
    y = (x * y0 - x1 * y0 - x * y1 + x0 * y1) / (x0 - x1)
    color = (cie1931_xyz(x) * y[:, None]).sum(axis=0, dtype=F32)
    color = color * ((MTS_WAVELENGTH_MAX - MTS_WAVELENGTH_MIN) / F32(steps))
    color = xyz_to_srgb(color)
    if bounded:
        color = np.clip(color, 0.0, 1.0)
    else:
        color = np.maximum(color, 0.0)
    return [float(c) for c in color]


def spectrum_from_file(path):
    """spectrum.cpp:9-38: `wavelength value` per line, '#' comments"""
    if not os.path.exists(path):
        raise RuntimeError('"%s": file does not exist!' % path)
    wl, val = [], []
    for line in open(path):
        line = line.strip()
        if not line or line[0] == "#":
            continue
        tok = line.split()
        if len(tok) != 2:
            raise RuntimeError('"%s": excess tokens after wavlengths-value pair in file:\n%s!' % (path, line))
        wl.append(float(tok[0])); val.append(float(tok[1]))
    return wl, val


def tabulated_to_rgb(wavelengths, values, within_emitter, name):
    """create_texture_from_spectrum, non-spectral branch (xml.cpp:1084-1140)"""
    unbounded = name in ("eta", "k", "int_ior", "ext_ior")                           # is_unbounded_spectrum (xml.cpp:83-85)
    scaled = [float(F32(v) * MTS_CIE_Y_NORMALIZATION) for v in values]
    return spectrum_to_rgb(wavelengths, scaled, bounded=not (within_emitter or unbounded))


# --------------------------------------------------------------------------------------------
# Spectrum plugins as parameter values of the spectral variant (src/spectra/regular.cpp, irregular.cpp, d65.cpp, blackbody.cpp).
# A parsed spectrum is dict(kind="regular", lambda_min, lambda_max, values) | dict(kind="irregular", wavelengths, values) |
# dict(kind="blackbody", temperature); `values` / `wavelengths` are float32 arrays.
PLUGINS = ("regular", "irregular", "d65", "blackbody", "spectrum")


def is_spectrum(v):
    """a parameter value that names a spectrum plugin (or the `spectrum` form of load_dict)"""
    return isinstance(v, dict) and v.get("type") in PLUGINS


def _floats(v, what):
    """a sequence, or the reference's comma / space separated string (string::tokenize(..., " ,"), regular.cpp:32-44)"""
    if isinstance(v, str):
        out = []
        for tok in re.split(r"[ ,]+", v.strip()):
            if not tok:
                continue
            try:
                out.append(float(tok))
            except ValueError:
                raise RuntimeError("Could not parse floating point value '%s'" % tok)
        return np.array(out, dtype=F32)
    if v is None:
        raise RuntimeError('Property "%s" has not been specified!' % what)
    return np.asarray(v, dtype=F32).reshape(-1).copy()


def _check_regular(lambda_min, lambda_max, values):
    """ContinuousDistribution::update (distr_1d.h:293-345)"""
    if values.size < 2:
        raise RuntimeError("ContinuousDistribution: needs at least two entries!")
    if not lambda_min < lambda_max:
        raise RuntimeError("ContinuousDistribution: invalid range!")
    if (values < 0).any():
        raise RuntimeError("ContinuousDistribution: entries must be non-negative!")
    return dict(kind="regular", lambda_min=float(F32(lambda_min)), lambda_max=float(F32(lambda_max)), values=values)


def _check_irregular(wavelengths, values):
    """IrregularContinuousDistribution::update (distr_1d.h:561-622)"""
    if wavelengths.size != values.size:
        raise RuntimeError("IrregularContinuousDistribution: 'pdf' and 'nodes' size mismatch!")
    if values.size < 2:
        raise RuntimeError("IrregularContinuousDistribution: needs at least two entries!")
    if not (np.diff(wavelengths) > 0).all():
        raise RuntimeError("IrregularContinuousDistribution: node positions must be strictly increasing!")
    if (values < 0).any():
        raise RuntimeError("IrregularContinuousDistribution: entries must be non-negative!")
    return dict(kind="irregular", wavelengths=wavelengths, values=values)


def from_pairs(wavelengths, values, within_emitter):
    """create_texture_from_spectrum, spectral branch (xml.cpp:1084-1125): wavelength:value pairs become a `regular` spectrum if all gaps
    equal the first within math::Epsilon<float>, an `irregular` one otherwise; inside emitters the values are scaled by
    MTS_CIE_Y_NORMALIZATION"""
    wl, val = np.asarray(wavelengths, dtype=F32).reshape(-1), np.asarray(values, dtype=F32).reshape(-1).copy()
    if wl.size != val.size or wl.size == 0:
        raise RuntimeError("spectrum: expected wavelength:value pairs")
    if within_emitter:
        val = val * MTS_CIE_Y_NORMALIZATION
    gaps = np.diff(wl)
    if (gaps < 0).any():
        raise RuntimeError("Wavelengths must be specified in increasing order!")
    eps = F32(np.finfo(F32).eps / 2)                 # math::Epsilon<float> (math.h: half the machine epsilon)
    if gaps.size == 0 or (np.abs(gaps[1:] - gaps[0]) <= eps).all():
        return _check_regular(wl[0], wl[-1], val)
    return _check_irregular(wl.copy(), val)


def parse(v, within_emitter=False, base_dir="."):
    """spectrum plugin dictionary -> parsed spectrum (the constructors of regular.cpp:21-57, irregular.cpp:21-66, d65.cpp:44-66,
    blackbody.cpp:54-57; `spectrum`: the value / filename forms of load_dict and of `<spectrum value="l:v, ..."/>`)"""
    t = v.get("type")
    known = {"type", "id"}
    if t == "regular":
        known |= {"lambda_min", "lambda_max", "values", "size"}
        for key in ("lambda_min", "lambda_max"):
            if key not in v:
                raise RuntimeError('Property "%s" has not been specified!' % key)
        out = _check_regular(F32(v["lambda_min"]), F32(v["lambda_max"]), _floats(v.get("values"), "values"))
    elif t == "irregular":
        known |= {"wavelengths", "values", "size"}
        out = _check_irregular(_floats(v.get("wavelengths"), "wavelengths"), _floats(v.get("values"), "values"))
    elif t == "d65":                                   # d65.cpp:44-66: expands into `regular`
        known |= {"scale"}
        scale = F32(v.get("scale", 1.0)) * F32(F32(1.0) / F32(10568.0))
        out = _check_regular(F32(360.0), F32(830.0), (_cie()["d65"] * scale).astype(F32))
    elif t == "blackbody":
        known |= {"temperature"}
        if "temperature" not in v:
            raise RuntimeError('Property "temperature" has not been specified!')
        out = dict(kind="blackbody", temperature=float(v["temperature"]))
    elif t == "spectrum":
        known |= {"value", "filename"}
        if "filename" in v:
            fn = v["filename"]
            wl, val = spectrum_from_file(fn if os.path.isabs(fn) else os.path.join(base_dir, fn))
        else:
            pairs = v.get("value")
            if isinstance(pairs, str):
                try:
                    pairs = [tuple(float(x) for x in tok.split(":")) for tok in re.split(r"[ ,]+", pairs.strip()) if tok]
                except ValueError:
                    raise RuntimeError('could not parse wavelength:value pairs: "%s"' % v.get("value"))
            a = np.asarray(pairs, dtype=F32)
            if a.ndim != 2 or a.shape[1] != 2:
                raise RuntimeError("spectrum: expected wavelength:value pairs")
            wl, val = a[:, 0], a[:, 1]
        out = from_pairs(wl, val, within_emitter)
    else:
        raise RuntimeError("Spectrum plugin '%s' is not supported by this backend (%s)" % (t, ", ".join(PLUGINS)))
    extra = [k for k in v if k not in known]
    if extra:
        raise RuntimeError('Error while loading: unreferenced property "%s" in spectrum plugin of type "%s"' % (extra[0], t))
    return out


def nodes(spec):
    """(wavelengths, values) of a parsed regular / irregular spectrum"""
    if spec["kind"] == "regular":
        n = spec["values"].size
        wl = (np.float64(spec["lambda_min"]) + np.arange(n) * ((np.float64(spec["lambda_max"]) - np.float64(spec["lambda_min"])) / (n - 1))).astype(F32)
        return wl, spec["values"]
    return spec["wavelengths"], spec["values"]


def to_rgb(spec, within_emitter, name):
    """what an RGB-variant scene uses for a parsed spectrum: `regular` / `irregular` are pre-integrated against the CIE observer as the
    loader pre-integrates wavelength:value pairs (xml.cpp:1126-1143).  An emitter spectrum already carries MTS_CIE_Y_NORMALIZATION
    (from_pairs; `d65` has its own 1 / 10568), any other gets it here, so that both variants see the same pairs the same way.
    `blackbody` raises as the reference does (blackbody.cpp:84-89)"""
    if spec["kind"] == "blackbody":
        raise RuntimeError("blackbody: Not implemented for non-spectral modes")
    wl, val = nodes(spec)
    if not within_emitter:
        val = val * MTS_CIE_Y_NORMALIZATION
    unbounded = name in ("eta", "k", "int_ior", "ext_ior")
    return spectrum_to_rgb(wl, val, bounded=not (within_emitter or unbounded))

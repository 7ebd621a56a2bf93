"""Host-side mirror of the reference's Python surface for the path-tracing hot path.

Class and method names follow the pybind11 bindings of Mitsuba 2 (``src/librender/python/scene_v.cpp:37-86``,
``integrator_v.cpp:61-170``, ``imageblock_v.cpp:5-40``, ``src/films/hdrfilm.cpp``) for the supported subset;
every compute call goes through the C ABI of ``libmtsamd.so`` (``include/mtsamd.h``).  PyTorch is used only
to own device memory and streams.
"""
import ctypes as C
import enum
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import _lib as L

RayEpsilon = float(np.float32(np.finfo(np.float32).eps / 2 * 1500))
ShadowEpsilon = float(np.float32(RayEpsilon) * np.float32(10))      # math.h:38: ShadowEpsilon = RayEpsilon * 10


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _dot3(a, b):
    """dot product of (N,3) tensors in the kernels' order of operations: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))"""
    return torch.addcmul(torch.addcmul(a[:, 0] * b[:, 0], a[:, 1], b[:, 1]), a[:, 2], b[:, 2])


def _planes(t, k, dev):
    """(N, k) values -> contiguous (k, N) float32 planes on `dev`, the layout of the operator entry points"""
    return torch.as_tensor(t, dtype=torch.float32, device=dev).reshape(-1, k).t().contiguous()


def _mask(active, dev):
    """`active` argument of an operator -> byte mask tensor, or None for all lanes"""
    if active is None or active is True:
        return None
    return torch.as_tensor(active, device=dev).reshape(-1).to(torch.uint8).contiguous()


# --------------------------------------------------------------------------------------------
# records (include/mitsuba/core/ray.h:21-62, include/mitsuba/render/interaction.h:33-126)
@dataclass
class Ray3f:
    o: torch.Tensor                     # (N,3)
    d: torch.Tensor                     # (N,3)
    mint: Optional[torch.Tensor] = None  # (N,), default RayEpsilon (ray.h:33)
    maxt: Optional[torch.Tensor] = None  # (N,), default +inf (ray.h:34)
    time: float = 0.0

    def __post_init__(self):
        n = self.o.shape[0]
        dev = self.o.device
        if self.mint is None:
            self.mint = torch.full((n,), RayEpsilon, dtype=torch.float32, device=dev)
        if self.maxt is None:
            self.maxt = torch.full((n,), float("inf"), dtype=torch.float32, device=dev)


@dataclass
class SurfaceInteraction3f:
    t: torch.Tensor
    prim_index: torch.Tensor
    shape_index: torch.Tensor
    p: Optional[torch.Tensor] = None
    n: Optional[torch.Tensor] = None
    uv: Optional[torch.Tensor] = None
    sh_frame_s: Optional[torch.Tensor] = None
    sh_frame_t: Optional[torch.Tensor] = None
    sh_frame_n: Optional[torch.Tensor] = None
    dp_du: Optional[torch.Tensor] = None
    dp_dv: Optional[torch.Tensor] = None
    wi: Optional[torch.Tensor] = None
    prim_uv: Optional[torch.Tensor] = None   # barycentric (u,v): the kd-tree "cache" (kdtree.h:2432-2452)
    # what Scene.ray_intersect remembers for the operator API: the scene (si.bsdf(), si.emitter()) and the direction tensor of the rays
    # (Emitter.eval on an escaped lane); the planes of a missed lane stay as they are
    _scene: Optional[object] = field(default=None, repr=False, compare=False)
    _ray_d: Optional[torch.Tensor] = field(default=None, repr=False, compare=False)

    def is_valid(self):
        """interaction.h:53-55"""
        return self.t != float("inf")

    def bsdf(self, ray=None):
        """SurfaceInteraction::bsdf (interaction.h:200-203): the BSDF of every lane's shape, as one per-lane handle.  `ray` is accepted
        and unused (no BSDF of this backend needs ray differentials)."""
        if self._scene is None:
            raise RuntimeError("SurfaceInteraction3f.bsdf(): the interaction was not made by Scene.ray_intersect (no shapes to look up)")
        return BSDF(scene=self._scene, lanes=self.shape_index)

    def emitter(self, scene, active=True):
        """SurfaceInteraction::emitter (interaction.h:161,225-231): the emitter of the shape on valid lanes, the scene's environment
        emitter on the others (none: every query on that lane gives 0)."""
        tables = scene._operator_tables()
        dev = self.shape_index.device
        shape = self.shape_index.to(torch.int64)
        valid = (shape >= 0) & (shape < scene.shape_count())
        per_shape = tables["emitter"].to(dev)[shape.clamp(0, max(scene.shape_count() - 1, 0))]
        index = torch.where(valid, per_shape, torch.full_like(per_shape, scene._environment))
        if active is not True and active is not None:
            index = torch.where(torch.as_tensor(active, device=dev).bool().reshape(-1), index, torch.full_like(index, -1))
        return Emitter(scene, lanes=index.to(torch.int32))

    def to_local(self, v):
        """Frame3f::to_local of the shading frame (frame.h:30-32)"""
        return torch.stack([_dot3(v, self.sh_frame_s), _dot3(v, self.sh_frame_t), _dot3(v, self.sh_frame_n)], dim=1)

    def to_world(self, v):
        """Frame3f::to_world of the shading frame (frame.h:35-37)"""
        return (self.sh_frame_s * v[:, 0:1] + self.sh_frame_t * v[:, 1:2]) + self.sh_frame_n * v[:, 2:3]

    def spawn_ray(self, d):
        """Interaction::spawn_ray (interaction.h:58-61): mint = RayEpsilon * (1 + max |p|), maxt = inf"""
        mint = (1.0 + self.p.abs().amax(dim=1)) * RayEpsilon
        return Ray3f(o=self.p, d=d, mint=mint, maxt=torch.full_like(mint, float("inf")))

    def spawn_ray_to(self, t):
        """Interaction::spawn_ray_to (interaction.h:64-69): the segment to point `t`, shortened by ShadowEpsilon at its far end"""
        d = t - self.p
        dist = _dot3(d, d).sqrt()
        d = d * (1.0 / dist).unsqueeze(1)
        return Ray3f(o=self.p, d=d, mint=(1.0 + self.p.abs().amax(dim=1)) * RayEpsilon, maxt=dist * (1.0 - ShadowEpsilon))


# --------------------------------------------------------------------------------------------
class ReconstructionFilter:
    """include/mitsuba/core/rfilter.h; discretisation from src/libcore/rfilter.cpp:9-20 via the C ABI."""
    kind = -1

    def __init__(self, param=0.0, param2=0.0):
        self.param, self.param2 = float(param), float(param2)
        table = (C.c_float * 32)()
        radius = C.c_float()
        border = C.c_int32()
        L.check(L.lib().mtsamd_rfilter_info(self.kind, self.param, self.param2, table, C.byref(radius), C.byref(border)))
        self._table = np.array(table, dtype=np.float32)
        self._radius = radius.value
        self._border = border.value

    def radius(self):
        return self._radius

    def border_size(self):
        return self._border

    def eval_discretized(self, x):
        idx = min(int(abs(np.float32(x) * np.float32(31.0 / self._radius))), 31)
        return float(self._table[idx])


class GaussianFilter(ReconstructionFilter):
    """src/rfilters/gaussian.cpp"""
    kind = 0

    def __init__(self, stddev=0.5):
        super().__init__(stddev)


class BoxFilter(ReconstructionFilter):
    """src/rfilters/box.cpp"""
    kind = 1

    def __init__(self, radius=0.5):
        super().__init__(radius)


class TentFilter(ReconstructionFilter):
    """src/rfilters/tent.cpp (radius 1: ImageBlock::put treats it like a one-pixel footprint, imageblock.cpp:117)"""
    kind = 2


class CatmullRomFilter(ReconstructionFilter):
    """src/rfilters/catmullrom.cpp"""
    kind = 3


class MitchellFilter(ReconstructionFilter):
    """src/rfilters/mitchell.cpp"""
    kind = 4

    def __init__(self, B=1.0 / 3.0, C=1.0 / 3.0):
        super().__init__(B, C)


class LanczosFilter(ReconstructionFilter):
    """src/rfilters/lanczos.cpp"""
    kind = 5

    def __init__(self, lobes=3):
        super().__init__(int(lobes))


def make_filter(name, *params):
    """reconstruction filter plugin by name: gaussian(stddev) | box(radius) | tent | catmullrom | mitchell(B, C) | lanczos(lobes)"""
    classes = {"gaussian": GaussianFilter, "box": BoxFilter, "tent": TentFilter, "catmullrom": CatmullRomFilter,
               "mitchell": MitchellFilter, "lanczos": LanczosFilter}
    if name not in classes:
        raise RuntimeError('Reconstruction filter "%s" is not supported by this backend (%s)' % (name, ", ".join(classes)))
    return classes[name](*params)


class ImageBlock:
    """src/librender/imageblock.cpp.  ``data()`` is a (H+2b, W+2b, C) float32 CUDA tensor."""

    def __init__(self, size, channel_count, filter=None, warn_negative=True, warn_invalid=True, border=True,
                 normalize=False, device="cuda"):
        if normalize:
            raise RuntimeError("ImageBlock: normalize=True is not supported by this backend")
        self._size = (int(size[0]), int(size[1]))
        self._offset = (0, 0)
        self._channels = int(channel_count)
        self._filter = filter
        self._border = filter.border_size() if (filter is not None and border) else 0
        self._device = torch.device(device)
        self._data = torch.zeros((self._size[1] + 2 * self._border, self._size[0] + 2 * self._border, self._channels),
                                 dtype=torch.float32, device=self._device)

    def size(self): return self._size
    def width(self): return self._size[0]
    def height(self): return self._size[1]
    def offset(self): return self._offset
    def set_offset(self, o): self._offset = (int(o[0]), int(o[1]))
    def channel_count(self): return self._channels
    def border_size(self): return self._border
    def data(self): return self._data
    def clear(self): self._data.zero_()

    def put(self, pos, values=None, active=None):
        """put(block) or put(pos, values): imageblock.cpp:49-77 / :80-172."""
        lib = L.lib()
        if isinstance(pos, ImageBlock):
            src = pos
            if src.channel_count() != self.channel_count():
                raise RuntimeError("ImageBlock::put(): mismatched channel counts!")
            L.check(lib.mtsamd_imageblock_put_block(_ptr(src._data), src._size[0], src._size[1], src._offset[0], src._offset[1],
                                                    src._border, _ptr(self._data), self._size[0], self._size[1], self._offset[0],
                                                    self._offset[1], self._border, self._channels, _stream()))
            return
        if self._filter is None:
            raise RuntimeError("ImageBlock::put(): a reconstruction filter is required")
        pos = torch.as_tensor(pos, dtype=torch.float32, device=self._device).reshape(-1, 2).contiguous()
        values = torch.as_tensor(values, dtype=torch.float32, device=self._device).reshape(-1, self._channels).contiguous()
        if active is not None:
            keep = torch.as_tensor(active, device=self._device).bool().reshape(-1)
            pos, values = pos[keep].contiguous(), values[keep].contiguous()
        f = self._filter
        L.check(lib.mtsamd_imageblock_put(self._size[0], self._size[1], self._offset[0], self._offset[1], self._channels, f.kind,
                                          f.param, f.param2, 0, self._border, pos.shape[0], _ptr(pos), _ptr(values), _ptr(self._data),
                                          _stream()))


# --------------------------------------------------------------------------------------------
class IndependentSampler:
    """src/samplers/independent.cpp (sample_count default 4, seed 0: src/librender/sampler.cpp:7-8)"""

    def __init__(self, sample_count=4, seed=0):
        self._sample_count = int(sample_count)
        self._seed = int(seed)

    def sample_count(self): return self._sample_count
    def seed_value(self): return self._seed

    # -- the wavefront sampler of a Python integrator (independent.cpp:61-94): one PCG32 stream per lane, on the device
    def seed(self, seed_value, size, first=0, device="cuda"):
        """Sampler::seed(seed_value, size): lane i becomes the stream the render kernels give global sample index first + i under
        seed = seed_value, so an integrator composed from the operators draws the numbers the built-in ones draw."""
        self._seed = int(seed_value)
        dev = torch.device(device)
        self._state = torch.empty((2, int(size)), dtype=torch.int64, device=dev)
        L.check(L.lib().mtsamd_sampler_seed(int(size), int(first), int(seed_value) & 0xFFFFFFFFFFFFFFFF, _ptr(self._state[0]),
                                            _ptr(self._state[1]), _stream()))

    def wavefront_size(self):
        return 0 if getattr(self, "_state", None) is None else self._state.shape[1]

    def _next(self, dims, active):
        if getattr(self, "_state", None) is None:
            raise RuntimeError("IndependentSampler: seed(seed_value, size) must be called before samples are drawn")
        n, dev = self._state.shape[1], self._state.device
        act = _mask(active, dev)
        if act is not None and act.shape[0] != n:
            raise RuntimeError("IndependentSampler: the mask has %d lanes, the sampler %d" % (act.shape[0], n))
        out = torch.empty((dims, n), dtype=torch.float32, device=dev)
        L.check(L.lib().mtsamd_sampler_next(n, dims, _ptr(self._state[0]), _ptr(self._state[1]), _ptr(act), _ptr(out), _stream()))
        return out

    def next_1d(self, active=True):
        """Sampler::next_1d (independent.cpp:76-88): (N,) floats; lanes masked out do not advance"""
        return self._next(1, active)[0]

    def next_2d(self, active=True):
        """Sampler::next_2d (independent.cpp:90-94): (N,2)"""
        return self._next(2, active).t().contiguous()


class HDRFilm:
    """src/films/hdrfilm.cpp + src/librender/film.cpp (defaults 768x576, gaussian filter)."""

    def __init__(self, width=768, height=576, crop_offset=None, crop_size=None, rfilter=None, file_format="openexr",
                 pixel_format="rgba", component_format="float16", high_quality_edges=False):
        self._size = (int(width), int(height))
        co = (0, 0) if crop_offset is None else (int(crop_offset[0]), int(crop_offset[1]))
        cs = self._size if crop_size is None else (int(crop_size[0]), int(crop_size[1]))
        self.set_crop_window(co, cs)
        self._filter = rfilter if rfilter is not None else GaussianFilter()
        self._storage = None
        self._channels = []
        self._dest_file = None
        self._hq_edges = bool(high_quality_edges)
        # hdrfilm.cpp:42-123: parameter validation and the per-format overrides
        ff, pf, cf = file_format.lower(), pixel_format.lower(), component_format.lower()
        if ff in ("openexr", "exr"):
            ff = "exr"
        elif ff not in ("rgbe", "pfm"):
            raise RuntimeError('The "file_format" parameter must either be equal to "openexr", "pfm", or "rgbe", found %s instead.' % ff)
        if pf not in ("luminance", "luminance_alpha", "rgb", "rgba", "xyz", "xyza"):
            raise RuntimeError('The "pixel_format" parameter must either be equal to "luminance", "luminance_alpha", "rgb", "rgba", '
                               '"xyz", "xyza". Found %s.' % pf)
        if cf not in ("float16", "float32", "uint32"):
            raise RuntimeError('The "component_format" parameter must either be equal to "float16", "float32", or "uint32". Found %s instead.' % cf)
        if ff == "rgbe":
            pf, cf = "rgb", "float32"
        elif ff == "pfm":
            pf, cf = (pf if pf in ("rgb", "luminance") else "rgb"), "float32"
        self._file_format, self._pixel_format, self._component_format = ff, pf, cf

    def size(self): return self._size
    def crop_size(self): return self._crop_size
    def crop_offset(self): return self._crop_offset
    def reconstruction_filter(self): return self._filter
    def has_high_quality_edges(self): return self._hq_edges

    def set_destination_file(self, filename):
        """hdrfilm.cpp:205-209"""
        self._dest_file = str(filename)

    def develop(self):
        """hdrfilm.cpp:322-342: convert the storage to pixel_format / component_format and write it to the destination
        file (the extension is replaced by the file format's)."""
        import os
        from . import bitmap as B
        if not self._dest_file:
            raise RuntimeError("Destination file not specified, cannot develop.")
        ext = {"exr": ".exr", "rgbe": ".rgbe", "pfm": ".pfm"}[self._file_format]
        root, cur = os.path.splitext(self._dest_file)
        filename = self._dest_file if cur.lower() == ext else root + ext
        raw = self.bitmap(raw=True)
        if raw.shape[2] != 5:           # hdrfilm.cpp:263-317: a film with AOVs is written as a multichannel image
            if self._file_format != "exr":
                raise RuntimeError("HDRFilm::develop(): only the X, Y, Z, A, W storage layout can be written")
            px = self.bitmap().cpu().numpy()
            names = ["R", "G", "B", "A"] + list(self._channels[5:])
            dt = {"float16": np.float16, "float32": np.float32, "uint32": np.uint32}[self._component_format]
            B.write_exr(filename, {n: np.ascontiguousarray(px[..., i]).astype(dt) for i, n in enumerate(names)})
            return filename
        if self._pixel_format in ("rgb", "rgba"):
            px = self.bitmap().cpu().numpy()
            px = px if self._pixel_format == "rgba" else px[..., :3]
            names = "RGBA"[:px.shape[2]]
        else:                           # Bitmap::convert from XYZAW: divide by the weight, keep XYZ / take Y
            r = raw.cpu().numpy()
            w = r[..., 4:5]
            inv = np.where(w != 0, 1.0 / np.where(w != 0, w, 1), 0).astype(np.float32)
            xyz, a = r[..., :3] * inv, r[..., 3:4] * inv
            px = {"xyz": xyz, "xyza": np.concatenate([xyz, a], 2), "luminance": xyz[..., 1:2],
                  "luminance_alpha": np.concatenate([xyz[..., 1:2], a], 2)}[self._pixel_format]
            names = {"xyz": "XYZ", "xyza": "XYZA", "luminance": "Y", "luminance_alpha": "YA"}[self._pixel_format]
        if self._file_format == "pfm":
            B.write_pfm(filename, px)
        elif self._file_format == "rgbe":
            B.write_rgbe(filename, px)
        else:
            dt = {"float16": np.float16, "float32": np.float32, "uint32": np.uint32}[self._component_format]
            B.write_exr(filename, {n: np.ascontiguousarray(px[..., i]).astype(dt) for i, n in enumerate(names)})
        return filename

    def set_crop_window(self, crop_offset, crop_size):
        """film.cpp:55-64"""
        if (crop_offset[0] < 0 or crop_offset[1] < 0 or crop_size[0] <= 0 or crop_size[1] <= 0 or
                crop_offset[0] + crop_size[0] > self._size[0] or crop_offset[1] + crop_size[1] > self._size[1]):
            raise RuntimeError("Invalid crop window specification!")
        self._crop_offset = (int(crop_offset[0]), int(crop_offset[1]))
        self._crop_size = (int(crop_size[0]), int(crop_size[1]))

    def prepare(self, channels=("X", "Y", "Z", "A", "W"), device="cuda"):
        """hdrfilm.cpp:188-203: storage ImageBlock(crop_size, n_channels), no filter / border."""
        if len(set(channels)) != len(channels):
            raise RuntimeError("Film::prepare(): duplicate channel name")
        self._storage = ImageBlock(self._crop_size, len(channels), device=device)
        self._storage.set_offset(self._crop_offset)
        self._channels = list(channels)

    def channels(self):
        """the channel names of the storage, as given to prepare()"""
        return list(self._channels)

    def put(self, block):
        self._storage.put(block)

    def bitmap(self, raw=False):
        """hdrfilm.cpp:249-320: raw=True -> the storage (X, Y, Z, A, W and the AOVs), else RGBA float32 (H, W, 4).  A storage with
        AOVs (n > 5 channels) gives the reference's multichannel bitmap (H, W, n - 1) (hdrfilm.cpp:263-317): R, G, B, A, then every
        AOV divided by the weight W (0 where W is 0); W itself is removed."""
        if self._storage is None:
            raise RuntimeError("HDRFilm::bitmap(): no storage (render first)")
        data = self._storage.data()
        if raw:
            return data
        n = data.shape[2]
        xyzaw = data if n == 5 else data[..., :5].contiguous()
        out = torch.empty((data.shape[0], data.shape[1], 4), dtype=torch.float32, device=data.device)
        L.check(L.lib().mtsamd_film_develop(_ptr(xyzaw), data.shape[0] * data.shape[1], _ptr(out), _stream()))
        if n == 5:
            return out
        w = data[..., 4:5]
        aovs = torch.where(w != 0, data[..., 5:] / torch.where(w != 0, w, torch.ones_like(w)), torch.zeros_like(data[..., 5:]))
        return torch.cat([out, aovs], dim=2)


LIBM_FUNCTIONS = ("sin", "cos", "tan", "exp", "log", "erf", "acos", "atan2", "atanh", "cosh")


def libm_eval(name, x, y=None):
    """The kernels' own elementary functions (csrc/device_libm.h) on a CUDA tensor of float32 arguments -- the role enoki::sin / exp /
    erf ... play in the reference (include/mitsuba/core/warp.h:54-90, render/microfacet.h:187-493).  `atan2` takes (y, x)."""
    fn = LIBM_FUNCTIONS.index(name)
    x = x.contiguous().float()
    if fn == 7:
        if y is None:
            raise RuntimeError("atan2 takes two arguments")
        y = y.contiguous().float()
    out = torch.empty_like(x)
    L.check(L.lib().mtsamd_libm_eval(fn, x.numel(), _ptr(x), _ptr(y) if fn == 7 else None, _ptr(out), _stream()))
    return out


def parse_fov(fov=None, focal_length=None, fov_axis="x", aspect=1.0):
    """src/librender/sensor.cpp:119-169"""
    if fov is not None and focal_length is not None:
        raise RuntimeError("Please specify either a focal length ('focal_length') or a field of view ('fov')!")
    f32 = np.float32
    if fov is not None:
        fov = f32(fov)
        fov_axis = fov_axis.lower()
        if fov_axis == "smaller":
            fov_axis = "y" if aspect > 1 else "x"
        elif fov_axis == "larger":
            fov_axis = "x" if aspect > 1 else "y"
    else:
        f = "50mm" if focal_length is None else str(focal_length)
        if f.endswith("mm"):
            f = f[:-2]
        try:
            value = f32(float(f))
        except ValueError:
            raise RuntimeError("Could not parse the focal length (must be of the form <x>mm, where <x> is a positive integer)!")
        fov = f32(2.0) * f32(np.degrees(np.arctan(f32(np.sqrt(f32(36 * 36 + 24 * 24))) / (f32(2.0) * value))))
        fov_axis = "diagonal"
    if fov_axis == "x":
        result = fov
    elif fov_axis == "y":
        result = f32(np.degrees(f32(2.0) * np.arctan(np.tan(f32(0.5) * f32(np.radians(fov))) * f32(aspect))))
    elif fov_axis == "diagonal":
        diagonal = f32(2.0) * np.tan(f32(0.5) * f32(np.radians(fov)))
        width = diagonal / f32(np.sqrt(f32(1.0) + f32(1.0) / f32(aspect * aspect)))
        result = f32(np.degrees(f32(2.0) * np.arctan(width * f32(0.5))))
    else:
        raise RuntimeError("The 'fov_axis' parameter must be set to one of 'smaller', 'larger', 'diagonal', 'x', or 'y'!")
    if result <= 0.0 or result >= 180.0:
        raise RuntimeError("The horizontal field of view must be in the range [0, 180]!")
    return float(result)


class PerspectiveCamera:
    """src/sensors/perspective.cpp"""

    def __init__(self, to_world=None, fov=None, focal_length=None, fov_axis="x", near_clip=1e-2, far_clip=1e4, film=None,
                 sampler=None):
        self._film = film if film is not None else HDRFilm()
        self._sampler = sampler if sampler is not None else IndependentSampler()
        self._to_world = np.eye(4, dtype=np.float32) if to_world is None else _f32(to_world).reshape(4, 4)
        if near_clip <= 0:
            raise RuntimeError("The 'near_clip' parameter must be greater than zero!")
        if near_clip >= far_clip:
            raise RuntimeError("The 'near_clip' parameter must be smaller than 'far_clip'.")
        self._near, self._far = float(near_clip), float(far_clip)
        w, h = self._film.size()
        self._x_fov = parse_fov(fov, focal_length, fov_axis, w / h)

    def film(self): return self._film
    def sampler(self): return self._sampler
    def x_fov(self): return self._x_fov
    def near_clip(self): return self._near
    def far_clip(self): return self._far
    def world_transform(self): return self._to_world

    def _fill_desc(self, d):
        d.to_world = (C.c_float * 16)(*self._to_world.reshape(-1).tolist())
        d.fov_x_deg = self._x_fov
        d.near_clip, d.far_clip = self._near, self._far
        f = self._film
        d.film_width, d.film_height = f.size()
        d.crop_x, d.crop_y = f.crop_offset()
        d.crop_width, d.crop_height = f.crop_size()
        d.rfilter = f.reconstruction_filter().kind
        d.rfilter_param = f.reconstruction_filter().param
        d.rfilter_param2 = f.reconstruction_filter().param2
        d.rfilter_analytic = 0
        d.sample_count = self._sampler.sample_count()
        d.seed = self._sampler.seed_value()
        d.aperture_radius, d.focus_distance = 0.0, 0.0

    def needs_aperture_sample(self):
        return False

    def sample_ray(self, position_sample, aperture_sample=None):
        """perspective.cpp:153-188 / thinlens.cpp:175-214 for (N,2) film-plane samples in [0,1)^2 (and (N,2) aperture samples)
        -> Ray3f."""
        ps = torch.as_tensor(position_sample, dtype=torch.float32, device="cuda").reshape(-1, 2)
        n = ps.shape[0]
        sx, sy = ps[:, 0].contiguous(), ps[:, 1].contiguous()
        apx = apy = None
        if aperture_sample is not None:
            ap = torch.as_tensor(aperture_sample, dtype=torch.float32, device="cuda").reshape(-1, 2)
            if ap.shape[0] != n:
                raise RuntimeError("aperture_sample must have one entry per position sample")
            apx, apy = ap[:, 0].contiguous(), ap[:, 1].contiguous()
        out = torch.empty((8, n), dtype=torch.float32, device="cuda")
        d = L.RenderDesc()
        self._fill_desc(d)
        d.max_depth, d.rr_depth = -1, 5
        L.check(L.lib().mtsamd_camera_sample_rays(C.byref(d), n, _ptr(sx), _ptr(sy), _ptr(apx) if apx is not None else None,
                                                  _ptr(apy) if apy is not None else None, *[_ptr(out[k]) for k in range(8)], _stream()))
        return Ray3f(o=out[0:3].t().contiguous(), d=out[3:6].t().contiguous(), mint=out[6].clone(), maxt=out[7].clone())


class ThinLensCamera(PerspectiveCamera):
    """src/sensors/thinlens.cpp: perspective camera with a circular aperture focused at `focus_distance`"""

    def __init__(self, aperture_radius=None, focus_distance=None, **kwargs):
        super().__init__(**kwargs)
        if aperture_radius is None:
            raise RuntimeError('Property "aperture_radius" has not been specified!')       # props.float_("aperture_radius"), thinlens.cpp:112
        self._aperture_radius = float(aperture_radius)
        if self._aperture_radius == 0.0:              # thinlens.cpp:114-117
            self._aperture_radius = float(np.finfo(np.float32).eps) / 2
        if self._aperture_radius < 0.0:
            raise RuntimeError("The 'aperture_radius' parameter must not be negative")
        self._focus_distance = float(focus_distance) if focus_distance is not None else self._far      # sensor.cpp:104

    def aperture_radius(self): return self._aperture_radius
    def focus_distance(self): return self._focus_distance

    def needs_aperture_sample(self):
        return True

    def _fill_desc(self, d):
        super()._fill_desc(d)
        d.aperture_radius, d.focus_distance = self._aperture_radius, self._focus_distance


def srgb_coeff_path(build=True):
    """The RGB -> spectrum coefficient table ('data/srgb.coeff' of the reference, src/librender/srgb.cpp:24-27): generated
    on first use with mtsamd_rgb2spec_build at the reference's resolution 64 (build artefact, not tracked)."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "srgb.coeff")
    if not os.path.exists(path) and build:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        L.check(L.lib().mtsamd_rgb2spec_build(path.encode(), 64, min(os.cpu_count() or 1, 16)))
    return path


def spectrum_descs(spectra, keep):
    """parsed spectra (mitsuba2_amd.spectrum.parse) -> array of mtsamd_spectrum_desc; the arrays they point to are appended to `keep`"""
    sp = (L.SpectrumDesc * max(len(spectra), 1))()
    for i, s in enumerate(spectra):
        sp[i].type = {"regular": 0, "irregular": 1, "blackbody": 2}[s["kind"]]
        if s["kind"] == "blackbody":
            sp[i].temperature = s["temperature"]
            continue
        values = _f32(s["values"]).reshape(-1)
        keep.append(values)
        sp[i].size, sp[i].values = values.size, values.ctypes.data_as(L.f32p)
        if s["kind"] == "regular":
            sp[i].lambda_min, sp[i].lambda_max = s["lambda_min"], s["lambda_max"]
        else:
            nodes = _f32(s["wavelengths"]).reshape(-1)
            keep.append(nodes)
            sp[i].wavelengths = nodes.ctypes.data_as(L.f32p)
    return sp


def spectrum_eval(spectrum, wavelengths):
    """Texture::eval of a spectrum plugin dictionary (or a parsed spectrum) at a tensor of wavelengths, on the device function the render
    kernels call (mtsamd_spectrum_eval)"""
    from . import spectrum as S
    spec = S.parse(spectrum) if "kind" not in spectrum else spectrum
    keep = []
    sp = spectrum_descs([spec], keep)
    lam = wavelengths.to(torch.float32).contiguous()
    out = torch.empty_like(lam)
    L.check(L.lib().mtsamd_spectrum_eval(sp, lam.numel(), _ptr(lam), _ptr(out), _stream()))
    return out


def spectrum_mean(spectrum):
    """Texture::mean() of a `regular` / `irregular` spectrum (mtsamd_spectrum_mean; host only)"""
    from . import spectrum as S
    spec = S.parse(spectrum) if "kind" not in spectrum else spectrum
    keep = []
    sp = spectrum_descs([spec], keep)
    mean = C.c_float()
    L.check(L.lib().mtsamd_spectrum_mean(sp, C.byref(mean)))
    return float(mean.value)


# --------------------------------------------------------------------------------------------
class Scene:
    """src/librender/scene.cpp: shapes + BSDFs + emitters uploaded to one GPU, BVH built by the library."""

    def __init__(self, scene_dict, device=0, sensor=None, integrator=None, variant="rgb"):
        lib = L.lib()
        if variant not in ("rgb", "spectral"):
            raise RuntimeError("unsupported variant '%s' (rgb or spectral)" % variant)
        self._variant = variant
        if not torch.cuda.is_available():
            raise RuntimeError("mitsuba2_amd requires a HIP device (torch.cuda.is_available() is False)")
        self._device_index = int(device)
        self._pending_vertices = {}    # shape -> (positions, normals): device clones update_vertices(normals="recompute") has not mirrored yet
        self._dict = scene_dict
        self._sensors = [sensor] if sensor is not None else []
        self._integrator = integrator
        meshes, bsdfs, emitters = scene_dict["meshes"], scene_dict["bsdfs"], scene_dict.get("emitters", [])
        keep = []
        md = (L.MeshDesc * len(meshes))()
        for i, m in enumerate(meshes):
            pos, faces = _f32(m["positions"]).reshape(-1, 3), np.ascontiguousarray(m["faces"], dtype=np.uint32).reshape(-1, 3)
            nrm = _f32(m["normals"]).reshape(-1, 3) if m.get("normals") is not None else None
            uv = _f32(m["texcoords"]).reshape(-1, 2) if m.get("texcoords") is not None else None
            keep += [pos, faces, nrm, uv]
            md[i].vertex_count, md[i].face_count = pos.shape[0], faces.shape[0]
            md[i].positions = pos.ctypes.data_as(L.f32p)
            md[i].faces = faces.ctypes.data_as(L.u32p)
            md[i].normals = nrm.ctypes.data_as(L.f32p) if nrm is not None else None
            md[i].texcoords = uv.ctypes.data_as(L.f32p) if uv is not None else None
            md[i].bsdf, md[i].emitter = int(m["bsdf"]), int(m.get("emitter", -1))
        tex = []                       # bitmap textures (src/textures/bitmap.cpp): reflectance = dict(type="bitmap", data=(H,W,3))
        self._bsdf_texture = {}
        self._param_texture = {}       # (bsdf record, parameter name) -> texture index: the textured parameters beside the reflectance
        tex_bindings = []              # (bsdf record, mtsamd_bsdf_param, texture index): mtsamd_texture_binding

        def add_texture(spec):
            kind = spec.get("type")
            if kind not in ("bitmap", "checkerboard"):
                raise RuntimeError("Texture plugin '%s' is not supported by this backend (bitmap, checkerboard)" % kind)
            data = None
            if kind == "bitmap":
                data = _f32(spec["data"])
                if data.ndim != 3 or data.shape[2] != 3:
                    raise RuntimeError("bitmap texture: expected (H, W, 3) linear RGB data")
            tex.append((kind, data, spec))
            return len(tex) - 1
        from . import bsdfs as B
        from . import spectrum as S
        self._bsdf_records = [B.normalize(b) for b in bsdfs]      # plugin defaults / validation (src/bsdfs/*.cpp constructors)
        flat = B.flatten(self._bsdf_records)                      # + the children of blendbsdf / mask records
        bd = (L.BsdfDesc * max(len(flat), 1))()
        bindings = []                  # (target, index, mtsamd_bsdf_param, parsed spectrum): mtsamd_spectrum_binding
        for i, n in enumerate(flat):
            bd[i].type, bd[i].twosided = n["type"], int(n["twosided"])
            bd[i].nested = (C.c_int32 * 2)(*n.get("nested", [-1, -1]))
            refl = n["reflectance"]
            if isinstance(refl, dict):
                bd[i].reflectance = (C.c_float * 3)(0.5, 0.5, 0.5)
                bd[i].texture = self._bsdf_texture[i] = add_texture(refl)
            else:
                bd[i].reflectance = (C.c_float * 3)(*[float(x) for x in refl])
                bd[i].texture = -1
            for name in ("specular_reflectance", "specular_transmittance", "eta", "k"):
                setattr(bd[i], name, (C.c_float * 3)(*n[name]))
            bd[i].int_ior, bd[i].ext_ior, bd[i].alpha_u, bd[i].alpha_v = n["int_ior"], n["ext_ior"], n["alpha_u"], n["alpha_v"]
            bd[i].distribution, bd[i].sample_visible, bd[i].nonlinear = n["distribution"], int(n["sample_visible"]), int(n["nonlinear"])
            bd[i].uniform_mask = n["uniform_mask"]
            shared = {}                # a textured `alpha` is one texture behind alpha_u and alpha_v
            for pname, spec in n.get("textures", {}).items():
                if id(spec) not in shared:
                    shared[id(spec)] = add_texture(spec)
                self._param_texture[(i, pname)] = shared[id(spec)]
            pt = {k: self._param_texture[(i, k)] for k in n.get("textures", {})}
            if "alpha_u" in pt and pt.get("alpha_v") == pt["alpha_u"]:
                tex_bindings.append((i, B.TEXTURE_PARAMS["alpha"], pt.pop("alpha_u")))
                del pt["alpha_v"]
            tex_bindings += [(i, B.TEXTURE_PARAMS[k], t) for k, t in pt.items()]
            for param, spec in (n.get("spectra", {}) if variant == "spectral" else {}).items():
                # tabulated spectra replace the colour (RGB variant: the pre-integrated colour stays)
                bindings.append((0, i, param, spec if "kind" in spec else S.parse(spec)))
        td = (L.TextureDesc * max(len(tex), 1))()
        for i, (kind, t, spec) in enumerate(tex):
            if kind == "bitmap":
                td[i].kind, td[i].width, td[i].height = 0, t.shape[1], t.shape[0]
                td[i].data = t.ctypes.data_as(L.f32p)
            else:                       # src/textures/checkerboard.cpp: color0 = .4, color1 = .2 by default
                td[i].kind = 1
                td[i].color0 = (C.c_float * 3)(*B._rgb(spec.get("color0"), 0.4))
                td[i].color1 = (C.c_float * 3)(*B._rgb(spec.get("color1"), 0.2))
            if spec.get("to_uv") is not None:       # Transform4f::extract(): the upper-left 3x3 acts on (u, v, 1)
                m = _f32(spec["to_uv"]).reshape(4, 4)
                td[i].to_uv = (C.c_float * 6)(float(m[0, 0]), float(m[0, 1]), float(m[0, 2]), float(m[1, 0]), float(m[1, 1]), float(m[1, 2]))
        self._texture_shapes = [t.shape if t is not None else (0, 0, 3) for (_, t, _) in tex]
        ed = (L.EmitterDesc * max(len(emitters), 1))()
        from . import emitters as E
        for i, e in enumerate(emitters):
            n = E.normalize(e)             # plugin defaults / validation (src/emitters/*.cpp constructors)
            ed[i].type = n["type"]
            ed[i].to_world = (C.c_float * 16)(*n["to_world"].reshape(-1).tolist())
            ed[i].radiance = (C.c_float * 3)(*n["radiance"])
            ed[i].cutoff_angle, ed[i].beam_width = n["cutoff_angle"], n["beam_width"]
            if n.get("spectrum") is not None:
                spec = n["spectrum"]
                if variant == "spectral":
                    bindings.append((1, i, 0, spec if "kind" in spec else S.parse(spec, within_emitter=True)))
                elif spec.get("kind") == "blackbody":
                    raise RuntimeError("blackbody: Not implemented for non-spectral modes")
            if n["type"] == E.TYPE_IDS["envmap"]:          # src/emitters/envmap.cpp: lat-long image (linear RGB), scale, to_world
                img = _f32(n["data"])
                if img.ndim != 3 or img.shape[2] != 3:
                    raise RuntimeError("envmap: expected (H, W, 3) linear RGB data")
                keep.append(img)
                ed[i].envmap_data = img.ctypes.data_as(L.f32p)
                ed[i].envmap_height, ed[i].envmap_width = img.shape[0], img.shape[1]
                ed[i].envmap_scale = n["scale"]
        sd = L.SceneDesc(md, len(meshes), bd, len(flat), ed, len(emitters), td, len(tex), 0, None)
        if variant == "spectral":
            sd.spectral = 1
            sd.rgb2spec_path = srgb_coeff_path().encode()
        handle = C.c_void_p()
        if tex_bindings:               # RGB variant only: the library refuses them in a spectral scene, with or without spectra
            tb = (L.TextureBinding * len(tex_bindings))()
            for i, (index, param, texture) in enumerate(tex_bindings):
                tb[i].bsdf, tb[i].param, tb[i].texture = index, param, texture
            L.check(lib.mtsamd_scene_create_with_textures(C.byref(sd), tb, len(tex_bindings), self._device_index, C.byref(handle)))
        elif bindings:
            sp, bn = spectrum_descs([b[3] for b in bindings], keep), (L.SpectrumBinding * len(bindings))()
            for i, (target, index, param, _) in enumerate(bindings):
                bn[i].target, bn[i].index, bn[i].param, bn[i].spectrum = target, index, param, i
            L.check(lib.mtsamd_scene_create_with_spectra(C.byref(sd), sp, len(bindings), bn, len(bindings), self._device_index, C.byref(handle)))
        else:
            L.check(lib.mtsamd_scene_create(C.byref(sd), self._device_index, C.byref(handle)))
        self._handle = handle
        self._n_spectra = len(bindings)
        self._shape_count = len(meshes)
        self._tables = None            # operator API: per-shape tables, read on first use
        self._environment = next((i for i, e in enumerate(emitters) if e.get("type", "area") in ("constant", "envmap")), -1)      # scene.cpp:44-48

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            try:
                L.lib().mtsamd_scene_destroy(h)
            except Exception:
                pass
            self._handle = None

    # -- accessors (scene_v.cpp:37-86)
    def sensors(self): return self._sensors
    def integrator(self): return self._integrator
    def shape_count(self): return self._shape_count

    def bbox(self):
        out = (C.c_float * 6)()
        L.check(L.lib().mtsamd_scene_bbox(self._handle, out))
        return np.array(out[:3], dtype=np.float32), np.array(out[3:], dtype=np.float32)

    def info(self):
        out = (C.c_uint32 * 6)()
        L.check(L.lib().mtsamd_scene_info(self._handle, out))
        return dict(zip(("primitives", "bvh_nodes", "bvh_depth", "shapes", "emitters", "lds_nodes"), [int(x) for x in out]))

    def set_bsdf_reflectance(self, index, rgb):
        L.check(L.lib().mtsamd_scene_set_bsdf_reflectance(self._handle, int(index), (C.c_float * 3)(*[float(x) for x in rgb])))

    def texture_index(self, bsdf, param="reflectance"):
        """Index of the texture behind a parameter of BSDF record `bsdf` (None if that parameter is constant): its (diffuse) reflectance
        or blend weight by default, or "alpha_u", "alpha_v" ("alpha": the texture both share), "specular_reflectance",
        "specular_transmittance"."""
        if param in ("reflectance", "diffuse_reflectance", "weight", "opacity"):
            return self._bsdf_texture.get(int(bsdf))
        if param == "alpha":
            u, v = self._param_texture.get((int(bsdf), "alpha_u")), self._param_texture.get((int(bsdf), "alpha_v"))
            return u if u == v else None
        return self._param_texture.get((int(bsdf), param))

    def update_texture(self, texture, data):
        """parameters_changed() for a BitmapTexture's `data` (bitmap.cpp:295-299); data: (H,W,3) tensor or array."""
        shape = self._texture_shapes[int(texture)]
        if isinstance(data, torch.Tensor):
            t = data.detach().to(torch.device("cuda", self._device_index), torch.float32).contiguous()
            if tuple(t.shape) != tuple(shape):
                raise RuntimeError("texture data has shape %s, expected %s" % (tuple(t.shape), tuple(shape)))
            # device-to-device copy enqueued on the current stream: stream-ordered with whatever wrote `t` and with the next render; a
            # temporary `t` is safe too (the caching allocator reuses its memory on this stream only after the copy)
            L.check(L.lib().mtsamd_scene_update_texture(self._handle, int(texture), _ptr(t), _stream()))
        else:
            a = _f32(data)
            if tuple(a.shape) != tuple(shape):
                raise RuntimeError("texture data has shape %s, expected %s" % (tuple(a.shape), tuple(shape)))
            L.check(L.lib().mtsamd_scene_update_texture(self._handle, int(texture), a.ctypes.data_as(C.c_void_p), _stream()))
            torch.cuda.current_stream().synchronize()
        if self._variant == "spectral":
            # the scene description follows the device (as update_envmap): a ParameterMap built afterwards starts from the new texels,
            # clamped to [0, 1] as the scene holds them.  A record's texture dictionary IS the one inside self._dict (bsdfs.normalize keeps
            # the object), so this writes both.  The spectral update converts the texels on the host anyway, so the copy of a device
            # tensor costs it nothing new; the RGB update stays an asynchronous device copy and is not mirrored
            new = data.detach().cpu().numpy() if isinstance(data, torch.Tensor) else data
            for i, t in self._bsdf_texture.items():
                if t == int(texture) and i < len(self._bsdf_records):
                    self._bsdf_records[i]["reflectance"]["data"] = np.clip(np.array(new, np.float32).reshape(shape), 0.0, 1.0)

    @property
    def _dict(self):
        """The scene description.  It follows the device: vertex arrays that update_vertices(normals="recompute") left on the device are
        copied into it before it is handed out, so every reader sees the scene as it is."""
        for shape, (pos, nrm) in list(self._pending_vertices.items()):
            mesh = self._description["meshes"][shape]
            mesh["positions"] = pos.cpu().numpy().reshape(-1, 3)
            mesh["normals"] = nrm.cpu().numpy().reshape(-1, 3)
            del self._pending_vertices[shape]
        return self._description

    @_dict.setter
    def _dict(self, value):
        self._pending_vertices.clear()
        self._description = value

    def _recompute_vertices(self, shape, positions, rebuild=0):
        """update_vertices(normals="recompute"): mtsamd_scene_update_vertices with MTSAMD_VERTICES_RECOMPUTE_NORMALS"""
        mesh = self._description["meshes"][shape]           # counts and the presence of normals never change: no need to flush for them
        n_vertices = _f32(mesh["positions"]).reshape(-1, 3).shape[0]
        dev = torch.device("cuda", self._device_index)
        if isinstance(positions, torch.Tensor):
            pos = positions.detach().to(device=dev, dtype=torch.float32).reshape(-1)
        else:
            pos = torch.from_numpy(_f32(positions).reshape(-1)).to(dev)
        if pos.numel() != 3 * n_vertices:
            raise RuntimeError("positions has %d values, expected 3 * %d" % (pos.numel(), n_vertices))
        if mesh.get("normals") is None:
            raise RuntimeError("shape %d was created without vertex normals: storing new normals in such a mesh is not implemented" % shape)
        pos = pos.clone()                                    # the caller may overwrite theirs; the scene reads and keeps this one
        nrm = torch.empty(3 * n_vertices, dtype=torch.float32, device=dev)
        L.check(L.lib().mtsamd_scene_update_vertices(self._handle, shape, _ptr(pos), None, 1 | rebuild, _ptr(nrm), _stream()))
        self._pending_vertices[shape] = (pos, nrm.clone())
        return nrm.reshape(-1, 3)

    def rebuild_accel(self, builder="lbvh"):
        """mtsamd_scene_rebuild_accel_with: a new topology of the accelerator, built on the device from the positions the scene holds
        now -- what a tree refitted through large vertex moves needs once accel_info(sah_cost=True) says it has degraded.  builder:
        "lbvh" (the fast one), or "sah": the binned-SAH tree a scene created from these positions would get, node for node.  Samples and
        queries are the same bits before and after; every setter's state is kept; a flat scene is left alone."""
        if builder not in ("sah", "lbvh"):
            raise RuntimeError("builder: \"sah\" or \"lbvh\", not %r" % (builder,))
        L.check(L.lib().mtsamd_scene_rebuild_accel_with(self._handle, ("sah", "lbvh").index(builder), 0, _stream()))

    def rebuild_levels(self):
        """Measurement aid (mtsamd_scene_rebuild_levels): [(nodes, milliseconds)] per level of the last rebuild_accel(builder="sah")"""
        n = C.c_uint32(0)
        L.check(L.lib().mtsamd_scene_rebuild_levels(self._handle, 0, None, None, C.byref(n)))
        nodes, ms = (C.c_uint32 * max(n.value, 1))(), (C.c_float * max(n.value, 1))()
        L.check(L.lib().mtsamd_scene_rebuild_levels(self._handle, n.value, nodes, ms, C.byref(n)))
        return [(int(nodes[i]), float(ms[i])) for i in range(n.value)]

    def accel_info(self, sah_cost=False):
        """mtsamd_scene_accel_info: counts and depths of the accelerator, its builder ("sah": creation, "lbvh": a rebuild), the number of
        rebuilds, and with sah_cost=True the SAH cost of the tree as it is now (0.0 for a flat scene)."""
        out = (C.c_uint32 * 8)()
        cost = C.c_double(0.0)
        L.check(L.lib().mtsamd_scene_accel_info(self._handle, out, C.byref(cost) if sah_cost else None))
        info = dict(zip(("bvh_nodes", "wide_nodes", "slots", "depth", "wdepth", "stack_depth"), [int(x) for x in out[:6]]))
        info["builder"] = ("sah", "lbvh")[int(out[6])]
        info["rebuilds"] = int(out[7])
        if sah_cost:
            info["sah_cost"] = float(cost.value)
        return info

    def update_vertices(self, shape, positions, normals=None, accel="refit"):
        """parameters_changed({"vertex_positions_buf"}) of mesh `shape` (mesh.cpp:781-804): new vertex positions, same vertex count and
        faces.  positions: (N, 3) or flat 3N, a numpy array or a torch tensor on the host or the device (a device tensor is read where it
        is).  A mesh with vertex normals gets `normals`, or -- None -- normals recomputed from the new positions with
        loaders.compute_vertex_normals (recompute_vertex_normals), which runs on the host in float64: a device tensor makes one round trip
        for it.  normals="recompute" recomputes them in the library instead (mtsamd_compute_vertex_normals' fp32 arithmetic, on the device
        for hierarchy scenes): with a device tensor no vertex data is copied to the host, the description is brought up to date when it is
        next read, and the call returns the (N, 3) normals as a device tensor.
        The accelerator is refitted (accel="refit") or, after the update, rebuilt in the same call (accel="rebuild": rebuild_accel();
        accel="rebuild-sah": rebuild_accel(builder="sah"));
        bbox(), the emitter tables and the scene description follow."""
        shape = int(shape)
        if accel not in ("refit", "rebuild", "rebuild-sah"):
            raise RuntimeError("accel: \"refit\", \"rebuild\" or \"rebuild-sah\", not %r" % (accel,))
        rebuild = {"refit": 0, "rebuild": 2, "rebuild-sah": 2 | 8}[accel]          # MTSAMD_VERTICES_REBUILD_ACCEL, .._ACCEL_SAH
        if not 0 <= shape < self._shape_count:
            raise RuntimeError("invalid shape index %d (the scene has %d shapes)" % (shape, self._shape_count))
        if isinstance(normals, str):
            if normals != "recompute":
                raise RuntimeError("normals: an array, None or \"recompute\", not %r" % normals)
            return self._recompute_vertices(shape, positions, rebuild)
        mesh = self._dict["meshes"][shape]
        n_vertices = _f32(mesh["positions"]).reshape(-1, 3).shape[0]
        dev = torch.device("cuda", self._device_index)

        def as_arg(x, what):
            """-> (pointer argument, object to keep alive, host copy)"""
            if isinstance(x, torch.Tensor):
                t = x.detach().to(torch.float32).contiguous()
                if t.numel() != 3 * n_vertices:
                    raise RuntimeError("%s has %d values, expected 3 * %d" % (what, t.numel(), n_vertices))
                host = None if t.is_cuda else t.numpy()
                if t.is_cuda:
                    t = t.to(dev)
                    return _ptr(t), t, host
                return host.ctypes.data_as(C.c_void_p), host, host
            a = _f32(x)
            if a.size != 3 * n_vertices:
                raise RuntimeError("%s has %d values, expected 3 * %d" % (what, a.size, n_vertices))
            return a.ctypes.data_as(C.c_void_p), a, a
        p_arg, p_keep, p_host = as_arg(positions, "positions")
        n_arg, n_keep, n_host = None, None, None
        if mesh.get("normals") is not None:
            if normals is None:
                from . import loaders
                if p_host is None:
                    p_host = p_keep.cpu().numpy()
                normals = loaders.compute_vertex_normals(p_host.reshape(-1, 3), mesh["faces"])
            n_arg, n_keep, n_host = as_arg(normals, "normals")
        elif normals is not None:
            raise RuntimeError("shape %d was created without vertex normals: none can be set" % shape)
        if rebuild:
            L.check(L.lib().mtsamd_scene_update_vertices(self._handle, shape, p_arg, n_arg, rebuild, None, _stream()))
        else:
            L.check(L.lib().mtsamd_scene_set_vertex_positions(self._handle, shape, p_arg, n_arg, _stream()))
        # the scene description follows the device, as for the other setters
        if p_host is None:
            p_host = p_keep.cpu().numpy()
        mesh["positions"] = np.array(p_host, np.float32).reshape(-1, 3)
        if n_keep is not None:
            if n_host is None:
                n_host = n_keep.cpu().numpy()
            mesh["normals"] = np.array(n_host, np.float32).reshape(-1, 3)

    def read_accel(self, which, words=None):
        """Test aid (mtsamd_scene_read_accel): one device array of the accelerator as a flat numpy array of 32-bit words.  which:
        "nodes", "qnodes", "wnodes", "tris", "tri_pos", "tri_nrm", "area_pmf", "area_cdf", "grid", or an array of the refit table of a
        hierarchy scene: "kids", "order", "node_child", "wide_child", "boxes", "slot_prim".  `words`: the array's length where info() and
        accel_info() do not give it; a wrong length is an error."""
        names = ("nodes", "qnodes", "wnodes", "tris", "tri_pos", "tri_nrm", "area_pmf", "area_cdf", "grid",
                 "kids", "order", "node_child", "wide_child", "boxes", "slot_prim")
        info = self.info()
        n_prims, n_nodes = info["primitives"], info["bvh_nodes"]
        has_normals = any(m.get("normals") is not None for m in self._dict["meshes"])
        sizes = dict(nodes=16 * n_nodes, qnodes=8 * n_nodes, tris=12 * n_prims, tri_pos=9 * n_prims, tri_nrm=9 * n_prims if has_normals else 0,
                     area_pmf=n_prims, area_cdf=n_prims, grid=6, node_child=2 * n_nodes)
        n_builder = 2 * n_nodes + 1                 # the binary tree of a hierarchy scene: one more leaf than inner nodes
        sizes.update(kids=2 * n_builder, order=n_builder, boxes=6 * n_builder, slot_prim=n_prims)
        if words is None and which in ("wnodes", "wide_child"):
            words = (16 if which == "wnodes" else 4) * self.accel_info()["wide_nodes"]
        if words is None:
            words = sizes[which]
        out = np.zeros(max(int(words), 1), np.uint32)
        L.check(L.lib().mtsamd_scene_read_accel(self._handle, names.index(which), out.ctypes.data_as(C.c_void_p), 4 * int(words)))
        return out[:int(words)]

    def update_envmap(self, data, rebuild_distribution=True):
        """parameters_changed() for the envmap emitter's `data` (envmap.cpp:220-253); data: (H, W, 3) linear RGB tensor or array.
        ``rebuild_distribution=False`` keeps the importance-sampling hierarchy of the previous texels."""
        if isinstance(data, torch.Tensor):
            data = data.detach().cpu().numpy()
        a = _f32(data)
        L.check(L.lib().mtsamd_scene_update_envmap(self._handle, a.ctypes.data_as(L.f32p), 1 if rebuild_distribution else 0))
        # the scene description follows the device: a ParameterMap built after an optimisation step starts from the new texels
        for em in self._dict.get("emitters", []):
            if em.get("type", "area") == "envmap":
                em["data"] = a.reshape(np.asarray(em["data"]).shape).copy()

    def set_bsdf_param(self, index, kind, values):
        """parameters_changed() after editing a constant parameter of a BSDF record (mtsamd_bsdf_param kinds: 0 (diffuse_)reflectance,
        1 specular_reflectance, 2 eta, 3 k, 4 alpha, 5 specular_transmittance)"""
        v = [float(x) for x in values] + [0.0, 0.0]
        L.check(L.lib().mtsamd_scene_set_bsdf_param(self._handle, int(index), int(kind), (C.c_float * 3)(*v[:3])))

    def set_aov_keep_limit(self, nbytes):
        """Device memory a multi-pass `aov` render may take to keep the streams of all passes, which makes its film equal the one-pass film
        bit for bit (default 2^30; 0: always splat pass by pass)."""
        L.check(L.lib().mtsamd_scene_set_aov_keep_limit(self._handle, int(nbytes)))

    def set_emitter_radiance(self, index, rgb):
        L.check(L.lib().mtsamd_scene_set_emitter_radiance(self._handle, int(index), (C.c_float * 3)(*[float(x) for x in rgb])))

    # -- queries
    def _soa(self, ray, active):
        dev = torch.device("cuda", self._device_index)
        o = ray.o.to(dev, torch.float32).t().contiguous()
        d = ray.d.to(dev, torch.float32).t().contiguous()
        mint = ray.mint.to(dev, torch.float32).contiguous()
        maxt = ray.maxt.to(dev, torch.float32).contiguous()
        act = None
        if active is not None and active is not True:
            act = torch.as_tensor(active, device=dev).to(torch.uint8).contiguous()
        r = L.Rays(_ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(mint), _ptr(maxt), _ptr(act))
        return r, (o, d, mint, maxt, act), o.shape[1], dev

    def ray_intersect(self, ray, active=True, full=True):
        """Scene::ray_intersect (scene.h:36).  full=False skips the SurfaceInteraction fill."""
        r, keep, n, dev = self._soa(ray, active)
        t = torch.empty(n, dtype=torch.float32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        shape = torch.empty(n, dtype=torch.int32, device=dev)
        if not full:
            u = torch.empty(n, dtype=torch.float32, device=dev)
            v = torch.empty(n, dtype=torch.float32, device=dev)
            L.check(L.lib().mtsamd_ray_intersect(self._handle, n, C.byref(r), _ptr(t), _ptr(prim), _ptr(shape), _ptr(u), _ptr(v), _stream()))
            return SurfaceInteraction3f(t=t, prim_index=prim, shape_index=shape, prim_uv=torch.stack([u, v], dim=1))
        si = torch.empty((26, n), dtype=torch.float32, device=dev)
        L.check(L.lib().mtsamd_ray_intersect_si(self._handle, n, C.byref(r), _ptr(t), _ptr(prim), _ptr(shape), _ptr(si), _stream()))
        g = lambda a, b: si[a:b].t().contiguous()
        return SurfaceInteraction3f(t=t, prim_index=prim, shape_index=shape, p=g(0, 3), n=g(3, 6), uv=g(6, 8), sh_frame_s=g(8, 11),
                                    sh_frame_t=g(11, 14), sh_frame_n=g(14, 17), dp_du=g(17, 20), dp_dv=g(20, 23), wi=g(23, 26),
                                    _scene=self, _ray_d=ray.d)

    def ray_intersect_naive(self, ray, active=True):
        """Scene::ray_intersect_naive (scene.h:38-44): brute force, for tests."""
        r, keep, n, dev = self._soa(ray, active)
        t = torch.empty(n, dtype=torch.float32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        shape = torch.empty(n, dtype=torch.int32, device=dev)
        u = torch.empty(n, dtype=torch.float32, device=dev)
        v = torch.empty(n, dtype=torch.float32, device=dev)
        L.check(L.lib().mtsamd_ray_intersect_naive(self._handle, n, C.byref(r), _ptr(t), _ptr(prim), _ptr(shape), _ptr(u), _ptr(v), _stream()))
        return SurfaceInteraction3f(t=t, prim_index=prim, shape_index=shape, prim_uv=torch.stack([u, v], dim=1))

    def ray_test(self, ray, active=True):
        """Scene::ray_test (scene.h:62)"""
        r, keep, n, dev = self._soa(ray, active)
        hit = torch.empty(n, dtype=torch.uint8, device=dev)
        L.check(L.lib().mtsamd_ray_test(self._handle, n, C.byref(r), _ptr(hit), _stream()))
        return hit.bool()

    # -- operator API (scene_v.cpp:37-86: shapes, sample_emitter_direction, pdf_emitter_direction)
    def _require_rgb(self, what):
        if self._variant != "rgb":
            raise RuntimeError("%s: the operator API is implemented for the RGB variant only (this scene is %s)" % (what, self._variant))

    def _operator_tables(self):
        """per shape: BSDF index, MTSAMD_BSDF_* flag word, emitter index or -1 (mtsamd_scene_shape_tables, read once), and the
        BSDFFlags of every top-level BSDF record"""
        if self._tables is None:
            n = self._shape_count
            raw = (C.c_int32 * max(3 * n, 1))()
            L.check(L.lib().mtsamd_scene_shape_tables(self._handle, raw))
            a = np.array(raw[:3 * n], dtype=np.int32).reshape(n, 3)
            dev = torch.device("cuda", self._device_index)
            flags = np.array([bsdf_flags(self._bsdf_records[b]) for b in a[:, 0]], dtype=np.int32)
            self._tables = dict(bsdf=a[:, 0].copy(), word=a[:, 1].copy(), emitter=torch.as_tensor(a[:, 2].copy(), device=dev),
                                emitter_host=a[:, 2].copy(), flags=torch.as_tensor(flags, device=dev), flags_host=flags)
        return self._tables

    def shapes(self):
        """Scene::shapes (scene.h:143-145)"""
        return [Shape(self, i) for i in range(self._shape_count)]

    def emitters(self):
        """Scene::emitters (scene.h:135-137)"""
        return [Emitter(self, index=i) for i in range(len(self._dict.get("emitters", [])))]

    def environment(self):
        """Scene::environment (scene.h:140): the `constant` / `envmap` emitter, or None"""
        return Emitter(self, index=self._environment) if self._environment >= 0 else None

    def sample_emitter_direction(self, ref, sample, test_visibility=True, active=True):
        """Scene::sample_emitter_direction (scene.cpp:165-189) -> (DirectionSample3f, spec (N,3)).  `ref` needs only `p`.  With
        test_visibility the shadow rays (ref.p, ds.d, RayEpsilon * (1 + max |p|), ds.dist * (1 - ShadowEpsilon)) go through ray_test and
        `spec` is zeroed on occluded lanes."""
        self._require_rgb("Scene.sample_emitter_direction")
        dev = torch.device("cuda", self._device_index)
        p, s2 = _planes(ref.p, 3, dev), _planes(sample, 2, dev)
        n = p.shape[1]
        if s2.shape[1] != n:
            raise RuntimeError("sample_emitter_direction: one 2D sample per reference point is required")
        act = _mask(active, dev)
        out = torch.empty((15, n), dtype=torch.float32, device=dev)
        index = torch.empty(n, dtype=torch.int32, device=dev)
        L.check(L.lib().mtsamd_sample_emitter_direction(self._handle, n, _ptr(p), _ptr(s2), _ptr(act), _ptr(out), _ptr(index), _stream()))
        g = lambda a, b: out[a:b].t().contiguous()
        ds = DirectionSample3f(p=g(0, 3), n=g(3, 6), d=g(6, 9), dist=out[9].clone(), pdf=out[10].clone(), delta=out[11] > 0.5, object=index)
        spec = g(12, 15)
        if test_visibility:
            ref_p = p.t().contiguous()
            ray = Ray3f(o=ref_p, d=ds.d, mint=(1.0 + ref_p.abs().amax(dim=1)) * RayEpsilon, maxt=ds.dist * (1.0 - ShadowEpsilon))
            # scene.cpp:179-186: only lanes with a non-zero pdf cast a shadow ray
            lanes = ds.pdf != 0.0
            if act is not None:
                lanes = lanes & act.bool()
            occluded = self.ray_test(ray, active=lanes)
            spec = torch.where(occluded.unsqueeze(1), torch.zeros_like(spec), spec)
        return ds, spec

    def pdf_emitter_direction(self, ref, ds, active=True):
        """Scene::pdf_emitter_direction (scene.cpp:191-206) of the emitters `ds.object` (per-lane indices, an Emitter handle or an
        index) for the directions of `ds`.  `ref` is accepted for the reference's signature; the densities here depend on `ds` alone."""
        self._require_rgb("Scene.pdf_emitter_direction")
        dev = torch.device("cuda", self._device_index)
        d, nrm = _planes(ds.d, 3, dev), _planes(ds.n, 3, dev)
        n = d.shape[1]
        index = _emitter_lanes(ds.object, n, dev)
        dist = torch.as_tensor(ds.dist, dtype=torch.float32, device=dev).reshape(-1).contiguous()
        delta = _mask(ds.delta, dev) if ds.delta is not None else None
        act = _mask(active, dev)
        pdf = torch.empty(n, dtype=torch.float32, device=dev)
        L.check(L.lib().mtsamd_pdf_emitter_direction(self._handle, n, _ptr(index), _ptr(d), _ptr(nrm), _ptr(dist), _ptr(delta), _ptr(act),
                                                     _ptr(pdf), _stream()))
        return pdf


# --------------------------------------------------------------------------------------------
# Operator API: BSDF / emitter / sampler queries on device streams (include/mitsuba/render/bsdf.h, records.h, emitter.h, shape.h;
# bindings src/librender/python/bsdf_v.cpp, records_v.cpp, emitter_v.cpp, shape_v.cpp).  RGB variant.
class TransportMode(enum.IntEnum):
    """bsdf.h:20-29"""
    Radiance = 0
    Importance = 1


class BSDFFlags(enum.IntFlag):
    """bsdf.h:38-124"""
    None_ = 0x00000
    Null = 0x00001
    DiffuseReflection = 0x00002
    DiffuseTransmission = 0x00004
    GlossyReflection = 0x00008
    GlossyTransmission = 0x00010
    DeltaReflection = 0x00020
    DeltaTransmission = 0x00040
    Delta1DReflection = 0x00080
    Delta1DTransmission = 0x00100
    Anisotropic = 0x01000
    SpatiallyVarying = 0x02000
    NonSymmetric = 0x04000
    FrontSide = 0x08000
    BackSide = 0x10000
    NeedsDifferentials = 0x20000
    Reflection = DiffuseReflection | DeltaReflection | Delta1DReflection | GlossyReflection
    Transmission = DiffuseTransmission | DeltaTransmission | Delta1DTransmission | GlossyTransmission | Null
    Diffuse = DiffuseReflection | DiffuseTransmission
    Glossy = GlossyReflection | GlossyTransmission
    Smooth = Diffuse | Glossy
    Delta = Null | DeltaReflection | DeltaTransmission
    Delta1D = Delta1DReflection | Delta1DTransmission
    All = Diffuse | Glossy | Delta | Delta1D


def has_flag(flags, f):
    """has_flag (bsdf.h:133) for a flag word or a tensor of flag words"""
    return (flags & int(f)) != 0


def bsdf_flags(record):
    """BSDF::flags() of a normalised record (mitsuba2_amd.bsdfs.normalize): the union of the component flags the plugin constructors
    set (src/bsdfs/*.cpp); blendbsdf / mask: the union over the children (mask adds Null)"""
    from . import bsdfs as B
    F = BSDFFlags
    t = record["type"]
    if t in (B.BLEND, B.MASK):
        flags = int(F.Null) if t == B.MASK else 0
        for c in record["children"]:
            flags |= bsdf_flags(c)
    else:
        aniso = int(F.Anisotropic) if record["alpha_u"] != record["alpha_v"] else 0
        flags = {B.DIFFUSE: F.DiffuseReflection | F.FrontSide, B.CONDUCTOR: F.DeltaReflection | F.FrontSide,
                 B.ROUGHCONDUCTOR: F.GlossyReflection | F.FrontSide | aniso,
                 B.DIELECTRIC: F.DeltaReflection | F.DeltaTransmission | F.FrontSide | F.BackSide | F.NonSymmetric,
                 B.THINDIELECTRIC: F.DeltaReflection | F.Null | F.FrontSide | F.BackSide,
                 B.PLASTIC: F.DeltaReflection | F.DiffuseReflection | F.FrontSide,
                 B.ROUGHPLASTIC: F.GlossyReflection | F.DiffuseReflection | F.FrontSide,
                 B.ROUGHDIELECTRIC: F.GlossyReflection | F.GlossyTransmission | F.FrontSide | F.BackSide | F.NonSymmetric | aniso}[t]
        flags = int(flags)
    if record.get("twosided"):
        flags |= int(F.FrontSide | F.BackSide)
    return flags


class BSDFContext:
    """bsdf.h:146-190.  Only the defaults are built: mode = Radiance, type_mask = all components, component = -1 (all)."""

    def __init__(self, mode=TransportMode.Radiance, type_mask=0x1FF, component=0xFFFFFFFF):
        self.mode, self.type_mask, self.component = mode, type_mask, component
        self._check()

    def _check(self):
        if int(self.mode) != int(TransportMode.Radiance):
            raise RuntimeError("BSDFContext: TransportMode.Importance is not built in this backend (Radiance only)")
        if int(self.type_mask) != 0x1FF or int(self.component) not in (0xFFFFFFFF, -1):
            raise RuntimeError("BSDFContext: component selection is not built in this backend (type_mask and component must keep "
                               "their defaults: all components)")


@dataclass
class BSDFSample3f:
    """bsdf.h:193-252"""
    wo: torch.Tensor            # (N,3) local frame
    pdf: torch.Tensor
    eta: torch.Tensor
    sampled_type: torch.Tensor  # BSDFFlags per lane: a Delta lobe (Null included) or the Smooth lobes of the hemisphere of wo; 0 = invalid
    sampled_component: Optional[torch.Tensor] = None
    # the kernel's own flags, for callers that want them without decoding sampled_type: the sampled lobe is discrete; the sample is valid
    delta: Optional[torch.Tensor] = None
    valid: Optional[torch.Tensor] = None


@dataclass
class DirectionSample3f:
    """records.h:20-209: PositionSample3f (p, n, pdf, delta, object) + d, dist.  `object` holds emitter indices (int32, -1 = none),
    an Emitter handle or None."""
    p: torch.Tensor
    n: torch.Tensor
    d: torch.Tensor = None
    dist: torch.Tensor = None
    pdf: torch.Tensor = None
    delta: torch.Tensor = None
    object: object = None

    def __init__(self, p=None, n=None, d=None, dist=None, pdf=None, delta=None, object=None):
        if isinstance(p, SurfaceInteraction3f):
            # DirectionSample(it, ref) (records.h:168-174): n is the SHADING normal of `it` (PositionSample(si), records.h:92-99); d and
            # dist come from it.p - ref.p, and lanes where `it` is not valid point along -it.wi (environment emitters)
            it, ref = p, n
            diff = it.p - ref.p
            dist = _dot3(diff, diff).sqrt()
            d = diff * (1.0 / dist).unsqueeze(1)
            d = torch.where(it.is_valid().unsqueeze(1), d, -it.wi)
            self.p, self.n, self.d, self.dist = it.p, it.sh_frame_n, d, dist
            self.pdf, self.delta, self.object = torch.zeros_like(dist), torch.zeros_like(dist, dtype=torch.bool), object
            return
        self.p, self.n, self.d, self.dist, self.pdf, self.delta, self.object = p, n, d, dist, pdf, delta, object


def _emitter_lanes(obj, n, dev):
    """DirectionSample3f.object / an emitter argument -> (n,) int32 emitter indices on `dev`"""
    if isinstance(obj, Emitter):
        obj = obj._lanes if obj._lanes is not None else obj._index
    if obj is None:
        obj = -1
    if isinstance(obj, (int, np.integer)):
        return torch.full((n,), int(obj), dtype=torch.int32, device=dev)
    t = torch.as_tensor(obj, device=dev).reshape(-1).to(torch.int32).contiguous()
    if t.shape[0] != n:
        raise RuntimeError("expected one emitter index per lane (%d), got %d" % (n, t.shape[0]))
    return t


class Shape:
    """include/mitsuba/render/shape.h: the accessors an integrator uses"""

    def __init__(self, scene, index):
        self._scene, self._index = scene, int(index)

    def bsdf(self):
        return BSDF(scene=self._scene, shape=self._index)

    def is_emitter(self):
        return int(self._scene._operator_tables()["emitter_host"][self._index]) >= 0

    def emitter(self):
        e = int(self._scene._operator_tables()["emitter_host"][self._index])
        return Emitter(self._scene, index=e) if e >= 0 else None


class Emitter:
    """include/mitsuba/render/emitter.h: one emitter of a scene (`index`), or a per-lane handle (`lanes`: int32 indices, -1 = none) as
    SurfaceInteraction3f.emitter returns it."""

    def __init__(self, scene, index=None, lanes=None):
        self._scene, self._index, self._lanes = scene, (None if index is None else int(index)), lanes

    def is_environment(self):
        return self._index is not None and self._index == self._scene._environment

    def eval(self, si, active=True):
        """Emitter::eval(si) (area.cpp:71-76, constant.cpp:53-57, envmap.cpp:132-146): an area emitter gives its radiance where
        si.wi.z > 0; the environment emitter is looked up along the direction of the ray that made `si` (a hand-made interaction:
        -si.wi, as the reference); delta emitters and "none" give 0."""
        scene = self._scene
        scene._require_rgb("Emitter.eval")
        dev = torch.device("cuda", scene._device_index)
        wi = _planes(si.wi, 3, dev)
        n = wi.shape[1]
        d = _planes(si._ray_d if getattr(si, "_ray_d", None) is not None else -torch.as_tensor(si.wi, device=dev), 3, dev)
        index = _emitter_lanes(self, n, dev)
        act = _mask(active, dev)
        out = torch.empty((3, n), dtype=torch.float32, device=dev)
        L.check(L.lib().mtsamd_emitter_eval(scene._handle, n, _ptr(index), _ptr(wi), _ptr(d), _ptr(act), _ptr(out), _stream()))
        return out.t().contiguous()


class BSDF:
    """include/mitsuba/render/bsdf.h: eval / pdf / sample / flags on device streams.  Three forms share the kernels: the BSDF of one
    shape (``shape.bsdf()``), a per-lane handle over shape indices (``si.bsdf()``), and a BSDF loaded on its own
    (``xml.load_string('<bsdf ...>')`` / ``xml.load_dict``), which is backed by a private one-triangle scene so that its record, textures
    and roughplastic tables go through the one ingestion path."""

    def __init__(self, scene=None, shape=None, lanes=None, plugin=None, device=0, variant="rgb"):
        self._scene, self._shape, self._lanes = scene, shape, lanes
        self._plugin, self._device, self._variant = plugin, int(device), variant
        if plugin is not None:
            from . import bsdfs as B
            self._record = B.normalize(plugin)      # constructor-time validation, as the plugin constructors
            self._shape = 0
        elif scene is None:
            raise RuntimeError("BSDF: a scene (with a shape index or per-lane shape indices) or a plugin dictionary is required")

    def record(self):
        """the normalised plugin parameters (mitsuba2_amd.bsdfs.normalize) of a single BSDF"""
        if self._plugin is not None:
            return self._record
        if self._lanes is not None:
            raise RuntimeError("BSDF.record(): a per-lane handle has no single record")
        return self._scene._bsdf_records[int(self._scene._operator_tables()["bsdf"][self._shape])]

    def _backing(self):
        if self._scene is None:      # a BSDF on its own: one triangle carries it
            tri = dict(positions=_f32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), faces=np.array([[0, 1, 2]], dtype=np.uint32), normals=None,
                       texcoords=_f32([[0, 0], [1, 0], [0, 1]]), bsdf=0, emitter=-1)
            self._scene = Scene(dict(meshes=[tri], bsdfs=[self._plugin], emitters=[]), device=self._device, variant=self._variant)
        self._scene._require_rgb("BSDF")
        return self._scene

    def flags(self):
        """BSDF::flags(): one flag word, or one per lane for a per-lane handle (0 on lanes without a shape)"""
        if self._plugin is not None:
            return bsdf_flags(self._record)
        tables = self._scene._operator_tables()
        if self._lanes is None:
            return int(tables["flags_host"][self._shape])
        shape = self._lanes.to(torch.int64)
        valid = (shape >= 0) & (shape < self._scene.shape_count())
        table = tables["flags"].to(shape.device)
        return torch.where(valid, table[shape.clamp(0, max(self._scene.shape_count() - 1, 0))], torch.zeros_like(table[:1]))

    def _query(self, ctx, si, active, extra):
        """the query struct of n rows; returns (struct, tensors kept alive, n, device)"""
        if not isinstance(ctx, BSDFContext):
            raise RuntimeError("BSDF: the first argument is a BSDFContext")
        ctx._check()
        scene = self._backing()
        dev = torch.device("cuda", scene._device_index)
        wi = _planes(si.wi, 3, dev)
        n = wi.shape[1]
        uv = _planes(si.uv, 2, dev) if getattr(si, "uv", None) is not None else None      # no uv: zeros (a dummy interaction with just wi)
        if self._lanes is not None:
            shape = torch.as_tensor(self._lanes, device=dev).reshape(-1).to(torch.int32).contiguous()
            if shape.shape[0] != n:
                raise RuntimeError("BSDF: the per-lane handle has %d lanes, the interaction %d" % (shape.shape[0], n))
        else:
            shape = torch.full((n,), int(self._shape), dtype=torch.int32, device=dev)
        act = _mask(active, dev)
        planes = [_planes(e, k, dev) for e, k in extra]
        for pl in planes + ([uv] if uv is not None else []):
            if pl.shape[1] != n:
                raise RuntimeError("BSDF: every argument needs one row per lane of the interaction (%d)" % n)
        rows = [r for pl in planes for r in pl]
        q = L.BsdfQuery()
        q.shape, q.wi_x, q.wi_y, q.wi_z = _ptr(shape), _ptr(wi[0]), _ptr(wi[1]), _ptr(wi[2])
        if uv is not None:
            q.u, q.v = _ptr(uv[0]), _ptr(uv[1])
        q.active = _ptr(act)
        return q, rows, (shape, wi, uv, act, planes), n, dev, scene

    def eval_pdf(self, ctx, si, wo, active=True):
        """BSDF::eval and BSDF::pdf in one launch -> (value (N,3), pdf (N,))"""
        q, rows, keep, n, dev, scene = self._query(ctx, si, active, [(wo, 3)])
        q.wo_x, q.wo_y, q.wo_z = _ptr(rows[0]), _ptr(rows[1]), _ptr(rows[2])
        out = torch.empty((4, n), dtype=torch.float32, device=dev)
        L.check(L.lib().mtsamd_bsdf_eval_pdf(scene._handle, n, C.byref(q), _ptr(out), _stream()))
        return out[0:3].t().contiguous(), out[3].clone()

    def eval(self, ctx, si, wo, active=True):
        """BSDF::eval (bsdf.h:360): the BSDF times the cosine foreshortening factor, (N,3)"""
        return self.eval_pdf(ctx, si, wo, active)[0]

    def pdf(self, ctx, si, wo, active=True):
        """BSDF::pdf (bsdf.h:391)"""
        return self.eval_pdf(ctx, si, wo, active)[1]

    def sample(self, ctx, si, sample1, sample2, active=True):
        """BSDF::sample (bsdf.h:329) -> (BSDFSample3f, weight (N,3)); an invalid sample has weight 0 and sampled_type 0"""
        q, rows, keep, n, dev, scene = self._query(ctx, si, active, [(sample1, 1), (sample2, 2)])
        q.sample1, q.sample2_x, q.sample2_y = _ptr(rows[0]), _ptr(rows[1]), _ptr(rows[2])
        out = torch.empty((10, n), dtype=torch.float32, device=dev)
        L.check(L.lib().mtsamd_bsdf_sample(scene._handle, n, C.byref(q), _ptr(out), _stream()))
        wo = out[0:3].t().contiguous()
        delta, valid = out[5] > 0.5, out[9] > 0.5
        F = BSDFFlags
        same = (wo[:, 2] * keep[1][2]) > 0
        null = (wo == -keep[1].t()).all(dim=1)
        kind = torch.where(delta, torch.where(same, int(F.DeltaReflection), torch.where(null, int(F.Null), int(F.DeltaTransmission))),
                           torch.where(same, int(F.DiffuseReflection | F.GlossyReflection), int(F.DiffuseTransmission | F.GlossyTransmission)))
        kind = torch.where(valid, kind, torch.zeros_like(kind)).to(torch.int32)
        bs = BSDFSample3f(wo=wo, pdf=out[3].clone(), eta=out[4].clone(), sampled_type=kind, delta=delta, valid=valid)
        return bs, out[6:9].t().contiguous()


# --------------------------------------------------------------------------------------------
class PathIntegrator:
    """src/integrators/path.cpp + MonteCarloIntegrator (src/librender/integrator.cpp:283-296)."""

    def __init__(self, max_depth=-1, rr_depth=5, paths_per_wave=0, pipeline=0, samples_per_pass=-1, timeout=-1.0, profile=False):
        if max_depth < 0 and max_depth != -1:
            raise RuntimeError("\"max_depth\" must be set to -1 (infinite) or a value >= 0")
        if rr_depth <= 0:
            raise RuntimeError("\"rr_depth\" must be set to a value greater than zero!")
        self.max_depth, self.rr_depth = int(max_depth), int(rr_depth)
        self.paths_per_wave = int(paths_per_wave)
        self.pipeline = int(pipeline)          # 0 automatic, 1 fused kernel, 2 split trace/shade kernels (same samples)
        # SamplingIntegrator properties (integrator.cpp:27-39): samples_per_pass (-1: all), timeout in seconds (-1: none)
        self.samples_per_pass, self.timeout = int(samples_per_pass), float(timeout)
        self.profile = bool(profile)           # per-launch HIP event timing of the split pipeline (stats: trace_*_ns)
        # scheduler knobs of mtsamd_render_desc (0 = library default; the image does not depend on them): a pass holds at most
        # 2^max_pass_log2 samples; finish_kernel 1 = never end a pass with k_finish, 2 = as soon as the sample cursors are dry
        self.max_pass_log2, self.finish_kernel = 0, 0
        self._scene = None
        self.stats = None

    def _desc(self, sensor, rows=None, partition=None):
        d = L.RenderDesc()
        sensor._fill_desc(d)
        d.max_depth, d.rr_depth = self.max_depth, self.rr_depth
        d.row_begin, d.row_end = (0, 0) if rows is None else (int(rows[0]), int(rows[1]))
        if partition is not None:       # (index, count, tile_rows): interleaved row tiles of the film
            d.part_index, d.part_count, d.part_tile_rows = (int(x) for x in partition)
        d.paths_per_wave = self.paths_per_wave
        d.pipeline = self.pipeline
        d.samples_per_pass, d.timeout, d.profile = self.samples_per_pass, self.timeout, int(self.profile)
        d.max_pass_log2, d.finish_kernel = int(self.max_pass_log2), int(self.finish_kernel)
        self._fill_integrator(d)
        return d

    def _fill_integrator(self, d):
        d.integrator = 0

    def aov_names(self):
        """SamplingIntegrator::aov_names (integrator.h:128-133)"""
        return []

    def aov_channels(self):
        """film channels of a render: X, Y, Z, A, W followed by the AOVs (integrator.cpp:72-77)"""
        return ["X", "Y", "Z", "A", "W"] + self.aov_names()

    def render(self, scene, sensor=None, rows=None, partition=None):
        """Integrator::render (integrator.h:42): renders into sensor.film(); returns False if cancelled.
        rows=(begin, end) / partition=(index, count, tile_rows) restrict the call to a part of the film
        (multi-GPU film partition); the film then holds that part's contribution only."""
        sensor = sensor if sensor is not None else scene.sensors()[0]
        film = sensor.film()
        film.prepare(self.aov_channels(), device="cuda:%d" % scene._device_index)
        d = self._desc(sensor, rows, partition)
        stats = (C.c_uint64 * 16)()
        self._scene = scene
        rc = L.lib().mtsamd_render(scene._handle, C.byref(d), _ptr(film._storage.data()), stats, _stream())
        self._scene = None
        if rc == -4:                     # MTSAMD_ERR_CANCELLED: render() returns false (integrator.cpp:175)
            return False
        L.check(rc)
        self.stats = dict(zip(("closest_hit_rays", "any_hit_rays", "samples", "iterations", "segments", "bounce_ns", "film_ns", "tri_tests",
                               "trace_closest_ns", "trace_closest_launches", "trace_any_ns", "trace_any_launches", "shade_ns", "shade_launches",
                               "passes", "timed_out"), [int(x) for x in stats]))
        return True

    def cancel(self):
        if self._scene is not None:
            L.lib().mtsamd_cancel(self._scene._handle)

    def sample(self, scene, sensor, first, count):
        """SamplingIntegrator::sample for whole sample indices: returns (rgb (N,3), mask (N,), position (N,2))."""
        d = self._desc(sensor)
        dev = torch.device("cuda", scene._device_index)
        rgba = torch.empty((count, 4), dtype=torch.float32, device=dev)
        pos = torch.empty((count, 2), dtype=torch.float32, device=dev)
        L.check(L.lib().mtsamd_sample_radiance(scene._handle, C.byref(d), int(first), int(count), _ptr(rgba), _ptr(pos), _stream()))
        return rgba[:, :3], rgba[:, 3] > 0.5, pos


class DirectIntegrator(PathIntegrator):
    """src/integrators/direct.cpp: direct illumination with multiple importance sampling of emitter and BSDF samples."""

    def __init__(self, shading_samples=None, emitter_samples=None, bsdf_samples=None, hide_emitters=False, paths_per_wave=0):
        super().__init__(paths_per_wave=paths_per_wave)
        if shading_samples is not None and (emitter_samples is not None or bsdf_samples is not None):      # direct.cpp:80-86
            raise RuntimeError("Cannot specify both 'shading_samples' and ('emitter_samples' and/or 'bsdf_samples').")
        base = 1 if shading_samples is None else int(shading_samples)
        self.emitter_samples = base if emitter_samples is None else int(emitter_samples)
        self.bsdf_samples = base if bsdf_samples is None else int(bsdf_samples)
        if self.emitter_samples < 0 or self.bsdf_samples < 0 or self.emitter_samples + self.bsdf_samples == 0:
            raise RuntimeError("Must have at least 1 BSDF or emitter sample!")
        self.hide_emitters = bool(hide_emitters)

    def _fill_integrator(self, d):
        d.integrator = 1
        d.emitter_samples, d.bsdf_samples, d.hide_emitters = self.emitter_samples, self.bsdf_samples, int(self.hide_emitters)


class DepthIntegrator(PathIntegrator):
    """src/integrators/depth.cpp: distance to the first intersection"""

    def _fill_integrator(self, d):
        d.integrator = 2


class MomentIntegrator(PathIntegrator):
    """src/integrators/moment.cpp: wraps a sampling integrator and adds its XYZ result and the second moments of it as AOVs
    (``<name>.X/Y/Z`` and ``m2_<name>.X/Y/Z``), from which a per-pixel variance estimate follows."""

    def __init__(self, nested, name="nested"):
        if not isinstance(nested, PathIntegrator) or isinstance(nested, MomentIntegrator):
            raise RuntimeError("Child objects must be of type 'SamplingIntegrator'!")
        super().__init__(paths_per_wave=nested.paths_per_wave, pipeline=nested.pipeline)
        self.nested, self.name = nested, name

    def aov_names(self):
        base = ["%s.%s" % (self.name, c) for c in "XYZ"]
        return base + ["m2_" + n for n in base]

    def _desc(self, sensor, rows=None, partition=None):
        d = self.nested._desc(sensor, rows, partition)
        d.moment = 1
        return d

    @staticmethod
    def mean_and_variance(film):
        """what test_renders.py:55-60 (bitmap_extract) takes from the developed film: the nested integrator's XYZ image and
        m2 - mean^2, both normalised by the accumulated filter weight"""
        raw = film.bitmap(raw=True)
        w = raw[..., 4:5]
        inv = torch.where(w != 0, 1.0 / torch.where(w != 0, w, torch.ones_like(w)), torch.zeros_like(w))
        mean, m2 = raw[..., 5:8] * inv, raw[..., 8:11] * inv
        return mean, m2 - mean * mean


AOV_TYPES = {"depth": (0, [""]), "position": (1, [".X", ".Y", ".Z"]), "uv": (2, [".U", ".V"]), "geo_normal": (3, [".X", ".Y", ".Z"]),
             "sh_normal": (4, [".X", ".Y", ".Z"]), "dp_du": (5, [".X", ".Y", ".Z"]), "dp_dv": (6, [".X", ".Y", ".Z"]),
             "duv_dx": (7, [".U", ".V"]), "duv_dy": (8, [".U", ".V"])}      # mtsamd_aov_type, channel suffixes (aov.cpp:92-134)


class AOVIntegrator(PathIntegrator):
    """src/integrators/aov.cpp: fields of the camera ray's surface interaction -- ``depth``, ``position``, ``uv``, ``geo_normal``,
    ``sh_normal``, ``dp_du``, ``dp_dv`` -- as film channels beside the render of a nested integrator.  ``aovs`` is a string of
    ``<name>:<type>`` pairs separated by commas or spaces.  ``duv_dx`` and ``duv_dy`` are accepted and always zero, as in the
    reference (kdtree.h:2353 zeroes them and aov.cpp never calls compute_partials).  `nested` (a path, direct or depth integrator, named
    `name`) adds ``<name>.R/G/B/A`` after the AOVs and fills X, Y, Z, A; exactly one nested integrator is supported.  Spectral variant:
    ``<name>.R/G/B`` is the linear transform of the XYZ sample, where the reference converts the spectrum itself (equal up to rounding)."""

    def __init__(self, aovs, nested=None, name="integrator_0"):
        if isinstance(nested, (list, tuple)):
            if len(nested) > 1:
                raise RuntimeError("aov: exactly one nested integrator is supported by this backend")
            nested = nested[0] if nested else None
        if nested is not None and (not isinstance(nested, PathIntegrator) or isinstance(nested, (MomentIntegrator, AOVIntegrator))):
            raise RuntimeError("aov: the nested integrator must be a path, direct or depth integrator")
        knobs = nested if nested is not None else PathIntegrator()
        super().__init__(paths_per_wave=knobs.paths_per_wave, pipeline=knobs.pipeline)
        self.nested, self.name = nested, str(name)
        self._names, self._types = [], []
        for tok in [t for t in str(aovs).replace(",", " ").split() if t]:      # string::tokenize(aovs, " ,") (aov.cpp:88-91)
            item = tok.split(":")
            if len(item) != 2 or not item[0] or not item[1]:
                raise RuntimeError("Invalid AOV specification: require <name>:<type> pair")
            if item[1] not in AOV_TYPES:
                raise RuntimeError('Invalid AOV type "%s"!' % item[1])
            kind, suffixes = AOV_TYPES[item[1]]
            self._types.append(kind)
            self._names += [item[0] + sfx for sfx in suffixes]
        if not self._types and nested is None:
            raise RuntimeError("aov: no AOV and no nested integrator")

    def aov_names(self):
        """aov.cpp:221-223: the string's AOVs, then per nested integrator its own AOVs (none here) and <name>.R/G/B/A (aov.cpp:136-151)"""
        out = list(self._names)
        if self.nested is not None:
            out += ["%s.%s" % (self.name, n) for n in self.nested.aov_names()] + ["%s.%s" % (self.name, c) for c in "RGBA"]
        return out

    def _desc(self, sensor, rows=None, partition=None):
        d = (self.nested if self.nested is not None else PathIntegrator(paths_per_wave=self.paths_per_wave))._desc(sensor, rows, partition)
        if self.nested is None:
            d.max_pass_log2, d.samples_per_pass, d.timeout = int(self.max_pass_log2), self.samples_per_pass, self.timeout
        return d

    def _aov_types(self):
        return (C.c_int32 * max(len(self._types), 1))(*self._types), len(self._types)

    def render(self, scene, sensor=None, rows=None, partition=None):
        sensor = sensor if sensor is not None else scene.sensors()[0]
        film = sensor.film()
        film.prepare(self.aov_channels(), device="cuda:%d" % scene._device_index)
        d = self._desc(sensor, rows, partition)
        stats = (C.c_uint64 * 16)()
        types, n = self._aov_types()
        self._scene = scene
        rc = L.lib().mtsamd_render_aov(scene._handle, C.byref(d), types, n, 0 if self.nested is None else 1, _ptr(film._storage.data()),
                                       stats, _stream())
        self._scene = None
        if rc == -4:
            return False
        L.check(rc)
        self.stats = dict(zip(("closest_hit_rays", "any_hit_rays", "samples", "iterations", "segments", "bounce_ns", "film_ns", "tri_tests",
                               "trace_closest_ns", "trace_closest_launches", "trace_any_ns", "trace_any_launches", "shade_ns", "shade_launches",
                               "passes", "timed_out"), [int(x) for x in stats]))
        return True

    def sample_aovs(self, scene, sensor, first, count):
        """The AOV part of AOVIntegrator::sample (aov.cpp:166-193) for whole sample indices: (values (N, C), position (N, 2)), C = the
        channels of the `aovs` string in order."""
        d = self._desc(sensor)
        dev = torch.device("cuda", scene._device_index)
        values = torch.empty((count, len(self._names)), dtype=torch.float32, device=dev)
        pos = torch.empty((count, 2), dtype=torch.float32, device=dev)
        types, n = self._aov_types()
        L.check(L.lib().mtsamd_sample_aovs(scene._handle, C.byref(d), types, n, int(first), int(count), _ptr(values), _ptr(pos), _stream()))
        return values, pos

    def sample(self, scene, sensor, first, count):
        """the nested integrator's result (aov.cpp:195-213: the first nested integrator's radiance is the integrator's own)"""
        if self.nested is None:
            raise RuntimeError("aov: no nested integrator to sample")
        return self.nested.sample(scene, sensor, first, count)


def make_sensor(params):
    """Build PerspectiveCamera/HDRFilm/IndependentSampler from a scenes.*_sensor() dict."""
    rp = params.get("rfilter_param")
    flt = make_filter(params["rfilter"], *([] if rp is None else (list(rp) if isinstance(rp, (list, tuple)) else [rp])))
    cx, cy, cw, ch = params["crop"]
    film = HDRFilm(params["width"], params["height"], (cx, cy), (cw, ch), flt)
    sampler = IndependentSampler(params["sample_count"], params["seed"])
    kw = dict(to_world=params["to_world"], fov=params["fov"], near_clip=params["near_clip"], far_clip=params["far_clip"], film=film, sampler=sampler)
    if params.get("aperture_radius") is not None:
        return ThinLensCamera(aperture_radius=params["aperture_radius"], focus_distance=params.get("focus_distance"), **kw)
    return PerspectiveCamera(**kw)

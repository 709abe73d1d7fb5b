"""Tensor clip augmentation with the names, arguments and random draws of the reference's coclr_utils/transforms.py, computed by
one fused HIP kernel (csrc/cliptf.hip) instead of a torch launch per op.

A clip is uint8 [N, H, W, 3] before ToFloatTensor / ToFloatTensorInZeroOne and float32 [3, N, H, W] after.  Every transform appends to a
small per-clip program; `Compose` runs the whole chain as one fused group (geometry folded into one index map on either side of at
most one bilinear resample, up to four colour ops, an optional normalise) and `Compose.batch(clips)` does so for a whole batch with one
parameter upload and at most two launches (a contrast op needs the per-frame mean first).  A chain that does not have that shape
(two resizes, geometry after a colour op, two contrast ops, ...) splits into consecutive groups, each its own launch.  A single
function call is a one-op program of the same kernel.

All randomness is drawn on the host from `random` and `np.random` by the reference's calls in the reference's order.

Where this module departs from the reference on purpose: colour ops on integer tensors raise TypeError (the reference's integer
blend truncates the ratio); random_grayscale takes the luma of each drawn frame over its colour channels (the reference hands its
frame axis to rgb_to_grayscale as the colour axis: the call asserts unless the clip has three frames, and then weights frames);
transforms return new tensors, never views.

5-D input [B, 3, N, H, W] is accepted by hflip / RandomHorizontalFlip and Normalize(channel=1) only, as coclr_classify.py uses them;
everything else on a 5-D tensor raises ValueError: use Compose.batch.

Test-time views (coclr_classify.py:540-556): FiveCrop, RandomHorizontalFlip(command=), and multi_view(clip, composes), which runs n
chains on ONE source clip as one launch; ten_crop_views lists the ten chains of the ten-crop protocol.  Two departures there: the
resample to img_dim is this module's bilinear (the reference's A.Scale is PIL bicubic on uint8 images), and the reference's
test-time ColorJitter(.., p=0.3), a random perturbation of an evaluation, is not applied.
"""
import math
import numbers
import random

import numpy as np
import torch

from .. import _lib

BRIGHTNESS, CONTRAST, SATURATION, GRAY = 0, 1, 2, 3          # SLIC_CLIPTF_* of include/slic_hip.h
SRC_U8, SRC_U8_255, SRC_F32 = 0, 1, 2
MAX_OPS = 4
_RAW, _GEO, _COLOUR, _DONE = 0, 1, 2, 3                      # how far a group's chain has come

_MAP = [("y0", "<i4"), ("y1", "<i4"), ("x0", "<i4"), ("x1", "<i4"), ("dy", "<i4"), ("dx", "<i4"), ("mx", "<i4"), ("fill", "<f4")]
_REC = np.dtype([("src", "<u8"), ("src_bytes", "<u8"), ("Hs", "<i4"), ("Ws", "<i4"), ("flags", "<i4"), ("Ha", "<i4"), ("Wa", "<i4"),
                 ("sc_y", "<f4"), ("sc_x", "<f4"), ("nops", "<i4"), ("a", _MAP), ("b", _MAP),
                 ("op_kind", "<i4", (MAX_OPS,)), ("op_fac", "<i4", (MAX_OPS,))])
_HEAD_FLOATS = 8
assert _REC.itemsize == 144                                  # SLIC_CLIPTF_REC_BYTES


class Map:
    """an H x W image whose pixel (y, x) is target pixel (y + dy, mx * x + dx) inside the rectangle [y0, y1) x [x0, x1) and `fill`
    outside it; crop, pad and flip fold into it"""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self.y0, self.y1, self.x0, self.x1 = 0, H, 0, W
        self.dy, self.dx, self.mx, self.fill = 0, 0, 1, 0.0

    @property
    def full(self):
        return (self.y0, self.y1, self.x0, self.x1) == (0, self.H, 0, self.W)

    @property
    def empty(self):
        return self.y0 >= self.y1 or self.x0 >= self.x1

    def crop(self, i, j, h, w):
        self.y0, self.y1 = min(max(self.y0 - i, 0), h), min(max(self.y1 - i, 0), h)
        self.x0, self.x1 = min(max(self.x0 - j, 0), w), min(max(self.x1 - j, 0), w)
        self.dy += i
        self.dx += self.mx * j
        self.H, self.W = h, w
        if self.empty:
            self.y0 = self.y1 = self.x0 = self.x1 = 0

    def flip(self):
        self.dx += self.mx * (self.W - 1)
        self.mx = -self.mx
        self.x0, self.x1 = self.W - self.x1, self.W - self.x0

    def can_pad(self, fill):
        return self.full or np.float32(fill) == np.float32(self.fill)

    def pad(self, left, right, top, bottom, fill):
        self.fill = float(np.float32(fill))
        self.y0, self.y1, self.x0, self.x1 = self.y0 + top, self.y1 + top, self.x0 + left, self.x1 + left
        self.dy -= top
        self.dx -= self.mx * left
        self.H, self.W = self.H + top + bottom, self.W + left + right

    def record(self):
        return (self.y0, self.y1, self.x0, self.x1, self.dy, self.dx, self.mx, self.fill)


class ClipGroup:
    """one clip's share of one launch: source, folded geometry, colour ops"""

    def __init__(self, src, kind, N, Hs, Ws, stage):
        self.src, self.kind, self.N, self.Hs, self.Ws, self.stage = src, kind, N, Hs, Ws, stage
        self.a = None                    # with a resample: the map the taps read through; (Ha, Wa, sc_y, sc_x) in self.resample
        self.resample = None
        self.cur = Map(Hs, Ws)           # the map being folded; the group's map b when it runs
        self.ops = []                    # (kind, float32 factors [N])
        self.norm = None                 # (mean [3], std [3]) float32

    @property
    def b(self):
        return self.cur

    @property
    def out_hw(self):
        return self.cur.H, self.cur.W

    @property
    def has_contrast(self):
        return any(k == CONTRAST for k, _ in self.ops)

    @property
    def launches(self):
        return ("stats", "apply") if self.has_contrast else ("apply",)

    @property
    def identity(self):
        return self.resample is None and self.cur.full and (self.cur.dy, self.cur.dx, self.cur.mx) == (0, 0, 1) \
            and not self.ops and self.norm is None and self.kind == SRC_F32 and self.stage != _RAW


def _check_clip(vid):
    if not isinstance(vid, torch.Tensor):
        raise TypeError(f"expected a tensor, got {type(vid).__name__}")
    if vid.requires_grad:
        raise ValueError("clip transforms take data: the input requires grad")
    if vid.dim() == 4 and vid.dtype == torch.uint8 and vid.shape[3] == 3:
        return
    if vid.dim() == 4 and vid.dtype == torch.float32 and vid.shape[0] == 3:
        return
    raise TypeError(f"a clip is uint8 [N, H, W, 3] or float32 [3, N, H, W], got {vid.dtype} {tuple(vid.shape)}")


class _Clip:
    """the program of one clip: consecutive groups, the last one open"""

    def __init__(self, vid):
        _check_clip(vid)
        if vid.dtype == torch.uint8:
            N, H, W, _ = vid.shape
            self.groups = [ClipGroup(vid, SRC_U8, N, H, W, _RAW)]
        else:
            _, N, H, W = vid.shape
            self.groups = [ClipGroup(vid, SRC_F32, N, H, W, _GEO)]

    @property
    def g(self):
        return self.groups[-1]

    def split(self):
        H, W = self.g.out_hw
        self.groups.append(ClipGroup(None, SRC_F32, self.g.N, H, W, _GEO))
        return self.g

    @property
    def shape(self):
        g = self.g
        return (g.N, g.Hs, g.Ws, 3) if g.stage == _RAW else (3, g.N) + g.out_hw

    def geometry(self):
        if self.g.stage == _RAW:
            raise ValueError("uint8 [N, H, W, 3] clips take ToFloatTensor / ToFloatTensorInZeroOne first")
        return self.g if self.g.stage == _GEO else self.split()

    def to_float(self, div):
        if self.g.stage != _RAW:
            raise ValueError("to_float_tensor takes a uint8 [N, H, W, 3] clip")
        self.g.kind, self.g.stage = (SRC_U8_255 if div else SRC_U8), _GEO

    def crop(self, i, j, h, w):
        g = self.geometry()
        H, W = g.out_hw
        i, j, h, w = int(i), int(j), int(h), int(w)
        if i < 0 or j < 0:
            raise ValueError(f"crop: negative corner ({i}, {j})")
        h, w = min(i + h, H) - i, min(j + w, W) - j          # a slice past the edge stops at the edge
        if h <= 0 or w <= 0:
            raise ValueError("crop: empty result")
        g.cur.crop(i, j, h, w)

    def flip(self):
        self.geometry().cur.flip()

    def pad(self, left, right, top, bottom, fill):
        if min(left, right, top, bottom) < 0:
            raise ValueError("pad: negative padding is not supported (use crop)")
        if left == right == top == bottom == 0:
            return
        g = self.geometry()
        if not g.cur.can_pad(fill):
            g = self.split()
        g.cur.pad(left, right, top, bottom, fill)

    def resize(self, size):
        g = self.geometry()
        if g.resample is not None:
            g = self.split()
        H, W = g.out_hw
        if isinstance(size, int):
            # the reference passes scale_factor: the source step is 1 / scale_factor, not in / out
            sf = float(size) / min(H, W)
            Ho, Wo = int(math.floor(float(H * sf))), int(math.floor(float(W * sf)))
            sc_y = sc_x = float(np.float32(1.0 / sf))
        else:
            Ho, Wo = (int(s) for s in size)
            sc_y, sc_x = float(np.float32(H) / np.float32(Ho)), float(np.float32(W) / np.float32(Wo))
        if Ho <= 0 or Wo <= 0:
            raise ValueError(f"resize: empty result {Ho} x {Wo}")
        g.a, g.resample, g.cur = g.cur, (H, W, sc_y, sc_x), Map(Ho, Wo)

    def colour(self, kind, factors):
        g = self.g
        if g.stage == _RAW:
            raise TypeError("colour ops take float clips (integer blending is not supported): call ToFloatTensorInZeroOne first")
        factors = np.ascontiguousarray(factors, dtype=np.float32).reshape(-1)
        if factors.shape[0] != g.N:
            raise ValueError(f"{factors.shape[0]} factors for {g.N} frames")
        if g.stage == _DONE or len(g.ops) == MAX_OPS or (kind == CONTRAST and g.has_contrast):
            g = self.split()
        g.ops.append((kind, factors))
        g.stage = _COLOUR

    def normalize(self, mean, std):
        g = self.g
        if g.stage == _RAW:
            raise ValueError("normalize takes a float [3, N, H, W] clip")
        if g.stage == _DONE:
            g = self.split()
        g.norm = (np.asarray(mean, dtype=np.float32).reshape(3), np.asarray(std, dtype=np.float32).reshape(3))
        g.stage = _DONE


class HipClipKernels:
    """the device side (csrc/cliptf.hip).  `kernels=` takes another provider with the same two methods (tests run the host logic on
    the CPU that way)."""

    def check(self, *tensors):
        _lib.require_device(*tensors)

    def run(self, groups, kind, N, Ho, Wo, norm):
        """one fused group for len(groups) clips -> float32 [B, 3, N, Ho, Wo]"""
        srcs = [g.src if g.src.is_contiguous() else g.src.contiguous() for g in groups]
        dev = srcs[0].device
        if any(s.device != dev for s in srcs):
            raise ValueError("clips of one batch live on different devices")
        host, contrast = self.table(groups, srcs, N, norm)
        with torch.cuda.device(dev):
            return self.launch(host, contrast, srcs, len(groups), N, Ho, Wo, kind, norm is not None)

    @staticmethod
    def table(groups, srcs, N, norm):
        """(the pinned host table of csrc/cliptf.hip's header comment, whether a clip has a contrast op)"""
        B = len(groups)
        first_fac = _HEAD_FLOATS + B * _REC.itemsize // 4
        nbytes = (first_fac + sum(len(g.ops) for g in groups) * N) * 4
        host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        raw = host.numpy()
        head = raw[:_HEAD_FLOATS * 4].view("<f4")
        head[:] = 0
        if norm is not None:
            head[0:3], head[3:6] = norm
        fac = raw.view("<f4")
        at = first_fac
        contrast = False
        rows = []
        no_map = (0, 0, 0, 0, 0, 0, 1, 0.0)
        for g, s in zip(groups, srcs):
            kinds, facs = [0] * MAX_OPS, [0] * MAX_OPS
            for k, (op, f) in enumerate(g.ops):
                kinds[k], facs[k] = op, at
                fac[at:at + N] = f
                at += N
                contrast |= op == CONTRAST
            if g.resample is not None:
                Ha, Wa, sc_y, sc_x = g.resample
                geo = (1 | (2 if (g.a.full and Wa >= 2) else 0), Ha, Wa, sc_y, sc_x)
            else:
                geo = (0, 0, 0, 1.0, 1.0)
            rows.append((s.data_ptr(), s.numel() * s.element_size(), g.Hs, g.Ws) + geo
                        + (len(g.ops), g.a.record() if g.resample is not None else no_map, g.b.record(), tuple(kinds), tuple(facs)))
        raw[_HEAD_FLOATS * 4:first_fac * 4].view(_REC)[:] = np.array(rows, dtype=_REC)
        return host, contrast

    def launch(self, host, contrast, srcs, B, N, Ho, Wo, kind, normalize):
        """upload the table; stats (with a contrast op) and apply.  srcs: the clips the table points at, alive until here"""
        dev = srcs[0].device
        nbytes = host.numel()
        table = host.to(dev, non_blocking=True)
        out = torch.empty((B, 3, N, Ho, Wo), dtype=torch.float32, device=dev)
        args = (_lib.ptr(table), _lib.c_void_p(host.data_ptr()), nbytes, B, N, Ho, Wo, kind)
        ws = None
        if contrast:
            ws = _lib.workspace(_lib.load().slic_clip_transform_workspace_bytes(B, N, Ho, Wo), dev, "cliptf")
            _lib.call("slic_clip_transform_stats", *args, _lib.ptr(ws), _lib.stream())
        _lib.call("slic_clip_transform_apply", *args, int(normalize), _lib.ptr(ws), _lib.ptr(out), _lib.stream())
        return out


_default_kernels = None


def _kern(kernels):
    global _default_kernels
    if kernels is not None:
        return kernels
    if _default_kernels is None:
        _default_kernels = HipClipKernels()
    return _default_kernels


def _launch(kern, groups):
    """run one group per clip as one fused launch pair"""
    g0 = groups[0]
    for g in groups[1:]:
        if (g.kind, g.N, g.out_hw) != (g0.kind, g0.N, g0.out_hw) or (g.norm is None) != (g0.norm is None) or \
                (g.norm is not None and not all(np.array_equal(a, b) for a, b in zip(g.norm, g0.norm))):
            return None
    Ho, Wo = g0.out_hw
    return kern.run(groups, g0.kind, g0.N, Ho, Wo, g0.norm)


def _run_clip(kern, clip):
    """a clip whose chain split: group after group -> [3, N, H, W]"""
    out = None
    for g in clip.groups:
        if g.src is None:
            g.src = out
        if g.stage == _RAW:
            raise ValueError("a uint8 clip passed through without ToFloatTensor: nothing to compute")
        out = _launch(kern, [g])[0]
    return out


def _execute(kern, clips):
    """[B, 3, N, Ho, Wo] of a list of clip programs: one fused launch when every chain is one group, else clip by clip"""
    if all(len(c.groups) == 1 and c.g.stage != _RAW for c in clips):
        out = _launch(kern, [c.g for c in clips])
        if out is not None:
            return out
    outs = [_run_clip(kern, c) for c in clips]
    if any(o.shape != outs[0].shape for o in outs):
        raise ValueError("the clips of a batch come out in different shapes: " + ", ".join(str(tuple(o.shape)) for o in outs))
    return torch.stack(outs)


class Program:
    """what the transforms of a chain append to; stands in for the clip tensor between them (`.shape`, `.size()`, `.dim()`)"""

    def __init__(self, vid, kernels=None):
        self.kern = _kern(kernels)
        self.source = vid
        if isinstance(vid, torch.Tensor) and vid.dim() == 5:
            if vid.requires_grad:
                raise ValueError("clip transforms take data: the input requires grad")
            if vid.dtype != torch.float32 or vid.shape[1] != 3:
                raise self._five_d("a 5-D input other than float32 [B, 3, N, H, W]")
            self.kern.check(vid)
            self.five_d = True
            self.clips = [_Clip(v) for v in vid]
        else:
            _check_clip(vid)
            self.kern.check(vid)
            self.five_d = False
            self.clips = [_Clip(vid)]

    @staticmethod
    def _five_d(what):
        return ValueError(f"{what}: on 5-D batches only hflip and Normalize(channel=1) follow the reference; use Compose.batch(clips) "
                          "for whole chains")

    def _four_d(self, what):
        if self.five_d:
            raise self._five_d(what)

    @property
    def shape(self):
        s = self.clips[0].shape
        return torch.Size(((len(self.clips),) + s) if self.five_d else s)

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self):
        return len(self.shape)

    @property
    def untouched(self):
        return all(len(c.groups) == 1 and (c.g.identity or c.g.stage == _RAW) for c in self.clips)

    def groups(self):
        """the fused groups of a 4-D chain, in launch order"""
        return list(self.clips[0].groups)

    def each(self, fn):
        for c in self.clips:
            fn(c)
        return self

    def run(self):
        if self.untouched:
            return self.source                     # as the reference: nothing applied, the input itself
        out = _execute(self.kern, self.clips)
        return out if self.five_d else out[0]


def _enter(vid, kernels=None):
    """(program, whether this call owns it): a transform called on a tensor is a one-op program, on a Program it appends"""
    if isinstance(vid, Program):
        return vid, False
    return Program(vid, kernels), True


def _leave(prog, own):
    return prog.run() if own else prog


def _factors(f):
    if isinstance(f, torch.Tensor):
        f = f.detach().cpu().numpy()
    return np.asarray(f, dtype=np.float64).astype(np.float32).reshape(-1)


def _frame_channel(prog, channel, gray_channel=0):
    if channel != 1 or gray_channel != 0:
        raise ValueError("clips are [3, N, H, W]: channel=1 and gray_channel=0 are the only layout supported")


def crop(vid, i, j, h, w, *, kernels=None):
    p, own = _enter(vid, kernels)
    p._four_d("crop")
    return _leave(p.each(lambda c: c.crop(i, j, h, w)), own)


def center_crop(vid, output_size, *, kernels=None):
    (h, w), (th, tw) = vid.shape[-2:], output_size
    return crop(vid, int(round((h - th) / 2.)), int(round((w - tw) / 2.)), th, tw, kernels=kernels)


def hflip(vid, *, kernels=None):
    p, own = _enter(vid, kernels)
    return _leave(p.each(lambda c: c.flip()), own)


def resize(vid, size, interpolation='bilinear', *, kernels=None):
    if interpolation != 'bilinear':
        raise ValueError("resize: bilinear only")
    p, own = _enter(vid, kernels)
    p._four_d("resize")
    return _leave(p.each(lambda c: c.resize(size)), own)


def pad(vid, padding, fill=0, padding_mode="constant", *, kernels=None):
    if padding_mode != "constant":
        raise ValueError("pad: constant mode only")
    padding = tuple(int(v) for v in padding)
    if len(padding) not in (2, 4):
        raise ValueError("pad: (left, right) or (left, right, top, bottom)")
    left, right, top, bottom = padding + (0, 0) * (len(padding) == 2)
    p, own = _enter(vid, kernels)
    p._four_d("pad")
    return _leave(p.each(lambda c: c.pad(left, right, top, bottom, fill)), own)


def to_normalized_float_tensor(vid, *, kernels=None):
    # [N,H,W,C] -> [C,N,H,W], / 255
    p, own = _enter(vid, kernels)
    p._four_d("to_normalized_float_tensor")
    return _leave(p.each(lambda c: c.to_float(True)), own)


def to_float_tensor(vid, *, kernels=None):
    # [N,H,W,C] -> [C,N,H,W]
    p, own = _enter(vid, kernels)
    p._four_d("to_float_tensor")
    return _leave(p.each(lambda c: c.to_float(False)), own)


def normalize(vid, mean, std, channel=0, *, kernels=None):
    p, own = _enter(vid, kernels)
    if channel != (1 if p.five_d else 0):
        raise ValueError("normalize: the colour axis is 0 of [3, N, H, W] and 1 of [B, 3, N, H, W]")
    return _leave(p.each(lambda c: c.normalize(mean, std)), own)


def rgb_to_grayscale(vid, channel=0, *, kernels=None):
    """[3, N, H, W] -> [N, H, W]: L = R * 0.2989 + G * 0.5870 + B * 0.1140 (gray on every frame, one channel of it)"""
    if channel != 0:
        raise ValueError("rgb_to_grayscale: clips are [3, N, H, W]")
    p, own = _enter(vid, kernels)
    p._four_d("rgb_to_grayscale")
    if not own:
        raise ValueError("rgb_to_grayscale changes the layout: it cannot sit inside a Compose chain")
    p.each(lambda c: c.colour(GRAY, np.ones(c.g.N, dtype=np.float32)))
    return p.run()[0]


def random_grayscale(vid, factor, channel=1, *, kernels=None):
    p, own = _enter(vid, kernels)
    p._four_d("random_grayscale")
    _frame_channel(p, channel)
    N = p.size(channel)
    gray_map = np.random.uniform(size=(N,)) < factor
    if gray_map.sum() == 0:
        return vid
    return _leave(p.each(lambda c: c.colour(GRAY, gray_map.astype(np.float32))), own)


def _adjust(what, kind, vid, factor, channel, gray_channel, kernels):
    p, own = _enter(vid, kernels)
    p._four_d(what)
    _frame_channel(p, channel, gray_channel)
    f = _factors(factor)
    return _leave(p.each(lambda c: c.colour(kind, f)), own)


def adjust_brightness(vid, brightness_factor, channel=1, *, kernels=None):
    return _adjust("adjust_brightness", BRIGHTNESS, vid, brightness_factor, channel, 0, kernels)


def adjust_contrast(vid, contrast_factor, channel=1, gray_channel=0, *, kernels=None):
    return _adjust("adjust_contrast", CONTRAST, vid, contrast_factor, channel, gray_channel, kernels)


def adjust_saturation(vid, saturation_factor, channel=1, gray_channel=0, *, kernels=None):
    return _adjust("adjust_saturation", SATURATION, vid, saturation_factor, channel, gray_channel, kernels)


def _random_adjust(what, kind, vid, factor, consistent, channel, gray_channel, kernels):
    p, own = _enter(vid, kernels)
    p._four_d(what)
    _frame_channel(p, channel, gray_channel)
    N = p.size(channel)
    if consistent:
        f = np.array([random.uniform(factor[0], factor[1])] * N)
    else:
        f = np.random.uniform(factor[0], factor[1], size=(N,))
    return _leave(p.each(lambda c: c.colour(kind, _factors(f))), own)


def random_adjust_brightness(vid, brightness_factor, consistent, channel=1, *, kernels=None):
    return _random_adjust("random_adjust_brightness", BRIGHTNESS, vid, brightness_factor, consistent, channel, 0, kernels)


def random_adjust_contrast(vid, contrast_factor, consistent, channel=1, gray_channel=0, *, kernels=None):
    return _random_adjust("random_adjust_contrast", CONTRAST, vid, contrast_factor, consistent, channel, gray_channel, kernels)


def random_adjust_saturation(vid, saturation_factor, consistent, channel=1, gray_channel=0, *, kernels=None):
    return _random_adjust("random_adjust_saturation", SATURATION, vid, saturation_factor, consistent, channel, gray_channel, kernels)


# Class interface

class Lambda:
    """torchvision.transforms.Lambda, for ColorJitter.get_params"""
    _plans = True

    def __init__(self, lambd):
        self.lambd = lambd

    def __call__(self, vid):
        return self.lambd(vid)


class Compose:
    """torchvision.transforms.Compose over these transforms: the chain runs fused.  A callable that is not one of this module's
    transforms gets the tensor computed so far and starts a new chain."""
    _plans = True

    def __init__(self, transforms, *, kernels=None):
        self.transforms = list(transforms)
        self.kernels = kernels

    def _through(self, prog):
        for t in self.transforms:
            if getattr(t, "_plans", False):
                prog = t(prog)
            else:
                prog = Program(t(prog.run()), self.kernels)
        return prog

    def plan(self, vid):
        """draw the parameters and fold the chain; nothing runs.  `.groups()` lists the fused groups, each with `.launches`"""
        return self._through(vid if isinstance(vid, Program) else Program(vid, self.kernels))

    def __call__(self, vid):
        own = not isinstance(vid, Program)
        return _leave(self.plan(vid), own)

    def batch(self, clips):
        """torch.stack([self(c) for c in clips]) — parameters drawn clip by clip in that order — as one fused launch (two with a
        contrast op): contiguous float32 [B, 3, N, H, W].  clips: a list of equal-shape 4-D clips or one tensor with a leading B."""
        if isinstance(clips, torch.Tensor) and clips.dim() != 5:
            raise ValueError("Compose.batch takes a list of 4-D clips or a tensor with a leading batch axis")
        progs = [self.plan(c) for c in clips]
        if not progs:
            raise ValueError("Compose.batch: no clips")
        if any(p.five_d for p in progs):
            raise ValueError("Compose.batch takes 4-D clips")
        return _execute(progs[0].kern, [p.clips[0] for p in progs])

    def __repr__(self):
        return self.__class__.__name__ + "(" + ", ".join(repr(t) for t in self.transforms) + ")"


class Stack:
    def __init__(self, dim=1):
        self.dim = dim

    def __call__(self, imgmap):
        return torch.stack(imgmap, self.dim)


def _corner(h, w, th, tw):
    """top-left corner of a th x tw window inside h x w: two randint draws, rows first"""
    return random.randint(0, h - th), random.randint(0, w - tw)


class RandomCrop:
    _plans = True

    def __init__(self, size):
        self.size = size

    @staticmethod
    def get_params(vid, output_size):
        """(i, j, h, w) of a random window of output_size; no draw when the clip already has that size"""
        h, w = vid.shape[-2:]
        th, tw = output_size
        if (h, w) == (th, tw):
            return 0, 0, h, w
        return _corner(h, w, th, tw) + (th, tw)

    def __call__(self, vid):
        return crop(vid, *self.get_params(vid, self.size))


class RandomSizedCrop:
    """a window of 50-100 % of the area and aspect 3:4 .. 4:3 (ten attempts, then a window of `size`), resized to `size`"""
    _plans = True
    ATTEMPTS = 10

    def __init__(self, size):
        self.size = size

    @staticmethod
    def get_params(vid, output_size):
        h, w = vid.shape[-2:]
        for _ in range(RandomSizedCrop.ATTEMPTS):
            target = random.uniform(0.5, 1) * (h * w)
            aspect = random.uniform(3. / 4, 4. / 3)
            tw, th = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
            if th <= h and tw <= w:
                return _corner(h, w, th, tw) + (th, tw)
        th, tw = output_size
        return _corner(h, w, th, tw) + (th, tw)

    def __call__(self, vid):
        p, own = _enter(vid)
        p._four_d("RandomSizedCrop")
        return _leave(resize(crop(p, *self.get_params(p, self.size)), self.size), own)


class CenterCrop:
    _plans = True

    def __init__(self, size):
        self.size = size

    def __call__(self, vid):
        return center_crop(vid, self.size)


class FiveCrop:
    """one of the five windows of coclr_utils/augmentation.py:64-90: where = 1 top-left, 2 top-right, 3 bottom-left, 4 bottom-right,
    5 centre.  Window 4 starts at row h - tw and is tw rows high, as the reference's box (w - tw, h - tw, w, h) is: the same window
    as the other three corners for a square size, a tw x tw one otherwise."""
    _plans = True

    def __init__(self, size, where=1):
        self.size = (int(size), int(size)) if isinstance(size, numbers.Number) else tuple(size)
        if where not in (1, 2, 3, 4, 5):
            raise ValueError(f"FiveCrop: where is 1 .. 5, not {where!r}")
        self.where = where

    def window(self, h, w):
        """(i, j, rows, columns) of the window inside an h x w frame"""
        th, tw = self.size
        if th > h or tw > w:
            raise ValueError("Requested crop size {} is bigger than input size {}".format(self.size, (h, w)))
        if self.where == 1:
            return 0, 0, th, tw
        if self.where == 2:
            return 0, w - tw, th, tw
        if self.where == 3:
            return h - th, 0, th, tw
        if self.where == 4:
            return h - tw, w - tw, tw, tw
        return int(round((h - th) / 2.)), int(round((w - tw) / 2.)), th, tw

    def __call__(self, vid):
        h, w = vid.shape[-2:]
        return crop(vid, *self.window(h, w))


class Resize:
    _plans = True

    def __init__(self, size):
        self.size = size

    def __call__(self, vid):
        return resize(vid, self.size)


class ToFloatTensorInZeroOne:
    _plans = True

    def __call__(self, vid):
        return to_normalized_float_tensor(vid)


class ToFloatTensor:
    _plans = True

    def __call__(self, vid):
        return to_float_tensor(vid)


class Normalize:
    _plans = True

    def __init__(self, mean, std, channel=0):
        self.mean = mean
        self.std = std
        self.channel = channel

    def __call__(self, vid):
        return normalize(vid, self.mean, self.std, self.channel)


class RandomHorizontalFlip:
    """command='left' never flips and command='right' always does (coclr_utils/augmentation.py:152-169, the forced forms of
    coclr_classify.py's test-time views); the draw is still made, as there"""
    _plans = True

    def __init__(self, p=0.5, command=None):
        if command not in (None, 'left', 'right'):
            raise ValueError(f"RandomHorizontalFlip: command is 'left', 'right' or None, not {command!r}")
        self.p = 0 if command == 'left' else 1 if command == 'right' else p

    def __call__(self, vid):
        if random.random() < self.p:
            return hflip(vid)
        return vid


class Pad:
    _plans = True

    def __init__(self, padding, fill=0):
        self.padding = padding
        self.fill = fill

    def __call__(self, vid):
        return pad(vid, self.padding, self.fill)


class RandomGray:
    _plans = True

    def __init__(self, p=0.5):
        self.p = p

    def __call__(self, vid):
        return random_grayscale(vid, self.p)


class ColorJitter:
    """brightness, contrast and saturation jitter in a shuffled order, with probability p; one factor per clip (consistent=True) or
    per frame"""
    _plans = True

    def __init__(self, brightness=0, contrast=0, saturation=0, consistent=False, p=1.0, n_channel=1, gray_channel=0):
        self.brightness = self._range(brightness, 'brightness')
        self.contrast = self._range(contrast, 'contrast')
        self.saturation = self._range(saturation, 'saturation')
        self.consistent, self.p, self.n_channel, self.gray_channel = consistent, p, n_channel, gray_channel

    @staticmethod
    def _range(value, name):
        """a number v means [1 - v, 1 + v]; a pair is taken as it is; None when the range is exactly [1, 1] (the op is left out)"""
        if isinstance(value, numbers.Number):
            if value < 0:
                raise ValueError(f"{name}: a single number must not be negative")
            value = [1 - value, 1 + value]
        elif isinstance(value, (tuple, list)) and len(value) == 2:
            if not 0 <= value[0] <= value[1] <= float('inf'):
                raise ValueError(f"{name}: the pair must satisfy 0 <= low <= high")
        else:
            raise TypeError(f"{name}: a number or a pair of numbers")
        return None if value[0] == value[1] == 1 else value

    @staticmethod
    def get_params(brightness, contrast, saturation, consistent, n_channel, gray_channel):
        """the enabled ops (None = left out) as a Compose in a freshly shuffled order; the factors are drawn when it is applied"""
        ops = []
        if brightness is not None:
            ops.append(Lambda(lambda vid: random_adjust_brightness(vid, brightness, consistent, n_channel)))
        if contrast is not None:
            ops.append(Lambda(lambda vid: random_adjust_contrast(vid, contrast, consistent, n_channel, gray_channel)))
        if saturation is not None:
            ops.append(Lambda(lambda vid: random_adjust_saturation(vid, saturation, consistent, n_channel, gray_channel)))
        random.shuffle(ops)
        return Compose(ops)

    def __call__(self, vid):
        if isinstance(vid, Program):
            vid._four_d("ColorJitter")
        elif isinstance(vid, torch.Tensor) and vid.dim() == 5:
            raise Program._five_d("ColorJitter")
        if random.random() >= self.p:
            return vid
        return self.get_params(self.brightness, self.contrast, self.saturation, self.consistent, self.n_channel, self.gray_channel)(vid)

    def __repr__(self):
        return f"{self.__class__.__name__}(brightness={self.brightness}, contrast={self.contrast}, saturation={self.saturation})"


# Views of one clip (coclr_classify.py:540-556: the test-time crops and flips)

def multi_view(clip, composes, *, kernels=None):
    """torch.stack([c(clip) for c in composes]) — parameters drawn chain by chain in that order — from ONE source clip: the per-clip
    records of a launch carry their own source pointer, so the n records share it.  One parameter upload and the launches of one
    Compose.batch when every chain folds into one group of one output shape; contiguous float32 [n_views, 3, N, H, W]."""
    composes = list(composes)
    if not composes:
        raise ValueError("multi_view: no views")
    progs = []
    for c in composes:
        if not isinstance(c, Compose):
            raise TypeError("multi_view takes Compose chains")
        progs.append(c.plan(Program(clip, kernels if kernels is not None else c.kernels)))
    if any(p.five_d for p in progs):
        raise ValueError("multi_view takes one 4-D clip")
    return _execute(progs[0].kern, [p.clips[0] for p in progs])


def ten_crop_views(crop, out, *, kernels=None):
    """the ten chains of coclr_classify.py's ten-crop test for a uint8 [N, H, W, 3] clip, in its order: centre, top-left, top-right,
    bottom-left, bottom-right unflipped, then the same five flipped (the flip comes before the window, as there).  Each is
    [0, 1] scaling, RandomHorizontalFlip(command=), FiveCrop(crop, where) and a bilinear resize to `out` (left out when the window
    already has that size).  The first chain alone is the centre-crop protocol, the first five the five-crop one."""
    crop = (int(crop), int(crop)) if isinstance(crop, numbers.Number) else tuple(int(v) for v in crop)
    out = (int(out), int(out)) if isinstance(out, numbers.Number) else tuple(int(v) for v in out)
    chains = []
    for command in ('left', 'right'):
        for where in (5, 1, 2, 3, 4):
            chain = [ToFloatTensorInZeroOne(), RandomHorizontalFlip(command=command), FiveCrop(crop, where)]
            if out != crop:
                chain.append(Resize(out))
            chains.append(Compose(chain, kernels=kernels))
    return chains

"""
Dropout of the classifier head (the `nn.Dropout(p)` in front of `linear`, models/resnet.py:194-198) on the device:
slic_dropout_fwd / slic_dropout_bwd (csrc/classify.hip).  The mask is never stored: it is a function of (seed, offset, element
index) through a counter-based generator, and the backward recomputes it.

(seed, offset) come from torch's default generator of the tensor's device, and every call advances that generator's offset, so
`torch.manual_seed(s)` reproduces a run and two consecutive calls draw different masks.  The random STREAM is not torch's: with
the same seed `nn.Dropout` on the reference's side zeroes other elements (an equally valid sample of the same distribution).
"""
import torch

from .._lib import SlicError, call, ptr, require_device, stream


def next_seed_offset(device, n):
    """(seed, offset) for one mask over n elements, taken from (and advancing) torch's default generator of `device`"""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[idx]
    seed, offset = int(gen.initial_seed()), int(gen.get_offset())
    gen.set_offset(offset + (int(n) + 3) // 4 * 4)           # torch keeps the offset a multiple of 4
    return seed & 0xFFFFFFFFFFFFFFFF, offset


def apply_mask(x, p, seed, offset, backward=False):
    """x (contiguous fp32 device tensor) through the mask of (p, seed, offset); forward and backward are the same map"""
    y = torch.empty_like(x)
    call("slic_dropout_bwd" if backward else "slic_dropout_fwd", ptr(x), x.numel(), float(p), seed, offset, ptr(y), stream())
    return y


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        ctx.key = (p,) + next_seed_offset(x.device, x.numel())
        return apply_mask(x, *ctx.key)

    @staticmethod
    def backward(ctx, dy):
        return apply_mask(dy.contiguous().float(), *ctx.key, backward=True), None


def dropout(x, p=0.5, training=True):
    """F.dropout(x, p, training) on the device; eval mode (or p == 0) hands x back unchanged"""
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
    if not training or p == 0.0 or x.numel() == 0:
        return x
    require_device(x)
    if x.dtype != torch.float32:
        raise SlicError("dropout: fp32 tensors only")
    return _Dropout.apply(x.contiguous(), float(p))

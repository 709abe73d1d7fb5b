"""
The loss and the accuracy of the reference's downstream classification (coclr_classify.py:216, 429-431):

    CrossEntropyLoss()                                   <- nn.CrossEntropyLoss() with its defaults (mean reduction, class-index targets)
    calc_topk_accuracy(output, target, topk=(1,))        <- coclr_utils/utils.py:55-75

One device pass (slic_softmax_ce_fwd, csrc/classify.hip) yields the loss AND the rank of every row's target logit; top-k hit
counts are `rank < k`.  The ranks of the last pass are kept, keyed by the tensors they came from, so calc_topk_accuracy on the
logits the loss was just computed from launches nothing.  Ties: a logit equal to the target's counts as ranked above it when its
class index is lower (torch.topk leaves that order unspecified; on distinct values the two agree exactly).
No CPU implementation: both raise SlicError without a device.
"""
import torch
import torch.nn as nn

from .._lib import SlicError, call, ptr, require_device, stream

HITS_HEAD = 3           # SLIC_CE_HITS_HEAD: {rows with a bad target, top-1 hits, top-5 hits} in front of the ranks

_last = [None]          # (logits, logits._version, target, target._version, hits) of the latest forward pass


def _check(logits, target):
    require_device(logits, target)
    if logits.dim() != 2 or target.dim() != 1 or target.shape[0] != logits.shape[0]:
        raise SlicError(f"cross entropy: expected [B, C] logits and [B] targets, got {tuple(logits.shape)} and {tuple(target.shape)}")
    if logits.dtype != torch.float32 or target.dtype != torch.int64:
        raise SlicError("cross entropy: fp32 logits and int64 (class index) targets only")
    if logits.shape[0] == 0 or logits.shape[1] == 0:
        raise SlicError("cross entropy: empty batch or no classes")
    if logits.stride(1) != 1 or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1]):
        logits = logits.contiguous()
    return logits, target.contiguous()


def _forward(logits, target):
    """returns (loss 0-d, lse [B, 2], hits int32 [HITS_HEAD + B]); raises on a target outside [0, C)"""
    B, C = logits.shape
    dev = logits.device
    ld = logits.stride(0) if B > 1 else max(C, logits.stride(0))
    lse = torch.empty(B, 2, dtype=torch.float32, device=dev)
    rowloss = torch.empty(B, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    hits = torch.empty(HITS_HEAD + B, dtype=torch.int32, device=dev)
    call("slic_softmax_ce_fwd", ptr(logits), ld, B, C, ptr(target), ptr(lse), ptr(rowloss), ptr(loss), ptr(hits), stream())
    bad = int(hits[0].item())        # the kernel flags a bad target instead of reading through it; reported here
    if bad:
        raise SlicError(f"cross entropy: {bad} target(s) outside [0, {C})")
    # detached aliases: same storage and version counter, no hold on the autograd graph behind the logits
    _last[0] = (logits.detach(), logits._version, target.detach(), target._version, hits)
    return loss, lse, hits


def _cached_hits(logits, target):
    c = _last[0]
    if (c is not None and c[0].data_ptr() == logits.data_ptr() and c[0].shape == logits.shape and c[0].stride() == logits.stride() and
            c[0]._version == c[1] == logits._version and c[2].data_ptr() == target.data_ptr() and c[2].shape == target.shape and
            c[2]._version == c[3] == target._version):
        return c[4]
    return None


class _SoftmaxCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        loss, lse, hits = _forward(logits, target)
        ctx.save_for_backward(logits, target, lse)
        ctx.mark_non_differentiable(hits)
        return loss, hits

    @staticmethod
    def backward(ctx, g, _gh):
        logits, target, lse = ctx.saved_tensors
        B, C = logits.shape
        ld = logits.stride(0) if B > 1 else max(C, logits.stride(0))
        dx = torch.empty(B, C, dtype=torch.float32, device=logits.device)
        call("slic_softmax_ce_bwd", ptr(logits), ld, ptr(lse), ptr(target), B, C, ptr(g.contiguous().float()), ptr(dx), stream())
        return dx, None


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss() (defaults) on the device.  After a forward: `hits` int32 [3 + B] = {0, top-1 hits, top-5 hits,
    rank of each row's target}, `top1_hits` / `top5_hits` 0-d views of it and `ranks` [B]."""

    def __init__(self):
        super().__init__()
        self.hits = None

    @property
    def top1_hits(self):
        return None if self.hits is None else self.hits[1]

    @property
    def top5_hits(self):
        return None if self.hits is None else self.hits[2]

    @property
    def ranks(self):
        return None if self.hits is None else self.hits[HITS_HEAD:]

    def forward(self, input, target):
        logits, target = _check(input, target)
        loss, hits = _SoftmaxCE.apply(logits, target)
        self.hits = hits
        return loss


def calc_topk_accuracy(output, target, topk=(1,)):
    """top-k accuracies of [B, C] logits against [B] targets: a list of 0-d tensors in [0, 1], one per k (coclr_utils/utils.py:55-75)"""
    logits, target = _check(output.detach(), target)
    B, C = logits.shape
    if max(topk) > C or min(topk) < 1:
        raise SlicError(f"calc_topk_accuracy: k must lie in [1, {C}], got {tuple(topk)}")
    hits = _cached_hits(logits, target)
    if hits is None:
        with torch.no_grad():
            _, _, hits = _forward(logits, target)
    res = []
    for k in topk:
        n = hits[1] if k == 1 else hits[2] if k == 5 else (hits[HITS_HEAD:] < k).sum()
        res.append(n.float().mul_(1 / B))
    return res

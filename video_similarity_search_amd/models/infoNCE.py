"""
The MoCo models of the reference's models/infoNCE.py, with the same names, constructor defaults, outputs and state-dict keys:

    concat_all_gather(tensor)
    InfoNCE(network, dim=128, K=2048, m=0.999, T=0.07)      forward(block)          -> (logits [B, 1 + K], zeros [B] int64)
    UberNCE(network, dim=128, K=2048, m=0.999, T=0.07)      forward(block, k_label) -> (logits [B, 1 + K], bool mask [B, 1 + K])

`block` is [B, 2, C, T, H, W]: view 0 goes through the query encoder, view 1 through the momentum (key) encoder.  An encoder is
nn.Sequential(trunk, AdaptiveAvgPool3d, Conv3d 1x1x1, ReLU, Conv3d 1x1x1), so a checkpoint has `encoder_q.0.*` (the trunk),
`encoder_q.2.*`, `encoder_q.4.*`, the same under `encoder_k`, `queue` [dim, K], `queue_ptr` [1] and, for UberNCE, `queue_label` [K].

What differs from the reference:
  * network: 'resnet10' .. 'resnet200' (generate_model(depth, projection_head=False)), 'r3d' (R3DNet((1, 1, 1, 1))) or a zero-argument
    callable returning a trunk module that maps a clip to pooled features [B, F] (F: its `feature_size` or `in_planes` attribute).
    The reference's only value, 's3d', raises NotImplementedError (the S3D backbone is not ported).
  * The Sequential is a parameter container.  The trunk runs through its own engine and returns pooled features; the head
    (Conv3d 1x1x1 + bias, ReLU, Conv3d 1x1x1 + bias, F.normalize(dim=1, eps=1e-12)) is ONE autograd node on two LinearPlan layers
    and slic_l2normalize_fwd / _bwd.
  * `queue` is the transposed view of a contiguous [K, dim] storage: the moco kernels read the rows in place, and an enqueue writes
    whole rows.
  * contrast(block, k_label=None, topk=(1, 5)) -> (loss, [acc_k ...]) is the same training step without the [B, 1 + K] matrix:
    slic_moco_ce_fwd / _bwd for the loss and slic_moco_topk_hits for the accuracies, both on the queue before the enqueue.  The
    accuracies are 0-d device tensors; nothing is read back.  In contrast() an empty queue slot (label -1) is never a positive, as
    in MemoryMoCo.softmax_loss; forward() builds the mask with the reference's plain `==`.
  * forward(block[, k_label], fused=True, topk=(1, 5)) returns contrast()'s outputs.  A model behind DistributedDataParallel takes
    the fused step this way, `wrapped(block, k_label, fused=True)`: the wrapper arms its gradient reduction (and broadcasts its
    buffers) in ITS forward, so calling `wrapped.module.contrast(...)` would leave every rank with its own gradients.
  * keyword-only kernels= takes another kernel provider (tests of the host logic pass a float64 NumPy one).

Batch shuffle.  With a process group of more than one rank the key batch is gathered, permuted with a permutation drawn on rank 0
and broadcast, each rank encodes its share, and the keys are gathered and un-permuted (all ranks need equal batch sizes).  With one
process, or no initialised group, the permutation is still drawn, so the RNG stream stays the reference's, but it is not applied:
the BatchNorm statistics of a permuted batch are those of the same set of samples, and un-permuting returns the same rows.
"""
import ctypes
import re

import torch
import torch.nn as nn

from .. import _lib
from .._lib import call, ptr, stream
from ..loss.NCE_loss import HipMoCoKernels, _MoCoFusedStep, _MoCoLogits, _MOCO_PARTS
from .. import optim as slic_optim

NORMALIZE_EPS = 1e-12          # F.normalize's default


# ------------------------------------------------------------------------------------------------------------------------------
# process-group helpers
# ------------------------------------------------------------------------------------------------------------------------------
def _world():
    dist = torch.distributed
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(), dist.get_rank()
    return 1, 0


@torch.no_grad()
def concat_all_gather(tensor):
    """torch.distributed.all_gather of equal-shaped tensors, concatenated along dim 0 in rank order (no gradient).  Without an
    initialised process group: the tensor itself."""
    world, _ = _world()
    if world == 1 and not (torch.distributed.is_available() and torch.distributed.is_initialized()):
        return tensor
    parts = [torch.ones_like(tensor) for _ in range(world)]
    torch.distributed.all_gather(parts, tensor.contiguous(), async_op=False)
    return torch.cat(parts, dim=0)


def shuffle_rows_of_rank(idx_shuffle, world, rank):
    """rows of the gathered batch that `rank` encodes: slice `rank` of the permutation"""
    return idx_shuffle.view(world, -1)[rank]


def unshuffle_rows_of_rank(idx_shuffle, world, rank):
    """rows of the gathered, shuffled keys that are `rank`'s own samples in their original order"""
    return torch.argsort(idx_shuffle).view(world, -1)[rank]


# ------------------------------------------------------------------------------------------------------------------------------
# device kernels
# ------------------------------------------------------------------------------------------------------------------------------
def _ks(top_ks):
    return (ctypes.c_int32 * len(top_ks))(*[int(k) for k in top_ks])


class HipInfoNCEKernels(HipMoCoKernels):
    """the device side of InfoNCE / UberNCE: HipMoCoKernels plus the rank of the best positive, the dense-mask rank and the
    projection head.  `optim_kernels` is handed to optim.momentum_update (None = the device)."""
    optim_kernels = None

    def __init__(self):
        super().__init__()
        self._plans = {}

    # -- accuracies
    def topk_hits(self, q, k, memory, T, k_label, queue_label, top_ks):
        """-> (rank int32 [B], saturated at max(top_ks); hits int32 [len(top_ks)])"""
        (B, D), K = q.shape, memory.shape[0]
        out = torch.empty(B + len(top_ks), dtype=torch.int32, device=q.device)
        ws = _lib.workspace((_MOCO_PARTS + 1) * B * 8, q.device, tag="moco")
        call("slic_moco_topk_hits", ptr(q), ptr(k), ptr(memory), B, K, D, float(T), ptr(k_label), ptr(queue_label), _ks(top_ks),
             len(top_ks), ptr(out), ptr(out[B:]), ptr(ws), stream())
        return out[:B], out[B:]

    def mask_hits(self, output, mask, top_ks):
        """-> (rank int32 [B], C for a row without a positive; hits int32 [len(top_ks)])"""
        B, C = output.shape
        out = torch.empty(B + len(top_ks), dtype=torch.int32, device=output.device)
        call("slic_mask_topk_hits", ptr(output), output.stride(0), ptr(mask), mask.stride(0), B, C, _ks(top_ks), len(top_ks),
             ptr(out), ptr(out[B:]), stream())
        return out[:B], out[B:]

    # -- projection head
    def _plan(self, C, N, device):
        from .conv_plan import LinearPlan
        key = (C, N, str(device))
        plan = self._plans.get(key)
        if plan is None:
            if C % 4 or N % 4:
                raise ValueError(f"InfoNCE head: feature size {C} and dim {N} must be multiples of 4")
            plan = self._plans[key] = LinearPlan(C, N, device)
        return plan

    def head_fwd(self, feat, w1, b1, w2, b2):
        """feat [B, F] -> y = normalize(W2 relu(W1 feat + b1) + b2) [B, dim]; -> (y, saved): the tensors head_bwd needs besides y"""
        B, F = feat.shape
        N = w2.shape[0]
        p1, p2 = self._plan(F, F, feat.device), self._plan(F, N, feat.device)
        p1.drop_packs()
        p2.drop_packs()
        feat = feat.contiguous().float()
        h = p1.rows_forward(feat, w1, bias=b1, relu=True)
        z = p2.rows_forward(h, w2, bias=b2)
        y = torch.empty(B, N, dtype=torch.float32, device=feat.device)
        inv = torch.empty(B, dtype=torch.float32, device=feat.device)
        call("slic_l2normalize_fwd", ptr(z), B, N, NORMALIZE_EPS, ptr(y), ptr(inv), stream())
        return y, (feat, h, inv)

    def head_bwd(self, dy, y, saved, w1, w2, need_dx):
        """-> (d feat or None, dW1, db1, dW2, db2)"""
        feat, h, inv = saved
        (B, F), N = feat.shape, y.shape[1]
        p1, p2 = self._plan(F, F, feat.device), self._plan(F, N, feat.device)
        dz = torch.empty_like(y)
        call("slic_l2normalize_bwd", ptr(dy.contiguous().float()), ptr(y), ptr(inv), B, N, ptr(dz), stream())
        # packs cached from head_fwd; the ReLU's backward rides in the second layer's data gradient (mask=h)
        dh, gw2, gb2 = p2.rows_backward(h, dz, w2, need_dx=True, need_dw=True, need_db=True, mask=h)
        dfeat, gw1, gb1 = p1.rows_backward(feat, dh, w1, need_dx=need_dx, need_dw=True, need_db=True)
        return dfeat, gw1, gb1, gw2, gb2


class _Head(torch.autograd.Function):
    """Conv3d 1x1x1 + bias -> ReLU -> Conv3d 1x1x1 + bias -> F.normalize(dim=1) on pooled features, as one node: two LinearPlan layers
    (HipInfoNCEKernels.head_fwd / head_bwd; DESIGN.md §3, linear layers)"""

    @staticmethod
    def forward(ctx, feat, w1, b1, w2, b2, kern, keep):
        y, saved = kern.head_fwd(feat.detach(), w1.detach(), b1.detach(), w2.detach(), b2.detach())
        if keep:
            ctx.kern = kern
            ctx.save_for_backward(w1, w2, y, *saved)         # y is this node's output: saved this way it makes no reference cycle
        return y

    @staticmethod
    def backward(ctx, dy):
        w1, w2, y, *saved = ctx.saved_tensors
        dfeat, gw1, gb1, gw2, gb2 = ctx.kern.head_bwd(dy, y, tuple(saved), w1.detach(), w2.detach(), ctx.needs_input_grad[0])
        return dfeat, gw1, gb1, gw2, gb2, None, None


# ------------------------------------------------------------------------------------------------------------------------------
# the models
# ------------------------------------------------------------------------------------------------------------------------------
def _make_trunk(network):
    if callable(network):
        return network()
    if network == 's3d':
        raise NotImplementedError("InfoNCE(network='s3d'): the S3D backbone is not ported (DESIGN §7); pass 'resnet18' .. 'resnet200', "
                                  "'r3d' or a callable that returns a trunk")
    if network == 'r3d':
        from .r3d import R3DNet
        return R3DNet(layer_sizes=(1, 1, 1, 1))
    m = re.fullmatch(r"resnet(\d+)", str(network))
    if m and int(m.group(1)) in (10, 18, 34, 50, 101, 152, 200):
        from .resnet import generate_model
        return generate_model(int(m.group(1)), projection_head=False)
    raise ValueError(f"InfoNCE: unknown network {network!r}")


def _feature_size(trunk):
    for name in ("feature_size", "in_planes"):
        v = getattr(trunk, name, None)
        if isinstance(v, int) and v > 0:
            return v
    from .r3d import R3DNet
    if isinstance(trunk, R3DNet):
        return 512
    raise ValueError("InfoNCE: the trunk must say how wide its pooled features are (an int attribute `feature_size`)")


class InfoNCE(nn.Module):
    """MoCo for video (models/infoNCE.py:38-200); see the module docstring"""
    _labelled = False

    def __init__(self, network='resnet18', dim=128, K=2048, m=0.999, T=0.07, *, kernels=None):
        super(InfoNCE, self).__init__()
        self.dim = dim
        self.K = K
        self.m = m
        self.T = T
        self._kernels = kernels
        encoders = []
        for _ in range(2):
            trunk = _make_trunk(network)
            F = _feature_size(trunk)
            encoders.append(nn.Sequential(trunk, nn.AdaptiveAvgPool3d((1, 1, 1)), nn.Conv3d(F, F, kernel_size=1, bias=True), nn.ReLU(),
                                          nn.Conv3d(F, dim, kernel_size=1, bias=True)))
        self.encoder_q, self.encoder_k = encoders
        self.param = {'feature_size': F}
        for param_q, param_k in zip(self.encoder_q.parameters(), self.encoder_k.parameters()):
            param_k.data.copy_(param_q.data)
            param_k.requires_grad = False
        queue = nn.functional.normalize(torch.randn(dim, K), dim=0)
        self.register_buffer("queue", queue.t().contiguous().t())            # [dim, K], a view of contiguous rows [K, dim]
        self.register_buffer("queue_ptr", torch.zeros(1, dtype=torch.long))
        if self._labelled:
            self.register_buffer("queue_label", torch.ones(K, dtype=torch.long) * -1)

    # -- pieces
    def _kern(self):
        if self._kernels is None:
            self._kernels = HipInfoNCEKernels()
        return self._kernels

    def _rows(self):
        """the queue as contiguous rows [K, dim] (a buffer that arrived in another layout is re-laid once)"""
        rows = self.queue.t()
        if not rows.is_contiguous():
            self.queue = rows.contiguous().t()
            rows = self.queue.t()
        return rows

    def _ptr(self):
        """queue_ptr as a Python number, read back only when the buffer changed behind our back (load_state_dict)"""
        key = (self.queue_ptr.data_ptr(), self.queue_ptr._version)
        if getattr(self, "_ptr_key", None) != key:
            self._ptr_host = int(self.queue_ptr)
            self._ptr_key = key
        return self._ptr_host

    def _encode(self, encoder, x):
        kern = self._kern()
        feat = encoder[0](x)
        feat = feat.reshape(feat.shape[0], -1)
        c1, c2 = encoder[2], encoder[4]
        keep = torch.is_grad_enabled() and (feat.requires_grad or any(p.requires_grad for p in (c1.weight, c1.bias, c2.weight, c2.bias)))
        return _Head.apply(feat, c1.weight, c1.bias, c2.weight, c2.bias, kern, keep)

    @torch.no_grad()
    def _momentum_update_key_encoder(self):
        slic_optim.momentum_update(self.encoder_k, self.encoder_q, self.m, kernels=self._kern().optim_kernels)

    @torch.no_grad()
    def _batch_shuffle_ddp(self, x):
        world, rank = _world()
        if world == 1:
            torch.randperm(x.shape[0])                        # drawn for the RNG stream, not applied (module docstring); no gather
            return x, None
        x_gather = concat_all_gather(x)
        idx_shuffle = torch.randperm(x_gather.shape[0]).to(x.device)
        torch.distributed.broadcast(idx_shuffle, src=0)
        return x_gather[shuffle_rows_of_rank(idx_shuffle, world, rank)], idx_shuffle

    @torch.no_grad()
    def _batch_unshuffle_ddp(self, x, idx_shuffle):
        if idx_shuffle is None:
            return x
        world, rank = _world()
        return concat_all_gather(x)[unshuffle_rows_of_rank(idx_shuffle, world, rank)]

    @torch.no_grad()
    def _dequeue_and_enqueue(self, keys, labels=None):
        kern = self._kern()
        keys = concat_all_gather(keys)
        if labels is not None:
            labels = concat_all_gather(labels)
        batch_size = keys.shape[0]
        ptr_ = self._ptr()
        if self.K % batch_size != 0:
            raise ValueError(f"InfoNCE: the queue size K = {self.K} must be a multiple of the gathered batch size {batch_size}")
        kern.enqueue(self._rows(), self.queue_label if self._labelled else None, kern.resident(keys),
                     labels.contiguous().long() if labels is not None else None, ptr_)
        ptr_ = (ptr_ + batch_size) % self.K
        self.queue_ptr[0] = ptr_
        self._ptr_host, self._ptr_key = ptr_, (self.queue_ptr.data_ptr(), self.queue_ptr._version)

    def _features(self, block, k_label):
        if block.dim() < 3 or block.shape[1] != 2:
            raise ValueError(f"InfoNCE expects block [B, 2, C, T, H, W], got {tuple(block.shape)}")
        if self._labelled and k_label is None:
            raise ValueError("UberNCE needs k_label [B]")
        if not self._labelled and k_label is not None:
            raise ValueError("InfoNCE takes no k_label (UberNCE does)")
        kern = self._kern()
        kern.check(block, k_label, self.queue)
        x1 = block[:, 0].contiguous()
        x2 = block[:, 1].contiguous()
        q = self._encode(self.encoder_q, x1)
        in_train_mode = q.requires_grad
        with torch.no_grad():
            if in_train_mode:
                self._momentum_update_key_encoder()
            x2, idx_shuffle = self._batch_shuffle_ddp(x2)
            k = self._encode(self.encoder_k, x2)
            k = self._batch_unshuffle_ddp(k, idx_shuffle)
        k = kern.resident(k.detach())
        if k_label is not None:
            k_label = k_label.detach().contiguous().long()
        return kern, q, k, k_label, in_train_mode

    # -- the reference's outputs
    def forward(self, block, k_label=None, *, fused=False, topk=(1, 5)):
        '''Output: logits, targets (InfoNCE) / logits, binary mask for positive pairs (UberNCE).  fused=True: contrast()'s
        (loss, [acc_k]) instead, for a model behind a wrapper whose forward must run (DistributedDataParallel arms its gradient
        reduction there): `wrapped(block, k_label, fused=True)`'''
        if fused:
            return self.contrast(block, k_label, topk)
        kern, q, k, k_label, in_train_mode = self._features(block, k_label)
        logits = _MoCoLogits.apply(q, k, self._rows(), self.T, kern, in_train_mode and torch.is_grad_enabled())
        if self._labelled:
            mask = k_label.unsqueeze(1) == self.queue_label.unsqueeze(0)
            target = torch.cat([torch.ones((mask.shape[0], 1), dtype=torch.bool, device=mask.device), mask], dim=1)
        else:
            target = torch.zeros(logits.shape[0], dtype=torch.long, device=logits.device)
        if in_train_mode:
            self._dequeue_and_enqueue(k, k_label)
        return logits, target

    # -- the same step without the logits
    def contrast(self, block, k_label=None, topk=(1, 5)):
        """-> (loss, [accuracy at k for k in topk]): the loss the epoch computes from forward()'s outputs (cross-entropy against
        column 0; with labels the mean of -(sum_pos log_softmax) / n_pos) and calc_topk_accuracy / calc_mask_accuracy, on the queue
        as it was before this step's keys went in.  topk: ascending, 1 <= k <= 8."""
        kern, q, k, k_label, in_train_mode = self._features(block, k_label)
        rows = self._rows()
        ql = self.queue_label if self._labelled else None
        with torch.no_grad():
            _, hits = kern.topk_hits(kern.resident(q.detach()), k, rows, self.T, k_label, ql, tuple(topk))
            accs = list((hits.to(torch.float32) / q.shape[0]).unbind(0))
        loss = _MoCoFusedStep.apply(q, k, rows, self.T, k_label, ql, kern, in_train_mode and torch.is_grad_enabled())
        if in_train_mode:
            self._dequeue_and_enqueue(k, k_label)
        return loss, accs


class UberNCE(InfoNCE):
    """the supervised InfoNCE (models/infoNCE.py:203-288): labels define the positives, `queue_label` [K] remembers the keys' labels"""
    _labelled = True

    def __init__(self, network='resnet18', dim=128, K=2048, m=0.999, T=0.07, *, kernels=None):
        super(UberNCE, self).__init__(network, dim, K, m, T, kernels=kernels)

    def forward(self, block, k_label, *, fused=False, topk=(1, 5)):
        return super(UberNCE, self).forward(block, k_label, fused=fused, topk=topk)

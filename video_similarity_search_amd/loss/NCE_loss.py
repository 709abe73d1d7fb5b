"""
Drop-in for the memory-bank NCE of the reference's loss/NCE_loss.py:
    NCEAverage(inputSize, outputSize, K, T, momentum)(l, ab, y, idx=None) -> (out_l, out_ab)   <- :10-88
    NCESoftmaxLoss()(x) -> scalar                                                               <- :341-352
    AliasMethod(probs).draw(N)                                                                  <- :246-307
Same buffers (`params`, `memory_l`, `memory_ab`), same cross-wiring (out_ab is scored against memory_l, out_l
against memory_ab), bank rows detached, momentum update + renormalise under no_grad.  The gather+bmm, its
backward, the bank update and the class-0 cross-entropy are HIP kernels (csrc/nce.hip).
    NCEAverage_intra_neg(inputSize, outputSize, K, T, momentum)(l, ab, neg, y, idx=None)       <- :91-184
    MemoryMoCo(inputSize, outputSize, K, T, use_softmax)(q, k) -> out [B, K+1]                  <- :188-241
MemoryMoCo scores a batch of queries against a dense queue (csrc/moco.hip): forward() returns the reference's output,
softmax_loss() is the fused step (NCESoftmaxLoss on the logits, or the multi-positive UberNCE loss with labels) that never
writes the [B, K+1] logits.
The use_softmax=False branch (:54-71: out = exp(score / T / Z) with the constants Z_l / Z_ab fixed on the first call and
kept in `params[2:4]`) and its NCECriterion (:312-337, Eq. 12 of the CMC paper) are not selected by SLIC
(online_train.py:701-710 builds NCEAverage with the default and NCESoftmaxLoss); they are restated on top of the same
score kernels — the exp / log over the [B, K+1] outputs are a few kilobytes of elementwise torch ops.
"""
import math

import torch
from torch import nn

from .. import _lib
from .._lib import call, ptr, stream


class AliasMethod(object):
    """Sampler over `probs`.  The reference builds alias tables on the host and draws with
    index_select + bernoulli (loss/NCE_loss.py:246-307); NCEAverage always passes uniform weights
    (`torch.ones(nLem)`, :14-15), for which every alias-table entry has prob 1 and the draw reduces to
    uniform integers — that is what this class does on the device.  Non-uniform tables are built the
    reference's way and sampled with torch ops (cold path)."""

    def __init__(self, probs):
        probs = probs.clone().float()
        if probs.sum() > 1:
            probs.div_(probs.sum())
        K = len(probs)
        self.n = K
        self.uniform = bool(torch.allclose(probs, torch.full_like(probs, 1.0 / K)))
        self.prob = torch.ones(K)
        self.alias = torch.zeros(K, dtype=torch.long)
        if not self.uniform:
            smaller, larger = [], []
            for kk, p in enumerate(probs):
                self.prob[kk] = K * p
                (smaller if self.prob[kk] < 1.0 else larger).append(kk)
            while len(smaller) > 0 and len(larger) > 0:
                small, large = smaller.pop(), larger.pop()
                self.alias[small] = large
                self.prob[large] = (self.prob[large] - 1.0) + self.prob[small]
                (smaller if self.prob[large] < 1.0 else larger).append(large)
            for last_one in smaller + larger:
                self.prob[last_one] = 1
        self.device = torch.device("cpu")

    def cuda(self):
        self.device = torch.device("cuda")
        self.prob = self.prob.cuda()
        self.alias = self.alias.cuda()

    def draw(self, N):
        kk = torch.randint(0, self.n, (N,), dtype=torch.long, device=self.prob.device)
        if self.uniform:
            return kk
        b = torch.bernoulli(self.prob.index_select(0, kk))
        return kk.mul(b.long()) + self.alias.index_select(0, kk).mul((1 - b).long())


class _BankScores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, bank, idx, T):
        f = feat.contiguous().float()
        B, D = f.shape
        K1 = idx.shape[1]
        out = torch.empty(B, K1, 1, dtype=torch.float32, device=f.device)
        # NCEAverage updates the bank in place right after scoring, so a training pass keeps the rows as scored
        # (written by the same kernel pass that reads them); under no_grad nothing is kept.
        rows = torch.empty(B * K1, D, dtype=torch.float32, device=f.device) if ctx.needs_input_grad[0] else None
        call("slic_nce_scores_fwd", ptr(bank), ptr(idx), ptr(f), B, K1, D, float(T), ptr(out), ptr(rows), stream())
        ctx.T, ctx.shape, ctx.rows = float(T), (B, K1, D), rows
        return out

    @staticmethod
    def backward(ctx, g):
        B, K1, D = ctx.shape
        g = g.contiguous().float()
        df = torch.empty(B, D, dtype=torch.float32, device=g.device)
        ident = torch.arange(B * K1, dtype=torch.long, device=g.device).view(B, K1)
        call("slic_nce_scores_bwd", ptr(ctx.rows), ptr(ident), ptr(g), B, K1, D, ctx.T, ptr(df), stream())
        ctx.rows = None
        return df, None, None, None


class NCEAverage(nn.Module):
    # outputSize = ndata, inputSize = num of features
    def __init__(self, inputSize, outputSize, K, T=0.07, momentum=0.5, use_softmax=True):
        super(NCEAverage, self).__init__()
        _lib.load()
        self.nLem = outputSize
        self.unigrams = torch.ones(self.nLem)
        self.multinomial = AliasMethod(self.unigrams)
        self.multinomial.cuda()
        self.K = K
        self.use_softmax = use_softmax
        self.register_buffer('params', torch.tensor([K, T, -1, -1, momentum]))
        stdv = 1. / math.sqrt(inputSize / 3)
        self.register_buffer('memory_l', torch.rand(outputSize, inputSize).mul_(2 * stdv).add_(-stdv))
        self.register_buffer('memory_ab', torch.rand(outputSize, inputSize).mul_(2 * stdv).add_(-stdv))

    def forward(self, l, ab, y, idx=None):  # index = y = label
        K, T, momentum = self._host_params()
        batchSize = l.size(0)
        if not l.is_cuda:
            raise _lib.SlicError("NCEAverage needs device tensors (no CPU fallback)")
        if idx is None:
            idx = self.multinomial.draw(batchSize * (self.K + 1)).view(batchSize, -1)
            idx.select(1, 0).copy_(y.data)
        idx = idx.contiguous()
        y = y.contiguous()
        # out_ab scores ab against memory_l, out_l scores l against memory_ab (NCE_loss.py:41-48)
        out_ab = _BankScores.apply(ab, self.memory_l, idx, T)
        out_l = _BankScores.apply(l, self.memory_ab, idx, T)
        if not self.use_softmax:
            # NCE_loss.py:54-71.  The reference sets Z from the RAW dot products (before the division by T): mean * outputSize
            outputSize = self.memory_l.size(0)
            Z_l, Z_ab = self.params[2].item(), self.params[3].item()
            if Z_l < 0:
                self.params[2] = out_l.detach().mean() * T * outputSize
                Z_l = self.params[2].item()
                print("normalization constant Z_l is set to {:.1f}".format(Z_l))
            if Z_ab < 0:
                self.params[3] = out_ab.detach().mean() * T * outputSize
                Z_ab = self.params[3].item()
                print("normalization constant Z_ab is set to {:.1f}".format(Z_ab))
            out_l = torch.exp(torch.div(out_l, Z_l))
            out_ab = torch.exp(torch.div(out_ab, Z_ab))
        with torch.no_grad():   # update memory (NCE_loss.py:73-86)
            B, D = l.shape
            call("slic_nce_bank_update", ptr(self.memory_l), ptr(y), ptr(l.detach().contiguous().float()), B, D,
                 float(momentum), stream())
            call("slic_nce_bank_update", ptr(self.memory_ab), ptr(y), ptr(ab.detach().contiguous().float()), B, D,
                 float(momentum), stream())
        return out_l, out_ab

    def _host_params(self):
        """(K, T, momentum) as Python numbers without a device round trip per step: `params` is a registered buffer (the reference
        reads it with .item() in every forward, NCE_loss.py:27-31); the host copy is refreshed when the buffer is written to"""
        key = (self.params.data_ptr(), self.params._version)
        if getattr(self, "_params_key", None) != key:
            v = self.params.detach().cpu().tolist()
            self._params_host = (int(v[0]), float(v[1]), float(v[4]))
            self._params_key = key
        return self._params_host

    def softmax_loss(self, l, ab, y, idx=None):
        """== NCESoftmaxLoss()(out_l) + NCESoftmaxLoss()(out_ab) for (out_l, out_ab) = self(l, ab, y, idx), banks updated the same
        way — the contrastive step of online_train.py:175-190 as three launches instead of a dozen.  Returns (loss, out_l, out_ab)
        with the outputs detached ([B, K+1, 1], for logging: the reference's loop only uses them through the loss)."""
        if not self.use_softmax:
            raise NotImplementedError("softmax_loss is the use_softmax=True step; NCECriterion goes through forward()")
        if not l.is_cuda:
            raise _lib.SlicError("NCEAverage needs device tensors (no CPU fallback)")
        _, T, momentum = self._host_params()
        B = l.size(0)
        if idx is None:
            idx = self.multinomial.draw(B * (self.K + 1)).view(B, -1)
            idx.select(1, 0).copy_(y.data)
        loss, scores = _FusedContrastStep.apply(l, ab, self.memory_l, self.memory_ab, idx.contiguous(), y.contiguous(), T, momentum)
        return loss, scores[1].unsqueeze(-1), scores[0].unsqueeze(-1)


_NCE_PARTS = 16          # slic_hip.h: SLIC_NCE_PARTS


class _FusedContrastStep(torch.autograd.Function):
    """contrast(l, ab, y) + NCESoftmaxLoss on both outputs as ONE autograd node over three launches (csrc/nce.hip:
    nce_fused_fwd / nce_fused_update / nce_fused_bwd)"""

    @staticmethod
    def forward(ctx, l, ab, mem_l, mem_ab, idx, y, T, momentum):
        l = l.contiguous().float()
        ab = ab.contiguous().float()
        B, D = l.shape
        K1 = idx.shape[1]
        dev = l.device
        scores = torch.empty(2, B, K1, dtype=torch.float32, device=dev)
        rows = torch.empty(2, B, K1, D, dtype=torch.float32, device=dev)
        # [lse | rowloss][side][b], then the SLIC_NCE_PARTS (max, sum-exp) pieces of every score row, then the loss
        nstat = 4 * B
        buf = torch.empty(nstat + 4 * B * _NCE_PARTS + 1, dtype=torch.float32, device=dev)
        stat, part, loss = buf[:nstat].view(2, 2, B), buf[nstat:-1], buf[-1]
        call("slic_nce_fused_fwd", ptr(mem_l), ptr(mem_ab), ptr(l), ptr(ab), ptr(idx), B, K1, D, float(T), ptr(scores), ptr(rows),
             ptr(part), stream())
        call("slic_nce_fused_update", ptr(mem_l), ptr(mem_ab), ptr(y), ptr(l), ptr(ab), B, D, float(momentum), ptr(part), ptr(scores),
             K1, ptr(stat[0]), ptr(stat[1]), ptr(loss), stream())
        ctx.mark_non_differentiable(scores)
        ctx.T, ctx.shape = float(T), (B, K1, D)
        # through save_for_backward: the scores handed back for logging are the buffer the backward reads, and a caller's in-place
        # edit must trip autograd's version check instead of corrupting the gradients; a second backward (retain_graph) works
        ctx.save_for_backward(rows, scores, stat)
        return loss, scores

    @staticmethod
    def backward(ctx, g, _gs):
        B, K1, D = ctx.shape
        rows, scores, stat = ctx.saved_tensors
        df = torch.empty(2, B, D, dtype=torch.float32, device=g.device)
        call("slic_nce_fused_bwd", ptr(rows), ptr(scores), ptr(stat[0]), B, K1, D, ctx.T, ptr(g.contiguous().float()), ptr(df), stream())
        return df[1], df[0], None, None, None, None, None, None


class _SoftmaxCE0(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, K1 = x.shape
        lse = torch.empty(B, dtype=torch.float32, device=x.device)
        rowloss = torch.empty(B, dtype=torch.float32, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        call("slic_softmax_ce0_fwd", ptr(x), B, K1, ptr(lse), ptr(rowloss), ptr(loss), stream())
        ctx.save_for_backward(x, lse)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, lse = ctx.saved_tensors
        B, K1 = x.shape
        dx = torch.empty_like(x)
        call("slic_softmax_ce0_bwd", ptr(x), ptr(lse), B, K1, ptr(g.contiguous().float()), ptr(dx), stream())
        return dx


class NCESoftmaxLoss(nn.Module):
    """Softmax cross-entropy loss (a.k.a., info-NCE loss in CPC paper) against class 0"""

    def __init__(self):
        super(NCESoftmaxLoss, self).__init__()

    def forward(self, x):
        bsz = x.shape[0]
        x = x.reshape(bsz, -1).contiguous().float()      # x.squeeze() of [B, K+1, 1]
        return _SoftmaxCE0.apply(x)


class NCECriterion(nn.Module):
    """Eq. (12) L_NCE of the CMC paper (loss/NCE_loss.py:312-337) on the use_softmax=False outputs [B, K+1, 1]:
    -(sum_b log(P_pos / (P_pos + m Pn + eps)) + sum_{b,k} log(m Pn / (P_neg + m Pn + eps))) / B with Pn = 1 / n_data"""

    def __init__(self, n_data):
        super(NCECriterion, self).__init__()
        self.n_data = n_data

    def forward(self, x):
        eps = 1e-7
        bsz = x.shape[0]
        m = x.size(1) - 1
        Pn = 1 / float(self.n_data)
        P_pos = x.select(1, 0)
        log_D1 = torch.div(P_pos, P_pos.add(m * Pn + eps)).log_()
        P_neg = x.narrow(1, 1, m)
        log_D0 = torch.div(P_neg.clone().fill_(m * Pn), P_neg.add(m * Pn + eps)).log_()
        return - (log_D1.sum(0) + log_D0.view(-1, 1).sum(0)) / bsz


class NCEAverage_intra_neg(NCEAverage):
    """NCEAverage with a third bank of intra-video negatives (loss/NCE_loss.py:91-184): each output scores the K+1 sampled rows of
    the opposite bank followed by the same rows of `memory_neg` -> [B, 2(K+1), 1]; all three banks get the momentum update.
    The same score / update kernels as NCEAverage, four score launches and three updates."""

    def __init__(self, inputSize, outputSize, K, T=0.07, momentum=0.5, use_softmax=True):
        if not torch.cuda.is_available():
            raise _lib.SlicError("NCEAverage_intra_neg needs a gfx950 device (no CPU fallback)")
        super(NCEAverage_intra_neg, self).__init__(inputSize, outputSize, K, T, momentum, use_softmax)
        stdv = 1. / math.sqrt(inputSize / 3)
        self.register_buffer('memory_neg', torch.rand(outputSize, inputSize).mul_(2 * stdv).add_(-stdv))

    def forward(self, l, ab, neg, y, idx=None):
        K, T, momentum = self._host_params()
        batchSize = l.size(0)
        if not l.is_cuda:
            raise _lib.SlicError("NCEAverage_intra_neg needs device tensors (no CPU fallback)")
        if idx is None:
            idx = self.multinomial.draw(batchSize * (self.K + 1)).view(batchSize, -1)
            idx.select(1, 0).copy_(y.data)
        idx = idx.contiguous()
        y = y.contiguous()
        # :124-137: the bank's rows, then memory_neg's rows at the same indices
        out_ab = torch.cat((_BankScores.apply(ab, self.memory_l, idx, T), _BankScores.apply(ab, self.memory_neg, idx, T)), 1)
        out_l = torch.cat((_BankScores.apply(l, self.memory_ab, idx, T), _BankScores.apply(l, self.memory_neg, idx, T)), 1)
        if not self.use_softmax:
            # :145-159.  Unlike NCEAverage, Z comes from the mean of exp(score / T) and divides the exponential
            outputSize = self.memory_l.size(0)
            out_ab = torch.exp(out_ab)
            out_l = torch.exp(out_l)
            Z_l, Z_ab = self.params[2].item(), self.params[3].item()
            if Z_l < 0:
                self.params[2] = out_l.detach().mean() * outputSize
                Z_l = self.params[2].item()
                print("normalization constant Z_l is set to {:.1f}".format(Z_l))
            if Z_ab < 0:
                self.params[3] = out_ab.detach().mean() * outputSize
                Z_ab = self.params[3].item()
                print("normalization constant Z_ab is set to {:.1f}".format(Z_ab))
            out_l = torch.div(out_l, Z_l).contiguous()
            out_ab = torch.div(out_ab, Z_ab).contiguous()
        with torch.no_grad():   # update memory (:161-182)
            B, D = l.shape
            for bank, f in ((self.memory_l, l), (self.memory_ab, ab), (self.memory_neg, neg)):
                call("slic_nce_bank_update", ptr(bank), ptr(y), ptr(f.detach().contiguous().float()), B, D, float(momentum), stream())
        return out_l, out_ab

    def softmax_loss(self, *args, **kwargs):
        raise NotImplementedError("the fused step is NCEAverage's; NCEAverage_intra_neg goes through forward()")


_MOCO_PARTS, _MOCO_DQ_PARTS = 256, 128          # slic_hip.h: SLIC_MOCO_PARTS, SLIC_MOCO_DQ_PARTS


class HipMoCoKernels:
    """the device side of MemoryMoCo (csrc/moco.hip).  `MemoryMoCo(kernels=)` takes another provider with the same methods (tests of
    the host logic on a GPU-less machine pass a NumPy one as an ARGUMENT; the product has no other)."""

    def __init__(self):
        _lib.load()

    def check(self, *tensors):
        for t in tensors:
            if t is not None and not t.is_cuda:
                raise _lib.SlicError("MemoryMoCo needs device tensors (no CPU fallback)")

    def resident(self, t):
        return t.contiguous().float()

    def logits_fwd(self, q, k, memory, T):
        (B, D), K = q.shape, memory.shape[0]
        out = torch.empty(B, K + 1, dtype=torch.float32, device=q.device)
        call("slic_moco_logits_fwd", ptr(q), ptr(k), ptr(memory), B, K, D, float(T), ptr(out), stream())
        return out

    def logits_bwd(self, dout, k, memory, T):
        (B, D), K = k.shape, memory.shape[0]
        dq = torch.empty(B, D, dtype=torch.float32, device=k.device)
        ws = _lib.workspace(_MOCO_DQ_PARTS * B * D * 4, k.device, tag="moco")
        call("slic_moco_logits_bwd", ptr(dout), ptr(k), ptr(memory), B, K, D, float(T), ptr(dq), ptr(ws), stream())
        return dq

    def ce_fwd(self, q, k, memory, T, k_label, queue_label):
        """-> (loss, stat [4, B] = logit[:, 0], lse, npos, row loss)"""
        (B, D), K = q.shape, memory.shape[0]
        buf = torch.empty(4 * B + 1, dtype=torch.float32, device=q.device)
        ws = _lib.workspace(_MOCO_PARTS * B * 16, q.device, tag="moco")
        call("slic_moco_ce_fwd", ptr(q), ptr(k), ptr(memory), B, K, D, float(T), ptr(k_label), ptr(queue_label), ptr(buf),
             ptr(buf[4 * B:]), ptr(ws), stream())
        return buf[4 * B], buf[:4 * B].view(4, B)

    def ce_bwd(self, q, k, memory, T, k_label, queue_label, stat):
        """-> d loss / d q [B, D]; memory and the labels as ce_fwd saw them"""
        (B, D), K = q.shape, memory.shape[0]
        dq = torch.empty(B, D, dtype=torch.float32, device=q.device)
        ws = _lib.workspace(_MOCO_DQ_PARTS * B * D * 4, q.device, tag="moco")
        call("slic_moco_ce_bwd", ptr(q), ptr(k), ptr(memory), B, K, D, float(T), ptr(k_label), ptr(queue_label), ptr(stat), None,
             ptr(dq), ptr(ws), stream())
        return dq

    def enqueue(self, memory, queue_label, k, k_label, index):
        (B, D), K = k.shape, memory.shape[0]
        call("slic_moco_enqueue", ptr(memory), ptr(queue_label), ptr(k), ptr(k_label), B, K, D, int(index), stream())


class _MoCoLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, memory, T, kern, keep):
        out = kern.logits_fwd(kern.resident(q), k, memory, T)
        ctx.T, ctx.kern = T, kern
        if keep:
            # forward() enqueues right after scoring: the backward gets the queue as it was scored (the reference clones it too, :214)
            ctx.save_for_backward(k, memory.clone())
        return out

    @staticmethod
    def backward(ctx, g):
        k, mem = ctx.saved_tensors
        return ctx.kern.logits_bwd(ctx.kern.resident(g), k, mem, ctx.T), None, None, None, None, None


class _MoCoFusedStep(torch.autograd.Function):
    """the loss of a MoCo step as one autograd node.  The queue changes right after the forward, so d loss / d q is computed here,
    against the queue as scored, and the backward only scales it: a later forward cannot reach into an earlier step's gradient."""

    @staticmethod
    def forward(ctx, q, k, memory, T, k_label, queue_label, kern, keep):
        q = kern.resident(q)
        loss, stat = kern.ce_fwd(q, k, memory, T, k_label, queue_label)
        if keep:
            ctx.save_for_backward(kern.ce_bwd(q, k, memory, T, k_label, queue_label, stat))
        return loss

    @staticmethod
    def backward(ctx, g):
        dq, = ctx.saved_tensors
        return dq * g, None, None, None, None, None, None, None


class MemoryMoCo(nn.Module):
    """Fixed-size queue with momentum encoder (loss/NCE_loss.py:188-241).  forward(q, k) -> out [B, K+1] (also for B = 1, where the
    reference's squeeze() drops the batch dimension), the batch of keys enqueued at `index` inside the call.
    Extensions, keyword-only: labels=True adds the buffer `queue_label` [K] (int64, -1 = empty slot) for the multi-positive loss of
    softmax_loss(q, k, k_label); kernels= takes another kernel provider (see HipMoCoKernels)."""

    def __init__(self, inputSize, outputSize, K, T=0.07, use_softmax=False, *, labels=False, kernels=None):
        super(MemoryMoCo, self).__init__()
        self.outputSize = outputSize
        self.inputSize = inputSize
        self.queueSize = K
        self.T = T
        self.index = 0
        self.use_softmax = use_softmax
        self.labels = bool(labels)
        self._kernels = kernels

        self.register_buffer('params', torch.tensor([-1]))
        stdv = 1. / math.sqrt(inputSize / 3)
        self.register_buffer('memory', torch.rand(self.queueSize, inputSize).mul_(2 * stdv).add_(-stdv))
        if self.labels:
            self.register_buffer('queue_label', torch.full((self.queueSize,), -1, dtype=torch.long))
        print('using queue shape: ({},{})'.format(self.queueSize, inputSize))

    def _kern(self):
        if self._kernels is None:
            self._kernels = HipMoCoKernels()
        return self._kernels

    def _host_Z(self):
        """params[0] as a Python number without a device round trip per step (see NCEAverage._host_params)"""
        key = (self.params.data_ptr(), self.params._version)
        if getattr(self, "_params_key", None) != key:
            self._Z_host = self.params[0].item()
            self._params_key = key
        return self._Z_host

    def _inputs(self, q, k, k_label):
        if q.dim() != 2 or q.shape != k.shape or q.shape[1] != self.inputSize:
            raise ValueError("MemoryMoCo expects q and k of shape [B, {}], got {} and {}".format(
                self.inputSize, tuple(q.shape), tuple(k.shape)))
        if q.shape[0] > self.queueSize:
            raise ValueError("MemoryMoCo: a batch of {} keys does not fit a queue of {} rows (the reference's index_copy_ with "
                             "repeated indices is undefined)".format(q.shape[0], self.queueSize))
        if k_label is not None and not self.labels:
            raise ValueError("MemoryMoCo: k_label needs a module built with labels=True")
        kern = self._kern()
        kern.check(q, k, k_label, self.memory)
        k = kern.resident(k.detach())
        if self.labels:
            # a step without labels leaves empty slots behind, never stale labels
            k_label = (torch.full((q.shape[0],), -1, dtype=torch.long, device=q.device) if k_label is None
                       else k_label.detach().contiguous().long())
        return kern, k, k_label

    def _enqueue(self, kern, k, k_label):
        with torch.no_grad():   # update memory (:233-239)
            kern.enqueue(self.memory, self.queue_label if self.labels else None, k, k_label, self.index)
            self.index = (self.index + k.shape[0]) % self.queueSize

    def forward(self, q, k):
        kern, k, k_label = self._inputs(q, k, None)
        out = _MoCoLogits.apply(q, k, self.memory, self.T, kern, torch.is_grad_enabled() and q.requires_grad)
        if not self.use_softmax:
            out = torch.exp(out)
            if self._host_Z() < 0:
                self.params[0] = out.detach().mean() * self.outputSize
                print("normalization constant Z is set to {:.1f}".format(self._host_Z()))
            out = torch.div(out, self._host_Z()).contiguous()
        self._enqueue(kern, k, k_label)
        return out

    def softmax_loss(self, q, k, k_label=None):
        """== NCESoftmaxLoss()(self(q, k)) with the same queue update, without the [B, K+1] logits.  With k_label [B] (labels=True):
        row b's positives are column 0 and every queue row of its label; loss = mean_b -(sum_pos log_softmax) / n_pos
        (online_train.py:96-97 on the mask of models/infoNCE.py:281-283), and the labels are enqueued with the keys."""
        if not self.use_softmax:
            raise NotImplementedError("softmax_loss is the use_softmax=True step; the exp / Z outputs go through forward()")
        multi = k_label is not None
        kern, k, k_label = self._inputs(q, k, k_label)
        loss = _MoCoFusedStep.apply(q, k, self.memory, self.T, k_label if multi else None, self.queue_label if multi else None, kern,
                                    torch.is_grad_enabled() and q.requires_grad)
        self._enqueue(kern, k, k_label)
        return loss

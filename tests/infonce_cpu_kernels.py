"""float64 NumPy provider with the methods of models.infoNCE.HipInfoNCEKernels: the reference of the GPU tests of the rank kernels
and the projection head, and the device stand-in of the host-logic tests (InfoNCE(kernels=NumpyInfoNCEKernels()) on a GPU-less
machine).  Tensors in, float64 / int32 tensors out."""
import numpy as np
import torch

from moco_cpu_kernels import NumpyMoCoKernels, _np, logits, positives
from optim_cpu_kernels import CpuOptimKernels

EPS = 1e-12


def rank_of_best(x, mask):
    """columns ordered by descending x, ties by ascending column: the number of columns ahead of the first masked column of every
    row; C for a row without one"""
    B, C = x.shape
    col = np.arange(C)[None, :]
    has = mask.any(1)
    bv = np.where(mask, x, -np.inf).max(1)
    bc = np.where(mask & (x == bv[:, None]), col, C).min(1)
    ahead = (x > bv[:, None]) | ((x == bv[:, None]) & (col < bc[:, None]))
    return np.where(has, ahead.sum(1), C).astype(np.int64)


def hits_of(rank, top_ks):
    return np.array([(rank < k).sum() for k in top_ks], np.int32)


def moco_rank(q, k, memory, T, k_label=None, queue_label=None):
    """unsaturated float64 rank of the best positive of slic_moco_topk_hits' logits"""
    x = logits(q, k, memory, T)
    return rank_of_best(x, positives(q.shape[0], memory.shape[0], k_label, queue_label))


def head(feat, w1, b1, w2, b2):
    """-> (y, h, z, n): y = z / max(|z|, eps), z = W2 relu(W1 feat + b1) + b2"""
    h = np.maximum(feat @ w1.reshape(w1.shape[0], -1).T + b1, 0.0)
    z = h @ w2.reshape(w2.shape[0], -1).T + b2
    n = np.maximum(np.linalg.norm(z, axis=1, keepdims=True), EPS)
    return z / n, h, z, n


def head_grads(dy, feat, w1, b1, w2, b2):
    y, h, z, n = head(feat, w1, b1, w2, b2)
    clamped = np.linalg.norm(z, axis=1, keepdims=True) <= EPS
    dz = np.where(clamped, dy / n, (dy - y * (dy * y).sum(1, keepdims=True)) / n)
    gw2, gb2 = dz.T @ h, dz.sum(0)
    dh = (dz @ w2.reshape(w2.shape[0], -1)) * (h > 0)
    gw1, gb1 = dh.T @ feat, dh.sum(0)
    return dh @ w1.reshape(w1.shape[0], -1), gw1.reshape(w1.shape), gb1, gw2.reshape(w2.shape), gb2


class NumpyInfoNCEKernels(NumpyMoCoKernels):
    def __init__(self):
        self.optim_kernels = CpuOptimKernels()                  # works on float64 parameters: the model under test is .double()

    def topk_hits(self, q, k, memory, T, k_label, queue_label, top_ks):
        r = np.minimum(moco_rank(_np(q), _np(k), _np(memory), T, _np(k_label), _np(queue_label)), max(top_ks))
        return torch.from_numpy(r.astype(np.int32)), torch.from_numpy(hits_of(r, top_ks))

    def mask_hits(self, output, mask, top_ks):
        r = rank_of_best(_np(output), _np(mask) != 0)
        return torch.from_numpy(r.astype(np.int32)), torch.from_numpy(hits_of(r, top_ks))

    def head_fwd(self, feat, w1, b1, w2, b2):
        y = head(*(_np(t) for t in (feat, w1, b1, w2, b2)))[0]
        return torch.from_numpy(y), (feat.detach().double(), b1.detach().double(), b2.detach().double())

    def head_bwd(self, dy, y, saved, w1, w2, need_dx):
        feat, b1, b2 = saved
        return tuple(torch.from_numpy(np.ascontiguousarray(g)) for g in head_grads(_np(dy), _np(feat), _np(w1), _np(b1), _np(w2), _np(b2)))

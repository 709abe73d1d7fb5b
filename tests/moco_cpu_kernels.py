"""float64 NumPy provider with the methods of loss.NCE_loss.HipMoCoKernels: the reference of the MoCo kernels' GPU tests and the
device stand-in of the host-logic tests (MemoryMoCo(kernels=NumpyMoCoKernels()) on a GPU-less machine).  Tensors in, float64
tensors out."""
import numpy as np
import torch


def _np(t):
    return None if t is None else t.detach().cpu().numpy().astype(np.float64 if t.is_floating_point() else np.int64)


def logits(q, k, memory, T):
    """[B, K+1] float64: column 0 = <q_b, k_b> / T, column 1 + j = <memory_j, q_b> / T"""
    return np.concatenate([(q * k).sum(1, keepdims=True), q @ memory.T], 1) / T


def positives(B, K, k_label, queue_label):
    """[B, K+1] bool: column 0, and every queue slot that carries the row's label (an empty slot, -1, never does)"""
    mask = np.zeros((B, K + 1), bool)
    mask[:, 0] = True
    if k_label is not None:
        mask[:, 1:] = (k_label[:, None] == queue_label[None, :]) & (queue_label[None, :] >= 0)
    return mask


def ce(q, k, memory, T, k_label=None, queue_label=None):
    """-> (loss, dq, stat [4, B]) of mean_b -(sum_pos log_softmax) / n_pos, all float64"""
    B, K = q.shape[0], memory.shape[0]
    x = logits(q, k, memory, T)
    mx = x.max(1, keepdims=True)
    lse = (mx + np.log(np.exp(x - mx).sum(1, keepdims=True)))[:, 0]
    mask = positives(B, K, k_label, queue_label)
    npos = mask.sum(1).astype(np.float64)
    rowloss = lse - (x * mask).sum(1) / npos
    c = (np.exp(x - lse[:, None]) - mask / npos[:, None]) / (B * T)
    dq = c[:, :1] * k + c[:, 1:] @ memory
    return rowloss.mean(), dq, np.stack([x[:, 0], lse, npos, rowloss])


class NumpyMoCoKernels:
    def check(self, *tensors):
        pass

    def resident(self, t):
        return t.contiguous().double()

    def logits_fwd(self, q, k, memory, T):
        return torch.from_numpy(logits(_np(q), _np(k), _np(memory), T))

    def logits_bwd(self, dout, k, memory, T):
        g = _np(dout)
        return torch.from_numpy((g[:, :1] * _np(k) + g[:, 1:] @ _np(memory)) / T)

    def ce_fwd(self, q, k, memory, T, k_label, queue_label):
        loss, _, stat = ce(_np(q), _np(k), _np(memory), T, _np(k_label), _np(queue_label))
        return torch.tensor(loss, dtype=torch.float64), torch.from_numpy(stat)

    def ce_bwd(self, q, k, memory, T, k_label, queue_label, stat):
        return torch.from_numpy(ce(_np(q), _np(k), _np(memory), T, _np(k_label), _np(queue_label))[1])

    def enqueue(self, memory, queue_label, k, k_label, index):
        ids = (index + torch.arange(k.shape[0])) % memory.shape[0]
        memory.index_copy_(0, ids, k.to(memory.dtype))
        if queue_label is not None:
            queue_label.index_copy_(0, ids, k_label)

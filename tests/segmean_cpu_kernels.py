"""TEST-ONLY mirrors of slic_segment_mean (include/slic_hip.h) and the NumPy provider that coclr_classify's functions take as
`kernels=` on the CPU:

    check_segments      the entry point's argument rules, raising ValueError with the rule's name
    segment_mean64      the definition in float64
    segment_mean32      float32 in the kernel's order: row maximum, sum of exp over 64 strided lanes folded by the xor butterfly,
                        exp(x - max) / sum added row by row in ascending r with the compensation term, w * sum rounded, then added
                        to the table
    NumpyClassifyKernels   HipClassifyKernels' methods on CPU tensors; `calls` lists (method name, detail) in call order

Never shipped, never imported by the package."""
import numpy as np
import torch

from clip_transforms_cpu_kernels import NumpyClipKernels
from validate_cpu_kernels import label_hits as label_hits_np

MAX_C = 4096


def check_segments(R, C, seg_off, rows, w, table_rows, ld=None, ldt=None):
    seg_off, rows = np.asarray(seg_off, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    V = len(rows)
    if len(seg_off) != V + 1 or len(w) != V or V < 1 or R < 1 or table_rows < 1:
        raise ValueError("sizes")
    if not 1 <= C <= MAX_C:
        raise ValueError("C outside [1, 4096]")
    if (ld is not None and ld < C) or (ldt is not None and ldt < C):
        raise ValueError("pitch below C")
    if seg_off[0] < 0 or seg_off[-1] > R:
        raise ValueError("offsets leave the rows")
    d = np.diff(seg_off)
    if (d < 0).any():
        raise ValueError("offsets not ascending")
    if (d == 0).any():
        raise ValueError("empty segment")
    if (rows < 0).any() or (rows >= table_rows).any():
        raise ValueError("row outside the table")
    if len(set(rows.tolist())) != V:
        raise ValueError("rows not distinct")


def softmax64(x):
    """rowwise softmax in float64 by the kernel's rule: a -inf beside a finite maximum is exactly 0, the rest as IEEE has it"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - x.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)


def segment_mean64(x, seg_off, rows, w, table, mode, accumulate):
    """-> a float64 copy of `table` [T, C] after the call (rows no segment addresses keep their values)"""
    x = np.asarray(x, dtype=np.float64)
    out = np.array(table, dtype=np.float64)
    f = softmax64(x) if mode == 1 else x
    for v, row in enumerate(rows):
        s = np.float64(w[v]) * f[seg_off[v]:seg_off[v + 1]].sum(axis=0)          # w as given: the caller rounds it to fp32 or not
        out[row] = out[row] + s if accumulate else s
    return out


def _butterfly(lanes):
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ o]
    return lanes[0]


def segment_mean32(x, seg_off, rows, w, table, mode, accumulate):
    """the same in float32, every sum in the kernel's order; `table` (float32 [T, C]) is updated in place and returned"""
    x = np.asarray(x, dtype=np.float32)
    C = x.shape[1]
    w = np.asarray(w, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        def add(acc, comp, val):             # seg_add: Neumaier's compensated addition, column by column
            t = acc + val
            comp += np.where(np.abs(acc) >= np.abs(val), (acc - t) + val, (val - t) + acc)
            return t

        for v, row in enumerate(rows):
            acc, comp = np.zeros(C, dtype=np.float32), np.zeros(C, dtype=np.float32)
            for r in range(seg_off[v], seg_off[v + 1]):
                if mode == 1:
                    m = np.float32(np.fmax.reduce(x[r], initial=-np.inf))          # fmaxf: a NaN does not become the maximum
                    e = np.exp(x[r] - m, dtype=np.float32)
                    lanes = np.zeros(64, dtype=np.float32)
                    for j0 in range(0, C, 64):          # lane l adds columns l, l + 64, ... in that order
                        part = e[j0:j0 + 64]
                        lanes[:len(part)] = lanes[:len(part)] + part
                    acc = add(acc, comp, e / _butterfly(lanes))
                else:
                    acc = add(acc, comp, x[r])
            y = (w[v] * np.where(np.isfinite(comp), acc + comp, acc)).astype(np.float32)
            table[row, :C] = table[row, :C] + y if accumulate else y
    return table


def target_ranks(table, targets):
    """rank[b] = #{j : x[b][j] > x[b][t]} + #{j < t : x[b][j] == x[b][t]} (slic_softmax_ce_fwd's rule), int64 [B]"""
    x = np.asarray(table)
    t = np.asarray(targets, dtype=np.int64)
    xt = x[np.arange(len(t)), t][:, None]
    before = np.arange(x.shape[1])[None, :] < t[:, None]
    return ((x > xt) | ((x == xt) & before)).sum(axis=1)


def topk64(q, g, k):
    """[Nq, k] int32: the k rows of g of largest cosine similarity to each row of q (float64, ties -> lower index)"""
    q, g = np.asarray(q, dtype=np.float64), np.asarray(g, dtype=np.float64)
    qn = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-300)
    gn = g / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-300)
    return np.argsort(-(qn @ gn.T), axis=1, kind="stable")[:, :k].astype(np.int32)


class NumpyClassifyKernels(object):
    def __init__(self):
        self.reads = 0
        self.calls = []
        self.clip = NumpyClipKernels()

    def segment_mean(self, x, seg_off, rows, w, table, mode, accumulate):
        R, C = x.shape
        check_segments(R, C, seg_off, rows, w, table.shape[0])
        assert table.dtype == torch.float32 and table.shape[1] == C and table.is_contiguous()
        self.calls.append(("segment_mean", dict(R=R, seg_off=list(seg_off), rows=list(rows), w=list(w), mode=mode, accumulate=accumulate,
                                                table=table)))
        segment_mean32(x.detach().numpy(), list(seg_off), list(rows), w, table.numpy(), mode, accumulate)

    def target_hits(self, table, targets):
        self.calls.append(("target_hits", None))
        t = targets.numpy()
        ok = (t >= 0) & (t < table.shape[1])
        rank = np.where(ok, target_ranks(table.numpy(), np.where(ok, t, 0)), -1)
        head = [(~ok).sum(), (rank == 0).sum(), ((rank >= 0) & (rank < 5)).sum()]
        return torch.from_numpy(np.concatenate([head, rank]).astype(np.int32))

    def topk_accuracy(self, logit, target, topk):
        self.calls.append(("topk_accuracy", None))
        rank = torch.from_numpy(target_ranks(logit.detach().numpy(), target.numpy()))
        return [(rank < k).sum().float().mul_(1 / logit.shape[0]) for k in topk]

    def centre(self, feat):
        self.calls.append(("centre", None))
        x = feat.detach().numpy().astype(np.float32)
        return torch.from_numpy(x - x.mean(axis=0, dtype=np.float64).astype(np.float32))

    def topk(self, q, g, k):
        self.calls.append(("topk", k))
        return torch.from_numpy(topk64(q.numpy(), g.numpy(), k))

    def label_hits(self, idx, q_labels, g_labels, top_ks):
        self.calls.append(("label_hits", list(top_ks)))
        return torch.from_numpy(label_hits_np(idx.numpy(), q_labels.numpy(), g_labels.numpy(), top_ks)[1].astype(np.int32))

    def read(self, t):
        self.reads += 1
        self.calls.append(("read", tuple(t.shape)))
        return t.detach().cpu().numpy()

"""
Drop-in for the retrieval / embedding-extraction functions of the reference's evaluate.py and
iic_retrieve_clips.py that sit on the hot path:

    get_distance_matrix(x, y=None, dist_metric)           <- evaluate.py:208-223
    get_closest_data_mat(distance_matrix, top_k)          <- evaluate.py:226-231
    get_topk_acc(distance_matrix, x_labels, y_labels, top_ks)   <- evaluate.py:287-307
    topk_acc_device(x, x_labels, y, y_labels, top_ks, dist_metric)   (the same value, search and counting on the device)
    k_nearest_embeddings(args, model, ..., plot=False)    <- evaluate.py:353-400
    evaluate(model, data_loader, ...) / get_embeddings_and_labels(...)   <- evaluate.py:146-205, 310-350
    topk_retrieval(args | arrays)                          <- iic_retrieve_clips.py:275-314
    knn_classify(x, x_labels, y, y_labels, k, weights)     (not in the reference: weighted k-NN classification accuracy on the top-k lists)
    retrieval_metrics(x, x_labels, y, y_labels, ks)        (not in the reference: precision@k, recall@k, mAP@k, MRR on the top-k lists)

The reference computes an N_q x N_g sklearn cosine_distances matrix on the host and argsorts every row.
Here the matrix (when a caller really wants it) comes from the fp32-MFMA gather-GEMM with a
(1 - s, clamp at 0) epilogue, and the top-k paths never build it: `cosine_topk` fuses the similarity GEMM
with a per-query streaming top-k (csrc/topk.hip); `euclidean_topk` runs the same kernels on q.g - |g|^2 / 2 and
recomputes the winners' distances directly (LOSS.DIST_METRIC 'euclidean').  Plot/heat-map helpers of evaluate.py
are out of scope.  knn_classify / retrieval_metrics consume the [Nq, k] tables where the search leaves them (csrc/knn.hip:
slic_knn_vote, slic_retrieval_ranked; classes with sklearn's names in neighbors.py); k_nearest_embeddings runs the k-NN monitor from its
one search when cfg.VAL.KNN_K > 0 and is otherwise unchanged.
"""
import ctypes
import functools
import json
import os

import numpy as np
import torch

from . import _lib
from ._lib import SlicConvArgs, call, ptr, stream


def __getattr__(name):
    # TOPK_BF16_EPS: the proven bound of |bf16 coarse score - fp32 score| the certified search lowers its thresholds by.  The library's
    # constant is the only copy (slic_cosine_topk_bf16_eps), read when somebody asks for it.
    if name == "TOPK_BF16_EPS":
        return float(_lib.load().slic_cosine_topk_bf16_eps())
    # the pair statistics (pairstats.py) are reachable from here, imported when somebody asks for them
    if name in ("pair_statistics", "view_statistics", "separation", "HipPairStatsKernels"):
        from . import pairstats
        return getattr(pairstats, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


_PRECISIONS = ("fp32", "bf16")


def _check_precision(precision):
    if precision not in _PRECISIONS:
        raise ValueError("precision must be 'fp32' or 'bf16', not %r" % (precision,))


def _dev(x):
    if not torch.cuda.is_available():
        raise _lib.SlicError("retrieval needs a gfx950 device (no CPU fallback)")
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))   # float64 .npy features are cast (D7)
    return x.detach().to(device="cuda", dtype=torch.float32).contiguous()


def _normalize(x, Dp):
    """sklearn normalize(X) rows; feature dim zero-padded to Dp (a multiple of 8)"""
    N, D = x.shape
    out = torch.empty(N, D, dtype=torch.float32, device=x.device)
    call("slic_normalize_rows", ptr(x), N, D, x.stride(0), ptr(out), stream())
    if Dp != D:
        p = torch.zeros(N, Dp, dtype=torch.float32, device=x.device)
        p[:, :D] = out
        out = p
    return out


def cosine_topk_sharded(queries, gallery_shard, k, process_group, row_offset=None, *, precision="fp32"):
    """Gallery sharded by rows across the ranks of `process_group` (queries replicated): every rank searches its
    shard, the [Nq, k] lists are all-gathered (RCCL) and merged on every GPU.  Returned indices are GLOBAL gallery
    rows (rank order == row order unless `row_offset` is given).  precision: as cosine_topk, for every shard's search."""
    _check_precision(precision)

    def search(q, g, k):
        return cosine_topk(q, g, k=k, precision=precision)
    return _topk_sharded(search, queries, gallery_shard, k, process_group, row_offset)


def euclidean_topk_sharded(queries, gallery_shard, k, process_group, row_offset=None):
    """cosine_topk_sharded for the euclidean metric: every rank's lists hold directly computed distances (each
    shard may centre on its own mean), so the merge orders them exactly as the unsharded search would."""
    return _topk_sharded(euclidean_topk, queries, gallery_shard, k, process_group, row_offset)


def _topk_sharded(search, queries, gallery_shard, k, process_group, row_offset):
    import torch.distributed as dist
    W = dist.get_world_size(process_group)
    g = _dev(gallery_shard)
    n_loc = torch.tensor([g.shape[0]], dtype=torch.int64, device=g.device)
    sizes = torch.empty(W, dtype=torch.int64, device=g.device)
    dist.all_gather_into_tensor(sizes, n_loc, group=process_group)
    if row_offset is None:
        row_offset = int(sizes[: dist.get_rank(process_group)].sum().item())
    kk = min(k, g.shape[0])
    idx, dst = search(queries, g, k=kk)
    Nq = idx.shape[0]
    pi = torch.full((Nq, k), -1, dtype=torch.int32, device=g.device)
    pd = torch.full((Nq, k), float("inf"), dtype=torch.float32, device=g.device)
    pi[:, :kk] = idx + row_offset
    pd[:, :kk] = dst
    api = torch.empty(W * Nq * k, dtype=torch.int32, device=g.device)
    apd = torch.empty(W * Nq * k, dtype=torch.float32, device=g.device)
    dist.all_gather_into_tensor(api, pi.reshape(-1), group=process_group)
    dist.all_gather_into_tensor(apd, pd.reshape(-1), group=process_group)
    out_i = torch.empty(Nq, k, dtype=torch.int32, device=g.device)
    out_d = torch.empty(Nq, k, dtype=torch.float32, device=g.device)
    call("slic_topk_merge_lists", ptr(apd), ptr(api), W, Nq, k, ptr(out_i), ptr(out_d), stream())
    return out_i, out_d


def cosine_topk(queries, gallery=None, k=20, *, precision="fp32", info=None):
    """indices [Nq, k] (int32) and cosine distances [Nq, k] of the k nearest gallery rows, ascending;
    gallery=None searches the queries themselves with the diagonal excluded (evaluate.py:221-222).

    precision="bf16": the similarity GEMM runs on the bf16 MFMA as a candidate pass and the result is still the exact top-k — the
    candidates are rescored from the fp32 rows and a per-query certificate (TOPK_BF16_EPS, csrc/topk_bf16.h) decides whether they hold
    the true k best; queries it does not cover are redone by the fp32 kernels.  The library takes the bf16 pass where it measured
    faster (slic_cosine_topk_bf16_plan; SLIC_TOPK_BF16=1 forces it) and the fp32 search elsewhere.  info: a dict that receives
    fallback_queries, overflow_queries, candidates, eps and path ("bf16" / "fp32") — one small device-to-host read, only when asked for."""
    _check_precision(precision)
    lib = _lib.load()
    q = _dev(queries)
    self_mask = gallery is None
    g = q if self_mask else _dev(gallery)
    D = q.shape[1]
    Dp = (D + 7) // 8 * 8
    qn = _normalize(q, Dp)
    gn = qn if self_mask else _normalize(g, Dp)
    Nq, Ng = qn.shape[0], gn.shape[0]
    idx = torch.empty(Nq, k, dtype=torch.int32, device=q.device)
    dist = torch.empty(Nq, k, dtype=torch.float32, device=q.device)
    if precision == "bf16":
        stats = torch.zeros(3, dtype=torch.int32, device=q.device) if info is not None else None
        ws = _lib.workspace(lib.slic_cosine_topk_bf16_workspace_bytes(Nq, Ng, Dp, k), q.device, "topk")
        call("slic_cosine_topk_bf16", ptr(qn), Nq, ptr(gn), Ng, Dp, k, int(self_mask), ptr(idx), ptr(dist), ptr(stats), ptr(ws), stream())
        if info is not None:
            plan = (ctypes.c_int * 6)()
            call("slic_cosine_topk_bf16_plan", Nq, Ng, Dp, k, plan)
            st = stats.tolist()
            info.update(fallback_queries=st[0], overflow_queries=st[1], candidates=st[2], eps=float(lib.slic_cosine_topk_bf16_eps()),
                        path="bf16" if plan[0] else "fp32")
        return idx, dist
    ws = _lib.workspace(lib.slic_cosine_topk_workspace_bytes(Nq, Ng, k), q.device, "topk")
    call("slic_cosine_topk", ptr(qn), Nq, ptr(gn), Ng, Dp, k, int(self_mask), ptr(idx), ptr(dist), ptr(ws), stream())
    if info is not None:
        info.update(fallback_queries=0, overflow_queries=0, candidates=0, eps=float(lib.slic_cosine_topk_bf16_eps()), path="fp32")
    return idx, dist


def euclidean_topk(queries, gallery=None, k=20, *, precision="fp32"):
    """indices [Nq, k] (int32) and euclidean distances [Nq, k] of the k nearest gallery rows, ascending (ties ->
    lower index); gallery=None searches the queries themselves with the diagonal excluded, as cosine_topk does.
    precision: 'fp32' only.  The certified bf16 candidate search of cosine_topk rests on unit rows; for raw rows the error bound of a
    bf16 score scales with |q| |g|, so there is no fixed eps to certify with: precision='bf16' raises ValueError."""
    _check_precision(precision)
    if precision != "fp32":
        raise ValueError("euclidean_topk: precision=%r is not supported (the bf16 candidate search needs unit rows)" % (precision,))
    lib = _lib.load()
    q = _dev(queries)
    self_mask = gallery is None
    g = q if self_mask else _dev(gallery)
    if g.shape[1] != q.shape[1]:
        raise ValueError("euclidean_topk: queries have %d columns, the gallery %d" % (q.shape[1], g.shape[1]))
    Nq, Ng, D = q.shape[0], g.shape[0], q.shape[1]
    idx = torch.empty(Nq, k, dtype=torch.int32, device=q.device)
    dist = torch.empty(Nq, k, dtype=torch.float32, device=q.device)
    ws = _lib.workspace(lib.slic_euclidean_topk_workspace_bytes(Nq, Ng, D, k), q.device, "topk")
    call("slic_euclidean_topk", ptr(q), Nq, q.stride(0), ptr(g), Ng, g.stride(0), D, k, int(self_mask), ptr(idx), ptr(dist),
         ptr(ws), stream())
    return idx, dist


def _topk_search(dist_metric, precision="fp32"):
    _check_precision(precision)
    if dist_metric == 'cosine':
        return cosine_topk if precision == "fp32" else functools.partial(cosine_topk, precision=precision)
    if dist_metric == 'euclidean':
        return euclidean_topk if precision == "fp32" else functools.partial(euclidean_topk, precision=precision)
    raise ValueError("dist_metric must be 'cosine' or 'euclidean', not %r" % (dist_metric,))


def get_distance_matrix(x_embeddings, y_embeddings=None, dist_metric='cosine'):
    """full distance matrix as np.ndarray, like the reference (validation-sized inputs; the top-k paths do not
    need it).  Self-distance diagonal = +inf when y is None."""
    assert (dist_metric in ['cosine', 'euclidean'])
    x = _dev(x_embeddings)
    y = x if y_embeddings is None else _dev(y_embeddings)
    Nx, Ny, D = x.shape[0], y.shape[0], x.shape[1]
    Np = (Ny + 3) // 4 * 4                  # the GEMM epilogue stores 16-byte chunks: row stride and N are multiples of 4
    if dist_metric == 'cosine':
        out = torch.empty(Nx, Np, dtype=torch.float32, device=x.device)[:, :Ny]
        # D = max(0, 1 - x_hat . y_hat): the gather-GEMM as a plain GEMM (1 tap) with scale -1, shift +1, ReLU
        Dp = (D + 31) // 32 * 32
        xn, yn = _normalize(x, Dp), (None if y_embeddings is None else _normalize(y, Dp))
        yn = xn if yn is None else yn
        tab = np.zeros((Dp // 4, 4), np.int32)
        tab[:, 0] = np.arange(Dp // 4) * 4
        tab[:, 1] = (1 << 3) | (1 << 10) | (1 << 17)          # tap offset (0, 0, 0)
        tab[:, 2] = np.arange(Dp // 4) * 4
        tab[:, 3] = 128 | (128 << 8) | (128 << 16)
        tabd = torch.from_numpy(tab).to(x.device)
        sc = torch.full((Np,), -1.0, device=x.device)
        sh = torch.full((Np,), 1.0, device=x.device)
        a = SlicConvArgs()
        a.src, a.wgt, a.dst, a.tab = xn.data_ptr(), yn.data_ptr(), out.data_ptr(), tabd.data_ptr()
        a.src_bytes, a.wgt_bytes = _lib.u32_bytes(xn, 'x_embeddings'), _lib.u32_bytes(yn, 'y_embeddings')
        a.scale, a.shift, a.relu = sc.data_ptr(), sh.data_ptr(), 1
        a.M, a.N, a.nchunks = Nx, Np, Dp // 4       # columns Ny..Np-1: rows past yn's range read as zeros
        a.Cs, a.Ts, a.Hs, a.Ws = Dp, 1, 1, 1
        a.Ga = a.Gb = a.Gc = 1
        a.sa = a.sb = a.sc = 1
        a.ldw, a.ldo = Dp, Np
        call("slic_conv_gemm", ctypes.byref(a), 0, stream())
    else:
        out = torch.empty(Nx, Ny, dtype=torch.float32, device=x.device)
        call("slic_pairwise_euclidean", ptr(x), Nx, ptr(y), Ny, D, ptr(out), stream())
    distance_matrix = out.cpu().numpy()
    if y_embeddings is None:
        np.fill_diagonal(distance_matrix, float('inf'))
    return distance_matrix


def get_closest_data_mat(distance_matrix, top_k):
    """top_k smallest per row, sorted (evaluate.py:226-231) — host numpy on an already materialised matrix"""
    idx = np.argpartition(distance_matrix, top_k, axis=-1)
    unsorted = np.take_along_axis(distance_matrix, idx[:, :top_k], axis=-1)
    order = np.argsort(unsorted, axis=-1)
    return np.take_along_axis(idx, order, axis=-1)


def _acc_from_indices(topk_indices, x_labels, y_labels, top_ks):
    x_labels = np.asarray(x_labels)
    y_labels = np.asarray(y_labels)
    lab = y_labels[topk_indices]                       # [Nq, kmax]
    hit = lab == x_labels[:, None]
    return np.array([hit[:, :k].any(axis=1).mean() for k in top_ks])


def get_topk_acc(distance_matrix, x_labels, y_labels=None, top_ks=[1, 5, 10, 20]):
    """evaluate.py:287-307 on a materialised matrix (kept for drop-in callers)"""
    topk_indices = get_closest_data_mat(distance_matrix, top_k=top_ks[-1])
    if y_labels is None:
        y_labels = x_labels
    return _acc_from_indices(topk_indices, x_labels, y_labels, top_ks)


def get_topk_acc_from_embeddings(x_embeddings, x_labels, y_embeddings=None, y_labels=None, top_ks=[1, 5, 10, 20],
                                 dist_metric='cosine', *, precision="fp32"):
    """the same accuracies without the matrix: fused GEMM + top-k on the device ('cosine' or 'euclidean'; precision: see cosine_topk)"""
    idx, _ = _topk_search(dist_metric, precision)(x_embeddings, y_embeddings, k=top_ks[-1])
    if y_labels is None:
        y_labels = x_labels
    return _acc_from_indices(idx.cpu().numpy(), x_labels, y_labels, top_ks)


def _labels_dev(labels, device):
    if torch.is_tensor(labels):
        return labels.detach().to(device=device, dtype=torch.int64).reshape(-1).contiguous()
    return torch.as_tensor(np.asarray(labels, dtype=np.int64).reshape(-1)).to(device)


def _label_hits(idx, q_labels, g_labels, top_ks, first_hit=None):
    """slic_topk_label_hits on a device-resident [Nq, k] index table: int32 [len(top_ks)] on the device, hits[i] = the number of
    query rows with a same-label gallery row among their first top_ks[i] neighbours (the counting of evaluate.py:296-305)"""
    _lib.require_device(idx)
    idx = idx.to(torch.int32).contiguous()
    q, g = _labels_dev(q_labels, idx.device), _labels_dev(g_labels, idx.device)
    if q.shape[0] != idx.shape[0]:
        raise ValueError("label_hits: %d query labels for %d rows of indices" % (q.shape[0], idx.shape[0]))
    ks = (ctypes.c_int32 * len(top_ks))(*[int(k) for k in top_ks])
    hits = torch.empty(len(top_ks), dtype=torch.int32, device=idx.device)
    call("slic_topk_label_hits", ptr(idx), idx.shape[0], idx.shape[1], ptr(q), ptr(g), g.shape[0], ks, len(top_ks), ptr(first_hit),
         ptr(hits), stream())
    return hits


def topk_acc_device(x_embeddings, x_labels, y_embeddings=None, y_labels=None, top_ks=[1, 5, 10, 20], dist_metric='cosine', *,
                    kernels=None, precision="fp32"):
    """the value get_topk_acc returns (np.ndarray[len(top_ks)], float64) with the search AND the counting on the device: top-k
    search + slic_topk_label_hits, one small read-back of len(top_ks) integers.  Labels: lists, arrays or tensors.
    kernels: a provider with topk / label_hits (validation.HipValidationKernels' interface) instead of the device.
    precision: see cosine_topk (the device search only; a provider keeps its own)."""
    _check_precision(precision)
    if kernels is None:
        idx, _ = _topk_search(dist_metric, precision)(x_embeddings, y_embeddings, k=top_ks[-1])
        hits = _label_hits(idx, x_labels, x_labels if y_labels is None else y_labels, top_ks)
    else:
        idx = kernels.topk(x_embeddings, y_embeddings, top_ks[-1], dist_metric)
        hits = kernels.label_hits(idx, x_labels, x_labels if y_labels is None else y_labels, top_ks)
    return hits.cpu().numpy().astype(np.float64) / idx.shape[0]


def _knn_provider(kernels):
    from .neighbors import HipKnnKernels
    return HipKnnKernels() if kernels is None else kernels       # raises SlicError without a gfx950 device


def _class_count(labels, num_classes):
    """the C of the vote: num_classes, or max label + 1 (host labels: no device work; a device tensor costs one read-back)"""
    if num_classes is None:
        if torch.is_tensor(labels):
            num_classes = int(labels.max()) + 1 if labels.numel() else 1
        else:
            a = np.asarray(labels)
            num_classes = int(a.max()) + 1 if a.size else 1
    return max(int(num_classes), 1)


def _knn_vote_summary(K, idx, dist, q_labels, g_labels, n_classes, weights, temperature, top_n):
    """one vote launch on a [Nq, k] table and the accuracies of its best classes as ONE device tensor:
    [len(top_n) top-n accuracies, the mean per-class accuracy] in float64.  A class counts among a query's n best only with a
    positive score: classes nobody voted for fill the tail of the ranking in class order and say nothing."""
    from .neighbors import WEIGHTS
    n_top = max(top_n)
    _, pred, score = K.vote(idx, dist, g_labels, n_classes, WEIGHTS[weights], temperature, n_top, False)
    match = (pred.to(torch.int64) == q_labels[:, None]) & (score > 0)
    Nq = idx.shape[0]
    accs = [match[:, :n].any(dim=1).sum().to(torch.float64) / Nq for n in top_n]
    # mean per-class accuracy of the top-1 prediction, over the classes that occur among the queries
    ok = (q_labels >= 0) & (q_labels < n_classes)
    ql = q_labels.clamp(0, n_classes - 1)
    per_class_n = torch.bincount(ql[ok], minlength=n_classes).to(torch.float64)
    per_class_hit = torch.bincount(ql[ok & match[:, 0]], minlength=n_classes).to(torch.float64)
    present = per_class_n > 0
    mean_class = (per_class_hit / per_class_n.clamp(min=1))[present].sum() / present.sum().clamp(min=1).to(torch.float64)
    return torch.stack(accs + [mean_class])


def knn_classify(x_embeddings, x_labels, y_embeddings=None, y_labels=None, k=20, weights='softmax', temperature=0.07, top_n=(1, 5),
                 num_classes=None, dist_metric='cosine', *, precision="fp32", kernels=None):
    """Weighted k-NN classification accuracy of the queries x against the gallery y (the k-NN monitor of InstDisc / MoCo / DINO with
    weights='softmax'; sklearn's KNeighborsClassifier with 'uniform' / 'distance'): one top-k search, one slic_knn_vote launch, one
    small read-back.  y_embeddings=None is the leave-one-out form on one set.  Labels are classes 0 .. num_classes - 1 (default:
    max label + 1; gallery labels < 0, noise used as pseudo-labels, never vote).
    -> {'top1': .., 'top5': .. (one per entry of top_n), 'mean_class_acc': .., 'n_queries': Nq}"""
    from .neighbors import WEIGHTS, check_vote_sizes
    _check_precision(precision)
    if weights not in WEIGHTS:
        raise ValueError("weights must be 'uniform', 'distance' or 'softmax', got {!r}".format(weights))
    if dist_metric not in ('cosine', 'euclidean'):
        raise ValueError("dist_metric must be 'cosine' or 'euclidean', not %r" % (dist_metric,))
    top_n = [int(n) for n in top_n]
    if not top_n or min(top_n) < 1:
        raise ValueError("top_n must hold positive integers, got {!r}".format(top_n))
    g_host = x_labels if y_labels is None else y_labels
    n_classes = _class_count(g_host, num_classes)
    check_vote_sizes("knn_classify", k, n_classes, max(top_n))
    K = _knn_provider(kernels)
    q_labels = K.labels(x_labels)
    g_labels = q_labels if y_embeddings is None else K.labels(y_labels)
    idx, dist = K.search(x_embeddings, y_embeddings, int(k), dist_metric, precision)
    rec = K.read(_knn_vote_summary(K, idx, dist, q_labels, g_labels, n_classes, weights, temperature, top_n))
    out = {"top%d" % n: float(rec[i]) for i, n in enumerate(top_n)}
    out["mean_class_acc"] = float(rec[len(top_n)])
    out["n_queries"] = int(idx.shape[0])
    return out


def _n_relevant(q_labels, g_labels, leave_one_out):
    """n_rel [Nq] int32: how many gallery rows carry the query's label (minus the query itself in the leave-one-out form), from a
    label histogram on the labels' own device"""
    both, inverse = torch.unique(torch.cat((q_labels, g_labels)), sorted=True, return_inverse=True)
    hist = torch.bincount(inverse[q_labels.shape[0]:], minlength=both.shape[0])
    n_rel = hist[inverse[:q_labels.shape[0]]]
    return (n_rel - 1 if leave_one_out else n_rel).to(torch.int32)


def retrieval_metrics(x_embeddings, x_labels, y_embeddings=None, y_labels=None, ks=(1, 5, 10, 20, 50), dist_metric='cosine', *,
                      precision="fp32", kernels=None):
    """Ranked retrieval quality of the queries x against the gallery y on the exact top-max(ks) lists: precision@k, recall@k, mAP@k
    (AP@k normalised by min(relevant rows, k)) and the mean reciprocal rank (0 for a query without a hit in the list).  One search,
    slic_retrieval_ranked, one small read-back; y_embeddings=None is the leave-one-out form.  Queries without any relevant gallery row
    stay out of the recall and mAP means (n_with_relevant counts the others); precision and mrr average over all queries.
    -> {'precision': {k: ..}, 'recall': {k: ..}, 'map': {k: ..}, 'mrr': .., 'n_with_relevant': ..}"""
    from .neighbors import MAX_CUTS, MAX_K
    _check_precision(precision)
    if dist_metric not in ('cosine', 'euclidean'):
        raise ValueError("dist_metric must be 'cosine' or 'euclidean', not %r" % (dist_metric,))
    ks = [int(v) for v in ks]
    if not 1 <= len(ks) <= MAX_CUTS or ks != sorted(ks) or ks[0] < 1:
        raise ValueError("ks must be 1 .. {} ascending positive cut-offs, got {!r}".format(MAX_CUTS, ks))
    if ks[-1] > MAX_K:
        raise ValueError("retrieval_metrics: ks up to {} are beyond the {} of the exact top-k search (full-ranking mAP needs every "
                         "relevant row's rank: DESIGN.md section 7j)".format(ks[-1], MAX_K))
    K = _knn_provider(kernels)
    q_labels = K.labels(x_labels)
    loo = y_embeddings is None
    g_labels = q_labels if loo else K.labels(y_labels)
    idx, _ = K.search(x_embeddings, y_embeddings, ks[-1], dist_metric, precision)
    _, _, record = K.ranked(idx, q_labels, g_labels, _n_relevant(q_labels, g_labels, loo), ks)
    rec = K.read(record)
    out = {"precision": {}, "recall": {}, "map": {}}
    for i, k in enumerate(ks):
        out["precision"][k], out["recall"][k], out["map"][k] = (float(v) for v in rec[3 * i:3 * i + 3])
    out["mrr"] = float(rec[3 * len(ks)])
    out["n_with_relevant"] = int(round(float(rec[3 * len(ks) + 1])))
    return out


def _knn_monitor(cfg, kernels, test_embeddings, test_labels, train_embeddings, train_labels):
    """k_nearest_embeddings with VAL.KNN_K > 0: ONE search at max(20, KNN_K) serves both the four retrieval accuracies (the top-20
    prefix of an exact sorted list is the exact top-20) and the k-NN classification monitor on its first KNN_K columns."""
    knn_k = int(cfg.VAL.KNN_K)
    weights = getattr(cfg.VAL, "KNN_WEIGHTS", "softmax")
    temperature = float(getattr(cfg.VAL, "KNN_T", 0.07))
    top_ks = [1, 5, 10, 20]
    K = _knn_provider(kernels)
    q_labels, g_labels = K.labels(test_labels), K.labels(train_labels)
    n_classes = _class_count(train_labels, None)
    from .neighbors import check_vote_sizes
    check_vote_sizes("k_nearest_embeddings (VAL.KNN_K)", knn_k, n_classes, 5)
    idx, dist = K.search(test_embeddings, train_embeddings, max(top_ks[-1], knn_k), cfg.LOSS.DIST_METRIC)
    head = idx[:, :top_ks[-1]].contiguous()
    hits = _label_hits(head, q_labels, g_labels, top_ks) if kernels is None else kernels.label_hits(head, q_labels, g_labels, top_ks)
    acc = hits.cpu().numpy().astype(np.float64) / idx.shape[0]
    knn = K.read(_knn_vote_summary(K, idx[:, :knn_k].contiguous(), dist[:, :knn_k].contiguous(), q_labels, g_labels, n_classes,
                                   weights, temperature, [1, 5]))
    return acc, (float(knn[0]), float(knn[1])), (knn_k, weights)


def k_nearest_embeddings(args, model, cuda, device, train_loader, test_loader, train_data, val_data, cfg, test_split='val',
                         plot=True, epoch=None, is_master_proc=True, evaluate_output=None, num_exemplar=None, service=None,
                         load_pkl=False, out_filename='global_retrieval_acc', *, kernels=None):
    """evaluate.py:353-400 with plot=False (what the training loop passes, online_train.py:737-739): embeddings of the test split and
    of the train split, top-1/5/10/20 retrieval accuracy of test against train on the master, the reference's prints and its line in
    tnet_checkpoints/<out_filename>.txt.  Returns the four accuracies on the master, [] elsewhere.  train_data / val_data are only
    used by the plot."""
    if plot:
        raise NotImplementedError("k_nearest_embeddings(plot=True): the exemplar plot helpers are out of scope; the training loop "
                                  "calls it with plot=False (online_train.py:737-739)")
    if is_master_proc:
        print('Getting embeddings...')
    test_embeddings, test_labels, _ = get_embeddings_and_labels(args, cfg, model, cuda, device, test_loader, split=test_split,
                                                                is_master_proc=is_master_proc, load_pkl=load_pkl)
    train_embeddings, train_labels, _ = get_embeddings_and_labels(args, cfg, model, cuda, device, train_loader, split='train',
                                                                  is_master_proc=is_master_proc, load_pkl=load_pkl)
    acc = []
    print('Computing top1/5/10/20 Acc...')
    knn_k = int(getattr(getattr(cfg, "VAL", None), "KNN_K", 0) or 0)       # opt-in: absent or 0 leaves every step below as it was
    knn = None
    if (is_master_proc):
        if knn_k > 0:
            acc, knn, knn_how = _knn_monitor(cfg, kernels, test_embeddings, test_labels, train_embeddings, train_labels)
        else:
            acc = topk_acc_device(test_embeddings, test_labels, train_embeddings, train_labels, dist_metric=cfg.LOSS.DIST_METRIC,
                                  kernels=kernels)
        if epoch is not None:
            # the reference's format string has two placeholders for its four arguments: the file holds top-1 and top-5
            to_write = 'epoch:{} {:.2f} {:.2f}'.format(epoch, 100.*acc[0], 100.*acc[1], 100.*acc[2], 100.*acc[3])
            to_write += '\n'
            from .online_train import _append_log
            _append_log(cfg, '{}.txt'.format(out_filename), to_write)
        print('Top1 Acc: {:.2f}%, Top5 Acc: {:.2f}%, Top10 Acc: {:.2f}%, Top20 Acc: {:.2f}%'.format(100.*acc[0], 100.*acc[1], 100.*acc[2], 100.*acc[3]))
        if knn is not None:
            print('kNN (k={}, {}) Top1 Acc: {:.2f}%, Top5 Acc: {:.2f}%'.format(knn_how[0], knn_how[1], 100.*knn[0], 100.*knn[1]))
            if epoch is not None:
                from .online_train import _append_log
                _append_log(cfg, 'knn_acc.txt', 'epoch:{} {:.2f} {:.2f}\n'.format(epoch, 100.*knn[0], 100.*knn[1]))
    return acc


def topk_retrieval(args=None, X_train=None, y_train=None, X_test=None, y_test=None, ks=(1, 5, 10, 20, 50),
                   dist_metric='cosine', *, precision="fp32"):
    """iic_retrieve_clips.py:275-314.  Either `args.feature_dir` holds {train,test}_{feature,class}.npy
    ([V, 10, D] features averaged over the 10 clips, :280,287) or arrays are passed directly.
    Returns {k: correct}; writes topk_correct.json next to the features like the reference.
    dist_metric: 'cosine' (the reference's) or 'euclidean'; precision: see cosine_topk."""
    search = _topk_search(dist_metric, precision)
    feature_dir = getattr(args, "feature_dir", None) if args is not None else None
    if feature_dir is not None:
        X_train = np.load(os.path.join(feature_dir, 'train_feature.npy'))
        y_train = np.load(os.path.join(feature_dir, 'train_class.npy'))
        X_test = np.load(os.path.join(feature_dir, 'test_feature.npy'))
        y_test = np.load(os.path.join(feature_dir, 'test_class.npy'))
    X_train, X_test = np.asarray(X_train), np.asarray(X_test)
    y_train, y_test = np.asarray(y_train), np.asarray(y_test)
    if X_train.ndim == 3:
        X_train = np.mean(X_train, 1)
        y_train = y_train[:, 0]
    if X_test.ndim == 3:
        X_test = np.mean(X_test, 1)
        y_test = y_test[:, 0]
    X_train = X_train.reshape((-1, X_train.shape[-1]))
    X_test = X_test.reshape((-1, X_test.shape[-1]))
    y_train, y_test = y_train.reshape(-1), y_test.reshape(-1)
    ks = list(ks)
    idx, _ = search(X_test, X_train, k=min(max(ks), len(X_train)))
    lab = y_train[idx.cpu().numpy()]
    hit = lab == y_test[:, None]
    topk_correct = {k: int(hit[:, :k].any(axis=1).sum()) for k in ks}
    for k in ks:
        correct, total = topk_correct[k], len(X_test)
        print('Top-{}, correct = {:.2f}, total = {}, acc = {:.3f}'.format(k, correct, total, correct / total))
    if feature_dir is not None:
        with open(os.path.join(feature_dir, 'topk_correct.json'), 'w') as fp:
            json.dump(topk_correct, fp)
    return topk_correct


# ------------------------------------------------------------------------------------------------
def evaluate(model, data_loader, device=None, is_master_proc=True, gather=True):
    """evaluate.py:146-205: eval-mode encoder over a loader of (input [b,3,T,S,S], targets [b], info, indexes [b]),
    no grad.  gather=True is the reference's return contract — per batch the (embedding, label, index) triples are
    all-gathered across ranks (misc/distributed_helper) and moved to the host: (Tensor[N',D] cpu, list[int], list[int]).
    gather=False keeps THIS rank's rows resident on its GPU: no collective, no per-batch D2H;
    returns (Tensor[n_local, D] on the device, list[int], list[int]) for the sharded k-means / retrieval to consume."""
    from .misc import distributed_helper as du_helper
    model.eval()
    embedding, vid_info, idxs = [], [], []
    world = du_helper.get_world_size()
    dev = torch.device("cuda") if device is None else torch.device(device)
    with torch.no_grad():
        for batch in data_loader:
            inp, targets, _info, indexes = batch
            inp = inp.to(dev, non_blocking=True)
            embedd = model(inp)
            if isinstance(embedd, tuple):
                embedd = embedd[0]
            embedd = embedd.flatten(1)
            if not gather:
                embedding.append(embedd.detach())
                vid_info.extend(torch.as_tensor(targets).tolist())
                idxs.extend(torch.as_tensor(indexes).tolist())
                continue
            targets = torch.as_tensor(targets).to(dev)
            indexes = torch.as_tensor(indexes).to(dev)
            if world > 1:
                embedd, targets, indexes = du_helper.all_gather([embedd, targets, indexes])
            embedding.append(embedd.detach().cpu())
            vid_info.extend(targets.cpu().tolist())
            idxs.extend(indexes.cpu().tolist())
    return torch.cat(embedding, dim=0), vid_info, idxs


def get_embeddings_and_labels(args, cfg, model, cuda, device, data_loader, split='val', is_master_proc=True,
                              load_pkl=False, save_pkl=False, gather=True):
    """evaluate.py:310-350 (same positional signature; the optional pkl cache uses torch.save/torch.load).
    gather=False: this rank's shard stays on its GPU (see evaluate); the pkl cache then holds per-rank files."""
    out_dir = getattr(cfg, "OUTPUT_PATH", None) if cfg is not None else None
    tag = split if gather else "{}_rank{}".format(split, torch.distributed.get_rank() if torch.distributed.is_initialized() else 0)
    names = [f"{tag}_embeddings.pkl", f"{tag}_labels.pkl", f"{tag}_idxs.pkl"]
    if load_pkl and out_dir and all(os.path.exists(os.path.join(out_dir, n)) for n in names):
        emb, labels, idxs = (torch.load(os.path.join(out_dir, n)) for n in names)
        return (emb if gather else emb.cuda()), labels, idxs
    embeddings, labels, idxs = evaluate(model, data_loader, device=device, is_master_proc=is_master_proc, gather=gather)
    if save_pkl and out_dir and (is_master_proc or not gather):
        for n, v in zip(names, (embeddings.cpu(), labels, idxs)):
            torch.save(v, os.path.join(out_dir, n))
    return embeddings, labels, idxs

"""References and mirror of the k-means helpers of csrc/kmeans.hip (M-step, relocation, finalize / status, the sharded combine,
preprocessing, the k-means++ step helpers): what tests/test_kmeans_kernels_gpu.py expects, and a stand-in for the device.

Two kinds of function:

  ref_*      plain NumPy in float64 — what the operation is.  Used where the header fixes no order (the spherical norm, the
             potentials of Gaussian rows, l2norm of Gaussian rows) and, on grid data, where float64 is exact in any order.
  the rest   the arithmetic the header fixes, bit for bit: the k-ascending fmaf chains (cnorm, dist_to_assigned, kpp_step), the
             ascending-row fp32 sums, the in-place j order of _average_centers and the 4-group shift terms come from the compiled
             oracle (oracle/kmeans.py), which states them in C with -ffp-contract=off; the 256-row double blocks, the rank-order
             fp32 combine, the status word's partition + tree, the counting sort and the searches are written out here.

Every ordered function takes `defects`: a set of names from DEFECTS, each switching ONE deviation on.  `Mirror(*defects)` wraps
the functions behind the interface of test_kmeans_kernels_gpu.Device; tests/test_kmeans_kernels_cpu.py runs every check on
Mirror() (must pass) and on Mirror(defect) (the check named in its table must fail)."""
import numpy as np

from oracle import kmeans as ok

F32 = np.float32
F64 = np.float64
KM_SB = 1024                    # rows per sort block, threads of km_place
TWO20 = 1048576.0

DEFECTS = {
    "far_tie_high": "select_far: a tie goes to the higher row",
    "far_no_mark": "select_far: a taken row is not marked, so it repeats",
    "reloc_reverse": "apply_relocation: entries applied in reverse",
    "reloc_stale": "apply_relocation: the second of two equal old_ids subtracts from the stale row",
    "fin_always_scale": "finalize: the empty-cluster source is always scaled",
    "fin_never_scale": "finalize: the empty-cluster source is never scaled",
    "fin_argmax_last": "finalize: the argmax takes the last maximum",
    "status_empties_precombine": "lloyd_global: the empties of status[1] are counted before the combine (on part 0)",
    "status_2p16": "status[2] rebuilt with 2^16 instead of 2^20",
    "combine_reverse": "combine_shards / lloyd_global: combined in reverse rank order",
    "sum_drop_tail": "sum_f32_to_f64 drops the N % 256 tail",
    "colstats_drop_tail": "col_stats drops the N % 1024 tail",
    "sort_per1": "counting sort: cluster offsets computed as if per == 1",
    "sort_unstable": "counting sort: rows of a cluster reversed",
    "cs_right": "cumsum_search: 'right' instead of 'left'",
    "cs_no_clip": "cumsum_search: no clip to N - 1",
    "perm_k4": "permute_k8: pattern [k0 k1 k2 k3 | k4 k5 k6 k7]",
    "cnorm_pairwise": "cnorm summed pairwise",
    "kpp_no_min": "kpp_step: no min with closest",
    "kpp_pot_fp32": "kpp_step: potential summed in fp32",
    "l2_fp32_acc": "l2norm_rows accumulates in fp32",
    "l2_recip": "l2norm_rows multiplies by the reciprocal instead of dividing",
    "sub_ignores_ldo": "sub_rowvec ignores ldo",
}
NONE = frozenset()


def f32(a):
    return np.ascontiguousarray(a, dtype=F32)


# ------------------------------------------------------------------ float64 references
def ref_cnorm(C):
    return (np.asarray(C, F64) ** 2).sum(1)


def ref_dist_to_assigned(X, C, labels):
    return ((np.asarray(X, F64) - np.asarray(C, F64)[labels]) ** 2).sum(1)


def ref_accumulate(X, labels, K):
    s = np.zeros((K, X.shape[1]), F64)
    np.add.at(s, labels, np.asarray(X, F64))
    return s, np.bincount(labels, minlength=K).astype(F64)


def ref_col_stats(X):
    x = np.asarray(X, F64)
    return x.sum(0), (x * x).sum(0)


def ref_l2norm(X):
    x = np.asarray(X, F64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / np.sqrt((x * x).sum(1, keepdims=True))


def ref_spherical(rows):
    """sklearn.preprocessing.normalize of the (float32) mean rows, in float64; a zero row stays"""
    r = np.asarray(rows, F64)
    n = np.sqrt((r * r).sum(1, keepdims=True))
    return np.where(n > 0, r / np.where(n > 0, n, 1.0), r)


def ref_kpp(X, cand, closest):
    x = np.asarray(X, F64)
    d = np.stack([((x - x[c]) ** 2).sum(1) for c in cand])
    if closest is not None:
        d = np.minimum(d, np.asarray(closest, F64)[None, :])
    return d, d.sum(1)


def ref_cumsum_search(v, vals):
    cs = np.cumsum(np.asarray(v, F64))
    return np.minimum(np.searchsorted(cs, vals, "left"), len(v) - 1).astype(np.int32)


def ref_select_far(dist, n_sel):
    """list-based: the rows that can be taken (a distance that compares greater than -1: never a NaN), sorted by
    (distance descending, row ascending); when they run out, (N, -1)"""
    N = len(dist)
    rows = sorted((-float(d), i) for i, d in enumerate(dist) if d > -1.0)
    idx = [i for _, i in rows[:n_sel]] + [N] * max(0, n_sel - len(rows))
    val = [-d for d, _ in rows[:n_sel]] + [-1.0] * max(0, n_sel - len(rows))
    after = np.array(dist, F32)
    after[[i for i in idx if i < N]] = -2.0
    return np.array(idx, np.int32), np.array(val, F32), after


# ------------------------------------------------------------------ the fixed orders
def cnorm(C, defects=NONE):
    C = f32(C)
    if "cnorm_pairwise" in defects:
        return (C * C).sum(1, dtype=F32)
    return ok.row_sqnorm_chain(C)


def dist_to_assigned(X, C, labels):
    return ok.dist_to_assigned(f32(X), f32(C), labels)


def sum_blocks_256(v, defects=NONE):
    """256 consecutive values added in double in order, then the block sums in order"""
    v = np.asarray(v, F64)
    if "sum_drop_tail" in defects:
        v = v[:len(v) // 256 * 256]
    tot = 0.0
    for b in range(0, len(v), 256):
        a = 0.0
        for x in v[b:b + 256]:
            a += x
        tot += a
    return float(tot)


def col_stats(X, defects=NONE):
    x = np.asarray(X, F64)
    if "colstats_drop_tail" in defects:
        x = x[:len(x) // 1024 * 1024]
    s1, s2 = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    for b in range(0, len(x), 1024):                       # 1024-row segments, rows ascending, segments in order
        p1, p2 = np.zeros(x.shape[1]), np.zeros(x.shape[1])
        for r in x[b:b + 1024]:
            p1 += r
            p2 += r * r
        s1 += p1
        s2 += p2
    return s1, s2


def permute_k8(X, defects=NONE):
    X = f32(X)
    if "perm_k4" in defects:
        return X.copy()
    N, D = X.shape
    return np.ascontiguousarray(X.reshape(N, D // 8, 8)[:, :, [0, 2, 4, 6, 1, 3, 5, 7]].reshape(N, D))


def l2norm_rows(X, defects=NONE):
    X = f32(X)
    if "l2_fp32_acc" in defects:
        s = np.cumsum(X * X, axis=1, dtype=F32)[:, -1:].astype(F64)
    else:
        s = (X.astype(F64) ** 2).sum(1, keepdims=True)
    nrm = np.sqrt(s).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        if "l2_recip" in defects:
            return X * (F32(1.0) / nrm)
        return X / nrm


def sort_order(labels, K, defects=NONE):
    """km_place's `order`: row ids sorted by label, stable"""
    labels = np.asarray(labels)
    N = len(labels)
    if "sort_unstable" in defects:
        return np.lexsort((-np.arange(N), labels)).astype(np.int64)
    order = np.argsort(labels, kind="stable").astype(np.int64)
    if "sort_per1" in defects and K > KM_SB:
        # thread t scans cluster t only: clusters >= 1024 keep their own total where the exclusive scan should stand
        tot = np.bincount(labels, minlength=K)
        off = np.concatenate([[0], np.cumsum(tot)[:-1]])
        bad = off.copy()
        bad[KM_SB:] = tot[KM_SB:]
        out = np.zeros(N, np.int64)
        rank = np.arange(N) - off[labels[order]]
        pos = bad[labels[order]] + rank
        keep = pos < N
        out[pos[keep]] = order[keep]
        return out
    return order


def accumulate(X, labels, K, defects=NONE):
    """fp32 sums per cluster over `order` (ascending rows when the sort is right), counts"""
    X = f32(X)
    cnt = np.bincount(labels, minlength=K)
    order = sort_order(labels, K, defects)
    sums, _ = ok.accumulate(X[order], np.repeat(np.arange(K), cnt).astype(np.int32), K)
    return sums, cnt.astype(F32)


def combine_f32(parts, defects=NONE):
    """parts[W, n] float32 added in rank order from +0"""
    parts = f32(parts)
    a = np.zeros(parts.shape[1], F32)
    for s in (range(len(parts) - 1, -1, -1) if "combine_reverse" in defects else range(len(parts))):
        a = a + parts[s]
    return a


def combine_f64(parts):
    a = np.zeros(parts.shape[1], F64)
    for s in range(len(parts)):
        a = a + np.asarray(parts[s], F64)
    return a.astype(F32)


def select_far(dist, n_sel, defects=NONE):
    dist = np.array(dist, F32)
    N = len(dist)
    idx, val = np.full(n_sel, -7, np.int32), np.full(n_sel, np.nan, F32)
    for e in range(n_sel):
        with np.errstate(invalid="ignore"):
            ok_rows = np.flatnonzero(dist > F32(-1.0))
        if len(ok_rows) == 0:
            idx[e], val[e] = N, -1.0
            continue
        m = dist[ok_rows].max()
        tied = ok_rows[dist[ok_rows] == m]
        i = tied[-1] if "far_tie_high" in defects else tied[0]
        idx[e], val[e] = i, m
        if "far_no_mark" not in defects:
            dist[i] = -2.0
    return idx, val, dist


def apply_relocation(xfar, old_ids, new_ids, sums, counts, defects=NONE):
    sums, counts = np.array(sums, F32), np.array(counts, F32)
    stale = sums.copy()
    seen = set()
    n = len(old_ids)
    for e in (range(n - 1, -1, -1) if "reloc_reverse" in defects else range(n)):
        o, w = int(old_ids[e]), int(new_ids[e])
        base = stale[o] if ("reloc_stale" in defects and o in seen) else sums[o]
        sums[o] = base - xfar[e]
        sums[w] = xfar[e]
        counts[w] = 1.0
        counts[o] -= F32(1.0)
        seen.add(o)
    return sums, counts


def average(sums, counts, defects=NONE):
    """_average_centers in sklearn's in-place j order: the rows before the optional normalisation"""
    sums, counts = f32(sums), f32(counts)
    K = len(counts)
    mx = counts.max()
    src = int(np.flatnonzero(counts == mx)[-1 if "fin_argmax_last" in defects else 0])
    rows = np.empty_like(sums)
    with np.errstate(divide="ignore"):
        alpha = (1.0 / counts.astype(F64)).astype(F32)
    for j in range(K):
        if counts[j] > 0:
            rows[j] = sums[j] * alpha[j]
        else:
            scaled = src < j and counts[src] > 0
            if "fin_always_scale" in defects:
                scaled = counts[src] > 0
            if "fin_never_scale" in defects:
                scaled = False
            rows[j] = sums[src] * (alpha[src] if scaled else F32(1.0))
    return rows


def spherical_rows(rows):
    """the mirror's normalisation: float32 in NumPy's order (the device: 128 strided fmaf chains and a tree; no order is fixed)"""
    rows = f32(rows)
    n = np.sqrt((rows * rows).sum(1, dtype=F32, keepdims=True))
    return np.where(n > 0, rows / np.where(n > 0, n, F32(1)), rows).astype(F32)


def shift_of(C_new, C_old):
    """sqrtf of the 4-group squared distance, groups ascending, then the D % 4 tail (the oracle's _center_shift)"""
    K = len(C_new)
    _, sh, _ = ok.finalize(f32(C_old), f32(C_new), np.ones(K, F32))
    return sh


def status_sum(shift):
    """km_status: thread t adds shift[j]^2 (double) for j = t, t + 256, ..., then a binary tree over the 256 partials"""
    sq = np.asarray(shift, F64) ** 2
    a = np.zeros(256)
    for b in range(0, len(sq), 256):
        c = sq[b:b + 256]
        a[:len(c)] += c
    s = 128
    while s > 0:
        a[:s] += a[s:2 * s]
        s //= 2
    return float(a[0])


def finalize_tail(rows, C_old, counts_for_status, n_changed, spherical, defects=NONE):
    C_new = spherical_rows(rows) if spherical else f32(rows)
    sh = shift_of(C_new, C_old)
    status = np.array([status_sum(sh), float((np.asarray(counts_for_status) == 0).sum()), float(n_changed), 0.0])
    return C_new, sh, ok.row_sqnorm_chain(C_new), permute_k8(C_new) if C_new.shape[1] % 8 == 0 else None, status


def nch_total(pairs, defects=NONE):
    pairs = np.asarray(pairs, F64)
    return float(pairs[:, 0].sum() + (65536.0 if "status_2p16" in defects else TWO20) * pairs[:, 1].sum())


def kpp_step(X, cand, closest, defects=NONE):
    X = f32(X)
    N = len(X)
    z = np.zeros(N, np.int32)
    nd = np.stack([ok.dist_to_assigned(X, X[c:c + 1], z) for c in cand])
    if closest is not None and "kpp_no_min" not in defects:
        nd = np.minimum(nd, f32(closest)[None, :])
    if "kpp_pot_fp32" in defects:
        pot = np.cumsum(nd, axis=1, dtype=F32)[:, -1].astype(F64)
    else:
        pot = nd.astype(F64).sum(1)
    return nd, pot


def cumsum_search(v, vals, defects=NONE):
    cs = np.cumsum(np.asarray(v, F64))
    idx = np.searchsorted(cs, vals, "right" if "cs_right" in defects else "left")
    if "cs_no_clip" not in defects:
        idx = np.minimum(idx, len(v) - 1)
    return idx.astype(np.int32)


# ------------------------------------------------------------------ the mirror behind the device's interface
class Mirror:
    """the functions above behind the methods of test_kmeans_kernels_gpu.Device (buffers with row strides in, arrays out)"""

    def __init__(self, *defects):
        unknown = set(defects) - set(DEFECTS)
        assert not unknown, unknown
        self.d = frozenset(defects)

    def cnorm(self, Cb, D):
        return cnorm(Cb[:, :D], self.d)

    def dist_to_assigned(self, Xb, D, Cb, labels):
        return dist_to_assigned(Xb[:, :D], Cb[:, :D], labels)

    def sum_f32_to_f64(self, v):
        return sum_blocks_256(v, self.d)

    def col_stats(self, Xb, D):
        return col_stats(Xb[:, :D], self.d)

    def sub_rowvec(self, Xb, D, v, ldo):
        N = len(Xb)
        out = np.full((N, ldo), np.nan, F32)
        r = Xb[:, :D] - f32(v)[None, :]
        if "sub_ignores_ldo" in self.d:
            out.reshape(-1)[:N * D] = r.reshape(-1)
        else:
            out[:, :D] = r
        return out

    def l2norm_rows(self, Xb, D, ldo):
        out = np.full((len(Xb), ldo), np.nan, F32)
        out[:, :D] = l2norm_rows(Xb[:, :D], self.d)
        return out

    def permute_k8(self, Xb, D, ldo):
        out = np.full((len(Xb), ldo), np.nan, F32)
        out[:, :D] = permute_k8(Xb[:, :D], self.d)
        return out

    def accumulate(self, Xb, D, labels, K, off=0):
        return accumulate(Xb[:, off:off + D], labels, K, self.d)

    def combine_shards(self, parts, K, D):
        c = combine_f32(parts, self.d)
        return c[:K * D].reshape(K, D), c[K * D:K * D + K]

    def select_far(self, dist, n_sel):
        return select_far(dist, n_sel, self.d)

    def apply_relocation(self, xfar_b, D, old_ids, new_ids, sums, counts):
        return apply_relocation(xfar_b[:, :D], old_ids, new_ids, sums, counts, self.d)

    def finalize(self, C_old, sums, counts, spherical=0, n_changed=None, want_cnorm=True, want_perm=True):
        C_new, sh, cn, cp, st = finalize_tail(average(sums, counts, self.d), C_old, counts,
                                              -1 if n_changed is None else n_changed, spherical, self.d)
        return C_new, cp if want_perm else None, cn if want_cnorm else None, sh, st

    def lloyd_step(self, X, C_old, labels_old, spherical=0):
        K = len(C_old)
        labels = ok.assign(f32(X), f32(C_old))
        nch = 0 if labels_old is None else int((labels != labels_old).sum())
        sums, counts = accumulate(X, labels, K, self.d)
        C_new, sh, cn, cp, st = finalize_tail(average(sums, counts, self.d), C_old, counts, nch, spherical, self.d)
        return labels, nch, sums, counts, C_new, cp, cn, sh, st

    def lloyd_global(self, parts, K, D, C_old, spherical=0):
        KD = K * D
        if parts.dtype == np.float64:
            c = combine_f64(parts[:, :KD + K])
        else:
            c = combine_f32(parts[:, :KD + K], self.d)
        sums, counts = c[:KD].reshape(K, D), c[KD:]
        for_status = f32(parts[0, KD:KD + K]) if "status_empties_precombine" in self.d else counts
        nch = nch_total(parts[:, KD + K:KD + K + 2], self.d)
        C_new, sh, cn, cp, st = finalize_tail(average(sums, counts, self.d), C_old, for_status, nch, spherical, self.d)
        return sums, counts, C_new, cp, cn, sh, st

    def kpp_step(self, Xb, D, cand, closest):
        return kpp_step(Xb[:, :D], cand, closest, self.d)

    def cumsum_search(self, v, vals):
        return cumsum_search(v, vals, self.d)

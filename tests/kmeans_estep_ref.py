"""Mirror of the STRUCTURE of the k-means E-step of csrc/kmeans.hip: what tests/test_kmeans_estep_gpu.py runs in the device's place.

The scores are the compiled oracle's (oracle/kmeans.py: `scores`, the chain and expression of `assign`).  What is written out
here is only what the kernels add on top of them:

  partial lists     every kernel leaves one (score, index) pair per row and LIST of centroids: 128 for km_assign_partial<4> and
                    km_assign_creg, 64 for km_assign_dma<128, 2, 1, 2>.  Inside a list a lane holds, per 32-centroid tile, the 16
                    accumulator slots c = tile + (g & 3) + 8 (g >> 2) + 4 h of its lane half h; it merges its slots ascending
                    with a strict '<', the two lane halves merge with '<' or (== and the lower index), and km_assign_creg's four
                    waves meet in LDS and merge ascending with a strict '<'.
  padding           a centroid >= K scores +inf and never wins; a lane that never saw a score below +inf holds index 0x7fffffff.
  the slice walk    km_assign_creg cuts the ceil(N / 32) sub-tiles evenly over gridDim.x slices (u0, u1), walks a slice as
                    `ntile` tiles of four sub-tiles, the last one of `npt_last`, and writes the rows below `pend`.
  km_combine        list 0, then groups of four lists, then a tail, each with a strict '<'; an index outside [0, K) becomes 0
                    (a row of NaN, or of +inf scores); *n_changed += rows of [0, N) whose label differs from labels_old.
  the histogram     the M-step's per-1024-row-block label histogram, filled by km_combine<true> or by km_block_hist.

Every function takes `defects`: names from DEFECTS, each switching ONE deviation on.  `Mirror(*defects, cus=...)` extends
kmeans_kernels_ref.Mirror with the E-step calls of test_kmeans_kernels_gpu.Device; tests/test_kmeans_estep_cpu.py runs every check
on Mirror() (must pass) and on Mirror(defect) (the check named in its table must fail)."""
import os

import numpy as np

import kmeans_kernels_ref as R
from oracle import kmeans as ok

F32, F64, I32 = np.float32, np.float64, np.int32
NONE = frozenset()
SENTINEL = 0x7fffffff
KM_SB = 1024
KM_SCAN_MAXN = 32768
CREG_MIN_SUBTILES = 6
POISON_SCORE, POISON_IDX = np.nan, -7           # a list entry no workgroup wrote

DEFECTS = {
    "tie_le": "km_combine merges with '<=': a later list wins a tie",
    "lane_tie_le": "a lane merges its accumulator slots with '<='",
    "wave_tie_le": "km_assign_creg's four waves merge with '<='",
    "half_tie_high": "the lane-half merge ignores the index: the upper half wins a tie",
    "pad_zero": "a centroid past K scores 0, not +inf",
    "combine_skip_tail": "km_combine ignores the lists after the last full group of four",
    "combine_from_1": "km_combine ignores list 0",
    "nch_set": "n_changed is overwritten, not added to",
    "nch_past_n": "the rows past N of km_combine's last workgroup count as changed",
    "ld_dense": "the row stride of X is taken as D",
    "slice_drop_partial_tile": "km_assign_creg does not write the rows of a slice's short last tile",
    "nan_sentinel": "an index outside [0, K) is not mapped to 0",
    "hist_drop_last_block": "the ragged last 1024-row block is missing from the histogram",
}


def f32(a):
    return np.ascontiguousarray(a, dtype=F32)


# ------------------------------------------------------------------ the route (km_assign_perm_plan of kmeans.hip)
def plan(N, K, D, ldx, cus):
    """(route, k-tiles, slices, centroid blocks, lists, cus) as slic_kmeans_assign_perm_plan reports them"""
    ncb = -(-K // 128)
    tiles = -(-N // 128)
    slices = min(cus // ncb if ncb <= cus else 0, tiles)
    creg = (D <= 512 and slices >= 1 and ncb * 128 * 7 <= K * 8 and tiles * 4 >= CREG_MIN_SUBTILES * slices
            and (-(-tiles // slices) * 128 + 128) * ldx * 4 < 2 ** 31)
    if creg:
        return (1, 16 if D > 256 else 8 if D > 128 else 4, slices, ncb, ncb, cus)
    return (0, 0, 0, -(-K // 64), -(-K // 64), cus)


def slice_walk(N, slices):
    """km_assign_creg's points per slice: dicts of u0, u1, ntile, npt_last, pbeg, pend, exactly as in the source"""
    subs = (N + 31) // 32
    out = []
    for x in range(slices):
        u0, u1 = subs * x // slices, subs * (x + 1) // slices
        ntile = (u1 - u0 + 3) // 4
        npt_last = (u1 - u0) - 4 * (ntile - 1)
        pbeg = u0 * 32
        prow = min(N - pbeg, (u1 - u0) * 32)
        out.append(dict(u0=u0, u1=u1, ntile=ntile, npt_last=npt_last, pbeg=pbeg, pend=pbeg + prow))
    return out


def slice_rows(N, slices, defects=NONE):
    """the rows each slice writes (one array per slice), tile by tile and sub-tile by sub-tile"""
    out = []
    for s in slice_walk(N, slices):
        rows = []
        for tile in range(s["ntile"]):
            npt = 4 if tile < s["ntile"] - 1 else s["npt_last"]
            if "slice_drop_partial_tile" in defects and npt < 4:
                continue
            op0 = s["pbeg"] + 128 * tile
            for pt in range(npt):
                r = np.arange(op0 + 32 * pt, op0 + 32 * pt + 32)
                rows.append(r[r < s["pend"]])
        out.append(np.concatenate(rows) if rows else np.zeros(0, np.int64))
    return out


def walk_forms(N, slices):
    """the forms of the walk a case exercises: what test_kmeans_estep_gpu's coverage set counts"""
    forms = set()
    for s in slice_walk(N, slices):
        if s["ntile"] > 0:
            forms.add(("npt_last", s["npt_last"]))
            forms.add("one_tile" if s["ntile"] == 1 else "several_tiles")
    forms.add("ragged_subtile" if N % 32 else "whole_subtiles")
    return forms


# ------------------------------------------------------------------ merges
def _lt(s, b):
    with np.errstate(invalid="ignore"):
        return s < b


def _le(s, b):
    with np.errstate(invalid="ignore"):
        return s <= b


def _eq(s, b):
    with np.errstate(invalid="ignore"):
        return s == b


def _take(best, bidx, s, si, how):
    """one merge step of (s, si) into (best, bidx): 'lt' strict, 'le', or 'lt_idx' ('<', or equal and the lower index)"""
    t = _lt(s, best) if how == "lt" else _le(s, best) if how == "le" else (_lt(s, best) | (_eq(s, best) & (si < bidx)))
    return np.where(t, s, best), np.where(t, si, bidx)


def partial_lists(S, K, kind, defects=NONE):
    """S[N, K] -> (pscore[G, N], pidx[G, N]) of one workgroup row: kind 'natural' | 'dma' | 'creg'"""
    N = S.shape[0]
    width = 64 if kind == "dma" else 128
    G = -(-K // width)
    Kp = G * width
    Sp = np.full((N, Kp), 0.0 if "pad_zero" in defects else np.inf, F32)
    Sp[:, :K] = S
    # c = 32 tile + 8 q + 4 h + e  (slot g = 4 q + e)
    Sl = Sp.reshape(N, Kp // 32, 4, 2, 4).transpose(0, 1, 3, 2, 4).reshape(N, Kp // 32, 2, 16)          # [row, tile, h, g]
    cl = np.arange(Kp, dtype=np.int64).reshape(Kp // 32, 4, 2, 4).transpose(0, 2, 1, 3).reshape(Kp // 32, 2, 16)
    lane = "le" if "lane_tie_le" in defects else "lt"
    tpl = width // 32                                  # tiles per list
    if kind == "creg":                                 # a wave per tile: 16 slots, the halves, then the four waves
        best = np.full((N, Kp // 32, 2), np.inf, F32)
        bidx = np.full((N, Kp // 32, 2), SENTINEL, np.int64)
        for g in range(16):
            best, bidx = _take(best, bidx, Sl[..., g], np.broadcast_to(cl[None, :, :, g], best.shape), lane)
        wb, wi = _halves(best, bidx, defects)          # [N, tiles]
        wb, wi = wb.reshape(N, G, tpl), wi.reshape(N, G, tpl)
        lb, li = wb[..., 0], wi[..., 0]
        for w in range(1, tpl):
            lb, li = _take(lb, li, wb[..., w], wi[..., w], "le" if "wave_tie_le" in defects else "lt")
    else:                                              # a lane walks its half of every tile of the list, then the halves
        Sl = Sl.reshape(N, G, tpl, 2, 16)
        cl = cl.reshape(G, tpl, 2, 16)
        best = np.full((N, G, 2), np.inf, F32)
        bidx = np.full((N, G, 2), SENTINEL, np.int64)
        for t in range(tpl):
            for g in range(16):
                best, bidx = _take(best, bidx, Sl[:, :, t, :, g], np.broadcast_to(cl[None, :, t, :, g], best.shape), lane)
        lb, li = _halves(best, bidx, defects)
    return np.ascontiguousarray(lb.T), np.ascontiguousarray(li.T)


def _halves(best, bidx, defects):
    """lane half 0 writes: its own pair against the other half's"""
    b0, i0, b1, i1 = best[..., 0], bidx[..., 0], best[..., 1], bidx[..., 1]
    return _take(b0, i0, b1, i1, "le" if "half_tie_high" in defects else "lt_idx")


def creg_lists(S, K, slices, defects=NONE):
    """km_assign_creg: the lists of the rows the slices write; every other entry keeps its poison"""
    N = S.shape[0]
    lb, li = partial_lists(S, K, "creg", defects)
    ps = np.full(lb.shape, POISON_SCORE, F32)
    pi = np.full(li.shape, POISON_IDX, np.int64)
    for rows in slice_rows(N, slices, defects):
        assert not np.any(pi[:, rows] != POISON_IDX) or "slice_drop_partial_tile" in defects, "two slices wrote one row"
        ps[:, rows], pi[:, rows] = lb[:, rows], li[:, rows]
    return ps, pi


def combine(ps, pi, K, labels_old, nch0, defects=NONE):
    """km_combine: (labels, winning score, n_changed afterwards or None)"""
    G, N = ps.shape
    if "combine_from_1" in defects:
        best, idx = np.full(N, np.inf, F32), np.full(N, SENTINEL, np.int64)
    else:
        best, idx = ps[0].copy(), pi[0].copy()
    how = "le" if "tie_le" in defects else "lt"
    g = 1
    while g + 4 <= G:
        for u in range(4):
            best, idx = _take(best, idx, ps[g + u], pi[g + u], how)
        g += 4
    if "combine_skip_tail" not in defects:
        while g < G:
            best, idx = _take(best, idx, ps[g], pi[g], how)
            g += 1
    if "nan_sentinel" not in defects:
        idx = np.where((idx < 0) | (idx >= K), 0, idx)
    labels = idx.astype(I32)
    nch = int(nch0)                                    # labels_old == NULL: *n_changed is not touched
    if labels_old is not None:
        cnt = int((labels != np.asarray(labels_old, I32)).sum())
        if "nch_past_n" in defects:
            cnt += -(-N // 256) * 256 - N
        nch = cnt if "nch_set" in defects else int(nch0) + cnt
    return labels, best.astype(F32), nch


def block_hist(labels, K, defects=NONE):
    """bc[ceil(N / 1024)][K]"""
    N = len(labels)
    nblk = -(-N // KM_SB)
    bc = np.zeros((nblk, K), np.int64)
    for b in range(nblk):
        if "hist_drop_last_block" in defects and b == nblk - 1 and N % KM_SB:
            continue
        bc[b] = np.bincount(labels[b * KM_SB:(b + 1) * KM_SB], minlength=K)
    return bc


def small_shard(N, D, ldx):
    """the shard sizes the M-step takes without a histogram (SLIC_KM_SCAN=0, read per call, switches that off)"""
    e = os.environ.get("SLIC_KM_SCAN")
    return not (e and e[0] == "0") and N <= KM_SCAN_MAXN and D <= 512 and D % 4 == 0 and N * ldx * 4 < 2 ** 32


def sums_from_hist(X, labels, K, bc, defects=NONE):
    """the counting sort places what the histogram counts: a block missing from it is missing from the sums"""
    N = len(labels)
    keep = np.zeros(N, bool)
    for b in range(len(bc)):
        if bc[b].sum():
            keep[b * KM_SB:(b + 1) * KM_SB] = True
    if not keep.any():
        return np.zeros((K, X.shape[1]), F32), np.zeros(K, F32)
    return R.accumulate(f32(X)[keep], labels[keep], K, defects & set(R.DEFECTS))


# ------------------------------------------------------------------ the mirror behind the device's interface
class Mirror(R.Mirror):
    """kmeans_kernels_ref.Mirror plus the E-step calls of test_kmeans_kernels_gpu.Device; `cus` stands for the device's CU count"""

    def __init__(self, *defects, cus=256):
        unknown = set(defects) - set(DEFECTS) - set(R.DEFECTS)
        assert not unknown, unknown
        self.d = frozenset(defects)
        self.cus = cus

    def _rows(self, Xb, D, off):
        Xb = f32(Xb)
        if "ld_dense" in self.d:
            flat = Xb.reshape(-1)[off:]
            n = len(Xb)
            return np.pad(flat, (0, max(0, n * D - len(flat))), constant_values=np.nan)[:n * D].reshape(n, D)
        return Xb[:, off:off + D]

    def estep_plan(self, N, K, D, ldx):
        return plan(N, K, D, ldx, self.cus)

    def _estep(self, X, C, kind, slices, labels_old, nch0, want_score):
        K = len(C)
        with np.errstate(invalid="ignore", over="ignore"):
            S = ok.scores(X, C)
        if kind == "creg":
            ps, pi = creg_lists(S, K, slices, self.d)
        else:
            ps, pi = partial_lists(S, K, kind, self.d)
        labels, best, nch = combine(ps, pi, K, labels_old, nch0, self.d)
        return labels, nch, best if want_score else None

    def estep_assign(self, Xb, D, Cb, xoff=0, coff=0, labels_old=None, nch0=12345, want_score=True):
        return self._estep(self._rows(Xb, D, xoff), f32(Cb)[:, coff:coff + D], "natural", 0, labels_old, nch0, want_score)

    def estep_assign_perm(self, Xb, D, Cb, xoff=0, coff=0, labels_old=None, nch0=12345, want_score=True, ldxp=None):
        """Xb, Cb in NATURAL column order (the device backend permutes them); ldxp: permuted on the device into rows ldxp apart"""
        p = self.estep_plan(len(Xb), len(Cb), D, ldxp or Xb.shape[1])
        return self._estep(self._rows(Xb, D, xoff), f32(Cb)[:, coff:coff + D], "creg" if p[0] else "dma", p[2], labels_old, nch0,
                           want_score)

    def _perm_labels(self, X, C, labels_old):
        p = self.estep_plan(len(X), len(C), X.shape[1], X.shape[1])
        return self._estep(f32(X), f32(C), "creg" if p[0] else "dma", p[2], labels_old, 0, False)[:2]

    def lloyd_step(self, X, C_old, labels_old, spherical=0):
        K = len(C_old)
        labels, nch = self._perm_labels(X, C_old, labels_old)
        nch = nch or 0
        sums, counts = sums_from_hist(X, labels, K, block_hist(labels, K, self.d), self.d)
        C_new, sh, cn, cp, st = R.finalize_tail(R.average(sums, counts, self.d), C_old, counts, nch, spherical, self.d)
        return labels, nch, sums, counts, C_new, cp, cn, sh, st

    def lloyd_local(self, X, C_old, labels_old, f64=False):
        """labels, sums, counts, the payload's n_changed pair"""
        (N, D), K = X.shape, len(C_old)
        labels, nch = self._perm_labels(X, C_old, labels_old)
        nch = nch or 0
        if small_shard(N, D, D):
            sums, counts = R.accumulate(X, labels, K, self.d & set(R.DEFECTS))
        else:
            sums, counts = sums_from_hist(X, labels, K, block_hist(labels, K, self.d), self.d)
        dt = F64 if f64 else F32
        return labels, sums.astype(dt), counts.astype(dt), np.array([nch & 0xFFFFF, nch >> 20], dt)

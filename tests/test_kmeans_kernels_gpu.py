"""GPU: the k-means helpers of csrc/kmeans.hip called directly through the C ABI at the shapes where their loops change form.

Entry points called by at least one case (COVERED: 16, and their 6 workspace queries; 298 cases):
  slic_kmeans_cnorm, slic_kmeans_permute_k8, slic_kmeans_accumulate, slic_kmeans_combine_shards, slic_kmeans_dist_to_assigned,
  slic_sum_f32_to_f64, slic_kmeans_select_far, slic_kmeans_apply_relocation, slic_kmeans_finalize, slic_kmeans_lloyd_step,
  slic_kmeans_lloyd_global, slic_col_stats, slic_sub_rowvec, slic_l2norm_rows, slic_kmeanspp_step, slic_cumsum_search
  (slic_kmeans_lloyd_local's M-step half is slic_kmeans_accumulate's code; the E-step entry points, whose calls `Device` also
  holds, have their cases in tests/test_kmeans_estep_gpu.py).

The checks are functions of a backend: `Device` calls the library; tests/test_kmeans_kernels_cpu.py runs the same functions with
the NumPy mirror (tests/kmeans_kernels_ref.py) in the device's place, unmutated and with one defect at a time.  Importing this
module does not touch the device.

Hygiene: every output starts as NaN (-7 for int32) in front of a 4096-byte guard tail that must come back unchanged, workspaces
have the size the library's own *_workspace_bytes gives plus such a tail, padding columns of strided inputs hold NaN, and every call
runs twice into fresh outputs that must be bit-equal.

Gates.  Integers, indices, counts and everything whose order the header fixes: bit-equal to the compiled oracle (oracle/kmeans.py)
or to the order written out in kmeans_kernels_ref.py.  Data on grids (stated beside each case) makes float64 exact in any order, so
those are bit-equal too; tests/test_kmeans_kernels_cpu.py re-adds every such sum in two orders.  The three reductions whose order
the header does not fix are gated as |got - float64| <= coef * 2^-24 * scale with coef derived beside the gate; the worst error /
gate ratio of each is kept in RATIOS and printed before it is asserted.  On an MI355X: lloyd_step.spherical 0.29,
finalize.spherical 0.25, kpp_step.pot.gauss 0.0014, l2norm_rows.gauss 0.57 (its gate is two roundings and one to spare and has no
reduction to be generous about: a correct result reaches 2 / 3 of it).

`shift` turned out bit-equal to the oracle's 4-group order (kmeans.hip is compiled with -ffp-contract=off, so the device's
d0*d0 + d1*d1 + d2*d2 + d3*d3 rounds like the C expression): that is the gate."""
import ctypes

import numpy as np
import pytest

import kmeans_kernels_ref as R
from oracle import kmeans as ok

pytestmark = pytest.mark.gpu
F32, F64, I32 = np.float32, np.float64, np.int32
GUARD = 4096
U = 2.0 ** -24
RATIOS = {}
CASES = {}

COVERED = [
    "slic_kmeans_cnorm", "slic_kmeans_permute_k8", "slic_kmeans_accumulate_workspace_bytes", "slic_kmeans_accumulate",
    "slic_kmeans_combine_shards", "slic_kmeans_dist_to_assigned", "slic_sum_f32_to_f64_workspace_bytes", "slic_sum_f32_to_f64",
    "slic_kmeans_select_far", "slic_kmeans_apply_relocation", "slic_kmeans_finalize", "slic_kmeans_lloyd_step_workspace_bytes",
    "slic_kmeans_lloyd_step", "slic_kmeans_lloyd_global", "slic_col_stats_workspace_bytes", "slic_col_stats", "slic_sub_rowvec",
    "slic_l2norm_rows", "slic_kmeanspp_step_workspace_bytes", "slic_kmeanspp_step", "slic_cumsum_search_workspace_bytes",
    "slic_cumsum_search",
]


def f32(a):
    return np.ascontiguousarray(a, dtype=F32)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def case(name):
    CASES[name] = CASES.get(name, 0) + 1


def exact(name, got, exp, what=""):
    """bit-equal (a NaN must be the same NaN; -0 is not +0)"""
    got = np.ascontiguousarray(got)
    exp = np.ascontiguousarray(exp, dtype=got.dtype)
    if not bits_equal(got, exp):
        u = f"u{got.dtype.itemsize}"
        bad = np.flatnonzero(got.reshape(-1).view(u) != exp.reshape(-1).view(u)) if got.shape == exp.shape else []
        first = [(int(i), got.reshape(-1)[i], exp.reshape(-1)[i]) for i in bad[:4]]
        raise AssertionError((name, what, got.shape, exp.shape, f"{len(bad)} of {got.size} differ", first))


def gate(name, got, ref, scale, coef, what=""):
    """finite, and |got - ref| <= coef 2^-24 scale elementwise; the worst ratio is printed before it is asserted"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (name, what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), (name, what, "not finite")
    tol = coef * U * np.broadcast_to(np.asarray(scale, F64), ref.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / tol)
    worst = float(r.max()) if r.size else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), worst)
    print(f"gate {name} {what}: worst error / gate = {worst:.4f} (coef {coef:g}, max error {float(err.max()) if err.size else 0:.3e})")
    assert worst <= 1.0, (name, what, worst)


def twice(fn):
    """two runs into fresh outputs, bit-equal"""
    a, b = fn(), fn()
    a2, b2 = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    for u, v in zip(a2, b2):
        assert (u is None and v is None) or bits_equal(np.asarray(u), np.asarray(v)), "two runs differ"
    return a


def pad(X, ld, off=0):
    """X in columns [off, off + D) of a NaN buffer with row stride ld"""
    X = f32(X)
    b = np.full((X.shape[0], ld), np.nan, F32)
    b[:, off:off + X.shape[1]] = X
    return b


def grid(rng, shape, step, lim):
    """multiples of `step` in [-lim, lim]"""
    n = int(round(lim / step))
    return (rng.integers(-n, n + 1, shape) * step).astype(F32)


# ------------------------------------------------------------------ the device backend
class Device:
    def __init__(self, lib):
        import torch
        from video_similarity_search_amd import _lib
        self.t, self.lib, self._lib = torch, lib, _lib
        self.pattern = (torch.arange(GUARD) % 251).to(torch.uint8).cuda()
        self._guards = []
        self.tdt = {np.dtype(F32): torch.float32, np.dtype(F64): torch.float64, np.dtype(I32): torch.int32}

    def up(self, a, dtype=F32):
        return None if a is None else self.t.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()       # a copy: inputs may be read-only

    def out(self, shape, dtype=F32, data=None):
        """NaN / -7 (or `data`) in front of a guard tail"""
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        buf = self.t.empty(n + GUARD, dtype=self.t.uint8, device="cuda")
        buf[n:] = self.pattern
        v = buf[:n].view(self.tdt[np.dtype(dtype)]).view(shape)
        if data is not None:
            v.copy_(self.t.from_numpy(np.ascontiguousarray(data, dtype=dtype)).view(shape))
        else:
            v.fill_(-7 if dtype == I32 else float("nan"))
        self._guards.append((buf, n))
        return v

    def ws(self, nbytes):
        buf = self.t.empty(int(nbytes) + GUARD, dtype=self.t.uint8, device="cuda")
        buf[:int(nbytes)] = 0xA5
        buf[int(nbytes):] = self.pattern
        self._guards.append((buf, int(nbytes)))
        return buf

    def run(self, name, *args):
        p = self._lib.ptr
        self._lib.call(name, *[p(a) if isinstance(a, self.t.Tensor) or a is None else a for a in args], self._lib.stream())
        self.t.cuda.synchronize()
        for buf, n in self._guards:
            assert self.t.equal(buf[n:], self.pattern), f"{name} wrote past a buffer of {n} bytes"
        self._guards = []

    @staticmethod
    def np(*ts):
        return tuple(None if t is None else t.cpu().numpy() for t in ts)

    @staticmethod
    def at(t, off_elems):
        return ctypes.c_void_p(t.data_ptr() + 4 * off_elems)

    # -- rowwise
    def cnorm(self, Cb, D):
        o = self.out((len(Cb),))
        self.run("slic_kmeans_cnorm", self.up(Cb), len(Cb), D, Cb.shape[1], o)
        return o.cpu().numpy()

    def dist_to_assigned(self, Xb, D, Cb, labels):
        o = self.out((len(Xb),))
        self.run("slic_kmeans_dist_to_assigned", self.up(Xb), len(Xb), D, Xb.shape[1], self.up(Cb), Cb.shape[1],
                 self.up(labels, I32), o)
        return o.cpu().numpy()

    def sum_f32_to_f64(self, v):
        w = self.ws(self.lib.slic_sum_f32_to_f64_workspace_bytes(len(v)))
        o = self.out((1,), F64)
        self.run("slic_sum_f32_to_f64", self.up(v), len(v), o, w)
        return float(o.cpu().numpy()[0])

    def col_stats(self, Xb, D):
        w = self.ws(self.lib.slic_col_stats_workspace_bytes(len(Xb), D))
        s, q = self.out((D,), F64), self.out((D,), F64)
        self.run("slic_col_stats", self.up(Xb), len(Xb), D, Xb.shape[1], s, q, w)
        return self.np(s, q)

    def sub_rowvec(self, Xb, D, v, ldo):
        o = self.out((len(Xb), ldo))
        self.run("slic_sub_rowvec", self.up(Xb), len(Xb), D, Xb.shape[1], self.up(v), o, ldo)
        return o.cpu().numpy()

    def l2norm_rows(self, Xb, D, ldo):
        o = self.out((len(Xb), ldo))
        self.run("slic_l2norm_rows", self.up(Xb), len(Xb), D, Xb.shape[1], o, ldo)
        return o.cpu().numpy()

    def permute_k8(self, Xb, D, ldo):
        o = self.out((len(Xb), ldo))
        self.run("slic_kmeans_permute_k8", self.up(Xb), len(Xb), D, Xb.shape[1], o, ldo)
        return o.cpu().numpy()

    # -- M-step
    def accumulate(self, Xb, D, labels, K, off=0):
        N = len(Xb)
        w = self.ws(self.lib.slic_kmeans_accumulate_workspace_bytes(N, K))
        sums, counts = self.out((K, D)), self.out((K,))
        x = self.up(Xb)
        self.run("slic_kmeans_accumulate", self.at(x, off), N, D, Xb.shape[1], self.up(labels, I32), K, sums, counts, w)
        return self.np(sums, counts)

    def combine_shards(self, parts, K, D):
        W, stride = parts.shape
        p = self.up(parts)
        sums, counts = self.out((K, D)), self.out((K,))
        self.run("slic_kmeans_combine_shards", p, self.at(p, K * D), stride, W, K, D, sums, counts)
        return self.np(sums, counts)

    def select_far(self, dist, n_sel):
        d = self.out((len(dist),), data=dist)
        idx, val = self.out((n_sel,), I32), self.out((n_sel,))
        self.run("slic_kmeans_select_far", d, len(dist), n_sel, idx, val)
        return self.np(idx, val, d)

    def apply_relocation(self, xfar_b, D, old_ids, new_ids, sums, counts):
        s, c = self.out(sums.shape, data=sums), self.out(counts.shape, data=counts)
        self.run("slic_kmeans_apply_relocation", self.up(xfar_b), xfar_b.shape[1], self.up(old_ids, I32), self.up(new_ids, I32),
                 len(old_ids), D, s, c)
        return self.np(s, c)

    def finalize(self, C_old, sums, counts, spherical=0, n_changed=None, want_cnorm=True, want_perm=True):
        K, D = C_old.shape
        C_new, sh, st = self.out((K, D)), self.out((K,)), self.out((4,), F64)
        cn = self.out((K,)) if want_cnorm else None
        cp = self.out((K, D)) if want_perm else None
        nch = None if n_changed is None else self.up([n_changed], I32)
        self.run("slic_kmeans_finalize", self.up(C_old), self.up(sums), self.up(counts), K, D, C_new, sh, cn, cp, spherical, nch, st)
        return self.np(C_new, cp, cn, sh, st)

    def lloyd_step(self, X, C_old, labels_old, spherical=0):
        (N, D), K = X.shape, len(C_old)
        w = self.ws(self.lib.slic_kmeans_lloyd_step_workspace_bytes(N, K))
        labels, nch = self.out((N,), I32), self.out((1,), I32)
        sums, counts, C_new, Cp_new = self.out((K, D)), self.out((K,)), self.out((K, D)), self.out((K, D))
        cn, sh, st = self.out((K,)), self.out((K,)), self.out((4,), F64)
        self.run("slic_kmeans_lloyd_step", self.up(X), self.up(R.permute_k8(X)), N, D, D, self.up(C_old),
                 self.up(R.permute_k8(C_old)), self.up(R.cnorm(C_old)), K, labels, self.up(labels_old, I32), nch, sums, counts,
                 C_new, Cp_new, cn, sh, spherical, st, w)
        labels, nch, sums, counts, C_new, Cp_new, cn, sh, st = self.np(labels, nch, sums, counts, C_new, Cp_new, cn, sh, st)
        return labels, int(nch[0]), sums, counts, C_new, Cp_new, cn, sh, st

    def lloyd_global(self, parts, K, D, C_old, spherical=0):
        W, stride = parts.shape
        is64 = parts.dtype == np.float64
        sums, counts, C_new, Cp_new = self.out((K, D)), self.out((K,)), self.out((K, D)), self.out((K, D))
        cn, sh, st = self.out((K,)), self.out((K,)), self.out((4,), F64)
        self.run("slic_kmeans_lloyd_global", self.up(parts, F64 if is64 else F32), int(is64), stride, W, self.up(C_old), K, D, sums,
                 counts, C_new, Cp_new, cn, sh, spherical, st)
        return self.np(sums, counts, C_new, Cp_new, cn, sh, st)

    # -- E-step (the cases live in tests/test_kmeans_estep_gpu.py)
    def estep_plan(self, N, K, D, ldx):
        out = (ctypes.c_int * 6)()
        assert self.lib.slic_kmeans_assign_perm_plan(N, K, D, ldx, out) == 0, self.lib.slic_last_error()
        return tuple(out)

    def _estep(self, name, x, N, D, ldx, c, K, ldc, cn, labels_old, nch0, want_score):
        w = self.ws(self.lib.slic_kmeans_assign_workspace_bytes(N, K))
        labels, nch = self.out((N,), I32), self.out((1,), I32, data=[nch0])
        score = self.out((N,)) if want_score else None
        self.run(name, x, N, D, ldx, c, K, ldc, self.up(cn), labels, self.up(labels_old, I32), nch, score, w)
        labels, nch, score = self.np(labels, nch, score)
        return labels, int(nch[0]), score

    def estep_assign(self, Xb, D, Cb, xoff=0, coff=0, labels_old=None, nch0=12345, want_score=True):
        """slic_kmeans_assign on the columns [xoff, xoff + D) of Xb and [coff, coff + D) of Cb"""
        x, c = self.up(Xb), self.up(Cb)
        return self._estep("slic_kmeans_assign", self.at(x, xoff), len(Xb), D, Xb.shape[1], self.at(c, coff), len(Cb), Cb.shape[1],
                           R.cnorm(Cb[:, coff:coff + D]), labels_old, nch0, want_score)

    def estep_assign_perm(self, Xb, D, Cb, xoff=0, coff=0, labels_old=None, nch0=12345, want_score=True, ldxp=None):
        """slic_kmeans_assign_perm; Xb, Cb arrive in natural column order and are permuted here: on the host inside their
        buffers, or (ldxp) X by slic_kmeans_permute_k8 into rows ldxp >= D + 4 apart that start 4 floats into a NaN buffer"""
        Cp = np.array(Cb, F32)
        Cp[:, coff:coff + D] = R.permute_k8(Cb[:, coff:coff + D])
        c = self.up(Cp)
        N = len(Xb)
        if ldxp is None:
            Xp = np.array(Xb, F32)
            Xp[:, xoff:xoff + D] = R.permute_k8(Xb[:, xoff:xoff + D])
            keep = self.up(Xp)
            xp, ldx = self.at(keep, xoff), Xb.shape[1]
        else:
            assert ldxp >= D + 4
            src, keep = self.up(Xb), self.out((N, ldxp))
            self.run("slic_kmeans_permute_k8", self.at(src, xoff), N, D, Xb.shape[1], self.at(keep, 4), ldxp)
            xp, ldx = self.at(keep, 4), ldxp
        return self._estep("slic_kmeans_assign_perm", xp, N, D, ldx, self.at(c, coff), len(Cb), Cb.shape[1],
                           R.cnorm(Cb[:, coff:coff + D]), labels_old, nch0, want_score)

    def lloyd_local(self, X, C_old, labels_old, f64=False):
        """labels, sums, counts and the n_changed pair of the payload"""
        (N, D), K = X.shape, len(C_old)
        w = self.ws(self.lib.slic_kmeans_lloyd_local_workspace_bytes(N, K))
        labels, pay = self.out((N,), I32), self.out((K * D + K + 2,), F64 if f64 else F32)
        self.run("slic_kmeans_lloyd_local", self.up(X), self.up(R.permute_k8(X)), N, D, D, self.up(R.permute_k8(C_old)),
                 self.up(R.cnorm(C_old)), K, labels, self.up(labels_old, I32), pay, int(f64), w)
        labels, pay = self.np(labels, pay)
        return labels, pay[:K * D].reshape(K, D), pay[K * D:K * D + K], pay[K * D + K:]

    # -- k-means++ helpers
    def kpp_step(self, Xb, D, cand, closest):
        N, T = len(Xb), len(cand)
        w = self.ws(self.lib.slic_kmeanspp_step_workspace_bytes(N, T))
        nd, pot = self.out((T, N)), self.out((T,), F64)
        self.run("slic_kmeanspp_step", self.up(Xb), N, D, Xb.shape[1], self.up(cand, I32), T, self.up(closest), nd, pot, w)
        return self.np(nd, pot)

    def cumsum_search(self, v, vals):
        w = self.ws(self.lib.slic_cumsum_search_workspace_bytes(len(v)))
        idx = self.out((len(vals),), I32)
        self.run("slic_cumsum_search", self.up(v), len(v), self.up(vals, F64), len(vals), idx, w)
        return idx.cpu().numpy()


# ------------------------------------------------------------------ slic_kmeans_accumulate
SORT_KS = (1024, 1025, 1365, 1366, 2100, 4099)       # per 1 | per 2 | last K with per-wave counts in LDS | first without | per 3 | per 5
SORT_LABELS = ("uniform", "one", "top40", "waves")
WIDE_DS = (516, 520, 1024, 2048)                     # gridDim.y = 2 (partly / barely inside D), 2 (full), 4


def sort_labels(kind, N, K, rng):
    if kind == "uniform":
        return rng.integers(0, K, N).astype(I32)
    if kind == "one":
        return np.full(N, K - 1, I32)
    if kind == "top40":                               # the first K - 40 clusters are empty
        return rng.integers(K - 40, K, N).astype(I32)
    # every wave of 64 rows holds the same 64 labels: each row shares its label with a row of every earlier wave
    return ((np.arange(N) % 64) * (K // 64) + K % 64).astype(I32)


def check_accumulate(be, env, N, D, K, kind, scan="0", ldx=None, off=0, seed=0):
    """counts == bincount, sums bit-equal to the ascending-row fp32 sums of the oracle"""
    case("accumulate")
    if scan is None:
        env.delenv("SLIC_KM_SCAN", raising=False)
    else:
        env.setenv("SLIC_KM_SCAN", scan)
    rng = np.random.default_rng(seed + K + D)
    X = f32(rng.standard_normal((N, D)))
    labels = sort_labels(kind, N, K, rng)
    assert labels.min() >= 0 and labels.max() < K
    Xb = pad(X, ldx or D, off)
    sums, counts = twice(lambda: be.accumulate(Xb, D, labels, K, off))
    es, _ = ok.accumulate(X, labels, K)
    exact("accumulate.counts", counts, np.bincount(labels, minlength=K).astype(F32), (N, D, K, kind, scan))
    exact("accumulate.sums", sums, es, (N, D, K, kind, scan))


# ------------------------------------------------------------------ slic_kmeans_lloyd_step
STEP_ROUTES = {"fused": (600, 16, 5), "unfused": (700, 1024, 9)}      # D <= 512: km_accumulate_average; above: km_accumulate + finalize
STEP_EMPTY = ("none", "before", "after")


def spherical_coef(D):
    """C_new = row / sqrtf(sum of row^2), the sum as 128 strided fmaf chains (ceil(D / 128) roundings) and a 7-level tree: its
    relative error is at most (ceil(D / 128) + 7) 2^-24 (all terms positive); the square root halves that and rounds once, the
    division rounds once; one to spare.  In units of 2^-24 |C_new|."""
    return (-(-D // 128) + 7) / 2 + 2 + 1


def step_problem(route, empty):
    N, D, K = STEP_ROUTES[route]
    rng = np.random.default_rng(11 + N)
    X = f32(rng.standard_normal((N, D)))
    C = X[rng.choice(N, K, replace=False)].copy()
    big = int(np.argmax(np.bincount(ok.assign(X, C), minlength=K)))
    C[[big, K // 2]] = C[[K // 2, big]]                 # the biggest cluster sits in the middle
    e = {"none": None, "before": 0, "after": K - 1}[empty]
    if e is not None:
        C[e] = 100.0                                    # a centre far from every row: its cluster is empty
    labels = ok.assign(X, C)
    cnt = np.bincount(labels, minlength=K)
    big = int(np.argmax(cnt))
    if e is None:
        assert cnt.min() > 0
    else:
        assert cnt[e] == 0 and (cnt == 0).sum() == 1 and ((e < big) if empty == "before" else (e > big)), (cnt, e, big)
    labels_old = np.where(rng.random(N) < 0.3, rng.integers(0, K, N), labels).astype(I32)
    return X, C, labels_old


def check_step_outputs(name, got, X, C_old, labels_old, spherical, what):
    """everything slic_kmeans_lloyd_step / _finalize / _lloyd_global writes after the sums, against the oracle"""
    labels, nch, sums, counts, C_new, Cp_new, cn, sh, st = got
    K, D = C_old.shape
    e_new, e_sh, e_tot = ok.finalize(C_old, sums, counts)
    if spherical:
        rows = R.average(sums, counts)
        exact(name + ".rows_vs_oracle", rows, e_new, what)
        ref = R.ref_spherical(rows)
        gate(name + ".spherical", C_new, ref, np.abs(ref), spherical_coef(D), what)
        e_new, e_sh = C_new, R.shift_of(C_new, C_old)   # downstream of the normalised rows: exact functions of them
    exact(name + ".C_new", C_new, e_new, what)
    exact(name + ".shift", sh, e_sh, what)
    if cn is not None:
        exact(name + ".cnorm_new", cn, ok.row_sqnorm_chain(e_new), what)
    if Cp_new is not None:
        exact(name + ".Cp_new", Cp_new, R.permute_k8(e_new), what)
    e_st = np.array([R.status_sum(e_sh), float((counts == 0).sum()), float(nch), 0.0])
    exact(name + ".status", st, e_st, what)
    if not spherical:                                   # the tree's double sum against the oracle's sequential one
        assert abs(st[0] - e_tot) <= K * 2.0 ** -52 * e_tot, (name, what, st[0], e_tot)


def check_lloyd_step(be, route, empty, spherical=0):
    case("lloyd_step")
    X, C_old, labels_old = step_problem(route, empty)
    K = len(C_old)
    for lo in (labels_old, None):
        what = (route, empty, spherical, "labels_old" if lo is not None else "NULL")
        got = twice(lambda: be.lloyd_step(X, C_old, lo, spherical))
        labels, nch, sums, counts = got[:4]
        e_lab = ok.assign(X, C_old)
        exact("lloyd_step.labels", labels, e_lab, what)
        assert nch == (0 if lo is None else int((e_lab != lo).sum())), (what, nch)
        es, ec = ok.accumulate(X, e_lab, K)
        exact("lloyd_step.sums", sums, es, what)
        exact("lloyd_step.counts", counts, ec, what)
        check_step_outputs("lloyd_step", got, X, C_old, lo, spherical, what)


# ------------------------------------------------------------------ slic_kmeans_finalize
FIN_DS = (4, 6, 8, 516)
FIN_COUNTS = {
    "zeros_0_mid_last": [0, 3, 5, 0, 5, 2, 0],          # two equal maxima: cluster 2 is the source; 0 precedes it, 3 and 6 follow
    "all_zero": [0, 0, 0, 0, 0, 0, 0],                  # source = cluster 0 as it stands (alpha = 1): every row is sums[0]
    "none_empty": [4, 1, 9, 2, 2, 7, 3],
}


def check_finalize(be, D, which, spherical=0):
    case("finalize")
    rng = np.random.default_rng(5 + D)
    counts = f32(FIN_COUNTS[which])
    K = len(counts)
    sums = f32(rng.standard_normal((K, D)) * np.maximum(counts, 1)[:, None])
    C_old = f32(rng.standard_normal((K, D)))
    for n_changed, want in ((None, True), (12345, False)):
        what = (D, which, spherical, n_changed, want)
        got = twice(lambda: be.finalize(C_old, sums, counts, spherical, n_changed, want, want and D % 8 == 0))
        assert (got[2] is None) == (not want) and (got[1] is None) == (not (want and D % 8 == 0))
        full = (None, -1 if n_changed is None else n_changed, sums, counts) + tuple(got)
        check_step_outputs("finalize", full, None, C_old, None, spherical, what)
        if which == "all_zero" and not spherical:
            exact("finalize.all_zero", got[0], np.tile(sums[0], (K, 1)), what)


def check_finalize_k300(be):
    """km_status loops (K > 256); a tenth of the clusters empty"""
    case("finalize")
    rng = np.random.default_rng(6)
    K, D = 300, 8
    counts = f32(rng.integers(0, 10, K))
    counts[[0, 150, 299]] = 0
    sums = f32(rng.standard_normal((K, D)) * np.maximum(counts, 1)[:, None])
    C_old = f32(rng.standard_normal((K, D)))
    got = twice(lambda: be.finalize(C_old, sums, counts, 0, 77))
    check_step_outputs("finalize", (None, 77, sums, counts) + tuple(got), None, C_old, None, 0, "K300")


# ------------------------------------------------------------------ slic_kmeans_lloyd_global / slic_kmeans_combine_shards
GLOBAL_FORMS = ((1, F32), (3, F32), (16, F32), (1, F64), (3, F64))


def global_parts(W, dtype):
    """W payloads [K*D sums | K counts | n_changed low 20 bits | n_changed >> 20 | 5 unused (NaN)] of mixed magnitude.
    Combined counts: cluster 2 is empty although part 0 holds +1 and part 1 holds -1 (W >= 3); cluster 1 leads in part 0 alone
    (500 there, -495 in part 1); the biggest combined count is cluster 3's; cluster 5 is empty in every part.  So the empty cluster
    2 precedes its source and copies the raw sum, 5 follows it and copies the mean."""
    K, D = 6, 8
    KD = K * D
    rng = np.random.default_rng(100 + W)
    parts = np.full((W, KD + K + 2 + 5), np.nan, F64)
    parts[:, :KD] = f32(rng.standard_normal((W, KD)) * 10.0 ** rng.integers(-3, 4, (W, KD)))
    cnt = np.zeros((W, K))
    cnt[:, 0] = rng.integers(0, 3, W)
    cnt[:, 3] = rng.integers(2, 5, W)
    cnt[:, 4] = rng.integers(0, 2, W)
    cnt[0, 0] = 1
    if W >= 3:
        cnt[0, 2], cnt[1, 2] = 1, -1
        cnt[0, 1], cnt[1, 1] = 500, -495
    else:
        cnt[0, 1] = 2
    parts[:, KD:KD + K] = cnt
    parts[:, KD + K:KD + K + 2] = rng.integers(0, 4, (W, 2))
    parts[0, KD + K:KD + K + 2] = (1048575, 3)
    if W > 1:
        parts[1, KD + K:KD + K + 2] = (5, 0)
    return K, D, parts.astype(dtype)


def check_global(be, W, dtype):
    case("lloyd_global")
    K, D, parts = global_parts(W, dtype)
    KD = K * D
    C_old = f32(np.random.default_rng(3).standard_normal((K, D)))
    what = (W, np.dtype(dtype).name)
    if dtype == F32:
        comb = R.combine_f32(parts[:, :KD + K])
        if W >= 3:                                      # the rank order is visible in the last bit
            assert not bits_equal(comb, R.combine_f32(parts[::-1, :KD + K]))
    else:
        comb = R.combine_f64(parts[:, :KD + K])
    e_sums, e_counts = comb[:KD].reshape(K, D), comb[KD:]
    if W >= 3:
        assert e_counts[2] == 0 and e_counts[5] == 0 and int(np.argmax(e_counts)) == 3 and parts[0, KD + 1] > e_counts[3]
    nch = R.nch_total(parts[:, KD + K:KD + K + 2])
    assert nch >= 2 ** 20
    sums, counts, C_new, Cp_new, cn, sh, st = twice(lambda: be.lloyd_global(parts, K, D, C_old))
    exact("lloyd_global.out_sums", sums, e_sums, what)
    exact("lloyd_global.out_counts", counts, e_counts, what)
    check_step_outputs("lloyd_global", (None, nch, e_sums, e_counts, C_new, Cp_new, cn, sh, st), None, C_old, None, 0, what)
    if dtype == F32:
        case("combine_shards")
        s2, c2 = twice(lambda: be.combine_shards(parts, K, D))
        exact("combine_shards.sums", s2, e_sums, what)
        exact("combine_shards.counts", c2, e_counts, what)


# ------------------------------------------------------------------ slic_kmeans_select_far
FAR_NS = (1, 1023, 1024, 1025, 5000)
FAR_SELS = (1, 3, 17)
FAR_KINDS = ("grid", "zeros", "nan")


def far_dist(N, kind, rng):
    if kind == "zeros":
        return np.zeros(N, F32)
    d = (rng.integers(0, 8, N) / 16.0).astype(F32)      # a 1/16 grid: most rows tie
    top = np.array([5, 6, 5 + 1024, 2000, 2001, 2000 + 1024])     # the maximum at rows i, i + 1 (two threads) and i + 1024 (one thread)
    d[top[top < N][:3]] = 1.0
    d[top[top < N][3:]] = 0.75
    if kind == "nan":
        d[np.array([0, 5, 700, 1024, N - 1])[np.array([0, 5, 700, 1024, N - 1]) < N]] = np.nan      # never taken
    return d


def check_select_far(be, N, n_sel, kind):
    case("select_far")
    dist = far_dist(N, kind, np.random.default_rng(N))
    idx, val, after = twice(lambda: be.select_far(dist, n_sel))
    e_idx, e_val, e_after = R.ref_select_far(dist, n_sel)
    what = (N, n_sel, kind)
    exact("select_far.far_idx", idx, e_idx, what)
    exact("select_far.far_dist", val, e_val, what)
    exact("select_far.dist_after", after, e_after, what)


# ------------------------------------------------------------------ slic_kmeans_apply_relocation
RELOC_CASES = ((1, 4), (1, 260), (4, 4), (4, 260))


def check_apply_relocation(be, n, D):
    """n = 4: old id 2 twice in a row, new id 1 of entry 0 is entry 3's old id; xfar rows ldf = D + 4 apart"""
    case("apply_relocation")
    rng = np.random.default_rng(n + D)
    K = 6
    old_ids, new_ids = ([2, 2, 5, 1], [1, 3, 4, 0]) if n == 4 else ([2], [0])
    sums = f32(rng.standard_normal((K, D)) * 8)
    counts = f32([0, 0, 9, 0, 0, 4])
    xfar = f32(rng.standard_normal((n, D)))
    s, c = twice(lambda: be.apply_relocation(pad(xfar, D + 4), D, np.array(old_ids, I32), np.array(new_ids, I32), sums, counts))
    es, ec = R.apply_relocation(xfar, old_ids, new_ids, sums, counts)
    exact("apply_relocation.sums", s, es, (n, D))
    exact("apply_relocation.counts", c, ec, (n, D))


# ------------------------------------------------------------------ the rowwise helpers
ROW_NS = (1, 63, 64, 65, 257, 1025, 2049)
ROW_DS = (4, 8, 12, 16, 20, 516)
COL_NS = (1, 1023, 1024, 1025, 3001)
COL_DS = (5, 64, 67)


def check_rowwise(be, N, D):
    """cnorm, dist_to_assigned, sub_rowvec, permute_k8, l2norm_rows (also at the odd D + 1) and sum_f32_to_f64 at one (N, D);
    N is the number of rows, of centres for cnorm, of values for the sum"""
    case("rowwise")
    rng = np.random.default_rng(1000 * N + D)
    what = (N, D)
    X = f32(rng.standard_normal((N, D)))
    exact("cnorm", twice(lambda: be.cnorm(pad(X, D + 4), D)), ok.row_sqnorm_chain(X), what)
    C = f32(rng.standard_normal((5, D)))
    labels = rng.integers(0, 5, N).astype(I32)
    exact("dist_to_assigned", twice(lambda: be.dist_to_assigned(pad(X, D + 8), D, pad(C, D + 4), labels)),
          ok.dist_to_assigned(X, C, labels), what)
    v = f32(rng.standard_normal(D))
    exact("sub_rowvec", twice(lambda: be.sub_rowvec(pad(X, D + 4), D, v, D + 8)), pad(X - v[None, :], D + 8), what)
    if D % 8 == 0:
        exact("permute_k8", twice(lambda: be.permute_k8(pad(X, D + 4), D, D + 8)), pad(R.permute_k8(X), D + 8), what)
    for Dl in (D, D + 1):
        # a 2^-4 grid with |v| <= 2: v^2 is a multiple of 2^-8 below 4, a row's sum needs 10 + 2 + 8 bits: exact in double, so
        # float32(x / float32(sqrt(sum))) is the only correct answer.  Row 1 is all zero: 0 / 0, a NaN row (as x / x.norm() in torch)
        G = grid(rng, (N, Dl), 2.0 ** -4, 2.0)
        if N > 1:
            G[1] = 0
        with np.errstate(invalid="ignore", divide="ignore"):
            e = G / np.sqrt((G.astype(F64) ** 2).sum(1, keepdims=True)).astype(F32)
        if N > 1:
            assert np.isnan(e[1]).all()
        got = twice(lambda: be.l2norm_rows(pad(G, Dl + 3), Dl, Dl + 5))
        assert np.array_equal(np.isnan(got[:, :Dl]), np.isnan(e)), ("l2norm_rows NaN pattern", what)
        exact("l2norm_rows", np.nan_to_num(got[:, :Dl], nan=7.0), np.nan_to_num(e, nan=7.0), (N, Dl))
        assert np.isnan(got[:, Dl:]).all(), ("l2norm_rows wrote its padding", what)
    vals = f32(rng.standard_normal(N) * 10.0 ** rng.integers(-3, 4, N))
    got = twice(lambda: be.sum_f32_to_f64(vals))
    exact("sum_f32_to_f64", np.array([got]), np.array([R.sum_blocks_256(vals)]), what)


def check_col_stats(be, N, D):
    """multiples of 2^-8 in [-4, 4]: squares are multiples of 2^-16 up to 16, so a column of 3001 rows needs 12 + 4 + 16 bits"""
    case("col_stats")
    G = grid(np.random.default_rng(N + D), (N, D), 2.0 ** -8, 4.0)
    s, q = twice(lambda: be.col_stats(pad(G, D + 1), D))
    es, eq = R.ref_col_stats(G)
    exact("col_stats.sum", s, es, (N, D))
    exact("col_stats.sumsq", q, eq, (N, D))


def check_l2norm_gauss(be):
    """Gaussian rows against float64: the norm's double sum is as good as exact, float32(sqrt) rounds once, the division once:
    2 units of 2^-24 |out|, one to spare"""
    case("l2norm_gauss")
    X = f32(np.random.default_rng(8).standard_normal((65, 2049)))
    got = twice(lambda: be.l2norm_rows(pad(X, 2052), 2049, 2049))
    ref = R.ref_l2norm(X)
    gate("l2norm_rows.gauss", got, ref, np.abs(ref), 3, (65, 2049))


def check_identity_perm(be):
    """permute_k8(C_new) == C_new_perm of finalize, both from the device"""
    case("permute_identity")
    rng = np.random.default_rng(9)
    K, D = 7, 16
    counts = f32(FIN_COUNTS["zeros_0_mid_last"])
    sums, C_old = f32(rng.standard_normal((K, D))), f32(rng.standard_normal((K, D)))
    C_new, cp, _, _, _ = be.finalize(C_old, sums, counts)
    exact("permute_k8(C_new) == C_new_perm", be.permute_k8(C_new, D, D), cp)


# ------------------------------------------------------------------ slic_kmeanspp_step
KPP_NS = (1, 255, 256, 257, 1300)
KPP_DS = (4, 64, 512)
KPP_TS = (1, 6, 16)


def kpp_cand(N, T):
    return np.array(([0, N - 1, N // 2, N // 2] + [(7 * t) % N for t in range(T)])[:T], I32)       # first, last and a repeated row


def check_kpp_grid(be, N, D, T, with_closest):
    """rows on a 2^-3 grid with |v| <= 2: a difference is a multiple of 2^-3 up to 4, its square a multiple of 2^-6 up to 16, a
    distance (D <= 1024) needs 14 + 6 bits: exact in float32 whatever the order; the potential of 1300 rows needs 11 more: exact in
    double whatever the order"""
    case("kpp_step")
    rng = np.random.default_rng(N + D + T)
    G = grid(rng, (N, D), 2.0 ** -3, 2.0)
    cand = kpp_cand(N, T)
    closest = (rng.integers(0, 8 * D, N) / 64.0).astype(F32) if with_closest else None
    nd, pot = twice(lambda: be.kpp_step(pad(G, D + 4), D, cand, closest))
    e_nd, e_pot = R.ref_kpp(G, cand, closest)
    what = (N, D, T, with_closest)
    exact("kpp_step.newdist", nd, R.kpp_step(G, cand, closest)[0], what)
    exact("kpp_step.newdist_vs_float64", nd, e_nd.astype(F32), what)
    assert np.array_equal(e_nd.astype(F32).astype(F64), e_nd)
    exact("kpp_step.pot", pot, e_pot, what)


def check_kpp_gauss(be, with_closest=True):
    """Gaussian rows: newdist is the fmaf chain, bit for bit.  pot against float64 of the whole operation: a distance carries
    2 roundings from its differences' squares and D from its chain (all terms positive: relative to the value); the double sum adds
    nothing visible at 2^-24.  coef = D + 2, in units of 2^-24 pot."""
    case("kpp_step")
    N, D, T = 1300, 64, 6
    rng = np.random.default_rng(21)
    X = f32(rng.standard_normal((N, D)))
    cand = kpp_cand(N, T)
    closest = f32(rng.random(N) * 2 * D) if with_closest else None
    nd, pot = twice(lambda: be.kpp_step(pad(X, D + 4), D, cand, closest))
    exact("kpp_step.newdist", nd, R.kpp_step(X, cand, closest)[0], "gauss")
    ref = R.ref_kpp(X, cand, closest)[1]
    gate("kpp_step.pot.gauss", pot, ref, ref, D + 2, "gauss")
    # and against the double sum of its own (exact-chain) distances: 1300 terms, 2^-53 each at most
    own = nd.astype(F64).sum(1)
    assert np.all(np.abs(pot - own) <= N * 2.0 ** -53 * own), (pot, own)


# ------------------------------------------------------------------ slic_cumsum_search
CS_NS = (1, 15, 16, 1023, 1024, 1025, 2064, 5000)
CS_TS = (1, 5, 16)
CS_STEP = 2.0 ** -10


def cs_problem(N):
    """v: multiples of 2^-10 in [0, 8], a third of them zero, zero runs after row 37 and after the first chunk (a chosen centre has
    distance 0); 5000 values of at most 8 need 16 + 10 bits: every prefix sum is exact in double"""
    rng = np.random.default_rng(N)
    v = (rng.integers(0, 8193, N) * (rng.random(N) < 0.67)).astype(F64) * CS_STEP
    v[0] = 3 * CS_STEP
    if N > 45:
        v[38:44] = 0
    if N > 1030:
        v[1024:1030] = 0
    cs = np.cumsum(v)
    inside, chunk = cs[min(N - 1, 37)], cs[min(N - 1, 1023)]
    q = [0.0, CS_STEP, inside, chunk, inside + CS_STEP, chunk + CS_STEP, cs[-1], 2 * cs[-1], cs[N // 2], cs[-1] + CS_STEP,
         cs[min(N - 1, 2047)], cs[min(N - 1, 2047)] + CS_STEP]
    return v.astype(F32), np.array(q, F64)


def check_cumsum_search(be, N, T):
    case("cumsum_search")
    v, q = cs_problem(N)
    assert np.array_equal(v.astype(F64) / CS_STEP, np.round(v.astype(F64) / CS_STEP))
    for b in range(0, len(q), T):
        vals = np.resize(q[b:b + T], T)
        got = twice(lambda: be.cumsum_search(v, vals))
        exact("cumsum_search", got, R.ref_cumsum_search(v, vals), (N, T, b))


# ------------------------------------------------------------------ argument rules (no device work: every call is refused first)
def check_argument_rules(lib):
    """every SLIC_REQUIRE of the covered entry points returns non-zero and names itself in slic_last_error; the pointers are never
    read (each call is refused before any launch: the rules stand at the top of every launcher in kmeans.hip)"""
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(p.value + 256)
    BIG = 1 << 31
    n = 0

    def refused(name, *args, say=None):
        nonlocal n
        n += 1
        assert getattr(lib, name)(*args, None) != 0, (name, args)
        assert (say or name).encode() in lib.slic_last_error(), (name, lib.slic_last_error())

    valid = {                                           # argument lists that would launch, and which pointers may be NULL
        "slic_kmeans_cnorm": ([p, 4, 8, 8, p], ()),
        "slic_kmeans_permute_k8": ([p, 4, 8, 8, q, 8], ()),
        "slic_kmeans_accumulate": ([p, 4, 8, 8, p, 3, p, p, p], ()),
        "slic_kmeans_combine_shards": ([p, p, 64, 2, 3, 8, p, p], ()),
        "slic_kmeans_dist_to_assigned": ([p, 4, 8, 8, p, 8, p, p], ()),
        "slic_sum_f32_to_f64": ([p, 4, p, p], ()),
        "slic_kmeans_select_far": ([p, 4, 1, p, p], ()),
        "slic_kmeans_apply_relocation": ([p, 8, p, p, 1, 8, p, p], ()),
        "slic_kmeans_finalize": ([p, q, p, 3, 8, ctypes.c_void_p(p.value + 128), p, p, p, 0, p, p], (7, 8, 10)),
        "slic_kmeans_lloyd_step": ([p, p, 4, 8, 8, p, p, p, 3, p, p, p, q, p, ctypes.c_void_p(p.value + 128), p, p, p, 0, p, p], (10,)),
        "slic_kmeans_lloyd_global": ([p, 0, 64, 2, p, 3, 8, q, p, ctypes.c_void_p(p.value + 128), p, p, p, 0, p], (10, 11)),
        "slic_col_stats": ([p, 4, 8, 8, p, p, p], ()),
        "slic_sub_rowvec": ([p, 4, 8, 8, p, p, 8], ()),
        "slic_l2norm_rows": ([p, 4, 8, 8, p, 8], ()),
        "slic_kmeanspp_step": ([p, 4, 8, 8, p, 2, p, p, p, p], (6,)),
        "slic_cumsum_search": ([p, 4, p, 2, p, p], ()),
    }

    def with_(name, **kw):
        a = list(valid[name][0])
        for k, v in kw.items():
            a[int(k[1:])] = v
        return a

    for name, (args, nullable) in valid.items():
        for i, a in enumerate(args):
            if isinstance(a, ctypes.c_void_p) and i not in nullable:
                refused(name, *with_(name, **{f"a{i}": None}))
    # D % 4 / D % 8
    refused("slic_kmeans_permute_k8", *with_("slic_kmeans_permute_k8", a2=12))
    refused("slic_kmeans_accumulate", *with_("slic_kmeans_accumulate", a2=6))
    refused("slic_kmeans_dist_to_assigned", *with_("slic_kmeans_dist_to_assigned", a2=6))
    refused("slic_sub_rowvec", *with_("slic_sub_rowvec", a2=6))
    refused("slic_kmeanspp_step", *with_("slic_kmeanspp_step", a2=6))
    refused("slic_kmeans_lloyd_step", *with_("slic_kmeans_lloyd_step", a3=12, a4=12))
    refused("slic_kmeans_lloyd_step", *with_("slic_kmeans_lloyd_step", a14=p))                    # C_new == C_old
    refused("slic_kmeans_lloyd_step", *with_("slic_kmeans_lloyd_step", a14=q))                    # C_new == sums
    refused("slic_kmeans_finalize", *with_("slic_kmeans_finalize", a4=12, a8=p))                 # C_new_perm needs D % 8
    refused("slic_kmeans_lloyd_global", *with_("slic_kmeans_lloyd_global", a6=4, a10=p))
    # a stride smaller than D
    refused("slic_kmeans_cnorm", *with_("slic_kmeans_cnorm", a3=4))
    refused("slic_kmeans_permute_k8", *with_("slic_kmeans_permute_k8", a3=4))
    refused("slic_kmeans_permute_k8", *with_("slic_kmeans_permute_k8", a5=4))
    refused("slic_kmeans_accumulate", *with_("slic_kmeans_accumulate", a3=4))
    refused("slic_kmeans_dist_to_assigned", *with_("slic_kmeans_dist_to_assigned", a3=4))
    refused("slic_kmeans_dist_to_assigned", *with_("slic_kmeans_dist_to_assigned", a5=4))
    refused("slic_kmeans_apply_relocation", *with_("slic_kmeans_apply_relocation", a1=4))
    refused("slic_col_stats", *with_("slic_col_stats", a3=7))
    refused("slic_sub_rowvec", *with_("slic_sub_rowvec", a3=4))
    refused("slic_sub_rowvec", *with_("slic_sub_rowvec", a6=4))
    refused("slic_l2norm_rows", *with_("slic_l2norm_rows", a3=7))
    refused("slic_l2norm_rows", *with_("slic_l2norm_rows", a5=7))
    refused("slic_kmeanspp_step", *with_("slic_kmeanspp_step", a3=4))
    # C_new aliasing
    refused("slic_kmeans_finalize", *with_("slic_kmeans_finalize", a5=p))                        # == C_old
    refused("slic_kmeans_finalize", *with_("slic_kmeans_finalize", a5=q))                        # == sums
    refused("slic_kmeans_lloyd_global", *with_("slic_kmeans_lloyd_global", a9=p))                # == C_old
    refused("slic_kmeans_lloyd_global", *with_("slic_kmeans_lloyd_global", a9=q))                # == sums
    # payload stride, T, K, D, N
    refused("slic_kmeans_lloyd_global", *with_("slic_kmeans_lloyd_global", a2=3 * 8 + 3 + 1))
    refused("slic_kmeans_lloyd_global", *with_("slic_kmeans_lloyd_global", a6=8200))
    refused("slic_kmeans_finalize", *with_("slic_kmeans_finalize", a4=8200))
    refused("slic_kmeanspp_step", *with_("slic_kmeanspp_step", a5=17))
    refused("slic_kmeanspp_step", *with_("slic_kmeanspp_step", a5=0))
    refused("slic_kmeanspp_step", *with_("slic_kmeanspp_step", a2=2048, a3=2048, a5=16))         # T D 4 > 64 KiB
    refused("slic_kmeans_accumulate", *with_("slic_kmeans_accumulate", a5=16385))
    refused("slic_kmeans_accumulate", *with_("slic_kmeans_accumulate", a1=BIG))                  # N >= 2^31: int32 row ids
    refused("slic_kmeans_select_far", *with_("slic_kmeans_select_far", a1=BIG))
    refused("slic_cumsum_search", *with_("slic_cumsum_search", a1=BIG))
    refused("slic_kmeanspp_step", *with_("slic_kmeanspp_step", a1=BIG))
    for name, i in (("slic_kmeans_cnorm", 1), ("slic_kmeans_accumulate", 1), ("slic_kmeans_accumulate", 5), ("slic_kmeans_select_far", 1),
                    ("slic_kmeans_select_far", 2), ("slic_kmeans_apply_relocation", 4), ("slic_kmeans_finalize", 3),
                    ("slic_sum_f32_to_f64", 1), ("slic_col_stats", 1), ("slic_cumsum_search", 1), ("slic_cumsum_search", 3),
                    ("slic_kmeanspp_step", 1), ("slic_kmeans_combine_shards", 3), ("slic_kmeans_lloyd_global", 3)):
        refused(name, *with_(name, **{f"a{i}": 0}))                                             # an empty problem
    return n


# ------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def dev(gpu):
    return Device(gpu)


@pytest.mark.parametrize("K", SORT_KS)
def test_accumulate_counting_sort(dev, monkeypatch, K):
    for kind in SORT_LABELS:
        check_accumulate(dev, monkeypatch, 3000, 8, K, kind)


def test_accumulate_column_slice(dev, monkeypatch):
    check_accumulate(dev, monkeypatch, 3000, 8, 1366, "uniform", ldx=24, off=4)
    check_accumulate(dev, monkeypatch, 3000, 8, 40, "uniform", scan=None, ldx=24, off=4)           # the one-launch scan route


@pytest.mark.parametrize("D", WIDE_DS)
def test_accumulate_wide_rows(dev, monkeypatch, D):
    for scan in (None, "0"):
        check_accumulate(dev, monkeypatch, 700, D, 9, "uniform", scan=scan)


def test_accumulate_largest_k(dev, monkeypatch):
    """K = 16384: km_block_hist with 64 KiB and km_place with 128 KiB of dynamic LDS"""
    check_accumulate(dev, monkeypatch, 3000, 4, 16384, "uniform")


@pytest.mark.parametrize("spherical", (0, 1))
@pytest.mark.parametrize("empty", STEP_EMPTY)
@pytest.mark.parametrize("route", list(STEP_ROUTES))
def test_lloyd_step(dev, route, empty, spherical):
    check_lloyd_step(dev, route, empty, spherical)


@pytest.mark.parametrize("D", FIN_DS)
def test_finalize(dev, D):
    for which in FIN_COUNTS:
        check_finalize(dev, D, which)
    check_finalize(dev, D, "zeros_0_mid_last", spherical=1)


def test_finalize_status_loops(dev):
    check_finalize_k300(dev)
    check_identity_perm(dev)


@pytest.mark.parametrize("W,dtype", GLOBAL_FORMS, ids=[f"{w}x{np.dtype(d).name}" for w, d in GLOBAL_FORMS])
def test_lloyd_global_and_combine_shards(dev, W, dtype):
    check_global(dev, W, dtype)


@pytest.mark.parametrize("N", FAR_NS)
def test_select_far(dev, N):
    for n_sel in FAR_SELS:
        for kind in FAR_KINDS:
            check_select_far(dev, N, n_sel, kind)


def test_apply_relocation(dev):
    for n, D in RELOC_CASES:
        check_apply_relocation(dev, n, D)


@pytest.mark.parametrize("D", ROW_DS)
def test_rowwise(dev, D):
    for N in ROW_NS:
        check_rowwise(dev, N, D)


def test_col_stats_and_l2norm(dev):
    for N in COL_NS:
        for D in COL_DS:
            check_col_stats(dev, N, D)
    check_l2norm_gauss(dev)


@pytest.mark.parametrize("D", KPP_DS)
def test_kmeanspp_step(dev, D):
    for N in KPP_NS:
        for T in KPP_TS:
            for with_closest in (True, False):
                check_kpp_grid(dev, N, D, T, with_closest)


def test_kmeanspp_step_gaussian_and_largest(dev):
    check_kpp_gauss(dev, True)
    check_kpp_gauss(dev, False)
    check_kpp_grid(dev, 300, 1024, 16, True)           # T D 4 = 64 KiB of candidate rows: the largest admitted size


@pytest.mark.parametrize("N", CS_NS)
def test_cumsum_search(dev, N):
    for T in CS_TS:
        check_cumsum_search(dev, N, T)


def test_argument_rules_then_a_valid_call(dev, gpu):
    assert check_argument_rules(gpu) >= 120
    check_rowwise(dev, 65, 8)
    print("cases:", dict(CASES), "ratios:", {k: round(v, 4) for k, v in RATIOS.items()})

"""
Host driver of the gfx950 k-means (C ABI: include/slic_hip.h, kernels: csrc/kmeans.hip).

Mirrors the object the reference builds at clustering/cluster_masks.py:70-71,
    KMeans(n_clusters=k, n_init=10).fit(embeddings).labels_
i.e. sklearn.cluster.KMeans (algorithm='lloyd'):
    KMeans.fit             sklearn/cluster/_kmeans.py:1427-1540  (centre X, tol, n_init loop, best inertia)
    _kmeans_single_lloyd   sklearn/cluster/_kmeans.py:624-752    (loop, strict / tol convergence, final E-step)
    _kmeans_plusplus       sklearn/cluster/_kmeans.py:174-277    (seeding; host RNG, device distances)
Only control flow lives here; every reduction/contraction is a HIP kernel reached through
`HipKernels` (one method per C-ABI entry point).  One host sync per Lloyd iteration (a 4-double
status word).

A Lloyd iteration has exactly two forms, and a run picks its form — and its E-step precision — once, before the loop:
    unsharded : ONE fused foreign call (slic_kmeans_lloyd_step[_bf16]: E-step, ordered M-step, averaging, status word);
    sharded   : local half -> poison rule -> ONE collective -> global half (below).
What a sharded fit asks of its process group (route of the collective, payload dtype, bounded waits, the small set-up exchanges)
is resolved once per fit: clustering/kmeans_exchange.py.

Multi-GPU: pass `process_group`; X is then this rank's contiguous row shard
(rank order == row order).  An iteration is two foreign calls around ONE collective over RCCL/xGMI
(it replaces the rank-0 k-means + barrier of online_train.py:625-662):
    slic_kmeans_lloyd_local  : E-step + ordered M-step on the rank's rows -> payload [K*D sums | K counts | n_changed]
    exchange='allreduce' (default): ONE all-reduce(sum) of the payload, widened to fp64 — a sum of a few fp32 values in
        fp64 is exact, so the result does not depend on RCCL's reduction order and every rank holds bit-identical
        centres; equals the oracle run with n_shards = -world (fp64 combine);
    exchange='allgather': ONE all-gather of the fp32 payloads, added in rank order on every GPU; equals the oracle
        run with n_shards = world (== sklearn's per-thread buffers reduced in thread order);
    slic_kmeans_lloyd_global : combine + averaging + shift + next norms + status word.

precision="bf16" (DESIGN.md §7f): the E-step of every iteration, sharded or not, and the final relabelling run as a certified bf16
candidate pass with exact rescoring (slic_kmeans_lloyd_step_bf16 / _lloyd_local_bf16 / _assign_bf16) — the same labels to the bit.  The
bf16 image and the norms of the centred rows are made once per fit, like the k-permuted copy and what k-means++ reads, and handed
down to the runs; its three counters are read once, after the fit (bf16_stats_).
"""
import ctypes
import functools
import os
import time

import numpy as np
import torch

from .. import _lib
from .._lib import call, ptr, stream
from ._device import require_device, resident_rows
from .kmeans_exchange import Exchange, _slic_oneshot  # noqa: F401 — tests/dist_gpu_worker.py reaches the one-shot set-up through this module


_POISON = float(2 ** 40)      # in the n_changed high slot of a sharded payload: this rank's local half failed (exact in fp32 and fp64, sums of <= 16 too)

class HipKernels:
    """Thin argument marshalling for the k-means entry points of libslic_hip.so.  The only kernel
    provider the package ships; `KMeans(kernels=...)` exists so the multi-process control flow can be
    exercised under gloo on a GPU-less host by the tests (tests/kmeans_cpu_kernels.py).

    What `KMeans` calls on its provider — a second provider implements these with the same argument meaning:
        check  to_device  col_stats  sub_rowvec  l2norm_rows  cnorm  dist_to_assigned  sum_f64            (fit, inertia)
        lloyd_step | lloyd_local + lloyd_global   finalize  assign   select_far  apply_relocation           (a Lloyd run)
        kpp_run                                                                                             (k-means++)
    and what a provider may lack, declared as class attributes instead of being probed for:
        uses_perm      True: the E-step reads k-permuted twins of the rows and the centres (permute_k8, assign_perm)
        has_bf16       True: bf16_image, assign_bf16, lloyd_step_bf16, lloyd_local_bf16 exist (they need uses_perm)
        kpp_run_batch  the lock-step seeding of an n_init loop (it needs uses_perm), or None"""

    device_type = "cuda"
    uses_perm = True       # E-step on k-permuted copies of X and the centres (LDS-DMA kernel)
    has_bf16 = True

    def check(self):
        require_device("k-means")
        _lib.check(_lib.load().slic_device_check(), "slic_device_check")

    def to_device(self, X):
        return resident_rows(X, "k-means", dense=True)

    def col_stats(self, X):
        N, Dp = X.shape
        cs = torch.empty(2, Dp, dtype=torch.float64, device=X.device)
        ws = _lib.workspace(_lib.load().slic_col_stats_workspace_bytes(N, Dp), X.device, "km_cs")
        call("slic_col_stats", ptr(X), N, Dp, X.stride(0), ptr(cs[0]), ptr(cs[1]), ptr(ws), stream())
        return cs

    def sub_rowvec(self, X, v, out):
        call("slic_sub_rowvec", ptr(X), X.shape[0], X.shape[1], X.stride(0), ptr(v), ptr(out), out.stride(0), stream())

    def cnorm(self, C, cnorm):
        call("slic_kmeans_cnorm", ptr(C), C.shape[0], C.shape[1], C.stride(0), ptr(cnorm), stream())

    def assign(self, X, C, cnorm, labels, labels_old, n_changed):
        N, Dp = X.shape
        K = C.shape[0]
        ws = _lib.workspace(_lib.load().slic_kmeans_assign_workspace_bytes(N, K), X.device, "km_assign")
        call("slic_kmeans_assign", ptr(X), N, Dp, X.stride(0), ptr(C), K, C.stride(0), ptr(cnorm), ptr(labels),
             ptr(labels_old), ptr(n_changed), None, ptr(ws), stream())

    def permute_k8(self, X, Xp):
        call("slic_kmeans_permute_k8", ptr(X), X.shape[0], X.shape[1], X.stride(0), ptr(Xp), Xp.stride(0), stream())

    def assign_perm(self, Xp, Cp, cnorm, labels, labels_old, n_changed):
        N, Dp = Xp.shape
        K = Cp.shape[0]
        ws = _lib.workspace(_lib.load().slic_kmeans_assign_workspace_bytes(N, K), Xp.device, "km_assign")
        call("slic_kmeans_assign_perm", ptr(Xp), N, Dp, Xp.stride(0), ptr(Cp), K, Cp.stride(0), ptr(cnorm), ptr(labels),
             ptr(labels_old), ptr(n_changed), None, ptr(ws), stream())

    def lloyd_step(self, X, Xp, C_old, Cp_old, cnorm_old, labels, labels_old, n_changed, sums, counts, C_new, Cp_new,
                   cnorm_new, shift, status, spherical=False):
        """one whole unsharded iteration in one foreign call (the Python loop is otherwise the bottleneck at ~0.6 ms)"""
        N, Dp = X.shape
        K = C_old.shape[0]
        assert X.stride(0) == Xp.stride(0) and C_old.is_contiguous() and Cp_old.is_contiguous() and C_new.is_contiguous()
        ws = _lib.workspace(_lib.load().slic_kmeans_lloyd_step_workspace_bytes(N, K), X.device, "km_step")
        call("slic_kmeans_lloyd_step", ptr(X), ptr(Xp), N, Dp, X.stride(0), ptr(C_old), ptr(Cp_old), ptr(cnorm_old), K,
             ptr(labels), ptr(labels_old), ptr(n_changed), ptr(sums), ptr(counts), ptr(C_new), ptr(Cp_new), ptr(cnorm_new),
             ptr(shift), int(spherical), ptr(status), ptr(ws), stream())

    def lloyd_local(self, X, Xp, C_old, Cp_old, cnorm_old, labels, labels_old, payload):
        """sharded iteration, part 1 (before the collective): E-step + ordered M-step -> payload (fp32 or fp64 tensor of
        K*D + K + 2 numbers)"""
        N, Dp = X.shape
        K = Cp_old.shape[0]
        assert X.stride(0) == Xp.stride(0) and Cp_old.is_contiguous() and payload.numel() == K * Dp + K + 2
        ws = _lib.workspace(_lib.load().slic_kmeans_lloyd_local_workspace_bytes(N, K), X.device, "km_step")
        call("slic_kmeans_lloyd_local", ptr(X), ptr(Xp), N, Dp, X.stride(0), ptr(Cp_old), ptr(cnorm_old), K, ptr(labels),
             ptr(labels_old), ptr(payload), int(payload.dtype == torch.float64), ptr(ws), stream())

    # ---- the certified bf16 E-step (include/slic_hip.h: slic_kmeans_*_bf16): same labels as the calls above
    def bf16_image(self, X, want_norms=False):
        """-> (bf16 image [N, Dp] of the rows as an int16 tensor, ||x_i|| or None)"""
        N, D = X.shape
        Dp = (D + 15) // 16 * 16
        img = torch.empty(N, Dp, dtype=torch.int16, device=X.device)
        norms = torch.empty(N, dtype=torch.float32, device=X.device) if want_norms else None
        call("slic_kmeans_bf16_image", ptr(X), N, D, X.stride(0), ptr(img), ptr(norms), stream())
        return img, norms

    def assign_bf16(self, X, Xb, xnorm, C, Cb, cnorm, labels, labels_old, n_changed, stats):
        N, Dp = X.shape
        K = C.shape[0]
        ws = _lib.workspace(_lib.load().slic_kmeans_assign_bf16_workspace_bytes(N, K), X.device, "km_assign_bf16")
        call("slic_kmeans_assign_bf16", ptr(X), ptr(Xb), ptr(xnorm), N, Dp, X.stride(0), ptr(C), ptr(Cb), ptr(cnorm), K, C.stride(0),
             ptr(labels), ptr(labels_old), ptr(n_changed), ptr(stats), ptr(ws), stream())

    def lloyd_step_bf16(self, X, Xp, Xb, xnorm, C_old, Cb, cnorm_old, labels, labels_old, n_changed, sums, counts, C_new, Cp_new,
                        cnorm_new, shift, status, stats, spherical=False):
        """lloyd_step with the bf16 E-step inside; Cb is scratch for C_old's image"""
        N, Dp = X.shape
        K = C_old.shape[0]
        assert X.stride(0) == Xp.stride(0) and C_old.is_contiguous() and C_new.is_contiguous()
        ws = _lib.workspace(_lib.load().slic_kmeans_lloyd_step_bf16_workspace_bytes(N, K), X.device, "km_step_bf16")
        call("slic_kmeans_lloyd_step_bf16", ptr(X), ptr(Xp), ptr(Xb), ptr(xnorm), N, Dp, X.stride(0), ptr(C_old), ptr(Cb), ptr(cnorm_old), K,
             ptr(labels), ptr(labels_old), ptr(n_changed), ptr(sums), ptr(counts), ptr(C_new), ptr(Cp_new), ptr(cnorm_new),
             ptr(shift), int(spherical), ptr(status), ptr(stats), ptr(ws), stream())

    def lloyd_local_bf16(self, X, Xp, Xb, xnorm, C_old, Cb, cnorm_old, labels, labels_old, payload, stats):
        """lloyd_local with the bf16 E-step inside"""
        N, Dp = X.shape
        K = C_old.shape[0]
        assert X.stride(0) == Xp.stride(0) and C_old.is_contiguous() and payload.numel() == K * Dp + K + 2
        ws = _lib.workspace(_lib.load().slic_kmeans_lloyd_local_bf16_workspace_bytes(N, K), X.device, "km_step_bf16")
        call("slic_kmeans_lloyd_local_bf16", ptr(X), ptr(Xp), ptr(Xb), ptr(xnorm), N, Dp, X.stride(0), ptr(C_old), ptr(Cb), ptr(cnorm_old), K,
             ptr(labels), ptr(labels_old), ptr(payload), int(payload.dtype == torch.float64), ptr(stats), ptr(ws), stream())

    def lloyd_global(self, parts, C_old, sums, counts, C_new, Cp_new, cnorm_new, shift, status, spherical=False):
        """sharded iteration, part 2 (after the collective): parts = [W, K*D + K + 2] gathered fp32 payloads or
        [1, K*D + K + 2] reduced fp64 payload -> combined sums / counts, new centres, status word"""
        K, Dp = C_old.shape
        W, stride = parts.shape
        call("slic_kmeans_lloyd_global", ptr(parts), int(parts.dtype == torch.float64), stride, W, ptr(C_old), K, Dp,
             ptr(sums), ptr(counts), ptr(C_new), ptr(Cp_new), ptr(cnorm_new), ptr(shift), int(spherical), ptr(status), stream())

    def l2norm_rows(self, X, out):
        call("slic_l2norm_rows", ptr(X), X.shape[0], X.shape[1], X.stride(0), ptr(out), out.stride(0), stream())

    def kpp_run(self, X, first, K, T, uniforms, idx_out, Xp=None, xnorm=None):
        N, Dp = X.shape
        assert Xp is None or Xp.stride(0) == X.stride(0)
        ws = _lib.workspace(_lib.load().slic_kmeanspp_run_workspace_bytes(N, T), X.device, "kpp_run")
        call("slic_kmeanspp_run", ptr(X), N, Dp, X.stride(0), int(first), int(K), int(T), ptr(uniforms), ptr(idx_out),
             ptr(Xp), ptr(xnorm), ptr(ws), stream())

    def kpp_run_batch(self, Xp, xnorm, firsts, K, T, uniforms, idx_out):
        """all R = len(firsts) initialisations of an n_init loop in lock-step (slic_kmeanspp_run_batch)"""
        N, Dp = Xp.shape
        R = len(firsts)
        arr = (ctypes.c_int32 * R)(*[int(f) for f in firsts])
        ws = _lib.workspace(_lib.load().slic_kmeanspp_run_batch_workspace_bytes(N, T, R), Xp.device, "kpp_batch")
        call("slic_kmeanspp_run_batch", ptr(Xp), ptr(xnorm), N, Dp, Xp.stride(0), R, arr, int(K), int(T), ptr(uniforms), ptr(idx_out),
             ptr(ws), stream())

    def accumulate(self, X, labels, K, sums, counts):
        N, Dp = X.shape
        ws = _lib.workspace(_lib.load().slic_kmeans_accumulate_workspace_bytes(N, K), X.device, "km_accum")
        call("slic_kmeans_accumulate", ptr(X), N, Dp, X.stride(0), ptr(labels), K, ptr(sums), ptr(counts),
             ptr(ws), stream())

    def combine_shards(self, allpart, K, Dp, sums, counts):
        W, stride = allpart.shape
        call("slic_kmeans_combine_shards", ptr(allpart), ptr(allpart[0, K * Dp:]), stride, W, K, Dp,
             ptr(sums), ptr(counts), stream())

    def finalize(self, C_old, sums, counts, C_new, shift, n_changed, status, cnorm_new=None, C_new_perm=None, spherical=False):
        K, Dp = C_old.shape
        call("slic_kmeans_finalize", ptr(C_old), ptr(sums), ptr(counts), K, Dp, ptr(C_new), ptr(shift),
             ptr(cnorm_new), ptr(C_new_perm), int(spherical), ptr(n_changed), ptr(status), stream())

    def dist_to_assigned(self, X, C, labels, dist):
        call("slic_kmeans_dist_to_assigned", ptr(X), X.shape[0], X.shape[1], X.stride(0), ptr(C), C.stride(0),
             ptr(labels), ptr(dist), stream())

    def sum_f64(self, v, out):
        ws = _lib.workspace(_lib.load().slic_sum_f32_to_f64_workspace_bytes(v.numel()), v.device, "km_sum")
        call("slic_sum_f32_to_f64", ptr(v), v.numel(), ptr(out), ptr(ws), stream())

    def select_far(self, dist, n_sel, far_idx, far_dist):
        call("slic_kmeans_select_far", ptr(dist), dist.numel(), n_sel, ptr(far_idx), ptr(far_dist), stream())

    def apply_relocation(self, xfar, old_ids, new_ids, sums, counts):
        n, Dp = xfar.shape
        call("slic_kmeans_apply_relocation", ptr(xfar), xfar.stride(0), ptr(old_ids), ptr(new_ids), n, Dp,
             ptr(sums), ptr(counts), stream())

    def kpp_step(self, X, cand, T, closest, newdist, pot):
        N, Dp = X.shape
        ws = _lib.workspace(_lib.load().slic_kmeanspp_step_workspace_bytes(N, T), X.device, "kpp_p")
        call("slic_kmeanspp_step", ptr(X), N, Dp, X.stride(0), ptr(cand), T, ptr(closest), ptr(newdist), ptr(pot),
             ptr(ws), stream())

    def cumsum_search(self, v, vals, T, idx_out):
        ws = _lib.workspace(_lib.load().slic_cumsum_search_workspace_bytes(v.numel()), v.device, "kpp_c")
        call("slic_cumsum_search", ptr(v), v.numel(), ptr(vals), T, ptr(idx_out), ptr(ws), stream())


def _dist_on(pg):
    # a process group of ONE rank still takes the sharded path (all-gather of one partial, ordered add): that is
    # how a single-GPU box exercises the RCCL code path
    return pg is not None and torch.distributed.is_initialized()


def _kpp_trials(K):
    """n_local_trials of _kmeans_plusplus: 2 + int(ln K)"""
    T = 2 + int(np.log(K))
    if T > 16:
        raise ValueError(f"k-means++ with n_clusters={K}: {T} local trials per centre, slic_kmeanspp_run takes at most 16 "
                         "(n_clusters < 3 269 018); pass init= explicitly")
    return T


class KMeans:
    """sklearn-shaped: KMeans(n_clusters, n_init=10, max_iter=300, tol=1e-4).fit(X) -> labels_, cluster_centers_,
    inertia_, n_iter_.  `init` may be 'k-means++' (default, as the reference uses), an [K, D] array, or a list of
    such arrays (one per run).  X: torch tensor [N, D] fp32 on a gfx950 device (a CPU tensor / ndarray is
    copied to the current device)."""

    def __init__(self, n_clusters, n_init=10, max_iter=300, tol=1e-4, init="k-means++", random_state=None,
                 process_group=None, fixed_iters=False, trace=False, kernels=None, spherical=False, exchange=None, precision=None):
        self.n_clusters = int(n_clusters)
        self.n_init = int(n_init)
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.init = init
        self.random_state = random_state
        self.process_group = process_group
        self.fixed_iters = bool(fixed_iters)   # throughput runs: skip the stopping tests
        self.trace = bool(trace)               # keep every iteration's labels (tests)
        # spherical k-means (clustering/cluster_masks.py:73-77 -> spherecluster.SphericalKMeans): rows L2-normalised, no
        # mean-centring, centres renormalised after every averaging, tol compared unscaled
        self.spherical = bool(spherical)
        exchange = exchange or os.environ.get("SLIC_KMEANS_EXCHANGE", "allreduce")
        assert exchange in ("allreduce", "allgather", "oneshot"), exchange
        self.exchange = exchange               # the sharded run's one collective per iteration (module docstring)
        self.k = kernels if kernels is not None else HipKernels()
        # the E-step's arithmetic: 'fp32' (the MFMA chain itself) or 'bf16' (certified bf16 candidates + exact rescoring: the same labels,
        # DESIGN.md §7f).  None: 'fp32', or — SLIC_KMEANS_BF16=1 — 'bf16' wherever the fit is inside that path's domain (D <= 512)
        if precision not in (None, "fp32", "bf16"):
            raise ValueError(f"precision={precision!r}: 'fp32' or 'bf16'")
        self.precision = precision
        self.bf16_stats_ = None
        self._ex = None                        # the current fit's Exchange (kmeans_exchange.py); None: not sharded
        self._fit_rs = None
        self._side = None

    # ------------------------------------------------------------------ helpers
    def _rng(self):
        """check_random_state(self.random_state), ONCE per fit (KMeans.fit, _kmeans.py:1467: the n_init runs share the stream)"""
        rs = self.random_state
        if rs is None:
            return np.random.mtrand._rand     # sklearn check_random_state(None): numpy's global RandomState
        if isinstance(rs, (int, np.integer)):
            if self._fit_rs is None:
                self._fit_rs = np.random.RandomState(rs)
            return self._fit_rs
        return rs

    def _rank_sum(self, t):
        """a float64 device tensor -> numpy; in a sharded fit the ranks' tensors added in rank order"""
        if self._ex is None:
            return t.cpu().numpy()
        parts = self._ex.gather(t).cpu().numpy()           # [W, *]
        tot = np.zeros_like(parts[0])
        for r in range(parts.shape[0]):
            tot += parts[r]
        return tot

    # ------------------------------------------------------------------ fit
    def fit(self, X):
        self._fit_rs = None
        self.init_indices_log_ = []
        bf16 = self._use_bf16(int(np.shape(X)[1]))                   # raises for precision='bf16' outside its domain: before any launch
        self.bf16_stats_ = None
        self.k.check()
        X = self.k.to_device(X)
        N, D = X.shape
        K = self.n_clusters
        dev = X.device
        # pad the feature dim to a multiple of 8 with zero columns (they add exact zeros to every chain)
        Dp = (D + 7) // 8 * 8
        if Dp != D:
            Xp = torch.zeros(N, Dp, dtype=torch.float32, device=dev)
            Xp[:, :D] = X
            X = Xp
        if _dist_on(self.process_group):
            self._ex = ex = Exchange(self.process_group, self.exchange, dev, K * Dp + K + 2)     # [sums | counts | n_changed lo, hi]
            self.communicator_kind_, self.payload_bytes_ = ex.communicator_kind_, ex.payload_bytes_
            sizes = ex.gather(torch.tensor([N], dtype=torch.int64, device=dev)).cpu().numpy().reshape(-1)
            self._row0 = int(sizes[:ex.rank].sum())
            Ng = int(sizes.sum())
        else:
            self._ex, self._row0, sizes, Ng = None, 0, np.array([N]), N

        if self.spherical:
            # SphericalKMeans.fit: X = normalize(X); the data is NOT centred and tol is used as given
            mean = np.zeros(Dp, np.float32)
            Xc = torch.empty_like(X)
            self.k.l2norm_rows(X, Xc)
            tol_abs = self.tol
        else:
            # X -= X.mean(axis=0)   (_kmeans.py:1479-1481)
            cs = self._rank_sum(self.k.col_stats(X))                    # global column sums / sums of squares
            mean = (cs[0] / float(Ng)).astype(np.float32)
            mean_d = torch.from_numpy(mean).to(dev)
            Xc = torch.empty_like(X)
            self.k.sub_rowvec(X, mean_d, Xc)
            # tol = mean(var(Xc, axis=0)) * tol   (_tolerance, _kmeans.py:279-288)
            tol_abs = 0.0
            if self.tol != 0:
                cs2 = self._rank_sum(self.k.col_stats(Xc))
                m = cs2[0] / float(Ng)
                var = cs2[1] / float(Ng) - m * m
                tol_abs = float(var[:D].sum() / D) * self.tol
        self.tol_abs_ = tol_abs

        inits = self.init
        if isinstance(inits, str):
            assert inits == "k-means++", inits
            inits = None
        elif isinstance(inits, (list, tuple)):
            inits = [np.asarray(a, np.float32) for a in inits]
        else:
            a = inits.detach().cpu().numpy() if torch.is_tensor(inits) else np.asarray(inits)
            inits = [np.asarray(a, np.float32)]
        n_runs = self.n_init if inits is None else len(inits)

        best = est = None
        seed = self._seed_rows(Xc, sizes, K) if inits is None else None
        seeds = self._kmeans_plusplus(seed, K, n_runs) if inits is None else None
        for run in range(n_runs):
            if inits is None:
                C0 = next(seeds)                           # rows of the centred matrix
            else:
                c = np.zeros((K, Dp), np.float32)
                c[:, :D] = inits[run] - mean[None, :D]
                C0 = torch.from_numpy(c).to(dev)
            if est is None:
                est = self._estep_images(Xc, seed, bf16)   # behind the first seeding: where these launches have always been
            res = self._lloyd_single(est, C0, tol_abs)
            if best is None or res["inertia"] < best["inertia"]:
                best = res
        self.labels_ = best["labels"].cpu().numpy()                 # np.int32, like sklearn's labels_
        self.labels_device_ = best["labels"]
        self.cluster_centers_ = best["centers"].cpu().numpy()[:, :D] + mean[None, :D]
        self.inertia_ = best["inertia"]
        self.n_iter_ = best["n_iter"]
        self.strict_ = best["strict"]
        self.n_relocations_ = best["n_relocations"]
        self.trace_ = best.get("trace")
        if bf16:
            st = est[4].cpu().tolist()                              # read once per fit
            self.bf16_stats_ = dict(rows_rescored=st[0], rows_overflowed=st[1], candidates=st[2])
        return self

    def _use_bf16(self, D):
        """does this fit run the certified bf16 E-step?  An explicit precision='bf16' outside the domain is an error, never a silent fp32 run"""
        Dp = (D + 7) // 8 * 8
        able = self.k.has_bf16 and self.k.uses_perm
        if self.precision == "bf16":
            if Dp > 512:
                raise ValueError(f"precision='bf16' takes D <= 512 (D={D}); use precision='fp32'")
            if not able:
                raise ValueError("precision='bf16': this kernel provider has no bf16 E-step")
            return True
        return self.precision is None and os.environ.get("SLIC_KMEANS_BF16", "0") == "1" and Dp <= 512 and able

    # ------------------------------------------------------------------ what a fit makes once and hands to its runs
    def _seed_rows(self, Xc, sizes, K):
        """what k-means++ reads -> (Xs, its k-permuted copy, its squared row norms): Xs is the centred matrix itself, or — sharded — the
        all-gathered one every rank seeds on (the provider's own images only where it uses_perm)"""
        _kpp_trials(K)                                                                  # raises before anything is launched
        k, ex = self.k, self._ex
        if ex is None:
            Xs = Xc
        elif int(sizes.min()) == int(sizes.max()):
            Xs = ex.gather(Xc).reshape(-1, Xc.shape[1]).contiguous()
        else:
            pad = torch.zeros(int(sizes.max()), Xc.shape[1], dtype=Xc.dtype, device=Xc.device)
            pad[: Xc.shape[0]] = Xc
            allp = ex.gather(pad)
            Xs = torch.cat([allp[r, : int(sizes[r])] for r in range(len(sizes))], 0).contiguous()
        if not k.uses_perm:
            return Xs, None, None
        Xsp = torch.empty_like(Xs)
        xn = torch.empty(Xs.shape[0], dtype=torch.float32, device=Xs.device)
        k.permute_k8(Xs, Xsp)
        k.cnorm(Xs, xn)
        return Xs, Xsp, xn

    def _estep_images(self, Xc, seed, bf16):
        """what every E-step of the fit reads -> (Xc, k-permuted copy, bf16 image, row norms, the bf16 counters); None where not used"""
        k = self.k
        Xp = Xb = xnb = bstats = None
        if k.uses_perm and seed is not None and seed[0] is Xc:
            Xp = seed[1]                                                                # the copy k-means++ already made
        elif k.uses_perm:
            Xp = torch.empty_like(Xc)
            k.permute_k8(Xc, Xp)
        if bf16:
            Xb, xnb = k.bf16_image(Xc, want_norms=True)
            bstats = torch.zeros(3, dtype=torch.int32, device=Xc.device)
        return Xc, Xp, Xb, xnb, bstats

    # ------------------------------------------------------------------ one Lloyd run
    def _lloyd_single(self, est, C, tol_abs):
        """_kmeans_single_lloyd with the host loop running ONE iteration behind the device: iteration it+1 is enqueued
        before iteration it's 4-double status word is read, so the read-back (and this Python) hide under the next
        E-step.  A speculatively launched iteration is simply ignored when the previous one turns out to have converged
        (it only reads the state it would need to keep: rings of 3 centre / label buffers, 2 partial-sum buffers)."""
        k, ex = self.k, self._ex
        Xc, Xp, Xb, xnb, bstats = est
        N, Dp = Xc.shape
        K = C.shape[0]
        dev = Xc.device
        on_gpu = Xc.is_cuda
        Cb = [C.contiguous().clone(), torch.empty_like(C), torch.empty_like(C)]          # iteration it: Cb[it%3] -> Cb[(it+1)%3]
        Lb = [torch.full((N,), -1, dtype=torch.int32, device=dev) for _ in range(3)]      # labels of iteration it: Lb[it%3]
        cnorm = [torch.empty(K, dtype=torch.float32, device=dev) for _ in range(3)]        # norms of Cb[i]: written by finalize
        Cp = [torch.empty_like(C) if k.uses_perm else None for _ in range(3)]              # permuted twins of Cb
        sph = dict(spherical=True) if self.spherical else {}
        n_changed = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2)]
        shift = torch.empty(K, dtype=torch.float32, device=dev)
        status = [torch.empty(4, dtype=torch.float64, device=dev) for _ in range(2)]
        host = [torch.empty(4, dtype=torch.float64).pin_memory() if on_gpu else torch.empty(4, dtype=torch.float64) for _ in range(2)]
        ev = [torch.cuda.Event() if on_gpu else None for _ in range(2)]
        done = [torch.cuda.Event() if on_gpu else None for _ in range(2)]
        side = self._side_stream(dev) if on_gpu else None
        # the E-step's precision, bound ONCE per run.  estep(Cin, Cpin, ...) is the fused step (unsharded) or the local half (sharded) with
        # the rows and their images in place; the bf16 forms take scratch for the centres' image where the fp32 forms take the permuted centres
        if Xb is None:
            estep = functools.partial(k.lloyd_step if ex is None else k.lloyd_local, Xc, Xp)
        else:
            step = k.lloyd_step_bf16 if ex is None else k.lloyd_local_bf16
            Cimg = torch.empty(K, Xb.shape[1], dtype=torch.int16, device=dev)              # the centres' image: rewritten every iteration

            def estep(Cin, Cpin, *a, **kw):
                step(Xc, Xp, Xb, xnb, Cin, Cimg, *a, bstats, **kw)

        def read_back(sl):
            if on_gpu:
                # the 32-byte status read-back goes through a side stream: on the compute stream the D2H copy and its
                # system-scope release would hold the next iteration's first kernel back by ~35 us
                done[sl].record()
                side.wait_event(done[sl])
                with torch.cuda.stream(side):
                    host[sl].copy_(status[sl], non_blocking=True)
                ev[sl].record(side)
            else:
                host[sl].copy_(status[sl])

        local_failure = []
        if ex is None:
            part = [torch.empty(K * Dp + K, dtype=torch.float32, device=dev) for _ in range(2)]   # [sums | counts]
            gsums = [p[: K * Dp] for p in part]
            gcounts = [p[K * Dp:] for p in part]
            sync = torch.cuda.Event.synchronize

            def launch(it):
                """enqueue iteration `it` (one fused call: E-step, M-step, averaging) and the async read-back of its status word"""
                sl = it & 1
                estep(Cb[it % 3], Cp[it % 3], cnorm[it % 3], Lb[it % 3], Lb[(it + 2) % 3], n_changed[sl], gsums[sl], gcounts[sl],
                      Cb[(it + 1) % 3], Cp[(it + 1) % 3], cnorm[(it + 1) % 3], shift, status[sl], **sph)
                read_back(sl)
        else:
            PL = K * Dp + K + 2                                          # [sums | counts | n_changed lo, hi]
            payload = [torch.empty(1, PL, dtype=ex.dtype, device=dev) for _ in range(2)]
            # reduced in place, or gathered into one row per rank
            parts = payload if ex.n_parts == 1 else [torch.empty(ex.n_parts, PL, dtype=ex.dtype, device=dev) for _ in range(2)]
            gsums = [torch.empty(K * Dp, dtype=torch.float32, device=dev) for _ in range(2)]
            gcounts = [torch.empty(K, dtype=torch.float32, device=dev) for _ in range(2)]
            sync = ex.sync

            def launch(it):
                """enqueue iteration `it` (local half, the ONE collective, global half) and the async read-back of its status word"""
                sl = it & 1
                # two foreign calls around the iteration's ONE collective.  A rank whose local half raises (an allocation that fails, a bad
                # argument) must still ENTER the collective, or its peers wait for it until the process group's timeout: it contributes a
                # POISONED payload — the n_changed high slot, which a healthy rank fills with < 2^11 — from then on, and raises the cause
                # where the loop reads that iteration's status; its peers see the poison in the same status word and raise there too.
                if not local_failure:
                    try:
                        estep(Cb[it % 3], Cp[it % 3], cnorm[it % 3], Lb[it % 3], Lb[(it + 2) % 3], payload[sl])
                    except Exception as e:                              # noqa: BLE001 — re-raised by read() of this iteration
                        local_failure.append((it, e))
                if local_failure:
                    payload[sl].zero_()
                    payload[sl].view(-1)[-1] = _POISON
                ex.reduce(payload[sl], parts[sl])
                if local_failure:
                    return          # no global half, no read-back: read() of the failed iteration raises (the loop runs one launch ahead of
                                    # its reads, so this rank keeps entering the collectives its peers enter until they all get there)
                k.lloyd_global(parts[sl], Cb[it % 3], gsums[sl], gcounts[sl], Cb[(it + 1) % 3], Cp[(it + 1) % 3], cnorm[(it + 1) % 3], shift,
                               status[sl], **sph)
                read_back(sl)

        def read(it):
            if local_failure and local_failure[0][0] <= it:
                raise local_failure[0][1]
            if on_gpu:
                sync(ev[it & 1])                                            # bounded where the exchange is the library's own
            st = host[it & 1].tolist()
            if ex is not None and st[2] >= _POISON:                     # n_changed = low + 2^20 * high: a peer's poisoned high slot
                raise _lib.SlicError("sharded k-means: a peer's local half of the Lloyd iteration failed (it raised the cause); "
                                     "every rank leaves the fit here instead of waiting in the next collective")
            return st

        trace = [] if self.trace else None
        strict = False
        n_reloc = 0
        it = 0
        if on_gpu:
            torch.cuda.synchronize(dev)
        t_loop = time.time()                                               # the Lloyd phase proper (SURVEY.md §8d metric 2)
        if self.max_iter > 0:
            k.cnorm(Cb[0], cnorm[0])                                       # later norms / permuted centres come out of the iterations
            if k.uses_perm:
                k.permute_k8(Cb[0], Cp[0])
            launch(0)
        while it < self.max_iter:
            speculated = it + 1 < self.max_iter
            if speculated:
                launch(it + 1)
            shift_tot, n_empty, n_chg, _ = read(it)
            if n_empty > 0:
                # rare: _relocate_empty_clusters_dense on iteration it's sums, then redo its averaging — and the
                # speculative iteration, which ran on the un-relocated centres
                sl = it & 1
                if self._relocate(Xc, Cb[it % 3], Lb[it % 3], gsums[sl], gcounts[sl], int(n_empty)):
                    n_reloc += 1
                    k.finalize(Cb[it % 3], gsums[sl], gcounts[sl], Cb[(it + 1) % 3], shift, n_changed[sl], status[sl],
                               cnorm[(it + 1) % 3], Cp[(it + 1) % 3], **sph)
                    shift_tot = status[sl].cpu().tolist()[0]
                    if speculated:
                        launch(it + 1)
            if trace is not None:
                trace.append(Lb[it % 3].cpu().numpy().copy())
            if not self.fixed_iters:
                if n_chg == 0:                                         # np.array_equal(labels, labels_old)
                    strict = True
                    break
                if shift_tot <= tol_abs:
                    break
            it += 1
        n_iter = min(it + 1, self.max_iter)
        if on_gpu:
            torch.cuda.synchronize(dev)
        self.lloyd_seconds_, self.lloyd_iters_ = time.time() - t_loop, n_iter      # assign + update + convergence test
        last = n_iter - 1                                              # last executed (and kept) iteration
        C = Cb[(last + 1) % 3] if self.max_iter > 0 else Cb[0]
        labels = Lb[last % 3] if self.max_iter > 0 else Lb[0]
        if not strict:
            # rerun the E-step so labels match the final centres (_kmeans.py:736-748); any buffer but `C`'s reader state
            out = Lb[(last + 1) % 3]
            cn = cnorm[(last + 1) % 3] if self.max_iter > 0 else cnorm[0]
            if self.max_iter <= 0:
                k.cnorm(C, cn)
            if Xb is not None:
                k.assign_bf16(Xc, Xb, xnb, C, k.bf16_image(C)[0], cn, out, None, None, bstats)
            elif k.uses_perm and self.max_iter > 0:
                k.assign_perm(Xp, Cp[(last + 1) % 3], cn, out, None, None)
            else:
                k.assign(Xc, C, cn, out, None, None)
            labels = out
        inertia = self._inertia(Xc, C, labels)
        res = dict(labels=labels, centers=C, inertia=inertia, n_iter=n_iter, strict=strict, n_relocations=n_reloc)
        if trace is not None:
            res["trace"] = np.stack(trace) if trace else np.zeros((0, N), np.int32)
        return res

    def _side_stream(self, dev):
        if self._side is None:
            self._side = torch.cuda.Stream(device=dev)
        return self._side

    def _inertia(self, Xc, C, labels):
        N = Xc.shape[0]
        dist = torch.empty(N, dtype=torch.float32, device=Xc.device)
        out = torch.empty(1, dtype=torch.float64, device=Xc.device)
        self.k.dist_to_assigned(Xc, C, labels, dist)
        self.k.sum_f64(dist, out)
        return float(self._rank_sum(out)[0])

    def _relocate(self, Xc, C_old, labels, gsums, gcounts, n_empty):
        """_relocate_empty_clusters_dense (_k_means_common.pyx:167-211).  Returns False when max(dist) == 0."""
        k, ex = self.k, self._ex
        N, Dp = Xc.shape
        dev = Xc.device
        n_sel = n_empty
        dist = torch.empty(N, dtype=torch.float32, device=dev)
        k.dist_to_assigned(Xc, C_old, labels, dist)
        far_idx = torch.empty(n_sel, dtype=torch.int32, device=dev)
        far_dist = torch.empty(n_sel, dtype=torch.float32, device=dev)
        k.select_far(dist, n_sel, far_idx, far_dist)
        fi = far_idx.long()
        valid = fi < N                                   # a shard smaller than n_empty runs out of rows
        fi = fi.clamp(max=N - 1)
        xfar = Xc.index_select(0, fi)
        old_ids = labels.index_select(0, fi)
        fd = torch.where(valid, far_dist, torch.full_like(far_dist, -1.0))
        if ex is not None:
            # merge the per-rank candidates by (dist desc, global row asc), keep n_empty
            gidx = fi + self._row0
            fdh = ex.gather(fd).reshape(-1).cpu().numpy()
            gih = ex.gather(gidx).reshape(-1).cpu().numpy()
            allx = ex.gather(xfar).reshape(-1, Dp)
            allold = ex.gather(old_ids).reshape(-1)
            order = np.lexsort((gih, -fdh))[:n_empty]
            order = order[fdh[order] >= 0]
            sel = torch.from_numpy(order).to(dev)
            xfar = allx.index_select(0, sel).contiguous()
            old_ids = allold.index_select(0, sel).contiguous()
            fdh = fdh[order]
        else:
            fdh = fd.cpu().numpy()
        if len(fdh) == 0 or fdh[0] == 0.0:
            return False
        empty = np.nonzero(gcounts.cpu().numpy() == 0)[0].astype(np.int32)[: len(fdh)]
        new_ids = torch.from_numpy(empty).to(dev)
        k.apply_relocation(xfar[: len(empty)].contiguous(), old_ids[: len(empty)].contiguous(), new_ids, gsums, gcounts)
        return True

    # ------------------------------------------------------------------ k-means++
    def _kmeans_plusplus(self, seed, K, R):
        """_kmeans_plusplus (_kmeans.py:174-277) for the R runs of the n_init loop, as a generator: run r's initial centres (rows of
        the centred matrix) are made when run r asks for them.  RNG draws on the host from numpy's legacy RandomState (as sklearn):
        per run the first row, then (K - 1) x T uniforms, all from ONE stream.  They do not depend on the data and Lloyd draws nothing,
        so a run's draws are made up front and its K - 1 steps (distances, potentials, cumsum-search) run back to back on the device
        (kpp_run) — or, where the lock-step kernel applies, the draws of ALL runs are made in that order at the first request and the
        R seedings take each step as one pass over X (kpp_run_batch).  In sharded runs every rank seeds on the all-gathered matrix
        and follows rank 0's draws (identical centres everywhere)."""
        k, ex = self.k, self._ex
        Xs, Xsp, xn = seed
        N = Xs.shape[0]
        dev = Xs.device
        rs = self._rng()
        T = _kpp_trials(K)

        def draw():
            first = np.array([rs.choice(N, p=np.full(N, 1.0 / N))], np.int64)
            u = rs.uniform(size=(K - 1, T)) if K > 1 else np.zeros((0, T))
            return (int(first[0]), u) if ex is None else (int(ex.bcast(first, dev)[0]), ex.bcast(u, dev) if K > 1 else u)

        def on_device(u):
            return torch.from_numpy(np.ascontiguousarray(u, dtype=np.float64)).to(dev)

        lockstep = (R > 1 and ex is None and k.kpp_run_batch is not None and R * T <= 160 and N * Xs.stride(0) * 4 < (1 << 31)
                    and os.environ.get("SLIC_KPP_BATCH", "1") != "0")
        if lockstep:
            draws = [draw() for _ in range(R)]
            idx_d = torch.empty(R, K, dtype=torch.int32, device=dev)
            k.kpp_run_batch(Xsp, xn, [f for f, _ in draws], K, T, on_device(np.stack([u for _, u in draws], 0)), idx_d)
            ih = idx_d.cpu().numpy().astype(np.int64)
        for r in range(R):
            if lockstep:
                idx, picks = idx_d[r], ih[r]
            else:
                first, u = draw()
                idx = torch.empty(K, dtype=torch.int32, device=dev)
                k.kpp_run(Xs, first, K, T, on_device(u), idx, Xsp, xn)
                picks = idx.cpu().numpy().astype(np.int64)
            self.init_indices_ = picks
            self.init_indices_log_.append(picks)                    # every run's picks
            yield Xs.index_select(0, idx.long()).contiguous()

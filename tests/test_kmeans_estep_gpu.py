"""GPU: the k-means E-step entry points of csrc/kmeans.hip called directly through the C ABI, bit for bit against the compiled
oracle (oracle/kmeans.py), at the shapes where the kernels and the combine pass change form.

Entry points: slic_kmeans_assign (km_assign_partial<4>), slic_kmeans_assign_perm (km_assign_dma<128, 2, 1, 2> or
km_assign_creg<4 | 8 | 16, 4>, told apart by slic_kmeans_assign_perm_plan), slic_kmeans_lloyd_step and slic_kmeans_lloyd_local
(the same E-step with the M-step's histogram: km_combine<true>, or km_combine<false> + km_block_hist), and their workspace
queries slic_kmeans_assign_workspace_bytes / slic_kmeans_lloyd_local_workspace_bytes.

The checks are functions of a backend: `Device` (test_kmeans_kernels_gpu) calls the library; tests/test_kmeans_estep_cpu.py runs
the same functions with the NumPy mirror (tests/kmeans_estep_ref.py), unmutated and with one defect at a time.  Importing this
module does not touch the device.

Hygiene as in test_kmeans_kernels_gpu: labels start as -7 and scores as NaN in front of a 4096-byte guard tail, workspaces have the
library's own size plus a guard, strided operands carry NaN in every padding column and offset, every call runs twice into fresh
outputs that must be bit-equal.  *n_changed starts at 12345 for the two assign entries (they add to it) and at poison for
lloyd_step / lloyd_local (they zero it themselves).

Every gate is bit equality with the oracle: labels, winning scores where requested, n_changed, payload sums / counts, and
everything check_step_outputs checks.  Nothing here has a tolerance.

The register route is reached at small N through a large K: ncb = cus / 2 (or cus / 3) centroid blocks leave two (three) point
slices, and the kernel is taken from about 1.5 * 128 * slices rows.  The N values come from a search over the mirror's slice walk
driven by the plan's slice count; COVER collects what ran and test_coverage asserts it (a form the device's CU count cannot reach
is a named skip)."""
import functools

import numpy as np
import pytest

import kmeans_estep_ref as E
from oracle import kmeans as ok
from test_kmeans_kernels_gpu import Device, bits_equal, case, check_step_outputs, exact, pad, twice, CASES

pytestmark = pytest.mark.gpu
F32, F64, I32 = np.float32, np.float64, np.int32
NCH0 = 12345
COVER = set()
UNREACHABLE = {}

NAT_CASES = ((1, 1, 8), (31, 31, 24), (32, 32, 32), (33, 33, 40), (127, 127, 136), (128, 128, 8), (129, 129, 40), (300, 257, 24),
             (300, 641, 32), (129, 641, 8), (1, 641, 136), (300, 1, 8))                               # lists of 128: G = 1, 2, 3, 6
DMA_CASES = ((1, 1, 8), (31, 63, 40), (32, 64, 512), (33, 65, 520), (127, 257, 1032), (128, 320, 8), (129, 321, 40),
             (300, 513, 512), (300, 257, 8), (129, 513, 1032), (300, 320, 520))                       # lists of 64: G = 1, 1, 1, 2, 5, 5, 6, 9
CREG_DS = {8: 4, 104: 4, 136: 8, 256: 8, 264: 16, 512: 16}                                            # D -> k-tiles per point tile
CREG_SEARCHED = (8, 136, 264)                                                                         # the N search; the others run its first N
WORKLOAD = (12288 + 77, 500, 512)
OLD_KINDS = (None, "all", "some", "same")
STEP_HIST = ((1500, 8, 12288), (1500, 8, 12289))      # K * 4 = 48 KiB: km_combine<true>; one more: km_combine<false> + km_block_hist
LOCAL_NS = (1, 1023, 1024, 1025, 2049)
LOCAL_SLAB_N = 32769                                  # above KM_SCAN_MAXN: the slab route whatever SLIC_KM_SCAN says
LOCAL_K, LOCAL_D = 250, 8


def f32(a):
    return np.ascontiguousarray(a, dtype=F32)


def frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def problem(N, K, D, seed=0):
    """rows near centres, two of them near the LAST centre (the one centroid of the last list when K = 64 m + 1 or 128 m + 1), one
    all-zero row (every score positive: only a padding centroid scoring 0 could beat them) and centre 0 moved away so that it is
    not that row's answer; with the oracle's labels and winning scores"""
    rng = np.random.default_rng(1000003 * seed + 7919 * N + 31 * K + D)
    C = f32(rng.standard_normal((K, D)))
    X = f32(C[rng.integers(0, K, N)] + 0.3 * rng.standard_normal((N, D)))
    if N >= 3 and K >= 3:
        C[0] *= 3.0
        X[N // 2] = 0.0
        X[[1, N - 1]] = C[K - 1] + F32(0.05) * X[[1, N - 1]]
    lab, best, _ = ok.assign(X, C, with_scores=True)
    return frozen(X, C, lab, best)


def old_labels(kind, lab, seed):
    if kind is None:
        return None
    if kind == "all":
        return (lab + 1).astype(I32)
    if kind == "same":
        return lab.copy()
    rng = np.random.default_rng(seed)
    return np.where(rng.random(len(lab)) < 0.3, lab + 1, lab).astype(I32)


def see_plan(be, N, K, D, ldx, expect):
    """the plan of a permuted-layout call: asserted against `expect` ('dma' | 'creg' | None), recorded in COVER"""
    p = be.estep_plan(N, K, D, ldx)
    route, nk, slices, cblocks, G, cus = p
    assert cus > 0 and G == cblocks and route in (0, 1), p
    if expect is not None:
        assert route == (1 if expect == "creg" else 0), (expect, p, (N, K, D, ldx))
    if route:
        assert nk == CREG_DS.get(D, nk) and slices >= 1 and cblocks == -(-K // 128), p
        COVER.add(("creg", nk))
        for f in E.walk_forms(N, slices):
            COVER.add(("creg", nk) + (f if isinstance(f, tuple) else (f,)))
    else:
        assert nk == 0 and slices == 0 and cblocks == -(-K // 64), p
        COVER.add(("dma",))
    COVER.add(("lists", "perm", G))
    return p


def run_assign(be, entry, X, C, ldx=None, ldc=None, xoff=0, coff=0, labels_old=None, want_score=True, ldxp=None):
    D = X.shape[1]
    Xb, Cb = pad(X, ldx or D, xoff), pad(C, ldc or D, coff)
    if entry == "natural":
        return twice(lambda: be.estep_assign(Xb, D, Cb, xoff, coff, labels_old, NCH0, want_score))
    return twice(lambda: be.estep_assign_perm(Xb, D, Cb, xoff, coff, labels_old, NCH0, want_score, ldxp))


def gate_assign(name, got, lab, best, labels_old, want_score, what, skip_score=()):
    labels, nch, score = got
    exact(name + ".labels", labels, lab, what)
    e_nch = NCH0 + (0 if labels_old is None else int((lab != labels_old).sum()))
    assert nch == e_nch, (name, what, "n_changed", nch, e_nch)
    if want_score:
        keep = np.setdiff1d(np.arange(len(lab)), np.asarray(skip_score, np.int64))
        exact(name + ".best_score", score[keep], best[keep], what)
    else:
        assert score is None


def check_assign(be, entry, N, K, D, expect=None, old="some", want_score=True, **operands):
    """one shape of slic_kmeans_assign ('natural') or slic_kmeans_assign_perm ('perm') against the oracle"""
    case("estep." + entry)
    X, C, lab, best = problem(N, K, D)
    if entry == "perm":
        see_plan(be, N, K, D, operands.get("ldxp") or operands.get("ldx") or D, expect)
    else:
        COVER.add(("natural",))
        COVER.add(("lists", "natural", -(-K // 128)))
    lo = old_labels(old, lab, N + K)
    what = (entry, N, K, D, old, want_score, tuple(sorted(operands.items())))
    gate_assign("assign." + entry, run_assign(be, entry, X, C, labels_old=lo, want_score=want_score, **operands), lab, best, lo,
                want_score, what)


# ------------------------------------------------------------------ the register route at small N
def creg_k(cus, div):
    """just below 128 * (cus / div) centroids: cus / div blocks, inside the 1/8 padding rule"""
    return 128 * (cus // div) - 3


def creg_shapes(be, D, ldx=None, searched=True):
    """(N, K) that the plan sends to the register kernel, chosen so that together they walk every form this CU count reaches:
    npt_last 1 .. 4, a slice of one tile, of several, whole and ragged last sub-tiles.  Two slices (cus / 2 blocks) reach them all
    on an even CU count; the three-slice shapes (cus / 3 blocks) add their own walks for D = 8."""
    cus = be.estep_plan(1024, 500, 8, 8)[5]
    out, seen = [], set()
    for div in (2, 3) if (searched and D == 8) else (2,):
        if cus // div < 1:
            continue
        K = creg_k(cus, div)
        for subs in range(6, 40):
            for N in (subs * 32 - 5, subs * 32):
                p = be.estep_plan(N, K, D, ldx or D)
                if p[0] != 1:
                    continue
                new = {(div, f) for f in E.walk_forms(N, p[2])} - seen
                if new:
                    out.append((N, K))
                    seen |= new
                    if not searched:
                        return out
    return out


def check_creg(be, D):
    shapes = creg_shapes(be, D, searched=D in CREG_SEARCHED)
    if not shapes:
        UNREACHABLE[("creg", CREG_DS[D], D)] = "no shape below 40 sub-tiles takes the register kernel on this CU count"
    for N, K in shapes:
        check_assign(be, "perm", N, K, D, expect="creg", old="some")
    return shapes


def check_workload(be):
    """the shape of the bench row's E-step, on whichever route this device's plan gives it"""
    N, K, D = WORKLOAD
    check_assign(be, "perm", N, K, D, expect=None, old="some", want_score=True)


# ------------------------------------------------------------------ ties
def tie_pairs(width):
    """(j1, j2 = a copy of j1): two slots of one lane; the two lane halves; two tiles / waves; + 64; + 128; lists 0 and 4 (on both
    sides of km_combine's first group of four); lists 3 and 5 (inside the group and in the tail when G = 6)"""
    return ((1, 2), (8, 12), (16, 48), (5, 69), (24, 152), (40, 4 * width + 40), (3 * width + 7, 5 * width + 7))


@functools.lru_cache(maxsize=None)
def tie_problem(N, K, D, width):
    rng = np.random.default_rng(77 + K + D)
    C = f32(rng.standard_normal((K, D)))
    pairs = tie_pairs(width)
    assert K > max(j2 for _, j2 in pairs) and len({j for p in pairs for j in p}) == 2 * len(pairs)
    for j1, j2 in pairs:
        C[j2] = C[j1]
    per = 16
    assert N >= per * len(pairs)
    X = f32(C[rng.integers(0, K, N)] + 0.3 * rng.standard_normal((N, D)))
    rows = rng.permutation(N)[:per * len(pairs)].reshape(len(pairs), per)        # spread over the tiles and slices
    for (j1, _), r in zip(pairs, rows):
        X[r] = C[j1] + F32(1e-3) * f32(rng.standard_normal((per, D)))
    lab, best, _ = ok.assign(X, C, with_scores=True)
    for (j1, j2), r in zip(pairs, rows):                # on the CPU first: the oracle gives these rows the LOWER copy
        assert (lab[r] == j1).sum() >= 8 and not (lab == j2).any(), (j1, j2, lab[r])
    return frozen(X, C, lab, best)


def check_ties(be, entry, N, K, D, expect=None):
    case("estep.ties")
    width = 64 if expect == "dma" else 128
    X, C, lab, best = tie_problem(N, K, D, width)
    if entry == "perm":
        see_plan(be, N, K, D, D, expect)
    got = run_assign(be, entry, X, C)
    for _, j2 in tie_pairs(width):
        assert not (got[0] == j2).any(), ("the upper copy of a duplicated centroid won", entry, expect, j2, np.flatnonzero(got[0] == j2)[:4])
    gate_assign("ties." + entry, got, lab, best, None, True, (entry, N, K, D))


def check_ties_creg(be):
    shapes = creg_shapes(be, 8, searched=False)
    if not shapes:
        UNREACHABLE[("ties", "creg")] = "no shape takes the register kernel on this CU count"
        return
    N, K = shapes[0]
    check_ties(be, "perm", max(N, 300), K, 8, "creg")


# ------------------------------------------------------------------ operands
def check_operands(be, entry, N, K, D, expect=None):
    """row strides above D with a column offset on both operands (NaN around them), best_score given and NULL, the four kinds of
    labels_old; for the permuted entry also X permuted on the device into rows ldxp > D apart"""
    for i, old in enumerate(OLD_KINDS):
        for want in ((True, False) if old in (None, "some") else (bool(i % 2),)):
            check_assign(be, entry, N, K, D, expect=expect, old=old, want_score=want, ldx=D + 8, ldc=D + 4, xoff=4, coff=4)
    check_assign(be, entry, N, K, D, expect=expect, old="some", want_score=True)                      # dense again, same problem
    if entry == "perm":
        check_assign(be, entry, N, K, D, expect=expect, old="some", want_score=True, ldx=D + 8, ldc=D + 4, xoff=4, coff=4, ldxp=D + 12)


def check_estep_argument_rules(lib, have_device):
    """every host rule of the four E-step entry points and of the plan query returns non-zero and names its entry point in
    slic_last_error; every call is refused before any launch, so this runs without a device too.  Returns the number of refusals."""
    import ctypes
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    odd = ctypes.c_void_p(p.value + 4)
    LONG = 1 << 22                                      # 128 rows of 2^22 floats: 2^31 bytes, past a buffer resource
    n = 0

    def refused(name, args, say=None, **kw):
        nonlocal n
        a = list(args)
        for k, v in kw.items():
            a[int(k[1:])] = v
        n += 1
        assert getattr(lib, name)(*a, None) != 0, (name, a)
        assert (say or name).encode() in lib.slic_last_error(), (name, lib.slic_last_error())

    # X, N, D, ldx, C, K, ldc, cnorm, labels, labels_old, n_changed, best_score, workspace
    assign = [p, 4, 8, 8, p, 3, 8, p, p, None, None, None, p]
    for name in ("slic_kmeans_assign", "slic_kmeans_assign_perm"):
        for i in (0, 4, 7, 8, 12):
            refused(name, assign, **{f"a{i}": None})
        for i in (1, 2, 5):
            refused(name, assign, **{f"a{i}": 0})                                               # an empty problem
        refused(name, assign, a2=12, a3=12, a6=12)                                            # D % 8
        refused(name, assign, a3=4)                                                           # ldx < D
        refused(name, assign, a6=4)                                                           # ldc < D
        refused(name, assign, a3=10)                                                          # rows not 16-byte aligned
        refused(name, assign, a6=10)
        refused(name, assign, a0=odd)
        refused(name, assign, a4=odd)
        refused(name, assign, a9=p)                                                           # labels_old without n_changed
    refused("slic_kmeans_assign_perm", assign, a3=LONG)
    refused("slic_kmeans_assign_perm", assign, a6=LONG)
    # X, Xp, N, D, ldx, C_old, Cp_old, cnorm_old, K, labels, labels_old, n_changed, sums, counts, C_new, Cp_new, cnorm_new, shift,
    # spherical, status, workspace
    q, r = ctypes.c_void_p(p.value + 128), ctypes.c_void_p(p.value + 256)
    step = [p, p, 4, 8, 8, p, p, p, 3, p, None, p, q, p, r, p, p, p, 0, p, p]
    for i in (2, 8):
        refused("slic_kmeans_lloyd_step", step, say="slic_kmeans_assign_perm", **{f"a{i}": 0})
    refused("slic_kmeans_lloyd_step", step, say="slic_kmeans_assign_perm", a4=4)
    refused("slic_kmeans_lloyd_step", step, a11=None)                                         # n_changed is not optional here
    refused("slic_kmeans_lloyd_step", step, a3=12, a4=12)
    # X, Xp, N, D, ldx, Cp_old, cnorm_old, K, labels, labels_old, payload, payload_f64, workspace
    local = [p, p, 4, 8, 8, p, p, 3, p, None, p, 0, p]
    for i in (0, 1, 5, 6, 8, 10, 12):
        refused("slic_kmeans_lloyd_local", local, **{f"a{i}": None})
    for i in (2, 3, 7):
        refused("slic_kmeans_lloyd_local", local, say="slic_kmeans_assign_perm", **{f"a{i}": 0})
    refused("slic_kmeans_lloyd_local", local, say="slic_kmeans_assign_perm", a3=12, a4=12)
    refused("slic_kmeans_lloyd_local", local, say="slic_kmeans_assign_perm", a4=4)
    refused("slic_kmeans_lloyd_local", local, say="slic_kmeans_assign_perm", a4=LONG)
    # the plan query: N, K, D, ldx, out  (no stream argument)
    out = (ctypes.c_int * 6)(*[-7] * 6)
    plan = lib.slic_kmeans_assign_perm_plan
    for a in ((4, 3, 8, 8, None), (0, 3, 8, 8, out), (4, 0, 8, 8, out), (4, 3, 0, 8, out), (4, 3, 12, 12, out), (4, 3, 8, 4, out),
              (4, 3, 8, 10, out), (4, 3, 8, LONG, out)):
        n += 1
        assert plan(*a) != 0 and b"slic_kmeans_assign_perm_plan" in lib.slic_last_error(), a
    assert list(out) == [-7] * 6                        # a refused query writes nothing
    rc = plan(4, 3, 8, 8, out)
    if have_device:
        assert rc == 0 and out[0] == 0 and out[3] == 1 and out[4] == 1 and out[5] > 0, list(out)
    else:                                               # the CU count is part of the answer: no device, no answer
        assert rc != 0 and b"slic_kmeans_assign_perm_plan" in lib.slic_last_error() and list(out) == [-7] * 6
        n += 1
    return n


def check_operands_creg(be):
    shapes = creg_shapes(be, 8, ldx=16, searched=False)
    if not shapes:
        UNREACHABLE[("operands", "creg")] = "no shape takes the register kernel on this CU count"
        return
    N, K = shapes[0]
    for old, want in (("some", True), (None, False), ("same", False)):
        check_assign(be, "perm", N, K, 8, expect="creg", old=old, want_score=want, ldx=16, ldc=12, xoff=4, coff=4)


# ------------------------------------------------------------------ NaN rows
@functools.lru_cache(maxsize=None)
def nan_problem(N, K, D, rows):
    """three rows with one NaN (every score NaN) and one with +inf in a column where every centre is negative (every score +inf):
    none of their scores compares below +inf, so their label is 0; all other rows keep the labels of the clean problem"""
    X0, C0, _, _ = problem(N, K, D, seed=5)
    X, C = X0.copy(), C0.copy()
    col = D - 3
    C[:, col] = -np.abs(C[:, col]) - F32(0.01)
    lab, best, _ = ok.assign(X, C, with_scores=True)
    cols = (0, D // 2 + 1, D - 1)
    for r, c in zip(rows[:3], cols):
        X[r, c] = np.nan
    X[rows[3], col] = np.inf
    lab = lab.copy()
    lab[list(rows)] = 0
    with np.errstate(invalid="ignore", over="ignore"):
        assert np.array_equal(ok.assign(X, C), lab)      # the oracle itself: 0 there, nothing else moved
    assert (np.delete(lab, list(rows)) != 0).sum() > N // 2
    return frozen(X, C, lab, best)


def check_nan_rows(be, entry, N, K, D, expect=None, slices=1):
    case("estep.nan")
    # rows in different sub-tiles of the first tile, in a later tile, and (register route) in every slice's range
    rows = tuple(sorted({3, 40, min(N - 1, 128 + 70), N - 2}))
    if expect == "creg":
        w = E.slice_walk(N, slices)
        rows = tuple(sorted({w[0]["pbeg"] + 3, w[0]["pbeg"] + 40, w[-1]["pbeg"] + 1, w[-1]["pend"] - 2}))
    assert len(rows) == 4
    X, C, lab, best = nan_problem(N, K, D, rows)
    lo = old_labels("some", lab, 3)
    got = run_assign(be, entry, X, C, labels_old=lo)
    gate_assign("nan." + entry, got, lab, best, lo, True, (entry, N, K, D, rows), skip_score=rows)


def check_nan_rows_creg(be):
    shapes = creg_shapes(be, 8, searched=False)
    if not shapes:
        UNREACHABLE[("nan", "creg")] = "no shape takes the register kernel on this CU count"
        return
    N, K = shapes[0]
    p = see_plan(be, N, K, 8, 8, "creg")
    check_nan_rows(be, "perm", N, K, 8, "creg", p[2])


# ------------------------------------------------------------------ the histogram forms
@functools.lru_cache(maxsize=None)
def hist_problem(N, D, K):
    """mostly empty clusters when K > N; labels_old differs on about 30 % of the rows"""
    rng = np.random.default_rng(N + K)
    C = f32(rng.standard_normal((K, D)))
    X = f32(C[rng.integers(0, K, N)] + 0.3 * rng.standard_normal((N, D)))
    lab = ok.assign(X, C)
    sums, counts = ok.accumulate(X, lab, K)
    return frozen(X, C, lab, old_labels("some", lab, N), sums, counts)


def check_step_hist(be, N, D, K):
    """slic_kmeans_lloyd_step on the two sides of the 48 KiB switch of the combine pass"""
    case("estep.lloyd_step")
    X, C, lab, lo, sums, counts = hist_problem(N, D, K)
    see_plan(be, N, K, D, D, None)
    COVER.add(("hist", "combine" if K * 4 <= 48 * 1024 else "block_hist"))
    for old in (lo, None):
        what = (N, D, K, "labels_old" if old is not None else "NULL")
        got = twice(lambda: be.lloyd_step(X, C, old))
        exact("step_hist.labels", got[0], lab, what)
        assert got[1] == (0 if old is None else int((lab != old).sum())), (what, got[1])
        exact("step_hist.sums", got[2], sums, what)
        exact("step_hist.counts", got[3], counts, what)
        check_step_outputs("step_hist", got, X, C, old, 0, what)


def check_local(be, env, N, scan, f64):
    """slic_kmeans_lloyd_local: the payload against ok.accumulate of the oracle's labels; SLIC_KM_SCAN=0 (read per call) sends a
    small shard through the histogram slab, N > 32768 goes there by itself"""
    case("estep.lloyd_local")
    if scan is None:
        env.delenv("SLIC_KM_SCAN", raising=False)
    else:
        env.setenv("SLIC_KM_SCAN", scan)
    X, C, lab, lo, sums, counts = hist_problem(N, LOCAL_D, LOCAL_K)
    see_plan(be, N, LOCAL_K, LOCAL_D, LOCAL_D, None)
    COVER.add(("hist", "slab" if (scan == "0" or N > 32768) else "none", "ragged" if N % 1024 else "whole"))
    dt = F64 if f64 else F32
    for old in (lo, None):
        what = (N, scan, f64, "labels_old" if old is not None else "NULL")
        labels, s, c, pair = twice(lambda: be.lloyd_local(X, C, old, f64))
        exact("local.labels", labels, lab, what)
        assert s.dtype == dt and c.dtype == dt and pair.dtype == dt
        exact("local.sums", s, sums.astype(dt), what)
        exact("local.counts", c, counts.astype(dt), what)
        n = 0 if old is None else int((lab != old).sum())
        exact("local.n_changed", pair, np.array([n & 0xFFFFF, n >> 20], dt), what)


# ------------------------------------------------------------------ every case, for either backend
def all_checks(be, env):
    for N, K, D in NAT_CASES:
        check_assign(be, "natural", N, K, D)
    for N, K, D in DMA_CASES:
        check_assign(be, "perm", N, K, D, expect="dma")
    for D in CREG_DS:
        check_creg(be, D)
    check_workload(be)
    check_ties(be, "natural", 300, 700, 8)
    check_ties(be, "perm", 300, 400, 8, "dma")
    check_ties_creg(be)
    check_operands(be, "natural", 300, 257, 40)
    check_operands(be, "perm", 300, 257, 40, "dma")
    check_operands_creg(be)
    check_nan_rows(be, "natural", 300, 257, 40)
    check_nan_rows(be, "perm", 300, 257, 40, "dma")
    check_nan_rows_creg(be)
    for N, D, K in STEP_HIST:
        check_step_hist(be, N, D, K)
    for f64 in (False, True):
        for N in LOCAL_NS:
            check_local(be, env, N, "0", f64)
        check_local(be, env, LOCAL_SLAB_N, None, f64)


def required_cover():
    """what a run of all_checks must have reached (the register route's entries can be excused by UNREACHABLE, by name)"""
    req = {("natural",), ("dma",), ("hist", "combine"), ("hist", "block_hist"), ("hist", "slab", "ragged"), ("hist", "slab", "whole")}
    req |= {("lists", "natural", g) for g in (1, 2, 3, 6)} | {("lists", "perm", g) for g in (1, 2, 5, 6, 9)}
    for nk in (4, 8, 16):
        req |= {("creg", nk)} | {("creg", nk, "npt_last", v) for v in (1, 2, 3, 4)}
        req |= {("creg", nk, f) for f in ("one_tile", "several_tiles", "ragged_subtile")}
    return req


def coverage_report():
    """(missing forms, printable summary)"""
    missing = sorted(required_cover() - COVER, key=str)
    routes = sorted({c[:2] for c in COVER if c[0] in ("natural", "dma", "creg")}, key=str)
    npt = sorted({(c[1], c[3]) for c in COVER if c[0] == "creg" and len(c) == 4 and c[2] == "npt_last"})
    walks = sorted({c[2] for c in COVER if c[0] == "creg" and len(c) == 3})
    lists = sorted({c[1:] for c in COVER if c[0] == "lists"})
    hist = sorted({c[1:] for c in COVER if c[0] == "hist"})
    text = (f"coverage: routes x k-tiles {routes}; (k-tiles, npt_last) {npt}; slice walks {walks}; lists {lists}; histogram forms {hist}; "
            f"cases {dict((k, v) for k, v in CASES.items() if k.startswith('estep'))}; unreachable {UNREACHABLE}")
    return missing, text


# ------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def dev(gpu):
    return Device(gpu)


@pytest.mark.parametrize("N,K,D", NAT_CASES)
def test_assign_natural(dev, N, K, D):
    check_assign(dev, "natural", N, K, D)


@pytest.mark.parametrize("N,K,D", DMA_CASES)
def test_assign_perm_dma_tile(dev, N, K, D):
    check_assign(dev, "perm", N, K, D, expect="dma")


@pytest.mark.parametrize("D", list(CREG_DS))
def test_assign_perm_centroids_in_registers(dev, D):
    shapes = check_creg(dev, D)
    print("register route, D =", D, "(N, K):", shapes)


def test_assign_perm_workload_shape(dev):
    check_workload(dev)


def test_ties_take_the_lower_copy(dev):
    check_ties(dev, "natural", 300, 700, 8)
    check_ties(dev, "perm", 300, 400, 8, "dma")
    check_ties_creg(dev)


def test_operands(dev):
    check_operands(dev, "natural", 300, 257, 40)
    check_operands(dev, "perm", 300, 257, 40, "dma")
    check_operands_creg(dev)


def test_nan_rows_get_label_zero(dev):
    check_nan_rows(dev, "natural", 300, 257, 40)
    check_nan_rows(dev, "perm", 300, 257, 40, "dma")
    check_nan_rows_creg(dev)


@pytest.mark.parametrize("N,D,K", STEP_HIST)
def test_lloyd_step_histogram_forms(dev, N, D, K):
    check_step_hist(dev, N, D, K)


@pytest.mark.parametrize("f64", (False, True), ids=("fp32", "fp64"))
def test_lloyd_local_histogram_forms(dev, monkeypatch, f64):
    for N in LOCAL_NS:
        check_local(dev, monkeypatch, N, "0", f64)
    check_local(dev, monkeypatch, LOCAL_SLAB_N, None, f64)


def reachable_walk_forms(cus, D):
    """the forms of the slice walk that SOME N below 200 sub-tiles reaches on the register route with this CU count (the plan's
    rule restated in kmeans_estep_ref.plan), whatever the search of creg_shapes found"""
    forms = set()
    for div in (2, 3):
        if cus // div < 1:
            continue
        for N in range(1, 6400):
            p = E.plan(N, creg_k(cus, div), D, D, cus)
            if p[0]:
                forms |= E.walk_forms(N, p[2])
    return {f if isinstance(f, tuple) else (f,) for f in forms}


def unreachable_cover(cus):
    """the entries of required_cover() that no shape can reach with `cus` compute units"""
    out = set()
    for D, nk in ((8, 4), (136, 8), (264, 16)):
        can = reachable_walk_forms(cus, D)
        out |= {r for r in required_cover() if r[0] == "creg" and r[1] == nk and (not can or (len(r) > 2 and r[2:] not in can))}
    return out


def test_argument_rules(gpu):
    assert check_estep_argument_rules(gpu, True) >= 60


def test_coverage(dev, monkeypatch):
    """runs last in the module: everything the issue lists was reached on this device; a form of the register route that this
    device's CU count cannot reach at any N is a skip that names it, anything else missing is a failure"""
    if not COVER:                                       # selected on its own
        all_checks(dev, monkeypatch)
    missing, text = coverage_report()
    print(text)
    cus = dev.estep_plan(1024, 500, 8, 8)[5]
    cannot = unreachable_cover(cus)
    rest = [m for m in missing if m not in cannot]
    assert not rest, rest
    if missing:
        pytest.skip(f"forms this device's {cus} compute units cannot reach: {missing}")

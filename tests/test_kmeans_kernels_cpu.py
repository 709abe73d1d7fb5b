"""CPU: the mirror of the k-means helper kernels (tests/kmeans_kernels_ref.py) through the cases and gates of
tests/test_kmeans_kernels_gpu.py, the mutation table, the exactness claims of the grids, the host-side argument rules of the entry
points (the library loads without a device) and the list of kmeans.hip's entry points against the modules that test them.

  defect                     caught by (tests/test_kmeans_kernels_gpu.py)
  far_tie_high               check_select_far N = 1025, grid (the maximum sits at rows 5, 6 and 1029)
  far_no_mark                check_select_far n_sel = 3
  reloc_reverse              check_apply_relocation n = 4 (new id 1 is a later entry's old id)
  reloc_stale                check_apply_relocation n = 4 (old id 2 twice)
  fin_always_scale           check_finalize zeros_0_mid_last (cluster 0 precedes its source)
  fin_never_scale            check_finalize zeros_0_mid_last (clusters 3 and 6 follow their source)
  fin_argmax_last            check_finalize zeros_0_mid_last (two equal maxima)
  status_empties_precombine  check_global W = 3 (part 0 counts 1 where the combined count is 0)
  status_2p16                check_global W = 3 (the pair (1048575, 3))
  combine_reverse            check_global W = 3 float32 (mixed magnitudes)
  sum_drop_tail              check_rowwise N = 257
  colstats_drop_tail         check_col_stats N = 1025
  sort_per1                  check_accumulate K = 1025, uniform
  sort_unstable              check_accumulate K = 1024, one label
  cs_right                   check_cumsum_search N = 1025 (a query that is a prefix sum followed by zeros)
  cs_no_clip                 check_cumsum_search N = 15 (twice the total)
  perm_k4                    check_rowwise D = 8
  cnorm_pairwise             check_rowwise D = 20
  kpp_no_min                 check_kpp_grid with closest
  kpp_pot_fp32               check_kpp_grid N = 1300, D = 512 (the potential needs 27 bits)
  l2_fp32_acc                check_l2norm_gauss (on the 2^-4 grid a float32 sum is exact too: the Gaussian rows catch it)
  l2_recip                   check_rowwise (the grid rows, bit for bit)
  sub_ignores_ldo            check_rowwise (ldo = D + 8)"""
import os
import re

import numpy as np
import pytest

import kmeans_kernels_ref as R
import test_kmeans_kernels_gpu as G
from oracle import kmeans as ok

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def all_checks(m, env):
    for K in G.SORT_KS:
        for kind in G.SORT_LABELS:
            G.check_accumulate(m, env, 3000, 8, K, kind)
    G.check_accumulate(m, env, 3000, 8, 1366, "uniform", ldx=24, off=4)
    G.check_accumulate(m, env, 3000, 8, 40, "uniform", scan=None, ldx=24, off=4)
    for D in G.WIDE_DS:
        for scan in (None, "0"):
            G.check_accumulate(m, env, 700, D, 9, "uniform", scan=scan)
    G.check_accumulate(m, env, 3000, 4, 16384, "uniform")
    for route in G.STEP_ROUTES:
        for empty in G.STEP_EMPTY:
            for spherical in (0, 1):
                G.check_lloyd_step(m, route, empty, spherical)
    for D in G.FIN_DS:
        for which in G.FIN_COUNTS:
            G.check_finalize(m, D, which)
        G.check_finalize(m, D, "zeros_0_mid_last", spherical=1)
    G.check_finalize_k300(m)
    G.check_identity_perm(m)
    for W, dtype in G.GLOBAL_FORMS:
        G.check_global(m, W, dtype)
    for N in G.FAR_NS:
        for n_sel in G.FAR_SELS:
            for kind in G.FAR_KINDS:
                G.check_select_far(m, N, n_sel, kind)
    for n, D in G.RELOC_CASES:
        G.check_apply_relocation(m, n, D)
    for D in G.ROW_DS:
        for N in G.ROW_NS:
            G.check_rowwise(m, N, D)
    for N in G.COL_NS:
        for D in G.COL_DS:
            G.check_col_stats(m, N, D)
    G.check_l2norm_gauss(m)
    for D in G.KPP_DS:
        for N in G.KPP_NS:
            for T in G.KPP_TS:
                for wc in (True, False):
                    G.check_kpp_grid(m, N, D, T, wc)
    G.check_kpp_gauss(m, True)
    G.check_kpp_gauss(m, False)
    G.check_kpp_grid(m, 300, 1024, 16, True)
    for N in G.CS_NS:
        for T in G.CS_TS:
            G.check_cumsum_search(m, N, T)


def test_the_mirror_passes_every_check(monkeypatch):
    """every case of the GPU module on the unmutated mirror; the un-ordered reductions, summed in NumPy's order instead of the
    device's, stay below half of their gates"""
    G.RATIOS.clear()
    G.CASES.clear()
    all_checks(R.Mirror(), monkeypatch)
    print("cases:", dict(G.CASES), "total", sum(G.CASES.values()))
    for k, v in sorted(G.RATIOS.items()):
        print(f"  {k:28s} {v:.4f}")
    assert set(G.RATIOS) == {"lloyd_step.spherical", "finalize.spherical", "l2norm_rows.gauss", "kpp_step.pot.gauss"}
    # l2norm_rows.gauss has no reduction to be generous about: its gate is the two roundings of float32(sqrt) and the division plus
    # one to spare, so a correct result reaches 2 / 3 of it (0.57 here); the other three stay below a half
    assert G.RATIOS.pop("l2norm_rows.gauss") <= 0.7
    assert max(G.RATIOS.values()) <= 0.5, G.RATIOS


MUTATIONS = [
    ("far_tie_high", lambda m, e: G.check_select_far(m, 1025, 1, "grid")),
    ("far_no_mark", lambda m, e: G.check_select_far(m, 1023, 3, "grid")),
    ("reloc_reverse", lambda m, e: G.check_apply_relocation(m, 4, 4)),
    ("reloc_stale", lambda m, e: G.check_apply_relocation(m, 4, 260)),
    ("fin_always_scale", lambda m, e: G.check_finalize(m, 8, "zeros_0_mid_last")),
    ("fin_never_scale", lambda m, e: G.check_finalize(m, 6, "zeros_0_mid_last")),
    ("fin_argmax_last", lambda m, e: G.check_finalize(m, 4, "zeros_0_mid_last")),
    ("status_empties_precombine", lambda m, e: G.check_global(m, 3, F32)),
    ("status_2p16", lambda m, e: G.check_global(m, 3, F64)),
    ("combine_reverse", lambda m, e: G.check_global(m, 3, F32)),
    ("sum_drop_tail", lambda m, e: G.check_rowwise(m, 257, 4)),
    ("colstats_drop_tail", lambda m, e: G.check_col_stats(m, 1025, 5)),
    ("sort_per1", lambda m, e: G.check_accumulate(m, e, 3000, 8, 1025, "uniform")),
    ("sort_unstable", lambda m, e: G.check_accumulate(m, e, 3000, 8, 1024, "one")),
    ("cs_right", lambda m, e: G.check_cumsum_search(m, 1025, 5)),
    ("cs_no_clip", lambda m, e: G.check_cumsum_search(m, 15, 16)),
    ("perm_k4", lambda m, e: G.check_rowwise(m, 63, 8)),
    ("cnorm_pairwise", lambda m, e: G.check_rowwise(m, 65, 20)),
    ("kpp_no_min", lambda m, e: G.check_kpp_grid(m, 257, 64, 6, True)),
    ("kpp_pot_fp32", lambda m, e: G.check_kpp_grid(m, 1300, 512, 1, False)),
    ("l2_fp32_acc", lambda m, e: G.check_l2norm_gauss(m)),
    ("l2_recip", lambda m, e: G.check_rowwise(m, 65, 12)),
    ("sub_ignores_ldo", lambda m, e: G.check_rowwise(m, 64, 16)),
]


def test_the_table_names_every_defect_of_the_mirror():
    listed = [d for d, _ in MUTATIONS]
    assert sorted(listed) == sorted(R.DEFECTS), set(listed) ^ set(R.DEFECTS)
    documented = {ln.split()[0] for ln in __doc__.split("caught by")[1].splitlines()[1:] if ln.startswith("  ")}
    assert documented == set(R.DEFECTS), documented ^ set(R.DEFECTS)


@pytest.mark.parametrize("defect,check", MUTATIONS, ids=[d for d, _ in MUTATIONS])
def test_defect_is_caught(defect, check, monkeypatch):
    check(R.Mirror(), monkeypatch)                        # the case passes on the mirror as it is ...
    with pytest.raises(AssertionError):                   # ... and fails with the one defect
        check(R.Mirror(defect), monkeypatch)


def test_defects_in_the_sort_are_caught_at_every_k_above_one_block(monkeypatch):
    """`per` > 1 is reached by K = 1025 .. 4099: the per == 1 offsets fail each of them, and pass K = 1024"""
    G.check_accumulate(R.Mirror("sort_per1"), monkeypatch, 3000, 8, 1024, "uniform")
    for K in G.SORT_KS[1:]:
        for kind in ("uniform", "top40", "one"):
            with pytest.raises(AssertionError):
                G.check_accumulate(R.Mirror("sort_per1"), monkeypatch, 3000, 8, K, kind)


# ------------------------------------------------------------------ the mirror against the oracle and against float64
def test_mirror_average_is_the_oracles_in_place_loop():
    rng = np.random.default_rng(0)
    for which, counts in G.FIN_COUNTS.items():
        counts = np.array(counts, F32)
        sums = rng.standard_normal((7, 12)).astype(F32)
        C_old = rng.standard_normal((7, 12)).astype(F32)
        e_new, e_sh, e_tot = ok.finalize(C_old, sums, counts)
        rows = R.average(sums, counts)
        assert G.bits_equal(rows, e_new), which
        assert G.bits_equal(R.shift_of(rows, C_old), e_sh), which
        assert abs(R.status_sum(e_sh) - e_tot) <= 7 * 2.0 ** -52 * e_tot


def test_ordered_functions_agree_with_float64():
    """the fixed orders compute the operation the float64 reference states (bound: one rounding per term, relative to the sum of
    the absolute terms)"""
    rng = np.random.default_rng(1)
    X, C = rng.standard_normal((300, 20)).astype(F32), rng.standard_normal((6, 20)).astype(F32)
    labels = rng.integers(0, 6, 300).astype(np.int32)
    assert np.all(np.abs(R.cnorm(X) - R.ref_cnorm(X)) <= 20 * G.U * R.ref_cnorm(X))
    d = R.ref_dist_to_assigned(X, C, labels)
    assert np.all(np.abs(R.dist_to_assigned(X, C, labels) - d) <= 22 * G.U * d)
    s, c = R.accumulate(X, labels, 6)
    rs, rc = R.ref_accumulate(X, labels, 6)
    absum = np.zeros((6, 20))
    np.add.at(absum, labels, np.abs(X.astype(F64)))
    assert np.array_equal(c, rc) and np.all(np.abs(s - rs) <= 300 * G.U * absum)
    v = rng.standard_normal(1000).astype(F32)
    assert abs(R.sum_blocks_256(v) - v.astype(F64).sum()) <= 1000 * 2.0 ** -53 * np.abs(v).sum()
    cs1, cs2 = R.col_stats(X)
    r1, r2 = R.ref_col_stats(X)
    assert np.allclose(cs1, r1, rtol=0, atol=1e-12 * 300) and np.allclose(cs2, r2, rtol=1e-13, atol=0)
    idx, val, after = R.select_far(v[:50], 5)
    ridx, rval, rafter = R.ref_select_far(v[:50], 5)
    assert np.array_equal(idx, ridx) and np.array_equal(val, rval) and np.array_equal(after, rafter)
    nd, pot = R.kpp_step(X, [0, 299, 5], None)
    rnd, rpot = R.ref_kpp(X, [0, 299, 5], None)
    assert np.all(np.abs(nd - rnd) <= 22 * G.U * rnd) and np.all(np.abs(pot - rpot) <= 22 * G.U * rpot)
    assert np.array_equal(R.cumsum_search(np.abs(v), [0.0, 3.0, 1e9]), R.ref_cumsum_search(np.abs(v), [0.0, 3.0, 1e9]))
    G_ = G.grid(rng, (9, 33), 2.0 ** -4, 2.0)
    G_[0, 0] = 1.0
    assert np.all(np.abs(R.l2norm_rows(G_) - R.ref_l2norm(G_)) <= 2 * G.U * np.abs(R.ref_l2norm(G_)))


def test_zero_row_of_l2norm_is_what_torch_gives():
    """x / x.norm() of an all-zero row on the CPU: NaN, which is what the header states for slic_l2norm_rows and check_rowwise pins"""
    import torch
    x = torch.zeros(2, 5)
    x[1, 2] = 3.0
    t = (x / torch.norm(x, dim=1, keepdim=True)).numpy()
    m = R.l2norm_rows(x.numpy())
    assert np.isnan(t[0]).all() and np.isnan(m[0]).all() and np.array_equal(t[1], m[1])


# ------------------------------------------------------------------ the exactness claims of the grids
def two_orders(a, axis, dtype):
    """the sum along `axis` ascending and descending, accumulated in `dtype`"""
    a = np.moveaxis(np.asarray(a, dtype), axis, 0)
    up, down = np.zeros(a.shape[1:], dtype), np.zeros(a.shape[1:], dtype)
    for r in a:
        up = up + r
    for r in a[::-1]:
        down = down + r
    return up, down


def test_grid_sums_are_exact_in_any_order():
    """every `exact in any order` of the GPU module: the sum ascending, descending and NumPy's pairwise agree in the stated format
    (and the bit counts stated beside the cases stay below 24 / 53)"""
    rng = np.random.default_rng(2)
    # col_stats: 2^-8 grid in [-4, 4], 3001 rows: 12 + 2 + 8 bits for the sum, 12 + 4 + 16 for the squares (< 53)
    g = G.grid(rng, (3001, 5), 2.0 ** -8, 4.0).astype(F64)
    for t in (g, g * g):
        up, down = two_orders(t, 0, F64)
        assert np.array_equal(up, down) and np.array_equal(up, t.sum(0))
    assert 12 + 4 + 16 < 53
    # l2norm_rows: 2^-4 grid, |v| <= 2, D <= 1024: 10 + 2 + 8 bits (< 53, and < 24: float32 sums are exact as well)
    g = G.grid(rng, (7, 1024), 2.0 ** -4, 2.0)
    up, down = two_orders(g.astype(F64) ** 2, 1, F64)
    up32, down32 = two_orders(g * g, 1, F32)
    assert np.array_equal(up, down) and np.array_equal(up32, down32) and np.array_equal(up, up32.astype(F64))
    # kpp_step: 2^-3 grid, |v| <= 2, D <= 1024: a distance needs 10 + 4 + 6 bits (< 24), the potential of 1300 rows 11 more (< 53)
    g = G.grid(rng, (1300, 1024), 2.0 ** -3, 2.0)
    d = (g - g[7]) ** 2
    up32, down32 = two_orders(d, 1, F32)
    d64 = ((g.astype(F64) - g[7].astype(F64)) ** 2).sum(1)
    assert np.array_equal(up32, down32) and np.array_equal(up32.astype(F64), d64) and 10 + 4 + 6 < 24
    up, down = two_orders(d64, 0, F64)
    assert up == down == d64.sum() and 10 + 4 + 6 + 11 < 53
    up32, down32 = two_orders(d64, 0, F32)
    assert up32 != up                                      # ... and float32 is not enough for the potential
    # cumsum_search: 2^-10 grid in [0, 8], 5000 values: 13 + 3 + 10 bits (< 53)
    v, _ = G.cs_problem(5000)
    up, down = two_orders(v, 0, F64)
    assert up == down == v.astype(F64).sum() and np.cumsum(v.astype(F64))[-1] == up and 13 + 3 + 10 < 53
    # lloyd_global's n_changed pairs: integers below 2^21 in float32 and float64
    assert F32(1048575) + F32(5) == 1048580 and R.nch_total([(1048575, 3), (5, 0)]) == 1048580 + 3 * 2 ** 20


def test_rank_order_is_visible_in_the_payloads():
    for W in (3, 16):
        K, D, parts = G.global_parts(W, F32)
        a, b = R.combine_f32(parts[:, :K * D]), R.combine_f32(parts[::-1, :K * D])
        assert not G.bits_equal(a, b), W


def test_step_problems_have_the_empty_cluster_on_the_stated_side():
    for route in G.STEP_ROUTES:
        for empty in G.STEP_EMPTY:
            G.step_problem(route, empty)                   # asserts inside


# ------------------------------------------------------------------ host argument rules (no device needed)
def test_host_argument_rules():
    from video_similarity_search_amd import _lib
    assert G.check_argument_rules(_lib.load()) >= 120


# ------------------------------------------------------------------ no entry point of kmeans.hip without a test module
COVERED_ELSEWHERE = {
    # the E-step, every entry point bit for bit against the oracle (its calls are methods of this module's Device)
    "slic_kmeans_assign_workspace_bytes": "test_kmeans_estep_gpu", "slic_kmeans_assign": "test_kmeans_estep_gpu",
    "slic_kmeans_assign_perm": "test_kmeans_estep_gpu", "slic_kmeans_assign_perm_plan": "test_kmeans_estep_gpu",
    "slic_kmeans_lloyd_local_workspace_bytes": "test_kmeans_estep_gpu", "slic_kmeans_lloyd_local": "test_kmeans_estep_gpu",
    # the certified bf16 E-step (csrc/kmeans_bf16.h, included by kmeans.hip)
    "slic_kmeans_bf16_plan": "test_kmeans_bf16_cpu", "slic_kmeans_bf16_eps": "test_kmeans_bf16_cpu",
    "slic_kmeans_bf16_image": "test_kmeans_bf16_gpu", "slic_kmeans_assign_bf16_workspace_bytes": "test_kmeans_bf16_gpu",
    "slic_kmeans_assign_bf16": "test_kmeans_bf16_gpu", "slic_kmeans_lloyd_step_bf16_workspace_bytes": "test_kmeans_bf16_gpu",
    "slic_kmeans_lloyd_step_bf16": "test_kmeans_bf16_gpu", "slic_kmeans_lloyd_local_bf16_workspace_bytes": "test_kmeans_bf16_gpu",
    "slic_kmeans_lloyd_local_bf16": "test_kmeans_bf16_gpu",
    # k-means++ as one device-driven sequence
    "slic_kmeanspp_run_workspace_bytes": "test_kmeans_gpu", "slic_kmeanspp_run": "test_kmeans_gpu",
    "slic_kmeanspp_run_batch_workspace_bytes": "test_kmeans_gpu", "slic_kmeanspp_run_batch": "test_kmeans_gpu",
}
# extern "C" but not part of the ABI (absent from include/slic_hip.h): the stamp counters scripts/dbg_km_stamps.py reads
NOT_ABI = {"slic_debug_km_counters"}


def test_every_entry_point_of_kmeans_hip_has_a_test_module():
    names = set()
    for f in ("kmeans.hip", "kmeans_bf16.h"):
        src = open(os.path.join(ROOT, "video_similarity_search_amd", "csrc", f)).read()
        names |= set(re.findall(r'extern "C"\s+[\w\s\*]*?\b(slic_\w+)\s*\(', src))
    assert len(names) > 30
    header = open(os.path.join(ROOT, "include", "slic_hip.h")).read()
    assert not [n for n in NOT_ABI if n in header] and not [n for n in names - NOT_ABI if n not in header]
    listed = set(G.COVERED) | set(COVERED_ELSEWHERE) | NOT_ABI
    assert names == listed, (sorted(names - listed), sorted(listed - names))
    assert not set(G.COVERED) & set(COVERED_ELSEWHERE)
    gpu_src = open(os.path.join(ROOT, "tests", "test_kmeans_kernels_gpu.py")).read()
    for n in G.COVERED:                                    # called by name in the GPU module, not only listed
        assert gpu_src.count(n) >= 2, n
    for n, mod in COVERED_ELSEWHERE.items():
        path = os.path.join(ROOT, "tests", mod + ".py")
        assert os.path.exists(path), mod
        body = open(path).read()
        # by its ABI name, or by the HipKernels method that wraps it (which sizes the workspace itself)
        stem = n.replace("slic_kmeans_", "").replace("slic_", "").replace("_workspace_bytes", "")
        assert n in body or stem in body, (n, mod)

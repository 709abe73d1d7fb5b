"""CPU: the NumPy mirror of csrc/loss.hip and csrc/nce.hip (tests/loss_cpu_kernels.py) against float64 through the cases and
gates of tests/test_loss_kernels_gpu.py run with the mirror in the device's place, the mutation table, and the host-side argument
rules of the entry points (the library loads without a device).

Two conditions decide whether a gate is right, and both are checked here.  Reachable: the unmutated float32 mirror, which sums in
NumPy's order and not the kernels', meets every gate with a factor 4 to spare (test_every_gate_is_reachable_with_a_factor_4).
Tight enough: every defect of the table below, switched on in the mirror alone, makes the named check raise
(test_mutation_is_caught).

Worst error / gate ratio of the unmutated mirror per gate, over all cases (the case that gives it in brackets):

  infonce_rows.loss                0.002  (1, 8, 65, 1.5)
  infonce_rows.rowloss             0.008  (5, 6, 200, 1.5)
  infonce_rows_bwd.dX              0.019  (5, 2, 130, None)
  infonce_rows_bwd.dY              0.051  (5, 6, 63, 1.5)
  margin_cos.loss                  0.001  (9, 64, 0, 0.25, 1.5)
  margin_cos.rowloss               0.014  (5, 63, 0, 0.0, None)
  margin_cos_bwd.dX                0.093  (5, 63, 0, 0.0, None)
  margin_cos_bwd.dY                0.095  (9, 64, 0, 0.25, 1.5)
  margin_cos_bwd.dZ                0.098  (9, 64, 0, 0.25, 1.5)
  margin_euclid.loss               0.022  (1, 2, 1, 0.25, None)
  margin_euclid.rowloss            0.047  (9, 64, 1, 0.25, 1.5)
  margin_euclid_bwd.dX             0.182  (9, 200, 1, 0.0, 1.5)
  margin_euclid_bwd.dY             0.164  (9, 200, 1, 0.0, 1.5)
  margin_euclid_bwd.dZ             0.160  (9, 64, 1, 0.25, 1.5)
  nce_bank_update                  0.109  (5, 130)
  nce_fused_bwd                    0.095  (3, 260, 260, None)
  nce_fused_bwd.chain              0.010  (1, 130, 132, 1.5)
  nce_fused_fwd.scores             0.200  (3, 130, 4, None)
  nce_fused_update.bank_ab         0.095  (1, 130, 132, 1.5)
  nce_fused_update.bank_l          0.113  (1, 130, 132, 1.5)
  nce_fused_update.loss            0.002  (3, 130, 4, None)
  nce_fused_update.lse             0.005  (3, 130, 4, None)
  nce_fused_update.rowloss         0.005  (3, 130, 4, None)
  nce_scores_bwd                   0.238  (3, 8, 132)
  nce_scores_fwd                   0.109  (3, 7, 4)
  ntxent.dE                        0.011  (66, 6, 1.5, False)
  ntxent.loss                      0.015  (2, 2, None, False)
  ntxent_euclid.dE                 0.005  (8, 70, 1.5)
  ntxent_euclid.dist               0.234  (258, 3, 1.5)
  ntxent_euclid.loss               0.006  (258, 3, 1.5)
  ntxent_euclid.rowloss            0.026  (258, 3, 1.5)
  pair_distance.cos                0.039  (3, 65, 0, 'plain')
  pair_distance.euclid             0.127  (5, 63, 1, 'plain')
  pair_distance_bwd.cos.dX         0.105  (5, 63, 0, 'plain')
  pair_distance_bwd.cos.dY         0.102  (9, 200, 0, 'plain')
  pair_distance_bwd.euclid.dX      0.180  (5, 63, 1, 'plain')
  pair_distance_bwd.euclid.dY      0.180  (5, 63, 1, 'plain')
  pdist.cos                        0.095  (9, None, 63)
  pdist.euclid                     0.164  (9, None, 63)
  softmax_ce0.loss                 0.012  (3, 255, 1.5)
  softmax_ce0.lse                  0.045  (3, 257, 1.5)
  softmax_ce0.rowloss              0.030  (3, 2, 1.5)
  softmax_ce0_bwd                  0.146  (3, 257, 1.5)

  mutation            caught by (tests/test_loss_kernels_gpu.py)
  sel_seen            check_select rank_chunks_m0 / _m1 (the rank lies beyond the first chunk)
  sel_tie_last        check_select mode2_ties; fallback_m1 (the closest negative is tied with a later one)
  sel_ge              check_select zero_loss_m1 / _m2
  sel_fallback_row    check_select fallback_m1
  sel_fallback_chunk  check_select fallback_m2
  sel_label32         check_select fallback_m1 (column 130 is labelled 5 + 2^32, the anchors 5)
  sel_anchor_label    check_select fallback_cross_m3, cross_129_5_m0
  selk_no_skip        check_select_k topup
  selk_no_topup       check_select_k topup
  selk_status_all     check_select_k short
  row_tail            check_pair_distance D = 130, check_margin D = 65, check_infonce_rows D = 200, check_nce_bank_update D = 65
  pd_eps_out          check_pair_distance 'dup' D = 65; check_pdist euclidean eps = 0.25
  pd_clamp_prod       check_pair_distance 'zero' (the backward: the forward is 1 - 0 either way)
  hinge_ge            check_margin margin = 0, both metrics (the row with y = z)
  gscale_ignored      every backward check with gscale = 1.5
  mean_n              the loss gate of check_margin, check_infonce_rows, check_ntxent, check_ntxent_euclid, check_ce0, check_nce_fused
  ntx_diag_inf        check_ntxent n = 6
  ntx_target          check_ntxent n = 33
  ntx_ld              check_ntxent n = 6 (the NaN padding is read, the output padding written)
  eucl_dup            check_ntxent_euclid n = 8
  eucl_256            check_ntxent_euclid n = 258
  infonce_pos_twice   check_infonce_rows
  nce_k_tail          check_nce_scores_bwd K1 = 70; check_nce_fused_bwd K1 = 129
  nce_d_slice         check_nce_scores_fwd D = 260; check_nce_scores_bwd D = 260; check_nce_fused_bwd D = 260; check_nce_fused D = 132
  nce_grid_stride     check_nce_scores_fwd K1 = 515
  nce_side            check_nce_fused
  nce_idle_part       check_nce_fused K1 = 1
  nce_dup_first       check_nce_fused B = 3
  ce0_no_shift        check_ce0

One remark the table owes.  nce_idle_part: an idle part is guarded twice, in nce_fused_fwd (`M > -INFINITY` before the eight groups
are merged, else -inf - -inf = NaN) and in nce_fused_update (`pp[2 c] > -INFINITY`); either guard alone keeps the result right, so
the mutant removes both."""
import ctypes

import numpy as np
import pytest
import torch

import loss_cpu_kernels as K
import test_loss_kernels_gpu as G

F32 = np.float32


class Mirror:
    """tests/loss_cpu_kernels.py behind the interface of test_loss_kernels_gpu.Device"""

    def __init__(self, *mut):
        self.mut = frozenset(mut)

    def select(self, Dm, labels, anc, pos, margin, mode, u):
        return K.triplet_select(Dm, labels, anc, None, pos, margin, mode, u, self.mut)

    def select_cross(self, Dm, col_labels, anc, anc_labels, pos, margin, mode, u):
        return K.triplet_select(Dm, col_labels, anc, anc_labels, pos, margin, mode, u, self.mut)

    def select_k(self, Dm, labels, anc, pos, margin, Kn, u):
        return K.triplet_select_k(Dm, labels, anc, pos, margin, Kn, u, self.mut)

    def pair_distance(self, X, Y, euclid):
        return K.pair_distance(X, Y, euclid, self.mut)

    def pair_distance_bwd(self, X, Y, Gr, euclid):
        return K.pair_distance_bwd(X, Y, Gr, euclid, self.mut)

    def pdist(self, V, eps, euclid):
        return K.pdist(V, eps, euclid, self.mut)

    def pdist2(self, X, Y, eps, euclid):
        return K.pdist2(X, Y, eps, euclid, self.mut)

    def margin_fwd(self, X, Y, Z, margin, euclid):
        return K.margin_fwd(X, Y, Z, margin, euclid, self.mut)

    def margin_bwd(self, X, Y, Z, st, gscale, euclid):
        return K.margin_bwd(X, Y, Z, st, gscale, euclid, self.mut)

    def infonce_fwd(self, X, Y, T):
        return K.infonce_rows_fwd(X, Y, T, self.mut)

    def infonce_bwd(self, X, Y, st, T, gscale):
        return K.infonce_rows_bwd(X, Y, st, T, gscale, self.mut)

    def ntxent(self, Eflat, n, D, lde, T, gscale, ldd):
        return K.ntxent(Eflat, n, D, lde, T, gscale, ldd, self.mut)

    def ntxent_euclid_fwd(self, E, T):
        return K.ntxent_euclid_fwd(E, T, self.mut)

    def ntxent_euclid_bwd(self, E, dist, wm, gscale):
        return K.ntxent_euclid_bwd(E, dist, wm, gscale, self.mut)

    def nce_scores_fwd(self, bank, idx, f, T, gather):
        return K.nce_scores_fwd(bank, idx, f, T, gather, self.mut)

    def nce_scores_bwd(self, bank, idx, dout, T):
        return K.nce_scores_bwd(bank, idx, dout, T, self.mut)

    def nce_bank_update(self, bank, y, f, momentum):
        return K.nce_bank_update(bank, y, f, momentum, self.mut)

    def ce0_fwd(self, x):
        return K.softmax_ce0_fwd(x, self.mut)

    def ce0_bwd(self, x, lse, gscale):
        return K.softmax_ce0_bwd(x, lse, gscale, self.mut)

    def fused_fwd(self, bank_l, bank_ab, f_l, f_ab, idx, T):
        return K.nce_fused_fwd(bank_l, bank_ab, f_l, f_ab, idx, T, self.mut)

    def fused_update(self, bank_l, bank_ab, y, f_l, f_ab, momentum, part, scores):
        return K.nce_fused_update(bank_l, bank_ab, y, f_l, f_ab, momentum, part, scores, self.mut)

    def fused_bwd(self, rows, scores, lse, T, gscale):
        return K.nce_fused_bwd(rows, scores, lse, T, gscale, self.mut)


def all_checks(m):
    """every case of the GPU module, on backend m"""
    for name in G.SEL_NAMED:
        G.check_select(m, name)
    for n, P, mode in G.SEL_RANDOM:
        G.check_select(m, G.sel_random(n, P, mode, 0))
    for name in G.SELK_NAMED:
        G.check_select_k(m, name)
    for n, D in G.ROW_SHAPES:
        for euclid in (0, 1):
            G.check_pair_distance(m, n, D, euclid)
    for D in (2, 65, 200):
        G.check_pair_distance(m, 5, D, 1, "dup")
    for D in (2, 63, 130):
        G.check_pair_distance(m, 3, D, 0, "zero")
    for mm in (None, 7):
        for D in (63, 130):
            for euclid, eps in [(0, 0.0), (1, 0.25), (1, 0.0)]:
                G.check_pdist(m, 9 if mm is None else 3, mm, D, euclid, eps)
    for n, D, margin, gscale in G.MARGIN_CASES:
        for euclid in (0, 1):
            G.check_margin(m, n, D, euclid, margin, gscale)
    for c in G.INFONCE_CASES:
        G.check_infonce_rows(m, *c)
    for c in G.NTX_CASES:
        G.check_ntxent(m, *c)
    for c in G.EUCL_CASES:
        G.check_ntxent_euclid(m, *c)
    for c in G.SCORES_FWD_CASES:
        G.check_nce_scores_fwd(m, *c)
    for c in G.SCORES_BWD_CASES:
        G.check_nce_scores_bwd(m, *c)
    for B in (1, 5):
        for D in (4, 65, 130):
            G.check_nce_bank_update(m, B, D)
    for K1 in (1, 2, 255, 257, 600):
        for B, gscale in [(1, None), (3, 1.5)]:
            G.check_ce0(m, B, K1, gscale)
    for c in G.FUSED_CASES:
        G.check_nce_fused(m, *c)
    for c in G.FUSED_BWD_CASES:
        G.check_nce_fused_bwd(m, *c)


# ------------------------------------------------------------------ the mirror against float64, gate by gate
def test_every_gate_is_reachable_with_a_factor_4():
    """the unmutated mirror passes every case of the GPU module (integer outputs exactly), and its worst error / gate ratio
    stays at or below 1 / 4 for every named gate"""
    G.RATIOS.clear()
    all_checks(Mirror())
    ratios = dict(G.RATIOS)
    G.RATIOS.clear()
    assert len(ratios) >= 40
    worst = {k: v for k, v in ratios.items() if v > 0.25}
    assert not worst, worst


def test_the_spelled_out_cosine_is_F_cosine_similarity():
    """where no norm is below the clamp, the formula the zero-row cases differentiate is F.cosine_similarity to the last bits"""
    rng = np.random.default_rng(0)
    x, y = G.t64(rng.standard_normal((5, 65))), G.t64(rng.standard_normal((5, 65)))
    a, b = G.cos64(x, y), G.cos64(x, y, True)
    assert torch.allclose(a, b, rtol=1e-14, atol=0)
    ga, gb = torch.autograd.grad(a.sum(), [x])[0], torch.autograd.grad(b.sum(), [x])[0]
    assert torch.allclose(ga, gb, rtol=1e-12, atol=1e-16)


def test_reference_draws_floor_like_the_exact_product():
    """u = float32((r + 0.5) / c): the float32 product floors to r for every set size the cases can meet"""
    for c in range(1, 261):
        for r in range(c):
            u = F32((r + 0.5) / c)
            assert int(u * F32(c)) == r and 0 <= u < 1
        assert int(np.nextafter(F32(1), F32(0)) * F32(c)) in (c - 1, c)          # the kernel clamps c to c - 1


# ------------------------------------------------------------------ the mutation table
MUTATIONS = [
    ("sel_seen", "rank_chunks_m0", lambda m: G.check_select(m, "rank_chunks_m0")),
    ("sel_seen", "rank_chunks_m1", lambda m: G.check_select(m, "rank_chunks_m1")),
    ("sel_tie_last", "mode2_ties", lambda m: G.check_select(m, "mode2_ties")),
    ("sel_tie_last", "fallback_m1", lambda m: G.check_select(m, "fallback_m1")),
    ("sel_ge", "zero_loss_m1", lambda m: G.check_select(m, "zero_loss_m1")),
    ("sel_ge", "zero_loss_m2", lambda m: G.check_select(m, "zero_loss_m2")),
    ("sel_fallback_row", "fallback_m1", lambda m: G.check_select(m, "fallback_m1")),
    ("sel_fallback_chunk", "fallback_m2", lambda m: G.check_select(m, "fallback_m2")),
    ("sel_label32", "fallback_m1", lambda m: G.check_select(m, "fallback_m1")),
    ("sel_anchor_label", "fallback_cross_m3", lambda m: G.check_select(m, "fallback_cross_m3")),
    ("sel_anchor_label", "cross_129_5_m0", lambda m: G.check_select(m, "cross_129_5_m0")),
    ("selk_no_skip", "topup", lambda m: G.check_select_k(m, "topup")),
    ("selk_no_topup", "topup", lambda m: G.check_select_k(m, "topup")),
    ("selk_status_all", "short", lambda m: G.check_select_k(m, "short")),
    ("row_tail", "pair_distance", lambda m: G.check_pair_distance(m, 5, 130, 0)),
    ("row_tail", "pair_distance-euclid", lambda m: G.check_pair_distance(m, 5, 130, 1)),
    ("row_tail", "margin", lambda m: G.check_margin(m, 3, 65, 0, 0.0, 1.5)),
    ("row_tail", "infonce", lambda m: G.check_infonce_rows(m, 5, 6, 200, 1.5)),
    ("row_tail", "pdist", lambda m: G.check_pdist(m, 9, None, 130, 0, 0.0)),
    ("row_tail", "bank_update", lambda m: G.check_nce_bank_update(m, 5, 65)),
    ("pd_eps_out", "pair_distance-dup", lambda m: G.check_pair_distance(m, 5, 65, 1, "dup")),
    ("pd_eps_out", "pdist", lambda m: G.check_pdist(m, 9, None, 63, 1, 0.25)),
    ("pd_clamp_prod", "pair_distance-zero", lambda m: G.check_pair_distance(m, 3, 63, 0, "zero")),
    ("hinge_ge", "margin-cos", lambda m: G.check_margin(m, 5, 63, 0, 0.0, None)),
    ("hinge_ge", "margin-euclid", lambda m: G.check_margin(m, 5, 63, 1, 0.0, None)),
    ("gscale_ignored", "margin", lambda m: G.check_margin(m, 9, 64, 0, 0.25, 1.5)),
    ("gscale_ignored", "margin-euclid", lambda m: G.check_margin(m, 9, 64, 1, 0.25, 1.5)),
    ("gscale_ignored", "infonce", lambda m: G.check_infonce_rows(m, 5, 6, 63, 1.5)),
    ("gscale_ignored", "ntxent", lambda m: G.check_ntxent(m, 6, 6, 1.5)),
    ("gscale_ignored", "ntxent_euclid", lambda m: G.check_ntxent_euclid(m, 8, 70, 1.5)),
    ("gscale_ignored", "ce0", lambda m: G.check_ce0(m, 3, 255, 1.5)),
    ("gscale_ignored", "fused", lambda m: G.check_nce_fused(m, 3, 15, 132, 1.5)),
    ("gscale_ignored", "fused_bwd", lambda m: G.check_nce_fused_bwd(m, 3, 32, 4, 1.5)),
    ("mean_n", "margin", lambda m: G.check_margin(m, 9, 64, 0, 0.25, 1.5)),
    ("mean_n", "infonce", lambda m: G.check_infonce_rows(m, 5, 6, 63, 1.5)),
    ("mean_n", "ntxent", lambda m: G.check_ntxent(m, 6, 6, 1.5)),
    ("mean_n", "ntxent_euclid", lambda m: G.check_ntxent_euclid(m, 8, 70, 1.5)),
    ("mean_n", "ce0", lambda m: G.check_ce0(m, 3, 255, 1.5)),
    ("mean_n", "fused", lambda m: G.check_nce_fused(m, 3, 15, 132, 1.5)),
    ("ntx_diag_inf", "ntxent", lambda m: G.check_ntxent(m, 6, 6, 1.5)),
    ("ntx_target", "ntxent", lambda m: G.check_ntxent(m, 33, 66, None)),
    ("ntx_ld", "ntxent", lambda m: G.check_ntxent(m, 6, 6, 1.5)),
    ("eucl_dup", "ntxent_euclid", lambda m: G.check_ntxent_euclid(m, 8, 70, 1.5)),
    ("eucl_256", "ntxent_euclid", lambda m: G.check_ntxent_euclid(m, 258, 3, 1.5)),
    ("infonce_pos_twice", "infonce", lambda m: G.check_infonce_rows(m, 5, 6, 63, 1.5)),
    ("nce_k_tail", "scores_bwd", lambda m: G.check_nce_scores_bwd(m, 3, 70, 132)),
    ("nce_k_tail", "fused_bwd", lambda m: G.check_nce_fused_bwd(m, 3, 129, 132, 1.5)),
    ("nce_d_slice", "scores_fwd", lambda m: G.check_nce_scores_fwd(m, 3, 9, 260, 1)),
    ("nce_d_slice", "scores_bwd", lambda m: G.check_nce_scores_bwd(m, 3, 57, 260)),
    ("nce_d_slice", "fused", lambda m: G.check_nce_fused(m, 3, 15, 132, 1.5)),
    ("nce_d_slice", "fused_bwd", lambda m: G.check_nce_fused_bwd(m, 1, 97, 260, None)),
    ("nce_grid_stride", "scores_fwd", lambda m: G.check_nce_scores_fwd(m, 3, 515, 260, 0)),
    ("nce_side", "fused", lambda m: G.check_nce_fused(m, 3, 15, 132, 1.5)),
    ("nce_idle_part", "fused", lambda m: G.check_nce_fused(m, 1, 1, 4, None)),
    ("nce_idle_part", "fused-K17", lambda m: G.check_nce_fused(m, 3, 17, 260, None)),
    ("nce_dup_first", "fused", lambda m: G.check_nce_fused(m, 3, 15, 132, 1.5)),
    ("ce0_no_shift", "ce0", lambda m: G.check_ce0(m, 1, 2, None)),
]


def test_the_table_names_every_mutation_of_the_mirror():
    listed = {m for m, _, _ in MUTATIONS}
    documented = {ln.split()[0] for ln in K.__doc__.split("the default is the empty set:")[1].splitlines() if ln.startswith("  ")}
    assert listed == documented, listed ^ documented


@pytest.mark.parametrize("mut,where,case", MUTATIONS, ids=[f"{m}-{w}" for m, w, _ in MUTATIONS])
def test_mutation_is_caught(mut, where, case):
    case(Mirror())                                        # the case passes on the mirror as it is ...
    with pytest.raises(AssertionError):                   # ... and fails with the one defect
        case(Mirror(mut))


# ------------------------------------------------------------------ host argument rules (no device needed)
def test_host_argument_rules():
    from video_similarity_search_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                 # never read: every call below is refused before any launch

    def refused(name, *args):
        assert getattr(lib, name)(*args, None) != 0, (name, args)
        assert name.encode() in lib.slic_last_error(), (name, lib.slic_last_error())

    # valid argument lists (pointers all `p`), and which pointers may be NULL
    valid = {
        "slic_ntxent_fwd": ([p, 4, 6, 8, 0.1, p, p], ()),
        "slic_ntxent_bwd": ([p, 4, 6, 0.1, p, p, 8], (4,)),
        "slic_ntxent_euclid_fwd": ([p, 4, 6, 0.1, p, p, p, p], ()),
        "slic_ntxent_euclid_bwd": ([p, p, p, 4, 6, p, p], (5,)),
        "slic_pair_distance": ([p, p, 4, 6, 0, p], ()),
        "slic_pair_distance_bwd": ([p, p, p, 4, 6, 0, p, p], ()),
        "slic_margin_cos_fwd": ([p, p, p, 4, 6, 0.1, p, p, p], ()),
        "slic_margin_cos_bwd": ([p, p, p, p, 4, 6, p, p, p, p], (6,)),
        "slic_margin_euclid_fwd": ([p, p, p, 4, 6, 0.1, p, p, p], ()),
        "slic_margin_euclid_bwd": ([p, p, p, p, 4, 6, p, p, p, p], (6,)),
        "slic_pdist": ([p, 4, 6, 0.0, 0, p], ()),
        "slic_pdist2": ([p, 4, p, 3, 6, 0.0, 0, p], ()),
        "slic_infonce_rows_fwd": ([p, p, 4, 6, 8, 0.1, p, p, p], ()),
        "slic_infonce_rows_bwd": ([p, p, p, 4, 6, 8, 0.1, p, p, p], (7,)),
        "slic_triplet_select": ([p, p, 8, p, p, 4, 0.1, 1, p, p], ()),
        "slic_triplet_select_k": ([p, p, 8, p, p, 4, 0.1, 5, p, p, p], ()),
        "slic_triplet_select_cross": ([p, p, 8, p, p, p, 4, 0.1, 1, p, p], ()),
        "slic_nce_scores_fwd": ([p, p, p, 2, 3, 8, 0.1, p, p], (8,)),
        "slic_nce_scores_bwd": ([p, p, p, 2, 3, 8, 0.1, p], ()),
        "slic_nce_bank_update": ([p, p, p, 2, 8, 0.5], ()),
        "slic_softmax_ce0_fwd": ([p, 2, 3, p, p, p], ()),
        "slic_softmax_ce0_bwd": ([p, p, 2, 3, p, p], (4,)),
        "slic_nce_fused_fwd": ([p, p, p, p, p, 2, 3, 8, 0.1, p, p, p], ()),
        "slic_nce_fused_update": ([p, p, p, p, p, 2, 8, 0.5, p, p, 3, p, p, p], (8, 9, 11, 12, 13)),
        "slic_nce_fused_bwd": ([p, p, p, 2, 3, 8, 0.1, p, p], (7,)),
    }

    def with_(name, **at):
        args = list(valid[name][0])
        for i, v in at.items():
            args[int(i[1:])] = v
        return args

    # any required pointer NULL
    for name, (args, optional) in valid.items():
        for i, a in enumerate(args):
            if a is p and i not in optional:
                refused(name, *with_(name, **{f"a{i}": None}))
    refused("slic_ntxent_fwd", *with_("slic_ntxent_fwd", a2=5))                # odd D
    refused("slic_ntxent_fwd", *with_("slic_ntxent_fwd", a3=5))                # lde < D
    refused("slic_ntxent_fwd", *with_("slic_ntxent_fwd", a1=1))                # n = 1
    refused("slic_ntxent_bwd", *with_("slic_ntxent_bwd", a6=5))                # ldd < D
    refused("slic_ntxent_bwd", *with_("slic_ntxent_bwd", a1=16000, a2=382, a6=382))      # (n + D + 4) * 4 = 65544 > 65536
    assert b"LDS" in lib.slic_last_error()
    refused("slic_ntxent_euclid_fwd", *with_("slic_ntxent_euclid_fwd", a1=5))  # odd n
    refused("slic_ntxent_euclid_fwd", *with_("slic_ntxent_euclid_fwd", a1=8194))
    for NY in (1, 9):
        refused("slic_infonce_rows_fwd", *with_("slic_infonce_rows_fwd", a3=NY))
        refused("slic_infonce_rows_bwd", *with_("slic_infonce_rows_bwd", a4=NY))
    for Kn in (0, 9):
        refused("slic_triplet_select_k", *with_("slic_triplet_select_k", a7=Kn))
    refused("slic_triplet_select", *with_("slic_triplet_select", a7=3))
    refused("slic_triplet_select", *with_("slic_triplet_select", a7=1, a8=None))
    refused("slic_triplet_select_cross", *with_("slic_triplet_select_cross", a8=4))
    for name, i in [("slic_nce_scores_fwd", 5), ("slic_nce_scores_bwd", 5), ("slic_nce_fused_fwd", 7), ("slic_nce_fused_bwd", 5)]:
        refused(name, *with_(name, **{f"a{i}": 6}))                            # D % 4
    refused("slic_nce_fused_update", *with_("slic_nce_fused_update", a11=None))          # part set, lse NULL
    assert lib.slic_ntxent_workspace_bytes(5, 6) == 256 + 3 * 256
    # the table above, and the list in the GPU module's docstring, name every entry point of the two files
    import os
    import re
    csrc = os.path.join(os.path.dirname(_lib.__file__), "csrc")
    declared = set()
    for src in ("loss.hip", "nce.hip"):
        with open(os.path.join(csrc, src)) as fh:
            declared |= set(re.findall(r'extern "C" \w+ (slic_\w+)\(', fh.read()))
    assert declared == set(valid) | {"slic_ntxent_workspace_bytes"}, declared ^ set(valid)
    assert all(name in G.__doc__ for name in declared)

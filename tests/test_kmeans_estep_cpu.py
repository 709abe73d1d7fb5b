"""CPU: the mirror of the k-means E-step's structure (tests/kmeans_estep_ref.py) through the cases and gates of
tests/test_kmeans_estep_gpu.py, the mutation table, the slice walk of the register kernel as a partition of the rows, the score
matrix of the oracle against its own argmin, and the host-side argument rules of the E-step entry points and of the plan query
(the library loads without a device).

  defect                     caught by (tests/test_kmeans_estep_gpu.py)
  tie_le                     check_ties natural (the copies 128 apart sit in two lists)
  lane_tie_le                check_ties natural (centroids 1 and 2: two slots of one lane)
  wave_tie_le                check_ties_creg (centroids 16 and 48: two waves of one workgroup)
  half_tie_high              check_ties perm, DMA route (centroids 8 and 12: the two lane halves)
  pad_zero                   check_assign natural (300, 257, 24): the all-zero row
  combine_skip_tail          check_assign perm (129, 321, 40): six lists, the rows near centroid 320
  combine_from_1             check_assign natural (300, 257, 24)
  nch_set                    check_assign natural (300, 641, 32): n_changed starts at 12345
  nch_past_n                 check_assign natural (300, 641, 32): 300 is no multiple of 256
  ld_dense                   check_operands natural (ldx = D + 8, NaN in the padding)
  slice_drop_partial_tile    check_creg D = 8 (a last tile of one sub-tile)
  nan_sentinel               check_nan_rows natural
  hist_drop_last_block       check_local N = 1025, SLIC_KM_SCAN=0"""
import numpy as np
import pytest

import kmeans_estep_ref as E
import test_kmeans_estep_gpu as G
from oracle import kmeans as ok

F32 = np.float32


def test_the_mirror_passes_every_check(monkeypatch):
    """every case of the GPU module on the unmutated mirror standing for 256 compute units: all of them pass, and together they
    reach everything the module's coverage test asks for"""
    G.COVER.clear()
    G.UNREACHABLE.clear()
    G.all_checks(E.Mirror(cus=256), monkeypatch)
    missing, text = G.coverage_report()
    print(text)
    assert not missing and not G.UNREACHABLE, (missing, G.UNREACHABLE)
    assert not G.unreachable_cover(256)
    G.COVER.clear()


@pytest.mark.parametrize("cus", (64, 255, 304))
def test_the_register_route_cases_follow_the_cu_count(cus, monkeypatch):
    """other CU counts (a partitioned device, an odd count, a larger part): the search still finds register-route shapes, every
    case passes on the mirror, and whatever the coverage misses is exactly what the reachability sweep says cannot be reached"""
    G.COVER.clear()
    G.UNREACHABLE.clear()
    m = E.Mirror(cus=cus)
    for D in (8, 136):
        shapes = G.check_creg(m, D)
        assert shapes and all(m.estep_plan(N, K, D, D)[0] == 1 for N, K in shapes)
    G.check_ties_creg(m)
    G.check_nan_rows_creg(m)
    missing = {c for c in G.required_cover() if c[0] == "creg" and c[1] in (4, 8)} - G.COVER
    assert missing <= G.unreachable_cover(cus), (cus, missing - G.unreachable_cover(cus))
    G.COVER.clear()
    G.UNREACHABLE.clear()


MUTATIONS = [
    ("tie_le", lambda m, e: G.check_ties(m, "natural", 300, 700, 8)),
    ("lane_tie_le", lambda m, e: G.check_ties(m, "natural", 300, 700, 8)),
    ("wave_tie_le", lambda m, e: G.check_ties_creg(m)),
    ("half_tie_high", lambda m, e: G.check_ties(m, "perm", 300, 400, 8, "dma")),
    ("pad_zero", lambda m, e: G.check_assign(m, "natural", 300, 257, 24)),
    ("combine_skip_tail", lambda m, e: G.check_assign(m, "perm", 129, 321, 40, expect="dma")),
    ("combine_from_1", lambda m, e: G.check_assign(m, "natural", 300, 257, 24)),
    ("nch_set", lambda m, e: G.check_assign(m, "natural", 300, 641, 32)),
    ("nch_past_n", lambda m, e: G.check_assign(m, "natural", 300, 641, 32)),
    ("ld_dense", lambda m, e: G.check_operands(m, "natural", 300, 257, 40)),
    ("slice_drop_partial_tile", lambda m, e: G.check_creg(m, 8)),
    ("nan_sentinel", lambda m, e: G.check_nan_rows(m, "natural", 300, 257, 40)),
    ("hist_drop_last_block", lambda m, e: G.check_local(m, e, 1025, "0", False)),
]


def test_the_table_names_every_defect_of_the_mirror():
    listed = [d for d, _ in MUTATIONS]
    assert sorted(listed) == sorted(E.DEFECTS), set(listed) ^ set(E.DEFECTS)
    documented = {ln.split()[0] for ln in __doc__.split("caught by")[1].splitlines()[1:] if ln.startswith("  ")}
    assert documented == set(E.DEFECTS), documented ^ set(E.DEFECTS)


@pytest.mark.parametrize("defect,check", MUTATIONS, ids=[d for d, _ in MUTATIONS])
def test_defect_is_caught(defect, check, monkeypatch):
    check(E.Mirror(), monkeypatch)                        # the case passes on the mirror as it is ...
    with pytest.raises(AssertionError):                   # ... and fails with the one defect
        check(E.Mirror(defect), monkeypatch)


def test_defects_of_the_merges_are_caught_on_every_route(monkeypatch):
    """the tie cases of all three kernels see a '<=' in km_combine; the short last tile and the sentinel are seen on the permuted
    routes too; both histogram forms of lloyd_step and the slab of lloyd_local see a block missing from the histogram"""
    for check in (lambda m: G.check_ties(m, "perm", 300, 400, 8, "dma"), G.check_ties_creg):
        check(E.Mirror())
        with pytest.raises(AssertionError):
            check(E.Mirror("tie_le"))
    for D in (136, 264):
        with pytest.raises(AssertionError):
            G.check_creg(E.Mirror("slice_drop_partial_tile"), D)
    for check in (lambda m: G.check_nan_rows(m, "perm", 300, 257, 40, "dma"), G.check_nan_rows_creg):
        with pytest.raises(AssertionError):
            check(E.Mirror("nan_sentinel"))
    with pytest.raises(AssertionError):
        G.check_operands(E.Mirror("ld_dense"), "perm", 300, 257, 40, "dma")
    for N, D, K in G.STEP_HIST:
        with pytest.raises(AssertionError):
            G.check_step_hist(E.Mirror("hist_drop_last_block"), N, D, K)
    for N in (1, 1023, 2049):
        with pytest.raises(AssertionError):
            G.check_local(E.Mirror("hist_drop_last_block"), monkeypatch, N, "0", True)
    G.check_local(E.Mirror("hist_drop_last_block"), monkeypatch, 1024, "0", False)          # no ragged block: nothing to drop
    G.check_local(E.Mirror("hist_drop_last_block"), monkeypatch, 1025, None, False)         # the small-shard route has no histogram
    G.COVER.clear()


# ------------------------------------------------------------------ the slice walk
def test_slice_walk_covers_every_row_exactly_once():
    """for a sweep of (N, slices): the rows the slices write are [0, N), each once; ntile and npt_last describe u1 - u0"""
    for slices in (1, 2, 3, 5, 8, 64, 128):
        for N in list(range(1, 700)) + [4095, 4096, 4097, 12365, 100000]:
            if slices > -(-N // 128):                    # the plan never asks for more slices than tiles
                continue
            rows = E.slice_rows(N, slices)
            allr = np.concatenate(rows)
            assert len(allr) == N and np.array_equal(np.sort(allr), np.arange(N)), (N, slices)
            for s in E.slice_walk(N, slices):
                assert s["ntile"] >= 1 and 1 <= s["npt_last"] <= 4 and 4 * (s["ntile"] - 1) + s["npt_last"] == s["u1"] - s["u0"]
                assert s["pbeg"] < s["pend"] <= N
    # with the defect, a slice whose last tile is short loses exactly that tile's rows
    rows = np.concatenate(E.slice_rows(283, 2, frozenset({"slice_drop_partial_tile"})))
    assert len(rows) == 256 and rows.max() == 255


# ------------------------------------------------------------------ the scores and the merges against the oracle's argmin
def test_scores_are_the_chain_of_assign():
    """first minimum and minimum of ok.scores == labels and winning score of ok.assign, bit for bit; every route of the mirror
    reduces the same matrix to the same answer"""
    rng = np.random.default_rng(4)
    for N, K, D in ((37, 1, 8), (130, 65, 24), (70, 300, 136), (50, 641, 520)):
        X, C = rng.standard_normal((N, D)).astype(F32), rng.standard_normal((K, D)).astype(F32)
        C[K // 2] = C[0]                                 # an exact tie somewhere
        S = ok.scores(X, C)
        lab, best, _ = ok.assign(X, C, with_scores=True)
        assert np.array_equal(S.argmin(1).astype(np.int32), lab) and G.bits_equal(S.min(1), best)
        for kind in ("natural", "dma", "creg"):
            ps, pi = (E.creg_lists(S, K, 1) if kind == "creg" and N >= 128 else E.partial_lists(S, K, kind))
            l2, b2, nch = E.combine(ps, pi, K, None, 5)
            assert np.array_equal(l2, lab) and G.bits_equal(b2, best) and nch == 5, (N, K, D, kind)


def test_plan_of_the_mirror_on_known_shapes():
    """the bench row's shape takes the register kernel on 256 CUs (4 blocks x 64 slices) and the DMA tile on 64; D > 512 and a K
    that pads more than 1 / 8 never take it"""
    assert E.plan(100000, 500, 512, 512, 256) == (1, 16, 64, 4, 4, 256)
    assert E.plan(12365, 500, 512, 512, 256) == (1, 16, 64, 4, 4, 256)
    assert E.plan(12365, 500, 512, 512, 64)[0] == 1 and E.plan(1200, 500, 512, 512, 256)[0] == 0
    assert E.plan(100000, 500, 520, 520, 256) == (0, 0, 0, 8, 8, 256)
    assert E.plan(100000, 400, 8, 8, 256)[0] == 0 and E.plan(100000, 448, 8, 8, 256)[0] == 1
    assert E.plan(400, 128 * 128 - 3, 8, 8, 256)[:5] == (1, 4, 2, 128, 128)


# ------------------------------------------------------------------ host argument rules (no device needed)
def test_host_argument_rules():
    import torch
    from video_similarity_search_amd import _lib
    assert G.check_estep_argument_rules(_lib.load(), torch.cuda.is_available()) >= 60

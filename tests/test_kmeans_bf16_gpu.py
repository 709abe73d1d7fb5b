"""GPU: the certified bf16 E-step of k-means against the fp32 E-step and the CPU oracle.  Bar: labels, n_changed and everything
downstream (sums, counts, centres, norms, shift, status, payloads, whole fits) equal to the bit; the statistics say which path ran."""
import os

import numpy as np
import pytest
import torch

import kmeans_bf16_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fp32_side_is_fp32(monkeypatch):
    monkeypatch.delenv("SLIC_KMEANS_BF16", raising=False)


def _both(X, C, seed=0):
    """one E-step through slic_kmeans_assign_bf16 and one through slic_kmeans_assign -> (labels, n_changed) of each, stats of the first"""
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd._lib import call, ptr, stream
    from video_similarity_search_amd.clustering.kmeans_hip import HipKernels
    k = HipKernels()
    lib = _lib.load()
    N, D = X.shape
    K = C.shape[0]
    Xd, Cd = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
    old = torch.from_numpy(np.random.default_rng(seed).integers(0, K, N).astype(np.int32)).cuda()
    cn = torch.empty(K, device="cuda")
    k.cnorm(Cd, cn)
    Xb, xn = k.bf16_image(Xd, want_norms=True)
    Cb, _ = k.bf16_image(Cd)
    assert Xb.shape == (N, (D + 15) // 16 * 16)
    stats = torch.zeros(3, dtype=torch.int32, device="cuda")
    lab_b = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    nch_b = torch.zeros(1, dtype=torch.int32, device="cuda")
    k.assign_bf16(Xd, Xb, xn, Cd, Cb, cn, lab_b, old, nch_b, stats)
    lab_f = torch.full((N,), -9, dtype=torch.int32, device="cuda")
    nch_f = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.slic_kmeans_assign_workspace_bytes(N, K), dtype=torch.uint8, device="cuda")
    call("slic_kmeans_assign", ptr(Xd), N, D, D, ptr(Cd), K, D, ptr(cn), ptr(lab_f), ptr(old), ptr(nch_f), None, ptr(ws), stream())
    torch.cuda.synchronize()
    return lab_b, int(nch_b.item()), lab_f, int(nch_f.item()), stats.cpu().tolist()


@pytest.mark.parametrize("N,K,D", ref.SHAPES)
def test_gaussian_rows_match_fp32_and_oracle(gpu, N, K, D):
    from oracle import kmeans as ok
    X, C = ref.gaussian_rows(N, K, D, N + K + D)
    lab_b, nch_b, lab_f, nch_f, stats = _both(X, C)
    assert torch.equal(lab_b, lab_f)
    assert np.array_equal(lab_b.cpu().numpy(), ok.assign(X, C))
    assert nch_b == nch_f
    print("N=%d K=%d D=%d stats %s" % (N, K, D, stats))
    assert stats[0] > 0                                              # the rescore path ran
    assert stats[1] <= stats[0] and stats[2] >= N


@pytest.mark.parametrize("N,K,D", ref.SHAPES)
def test_blobs_need_no_rescoring(gpu, N, K, D):
    """tests/test_kmeans_bf16_cpu.py shows on the host emulation that every row of these inputs has exactly one candidate, with room"""
    from oracle import kmeans as ok
    X, C = ref.blobs(N, K, D)
    lab_b, nch_b, lab_f, nch_f, stats = _both(X, C)
    assert torch.equal(lab_b, lab_f)
    assert np.array_equal(lab_b.cpu().numpy(), ok.assign(X, C))
    assert nch_b == nch_f
    assert stats == [0, 0, N]


def test_ties_take_the_first_index(gpu):
    N, K, D = 2048, 500, 512
    X, C = ref.gaussian_rows(N, K, D, 11)
    C[200] = C[3]                                                    # an exact copy in another 128-centroid block
    C[401] = C[7]
    C[401, 5] = np.nextafter(C[401, 5], np.float32(np.inf))          # one ulp away in one coordinate
    C[9] = C[300]                                                    # the copy has the LOWER index
    lab_b, nch_b, lab_f, nch_f, stats = _both(X, C)
    assert torch.equal(lab_b, lab_f) and nch_b == nch_f
    lb = lab_b.cpu().numpy()
    assert not np.any(lb == 200) and np.any(lb == 3)
    assert not np.any(lb == 300) and np.any(lb == 9)
    assert stats[0] >= int(np.sum((lb == 3) | (lb == 9)))            # a row nearest to a tied pair cannot be decided by the bf16 pass
    # all-equal scores: every centroid a candidate of every row, label 0
    lab_b, _, lab_f, _, _ = _both(np.ones((300, 16), np.float32), np.zeros((140, 16), np.float32))
    assert torch.equal(lab_b, lab_f) and int(lab_b.abs().max().item()) == 0


def test_overflow_runs_the_exact_chain_over_all_centroids(gpu):
    N, K, D = 261, 500, 512
    rng = np.random.default_rng(5)
    u = rng.standard_normal(D)
    u /= np.linalg.norm(u)
    C = (u[None, :] + 1e-4 * rng.standard_normal((K, D))).astype(np.float32)
    X = rng.standard_normal((N, D)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    lab_b, nch_b, lab_f, nch_f, stats = _both(X, C)
    assert torch.equal(lab_b, lab_f) and nch_b == nch_f
    assert stats[1] == N and stats[0] == N and stats[2] == N * K


def test_nan_rows_and_bad_shapes(gpu):
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.clustering.kmeans_hip import HipKernels
    X, C = ref.gaussian_rows(300, 40, 64, 3)
    X[17] = np.nan
    lab_b, _, lab_f, _, _ = _both(X, C)
    assert torch.equal(lab_b, lab_f)
    k = HipKernels()
    Xd = torch.randn(64, 520, device="cuda")
    with pytest.raises(_lib.SlicError):                              # the C entry refuses; it does not switch precision
        k.bf16_image(Xd)


def _step_buffers(N, K, D):
    z = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="cuda")
    return dict(labels=z(N, dt=torch.int32), n_changed=torch.zeros(1, dtype=torch.int32, device="cuda"), sums=z(K * D), counts=z(K),
                C_new=z(K, D), Cp_new=z(K, D), cnorm_new=z(K), shift=z(K), status=z(4, dt=torch.float64))


@pytest.mark.parametrize("N,K,D,spherical", [(4099, 130, 264, False), (2048, 500, 512, True), (1037, 5, 8, False), (40000, 500, 512, False)])
def test_iteration_calls_equal_fp32(gpu, N, K, D, spherical):
    """(40000 rows: the shard is past km_scan_accumulate's limit, so the histogram the E-step hands to the counting sort is compared too)"""
    from video_similarity_search_amd.clustering.kmeans_hip import HipKernels
    k = HipKernels()
    X, C = ref.gaussian_rows(N, K, D, 2 * N + K)
    Xd, Cd = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
    Xp, Cp = torch.empty_like(Xd), torch.empty_like(Cd)
    k.permute_k8(Xd, Xp)
    k.permute_k8(Cd, Cp)
    cn = torch.empty(K, device="cuda")
    k.cnorm(Cd, cn)
    old = torch.from_numpy(np.random.default_rng(1).integers(0, K, N).astype(np.int32)).cuda()
    Xb, xn = k.bf16_image(Xd, want_norms=True)
    Cimg = torch.empty(K, Xb.shape[1], dtype=torch.int16, device="cuda")
    stats = torch.zeros(3, dtype=torch.int32, device="cuda")
    f, b = _step_buffers(N, K, D), _step_buffers(N, K, D)
    sph = dict(spherical=True) if spherical else {}
    k.lloyd_step(Xd, Xp, Cd, Cp, cn, f["labels"], old, f["n_changed"], f["sums"], f["counts"], f["C_new"], f["Cp_new"], f["cnorm_new"],
                 f["shift"], f["status"], **sph)
    k.lloyd_step_bf16(Xd, Xp, Xb, xn, Cd, Cimg, cn, b["labels"], old, b["n_changed"], b["sums"], b["counts"], b["C_new"], b["Cp_new"],
                      b["cnorm_new"], b["shift"], b["status"], stats, **sph)
    torch.cuda.synchronize()
    for name in f:
        assert torch.equal(f[name], b[name]), name
    assert stats.cpu().tolist()[2] >= N
    for dt in (torch.float32, torch.float64):
        pf = torch.empty(K * D + K + 2, dtype=dt, device="cuda")
        pb = torch.empty_like(pf)
        lf, lb = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, dtype=torch.int32, device="cuda")
        k.lloyd_local(Xd, Xp, Cd, Cp, cn, lf, old, pf)
        k.lloyd_local_bf16(Xd, Xp, Xb, xn, Cd, Cimg, cn, lb, old, pb, stats)
        torch.cuda.synchronize()
        assert torch.equal(lf, lb) and torch.equal(pf, pb), dt


@pytest.mark.parametrize("name", ["unstructured", "clustered_empty", "d128"])
def test_fit_matches_fp32_oracle_and_golden(gpu, golden_dir, name):
    from oracle import kmeans as ok
    from video_similarity_search_amd.clustering import KMeans
    g = dict(np.load(os.path.join(golden_dir, f"kmeans_{name}.npz")))
    X, init = g["X"], g["init"]
    kb = KMeans(n_clusters=init.shape[0], init=init, n_init=1, trace=True, precision="bf16").fit(torch.from_numpy(X))
    kf = KMeans(n_clusters=init.shape[0], init=init, n_init=1, trace=True).fit(torch.from_numpy(X))
    assert kf.bf16_stats_ is None
    mean = ok.col_mean(X)
    r = ok.lloyd(X - mean, init - mean, tol_abs=ok.tolerance(X - mean, 1e-4), trace=True)
    assert kb.n_iter_ == r["n_iter"] == int(g["n_iter"]) and kb.strict_ == r["strict"]
    assert np.array_equal(kb.trace_, r["trace"])
    assert np.array_equal(kb.labels_, r["labels"]) and np.array_equal(kb.labels_, g["labels"]) and kb.labels_.dtype == np.int32
    np.testing.assert_allclose(kb.cluster_centers_, r["centers"] + mean, rtol=0, atol=0)
    assert kb.inertia_ == pytest.approx(r["inertia"], rel=1e-12)
    if name == "clustered_empty":
        assert kb.n_relocations_ >= 1 and kb.n_relocations_ == r["n_relocations"]
    assert np.array_equal(kb.labels_, kf.labels_) and np.array_equal(kb.cluster_centers_, kf.cluster_centers_)
    assert kb.n_iter_ == kf.n_iter_ and kb.inertia_ == kf.inertia_
    st = kb.bf16_stats_
    assert set(st) == {"rows_rescored", "rows_overflowed", "candidates"} and st["candidates"] >= X.shape[0] * kb.n_iter_
    assert st["rows_overflowed"] <= st["rows_rescored"]


@pytest.mark.parametrize("method", ["kmeans", "spherical_kmeans"])
def test_fit_cluster_passes_precision_through(gpu, method):
    from video_similarity_search_amd.clustering import fit_cluster
    rng = np.random.default_rng(2)
    emb = torch.from_numpy(rng.standard_normal((3000, 72)).astype(np.float32)).cuda()
    init = emb[:24].cpu().numpy().copy()
    lf = fit_cluster(emb, method, k=24, n_init=1, init=init)
    assert fit_cluster.last_model.bf16_stats_ is None
    lb = fit_cluster(emb, method, k=24, n_init=1, init=init, precision="bf16")
    assert fit_cluster.last_model.bf16_stats_ is not None
    assert np.array_equal(lf, lb)


def test_env_switch_and_domain(gpu, monkeypatch):
    from video_similarity_search_amd.clustering import KMeans
    X, C = ref.gaussian_rows(1500, 20, 40, 9)
    with pytest.raises(ValueError):
        KMeans(4, precision="bf16").fit(torch.randn(64, 520).cuda())
    monkeypatch.setenv("SLIC_KMEANS_BF16", "1")
    ke = KMeans(20, init=C, n_init=1).fit(torch.from_numpy(X))
    assert ke.bf16_stats_ is not None
    kw = KMeans(4, n_init=1, max_iter=2, random_state=0).fit(torch.randn(64, 520).cuda())      # outside the domain: the forced switch stays off
    assert kw.bf16_stats_ is None
    monkeypatch.delenv("SLIC_KMEANS_BF16")
    kf = KMeans(20, init=C, n_init=1).fit(torch.from_numpy(X))
    assert kf.bf16_stats_ is None and np.array_equal(kf.labels_, ke.labels_) and kf.n_iter_ == ke.n_iter_

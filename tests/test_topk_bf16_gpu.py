"""GPU: the certified bf16 candidate search (cosine_topk(..., precision="bf16"), csrc/topk_bf16.h) returns the exact top-k: against the
float64 oracle, against the fp32 path, on data that certifies (ordinary rows), data that cannot (a crowd inside eps, exact duplicates)
and on the self search.  Every search here runs with SLIC_TOPK_BF16=1, so the bf16 kernels are what is tested whatever the library's
own measured choice for a shape is (info["path"] says which path a call took)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _force_bf16(monkeypatch):
    monkeypatch.setenv("SLIC_TOPK_BF16", "1")               # the library reads the switch at every call


def _search(Q, G, k, precision):
    from video_similarity_search_amd.evaluate import cosine_topk
    info = {}
    idx, dist = cosine_topk(Q, G, k=k, precision=precision, info=info)
    return idx.cpu().numpy(), dist.cpu().numpy(), info


def _agrees_with_fp32(ib, db, ia, da):
    """bf16 path (ib, db) against the fp32 path (ia, da): both are within 3e-6 of the true distances, so slot by slot they differ by at
    most 6e-6, and an index may differ only where the two lists' distances do not — a swap among near-ties"""
    assert np.abs(db - da).max() <= 6e-6
    diff = ib != ia
    assert np.all(np.abs(db[diff] - da[diff]) <= 6e-6)
    return float(diff.mean())


def _vs_oracle(Q, G, idx, dist, k, rng, self_search=False):
    from oracle import retrieval as orr
    sub = rng.choice(Q.shape[0], min(Q.shape[0], 48), replace=False)
    d = orr.cosine_distances(Q[sub].astype(np.float64), G.astype(np.float64))
    if self_search:
        d[np.arange(len(sub)), sub] = np.inf
    ref = np.argsort(d, axis=1, kind="stable")[:, :k]
    np.testing.assert_allclose(dist[sub], np.take_along_axis(d, ref, axis=1), atol=3e-6)
    assert (idx[sub] == ref).mean() > 0.99


@pytest.mark.parametrize("Nq,Ng,D,k,Din", [(300, 40000, 200, 50, 200), (257, 33000, 128, 16, 128), (5, 32768, 64, 20, 64),
                                           (128, 50000, 512, 88, 512), (65, 32781, 104, 1, 100)])
def test_bf16_exact_on_gaussian_rows(gpu, Nq, Ng, D, k, Din):
    """flat Gaussian rows with one zero gallery row; (65, 32781, 104, 1) has inputs of 100 columns (padded to 104, bf16 rows of 112) and
    k = 1, which only the switch reaches.  The fallback share is capped: the test must not pass on the fp32 fallback alone."""
    rng = np.random.default_rng(Nq + Ng + k)
    Q = rng.standard_normal((Nq, Din)).astype(np.float32)
    G = rng.standard_normal((Ng, Din)).astype(np.float32)
    G[3] = 0.0
    ib, db, info = _search(Q, G, k, "bf16")
    ia, da, info32 = _search(Q, G, k, "fp32")
    assert info["path"] == "bf16" and info32["path"] == "fp32"
    print("(%d, %d, %d, k=%d): fallback %d, overflow %d, candidates/query %.1f, eps %.4f"
          % (Nq, Ng, D, k, info["fallback_queries"], info["overflow_queries"], info["candidates"] / Nq, info["eps"]))
    _vs_oracle(Q, G, ib, db, k, rng)
    _agrees_with_fp32(ib, db, ia, da)
    assert (np.diff(db, axis=1) >= 0).all()
    assert info["fallback_queries"] <= 0.10 * Nq
    assert info["candidates"] >= k * (Nq - info["overflow_queries"] - info["fallback_queries"])


def test_bf16_crowd_inside_eps_falls_back(gpu, monkeypatch):
    """every gallery row within eps of every other: no query can be certified (the candidate buffers overflow), all of them are redone by
    the fp32 streaming kernels, and the result is that path's, bit for bit"""
    rng = np.random.default_rng(41)
    v = rng.standard_normal(128).astype(np.float32)
    G = (v[None, :] + 1e-3 * rng.standard_normal((40000, 128))).astype(np.float32)
    Q = (v[None, :] + 1e-3 * rng.standard_normal((64, 128))).astype(np.float32)
    ib, db, info = _search(Q, G, 10, "bf16")
    assert info["path"] == "bf16" and info["fallback_queries"] == 64
    monkeypatch.setenv("SLIC_TOPK_COLLECT", "0")            # the fp32 streaming kernels themselves
    ia, da, _ = _search(Q, G, 10, "fp32")
    monkeypatch.delenv("SLIC_TOPK_COLLECT")
    assert np.array_equal(ib, ia) and np.array_equal(db, da)
    ic, dc, _ = _search(Q, G, 10, "fp32")                  # and the fp32 default
    assert np.array_equal(ib, ic) and np.array_equal(db, dc)


def test_bf16_overflow_with_exact_duplicates(gpu):
    """64 distinct rows x 4096 copies: every score a query reaches is reached 4096 times, the candidate buffers (2048 slots) overflow and
    every query is redone by the streaming kernels — exact, ties to the lower index"""
    from oracle import retrieval as orr
    rng = np.random.default_rng(3)
    base = rng.standard_normal((64, 64)).astype(np.float32)
    G = np.tile(base, (4096, 1))                            # row i = base[i % 64]
    Q = rng.standard_normal((200, 64)).astype(np.float32)
    k = 50
    ib, db, info = _search(Q, G, k, "bf16")
    assert info["path"] == "bf16" and info["overflow_queries"] == 200 and info["fallback_queries"] == 200
    d = orr.cosine_distances(Q.astype(np.float64), base.astype(np.float64))
    best = np.argmin(d, axis=1)
    assert np.array_equal(ib, best[:, None] + 64 * np.arange(k)[None, :])


def test_bf16_self_search(gpu):
    rng = np.random.default_rng(77)
    X = rng.standard_normal((33000, 128)).astype(np.float32)
    ib, db, info = _search(X, None, 5, "bf16")
    ia, da, _ = _search(X, None, 5, "fp32")
    assert info["path"] == "bf16" and info["fallback_queries"] <= 3300
    assert not np.any(ib == np.arange(33000)[:, None])
    _agrees_with_fp32(ib, db, ia, da)
    _vs_oracle(X, X, ib, db, 5, rng, self_search=True)


def test_bf16_clustered_gallery(gpu):
    """40 directions + 0.05 noise: crowds of near-equal scores around every query.  Exact all the same; how many queries the certificate
    leaves to the fallback is recorded, not bounded"""
    rng = np.random.default_rng(2025)
    Ng, D, k, Nq = 40000, 256, 50, 300
    cent = rng.standard_normal((40, D)).astype(np.float32)
    G = (cent[rng.integers(0, 40, Ng)] + 0.05 * rng.standard_normal((Ng, D))).astype(np.float32)
    Q = (G[rng.integers(0, Ng, Nq)] + 0.3 * rng.standard_normal((Nq, D))).astype(np.float32)
    ib, db, info = _search(Q, G, k, "bf16")
    ia, da, _ = _search(Q, G, k, "fp32")
    assert info["path"] == "bf16"
    print("clustered gallery: fallback share %.3f (overflowed %d of %d), candidates/query %.1f"
          % (info["fallback_queries"] / Nq, info["overflow_queries"], Nq, info["candidates"] / Nq))
    _agrees_with_fp32(ib, db, ia, da)
    _vs_oracle(Q, G, ib, db, k, rng)


def test_bf16_is_deterministic(gpu):
    rng = np.random.default_rng(5)
    Q = rng.standard_normal((300, 200)).astype(np.float32)
    G = rng.standard_normal((40000, 200)).astype(np.float32)
    i1, d1, _ = _search(Q, G, 50, "bf16")
    i2, d2, _ = _search(Q, G, 50, "bf16")
    assert np.array_equal(i1, i2) and np.array_equal(d1.view(np.int32), d2.view(np.int32))


def test_bf16_k_too_large_fails_loudly(gpu):
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.evaluate import cosine_topk
    x = torch.randn(40000, 64)
    with pytest.raises(_lib.SlicError):
        cosine_topk(x[:10], x, k=89, precision="bf16")
    with pytest.raises(_lib.SlicError):
        cosine_topk(x[:10], x, k=89)


def test_bf16_passes_through_the_callers(gpu, golden_dir):
    from video_similarity_search_amd.evaluate import topk_retrieval, topk_acc_device, get_topk_acc_from_embeddings
    g = dict(np.load(os.path.join(golden_dir, "retrieval.npz")))
    hits = topk_retrieval(X_train=g["X_train"], y_train=g["y_train"], X_test=g["X_test"], y_test=g["y_test"], ks=list(g["ks"]),
                          precision="bf16")
    assert [hits[int(k)] for k in g["ks"]] == list(g["topk_correct"])
    rng = np.random.default_rng(11)
    Q = rng.standard_normal((300, 200)).astype(np.float32)
    G = rng.standard_normal((40000, 200)).astype(np.float32)
    ql, gl = rng.integers(0, 50, 300), rng.integers(0, 50, 40000)
    a32 = topk_acc_device(Q, ql, G, gl)
    a16 = topk_acc_device(Q, ql, G, gl, precision="bf16")
    assert np.array_equal(a32, a16)
    assert np.array_equal(get_topk_acc_from_embeddings(Q, ql, G, gl, precision="bf16"), a32)

"""CPU: the certified bf16 E-step of k-means — its ABI, its plan query, the Python switches, and, on a host emulation of what the kernel
computes (tests/kmeans_bf16_ref.py), the two facts its exactness rests on: |cs - s| <= b(i, j) for every pair, and the oracle's label
is always a candidate.  Also the condition the GPU test's separated blobs rely on: exactly one candidate per row, with room."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import kmeans_bf16_ref as ref

NAMES = ["slic_kmeans_bf16_plan", "slic_kmeans_bf16_eps", "slic_kmeans_bf16_image", "slic_kmeans_assign_bf16_workspace_bytes",
         "slic_kmeans_assign_bf16", "slic_kmeans_lloyd_step_bf16_workspace_bytes", "slic_kmeans_lloyd_step_bf16",
         "slic_kmeans_lloyd_local_bf16_workspace_bytes", "slic_kmeans_lloyd_local_bf16"]
U = 2.0 ** -8


def test_header_table_and_library_agree():
    from video_similarity_search_amd import _lib
    txt = open(os.path.join(ROOT, "include", "slic_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, txt), n
        assert n in _lib.SIGNATURES, n
        assert hasattr(lib, n), n
    # the fp32 iteration calls plus image, norms, centre image (and the natural-order centres the exact chain reads) and stats
    assert len(_lib.SIGNATURES["slic_kmeans_lloyd_step_bf16"][1]) == len(_lib.SIGNATURES["slic_kmeans_lloyd_step"][1]) + 3
    assert len(_lib.SIGNATURES["slic_kmeans_lloyd_local_bf16"][1]) == len(_lib.SIGNATURES["slic_kmeans_lloyd_local"][1]) + 4


def test_eps_is_the_one_constant():
    from video_similarity_search_amd import _lib
    lib = _lib.load()
    assert float(lib.slic_kmeans_bf16_eps()) == float(lib.slic_cosine_topk_bf16_eps()) == float(np.float32(0.008))
    # §7f: (2u + u^2) + gamma_D (1 + u)^2 + gamma_D at D = 512 with a unit roundoff of 2^-23 per addition, and the room the fp32 norms
    # (relative error below 1e-4, far above what D * 2^-24 makes of it) take out of the constant
    g = 512 * 2.0 ** -23 / (1 - 512 * 2.0 ** -23)
    assert ((2 * U + U * U) + g * (1 + U) ** 2 + g) * (1 + 1e-4) ** 2 < ref.eps()


def test_plan_answers_without_a_device():
    from video_similarity_search_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int64 * 6)()
    assert lib.slic_kmeans_bf16_plan(100000, 500, 512, out) == 0
    assert list(out) == [1, 512, out[2], 4, 100000 * 512 * 2, 500 * 512 * 2] and out[2] >= 8
    assert lib.slic_kmeans_bf16_plan(1037, 33, 104, out) == 0 and out[0] == 1 and out[1] == 112 and out[3] == 1
    assert lib.slic_kmeans_bf16_plan(1000, 10, 520, out) == 0 and out[0] == 0           # outside the domain: said, not an error
    assert lib.slic_kmeans_bf16_plan(1000, 10, 12, out) == 0 and out[0] == 0
    assert lib.slic_kmeans_bf16_plan(0, 10, 8, out) != 0
    assert b"slic_kmeans_bf16_plan" in lib.slic_last_error()
    assert lib.slic_kmeans_assign_bf16_workspace_bytes(100000, 500) >= 4 * 100000 * (8 + out[2] * 8)


def test_python_switches(monkeypatch):
    from video_similarity_search_amd.clustering import KMeans, fit_cluster
    with pytest.raises(ValueError):
        KMeans(4, precision="bogus")
    with pytest.raises(ValueError):
        fit_cluster(torch.randn(64, 8), "kmeans", k=4, precision="fp16")
    with pytest.raises(ValueError):                                   # before any launch: raised on a host without a device too
        KMeans(4, precision="bf16").fit(torch.randn(64, 520))
    monkeypatch.delenv("SLIC_KMEANS_BF16", raising=False)
    assert KMeans(4)._use_bf16(64) is False and KMeans(4, precision="bf16")._use_bf16(64) is True
    assert KMeans(4).bf16_stats_ is None
    monkeypatch.setenv("SLIC_KMEANS_BF16", "1")
    assert KMeans(4)._use_bf16(64) is True and KMeans(4)._use_bf16(520) is False      # forced only inside the domain
    assert KMeans(4, precision="fp32")._use_bf16(64) is False                       # the caller's word wins
    monkeypatch.setenv("SLIC_KMEANS_BF16", "0")
    assert KMeans(4)._use_bf16(64) is False


def _midpoint_row(D, norm):
    """§7e's tight construction: every entry 2^e (1 + 2^-8), a tie that rounds down by nearly the whole unit roundoff; the exponents are
    the base-4 digits of the squared norm asked for, largest first (scaling a unit row by 0.1 or 3 would move the entries off the ties)"""
    T = norm ** 2 * (1.0 + 2.0 ** -8) ** -2
    acc, ex = 0.0, []
    for _ in range(D):
        rem = T - acc
        e = max(int(np.floor(np.log2(rem) / 2)) if rem > 4.0 ** -40 else -40, -40)
        ex.append(e)
        acc += 4.0 ** e
    return np.array([2.0 ** e * (1.0 + 2.0 ** -8) for e in ex], np.float64)


def _inputs(D):
    rng = np.random.default_rng(100 + D)
    N, K = 160, 48
    g = rng.standard_normal((N, D)).astype(np.float32)
    yield "gaussian", g, g[rng.choice(N, K, replace=False)].copy()
    Xn, Cn = ref.gaussian_rows(N, K, D, D)
    yield "centred", (2.5 * Xn).astype(np.float32), (2.5 * Cn + 0.01 * rng.standard_normal((K, D))).astype(np.float32)
    cent = rng.standard_normal((12, D))
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    Xc = (cent[rng.integers(0, 12, N)] + 0.35 * rng.standard_normal((N, D)) / np.sqrt(D)).astype(np.float32)
    Xc -= Xc.mean(0)
    yield "clustered", Xc, Xc[rng.choice(N, K, replace=False)].copy()
    ms, ml = _midpoint_row(D, 0.1), _midpoint_row(D, 3.0)
    T64 = np.stack([ms, ml, -ms, -ml])
    T = T64.astype(np.float32)
    assert np.array_equal(T.astype(np.float64), T64)                 # the ties are fp32 numbers
    nr = np.linalg.norm(T64[:2], axis=1)
    assert 0.097 < nr[0] <= 0.1 * (1 + 1e-12) and 2.9 < nr[1] <= 3.0 * (1 + 1e-12)
    yield "tight", T, np.concatenate([T, g[:4]]).astype(np.float32)


@pytest.mark.parametrize("D", [8, 104, 512])
def test_bound_holds_and_argmin_is_a_candidate(D):
    from oracle import kmeans as ok
    for name, X, C in _inputs(D):
        s = ref.exact_scores(X, C)
        cs, b = ref.coarse(X, C)
        err = np.abs(cs.astype(np.float64) - s.astype(np.float64))
        ratio = float((err / b).max())
        cand, ub, lo = ref.candidates(cs, b)
        lab = ok.assign(X, C)
        print("D=%d %-9s max |cs - s| / b = %.3f   candidates per row: mean %.2f max %d" % (D, name, ratio, cand.sum(1).mean(), cand.sum(1).max()))
        assert (err <= b).all(), (name, ratio)
        assert cand[np.arange(len(lab)), lab].all(), name
        # every centroid that ties with the argmin in the exact score is a candidate too ("first index wins" survives)
        ties = s == s[np.arange(len(lab)), lab][:, None]
        assert cand[ties].all(), name
        if name == "tight" and D >= 104:
            # not padded: the dominant term is met to within a few per cent (2 eps |x| |c| against 2 * 0.994 * 2u |x| |c| on x = c)
            assert ratio > 0.9


@pytest.mark.parametrize("N,K,D", ref.SHAPES)
def test_blobs_have_one_candidate_with_room(N, K, D):
    """what tests/test_kmeans_bf16_gpu.py's blob case relies on — stats == {0, 0, N} — holds by this emulation alone: one candidate per
    row, and the runner-up's cs - b clears ub by far more than a different fp32 summation order inside the MFMA could move either
    (each dot by at most gamma_D |x| |c|, D * 2^-23 relative, so each side of the comparison by 2 gamma_D |x| |c| (1 + 2 eps))"""
    from oracle import kmeans as ok
    X, C = ref.blobs(N, K, D)
    cs, b = ref.coarse(X, C)
    cand, ub, lo = ref.candidates(cs, b)
    assert (cand.sum(1) == 1).all()
    assert np.array_equal(cand.argmax(1), ok.assign(X, C))
    if K > 1:
        runner = np.sort(lo, 1)[:, 1]
        nmax = float(np.linalg.norm(X, axis=1).max() * np.linalg.norm(C, axis=1).max())
        assert ((runner - ub) > 8 * D * 2.0 ** -23 * nmax).all(), float((runner - ub).min())


def test_gaussian_rows_need_rescoring():
    """the other GPU case: rows against K of themselves at the largest test shape — some rows keep several candidates (stats[0] > 0)"""
    N, K, D = ref.SHAPES[-1]
    X, C = ref.gaussian_rows(N, K, D, N + K + D)
    cs, b = ref.coarse(X, C)
    cand, _, _ = ref.candidates(cs, b)
    n = cand.sum(1)
    print("candidates per row: mean %.2f, rows with more than one %.1f %%, max %d" % (n.mean(), 100.0 * (n > 1).mean(), n.max()))
    assert (n > 1).mean() > 0.2

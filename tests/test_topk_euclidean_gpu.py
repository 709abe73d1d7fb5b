"""GPU: euclidean top-k retrieval (slic_euclidean_topk / evaluate.euclidean_topk) against a float64 direct-distance oracle computed
here, the collect and streaming paths against each other, exactness at duplicates / near-duplicates / far-from-origin data, the
drop-in accuracies, the sharded merge, and the cosine path left untouched by euclidean calls in the same process."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dist64(Q, G):
    """[Nq, Ng] float64 euclidean distances of float32 rows (direct form on small inputs, the Gram form on large ones — float64 keeps
    its cancellation far below the tolerances used here)"""
    Q, G = np.asarray(Q, np.float64), np.asarray(G, np.float64)
    if Q.shape[0] * G.shape[0] * Q.shape[1] <= 2e7:
        return np.sqrt(((Q[:, None, :] - G[None, :, :]) ** 2).sum(-1))
    d2 = (Q * Q).sum(1)[:, None] + (G * G).sum(1)[None, :] - 2.0 * Q @ G.T
    return np.sqrt(np.maximum(d2, 0.0))


def _oracle(Q, G, k, self_mask=False):
    d = _dist64(Q, G)
    if self_mask:
        np.fill_diagonal(d, np.inf)
    ref = np.argsort(d, axis=1, kind="stable")[:, :k]
    return d, ref, np.take_along_axis(d, ref, axis=1)


def _check_vs_oracle(idx, dist, d, ref, refd, agree=0.99):
    idx, dist = np.asarray(idx), np.asarray(dist)
    np.testing.assert_allclose(dist, refd, rtol=1e-5, atol=1e-6)
    same = idx == ref
    assert same.mean() >= agree, same.mean()
    # every disagreement is a near-tie: the row returned at that rank lies (in float64) as far as the oracle's row at that rank
    for q, j in np.argwhere(~same):
        got = d[q, idx[q, j]]
        assert abs(got - refd[q, j]) <= 1e-5 * refd[q, j] + 1e-6, (q, j, got, refd[q, j])
    assert (np.diff(dist, axis=1) >= 0).all()


@contextlib.contextmanager
def _collect_env(v):
    old = os.environ.get("SLIC_TOPK_COLLECT")
    os.environ["SLIC_TOPK_COLLECT"] = v
    try:
        yield
    finally:
        if old is None:
            del os.environ["SLIC_TOPK_COLLECT"]
        else:
            os.environ["SLIC_TOPK_COLLECT"] = old


# the cosine tests' shape list: every partial-kernel instantiation (query operand in registers with 4 / 8 / 16 k-tiles, the 2-stage
# ring for D > 512, short pending columns at large k, ragged last slices), a zero gallery row
# (k = 88 leaves 2 or 3 pending slots per lane: topk_partial_qreg<NK, 2, ..>, here with NK = 4, 8 and 16)
@pytest.mark.parametrize("Nq,Ng,D,k", [(1, 50, 8, 50), (129, 1000, 128, 1), (1000, 20000, 512, 20), (33, 257, 40, 7),
                                       (200, 3001, 256, 50), (300, 40000, 200, 50), (64, 2000, 640, 10),
                                       (100, 5000, 512, 88), (130, 700, 1024, 3), (33, 257, 40, 88), (33, 300, 136, 88)])
def test_euclidean_topk_shapes_vs_oracle(gpu, Nq, Ng, D, k):
    from video_similarity_search_amd.evaluate import euclidean_topk
    rng = np.random.default_rng(Nq + Ng + 1)
    Q = rng.standard_normal((Nq, D)).astype(np.float32)
    G = rng.standard_normal((Ng, D)).astype(np.float32)
    G[3] = 0.0
    idx, dist = euclidean_topk(Q, G, k=k)
    _check_vs_oracle(idx.cpu().numpy(), dist.cpu().numpy(), *_oracle(Q, G, k))


def test_euclidean_topk_strided_rows_abi(gpu):
    """the C ABI takes raw rows with a row stride (ldq, ldg > D) and a D that is no multiple of 8"""
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd._lib import call, ptr, stream
    rng = np.random.default_rng(21)
    Nq, Ng, D, k = 70, 3000, 37, 12
    Qb = torch.from_numpy(rng.standard_normal((Nq, 50)).astype(np.float32)).cuda()
    Gb = torch.from_numpy(rng.standard_normal((Ng, 41)).astype(np.float32)).cuda()
    Q, G = Qb[:, :D], Gb[:, :D]
    idx = torch.empty(Nq, k, dtype=torch.int32, device="cuda")
    dist = torch.empty(Nq, k, dtype=torch.float32, device="cuda")
    lib = _lib.load()
    ws = torch.empty(lib.slic_euclidean_topk_workspace_bytes(Nq, Ng, D, k), dtype=torch.uint8, device="cuda")
    call("slic_euclidean_topk", ptr(Q), Nq, Q.stride(0), ptr(G), Ng, G.stride(0), D, k, 0, ptr(idx), ptr(dist), ptr(ws), stream())
    Qh, Gh = Q.cpu().numpy(), G.cpu().numpy()
    _check_vs_oracle(idx.cpu().numpy(), dist.cpu().numpy(), *_oracle(Qh, Gh, k))


# collect (threshold -> collect -> select) and streaming search the same scores with the same tie rule, and the refine sees the same
# candidate set: the lists must be IDENTICAL, bit for bit
@pytest.mark.parametrize("Nq,Ng,D,k", [(300, 40000, 200, 50), (1000, 100000, 512, 50), (257, 65613, 128, 1), (128, 50000, 512, 88)])
def test_euclidean_topk_collect_equals_streaming(gpu, Nq, Ng, D, k):
    from video_similarity_search_amd.evaluate import euclidean_topk
    rng = np.random.default_rng(Nq + Ng + k)
    Q = rng.standard_normal((Nq, D)).astype(np.float32)
    G = rng.standard_normal((Ng, D)).astype(np.float32)
    G[3] = 0.0
    with _collect_env("1"):
        ia, da = [t.cpu().numpy() for t in euclidean_topk(Q, G, k=k)]
    with _collect_env("0"):
        ib, db = [t.cpu().numpy() for t in euclidean_topk(Q, G, k=k)]
    assert np.array_equal(ia, ib) and np.array_equal(da, db)
    sub = rng.choice(Nq, min(Nq, 32), replace=False)
    d, ref, refd = _oracle(Q[sub], G, k)
    _check_vs_oracle(ia[sub], da[sub], d, ref, refd)


def test_euclidean_topk_exact_duplicates(gpu):
    """planted copies of a query come back first, at distance exactly 0, lower gallery index first (on both paths)"""
    from video_similarity_search_amd.evaluate import euclidean_topk
    rng = np.random.default_rng(31)
    for Ng in (5000, 40000):
        Q = rng.standard_normal((40, 128)).astype(np.float32) * 3 + 1
        G = rng.standard_normal((Ng, 128)).astype(np.float32) * 3 + 1
        rows = {}
        for i in range(40):
            r = np.sort(rng.choice(Ng, 1 + i % 3, replace=False))
            G[r] = Q[i]
            rows[i] = r
        for env in ("0", "1"):
            with _collect_env(env):
                idx, dist = [t.cpu().numpy() for t in euclidean_topk(Q, G, k=20)]
            for i, r in rows.items():
                n = len(r)
                assert list(idx[i, :n]) == list(r), (Ng, env, i, idx[i, :n], r)
                assert (dist[i, :n] == 0.0).all()
                assert dist[i, n] > 0.0


def test_euclidean_topk_near_duplicates_ordered(gpu):
    """rows 1e-3 .. 8e-3 away from a query of norm ~30 — far below the fp32 score's resolution — come back in their true order"""
    from video_similarity_search_amd.evaluate import euclidean_topk
    rng = np.random.default_rng(41)
    Nq, Ng, D = 24, 20000, 128
    Q = rng.standard_normal((Nq, D))
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True) * 30).astype(np.float32)
    G = (rng.standard_normal((Ng, D)) * (30 / np.sqrt(D))).astype(np.float32)
    for i in range(Nq):
        r = rng.choice(Ng, 8, replace=False)
        u = rng.standard_normal((8, D))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        G[r] = (Q[i].astype(np.float64) + 1e-3 * rng.permutation(np.arange(1, 9))[:, None] * u).astype(np.float32)
    idx, dist = [t.cpu().numpy() for t in euclidean_topk(Q, G, k=10)]
    d, ref, refd = _oracle(Q, G, 10)
    assert np.array_equal(idx[:, :8], ref[:, :8])
    np.testing.assert_allclose(dist, refd, rtol=1e-5, atol=1e-6)


def test_euclidean_topk_far_from_origin(gpu):
    """data shifted by a common offset of 1e3: the centring pre-pass keeps the ranking, the refine the distances"""
    from video_similarity_search_amd.evaluate import euclidean_topk
    rng = np.random.default_rng(51)
    off = (1e3 * (1 + rng.random(64))).astype(np.float32)
    Q = (rng.standard_normal((60, 64)) + off).astype(np.float32)
    G = (rng.standard_normal((6000, 64)) + off).astype(np.float32)
    idx, dist = euclidean_topk(Q, G, k=30)
    _check_vs_oracle(idx.cpu().numpy(), dist.cpu().numpy(), *_oracle(Q, G, 30))


def test_euclidean_topk_self_search(gpu):
    from video_similarity_search_amd.evaluate import euclidean_topk
    rng = np.random.default_rng(61)
    for N in (700, 33000):
        X = rng.standard_normal((N, 48)).astype(np.float32)
        idx, dist = [t.cpu().numpy() for t in euclidean_topk(X, None, k=20)]
        assert not (idx == np.arange(N)[:, None]).any()
        sub = rng.choice(N, 50, replace=False)
        d = _dist64(X[sub], X)
        d[np.arange(50), sub] = np.inf
        ref = np.argsort(d, axis=1, kind="stable")[:, :20]
        _check_vs_oracle(idx[sub], dist[sub], d, ref, np.take_along_axis(d, ref, axis=1))


def test_euclidean_drop_in_accuracies(gpu, golden_dir):
    from video_similarity_search_amd.evaluate import (get_distance_matrix, get_topk_acc, get_topk_acc_from_embeddings,
                                                      topk_retrieval)
    g = dict(np.load(os.path.join(golden_dir, "retrieval.npz")))
    top_ks = [1, 5, 10, 20]
    X, y = g["X_train"][:500], g["y_train"][:500]
    a = get_topk_acc_from_embeddings(X, y, top_ks=top_ks, dist_metric='euclidean')
    b = get_topk_acc(get_distance_matrix(X, None, 'euclidean'), y, top_ks=top_ks)
    np.testing.assert_array_equal(a, b)
    a = get_topk_acc_from_embeddings(g["X_test"], g["y_test"], g["X_train"], g["y_train"], top_ks=top_ks, dist_metric='euclidean')
    b = get_topk_acc(get_distance_matrix(g["X_test"], g["X_train"], 'euclidean'), g["y_test"], g["y_train"], top_ks=top_ks)
    np.testing.assert_array_equal(a, b)
    ks = [int(k) for k in g["ks"]]
    hits = topk_retrieval(X_train=g["X_train"], y_train=g["y_train"], X_test=g["X_test"], y_test=g["y_test"], ks=ks,
                          dist_metric='euclidean')
    d = _dist64(g["X_test"].astype(np.float32), g["X_train"].astype(np.float32))
    ref = np.argsort(d, axis=1, kind="stable")[:, :max(ks)]
    hit = g["y_train"][ref] == g["y_test"][:, None]
    assert hits == {k: int(hit[:, :k].any(axis=1).sum()) for k in ks}
    with pytest.raises(ValueError):
        get_topk_acc_from_embeddings(X, y, top_ks=top_ks, dist_metric='manhattan')
    with pytest.raises(ValueError):
        topk_retrieval(X_train=X, y_train=y, X_test=X, y_test=y, dist_metric='l1')


def test_euclidean_sharded_merge(gpu):
    """three shards (each centred on its own mean) merged with slic_topk_merge_lists == the unsharded search, bit for bit; and the RCCL
    path on a one-rank group"""
    import torch.distributed as dist
    from video_similarity_search_amd._lib import call, ptr, stream
    from video_similarity_search_amd.evaluate import euclidean_topk, euclidean_topk_sharded
    rng = np.random.default_rng(71)
    Q = rng.standard_normal((200, 64)).astype(np.float32)
    G = (rng.standard_normal((3000, 64)) + np.linspace(0, 3, 3000)[:, None]).astype(np.float32)   # shard means differ
    k = 10
    ref_i, ref_d = euclidean_topk(Q, G, k=k)
    parts_i, parts_d, off = [], [], 0
    for sh in np.array_split(G, 3):
        i, d = euclidean_topk(Q, sh, k=k)
        parts_i.append(i + off)
        parts_d.append(d)
        off += len(sh)
    pi, pd = torch.stack(parts_i).contiguous(), torch.stack(parts_d).contiguous()
    oi, od = torch.empty_like(ref_i), torch.empty_like(ref_d)
    call("slic_topk_merge_lists", ptr(pd), ptr(pi), 3, 200, k, ptr(oi), ptr(od), stream())
    assert torch.equal(oi, ref_i) and torch.equal(od, ref_d)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29578")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        si, sd = euclidean_topk_sharded(Q, G, k, dist.group.WORLD)
        assert torch.equal(si, ref_i) and torch.equal(sd, ref_d)
    finally:
        dist.destroy_process_group()


def test_cosine_unchanged_by_euclidean_calls(gpu):
    """the euclidean instantiations have launch attributes of their own: cosine results before and after euclidean calls (both paths,
    LDS-hungry k = 88 and tiny lists) are identical"""
    from video_similarity_search_amd.evaluate import cosine_topk, euclidean_topk
    rng = np.random.default_rng(81)
    Q = rng.standard_normal((300, 256)).astype(np.float32)
    G = rng.standard_normal((40000, 256)).astype(np.float32)
    cases = [(G, 50, "1"), (G, 88, "0"), (G[:3000], 5, "0"), (G, 20, "1")]

    def cos_all():
        out = []
        for g, k, env in cases:
            with _collect_env(env):
                out.append([t.cpu().numpy() for t in cosine_topk(Q, g, k=k)])
        return out
    before = cos_all()
    for g, k, env in cases:
        for e in ("0", "1"):
            with _collect_env(e):
                euclidean_topk(Q, g, k=k)
    euclidean_topk(rng.standard_normal((50, 700)).astype(np.float32), rng.standard_normal((900, 700)).astype(np.float32), k=88)  # D > 512
    after = cos_all()
    for (ia, da), (ib, db) in zip(before, after):
        assert np.array_equal(ia, ib) and np.array_equal(da, db)


# One process per line of calls (D = 256: the register-operand kernels with 8 k-tiles; LDS bytes from topk_stream / topk_collect):
#   "big"     k = 88 on 5000 rows: streaming, 2 or 3 pending slots per lane -> topk_partial_qreg<8, 2, EU> at 162832 B, the largest size
#   "big4"    k = 40 on 5000 rows: streaming, 27 (euclidean, 48 ranked: 22) pending slots -> topk_partial_qreg<8, 4, EU> at 162832 B
#   "collect" k = 20 on 40000 rows: the collect path launches the SAME topk_partial_qreg<8, 4, EU> twice with smaller sizes — the
#             sample pass (<= 16 entries per list: <= 147 KB) and the exact fallback (k = 20, 32 pending slots: 152592 B, +2048 euclidean)
# so "big4, collect, big4" asks one kernel for 162832, < 150000, 152592 and 162832 bytes again: a limit that followed the last request
# down would refuse the last launch.
_LDS_SEQUENCE_CHILD = """
import sys, numpy as np
from video_similarity_search_amd.evaluate import cosine_topk, euclidean_topk
search = {"cosine": cosine_topk, "euclidean": euclidean_topk}[sys.argv[1]]
rng = np.random.default_rng(91)
Q = rng.standard_normal((300, 256)).astype(np.float32)
G = rng.standard_normal((40000, 256)).astype(np.float32)
calls = {"big": lambda: search(Q, G[:5000], k=88), "big4": lambda: search(Q, G[:5000], k=40), "collect": lambda: search(Q, G, k=20)}
out = {}
for n, call in enumerate(sys.argv[3].split(",")):
    idx, dist = calls[call]()
    out["idx%d" % n], out["dist%d" % n] = idx.cpu().numpy(), dist.cpu().numpy()
np.savez(sys.argv[2], **out)
"""


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_topk_lds_limit_survives_smaller_launches(gpu, tmp_path, metric):
    """k = 88 and k = 40 (the largest LDS size of both streaming instantiations), then a collect-path search whose launches ask the
    k = 40 kernel for less, then k = 40 and k = 88 again, all in ONE process: the smaller requests in between must not lower a
    limit.  Every result equals the same call's result as the first call of a process."""
    import subprocess
    import sys
    from conftest import ROOT
    from video_similarity_search_amd import _lib
    plan = (ctypes.c_int * 6)()
    for k, on in ((20, 1), (28, 1), (40, 0), (48, 0), (88, 0)):          # (28 / 48: what the euclidean search ranks for k = 20 / 40)
        _lib.check(gpu.slic_cosine_topk_plan(300, 40000 if on else 5000, 256, k, plan), "slic_cosine_topk_plan")
        assert plan[0] == on, (k, "the middle search must take the collect path, the others the streaming path")

    def child(calls):
        f = str(tmp_path / (calls.replace(",", "_") + ".npz"))
        env = dict(os.environ, PYTHONPATH=ROOT)
        env.pop("SLIC_TOPK_COLLECT", None)
        r = subprocess.run([sys.executable, "-c", _LDS_SEQUENCE_CHILD, metric, f, calls], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        return dict(np.load(f))
    order = ("big", "big4", "collect", "big4", "big")
    seq = child(",".join(order))
    fresh = {c: child(c) for c in set(order)}
    for n, c in enumerate(order):
        assert np.array_equal(seq["idx%d" % n], fresh[c]["idx0"]) and np.array_equal(seq["dist%d" % n], fresh[c]["dist0"]), (metric, n, c)
    assert [seq["idx%d" % n].shape[1] for n in range(5)] == [88, 40, 20, 40, 88]


def test_euclidean_topk_errors(gpu):
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.evaluate import euclidean_topk
    Q = torch.randn(10, 16, device="cuda")
    G = torch.randn(500, 16, device="cuda")
    idx, _ = euclidean_topk(Q, G, k=88)
    assert idx.shape == (10, 88)
    for k, g in ((0, G), (89, G), (89, G[:100]), (51, G[:50])):
        with pytest.raises(_lib.SlicError):
            euclidean_topk(Q, g, k=k)

"""CPU, world_size 2 over gloo: the N>1 path of the sharded k-means (KMeans(process_group=...)) — ONE collective per
iteration (fp64 all-reduce of [sums | counts | n_changed], or all-gather of the fp32 payloads + rank-ordered combine),
relocation candidate merge — driven with the oracle-backed kernel provider, and checked against the single-process
oracle run with n_shards = -2 (fp64 combine) / 2 (ordered fp32 combine).
Also the reference-shaped collectives of misc/distributed_helper.py."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, case, out_dir, exchange):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.distributed.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", world_size=world, rank=rank)
    try:
        from kmeans_cpu_kernels import OracleKernels
        from video_similarity_search_amd.clustering.kmeans_hip import KMeans
        import video_similarity_search_amd.misc.distributed_helper as du
        g = dict(np.load(case))
        X, init = g["X"], g["init"]
        N = len(X)
        per = (N + world - 1) // world
        shard = torch.from_numpy(X[rank * per:(rank + 1) * per])
        calls = {"n": 0}
        log = []                                                   # the two halves of every iteration and the collectives, in call order
        for fn in ("all_reduce", "all_gather_into_tensor", "all_gather", "broadcast"):
            def counted(*a, _f=getattr(torch.distributed, fn), **kw):
                calls["n"] += 1
                log.append("collective")
                return _f(*a, **kw)
            setattr(torch.distributed, fn, counted)

        class Logged(OracleKernels):
            def lloyd_local(self, *a, **kw):
                log.append("lloyd_local")
                return super().lloyd_local(*a, **kw)

            def lloyd_global(self, *a, **kw):
                log.append("lloyd_global")
                return super().lloyd_global(*a, **kw)

        km = KMeans(n_clusters=init.shape[0], init=init, n_init=1, process_group=torch.distributed.group.WORLD,
                    kernels=Logged(), trace=True, exchange=exchange).fit(shard)
        n_coll = calls["n"]
        with open(os.path.join(out_dir, f"log_r{rank}.txt"), "w") as f:
            f.write("\n".join(log))
        # reference-shaped helpers (misc/distributed_helper.py:41-64)
        t = torch.tensor([float(rank + 1)])
        du.all_reduce([t], avg=True)
        gl = du.all_gather([torch.from_numpy(km.labels_.astype(np.int64))])[0]
        assert abs(t.item() - (world + 1) / 2) < 1e-6 and du.get_world_size() == world
        assert du.is_master_proc() == (rank == 0)
        # cluster-label hand-off as a broadcast (online_train.iterative_cluster_step)
        from video_similarity_search_amd.online_train import broadcast_cluster_labels
        got = broadcast_cluster_labels(gl.numpy() if rank == 0 else None, N, "cpu", rank == 0)
        assert got.dtype == np.int32 and np.array_equal(got, gl.numpy())
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), labels=km.labels_, centers=km.cluster_centers_, n_iter=km.n_iter_,
                 strict=km.strict_, inertia=km.inertia_, all_labels=gl.numpy(), nreloc=km.n_relocations_, n_coll=n_coll)
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("exchange", ["allreduce", "allgather"])
@pytest.mark.parametrize("name", ["clustered_empty", "d128"])
def test_sharded_kmeans_two_ranks_gloo(golden_dir, tmp_path, name, exchange, monkeypatch):
    from oracle import kmeans as ok
    case = os.path.join(golden_dir, f"kmeans_{name}.npz")
    world = 2
    # count the collectives the Lloyd loop issues: the workers log every torch.distributed call they make
    mp.spawn(_worker, args=(world, _free_port(), case, str(tmp_path), exchange), nprocs=world, join=True)
    g = dict(np.load(case))
    X, init = g["X"], g["init"]
    mean = ok.col_mean(X)
    Xc = X - mean
    ref = ok.lloyd(Xc, init - mean, tol_abs=ok.tolerance(Xc, 1e-4), n_shards=-world if exchange == "allreduce" else world)
    r0, r1 = (dict(np.load(os.path.join(tmp_path, f"r{r}.npz"))) for r in range(world))
    labels = np.concatenate([r0["labels"], r1["labels"]])
    assert np.array_equal(labels, ref["labels"])                      # sharded run == oracle with n_shards = 2
    assert np.array_equal(labels, g["labels"])                        # and sklearn's golden
    assert np.array_equal(r0["all_labels"], labels) and np.array_equal(r1["all_labels"], labels)
    assert int(r0["n_iter"]) == int(r1["n_iter"]) == ref["n_iter"]
    assert bool(r0["strict"]) == ref["strict"]
    assert np.array_equal(r0["centers"], r1["centers"])               # every rank holds bit-identical centres
    np.testing.assert_allclose(r0["centers"], ref["centers"] + mean, rtol=0, atol=1e-6)
    assert abs(float(r0["inertia"]) - ref["inertia"]) <= 1e-9 * ref["inertia"]
    if name == "clustered_empty":
        assert int(r0["nreloc"]) >= 1
    else:
        # ONE collective per Lloyd iteration: n_iter + 1 launches (the loop runs one iteration ahead of
        # the host) + the fit's fixed set-up / wrap-up exchanges (shard sizes, column means, tolerance, inertia)
        assert int(r0["n_coll"]) <= int(r0["n_iter"]) + 1 + 6, (int(r0["n_coll"]), int(r0["n_iter"]))
        # the order inside an iteration, on every rank: local half -> the ONE collective -> global half, n_iter + 1 times.  The log is
        # cut at the first local half (before it: the set-up exchanges) and behind the last global half (after it: the inertia's)
        for r in range(world):
            log = open(os.path.join(tmp_path, f"log_r{r}.txt")).read().split("\n")
            loop = log[log.index("lloyd_local"):len(log) - log[::-1].index("lloyd_global")]
            assert loop == ["lloyd_local", "collective", "lloyd_global"] * (int(r0["n_iter"]) + 1), loop


def _failing_worker(rank, world, port, case, out_dir):
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.distributed.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", world_size=world, rank=rank)
    try:
        from kmeans_cpu_kernels import OracleKernels
        from video_similarity_search_amd.clustering.kmeans_hip import KMeans
        g = dict(np.load(case))
        X, init = g["X"], g["init"]
        per = (len(X) + world - 1) // world
        shard = torch.from_numpy(X[rank * per:(rank + 1) * per])

        log = []                                                    # the halves of every iteration and the collectives, in call order
        for fn in ("all_reduce", "all_gather_into_tensor", "all_gather", "broadcast"):
            def counted(*a, _f=getattr(torch.distributed, fn), **kw):
                log.append("collective")
                return _f(*a, **kw)
            setattr(torch.distributed, fn, counted)

        class Failing(OracleKernels):
            n = 0

            def lloyd_local(self, *a, **kw):
                Failing.n += 1
                if rank == 1 and Failing.n == 3:                    # the third iteration's local half of rank 1
                    log.append("lloyd_local FAILED")
                    raise MemoryError("injected: the local half of iteration 2 failed on rank 1")
                log.append("lloyd_local")
                return super().lloyd_local(*a, **kw)

            def lloyd_global(self, *a, **kw):
                log.append("lloyd_global")
                return super().lloyd_global(*a, **kw)

        t0 = time.time()
        msg = "no exception"
        try:
            KMeans(n_clusters=init.shape[0], init=init, n_init=1, max_iter=50, tol=0.0, process_group=torch.distributed.group.WORLD,
                   kernels=Failing()).fit(shard)
        except Exception as e:                                      # noqa: BLE001
            msg = f"{type(e).__name__}: {e}"
        dt = time.time() - t0
        torch.distributed.barrier()      # both ranks get here (each caught its exception): do not tear a socket down under the peer's last receive
        with open(os.path.join(out_dir, f"fail_r{rank}.txt"), "w") as f:
            f.write(f"{dt:.3f}\n{msg}\n")
        with open(os.path.join(out_dir, f"fail_log_r{rank}.txt"), "w") as f:
            f.write("\n".join(log))
    finally:
        torch.distributed.destroy_process_group()


def test_sharded_kmeans_local_failure_reaches_every_rank(golden_dir, tmp_path):
    """a rank whose local half of an iteration raises still enters the iteration's collective with a poisoned payload: it raises the
    cause, its peer raises a SlicError at the same iteration — within seconds, not at the process group's timeout"""
    case = os.path.join(golden_dir, "kmeans_d128.npz")
    mp.spawn(_failing_worker, args=(2, _free_port(), case, str(tmp_path)), nprocs=2, join=True)
    r0 = open(os.path.join(tmp_path, "fail_r0.txt")).read().splitlines()
    r1 = open(os.path.join(tmp_path, "fail_r1.txt")).read().splitlines()
    assert r1[1].startswith("MemoryError: injected"), r1
    assert r0[1].startswith("SlicError") and "peer" in r0[1], r0
    assert float(r0[0]) < 60 and float(r1[0]) < 60
    # the poison rule's order on the failing rank: two whole iterations, then the failed local half is followed by that iteration's
    # collective all the same, and no global half is launched for it or after it
    log = open(os.path.join(tmp_path, "fail_log_r1.txt")).read().split("\n")
    at = log.index("lloyd_local FAILED")
    assert log[log.index("lloyd_local"):at] == ["lloyd_local", "collective", "lloyd_global"] * 2, log
    assert log[at + 1] == "collective" and "lloyd_global" not in log[at:] and "lloyd_local" not in log[at + 1:], log


def test_single_process_driver_matches_oracle_cpu(golden_dir):
    """the host control flow (no process group) with the oracle-backed kernels reproduces the oracle's Lloyd run"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from kmeans_cpu_kernels import OracleKernels
    from oracle import kmeans as ok
    from video_similarity_search_amd.clustering.kmeans_hip import KMeans
    g = dict(np.load(os.path.join(golden_dir, "kmeans_unstructured.npz")))
    km = KMeans(n_clusters=16, init=g["init"], n_init=1, kernels=OracleKernels(), trace=True).fit(torch.from_numpy(g["X"]))
    assert km.n_iter_ == int(g["n_iter"]) and np.array_equal(km.labels_, g["labels"])
    for m in range(1, km.n_iter_):
        assert np.array_equal(km.trace_[m], g["trace"][m - 1])

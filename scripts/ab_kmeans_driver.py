"""Host cost of the k-means driver (clustering/kmeans_hip.py) against another revision of it, on one gfx950 device — the kernels are the
same library, so only host time can differ (table and verdicts: profiles/kmeans_driver_refactor.txt):

    git show REV:video_similarity_search_amd/clustering/kmeans_hip.py > kmeans_parent.py
    python scripts/ab_kmeans_driver.py kmeans_parent.py REV [OUT.txt]

Three drivers alternate, three repeats each: the parent revision, the tree's driver, and a second copy of the parent (an A/A control:
what the condition does to a driver that is the parent).  Per repeat the median of the timed fits; condition per row: the driver's
median over its repeats <= the parent's median + the parent's own spread (its slowest repeat - its fastest).
Rows: the k-means row of bench.py (100k x 512, K = 500, explicit init, 20 fixed iterations: 4 warm-up fits, 5 timed) without a
process group and on a one-rank group with exchange = allreduce / oneshot; fit_cluster(emb, 'kmeans', 500) as bench.py --full calls
it (n_init = 10, k-means++: 1 warm-up, 3 timed) and the same call at 10k x 128, K = 100 (4 warm-up, 5 timed)."""
import contextlib
import importlib.util
import io
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from video_similarity_search_amd.clustering import cluster_masks  # noqa: E402
from video_similarity_search_amd.clustering.kmeans_hip import KMeans as NewKMeans  # noqa: E402


def load_driver(path, name):
    """another revision of clustering/kmeans_hip.py as a sibling module of the package's own (its relative imports resolve)"""
    spec = importlib.util.spec_from_file_location("video_similarity_search_amd.clustering." + name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.KMeans


ParentKMeans = load_driver(sys.argv[1], "_kmeans_parent")
DRIVERS = (("parent", ParentKMeans), ("new", NewKMeans), ("control", load_driver(sys.argv[1], "_kmeans_parent_again")))
OUT = sys.argv[3] if len(sys.argv) > 3 else os.devnull
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


def repeats(make_fit, warm, timed, metrics):
    """-> {driver: {metric: [median of `timed` fits] x 3 repeats}}, parent and new alternating"""
    res = {d: {m: [] for m in metrics} for d, _ in DRIVERS}
    for rep in range(3):
        for d, cls in DRIVERS:
            fit = make_fit(cls)
            for _ in range(warm):
                fit()
            vals = [fit() for _ in range(timed)]
            for i, m in enumerate(metrics):
                res[d][m].append(statistics.median(v[i] for v in vals))
    return res


def report(row, res, unit, scale):
    for m in next(iter(res.values())):
        p = [v * scale for v in res["parent"][m]]
        pm, spread = statistics.median(p), max(p) - min(p)
        for who in ("new", "control"):
            n = [v * scale for v in res[who][m]]
            nm = statistics.median(n)
            say("{:44s} {:22s} parent {} med {:.4f} | {:7s} {} med {:.4f} | bound {:.4f} {} -> {}".format(
                row, m + " [" + unit + "]", " ".join("%.4f" % v for v in p), pm, who, " ".join("%.4f" % v for v in n), nm, pm + spread, unit,
                "inside" if nm <= pm + spread else "OUTSIDE"))


def bench_shaped(pg, exchange):
    N, D, K, iters = 100000, 512, 500, 20
    rng = np.random.default_rng(1)
    X = rng.standard_normal((N, D)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    init = X[rng.choice(N, K, replace=False)].copy()
    Xd = torch.from_numpy(X).cuda()

    def make_fit(cls):
        km = cls(n_clusters=K, init=init, n_init=1, max_iter=iters, tol=0.0, fixed_iters=True, process_group=pg, exchange=exchange)

        def fit():
            torch.cuda.synchronize()
            t0 = time.time()
            km.fit(Xd)
            torch.cuda.synchronize()
            dt = time.time() - t0
            assert km.lloyd_iters_ == iters
            return km.lloyd_seconds_ / iters, dt
        return fit
    return repeats(make_fit, 4, 5, ("lloyd_seconds_/iters", "whole fit"))


def reference_call(N, D, K, warm, timed):
    rngc = np.random.default_rng(1)
    cent = rngc.standard_normal((K, D))
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    Xc = torch.from_numpy((cent[rngc.integers(0, K, N)] + 0.35 * rngc.standard_normal((N, D)) / np.sqrt(D)).astype(np.float32)).cuda()
    labels = {}

    def make_fit(cls):
        def fit():
            cluster_masks.KMeans = cls
            np.random.seed(1)
            torch.cuda.synchronize()
            t0 = time.time()
            with contextlib.redirect_stdout(io.StringIO()):
                lab = cluster_masks.fit_cluster(Xc, 'kmeans', k=K, l2normalize=True)
            torch.cuda.synchronize()
            dt = time.time() - t0
            labels[cls] = (lab, cluster_masks.fit_cluster.last_model.inertia_, cluster_masks.fit_cluster.last_model.n_iter_)
            return (dt,)
        return fit
    res = repeats(make_fit, warm, timed, ("fit_cluster wall",))
    a, b = labels[ParentKMeans], labels[NewKMeans]
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], "parent and new driver disagree"
    return res


def main():
    say("k-means driver: parent (%s) vs rewritten, alternating, 3 repeats each; per row the three per-repeat medians" % sys.argv[2])
    say("condition per row: median <= parent median + (parent slowest - parent fastest); control = a second copy of the parent")
    say("device: " + torch.cuda.get_device_name(0))
    report("bench-shaped 100kx512 K=500 20 it, no group", bench_shaped(None, None), "ms", 1e3)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29643", RANK="0", WORLD_SIZE="1")
    dist.init_process_group("nccl")
    torch.cuda.set_device(0)
    try:
        for ex in ("allreduce", "oneshot"):
            report("bench-shaped, one-rank group, " + ex, bench_shaped(dist.group.WORLD, ex), "ms", 1e3)
    finally:
        dist.destroy_process_group()
    report("fit_cluster(emb,'kmeans',500) 100kx512 n_init=10", reference_call(100000, 512, 500, 1, 3), "s", 1.0)
    report("fit_cluster small 10kx128 K=100 n_init=10", reference_call(10000, 128, 100, 4, 5), "ms", 1e3)
    say("done")


if __name__ == "__main__":
    main()

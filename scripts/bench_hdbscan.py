"""HDBSCAN (cosine) on the device: the whole fit, one Boruvka round's streamed pass, and the host share.

    python scripts/bench_hdbscan.py [--reps 3] [--warmup 1] [--out profiles/hdbscan.txt]
    python scripts/bench_hdbscan.py --sklearn [--out FILE]        # host only: sklearn's HDBSCAN(metric='cosine') at 5 000 and 20 000 rows

Rows: clustered unit rows (N / 50 blobs) plus 10 % uniform noise, at 20 000 x 128, 100 000 x 128 and 100 000 x 512;
HDBSCAN(min_cluster_size=5, min_samples=5).  One JSON line per size:
  wall_ms, wall_ms_min  median / minimum over --reps of the whole fit (rows already on the device; host clock around the call);
  host_tree_ms          the host part after the tree (single linkage, condensing, stability, selection, labels), from stats_;
  host_share            1 - (device ms of the core call and all rounds) / wall, from one more fit with SLIC_HDBSCAN_TIMING=1: the
                        union-find merges between the rounds, the copies and the tree part;
  rounds, ms_core, ms_rounds, ms_last_round, ms_last_pass   device events of that fit (the last round searches all rows, like the first);
  topk1_ms              the yardstick: cosine_topk(X, X, k=1) in the same run on the same rows, the same GEMM with a lighter epilogue
                        (device events, median of --reps), and pass_over_topk1 = ms_last_pass / topk1_ms.  Not a gate: the round's
                        epilogue adds two gathers, a max and a compare, so a ratio above about 1.5 points at the kernel.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def clustered_host(N, D, seed=0):
    rng = np.random.default_rng(seed)
    K = max(2, N // 50)
    cen = rng.standard_normal((K, D)).astype(np.float32)
    X = cen[rng.integers(0, K, N)] + np.float32(0.25 * (16.0 / D) ** 0.5) * rng.standard_normal((N, D)).astype(np.float32)
    nn = N // 10
    X[:nn] = rng.standard_normal((nn, D))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X[rng.permutation(N)]


def run_sklearn(out):
    from sklearn.cluster import HDBSCAN
    for N in (5000, 20000):
        X = clustered_host(N, 128, seed=N).astype(np.float64)
        t = time.perf_counter()
        m = HDBSCAN(min_cluster_size=5, min_samples=5, metric='cosine', copy=True).fit(X)
        row = dict(case="sklearn_host", N=N, D=128, wall_s=round(time.perf_counter() - t, 2), clusters=int(m.labels_.max()) + 1,
                   cpus=os.cpu_count())
        print(json.dumps(row), flush=True)
        if out:
            out.write(json.dumps(row) + "\n")


def run_case(N, D, reps, warmup, out):
    import torch
    from video_similarity_search_amd.clustering.hdbscan import HDBSCAN
    from video_similarity_search_amd.evaluate import cosine_topk
    X = torch.from_numpy(clustered_host(N, D, seed=N + D)).cuda()
    for _ in range(warmup):
        HDBSCAN(5, 5).fit(X)
    times, tree = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        m = HDBSCAN(5, 5).fit(X)
        times.append((time.perf_counter() - t) * 1e3)
        tree.append(m.stats_["seconds_host_tree"] * 1e3)
    os.environ["SLIC_HDBSCAN_TIMING"] = "1"
    try:
        torch.cuda.synchronize()
        t = time.perf_counter()
        mt = HDBSCAN(5, 5).fit(X)
        wall_t = (time.perf_counter() - t) * 1e3
    finally:
        os.environ.pop("SLIC_HDBSCAN_TIMING", None)
    assert np.array_equal(mt.labels_, m.labels_) and np.array_equal(mt.mst_weights_, m.mst_weights_)
    s = mt.stats_
    cosine_topk(X, X, k=1)
    tk = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        cosine_topk(X, X, k=1)
        b.record()
        torch.cuda.synchronize()
        tk.append(a.elapsed_time(b))
    topk1 = statistics.median(tk)
    row = dict(case="clustered", N=N, D=D, min_cluster_size=5, min_samples=5, wall_ms=round(statistics.median(times), 1),
               wall_ms_min=round(min(times), 1), host_tree_ms=round(statistics.median(tree), 1),
               host_share=round(1.0 - (s["ms_core"] + s["ms_rounds"]) / wall_t, 3), rounds=int(s["rounds"]),
               rows_searched=s["rows_searched"], ms_core=round(s["ms_core"], 2), ms_rounds=round(s["ms_rounds"], 2),
               ms_last_round=round(s["ms_last_round"], 2), ms_last_pass=round(s["ms_last_pass"], 2), topk1_ms=round(topk1, 2),
               pass_over_topk1=round(s["ms_last_pass"] / topk1, 2), clusters=int(m.n_clusters_), noise=int((m.labels_ < 0).sum()))
    print(json.dumps(row), flush=True)
    if out:
        out.write(json.dumps(row) + "\n")
        out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    if a.sklearn:
        run_sklearn(out)
        return
    import torch
    torch.cuda.set_device(0)
    for N, D in ((20000, 128), (100000, 128), (100000, 512)):
        run_case(N, D, a.reps, a.warmup, out)


if __name__ == "__main__":
    main()

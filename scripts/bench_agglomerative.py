"""Average-linkage agglomerative clustering (cosine, distance_threshold 0.24) on the device: wall time, rounds, query rows and the share of
the time spent inside slic_cosine_topk.

    python scripts/bench_agglomerative.py [--reps 3] [--warmup 1] [--out profiles/agglomerative.txt]

Cases: nested blobs (101 centres x 8 sub-centres) at 9 537 x 512 (the UCF101 split-1 train size) and at 100 000 x 512.  One JSON line
per case:
  wall_ms / wall_ms_min  median and minimum over --reps of the whole fit (rows already on the device; host clock around a call that ends in
                         the device-to-host copy of the labels);
  rounds, query_rows     what the fit reports; all_live_rows = the rows a search without the nearest-neighbour cache would have queried
                         (the sum of the live counts over the rounds);
  search_ms, search_share  device events around every slic_cosine_topk call (SLIC_AGGLO_TIMING=1), summed over one more fit, and that
                         sum over that fit's wall time;
  sklearn_s              at the first size, when sklearn can be imported: its AgglomerativeClustering on the same rows on the host, and
                         partitions asserted equal.  At 100 000 rows sklearn needs a 40 GB condensed float64 matrix: not run, no ratio.
A machine without a device fails here: nothing is measured on the CPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_similarity_search_amd.clustering.agglomerative import AgglomerativeClustering, HipAggloKernels  # noqa: E402

T = 0.24


def nested_blobs(N, D, seed, top=101, sub=8, subspread=0.4, spread=0.5):
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.randn(top, 1, D, device="cuda", generator=g) + subspread * torch.randn(top, sub, D, device="cuda", generator=g)
    c = c.reshape(-1, D)
    y = torch.randint(0, len(c), (N,), device="cuda", generator=g)
    return (c[y] + spread * torch.randn(N, D, device="cuda", generator=g)).contiguous()


def canonical(labels):
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv.reshape(-1)]


class _Counting(HipAggloKernels):
    """counts the live clusters at the start of every round"""

    def start(self, rows):
        self.all_live = 0
        return super().start(rows)

    def round(self, threshold):
        self.all_live += self.A
        return super().round(threshold)


def run_case(N, D, reps, warmup, with_sklearn):
    X = nested_blobs(N, D, seed=N)
    for _ in range(warmup):
        AgglomerativeClustering(distance_threshold=T).fit(X)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        m = AgglomerativeClustering(distance_threshold=T).fit(X)
        times.append((time.perf_counter() - t) * 1e3)
    os.environ["SLIC_AGGLO_TIMING"] = "1"
    try:
        k = _Counting()
        torch.cuda.synchronize()
        t = time.perf_counter()
        mt = AgglomerativeClustering(distance_threshold=T, kernels=k).fit(X)
        timed_ms = (time.perf_counter() - t) * 1e3
    finally:
        os.environ.pop("SLIC_AGGLO_TIMING", None)
    assert np.array_equal(mt.labels_, m.labels_)
    row = dict(N=N, D=D, threshold=T, wall_ms=round(statistics.median(times), 2), wall_ms_min=round(min(times), 2),
               clusters=int(m.n_clusters_), rounds=int(m.rounds_), query_rows=int(m.n_query_rows_), all_live_rows=int(k.all_live),
               fallback_merges=int(m.n_fallback_merges_), search_ms=round(k.search_ns / 1e6, 2), timed_fit_ms=round(timed_ms, 2),
               search_share=round(k.search_ns / 1e6 / timed_ms, 3))
    if with_sklearn:
        try:
            from sklearn.cluster import AgglomerativeClustering as SkAgglo
        except ImportError:
            row["sklearn_s"] = "sklearn not importable: not measured"
        else:
            Xh = X.cpu().numpy()
            t = time.perf_counter()
            ref = SkAgglo(n_clusters=None, linkage='average', distance_threshold=T, metric='cosine').fit(Xh)
            row["sklearn_s"] = round(time.perf_counter() - t, 2)
            row["sklearn_partition_equal"] = bool(np.array_equal(canonical(ref.labels_), m.labels_))      # asserted by main()
    else:
        row["sklearn_s"] = "not run: the condensed float64 matrix of {} rows is {:.0f} GB".format(N, N * (N - 1) / 2 * 8 / 1e9)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="9537,100000")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_agglomerative.py needs a gfx950 device: nothing is measured on the CPU")
    torch.cuda.set_device(0)
    sizes = [int(v) for v in a.sizes.split(",")]
    rows = [run_case(N, 512, a.reps, a.warmup, with_sklearn=(i == 0 and N <= 20000)) for i, N in enumerate(sizes)]
    if a.out:
        with open(a.out, "w") as f:
            f.write("# scripts/bench_agglomerative.py --reps {} --warmup {} on {}\n".format(a.reps, a.warmup, torch.cuda.get_device_name(0)))
            for r in rows:
                f.write(json.dumps(r) + "\n")
    assert all(r.get("sklearn_partition_equal", True) for r in rows), "partition differs from sklearn's"


if __name__ == "__main__":
    main()

"""OPTICS (cosine, cluster_method='dbscan') on the device: wall time, per-pass time, walk steps and launches, next to this library's
DBSCAN on the same rows and, where sklearn imports, sklearn.cluster.OPTICS on the host.

    python scripts/bench_optics.py [--reps 5] [--warmup 1] [--out FILE.txt] [--sklearn-rows 5000]

Cases (min_samples = 3, max_eps = 0.2, the reference's call):
  clustered   20 000 x 128 and 100 000 x 128 unit rows in clusters of tens to hundreds of rows + 10 % scattered rows
  medium      20 000 x 128 in clusters of 300 to 1000 rows: beyond the size up to which every cluster is walked by one workgroup
  one_big     20 000 x 128 with one cluster holding 90 % of the rows: the unfavourable case, the walk is ~N dependent steps
Per case one line each for
  optics          the whole fit (labels, core distances, walk); input on the device, results copied to the host
  optics_labels   the labels-only call (NULL walk outputs)
  dbscan          DBSCAN(eps = max_eps, min_samples) of this library
The three are timed alternately inside one loop (--reps rounds after --warmup), host clock around a call that ends synchronised;
median, min and max of the rounds are printed.  Pass times are device events from one more call with SLIC_OPTICS_TIMING=1.
`optics@lds_rows=R` repeats the full fit with SLIC_OPTICS_LDS_ROWS=R, alternating with the default in the same loop: R is the size of
the largest cluster up to which every cluster is walked by one workgroup (beyond it the clusters above min(R, 64) rows go through the
host loop; 0 = every cluster through the host loop, 1024 = one workgroup each whenever they fit).  What the rule in csrc/optics.hip
was picked from."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_similarity_search_amd.clustering.dbscan import DBSCAN  # noqa: E402
from video_similarity_search_amd.clustering.optics import OPTICS, HipOpticsKernels  # noqa: E402

EPS, MS = 0.2, 3
_out = []


def say(line):
    print(line, flush=True)
    _out.append(line)


def rows_in_clusters(N, D, sizes, seed, scattered=0.1):
    """unit rows: cluster i has sizes[i] rows at cosine distance ~0.1 from each other; the rest of the N rows are scattered"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    sizes = torch.as_tensor(sizes, device="cuda")
    y = torch.repeat_interleave(torch.arange(len(sizes), device="cuda"), sizes)
    cen = torch.randn(len(sizes), D, device="cuda", generator=g)
    X = cen[y] + 0.33 * torch.randn(len(y), D, device="cuda", generator=g)
    X = torch.cat([X, torch.randn(N - len(y), D, device="cuda", generator=g)])
    X = X[torch.randperm(N, device="cuda", generator=g)]
    return (X / X.norm(dim=1, keepdim=True)).contiguous()


def sizes_between(total, lo, hi, seed):
    rng = np.random.default_rng(seed)
    out = []
    while sum(out) + hi <= total:
        out.append(int(rng.integers(lo, hi + 1)))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def fmt(ts):
    return "median {:9.2f} ms  min {:9.2f}  max {:9.2f}  (n={})".format(statistics.median(ts), min(ts), max(ts), len(ts))


def with_env(key, val, fn):
    old = os.environ.get(key)
    os.environ[key] = str(val)
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = old


def run_case(name, X, reps, warmup, lds_rows=()):
    N, D = X.shape
    k = HipOpticsKernels()
    sides = {
        "optics": lambda: OPTICS(min_samples=MS, max_eps=EPS).fit(X),
        "optics_labels": lambda: k.optics(X, EPS, MS, walk=False),
        "dbscan": lambda: DBSCAN(eps=EPS, min_samples=MS).fit(X),
    }
    for r in lds_rows:
        sides["optics@lds_rows={}".format(r)] = (lambda r=r: with_env("SLIC_OPTICS_LDS_ROWS", r, sides["optics"]))
    times = {s: [] for s in sides}
    res = {}
    for it in range(warmup + reps):
        for s, fn in sides.items():
            ms, res[s] = timed(fn)
            if it >= warmup:
                times[s].append(ms)
    m = with_env("SLIC_OPTICS_TIMING", 1, sides["optics"])
    st = m.stats_
    assert np.array_equal(m.labels_, res["optics"].labels_) and np.array_equal(m.ordering_, res["optics"].ordering_)
    assert np.array_equal(res["optics_labels"][0], m.labels_)
    for r in lds_rows:
        o = res["optics@lds_rows={}".format(r)]
        assert np.array_equal(o.ordering_, m.ordering_) and np.array_equal(o.reachability_, m.reachability_)
    db = res["dbscan"].labels_
    sizes = np.bincount(m.labels_[m.labels_ >= 0]) if m.n_clusters_ else np.zeros(1, int)
    say("{} {} x {}: {} clusters (median {} rows, largest {}), {} noise, {} core; DBSCAN labels {} rows that OPTICS leaves noise".format(
        name, N, D, m.n_clusters_, int(np.median(sizes)), int(sizes.max()), int((m.labels_ < 0).sum()), int(st["core_rows"]),
        int(((db >= 0) & (m.labels_ < 0)).sum())))
    for s in sides:
        say("  {:24s} {}".format(s, fmt(times[s])))
    say("  passes (ms): " + "  ".join("{} {:.3f}".format(p[3:], st[p]) for p in st if p.startswith("ms_")))
    say("  walk: {} dependent steps, {} launches, {} clusters through the host loop; float64 rechecks {} (labels) + {} (walk)".format(
        int(st["walk_steps"]), int(st["walk_launches"]), int(st["host_loop_clusters"]), int(st["band_rechecks"]),
        int(st["walk_band_rechecks"])))
    walk_adds = statistics.median(times["optics"]) - statistics.median(times["optics_labels"])
    say("  the core distances and the walk add {:.2f} ms to the labels-only call ({:.2f} x DBSCAN)".format(
        walk_adds, statistics.median(times["optics"]) / statistics.median(times["dbscan"])))
    return m


def run_sklearn(X, m):
    try:
        from sklearn.cluster import OPTICS as SkOPTICS
    except ImportError:
        say("sklearn: not importable here, not measured")
        return
    Xh = X.cpu().numpy().astype(np.float64)
    t = time.perf_counter()
    sk = SkOPTICS(min_samples=MS, max_eps=EPS, metric='cosine', cluster_method='dbscan', n_jobs=-1).fit(Xh)
    dt = time.perf_counter() - t
    say("sklearn.cluster.OPTICS on the host, {} x {} (one run, n_jobs=-1): {:.1f} s; labels equal the device's: {}".format(
        X.shape[0], X.shape[1], dt, bool(np.array_equal(sk.labels_, m.labels_))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sklearn-rows", type=int, default=5000, help="0: skip sklearn (20 000 rows take it minutes)")
    ap.add_argument("--small", action="store_true", help="20 000-row cases only")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    say("device: {}".format(torch.cuda.get_device_name(0)))
    X = rows_in_clusters(20000, 128, sizes_between(18000, 20, 300, 1), seed=1)
    m = run_case("clustered", X, a.reps, a.warmup, lds_rows=(0, 64))
    if a.sklearn_rows:
        run_sklearn(X[:a.sklearn_rows], m if a.sklearn_rows >= len(X) else OPTICS(min_samples=MS, max_eps=EPS).fit(X[:a.sklearn_rows]))
    X = rows_in_clusters(20000, 128, sizes_between(18000, 300, 1000, 2), seed=2)
    run_case("medium", X, a.reps, a.warmup, lds_rows=(0, 1024))
    X = rows_in_clusters(20000, 128, [18000], seed=3)
    run_case("one_big", X, max(2, a.reps // 2), 1)
    if not a.small:
        X = rows_in_clusters(100000, 128, sizes_between(90000, 20, 300, 4), seed=4)
        run_case("clustered", X, a.reps, a.warmup)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(_out) + "\n")


if __name__ == "__main__":
    main()

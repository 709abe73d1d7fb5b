"""DBSCAN (cosine) on the device: wall time and per-pass time at the sizes the project benchmarks.

    python scripts/bench_dbscan.py [--reps 5] [--warmup 1] [--out FILE.json]

Cases: DBSCAN(0.14, 2) and DBSCAN(0.14, 5) on clustered synthetic rows (2000 blobs + 10 % uniform noise) at 100k x 128 and
100k x 512, and 100k x 128 identical rows (every pair a neighbour: the link pass's tile skip).  One JSON line per case:
  wall_ms            median over --reps of the whole fit (input already on the device; host clock around a synchronised call,
                     the three small device-to-host copies of the results included), and the minimum;
  ms_<pass>          device events between the passes, from one more call with SLIC_DBSCAN_TIMING=1;
  core / clusters / band_rechecks / skipped_tiles   what the call reported;
  count_roofline_ms  the count pass's matrix work, N^2 / 2 * Dp * 2 FLOP over the upper triangle of tiles (128-row tiles: the
                     diagonal ones in full), at 157.3 TFLOP/s (fp32 MFMA peak), and count_pct_of_peak = that over ms_count.
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
from video_similarity_search_amd.clustering.dbscan import DBSCAN  # noqa: E402

MFMA_PEAK = 157.3e12


def clustered(N, D, seed=0, K=2000, spread=0.25):
    g = torch.Generator(device="cuda").manual_seed(seed)
    cen = torch.randn(K, D, device="cuda", generator=g)
    y = torch.randint(0, K, (N,), device="cuda", generator=g)
    X = cen[y] + spread * (16.0 / D) ** 0.5 * torch.randn(N, D, device="cuda", generator=g)
    nn = N // 10
    X[:nn] = torch.randn(nn, D, device="cuda", generator=g)
    return X.contiguous()


def run_case(name, X, eps, ms, reps, warmup):
    N, D = X.shape
    for _ in range(warmup):
        DBSCAN(eps, ms).fit(X)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        m = DBSCAN(eps, ms).fit(X)
        times.append((time.perf_counter() - t) * 1e3)
    os.environ["SLIC_DBSCAN_TIMING"] = "1"
    try:
        mt = DBSCAN(eps, ms).fit(X)
    finally:
        os.environ.pop("SLIC_DBSCAN_TIMING", None)
    assert np.array_equal(mt.labels_, m.labels_)
    s = mt.stats_
    Dp = (D + 7) // 8 * 8
    T = (N + 127) // 128
    flop = T * (T + 1) / 2 * 128 * 128 * Dp * 2
    roof = flop / MFMA_PEAK * 1e3
    row = dict(case=name, N=N, D=D, eps=eps, min_samples=ms, wall_ms=round(statistics.median(times), 2),
               wall_ms_min=round(min(times), 2),
               **{k: round(v, 3) for k, v in s.items() if k.startswith("ms_")},
               core=int(s["core_rows"]), border_candidates=int(s["border_candidates"]), clusters=int(m.n_clusters_),
               noise=int((m.labels_ < 0).sum()), band_rechecks=int(s["band_rechecks"]), skipped_tiles=int(s["skipped_tiles"]),
               count_tflop=round(flop / 1e12, 3), count_roofline_ms=round(roof, 3),
               count_pct_of_peak=round(100 * roof / s["ms_count"], 1) if s["ms_count"] > 0 else None)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    for D in (128, 512):
        X = clustered(100000, D, seed=D)
        for ms in (2, 5):
            rows.append(run_case("clustered", X, 0.14, ms, a.reps, a.warmup))
        del X
    X = torch.randn(1, 128, device="cuda").expand(100000, 128).contiguous()
    rows.append(run_case("identical", X, 0.14, 2, a.reps, a.warmup))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

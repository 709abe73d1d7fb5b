"""micro-benchmark (GPU box): one k-means++ seeding at 100k x 512, K = 500, T = 8 through each entry point

    python scripts/bench_kpp.py [--reps 20] [--warmup 3]

Rows: kpp_run with the k-permuted copy (matrix pipe), kpp_run without it (kpp_dist_rows), kpp_run_batch with R = 10 (all ten
initialisations of n_init = 10 in lock-step; the time is per call, i.e. for the ten).  Every seeding is timed on the host clock
between device synchronises; the median over --reps is printed as one JSON line.  SLIC_LIB_PATH selects another build of the library."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_similarity_search_amd import _lib  # noqa: E402
from video_similarity_search_amd.clustering.kmeans_hip import HipKernels  # noqa: E402

N, D, K, T, R = 100000, 512, 500, 8, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kpp.py needs a gfx950 device: nothing is measured on the CPU")
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn(N, D, device="cuda", generator=g)
    X /= X.norm(dim=1, keepdim=True)
    k = HipKernels()
    Xp, xn = torch.empty_like(X), torch.empty(N, device="cuda")
    k.permute_k8(X, Xp)
    k.cnorm(X, xn)
    rng = np.random.default_rng(1)
    u = torch.from_numpy(rng.random((R, K - 1, T))).cuda()
    firsts = [int(f) for f in rng.integers(0, N, R)]
    idx = torch.empty(R, K, dtype=torch.int32, device="cuda")
    rows = {
        "kpp_run_mfma_ms": lambda: k.kpp_run(X, firsts[0], K, T, u[0], idx[0], Xp, xn),
        "kpp_run_valu_ms": lambda: k.kpp_run(X, firsts[0], K, T, u[0], idx[0]),
        "kpp_run_batch_r10_ms": lambda: k.kpp_run_batch(Xp, xn, firsts, K, T, u, idx),
    }
    out = {"lib": _lib.LIB_PATH, "reps": a.reps}
    for name, f in rows.items():
        for _ in range(a.warmup):
            f()
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t) * 1e3)
        out[name] = round(statistics.median(times), 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

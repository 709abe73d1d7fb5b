#!/usr/bin/env python
"""k-means Lloyd iteration: the fp32 E-step against the certified bf16 E-step (KMeans(precision=...)), same process, fits alternating.

Protocol of bench.py's kmeans_secondary: N x D rows, K clusters, init from data rows, tol = 0, 20 fixed iterations, warm-up fits first,
then KMeans.lloyd_seconds_ / iterations.  Per data set: ms per iteration of both precisions (median, and max - min of the fp32 side as
the spread to read a difference against), bf16_stats_ per E-step, and whether the two fits' labels are equal.

    python scripts/bench_kmeans_bf16.py [--out profiles/kmeans_bf16.txt]

* flat     : Gaussian unit rows (bench.py's data), D = 512 / 256 / 128
* clustered: 500 unit directions + 0.35 N(0, 1) / sqrt(D) (the generator of bench.py's reference-shaped clustering call), normalised
* tight    : the standalone E-step with K centres within 1e-3 of each other — every row overflows its slots and takes the exact chain
             over all K centroids (device events, median of 9)
* the kernels of an iteration: one child process under `rocprofv3 --kernel-trace --stats` runs fits of both precisions on the flat
  D = 512 data.
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OUT = []


def say(s):
    print(s, flush=True)
    OUT.append(s)


def make_data(kind, N, K, D, seed=1):
    rng = np.random.default_rng(seed)
    if kind == "flat":
        X = rng.standard_normal((N, D)).astype(np.float32)
    else:
        cent = rng.standard_normal((K, D))
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
        X = (cent[rng.integers(0, K, N)] + 0.35 * rng.standard_normal((N, D)) / np.sqrt(D)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    init = X[rng.choice(N, K, replace=False)].copy()
    return torch.from_numpy(X).cuda(), init


def fits(kind, N, K, D, iters, warm, reps):
    from video_similarity_search_amd.clustering import KMeans
    Xd, init = make_data(kind, N, K, D)
    km = {p: KMeans(n_clusters=K, init=init, n_init=1, max_iter=iters, tol=0.0, fixed_iters=True, precision=p) for p in ("fp32", "bf16")}
    ms = {p: [] for p in km}
    for i in range(warm + reps):
        for p in ("fp32", "bf16"):
            km[p].fit(Xd)
            if i >= warm:
                ms[p].append(km[p].lloyd_seconds_ / iters * 1e3)
    same = bool(np.array_equal(km["fp32"].labels_, km["bf16"].labels_)) and km["fp32"].inertia_ == km["bf16"].inertia_
    st = km["bf16"].bf16_stats_
    e = iters + 1                                                    # E-steps of a fit: the iterations and the final relabelling
    f, b = np.array(ms["fp32"]), np.array(ms["bf16"])
    say("%-9s %7d x %3d K=%d | fp32 %.3f ms/iter (spread %.3f) | bf16 %.3f ms/iter (spread %.3f) | bf16/fp32 %.2f | per E-step: rescored %.1f %% "
        "overflowed %.2f %% candidates/row %.2f | same result: %s"
        % (kind, N, D, K, np.median(f), f.max() - f.min(), np.median(b), b.max() - b.min(), np.median(b) / np.median(f),
           100.0 * st["rows_rescored"] / e / N, 100.0 * st["rows_overflowed"] / e / N, st["candidates"] / e / N, same))
    del Xd
    torch.cuda.empty_cache()


def tight(N, K, D, reps=9):
    from video_similarity_search_amd.clustering.kmeans_hip import HipKernels
    k = HipKernels()
    rng = np.random.default_rng(3)
    X = rng.standard_normal((N, D)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    u = rng.standard_normal(D)
    u /= np.linalg.norm(u)
    C = (u[None, :] + 1e-3 * rng.standard_normal((K, D)) / np.sqrt(D)).astype(np.float32)
    Xd, Cd = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
    Xp, Cp = torch.empty_like(Xd), torch.empty_like(Cd)
    k.permute_k8(Xd, Xp)
    k.permute_k8(Cd, Cp)
    cn = torch.empty(K, device="cuda")
    k.cnorm(Cd, cn)
    Xb, xn = k.bf16_image(Xd, want_norms=True)
    lf, lb = (torch.empty(N, dtype=torch.int32, device="cuda") for _ in range(2))
    stats = torch.zeros(3, dtype=torch.int32, device="cuda")

    def timed(fn):
        t = []
        for i in range(reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= 2:
                t.append(a.elapsed_time(b))
        return np.array(t)
    tf = timed(lambda: k.assign_perm(Xp, Cp, cn, lf, None, None))
    stats.zero_()
    tb = timed(lambda: k.assign_bf16(Xd, Xb, xn, Cd, k.bf16_image(Cd)[0], cn, lb, None, None, stats))
    st = stats.cpu().tolist()
    say("tight     %7d x %3d K=%d | E-step alone: fp32 %.3f ms (spread %.3f) | bf16 %.3f ms | bf16/fp32 %.2f | overflowed %.1f %% | same labels: %s"
        % (N, D, K, np.median(tf), tf.max() - tf.min(), np.median(tb), np.median(tb) / np.median(tf), 100.0 * st[1] / (reps + 2) / N,
           bool(torch.equal(lf, lb))))


def child(a):
    from video_similarity_search_amd.clustering import KMeans
    Xd, init = make_data("flat", a.n, a.k, 512)
    for p in ("fp32", "bf16"):
        km = KMeans(n_clusters=a.k, init=init, n_init=1, max_iter=a.iters, tol=0.0, fixed_iters=True, precision=p)
        for _ in range(4):
            km.fit(Xd)
    torch.cuda.synchronize()


def trace(a):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child",
               "--n", str(a.n), "--k", str(a.k), "--iters", str(a.iters)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        f = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
        if r.returncode != 0 or not f:
            say("# kernel split: rocprofv3 run failed (exit %d)\n%s" % (r.returncode, r.stderr[-800:]))
            return
        say("# kernels of 4 fp32 fits and 4 bf16 fits, flat rows, D = 512 (rocprofv3 --kernel-trace --stats): name, calls, average us, share of device time")
        for row in csv.DictReader(open(f[-1])):
            if float(row["Percentage"]) < 0.05:
                continue
            name = row["Name"]
            name = name if len(name) <= 70 else name[:67] + "..."
            say("%-70s %5s %10.1f %6.2f%%" % (name, row["Calls"], float(row["AverageNs"]) / 1e3, float(row["Percentage"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--k", type=int, default=500)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    say("# k-means Lloyd iteration, fp32 E-step vs certified bf16 E-step; %s" % torch.cuda.get_device_name(0))
    for D in (512, 256, 128):
        fits("flat", a.n, a.k, D, a.iters, a.warmup, a.reps)
    fits("clustered", a.n, a.k, 512, a.iters, a.warmup, a.reps)
    tight(a.n, a.k, 512)
    if not a.no_trace:
        trace(a)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()

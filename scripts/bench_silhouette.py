#!/usr/bin/env python
"""Silhouette from cluster sums (slic_silhouette) at the cluster step's sizes, next to the k-means E-step at the same N, K, D — the same
N x K x D contraction on the same ring, with (min, argmin) in place of (own, min over the others, argmin).

    python scripts/bench_silhouette.py [--out profiles/silhouette.txt]

Method of scripts/bench_kmeans_bf16.py: device events around the call, warm-up first, median of 100 (max - min as the spread).
* the whole call: slic_silhouette with the workspace sized for Kmax = N - 1 (the Python default: the count of clusters is not known
  before the call) and for Kmax = K;
* the E-step: slic_kmeans_assign_perm on the permuted rows against K permuted centres;
* the kernels of the call: one child process under `rocprofv3 --kernel-trace --stats`.
Rows: K unit directions + 0.35 N(0, 1) / sqrt(D), normalised; labels = the direction a row was drawn around.
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
SHAPES = ((100000, 128, 1000), (100000, 128, 25000), (240000, 128, 1000))


def say(s):
    print(s, flush=True)
    OUT.append(s)


def make_data(N, D, K, seed=1):
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((K, D))
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    z = np.concatenate([np.arange(K), rng.integers(0, K, N - K)])
    rng.shuffle(z)
    X = (cent[z] + 0.35 * rng.standard_normal((N, D)) / np.sqrt(D)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return torch.from_numpy(X).cuda(), torch.from_numpy(z.astype(np.int32)).cuda(), torch.from_numpy(cent.astype(np.float32)).cuda()


def timed(fn, reps, warm=5):
    t = []
    for i in range(reps + warm):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warm:
            t.append(a.elapsed_time(b))
    return np.array(t)


def silhouette_call(Xd, ld, metric, kmax):
    """-> (a closure that makes the library call, the record tensor)"""
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd._lib import call, ptr, stream
    N, D = Xd.shape
    nbytes = _lib.load().slic_silhouette_workspace_bytes(N, D, kmax)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    f = torch.empty((3, N), dtype=torch.float32, device="cuda")
    near = torch.empty(N, dtype=torch.int32, device="cuda")
    rec = torch.empty(4, dtype=torch.float64, device="cuda")
    cm, cl = torch.empty(kmax, dtype=torch.float64, device="cuda"), torch.empty(kmax, dtype=torch.int32, device="cuda")

    def fn():
        call("slic_silhouette", ptr(Xd), N, D, Xd.stride(0), ptr(ld), metric, 0, 0, kmax, ptr(f[0]), ptr(f[1]), ptr(f[2]), ptr(near), ptr(rec),
             ptr(cm), ptr(cl), ptr(ws), stream())
    return fn, rec, nbytes


def estep_call(Xd, Cd):
    from video_similarity_search_amd.clustering.kmeans_hip import HipKernels
    k = HipKernels()
    Xp, Cp = torch.empty_like(Xd), torch.empty_like(Cd)
    k.permute_k8(Xd, Xp)
    k.permute_k8(Cd, Cp)
    cn = torch.empty(Cd.shape[0], device="cuda")
    k.cnorm(Cd, cn)
    lab = torch.empty(Xd.shape[0], dtype=torch.int32, device="cuda")
    return lambda: k.assign_perm(Xp, Cp, cn, lab, None, None)


def shape(N, D, K, reps):
    Xd, ld, Cd = make_data(N, D, K)
    te = timed(estep_call(Xd, Cd), reps)
    for metric, name in ((0, "cosine"), (1, "sqeuclidean")):
        for kmax in (N - 1, K):
            fn, rec, nbytes = silhouette_call(Xd, ld, metric, kmax)
            t = timed(fn, reps)
            r = rec.cpu().numpy()
            say("%7d x %3d K=%5d %-11s Kmax=%6d | call %.3f ms (spread %.3f) | E-step %.3f ms (spread %.3f) | call / E-step %.2f | "
                "score %.4f clusters %d status %d | workspace %.1f MB"
                % (N, D, K, name, kmax, np.median(t), t.max() - t.min(), np.median(te), te.max() - te.min(), np.median(t) / np.median(te),
                   r[0], int(r[1]), int(r[3]), nbytes / 1e6))
    del Xd, ld, Cd
    torch.cuda.empty_cache()


def child(a):
    Xd, ld, Cd = make_data(a.n, a.d, a.k)
    fn, _, _ = silhouette_call(Xd, ld, 0, a.n - 1)
    est = estep_call(Xd, Cd)
    for _ in range(10):
        fn()
        est()
    torch.cuda.synchronize()


def trace(N, D, K):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child",
               "--n", str(N), "--d", str(D), "--k", str(K)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        f = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
        if r.returncode != 0 or not f:
            say("# kernel split: rocprofv3 run failed (exit %d)\n%s" % (r.returncode, r.stderr[-800:]))
            return
        say("# kernels of 10 cosine calls (Kmax = N - 1) and 10 E-steps, %d x %d K=%d (rocprofv3 --kernel-trace --stats): name, calls, "
            "average us, share of device time" % (N, D, K))
        for row in csv.DictReader(open(f[-1])):
            if float(row["Percentage"]) < 0.05:
                continue
            name = row["Name"]
            name = name if len(name) <= 70 else name[:67] + "..."
            say("%-70s %5s %10.1f %6.2f%%" % (name, row["Calls"], float(row["AverageNs"]) / 1e3, float(row["Percentage"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    say("# silhouette from cluster sums vs the k-means E-step at the same N, K, D; %s; median of %d" % (torch.cuda.get_device_name(0), a.reps))
    for N, D, K in SHAPES:
        shape(N, D, K, a.reps)
    if not a.no_trace:
        for N, D, K in SHAPES[:2]:
            trace(N, D, K)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()

"""NMI / AMI of the cluster step: the device call against the two scikit-learn calls it replaces, at the two working sizes.

    python scripts/bench_cluster_metrics.py [--reps 5] [--warmup 2] [--host-reps 1] [--out FILE.json]

Cases: 240 000 labels, 400 classes against 1000 clusters; 100 000 labels, 101 classes against a FINCH-like first partition of
about N / 4 clusters.  One JSON line per case:
  device_ms          median over --reps of cluster_scores (labels already on the device; host clock around a call that ends in the
                     read-back of the record, which synchronises), and the minimum;
  device_ms_host_in  the same with the labels as host lists, as iterative_cluster_step passes them (conversion + upload included);
  sklearn_ms         on the same host: normalized_mutual_info_score + adjusted_mutual_info_score on the same labels (the parent
                     route; median of --host-reps), and its two parts;
  ratio              sklearn_ms / device_ms_host_in — like for like: both start from host labels and end with two Python floats;
  emi_terms          sum_ij (min(a_i, b_j) - max(1, a_i + b_j - N) + 1): the terms of the expected-mutual-information sum;
  d_nmi, d_ami       |device - sklearn|.
Without scikit-learn the sklearn_* fields and the ratio are null and the device is still timed.
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
from video_similarity_search_amd.clustering import cluster_scores  # noqa: E402


def working_size(which):
    rng = np.random.default_rng(77 + which)
    if which == 0:
        N = 240000
        lt = rng.integers(0, 400, N)
        lp = np.where(rng.random(N) < 0.4, lt * 2 + rng.integers(0, 2, N), rng.integers(0, 1000, N))
    else:
        N = 100000
        lt = rng.integers(0, 101, N)
        lp = lt * 250 + rng.integers(0, 248, N)
    return lt.astype(np.int32), lp.astype(np.int32)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return r, ts


def emi_terms(lt, lp):
    a = np.unique(lt, return_counts=True)[1].astype(np.int64)
    b = np.unique(lp, return_counts=True)[1].astype(np.int64)
    N = len(lt)
    total = 0
    for x in a:
        total += int((np.minimum(x, b) - np.maximum(1, x + b - N) + 1).clip(0).sum())
    return total


def run_case(name, lt, lp, reps, warmup, host_reps):
    dt, dp = torch.from_numpy(lt).cuda(), torch.from_numpy(lp).cuda()
    s, t_dev = timed(lambda: cluster_scores(dt, dp), reps, warmup)
    llt, llp = lt.tolist(), lp.tolist()
    s2, t_host_in = timed(lambda: cluster_scores(llt, llp), reps, 1)
    assert s2 == s
    row = dict(case=name, N=len(lt), n_classes=s["n_classes"], n_clusters=s["n_clusters"], emi_terms=emi_terms(lt, lp),
               device_ms=round(statistics.median(t_dev), 3), device_ms_min=round(min(t_dev), 3),
               device_ms_host_in=round(statistics.median(t_host_in), 3), NMI=s["NMI"], AMI=s["AMI"],
               sklearn_ms=None, sklearn_nmi_ms=None, sklearn_ami_ms=None, ratio=None, d_nmi=None, d_ami=None)
    try:
        from sklearn.metrics import adjusted_mutual_info_score, normalized_mutual_info_score
    except ImportError:
        adjusted_mutual_info_score = None
    if adjusted_mutual_info_score is not None:
        tn, ta = [], []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            nmi = normalized_mutual_info_score(llt, llp)
            t1 = time.perf_counter()
            ami = adjusted_mutual_info_score(llt, llp)
            t2 = time.perf_counter()
            tn.append((t1 - t0) * 1e3)
            ta.append((t2 - t1) * 1e3)
        both = statistics.median([x + y for x, y in zip(tn, ta)])
        row.update(sklearn_ms=round(both, 1), sklearn_nmi_ms=round(statistics.median(tn), 1), sklearn_ami_ms=round(statistics.median(ta), 1),
                   ratio=round(both / statistics.median(t_host_in), 1), d_nmi=abs(nmi - s["NMI"]), d_ami=abs(ami - s["AMI"]))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = [run_case(n, *working_size(i), a.reps, a.warmup, a.host_reps) for i, n in enumerate(("240k_400x1000", "100k_101x25k"))]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

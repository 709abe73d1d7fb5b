"""Top-k retrieval by metric: cosine_topk against euclidean_topk on the same data, and the old euclidean route.

    python scripts/bench_topk_metric.py [--reps 7] [--warmup 2] [--out FILE.json]

* 10k queries x 100k gallery rows at D = 128 and 512, k in {1, 20, 50, 88}: device-event time per call (the wrappers' whole work:
  normalisation for cosine, the centring pre-pass and the refine for euclidean), the two metrics interleaved call by call after a
  warm-up of each, median and minimum over --reps;
* the share of the fp32 matrix pipe's roofline (2 Nq Ng D FLOP at 157.3 TFLOP/s) each call reaches, and for euclidean the refine's
  own traffic (Nq * min(k + 8, 88) * D floats read at 6.3 TB/s) beside it;
* the margin's price: euclidean at k = 50 with its default list (k + 8 ranked by score, refined) against SLIC_TOPK_EU_MARGIN=0;
* the route euclidean evaluation took before: get_distance_matrix(.., 'euclidean') + get_topk_acc (dense matrix, host copy,
  argpartition) at a size the host holds, against get_topk_acc_from_embeddings(.., dist_metric='euclidean') at that size (wall time).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_similarity_search_amd.evaluate import (cosine_topk, euclidean_topk, get_distance_matrix, get_topk_acc,  # noqa: E402
                                                  get_topk_acc_from_embeddings)

MFMA_PEAK = 157.3e12      # fp32 v_mfma_f32_32x32x2_f32, FLOP/s
HBM = 6.3e12              # measured, bytes/s


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def bench_metrics(reps, warmup, out):
    Nq, Ng = 10000, 100000
    gen = torch.Generator(device="cuda").manual_seed(5)
    for D in (128, 512):
        Q = torch.randn(Nq, D, device="cuda", generator=gen)
        G = torch.randn(Ng, D, device="cuda", generator=gen)
        for k in (1, 20, 50, 88):
            fns = {"cosine": lambda: cosine_topk(Q, G, k=k), "euclidean": lambda: euclidean_topk(Q, G, k=k)}
            for _ in range(warmup):
                for f in fns.values():
                    f()
            torch.cuda.synchronize()
            ts = {m: [] for m in fns}
            for _ in range(reps):
                for m, f in fns.items():                        # interleaved: drift hits both metrics alike
                    ts[m].append(_timed(f))
            mfma_ms = 2.0 * Nq * Ng * D / MFMA_PEAK * 1e3
            refine_ms = Nq * min(k + 8, 88) * D * 4 / HBM * 1e3
            for m in fns:
                med, mn = float(np.median(ts[m])), float(np.min(ts[m]))
                rec = dict(metric=m, Nq=Nq, Ng=Ng, D=D, k=k, ms_median=round(med, 3), ms_min=round(mn, 3),
                           mfma_roofline_ms=round(mfma_ms, 3), roofline_share=round(mfma_ms / med, 3))
                if m == "euclidean":
                    rec["refine_roofline_ms"] = round(refine_ms, 3)
                    rec["vs_cosine"] = round(med / float(np.median(ts["cosine"])), 3)
                print(json.dumps(rec), flush=True)
                out.append(rec)
        del Q, G
        torch.cuda.empty_cache()


def bench_margin(reps, warmup, out):
    """the refine's margin: euclidean at k = 50 with the default list of k + 8 against SLIC_TOPK_EU_MARGIN=0 (list of k), interleaved"""
    Nq, Ng, k = 10000, 100000, 50
    gen = torch.Generator(device="cuda").manual_seed(6)
    for D in (128, 512):
        Q = torch.randn(Nq, D, device="cuda", generator=gen)
        G = torch.randn(Ng, D, device="cuda", generator=gen)
        ts = {"8": [], "0": []}

        def run(m):
            os.environ["SLIC_TOPK_EU_MARGIN"] = m
            try:
                return _timed(lambda: euclidean_topk(Q, G, k=k))
            finally:
                del os.environ["SLIC_TOPK_EU_MARGIN"]
        for _ in range(warmup):
            for m in ts:
                run(m)
        for _ in range(reps):
            for m in ts:
                ts[m].append(run(m))
        rec = dict(margin_bench="euclidean, k = 50", Nq=Nq, Ng=Ng, D=D, ms_margin8=round(float(np.median(ts["8"])), 3),
                   ms_margin0=round(float(np.median(ts["0"])), 3))
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del Q, G
        torch.cuda.empty_cache()


def bench_old_route(out):
    """dense euclidean matrix + host top-k (what evaluate.py:130 / validation.py did) against the device top-k, same data"""
    Nq, Ng, D, top_ks = 1000, 100000, 512, [1, 5, 10, 20]
    rng = np.random.default_rng(7)
    X = torch.from_numpy(rng.standard_normal((Nq, D)).astype(np.float32)).cuda()
    Y = torch.from_numpy(rng.standard_normal((Ng, D)).astype(np.float32)).cuda()
    xl, yl = rng.integers(0, 100, Nq), rng.integers(0, 100, Ng)
    get_topk_acc_from_embeddings(X, xl, Y, yl, top_ks=top_ks, dist_metric='euclidean')     # warm-up (workspace, attributes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a = get_topk_acc_from_embeddings(X, xl, Y, yl, top_ks=top_ks, dist_metric='euclidean')
    t1 = time.perf_counter()
    dm = get_distance_matrix(X, Y, 'euclidean')
    t2 = time.perf_counter()
    b = get_topk_acc(dm, xl, yl, top_ks=top_ks)
    t3 = time.perf_counter()
    rec = dict(route="old euclidean: get_distance_matrix + get_topk_acc", Nq=Nq, Ng=Ng, D=D, k=top_ks[-1],
               matrix_and_copy_ms=round((t2 - t1) * 1e3, 1), host_topk_ms=round((t3 - t2) * 1e3, 1),
               total_ms=round((t3 - t1) * 1e3, 1), device_topk_ms=round((t1 - t0) * 1e3, 2),
               speedup=round((t3 - t1) / (t1 - t0), 1), same_accuracies=bool(np.array_equal(a, b)))
    print(json.dumps(rec), flush=True)
    out.append(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    bench_metrics(a.reps, a.warmup, out)
    bench_margin(a.reps, a.warmup, out)
    bench_old_route(out)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

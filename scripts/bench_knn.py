"""k-NN classification and ranked retrieval metrics on the top-k lists: the two kernels of csrc/knn.hip against plain torch ops on the
same index table and against the host NumPy path (index table copied to the host, y_train[idx] in NumPy), and the whole calls.

    python scripts/bench_knn.py [--iters 100] [--reps 5] [--out FILE.txt]

Shapes: 10 000 queries x 100 000 gallery rows x 128 dimensions (unit-normal rows around class centres); k = 20 and 88 at C = 101 classes,
k = 20 at C = 700.  Per shape ONE search leaves idx / dist [Nq, k] on the device; the rows below all read that table.
  vote/...      slic_knn_vote (softmax weights, T = 0.07, the 5 best classes) | torch: labels[idx], exp, one-hot scatter_add_ into
                [Nq, C], topk(5) | host: idx and dist copied to the host, the same in NumPy (bincount over q * C + label, argpartition)
  ranked/...    slic_retrieval_ranked (cut-offs 1, 5, 10, 20 and k when it is larger; both launches) | torch: labels[idx] == q, cumsum,
                the three ratios and their means | host: idx copied to the host, the same in NumPy
  device rows:  HIP events around one call, the sides ALTERNATING call by call, median of --iters after 10 warm calls of each
  host rows:    host clock around the copy and the NumPy work (that IS the path's cost), median of --reps
  call/...      knn_classify and retrieval_metrics as a user calls them (search + kernel + read-back; host clock, synchronised, median
                of --reps) beside the search alone: the search dominates, so no ratio of the whole is claimed
Needs the GPU: without one the script fails.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_similarity_search_amd.evaluate import cosine_topk, knn_classify, retrieval_metrics, _n_relevant  # noqa: E402
from video_similarity_search_amd.neighbors import HipKnnKernels  # noqa: E402

T = 0.07
SOFTMAX = 2


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3          # us


def alternate(fa, fb, iters):
    for _ in range(10):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(iters):
        ta.append(event_time(fa))
        tb.append(event_time(fb))
    return (statistics.median(ta), max(ta) - min(ta)), (statistics.median(tb), max(tb) - min(tb))


def host_time(fn, reps):
    out = []
    for rep in range(reps + 1):             # repetition 0 warms up
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep:
            out.append((time.perf_counter() - t) * 1e6)
    return statistics.median(out), max(out) - min(out)


def torch_vote(idx, dist, g_labels, C):
    lab = g_labels[idx.long()]
    w = torch.exp((dist[:, :1] - dist) * (1.0 / T))
    scores = torch.zeros(idx.shape[0], C, dtype=torch.float32, device=idx.device).scatter_add_(1, lab, w)
    return scores.topk(5, dim=1)


def numpy_vote(idx, dist, g_labels_host, C):
    i, d = idx.cpu().numpy(), dist.cpu().numpy()
    lab = g_labels_host[i]
    w = np.exp((d[:, :1] - d) * np.float32(1.0 / T))
    flat = (np.arange(i.shape[0])[:, None] * C + lab).ravel()
    scores = np.bincount(flat, weights=w.ravel(), minlength=i.shape[0] * C).reshape(i.shape[0], C)
    return np.argpartition(-scores, 5, axis=1)[:, :5]


def torch_ranked(idx, q_labels, g_labels, n_rel, ks):
    h = g_labels[idx.long()] == q_labels[:, None]
    c = h.cumsum(1).to(torch.float64)
    terms = torch.where(h, c / torch.arange(1, idx.shape[1] + 1, device=idx.device, dtype=torch.float64), torch.zeros((), dtype=torch.float64, device=idx.device))
    ap = terms.cumsum(1)
    nr = n_rel.to(torch.float64)
    rel = nr > 0
    out = []
    for K in ks:
        out.append((c[:, K - 1] / K).mean())
        out.append((c[:, K - 1] / nr)[rel].mean())
        out.append((ap[:, K - 1] / nr.clamp(max=K))[rel].mean())
    first = torch.where(h.any(1), h.to(torch.int8).argmax(1), torch.full_like(n_rel, -1).long())
    out.append(torch.where(first >= 0, 1.0 / (first + 1).to(torch.float64), torch.zeros((), dtype=torch.float64, device=idx.device)).mean())
    return torch.stack(out)


def numpy_ranked(idx, q_host, g_host, n_rel_host, ks):
    i = idx.cpu().numpy()
    h = g_host[i] == q_host[:, None]
    c = np.cumsum(h, axis=1).astype(np.float64)
    ap = np.cumsum(np.where(h, c / np.arange(1, i.shape[1] + 1), 0.0), axis=1)
    nr = n_rel_host.astype(np.float64)
    rel = nr > 0
    out = []
    for K in ks:
        out += [(c[:, K - 1] / K).mean(), (c[rel, K - 1] / nr[rel]).mean(), (ap[rel, K - 1] / np.minimum(nr[rel], K)).mean()]
    out.append(np.where(h.any(1), 1.0 / (h.argmax(1) + 1), 0.0).mean())
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--ng", type=int, default=100000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn.py measures on the GPU; none found")
    Nq, Ng, D = args.nq, args.ng, 128
    K = HipKnnKernels()
    lines = ["k-NN vote and ranked retrieval metrics on the top-k lists: %d queries x %d gallery rows x %d (scripts/bench_knn.py)" % (Nq, Ng, D),
             "device rows: HIP events, sides alternating, median of %d (spread = max - min); host rows: host clock, median of %d" % (
                 args.iters, args.reps),
             "%-28s %12s %10s %12s %10s %9s" % ("row", "kernel us", "spread", "other us", "spread", "other/krn")]

    def report(name, new, other):
        verdict = "" if new[0] <= other[0] else "   THE OTHER PATH WINS"
        lines.append("%-28s %12.1f %10.1f %12.1f %10.1f %9.2f%s" % (name, new[0], new[1], other[0], other[1], other[0] / new[0], verdict))
        print(lines[-1], flush=True)

    def note(text):
        lines.append(text)
        print(text, flush=True)

    print("\n".join(lines), flush=True)
    for (k, C) in ((20, 101), (88, 101), (20, 700)):
        gen = torch.Generator(device="cuda").manual_seed(k + C)
        cen = torch.randn(C, D, device="cuda", generator=gen)
        g_labels = torch.randint(0, C, (Ng,), device="cuda", generator=gen)
        q_labels = torch.randint(0, C, (Nq,), device="cuda", generator=gen)
        gal = cen[g_labels] + 1.5 * torch.randn(Ng, D, device="cuda", generator=gen)
        qry = cen[q_labels] + 1.5 * torch.randn(Nq, D, device="cuda", generator=gen)
        idx, dist = cosine_topk(qry, gal, k=k)
        n_rel = _n_relevant(q_labels, g_labels, False)
        g_host, q_host, n_rel_host = g_labels.cpu().numpy(), q_labels.cpu().numpy(), n_rel.cpu().numpy()
        ks = [v for v in (1, 5, 10, 20) if v <= k] + ([k] if k > 20 else [])
        tag = "k%d/C%d" % (k, C)

        # the sides agree before they are timed
        _, pred, _ = K.vote(idx, dist, g_labels, C, SOFTMAX, T, 5, False)
        agree = (pred[:, 0].long() == torch_vote(idx, dist, g_labels, C)[1][:, 0]).float().mean().item()
        rec = K.ranked(idx, q_labels, g_labels, n_rel, ks)[2]
        diff = (rec[:-1] - torch_ranked(idx, q_labels, g_labels, n_rel, ks)).abs().max().item()
        note("%-28s top-1 class equal to the torch monitor's on %.4f of the queries; ranked means differ by at most %.3g" % (
            "check/" + tag, agree, diff))

        new, other = alternate(lambda: K.vote(idx, dist, g_labels, C, SOFTMAX, T, 5, False), lambda: torch_vote(idx, dist, g_labels, C),
                               args.iters)
        report("vote/%s/torch" % tag, new, other)
        report("vote/%s/host-numpy" % tag, new, host_time(lambda: numpy_vote(idx, dist, g_host, C), args.reps))
        new, other = alternate(lambda: K.ranked(idx, q_labels, g_labels, n_rel, ks),
                               lambda: torch_ranked(idx, q_labels, g_labels, n_rel, ks), args.iters)
        report("ranked/%s/torch" % tag, new, other)
        report("ranked/%s/host-numpy" % tag, new, host_time(lambda: numpy_ranked(idx, q_host, g_host, n_rel_host, ks), args.reps))

        search = host_time(lambda: cosine_topk(qry, gal, k=k), args.reps)
        whole_c = host_time(lambda: knn_classify(qry, q_labels, gal, g_labels, k=k, num_classes=C), args.reps)
        whole_r = host_time(lambda: retrieval_metrics(qry, q_labels, gal, g_labels, ks=ks), args.reps)
        note("%-28s search alone %.0f us (spread %.0f) | knn_classify %.0f us (spread %.0f) | retrieval_metrics %.0f us (spread %.0f)" % (
            "call/" + tag, search[0], search[1], whole_c[0], whole_c[1], whole_r[0], whole_r[1]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""The validation pass after the encoder: the per-batch work and the 'global' finish, old pieces against the fused path.

    python scripts/bench_validate.py [--reps 5] [--iters 20] [--out FILE.txt]

Rows (B = 80 triplets = VAL.BATCH_SIZE's default, D = 128, both metrics; embeddings already on the device):
  batch/<metric>/triplet       what every batch costs under VAL.METRIC 'global': distances, margin loss, accuracy
  batch/<metric>/local_batch   the same plus the batch's own top-1 / top-5 (VAL.METRIC 'local_batch')
  finish/<metric>/N            the 'global' finish over N anchors: top-1 / top-5 of every anchor among the others
(a) old = the reference's loop body over the package's older public pieces: Tripletnet's two pair_distance calls,
    torch.nn.MarginRankingLoss, the accuracy formula, two .item() reads per batch; get_distance_matrix + get_topk_acc on the host.
(b) new = slic_triplet_val_batch into a row of the device record, cosine_topk / euclidean_topk + slic_topk_label_hits; the record is
    read once per --iters batches (a log interval).
Time: host clock around --iters synchronised iterations after --iters warm ones (the old path's cost IS host work and round trips, so
device events alone would miss it), per iteration; median over --reps repetitions and their spread (max - min).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_similarity_search_amd.evaluate import get_distance_matrix, get_topk_acc, topk_acc_device  # noqa: E402
from video_similarity_search_amd.models.triplet_net import pair_distance  # noqa: E402
from video_similarity_search_amd.validation import HipValidationKernels, TOP_KS  # noqa: E402


def timed(fn, iters, reps, finish=None):
    out = []
    for rep in range(reps + 1):                      # repetition 0 warms up
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(iters):
            fn(i)
        if finish is not None:
            finish()
        torch.cuda.synchronize()
        if rep:
            out.append((time.perf_counter() - t) * 1e6 / iters)
    return statistics.median(out), max(out) - min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, D = 80, 128
    g = torch.Generator(device="cuda").manual_seed(0)
    ex, ey, ez = (torch.randn(B, D, device="cuda", generator=g) for _ in range(3))
    ta = torch.randint(0, 50, (B,), generator=torch.Generator().manual_seed(1))
    lab_host = torch.cat((ta, ta))
    lab_dev = lab_host.cuda()
    crit = torch.nn.MarginRankingLoss(margin=0.2)
    K = HipValidationKernels()
    rec = torch.zeros(args.iters, 5, device="cuda")
    lines = ["%-34s %12s %10s %12s %10s %8s" % ("row", "old us", "spread", "new us", "spread", "old/new")]

    def report(name, old, new):
        verdict = "" if new[0] <= old[0] + max(old[1], new[1]) else "   SLOWER than the old path beyond the spread"
        lines.append("%-34s %12.1f %10.1f %12.1f %10.1f %8.2f%s" % (name, old[0], old[1], new[0], new[1], old[0] / new[0], verdict))
        print(lines[-1], flush=True)

    for metric in ("cosine", "euclidean"):
        euclid = metric == "euclidean"

        def old_triplet(i):
            dista, distb = pair_distance(ex, ey, metric), pair_distance(ex, ez, metric)
            loss = crit(dista, distb, torch.full_like(dista, -1))
            acc = ((distb - dista) > 0).sum() * 1.0 / dista.size()[0]
            return acc.item(), loss.item()

        def old_local(i):
            old_triplet(i)
            e = torch.cat((ex.cpu(), ey.cpu()), dim=0)
            t = get_topk_acc(get_distance_matrix(e, dist_metric=metric), lab_host.tolist())
            return torch.tensor(t[0]).cuda(), torch.tensor(t[1]).cuda()

        def new_triplet(i):
            K.val_batch(ex, ey, ez, euclid, 0.2, rec[i])

        def new_local(i):
            K.val_batch(ex, ey, ez, euclid, 0.2, rec[i])
            e = torch.cat((ex, ey), dim=0)
            hits = K.label_hits(K.topk(e, None, TOP_KS[-1], metric), lab_dev, lab_dev, TOP_KS)
            rec[i, 3:5] = hits[:2].to(torch.float32) / e.shape[0]

        read = lambda: K.read_record(rec)       # noqa: E731
        with torch.no_grad():
            report("batch/%s/triplet" % metric, timed(old_triplet, args.iters, args.reps), timed(new_triplet, args.iters, args.reps, read))
            report("batch/%s/local_batch" % metric, timed(old_local, args.iters, args.reps), timed(new_local, args.iters, args.reps, read))
            for N in (3783, 10000):
                emb = torch.randn(N, D, device="cuda", generator=g)
                labels = torch.randint(0, 400, (N,), generator=torch.Generator().manual_seed(2))
                ldev = labels.cuda()
                llist = labels.tolist()
                old = timed(lambda i: get_topk_acc(get_distance_matrix(emb.cpu(), dist_metric=metric), llist), 2, args.reps)
                new = timed(lambda i: topk_acc_device(emb, ldev, dist_metric=metric), args.iters, args.reps)
                report("finish/%s/%d" % (metric, N), old, new)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

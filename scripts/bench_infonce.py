"""Times the MoCo training step of models/infoNCE.py and its accuracy kernel on one device, in one run, and writes a table:
    python scripts/bench_infonce.py --out profiles/infonce.txt
B in {32, 128}, D = 128, K in {2048, 16384}, for InfoNCE (one positive) and UberNCE (labels: about K / 64 positives a row).
  kernels: slic_moco_topk_hits alone against slic_moco_ce_fwd alone, same inputs (top_ks (1, 5)).
  step:    (a) model.contrast: fused loss + fused accuracies, forward + backward;
           (b) model.forward + torch cross-entropy (the mask loss for UberNCE) + the accuracy computed the way the reference shapes it
               (top-k indices, one-hot scatter per k, product with the mask), forward + backward, same device.
The trunk is a pooling stub (the step's own cost is the head, the contrast and the accuracy; a 3D ResNet in front would hide them),
so the step times compare the two paths and are not the time of a training step.  The two sides of every comparison alternate call
by call in one loop (both on the same model and queue); HIP events around every call, --warmup calls discarded, median of --runs
[min, p90], microseconds."""
import argparse
import contextlib
import io
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, T, FEAT = 128, 0.07, 512
SHAPES = [(B, K) for K in (2048, 16384) for B in (32, 128)]


def timed_pair(fa, fb, warmup, runs):
    """the two variants ALTERNATE call by call, so clock and allocator drift over the run falls on both alike; each call sits between
    HIP events of its own.  -> ((median, min, p90) of fa, the same of fb)"""
    import torch
    times = ([], [])
    for i in range(warmup + runs):
        for which, fn in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times[which].append(e0.elapsed_time(e1) * 1e3)
    out = []
    for t in times:
        t.sort()
        out.append((statistics.median(t), t[0], t[int(0.9 * len(t))]))
    return out


def reference_shaped_accuracy(output, mask, topk):
    """some positive among the k largest, through top-k indices and a one-hot per rank, as the reference computes it"""
    import torch
    _, pred = output.topk(max(topk), 1, True, True)
    seen = torch.zeros_like(mask, dtype=torch.long)
    res = []
    for j in range(max(topk)):
        seen = seen + torch.zeros_like(seen).scatter(1, pred[:, j:j + 1], 1)
        if j + 1 in topk:
            res.append(((seen * mask).sum(1) >= 1).float().mean(0))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=100)
    a = ap.parse_args()
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from video_similarity_search_amd.models.infoNCE import HipInfoNCEKernels, InfoNCE, UberNCE
    if not torch.cuda.is_available():
        raise SystemExit("bench_infonce needs the GPU: nothing is measured without one")

    class PoolTrunk(nn.Module):
        feature_size = FEAT

        def __init__(self):
            super().__init__()
            self.scale = nn.Parameter(torch.ones(FEAT))

        def forward(self, x):
            return x.reshape(x.shape[0], FEAT, -1).mean(-1) * self.scale

    kern = HipInfoNCEKernels()
    fmt = lambda t: "{:8.1f} [{:7.1f},{:8.1f}]".format(*t)
    lines = ["InfoNCE / UberNCE on one device, D = {}, T = {}: microseconds per call (HIP events), median of {} runs after {} warm-up "
             "calls [min, p90]; the two sides of a row alternate call by call".format(D, T, a.runs, a.warmup), "",
             "kernels: slic_moco_topk_hits (top_ks 1, 5) against slic_moco_ce_fwd, the same q, k, queue and labels",
             "{:>5} {:>6} {:>7} | {:>27} | {:>27} | {:>9}".format("B", "K", "labels", "topk_hits", "ce_fwd", "hits/ce")]
    torch.manual_seed(0)
    for B, K in SHAPES:
        q, k = (F.normalize(torch.randn(B, D, device="cuda"), dim=1) for _ in range(2))
        mem = F.normalize(torch.randn(K, D, device="cuda"), dim=1)
        ql = torch.randint(0, 64, (K,), device="cuda")
        kl = torch.randint(0, 64, (B,), device="cuda")
        for lab in (False, True):
            args = (q, k, mem, T, kl if lab else None, ql if lab else None)
            th, tc = timed_pair(lambda: kern.topk_hits(*args, (1, 5)), lambda: kern.ce_fwd(*args), a.warmup, a.runs)
            lines.append("{:>5} {:>6} {:>7} | {:>27} | {:>27} | {:>9.2f}".format(B, K, "yes" if lab else "no", fmt(th), fmt(tc), th[0] / tc[0]))
    lines += ["", "step (pooling-stub trunk, head {} -> {} -> {}): (a) contrast, fused loss + accuracies; (b) forward + torch loss + "
              "reference-shaped top-k / scatter accuracy; forward + backward".format(FEAT, FEAT, D),
              "{:>8} {:>5} {:>6} | {:>27} | {:>27} | {:>7}".format("model", "B", "K", "(a) contrast", "(b) forward + torch", "(a)/(b)")]
    for cls in (InfoNCE, UberNCE):
        for B, K in SHAPES:
            labelled = cls is UberNCE
            with contextlib.redirect_stdout(io.StringIO()):
                m = cls(PoolTrunk, D, K, 0.999, T).cuda().train()
            if labelled:
                m.queue_label.copy_(torch.randint(0, 64, (K,), device="cuda"))
            block = torch.randn(B, 2, 3, 2, 16, 16, device="cuda")
            lab = torch.randint(0, 64, (B,), device="cuda") if labelled else None

            def step_a():
                m.zero_grad(set_to_none=True)
                loss, accs = m.contrast(block, lab, (1, 5))
                loss.backward()

            def step_b():
                m.zero_grad(set_to_none=True)
                if labelled:
                    logits, mask = m(block, lab)
                    loss = (-(F.log_softmax(logits, dim=1) * mask).sum(1) / mask.sum(1)).mean()
                else:
                    logits, target = m(block)
                    loss = F.cross_entropy(logits, target)
                    mask = torch.zeros_like(logits, dtype=torch.bool)
                    mask[:, 0] = True
                reference_shaped_accuracy(logits.detach(), mask, (1, 5))
                loss.backward()

            ta, tb = timed_pair(step_a, step_b, a.warmup, a.runs)
            lines.append("{:>8} {:>5} {:>6} | {:>27} | {:>27} | {:>7.2f}".format(cls.__name__, B, K, fmt(ta), fmt(tb), ta[0] / tb[0]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

"""Linear-probe step time and the cross-entropy kernels' time (profiles/classifier_head.txt).

    python scripts/bench_classifier_head.py [--batch 32] [--depth 18] [--classes 101] [--steps 20] [--warmup 5] [--out FILE]

(a) the linear-probe step (backbone frozen, model.eval(); forward + CrossEntropyLoss + backward + SGD step) on the probe path,
(b) the same state with the path switched off (SLIC_PROBE=0): all six segments run their saving forward, as before the path existed,
(c) the eval forward alone under torch.no_grad(),
(d) slic_softmax_ce_fwd + _bwd beside torch's F.cross_entropy (+ backward) + topk on the same logits.
HIP events around every step, each row = median [min .. max] of the timed steps after the warm-up; peak memory per mode."""
import argparse
import contextlib
import io
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from video_similarity_search_amd.loss import CrossEntropyLoss, calc_topk_accuracy     # noqa: E402
from video_similarity_search_amd.models import generate_model                          # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return f"{statistics.median(ms):9.3f} ms  [{min(ms):.3f} .. {max(ms):.3f}]  n={steps}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--depth", type=int, default=18)
    ap.add_argument("--classes", type=int, default=101)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = generate_model(a.depth, n_input_channels=3, shortcut_type='B', conv1_t_size=7, conv1_t_stride=1, no_max_pool=True,
                           widen_factor=1.0, projection_head=False, classifier=True, num_classes=a.classes, dropout=0.9).cuda()
    for k, p in m.named_parameters():
        p.requires_grad_(k.startswith("linear"))
    m.eval()
    x = torch.randn(a.batch, 3, a.frames, a.size, a.size, device="cuda")
    y = torch.randint(0, a.classes, (a.batch,), device="cuda")
    crit = CrossEntropyLoss()
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-3)

    def step():
        opt.zero_grad()
        logits = m(x)
        loss = crit(logits, y)
        loss.backward()
        opt.step()
        calc_topk_accuracy(logits, y, (1, 5))

    def fwd():
        with torch.no_grad():
            m(x)

    lines = [f"linear probe, depth {a.depth}, B = {a.batch}, clip [3, {a.frames}, {a.size}, {a.size}], C = {a.classes}, "
             f"{torch.cuda.get_device_name(0)}, warm-up {a.warmup}, HIP events per step"]
    for tag, env in (("(a) probe path", "1"), ("(b) path off: six saving segments", "0")):
        os.environ["SLIC_PROBE"] = env
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        lines.append(f"{tag:40s} {timed(step, a.steps, a.warmup)}   peak {torch.cuda.max_memory_allocated() / 2 ** 20:8.0f} MiB")
    os.environ.pop("SLIC_PROBE", None)
    torch.cuda.reset_peak_memory_stats()
    lines.append(f"{'(c) eval forward alone (no_grad)':40s} {timed(fwd, a.steps, a.warmup)}   peak {torch.cuda.max_memory_allocated() / 2 ** 20:8.0f} MiB")

    logits = torch.randn(a.batch, a.classes, device="cuda")

    def ce_ours():
        lg = logits.detach().requires_grad_(True)
        crit(lg, y).backward()                     # the ranks (top-1 / top-5) come with the forward

    def ce_torch():
        lg = logits.detach().requires_grad_(True)
        torch.nn.functional.cross_entropy(lg, y).backward()
        lg.detach().topk(5, 1, True, True)

    lines.append(f"{'(d) slic_softmax_ce fwd + bwd (+ ranks)':40s} {timed(ce_ours, a.steps, a.warmup)}")
    lines.append(f"{'    torch cross_entropy fwd + bwd, topk':40s} {timed(ce_torch, a.steps, a.warmup)}")
    lines.append("    ((d) is host-bound at this size: the loss wrapper reads the bad-target flag back, one synchronisation per forward)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

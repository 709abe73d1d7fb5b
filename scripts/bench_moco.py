"""Times one MoCo step three ways on one device and writes a table:
    python scripts/bench_moco.py --out profiles/moco.txt
  (a) MemoryMoCo.softmax_loss forward + backward (the fused step);
  (b) MemoryMoCo.forward + NCESoftmaxLoss forward + backward;
  (c) the reference's op sequence (loss/NCE_loss.py:204-241 + NCESoftmaxLoss) as plain torch ops on the same device.
B in {32, 104}, D = 128, K in {2048, 16384, 65536}.  HIP events around every step, --warmup steps discarded, the median of --runs.
`--only a|b|c --shape B,K` times one cell (the driver below runs every cell as a child of its own under a time limit)."""
import argparse
import contextlib
import io
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, T = 128, 0.07
SHAPES = [(B, K) for K in (2048, 16384, 65536) for B in (32, 104)]


def one_cell(which, B, K, warmup, runs):
    import torch
    import torch.nn.functional as F
    from video_similarity_search_amd.loss.NCE_loss import MemoryMoCo, NCESoftmaxLoss
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = MemoryMoCo(D, 1000, K, T, use_softmax=True).cuda()
    m.memory.copy_(F.normalize(torch.randn(K, D, device="cuda"), dim=1))
    q = F.normalize(torch.randn(B, D, device="cuda"), dim=1).requires_grad_(True)
    k = F.normalize(torch.randn(B, D, device="cuda"), dim=1)
    crit = NCESoftmaxLoss()
    state = {"index": 0}

    def step_a():
        m.softmax_loss(q, k).backward()

    def step_b():
        crit(m(q, k)).backward()

    def step_c():
        l_pos = torch.bmm(q.view(B, 1, -1), k.view(B, -1, 1)).view(B, 1)
        queue = m.memory.clone()
        l_neg = torch.mm(queue.detach(), q.transpose(1, 0)).transpose(0, 1)
        out = torch.div(torch.cat((l_pos, l_neg), dim=1), T).contiguous()
        loss = F.cross_entropy(out, torch.zeros(B, dtype=torch.long, device="cuda"))
        with torch.no_grad():
            ids = torch.fmod(torch.arange(B, device="cuda") + state["index"], K).long()
            m.memory.index_copy_(0, ids, k)
            state["index"] = (state["index"] + B) % K
        loss.backward()

    step = {"a": step_a, "b": step_b, "c": step_c}[which]
    times = []
    for i in range(warmup + runs):
        q.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1) * 1e3)
    times.sort()
    print("RESULT {} {} {} {:.1f} {:.1f} {:.1f}".format(which, B, K, statistics.median(times), times[0], times[int(0.9 * len(times))]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--only", default=None)
    ap.add_argument("--shape", default=None)
    ap.add_argument("--cell-timeout", type=int, default=90)
    a = ap.parse_args()
    if a.only:
        B, K = (int(v) for v in a.shape.split(","))
        one_cell(a.only, B, K, a.warmup, a.runs)
        return
    rows = {}
    for B, K in SHAPES:
        for which in "abc":
            # a fresh child per cell, one at a time, each under its own limit; a failed or overdue cell ends the run
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", which, "--shape", "{},{}".format(B, K),
                                "--warmup", str(a.warmup), "--runs", str(a.runs)], capture_output=True, text=True, timeout=a.cell_timeout)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit("cell {} B={} K={} failed (rc={})".format(which, B, K, r.returncode))
            rows[(which, B, K)] = [float(v) for v in line[0].split()[4:]]
    lines = ["MoCo step, D = {}, T = {}: microseconds per step (HIP events), median of {} runs after {} warm-up steps [min, p90]".format(D, T, a.runs, a.warmup),
             "  (a) MemoryMoCo.softmax_loss fwd + bwd   (b) MemoryMoCo.forward + NCESoftmaxLoss fwd + bwd   (c) the reference's torch ops, same device",
             "{:>5} {:>6} | {:>24} | {:>24} | {:>24} | {:>7} | {}".format("B", "K", "(a) fused", "(b) unfused", "(c) torch ops", "(a)/(c)", "queue MB")]
    for B, K in SHAPES:
        cell = lambda w: "{:8.1f} [{:6.1f},{:7.1f}]".format(*rows[(w, B, K)])
        lines.append("{:>5} {:>6} | {:>24} | {:>24} | {:>24} | {:>7.2f} | {:.1f}".format(
            B, K, cell("a"), cell("b"), cell("c"), rows[("a", B, K)][0] / rows[("c", B, K)][0], K * D * 4 / 2 ** 20))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

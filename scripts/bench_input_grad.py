"""The clip's gradient on the device: the stem data-gradient kernel against the generic kernels, and what asking for x.grad costs a
training step.

    python scripts/bench_input_grad.py [--reps 7] [--warmup 2] [--out profiles/input_grad.txt]

Kernel rows (one JSON line per batch size, B = 32 and B = 8, clip 3 x 16 x 112 x 112, N = 64): ConvPlan.input_grad — weights
already packed — through
  fast      slic_conv_stem_dgrad (csrc/stem_dgrad.hip), and
  fallback  SLIC_STEM_DGRAD=0: a non-W-run plan on slic_conv_gemm's data-gradient geometry (four parity classes, 3 channels padded to 4
            on 64-column tiles) + the copy to NCDHW — what the library could do before the kernel existed.
The two alternate inside every repeat; a repeat is a device-event pair around `--calls` back-to-back calls.  ms = median over the
repeats, spread = (min, max).  real TFLOP/s = 2 B To Ho Wo N C 343 over the time (the gradient's own multiply-adds: the floor at
157.3 TFLOP/s is 1.34 ms at B = 32), executed TFLOP/s = 448 x 16 / (343 x 12) = 1.74 x that (zero tap slots and pad columns the
kernel multiplies).  max_diff: fast against fallback on the timed inputs, asserted at the gate of the tests
((2e-6 sqrt(N 343 / 4) + 1e-6) max(1, |g|max)).

Step rows (B = 32 and B = 8): one R3D-18 + NT-Xent training step (forward, loss, backward, SGD update — bench.py's step) with the
clip requiring a gradient and without, alternating, device events around each step.
A machine without a device fails here: nothing is measured on the CPU.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_similarity_search_amd.models import generate_model  # noqa: E402
from video_similarity_search_amd.models.conv_plan import ConvPlan  # noqa: E402
from video_similarity_search_amd.loss import OnlineTripletLoss  # noqa: E402

PEAK_TFLOPS = 157.3                      # fp32 MFMA / vector peak of an MI355X
C, N, KERNEL, STRIDE, PAD, DIMS = 3, 64, (7, 7, 7), (1, 2, 2), (3, 3, 3), (16, 112, 112)
R3D18_KW = dict(hidden_layer=2048, out_dim=128, num_classes=101, n_input_channels=3, shortcut_type='B',
                conv1_t_size=7, conv1_t_stride=1, no_max_pool=True, widen_factor=1.0, projection_head=True,
                predict_temporal_ds=False, spatio_temporal_attention=False, classifier=False, dropout=None)


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def summary(ts):
    return dict(ms=round(statistics.median(ts), 3), spread=[round(min(ts), 3), round(max(ts), 3)])


def kernel_row(B, reps, warmup, calls):
    g = torch.Generator(device="cuda").manual_seed(B)
    plan = ConvPlan(C, N, KERNEL, STRIDE, PAD, DIMS, "cuda")
    w = torch.randn((N, C) + KERNEL, device="cuda", generator=g) / np.sqrt(N * 343 / 4)
    dz = torch.randn((B,) + plan.out_dims + (N,), device="cuda", generator=g)
    outs = {v: torch.empty((B, C) + DIMS, device="cuda") for v in ("fast", "fallback")}

    def run(v):
        os.environ["SLIC_STEM_DGRAD"] = "1" if v == "fast" else "0"
        plan.input_grad(dz, w, B, out=outs[v])

    times = {"fast": [], "fallback": []}
    try:
        for v in times:
            for _ in range(warmup):
                run(v)
        torch.cuda.synchronize()
        for _ in range(reps):
            for v in times:
                times[v].append(timed(lambda: run(v), calls))
    finally:
        os.environ.pop("SLIC_STEM_DGRAD", None)
    gmax = outs["fallback"].abs().max().item()
    diff = (outs["fast"] - outs["fallback"]).abs().max().item()
    gate = (2e-6 * np.sqrt(N * 343 / 4) + 1e-6) * max(1.0, gmax)
    real = 2.0 * B * int(np.prod(plan.out_dims)) * N * C * 343
    row = dict(what="kernel", B=B, clip=[C] + list(DIMS), N=N, calls_per_repeat=calls, repeats=reps,
               real_tflop=round(real / 1e12, 4), floor_ms=round(real / (PEAK_TFLOPS * 1e12) * 1e3, 3), max_diff=diff, gate=gate)
    for v, ts in times.items():
        s = summary(ts)
        row[v] = dict(s, real_tflops=round(real / s["ms"] / 1e9, 1))
    row["fast"]["executed_tflops"] = round(real * 448 * 16 / (343 * 12) / row["fast"]["ms"] / 1e9, 1)
    row["fast"]["floor_share"] = round(row["floor_ms"] / row["fast"]["ms"], 3)
    row["speedup"] = round(row["fallback"]["ms"] / row["fast"]["ms"], 2)
    row["faster_beyond_spread"] = bool(row["fast"]["spread"][1] < row["fallback"]["spread"][0])
    print(json.dumps(row), flush=True)
    assert diff <= gate, (diff, gate)
    return row


def step_row(B, reps, warmup):
    with contextlib.redirect_stdout(io.StringIO()):
        model = generate_model(18, **R3D18_KW).cuda().train()
    crit = OnlineTripletLoss(0.2, 'cosine')
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.5)
    x = torch.from_numpy(np.random.default_rng(7).standard_normal((B, 3, 16, 112, 112)).astype(np.float32)).cuda()
    labels = torch.arange(B // 2).repeat(2).cuda()

    def step(with_grad):
        xin = x.detach().requires_grad_(with_grad)
        loss, _ = crit(model(xin), labels, sampling_strategy='noise_contrastive')
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        assert (xin.grad is not None) == with_grad

    times = {"without": [], "with_clip_grad": []}
    for _ in range(warmup):
        step(False)
        step(True)
    torch.cuda.synchronize()
    for _ in range(reps):
        for name in times:
            times[name].append(timed(lambda: step(name == "with_clip_grad"), 1))
    row = dict(what="train_step", B=B, repeats=reps, **{k: summary(v) for k, v in times.items()})
    row["clip_grad_cost_ms"] = round(row["with_clip_grad"]["ms"] - row["without"]["ms"], 3)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--step-reps", type=int, default=12)
    ap.add_argument("--batches", default="32,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_grad.py needs a gfx950 device: nothing is measured on the CPU")
    torch.cuda.set_device(0)
    batches = [int(v) for v in a.batches.split(",")]
    rows = [kernel_row(B, a.reps, a.warmup, a.calls) for B in batches]
    rows += [step_row(B, a.step_reps, max(a.warmup, 3)) for B in batches]
    if a.out:
        with open(a.out, "w") as f:
            f.write("# scripts/bench_input_grad.py --reps {} --warmup {} --calls {} --step-reps {} on {}\n".format(
                a.reps, a.warmup, a.calls, a.step_reps, torch.cuda.get_device_name(0)))
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

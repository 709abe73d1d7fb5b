"""cosine_topk: the fp32 search against the certified bf16 candidate search (precision="bf16"), interleaved in one process.

    python scripts/bench_topk_bf16.py [--reps 9] [--warmup 2] [--nq 10000] [--ng 100000] [--d 512] [--no-trace] [--out FILE]

* 10 000 x 100 000 x 512 (bench.py's configs[4]), k in {1, 16, 50, 88}; data: flat Gaussian rows, and a clustered gallery (40 directions
  + 0.05 noise, queries = gallery rows + 0.3 noise);
* per cell: device-event time of the whole wrapper call (normalisation included, the same on both sides), A and B alternating call by
  call after a warm-up of each; median, minimum, and the fp32 side's own run-to-run spread (max - min over its reps) — bf16 is "ahead"
  only if its median beats the fp32 median by more than that spread;
* the bf16 side runs with SLIC_TOPK_BF16=1 (the kernels under test whatever the library's own choice is); its fallback share and mean
  candidates per query come from one extra call with info=;
* the kernels' split: one child process under `rocprofv3 --kernel-trace --stats` runs three bf16 calls at k = 50 on the Gaussian data.
Everything printed also goes to --out (profiles/topk_bf16.txt is a run of this script).
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from video_similarity_search_amd.evaluate import cosine_topk  # noqa: E402

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def make_data(kind, Nq, Ng, D, seed=5):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "gaussian":
        return torch.randn(Nq, D, device="cuda", generator=gen), torch.randn(Ng, D, device="cuda", generator=gen)
    cent = torch.randn(40, D, device="cuda", generator=gen)
    G = cent[torch.randint(0, 40, (Ng,), device="cuda", generator=gen)] + 0.05 * torch.randn(Ng, D, device="cuda", generator=gen)
    Q = G[torch.randint(0, Ng, (Nq,), device="cuda", generator=gen)] + 0.3 * torch.randn(Nq, D, device="cuda", generator=gen)
    return Q, G


def bf16_call(Q, G, k, info=None):
    os.environ["SLIC_TOPK_BF16"] = "1"
    try:
        return cosine_topk(Q, G, k=k, precision="bf16", info=info)
    finally:
        del os.environ["SLIC_TOPK_BF16"]


def ab(a):
    say("# %d x %d x %d; ms per cosine_topk call (device events), fp32 / bf16 alternating, %d reps after %d warm-up calls each"
        % (a.nq, a.ng, a.d, a.reps, a.warmup))
    say("%-10s %3s  %8s %8s %8s   %8s %8s   %7s  %9s %9s %10s" % ("data", "k", "fp32 med", "fp32 min", "spread", "bf16 med", "bf16 min",
                                                                 "ratio", "fallback", "overflow", "cand/query"))
    for kind in ("gaussian", "clustered"):
        Q, G = make_data(kind, a.nq, a.ng, a.d)
        for k in (1, 16, 50, 88):
            fns = {"fp32": lambda: cosine_topk(Q, G, k=k), "bf16": lambda: bf16_call(Q, G, k)}
            for _ in range(a.warmup):
                for f in fns.values():
                    f()
            torch.cuda.synchronize()
            ts = {m: [] for m in fns}
            for _ in range(a.reps):
                for m, f in fns.items():
                    ts[m].append(_timed(f))
            info = {}
            ib, db = bf16_call(Q, G, k, info)
            ia, da = cosine_topk(Q, G, k=k)
            same = float((ia == ib).float().mean().item())
            dmax = float((da - db).abs().max().item())
            f32, b16 = np.array(ts["fp32"]), np.array(ts["bf16"])
            spread = float(f32.max() - f32.min())
            ahead = float(np.median(f32) - np.median(b16)) > spread
            say("%-10s %3d  %8.3f %8.3f %8.3f   %8.3f %8.3f   %7.3f  %8.2f%% %8.2f%% %10.1f   %s  (indices equal %.5f, max |d dist| %.1e, path %s)"
                % (kind, k, np.median(f32), f32.min(), spread, np.median(b16), b16.min(), np.median(b16) / np.median(f32),
                   100.0 * info["fallback_queries"] / a.nq, 100.0 * info["overflow_queries"] / a.nq, info["candidates"] / a.nq,
                   "bf16 ahead" if ahead else "not ahead", same, dmax, info["path"]))
        del Q, G
        torch.cuda.empty_cache()


def child(a):
    Q, G = make_data("gaussian", a.nq, a.ng, a.d)
    for _ in range(3):
        bf16_call(Q, G, 50)
    torch.cuda.synchronize()


def trace(a):
    """the kernels of a bf16 call at k = 50, from a child process of its own under rocprofv3"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child",
               "--nq", str(a.nq), "--ng", str(a.ng), "--d", str(a.d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        f = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
        if r.returncode != 0 or not f:
            say("# kernel split: rocprofv3 run failed (exit %d)\n%s" % (r.returncode, r.stderr[-800:]))
            return
        say("# kernels of 3 bf16 calls at k = 50, Gaussian rows (rocprofv3 --kernel-trace --stats): name, calls, average us, share of device time")
        for row in csv.DictReader(open(f[-1])):
            name = row["Name"]
            name = name if len(name) <= 90 else name[:87] + "..."
            say("%-90s %4s %10.1f %6.2f%%" % (name, row["Calls"], float(row["AverageNs"]) / 1e3, float(row["Percentage"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--ng", type=int, default=100000)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.no_trace:
        trace(a)                                   # before this process opens the device
    ab(a)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

"""The clip augmentation chain of a training batch, fused (coclr_utils.transforms.Compose.batch: one parameter upload, one or two
launches) against the same chain as plain torch ops on the same device (what a user of the reference's module runs today: a launch per
op and per clip, each reading and writing the fp32 clip).

    python scripts/bench_clip_transforms.py [--reps 20] [--warmup 3] [--out profiles/clip_transforms.txt]

Chain: ToFloatTensorInZeroOne -> RandomSizedCrop((112, 112)) -> RandomHorizontalFlip -> ColorJitter(0.4, 0.4, 0.4, consistent=True) ->
RandomGray(0.2) -> Normalize, and the same without the contrast op (no stats launch).  B = 32 clips of N = 16 frames, 128 x 171 uint8.
Both sides get the same parameters: the fused side draws them (seeded per repetition), the torch side reads them off the plan, and the
two outputs are compared (max_abs_diff).  One JSON line per case:
  fused_ms / fused_ms_min, torch_ms / torch_ms_min   device events around the whole call, host planning included; median and minimum
  ratio                                              torch_ms / fused_ms
  kernel_ms / kernel_ms_min                          device events around the table upload and the launches alone (the host has planned)
  fused_bytes, kernel_hbm_share                      bytes the fused kernels must move (the uint8 crop windows once per launch that
                                                     reads them + the fp32 output once) over kernel_ms_min, as a share of the 6.29 TB/s
                                                     a float4 copy reaches on this part (8.0 TB/s is the HBM3E peak)
A machine without a device fails here: nothing is measured on the CPU.
"""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_similarity_search_amd.coclr_utils import transforms as T  # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
HBM_COPY_RATE = 6.29e12
SIZE = (112, 112)


class _Timed(T.HipClipKernels):
    """device events around the upload and the launches"""

    def __init__(self):
        self.pairs = []

    def launch(self, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = super().launch(*a)
        e1.record()
        self.pairs.append((e0, e1))
        return out


def chain(contrast, kernels=None):
    return T.Compose([T.ToFloatTensorInZeroOne(), T.RandomSizedCrop(SIZE), T.RandomHorizontalFlip(),
                      T.ColorJitter(0.4, 0.4 if contrast else 0, 0.4, consistent=True), T.RandomGray(0.2), T.Normalize(MEAN, STD)],
                     kernels=kernels)


def seed(s):
    random.seed(s)
    np.random.seed(s)


def torch_clip(clip, g):
    """one clip through the chain as separate torch ops, with the parameters of the planned group g"""
    dev = clip.device
    N = g.N
    v = clip.permute(3, 0, 1, 2).to(torch.float32) / 255
    a = g.a
    v = v[..., a.dy:a.dy + a.H, a.dx:a.dx + a.W]
    v = F.interpolate(v, size=SIZE, mode='bilinear', align_corners=False)
    if g.b.mx < 0:
        v = v.flip(dims=(-1,))

    def gray(x):
        return (0.2989 * x[0] + 0.5870 * x[1] + 0.1140 * x[2]).unsqueeze(0)

    for kind, fac in g.ops:
        f = torch.from_numpy(fac).to(dev).view(1, N, 1, 1)
        if kind == T.GRAY:
            v = gray(v) * f + v * (1 - f)
        else:
            other = 0 if kind == T.BRIGHTNESS else gray(v).mean(3, keepdim=True).mean(2, keepdim=True) if kind == T.CONTRAST else gray(v)
            v = (f * v + (1 - f) * other).clamp(0, 1)
    mean = torch.as_tensor(MEAN).to(dev).view(3, 1, 1, 1)
    std = torch.as_tensor(STD).to(dev).view(3, 1, 1, 1)
    return (v - mean) / std


def timed(fn, reps, warmup):
    out = None
    for i in range(warmup):
        out = fn(1000 + i)
    times = []
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn(i)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return out, times


def run_case(contrast, B, N, H, W, reps, warmup):
    g = torch.Generator(device="cuda").manual_seed(7)
    clips = torch.randint(0, 256, (B, N, H, W, 3), device="cuda", dtype=torch.uint8, generator=g)
    c = chain(contrast)

    def fused(s):
        seed(s)
        return c.batch(clips)

    def plain(s):
        seed(s)
        plans = [c.plan(clip) for clip in clips]                       # the draws; nothing runs
        return torch.stack([torch_clip(clip, p.groups()[0]) for clip, p in zip(clips, plans)])

    a, tf = timed(fused, reps, warmup)
    b, tt = timed(plain, reps, warmup)
    k = _Timed()
    ck = chain(contrast, k)
    for i in range(reps):
        seed(i)
        ck.batch(clips)
    torch.cuda.synchronize()
    tk = [e0.elapsed_time(e1) for e0, e1 in k.pairs]
    seed(reps - 1)
    groups = [c.plan(clip).groups()[0] for clip in clips]
    window = sum(3 * N * g_.a.H * g_.a.W for g_ in groups)
    launches = 2 if any(g_.has_contrast for g_ in groups) else 1
    nbytes = window * launches + 4 * a.numel()
    row = dict(chain="bench chain" if contrast else "bench chain without contrast", B=B, N=N, source=[H, W], out=list(a.shape),
               launches=launches, fused_ms=round(statistics.median(tf), 4), fused_ms_min=round(min(tf), 4),
               torch_ms=round(statistics.median(tt), 4), torch_ms_min=round(min(tt), 4),
               ratio=round(statistics.median(tt) / statistics.median(tf), 2), max_abs_diff=float((a - b).abs().max()),
               kernel_ms=round(statistics.median(tk), 4), kernel_ms_min=round(min(tk), 4),
               fused_bytes=int(nbytes), kernel_hbm_share=round(nbytes / (min(tk) * 1e-3) / HBM_COPY_RATE, 3))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_transforms.py needs a gfx950 device: nothing is measured on the CPU")
    torch.cuda.set_device(0)
    rows = [run_case(contrast, a.batch, 16, 128, 171, a.reps, a.warmup) for contrast in (True, False)]
    if a.out:
        with open(a.out, "w") as f:
            f.write("# scripts/bench_clip_transforms.py --reps {} --warmup {} on {}\n".format(a.reps, a.warmup, torch.cuda.get_device_name(0)))
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Pair statistics (slic_pair_stats) at the cluster step's sizes, next to two yardsticks:
  (a) the count pass of slic_dbscan_cosine at the same N and D (SLIC_DBSCAN_TIMING=1: prep + count) — the same streamed GEMM with a
      one-comparison epilogue (eps = 0: no score reaches the band), which shows what the histogram epilogue costs (self form only);
  (b) the same statistics as torch ops in row chunks on the same device (GEMM, clamp, bin, bincount, masked float64 sums).

    python scripts/bench_pair_stats.py [--out profiles/pair_stats.txt]

Device events around every call, warm-up first, the sides alternating call by call inside one loop, median of --reps (max - min as the
spread).  slic_pair_stats is timed with one LDS table per workgroup (what runs) and, with SLIC_PAIR_STATS_TABLES=4 where that fits
(bins <= 1024), with one table per wave.  Rows: flat Gaussian rows (every distance near 1: the concentrated case) and
rows around 101 centres; 101 labels either way.  The counts of (b) are checked against the call's.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OUT = []
SHAPES = ((20000, None, 128), (100000, None, 128), (10000, 100000, 128))
BINS = (64, 256, 4096)
CLASSES = 101


def say(s):
    print(s, flush=True)
    OUT.append(s)


def make_rows(kind, N, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lab = torch.randint(0, CLASSES, (N,), generator=g, device="cuda", dtype=torch.int32)
    x = torch.randn(N, D, generator=g, device="cuda")
    if kind == "clustered":
        cen = torch.randn(CLASSES, D, generator=torch.Generator(device="cuda").manual_seed(7), device="cuda")
        x = cen[lab.long()] + 0.5 * x
    return x.contiguous(), lab


def pair_stats_call(x, lx, y, ly, bins):
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd._lib import call, ptr, stream
    Nx, D = x.shape
    Ny = 0 if y is None else y.shape[0]
    ws = torch.empty(_lib.load().slic_pair_stats_workspace_bytes(Nx, Ny, D, bins), dtype=torch.uint8, device="cuda")
    out = torch.empty(2 * bins + 9, dtype=torch.int64, device="cuda")

    def fn():
        call("slic_pair_stats", ptr(x), Nx, x.stride(0), ptr(lx), ptr(y), Ny, 0 if y is None else y.stride(0), ptr(ly), D, bins, 0, 0, 2.0,
             ptr(out), ptr(out[2 * bins:]), ptr(ws), stream())
    return fn, out


def dbscan_count_call(x):
    """-> a closure that runs slic_dbscan_cosine(eps = 0, min_samples = 2) and returns the ms of its prep and count passes"""
    import ctypes
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd._lib import call, ptr, stream
    N, D = x.shape
    ws = torch.empty(_lib.load().slic_dbscan_cosine_workspace_bytes(N, D), dtype=torch.uint8, device="cuda")
    labels = torch.empty(N, dtype=torch.int32, device="cuda")
    core = torch.empty(N, dtype=torch.uint8, device="cuda")
    ncl = torch.empty(1, dtype=torch.int32, device="cuda")
    host = (ctypes.c_double * 10)()

    def fn():
        os.environ["SLIC_DBSCAN_TIMING"] = "1"
        try:
            call("slic_dbscan_cosine", ptr(x), N, x.stride(0), D, 0.0, 2, ptr(labels), ptr(core), None, ptr(ncl), ptr(ws), stream())
            call("slic_dbscan_cosine_stats", ptr(ws), host, stream())
        finally:
            os.environ.pop("SLIC_DBSCAN_TIMING", None)
        return host[4], host[5]
    return fn


def torch_call(x, lx, y, ly, bins, chunk=4096):
    """the statistics as torch ops: -> a closure returning (counts int64 [2, bins], sums float64 [6])"""
    self_form = y is None
    ly = lx if self_form else ly
    cols = torch.arange((x if self_form else y).shape[0], device="cuda")

    def fn():
        xn = torch.nn.functional.normalize(x, dim=1)
        yn = xn if self_form else torch.nn.functional.normalize(y, dim=1)
        counts = torch.zeros(2 * bins + 1, dtype=torch.int64, device="cuda")
        sums = torch.zeros(6, dtype=torch.float64, device="cuda")
        for i0 in range(0, xn.shape[0], chunk):
            i1 = min(i0 + chunk, xn.shape[0])
            yy, ll, cc = (yn[i0:], ly[i0:], cols[i0:]) if self_form else (yn, ly, cols)       # the columns at or right of the chunk
            d = (1.0 - xn[i0:i1] @ yy.T).clamp_(0.0, 2.0)
            same = lx[i0:i1, None] == ll[None, :]
            idx = (d * (bins / 2)).long().clamp_(max=bins - 1) + same.long() * bins
            if self_form:
                valid = cc[None, :] > torch.arange(i0, i1, device="cuda")[:, None]
                idx = torch.where(valid, idx, 2 * bins)
                d = torch.where(valid, d, 0.0)
                e = torch.where(valid, torch.exp(-4.0 * d), 0.0)
            else:
                e = torch.exp(-4.0 * d)
            counts += torch.bincount(idx.reshape(-1), minlength=2 * bins + 1)
            ds, es = torch.where(same, d, 0.0), torch.where(same, e, 0.0)
            tot = torch.stack([d.sum(dtype=torch.float64), ds.sum(dtype=torch.float64), (d * d).sum(dtype=torch.float64),
                               (ds * ds).sum(dtype=torch.float64), e.sum(dtype=torch.float64), es.sum(dtype=torch.float64)])
            sums += torch.stack([tot[0] - tot[1], tot[1], tot[2] - tot[3], tot[3], tot[4] - tot[5], tot[5]])
        return counts[:2 * bins].reshape(2, bins), sums
    return fn


def timed_alternating(sides, reps, warm=3):
    """sides: {name: closure}; every repetition runs each side once, in turn -> {name: ms array}.  A closure that returns a pair of
    floats (the DBSCAN passes) is timed by that pair's sum instead of the events around it."""
    t = {k: [] for k in sides}
    for i in range(reps + warm):
        for k, fn in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r = fn()
            b.record()
            b.synchronize()
            if i >= warm:
                t[k].append(sum(r) if isinstance(r, tuple) and len(r) == 2 and isinstance(r[0], float) else a.elapsed_time(b))
    return {k: np.array(v) for k, v in t.items()}


def med(v):
    return "%9.3f ms (spread %7.3f)" % (np.median(v), v.max() - v.min())


def shape(Nx, Ny, D, reps, kinds, bins_list):
    for kind in kinds:
        x, lx = make_rows(kind, Nx, D, 1)
        y, ly = (None, None) if Ny is None else make_rows(kind, Ny, D, 2)
        pairs = Nx * (Nx - 1) // 2 if Ny is None else Nx * Ny
        for bins in bins_list:
            fn, out = pair_stats_call(x, lx, y, ly, bins)
            tfn = torch_call(x, lx, y, ly, bins)

            def per_wave():
                os.environ["SLIC_PAIR_STATS_TABLES"] = "4"
                try:
                    fn()
                finally:
                    os.environ.pop("SLIC_PAIR_STATS_TABLES", None)

            sides = {"call": fn}
            if bins <= 1024:
                sides["per_wave"] = per_wave
            if Ny is None:
                sides["dbscan"] = dbscan_count_call(x)
            sides["torch"] = tfn
            t = timed_alternating(sides, reps)
            fn()
            got = out.cpu().numpy()
            hist, rec = got[:2 * bins].reshape(2, bins), got[2 * bins:].view(np.float64)
            tc, tsum = tfn()
            tc, tsum = tc.cpu().numpy(), tsum.cpu().numpy()
            moved = int(np.abs(np.cumsum(hist, 1) - np.cumsum(tc, 1)).max())
            ok = hist.sum() == pairs and tc.sum() == pairs and (hist.sum(1) == tc.sum(1)).all()
            line = "%6d x %6s x %3d %-9s bins %4d | pair_stats %s" % (Nx, "self" if Ny is None else Ny, D, kind, bins, med(t["call"]))
            if "per_wave" in t:
                line += " | one table per wave %s" % med(t["per_wave"])
            if "dbscan" in t:
                line += " | dbscan prep + count %s | pair_stats / that %.2f" % (med(t["dbscan"]), np.median(t["call"]) / np.median(t["dbscan"]))
            line += " | torch %s | torch / pair_stats %.2f" % (med(t["torch"]), np.median(t["torch"]) / np.median(t["call"]))
            line += " | %.1f Gpairs/s | counts %s, largest cumulative count apart from torch's %d, mean d diff %.6f (torch %.6f)" % (
                pairs / np.median(t["call"]) / 1e6, "agree" if ok else "DIFFER", moved, rec[2] / max(rec[0], 1), tsum[0] / max(tc[0].sum(), 1))
            say(line)
        del x, lx, y, ly
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", type=int, nargs="*", default=None, help="indices into SHAPES (default: all)")
    ap.add_argument("--kinds", nargs="*", default=["flat", "clustered"])
    ap.add_argument("--bins", type=int, nargs="*", default=list(BINS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        say("# NOTE: --reps %d is below the 20 the figures in profiles/pair_stats.txt were taken with" % a.reps)
    say("# slic_pair_stats (t = 2) vs the DBSCAN count pass and vs torch ops in row chunks; %s; median of %d, sides alternating"
        % (torch.cuda.get_device_name(0), a.reps))
    for i, (Nx, Ny, D) in enumerate(SHAPES):
        if a.shapes is None or i in a.shapes:
            shape(Nx, Ny, D, a.reps, a.kinds, a.bins)
            if a.out:
                with open(a.out, "w") as f:
                    f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Exact t-SNE on the device (csrc/tsne.hip, manifold.TSNE) at N = 2 000 / 10 000 / 20 000, D = 50, next to sklearn on the host.

    python scripts/bench_tsne.py [--out profiles/tsne.txt]          the device part (needs the MI355X)
    python scripts/bench_tsne.py --host [--out ...]                 sklearn on the host: method='exact' at 2 000, 'barnes_hut' at
                                                                    2 000 and 10 000 (one run each: they take minutes)

Device method: HIP events around the work, warm-up first, medians of whole runs.
* the three once-per-fit passes (squared distances, the perplexity search, the symmetrisation): one event pair each, median of 5;
* one iteration: an event pair around 200 consecutive slic_tsne_step calls (three launches each, no read-back), median of 7 such
  runs, without and with the KL pieces; beside it the rate at which the pass reads P (N^2 x 4 bytes over the time of one iteration,
  which holds all three launches) and that rate over 6.29 TB/s, the float4-copy rate measured on this device, and over the 8 TB/s
  of its data sheet.  P at N = 2 000 is 16 MB and lives in the caches; at 10 000 (400 MB) and 20 000 (1.6 GB) it comes from HBM;
* the whole fit: TSNE(perplexity=30, init='random', random_state=0).fit, an event pair around it (it ends in the read-back of the
  embedding), median of 3; max_iter = 1000.
Rows: six Gaussian blobs (centres 4 N(0, 1), rows centre + N(0, 1)), the generator of the tests.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OUT = []
SIZES = (2000, 10000, 20000)
D = 50
COPY_RATE, SPEC_RATE = 6.29e12, 8.0e12


def say(s):
    print(s, flush=True)
    OUT.append(s)


def blobs(N, seed=0):
    rs = np.random.RandomState(seed)
    centres = 4.0 * rs.standard_normal((6, D))
    return (centres[rs.randint(0, 6, N)] + rs.standard_normal((N, D))).astype(np.float32)


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def device(sizes, fits):
    import torch
    from video_similarity_search_amd import TSNE
    from video_similarity_search_amd.manifold import HipTsneKernels
    k = HipTsneKernels()
    say("# exact t-SNE, dense P, D = %d, perplexity 30; %s" % (D, torch.cuda.get_device_name(0)))
    for N in sizes:
        X = blobs(N)
        x = k.rows(X)
        t = {"sqdist": [], "cond_p": [], "symmetrize": []}
        for rep in range(6):                                    # the first is the warm-up
            ms, P = event_ms(lambda: k.sqdist(x))
            t["sqdist"].append(ms)
            t["cond_p"].append(event_ms(lambda: k.cond_p(P, 30.0))[0])
            t["symmetrize"].append(event_ms(lambda: k.symmetrize(P))[0])
            if rep < 5:
                del P
        once = {n: float(np.median(v[1:])) for n, v in t.items()}
        Y0 = (1e-4 * np.random.RandomState(0).standard_normal((N, 2))).astype(np.float32)
        per = {}
        for want_kl in (False, True):
            runs = []
            for rep in range(8):
                st = k.start(Y0, P)
                for _ in range(250 if rep else 20):             # past the exaggerated stage's first steps: the points have moved apart
                    k.step(P, st, 12.0, 0.5, max(N / 48.0, 50.0), False)

                def many():
                    for _ in range(200):
                        k.step(P, st, 1.0, 0.8, max(N / 48.0, 50.0), want_kl)
                ms = event_ms(many)[0]
                if rep:
                    runs.append(ms / 200.0)
            per[want_kl] = np.array(runs)
        it = float(np.median(per[False]))
        rate = N * N * 4.0 / (it * 1e-3)
        say("N = %6d | once per fit: distances %.3f ms, perplexity search %.3f ms, symmetrise %.3f ms | one iteration %.4f ms "
            "(spread %.4f; with the KL pieces %.4f ms) | P read at %.2f TB/s = %.0f %% of the measured copy rate, %.0f %% of the data sheet"
            % (N, once["sqdist"], once["cond_p"], once["symmetrize"], it, per[False].max() - per[False].min(), float(np.median(per[True])),
               rate / 1e12, 100 * rate / COPY_RATE, 100 * rate / SPEC_RATE))
        del P
        torch.cuda.empty_cache()
        ft = []
        for rep in range(fits + 1):
            m = TSNE(perplexity=30, init="random", random_state=0)
            ft.append(event_ms(lambda: m.fit(x))[0])
        ft = np.array(ft[1:])
        say("N = %6d | whole fit (1000 iterations, 20 record reads) %.1f ms (median of %d, spread %.1f) | KL %.4f, n_iter_ %d"
            % (N, float(np.median(ft)), fits, ft.max() - ft.min(), m.kl_divergence_, m.n_iter_))


def host():
    import sklearn
    from sklearn.manifold import TSNE
    say("# sklearn %s on the host (%d CPUs visible), D = %d, perplexity 30, init='random', one run each" % (sklearn.__version__, os.cpu_count(), D))
    for method, N in (("exact", 2000), ("barnes_hut", 2000), ("barnes_hut", 10000)):
        X = blobs(N)
        t0 = time.perf_counter()
        m = TSNE(n_components=2, perplexity=30, method=method, init="random", random_state=0).fit(X)
        say("sklearn method=%-10s N = %6d | whole fit %.1f s | KL %.4f, n_iter_ %d" % (method, N, time.perf_counter() - t0, m.kl_divergence_, m.n_iter_))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true", help="time sklearn on the host instead of the device")
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--fits", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.host:
        host()
    else:
        device(a.sizes, a.fits)
    if a.out:
        with open(a.out, "a" if os.path.exists(a.out) else "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()

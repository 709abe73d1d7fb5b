"""Generates tests/golden/kmeanspp_picks.npz: the rows the device k-means++ seeding picks, recorded from the library itself
(needs a gfx950 device; a record of what the kernels compute, not an outside reference):

    python tests/golden/make_goldens_kmeanspp.py            # writes the file
    python tests/golden/make_goldens_kmeanspp.py --check    # regenerates and compares with the file instead

The other k-means++ tests compare the paths with each other and, on well-separated blobs, with a float64 restatement.  This file pins
the picks where the order of the summations decides: every shape is drawn once as blobs and once as plain standard_normal, which has
no structure, so a pick depends on the last bits of the potentials and the chunk sums.  A change that moves both paths the same way
shows here.

Single runs (slic_kmeanspp_run), each recorded without the permuted copy (kpp_dist_rows, VALU) and with it (matrix pipe):
    333 x 8,  K 5      fewer rows than one 128-row block, last 64-row chunk partial, one k-tile, T = 3
    4130 x 40, K 24    65 chunks (odd: the last workgroup has no second chunk), partial tail k-tile, T = 5
    6000 x 64, K 24    the shape of test_kmeanspp_run_matches_stepwise
    2200 x 16, K 1100  T = 9: kpp_dist_rows<16> on the VALU path
Lock-step runs (slic_kmeanspp_run_batch), R * T candidate rows = 1 .. 5 MFMA row tiles (5 is the limit):
    333 x 8 K 5 R 3 (9 rows) | 4130 x 40 K 24 R 10 (50) | 1500 x 64 K 60 R 13 (78) | 3000 x 64 K 60 R 20 (120) | 2000 x 32 K 410 R 20 (160)

Per case the file holds the picks only, plus the float64 sums of X and of the uniforms (a guard: the inputs are regenerated from the
seed by whoever reads the file, tests/test_kmeanspp_picks_gpu.py)."""
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kmeanspp_picks.npz")
SINGLE = [(333, 8, 5), (4130, 40, 24), (6000, 64, 24), (2200, 16, 1100)]
BATCH = [(333, 8, 5, 3), (4130, 40, 24, 10), (1500, 64, 60, 13), (3000, 64, 60, 20), (2000, 32, 410, 20)]
KINDS = ("blobs", "normal")


def name(N, D, K, kind, R=0):
    return ("batch_{}x{}_k{}_r{}_{}" if R else "single_{}x{}_k{}_{}").format(*((N, D, K, R, kind) if R else (N, D, K, kind)))


def inputs(N, D, K, kind, R=0):
    """X, T, uniforms ([K - 1][T], or [R][K - 1][T] for a lock-step case), all from one generator seeded by the case"""
    rng = np.random.default_rng([N, D, K, R, KINDS.index(kind)])
    T = 2 + int(np.log(K))
    if kind == "blobs":
        cen = rng.standard_normal((K, D)) * 3
        X = (cen[rng.integers(0, K, N)] + 0.3 * rng.standard_normal((N, D))).astype(np.float32)
    else:
        X = rng.standard_normal((N, D)).astype(np.float32)
    u = rng.random((R, K - 1, T) if R else (K - 1, T))
    return X, T, u


def first_of(N, r=0):
    return (1234 + 97 * r) % N


class Device:
    """X on the device with its k-permuted copy and row norms, and the two entry points"""

    def __init__(self, X):
        import torch
        from video_similarity_search_amd.clustering.kmeans_hip import HipKernels
        self.torch, self.k = torch, HipKernels()
        self.X = torch.from_numpy(X).cuda()
        self.Xp, self.xn = torch.empty_like(self.X), torch.empty(len(X), device="cuda")
        self.k.permute_k8(self.X, self.Xp)
        self.k.cnorm(self.X, self.xn)

    def single(self, first, K, T, u, mfma):
        idx = self.torch.empty(K, dtype=self.torch.int32, device="cuda")
        ud = self.torch.from_numpy(np.ascontiguousarray(u)).cuda()
        self.k.kpp_run(self.X, first, K, T, ud, idx, *((self.Xp, self.xn) if mfma else ()))
        return idx.cpu().numpy()

    def batch(self, firsts, K, T, u):
        idx = self.torch.empty(len(firsts), K, dtype=self.torch.int32, device="cuda")
        ud = self.torch.from_numpy(np.ascontiguousarray(u)).cuda()
        self.k.kpp_run_batch(self.Xp, self.xn, firsts, K, T, ud, idx)
        return idx.cpu().numpy()


def generate():
    data = {}
    for kind in KINDS:
        for N, D, K in SINGLE:
            X, T, u = inputs(N, D, K, kind)
            dev, n = Device(X), name(N, D, K, kind)
            data[n + "__valu"] = dev.single(first_of(N), K, T, u, mfma=False)
            data[n + "__mfma"] = dev.single(first_of(N), K, T, u, mfma=True)
            data[n + "__sums"] = np.array([X.sum(dtype=np.float64), u.sum()])
            print("{:32s} T={} valu == mfma on {} of {} picks".format(n, T, int((data[n + "__valu"] == data[n + "__mfma"]).sum()), K))
        for N, D, K, R in BATCH:
            X, T, u = inputs(N, D, K, kind, R)
            n = name(N, D, K, kind, R)
            data[n + "__picks"] = Device(X).batch([first_of(N, r) for r in range(R)], K, T, u)
            data[n + "__sums"] = np.array([X.sum(dtype=np.float64), u.sum()])
            print("{:32s} T={} R*T={}".format(n, T, R * T))
    return data


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    data = generate()
    if "--check" in sys.argv[1:]:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(data), "the cases differ from the file's"
        bad = [k for k in data if not np.array_equal(old[k], data[k])]
        assert not bad, "differs from {}: {}".format(OUT, bad)
        print("reproduces", OUT, "exactly:", len(data), "arrays")
    else:
        np.savez_compressed(OUT, **data)
        print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

"""Generates tests/golden/cluster_metrics.npz: sklearn 1.7.2's normalized_mutual_info_score and adjusted_mutual_info_score
(average_method='arithmetic') and their parts on small seeded label pairs.

    python tests/golden/make_goldens_cluster_metrics.py

Every case stores labels_true, labels_pred (int32) and rec = [MI, H_true, H_pred, EMI, NMI, AMI] as sklearn computes them
(mutual_info_score, entropy, expected_mutual_information, and the two scores).  sklearn is needed here only, not by the tests."""
import os

import numpy as np
import sklearn
from sklearn.metrics import adjusted_mutual_info_score, mutual_info_score, normalized_mutual_info_score
from sklearn.metrics.cluster import contingency_matrix, entropy, expected_mutual_information

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cluster_metrics.npz")


def noisy(rng, truth, k, frac):
    """a copy of `truth` with a fraction of the labels redrawn from 0 .. k - 1"""
    out = truth.copy()
    hit = rng.random(len(truth)) < frac
    out[hit] = rng.integers(0, k, int(hit.sum()))
    return out


def cases():
    rng = np.random.default_rng(20261017)
    out = {}
    out["independent_small"] = (rng.integers(0, 7, 500), rng.integers(0, 11, 500))
    out["independent_large"] = (rng.integers(0, 40, 6000), rng.integers(0, 100, 6000))
    truth = rng.integers(0, 20, 4000)
    for tag, frac in (("05", 0.05), ("30", 0.3), ("80", 0.8)):
        out["noisy_" + tag] = (truth, noisy(rng, truth, 20, frac))
    out["identical"] = (truth[:1500], truth[:1500].copy())
    perm = rng.permutation(20)
    out["permuted_values"] = (truth[:1500], perm[truth[:1500]])
    out["one_cluster"] = (rng.integers(0, 9, 300), np.zeros(300, np.int64))
    out["one_class"] = (np.full(300, 3), rng.integers(0, 9, 300))
    out["one_and_one"] = (np.full(50, 7), np.full(50, -1))
    out["n1"] = (np.array([5]), np.array([-2]))
    out["n2_same"] = (np.array([0, 1]), np.array([1, 0]))
    out["n2_split"] = (np.array([0, 0]), np.array([0, 1]))
    lt = rng.integers(0, 6, 800)
    lp = noisy(rng, lt, 6, 0.2)
    lp[rng.random(800) < 0.25] = -1                                       # DBSCAN noise: a cluster like any other
    out["with_noise_label"] = (lt, lp)
    vals = np.array([-2147483648, -70000, -1, 0, 3, 1000, 65536, 2147483647])
    out["sparse_values"] = (vals[rng.integers(0, 8, 1000)], vals[::-1][noisy(rng, rng.integers(0, 8, 1000), 8, 0.5)])
    n = 4000
    lt = rng.integers(0, 30, n)
    out["finch_like"] = (lt, lt * 40 + rng.integers(0, 34, n))            # about N / 4 clusters, each inside one class
    out["many_against_many"] = (rng.integers(0, 300, 3000), rng.integers(0, 500, 3000))
    out["negative_ami"] = (np.arange(24) % 4, np.arange(24) // 4 % 3)       # a perfectly even 4 x 3 table: MI = 0 < EMI
    return {k: (np.asarray(a, np.int64), np.asarray(b, np.int64)) for k, (a, b) in out.items()}


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    data = {}
    neg = False
    for name, (lt, lp) in cases().items():
        c = contingency_matrix(lt, lp, sparse=True)
        rec = np.array([mutual_info_score(lt, lp), entropy(lt), entropy(lp), expected_mutual_information(c, len(lt)),
                        normalized_mutual_info_score(lt, lp), adjusted_mutual_info_score(lt, lp)], dtype=np.float64)
        data[name + "__labels_true"] = lt.astype(np.int32)
        data[name + "__labels_pred"] = lp.astype(np.int32)
        data[name + "__rec"] = rec
        neg |= rec[5] < -1e-3
        print("{:20s} N={:5d} classes={:4d} clusters={:4d}  MI={:.6f} EMI={:.6f} NMI={:.6f} AMI={:+.6f}".format(
            name, len(lt), len(np.unique(lt)), len(np.unique(lp)), rec[0], rec[3], rec[4], rec[5]))
    assert neg, "no case with a negative AMI"
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

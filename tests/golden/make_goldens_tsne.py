"""Writes tests/golden/tsne.npz: sklearn 1.7.2's results on the inputs of tests/tsne_ref.py, and what the float32 restatement
(tests/tsne_cpu_kernels.py) shows against the float64 one — the figures the device tests' bounds are multiples of.  Small arrays
and scalars only.  Run from the repository root:  python tests/golden/make_goldens_tsne.py"""
import os
import sys

import numpy as np
import sklearn
from sklearn.decomposition import PCA
from sklearn.manifold import TSNE, trustworthiness
from sklearn.manifold import _t_sne, _utils

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tsne_ref as R                                            # noqa: E402
from tsne_cpu_kernels import NumpyTsneKernels                   # noqa: E402


def main():
    out = {"sklearn_version": np.array(sklearn.__version__)}
    K = NumpyTsneKernels()

    # conditional P: sklearn's own search and the float32 restatement against the converged float64 search, on the same distances
    for case in R.COND_CASES:
        N, D, perp = case
        d2 = R.sqdist64(R.cond_input(case)).astype(np.float32)
        oracle = R.cond_p64(d2, perp)
        sk = np.asarray(_utils._binary_search_perplexity(d2, float(perp), 0))
        P32 = d2.copy()
        K.cond_p(P32, perp)
        key = R.cond_key(case)
        out[key + "_sk_err"] = np.abs(sk[:-1] - oracle[:-1]).max()
        out[key + "_sk_H_err"] = np.abs(R.entropy(sk[:-1]) - np.log(perp)).max()
        out[key + "_sk_H_err_outlier"] = abs(R.entropy(sk[-1:])[0] - np.log(perp))
        out[key + "_oracle_H_err"] = np.abs(R.entropy(oracle) - np.log(perp)).max()
        out[key + "_r32_err"] = np.abs(P32[:-1] - oracle[:-1]).max()
        out[key + "_r32_eval_err"] = np.abs(R.entropy(P32) - K.last_H).max()
        print(key, {k[len(key) + 1:]: float(v) for k, v in out.items() if k.startswith(key)})

    # symmetrise: sklearn's _joint_probabilities on the (65, 3, 5) input without the outlier
    N, D, perp = R.COND_CASES[0]
    d2 = R.sqdist64(R.blobs(N, D, 100 + N + D, outlier=False)).astype(np.float32)
    out["joint_sk"] = np.asarray(_t_sne._joint_probabilities(d2, float(perp), 0), dtype=np.float64)
    out["joint_sk_err"] = np.abs(np.asarray(_utils._binary_search_perplexity(d2, float(perp), 0)) - R.cond_p64(d2, perp)).max()
    print("joint", out["joint_sk"].shape, float(out["joint_sk_err"]))

    # forces: the float32 restatement against float64, per component over the row's absolute-term sum, in ulp(fp32)
    for case in R.FORCE_CASES:
        N, scale, e = case
        P, Y = R.joint_input(case), R.embedding(N, scale, 7)
        g64, Z64, kl64, S = R.forces64(P, Y, e)
        g32, Z32, kl32 = K.forces(P, Y, e, True)
        out[R.force_key(case) + "_r32_ulp"] = (np.abs(g32 - g64) / S).max() / R.ULP32
        print(R.force_key(case), float(out[R.force_key(case) + "_r32_ulp"]), abs(Z32 / Z64 - 1), abs(kl32 / kl64 - 1))

    # twenty steps from a stored init: the float32 restatement's drift from the float64 stepper
    P = R.joint_input((R.STEPS_N,))
    Y0 = (1e-4 * np.random.RandomState(11).standard_normal((R.STEPS_N, 2))).astype(np.float32)
    Y64 = R.descend64(P, Y0, R.STEPS, 12.0, 0.5, 50.0)
    st = K.start(Y0, P)
    for _ in range(R.STEPS):
        K.step(P, st, 12.0, 0.5, 50.0, False)
    out["steps_Y0"] = Y0
    out["steps_r32_drift"] = np.abs(st["Y"] - Y64).max() / np.abs(Y64).max()
    print("steps drift", float(out["steps_r32_drift"]))

    # end to end: sklearn's exact method from eight stored random inits
    e = R.E2E
    X = R.blobs(e["N"], e["D"], 500, special=False)
    inits = np.stack([(1e-4 * np.random.RandomState(s).standard_normal((e["N"], 2))).astype(np.float32) for s in range(e["n_init"])])
    kl, tw, nit = [], [], []
    for Y0 in inits:
        m = TSNE(n_components=2, perplexity=e["perplexity"], method="exact", init=Y0.copy()).fit(X)
        kl.append(m.kl_divergence_)
        tw.append(trustworthiness(X, m.embedding_, n_neighbors=10))
        nit.append(m.n_iter_)
        own = R.trustworthiness(X, m.embedding_, 10)            # sklearn ranks fp32 expansion-form distances: near-ties may swap
        assert abs(tw[-1] - own) < 2e-5, (tw[-1], own)
        print("e2e", kl[-1], tw[-1], nit[-1], "own trustworthiness differs by", tw[-1] - own)
    out.update(e2e_X=X, e2e_inits=inits, e2e_sk_kl=np.array(kl), e2e_sk_trust=np.array(tw), e2e_sk_n_iter=np.array(nit))

    # PCA: sklearn on the float64 copy, and how far its own float32 run is from that
    for N, D, n, ratio in R.PCA_CASES:
        X = R.decaying(N, D, ratio, 900 + N)
        p64 = PCA(n_components=n, svd_solver="full").fit(X.astype(np.float64))
        p32 = PCA(n_components=n, svd_solver="full").fit(X)
        r64, r32 = p64.transform(X.astype(np.float64)), p32.transform(X)
        key = "pca_{}_{}_{}".format(N, D, n)
        out[key + "_var"] = p64.explained_variance_
        out[key + "_ratio"] = p64.explained_variance_ratio_
        out[key + "_rows"] = r64.astype(np.float32)
        out[key + "_sign"] = np.sign(p64.components_[np.arange(n), np.argmax(np.abs(p64.components_), axis=1)])
        out[key + "_var_diff"] = np.abs(p32.explained_variance_ - p64.explained_variance_).max()
        out[key + "_rows_diff"] = np.abs(r32 - r64).max()
        V, mean, var, rows = R.pca64(X, n)
        print(key, float(out[key + "_var_diff"]), float(out[key + "_rows_diff"]), "restatement vs sklearn:",
              np.abs(var - p64.explained_variance_).max(), np.abs(rows - r64).max())

    path = os.path.join(HERE, "tsne.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

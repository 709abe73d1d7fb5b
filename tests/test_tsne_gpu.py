"""GPU: the t-SNE and PCA kernels (csrc/tsne.hip) one entry point at a time against the float64 restatement (tsne_ref.py), with
bounds that are either derived here or multiples of what sklearn itself / the float32 restatement (tsne_cpu_kernels.py) show on
the same case (tests/golden/tsne.npz, written by tests/golden/make_goldens_tsne.py); then twenty steps, the whole fit against
sklearn's spread over eight inits, PCA, and the limits.  Every case prints its figures before it asserts."""
import os

import numpy as np
import pytest
import torch

import tsne_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
Z = np.load(os.path.join(GOLDEN, "tsne.npz"))
_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def K(gpu):
    from video_similarity_search_amd.manifold import HipTsneKernels
    return HipTsneKernels()


def one_step(K, P, Y, upd, gains, e, momentum, lr, want_kl=True):
    """one slic_tsne_step on copies -> host (Y, update, gains, grad, record)"""
    st = K.start(Y, P)
    st["update"], st["gains"] = dev(np.asarray(upd, dtype=np.float32)), dev(np.asarray(gains, dtype=np.float32))
    grad = torch.full_like(st["Y"], float("nan"))
    K.step(P, st, e, momentum, lr, want_kl, grad_out=grad)
    return st["Y"].cpu().numpy(), st["update"].cpu().numpy(), st["gains"].cpu().numpy(), grad.cpu().numpy(), K.record(st)


# ---------------------------------------------------------------- 1. squared distances
@pytest.mark.parametrize("N,D,strided", [(2, 1, False), (65, 3, False), (257, 50, True), (257, 130, False)])
def test_sqdist(K, N, D, strided):
    """every fp32 term (x_i - x_j)^2 carries the subtraction's rounding twice (2^-23 relative) and the D terms are added in a fixed
    order (D - 1 additions of 2^-24 each, the multiply fused), so the relative error of a sum of non-negative terms is below
    (D + 2) 2^-23: one rounding step of 2^-23 for each of D + 2 roundings, generously"""
    X = R.blobs(max(N, 6), D, 40 + N + D, outlier=False)[:N]
    if N > 1:
        X[1] = X[0]
    if strided:
        buf = torch.zeros(N, D + 7, dtype=torch.float32, device="cuda")
        buf[:, :D] = dev(X)
        x = buf[:, :D]
        assert x.stride(0) == D + 7
    else:
        x = dev(X)
    d2 = K.sqdist(K.rows(x)).cpu().numpy()
    ref = R.sqdist64(X)
    err = (np.abs(d2 - ref) / np.maximum(ref, np.finfo(np.float64).tiny)).max()
    print("sqdist", N, D, "max relative error", err, "bound", (D + 2) * 2.0 ** -23)
    assert err <= (D + 2) * 2.0 ** -23
    assert (np.diag(d2) == 0).all() and d2[0, 1] == 0 and d2[1, 0] == 0
    assert np.array_equal(d2, d2.T)


# ---------------------------------------------------------------- 2. conditional P
def cond_case(case):
    def make():
        d2 = R.sqdist64(R.cond_input(case)).astype(np.float32)
        return d2, R.cond_p64(d2, case[2])
    return cached(("cond", case), make)


@pytest.mark.parametrize("case", R.COND_CASES, ids=R.cond_key)
def test_cond_p(K, case):
    N, D, perp = case
    d2, oracle = cond_case(case)
    P = dev(d2)
    beta = K.cond_p(P, perp).cpu().numpy()
    P = P.cpu().numpy()
    key = R.cond_key(case)
    assert np.isfinite(P).all() and (np.diag(P) == 0).all() and (beta > 0).all()
    # entropy: the search stops within 1e-5 of log(perplexity) as IT evaluates the entropy (fp32 exp, float64 sums); the float64
    # entropy of the fp32 row it returns differs from that by the evaluation error the float32 restatement shows on this case
    H_err = np.abs(R.entropy(P) - np.log(perp))
    H_bound = 1e-5 + float(Z[key + "_r32_eval_err"])
    print(key, "entropy off by", H_err[:-1].max(), "outlier row", H_err[-1], "bound", H_bound, "(evaluation error",
          float(Z[key + "_r32_eval_err"]), "; sklearn off by", float(Z[key + "_sk_H_err"]), ", on the outlier", float(Z[key + "_sk_H_err_outlier"]), ")")
    assert (H_err <= H_bound).all()                                 # the outlier row included: the shifted search converges on it
    # against the converged float64 search: 4 x what sklearn's own search shows against it (two correct searches may stop on
    # opposite sides of the target)
    err, bound = np.abs(P - oracle), 4.0 * float(Z[key + "_sk_err"])
    print(key, "max |P - oracle|", err[:-1].max(), "outlier row", err[-1].max(), "bound", bound, "(float32 restatement:", float(Z[key + "_r32_err"]), ")")
    assert err[:-1].max() <= bound
    assert err[-1].max() <= bound                                   # the outlier row: against the float64 oracle only
    sums = P.astype(np.float64).sum(axis=1)
    print(key, "row sums off by", np.abs(sums - 1).max())
    assert np.abs(sums - 1).max() <= 4 * R.ULP32


# ---------------------------------------------------------------- 3. symmetrise
def test_symmetrize(K):
    N, D, perp = R.COND_CASES[0]
    d2 = R.sqdist64(R.blobs(N, D, 100 + N + D, outlier=False)).astype(np.float32)
    P = dev(d2)
    K.cond_p(P, perp)
    Pc = P.cpu().numpy().astype(np.float64)
    J = K.symmetrize(P).cpu().numpy()
    assert np.array_equal(J, J.T) and (np.diag(J) == 0).all()
    # sum: N^2 entries each rounded once to fp32 from the float64 quotient: |sum - 1| <= 2^-24 sum J + the float64 fold's own error
    total = J.astype(np.float64).sum()
    print("symmetrize: sum", total, "off by", abs(total - 1))
    assert abs(total - 1) <= 2.0 ** -24 + N * N * R.EPS
    ref = R.joint(Pc)
    assert np.abs(J - ref).max() <= 2.0 ** -24 * ref.max() + R.EPS
    # sklearn's _joint_probabilities on the same distances: each conditional entry is within E_device + E_sklearn of the oracle,
    # E_device <= 4 E_sklearn (test 2), and a joint entry is (p_ij + p_ji) / 2N
    iu = np.triu_indices(N, 1)
    d = np.abs(J[iu] - Z["joint_sk"]).max()
    bound = 5.0 * float(Z["joint_sk_err"]) / N + 2.0 ** -24 * ref.max()
    print("symmetrize: max |J - sklearn|", d, "bound", bound)
    assert d <= bound


# ---------------------------------------------------------------- 4. forces and gradient
@pytest.mark.parametrize("case", R.FORCE_CASES, ids=R.force_key)
def test_forces(K, case):
    N, scale, e = case
    Ph = cached(("joint", N), lambda: R.joint_input(case))
    Y = R.embedding(N, scale, 7)
    g64, Z64, kl64, S = cached(("f64", case), lambda: R.forces64(Ph, Y, e))
    _, _, _, grad, rec = one_step(K, dev(Ph), Y, np.zeros_like(Y), np.ones_like(Y), e, 0.0, 0.0)
    assert np.isfinite(grad).all() and np.isfinite(rec).all()
    ulp = (np.abs(grad - g64) / S).max() / R.ULP32                  # S [N, 2]: per component, as the error is
    bound = 4.0 * float(Z[R.force_key(case) + "_r32_ulp"])
    print(R.force_key(case), "gradient error / row's absolute-term sum:", ulp, "ulp; bound", bound, "ulp; Z off by", abs(rec[0] / Z64 - 1),
          "KL off by", abs(rec[1] / kl64 - 1))
    assert ulp <= bound
    assert abs(rec[0] / Z64 - 1) <= 1e-6 and abs(rec[1] / kl64 - 1) <= 1e-6
    assert abs(rec[3] - Ph.astype(np.float64).sum()) <= 1e-6


# ---------------------------------------------------------------- 5. update
@pytest.mark.parametrize("momentum", [0.5, 0.8])
def test_update_rule(K, momentum):
    """gain up (update and gradient disagree in sign), gain down, gain held at the floor, a zero update (no sign: gain down), under
    both momenta; the float32 restatement fed the device's own gradient must agree within 2 ulp"""
    N = 257
    Ph = cached(("joint", N), lambda: R.joint_input((N,)))
    Y = R.embedding(N, 1.0, 7)
    g64 = R.forces64(Ph, Y, 1.0)[0]
    rs = np.random.RandomState(3)
    sgn = np.where(rs.rand(N, 2) < 0.5, -1.0, 1.0)
    upd = (sgn * np.sign(g64) * np.abs(g64) * rs.rand(N, 2) * 100).astype(np.float32)
    upd[rs.rand(N, 2) < 0.1] = 0
    gains = rs.choice(np.array([0.01, 0.0124, 0.5, 1.0, 3.7], dtype=np.float32), size=(N, 2))
    Y1, u1, g1, grad, rec = one_step(K, dev(Ph), Y, upd, gains, 1.0, momentum, 50.0, want_kl=False)
    rY, ru, rg, gg = R.update_rule(Y, upd, gains, grad, momentum, 50.0, np.float32)
    inc = upd * grad < 0
    assert inc.any() and (~inc).any() and (rg[~inc] == np.float32(0.01)).any() and (rg[inc] > gains[inc]).all() and (upd == 0).any()
    for name, a, b in (("gains", g1, rg), ("update", u1, ru), ("Y", Y1, rY)):
        d = np.abs(a.astype(np.float64) - b) / np.spacing(np.abs(b))
        print("update rule, momentum", momentum, name, "max ulp", d.max())
        assert d.max() <= 2
    assert abs(rec[2] / np.sqrt((gg.astype(np.float64) ** 2).sum()) - 1) <= 1e-6 and np.isnan(rec[1])


# ---------------------------------------------------------------- 6. twenty steps
def test_twenty_steps(K):
    N = R.STEPS_N
    Ph = cached(("joint", N), lambda: R.joint_input((N,)))
    Y0 = Z["steps_Y0"]
    Y64 = R.descend64(Ph, Y0, R.STEPS, 12.0, 0.5, 50.0)
    runs = []
    P = dev(Ph)
    for _ in range(2):
        st = K.start(Y0, P)
        for _ in range(R.STEPS):
            K.step(P, st, 12.0, 0.5, 50.0, False)
        runs.append(K.embedding(st))
    drift, bound = np.abs(runs[0] - Y64).max() / np.abs(Y64).max(), 4.0 * float(Z["steps_r32_drift"])
    print("twenty steps: drift", drift, "bound", bound)
    assert drift <= bound
    assert np.array_equal(runs[0], runs[1])


# ---------------------------------------------------------------- 7. end to end
@pytest.mark.parametrize("i", range(R.E2E["n_init"]))
def test_end_to_end(gpu, i):
    from video_similarity_search_amd import TSNE
    kl, tw = Z["e2e_sk_kl"], Z["e2e_sk_trust"]
    X = np.array(Z["e2e_X"])
    m = TSNE(perplexity=R.E2E["perplexity"], init=Z["e2e_inits"][i]).fit(X)
    t = R.trustworthiness(X, m.embedding_, 10)
    print("init", i, "KL", m.kl_divergence_, "(sklearn", kl[i], "; rule <=", kl.max() + np.ptp(kl), ") trustworthiness", t, "(sklearn", tw[i],
          "; rule >=", tw.min() - np.ptp(tw), ") n_iter_", m.n_iter_)
    assert m.embedding_.shape == (X.shape[0], 2) and m.embedding_.dtype == np.float32 and np.isfinite(m.embedding_).all()
    assert m.kl_divergence_ <= kl.max() + np.ptp(kl)
    assert t >= tw.min() - np.ptp(tw)
    assert m.n_iter_ == int(Z["e2e_sk_n_iter"][i]) == 999           # all 1000 iterations run; sklearn reports the index of the last
    assert m.learning_rate_ == 50.0


# ---------------------------------------------------------------- 8. PCA
@pytest.mark.parametrize("N,D,n,ratio", R.PCA_CASES)
def test_pca(gpu, N, D, n, ratio):
    from video_similarity_search_amd import PCA
    X = R.decaying(N, D, ratio, 900 + N)
    key = "pca_{}_{}_{}".format(N, D, n)
    p = PCA(n_components=n)
    rows = p.fit_transform(X)
    dv, dr = np.abs(p.explained_variance_ - Z[key + "_var"]).max(), np.abs(rows - Z[key + "_rows"]).max()
    print(key, "explained_variance_ off by", dv, "bound", 4 * float(Z[key + "_var_diff"]), "; rows off by", dr, "bound", 4 * float(Z[key + "_rows_diff"]))
    assert dv <= 4 * float(Z[key + "_var_diff"])
    assert dr <= 4 * float(Z[key + "_rows_diff"])                  # signs equal, not merely equal up to sign
    big = np.argmax(np.abs(p.components_), axis=1)
    assert np.array_equal(np.sign(p.components_[np.arange(n), big]), Z[key + "_sign"]) and (Z[key + "_sign"] == 1).all()
    assert np.abs(p.explained_variance_ratio_ - Z[key + "_ratio"]).max() <= 4 * float(Z[key + "_var_diff"]) / Z[key + "_var"].sum()
    assert np.abs(p.transform(dev(X)) - rows).max() == 0 and p.components_.shape == (n, D) and p.mean_.shape == (D,)


# ---------------------------------------------------------------- 9. limits, projection
def test_limits(K):
    from video_similarity_search_amd import TSNE, _lib
    X = R.blobs(20, 4, 1, special=False)
    with pytest.raises(ValueError):
        TSNE(perplexity=30).fit(X)
    with pytest.raises(NotImplementedError):
        TSNE(method="barnes_hut", perplexity=5).fit(X)
    with pytest.raises(_lib.SlicError):
        K._workspace(65537, torch.device("cuda"))
    with pytest.raises(_lib.SlicError):
        K._workspace(1, torch.device("cuda"))


def test_tsne_projection(gpu):
    from video_similarity_search_amd import tsne_projection
    rs = np.random.RandomState(5)
    labels = rs.randint(0, 12, 400)
    emb = (4.0 * rs.standard_normal((12, 60))[labels] + rs.standard_normal((400, 60))).astype(np.float32)
    coords, mask = tsne_projection(dev(emb), labels, num_classes=12, n_class_subset=5, seed=42, perplexity=20, n_pca=50)
    np.random.seed(42)
    subset = np.random.permutation(12)[:5]
    assert np.array_equal(mask, np.isin(labels, subset)) and coords.shape == (int(mask.sum()), 2) and np.isfinite(coords).all()
    t = R.trustworthiness(emb[mask], coords, 10)
    print("tsne_projection: trustworthiness", t)
    assert t >= 0.9

"""CPU: the silhouette's float64 reference and fp32 mirror (tests/silhouette_cpu_kernels.py) against the sklearn 1.7.2 goldens
(tests/golden/silhouette.npz), the derived gate and the defects it must catch, the host driver (clustering/metrics.py) through the
NumPy provider, and the cluster step's opt-in lines; the device path is test_silhouette_gpu.py.

GATE (derived, not tuned; u = 2^-24): float64 statistics rounded once to fp32 and a length-D fp32 fmaf chain bound the error of a
mean distance to a cluster by delta = (D + 8) u (cosine) resp. (D + 8) u (|x_i| + R)^2, R^2 = max_C Q_C / |C| (sqeuclidean); the own
term carries |C| / (|C| - 1) <= 2, so |ds| <= 3 delta / max(a, b) to first order; rows are gated at 4 delta / max(a64, b64), rows with
max(a64, b64) < 0.05 are left out (at most 1 % of them, asserted), the mean is gated at the mean of the row gates."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from silhouette_cases import GOLDEN_CASES, METRICS, checksum, draw, run_step, run_step_recorded, step_inputs
from silhouette_cpu_kernels import (DEFECTS, NumpySilhouetteKernels, check_mean, check_rows, deltas, gates, silhouette_fp64,
                                    silhouette_mirror)

Z = np.load(os.path.join(GOLDEN, "silhouette.npz"))
CASES = [(n, m) for n in GOLDEN_CASES for m in METRICS]
_cache = {}


def case(name, metric):
    """(x, labels, float64 reference), computed once"""
    if name not in _cache:
        _cache[name] = draw(*GOLDEN_CASES[name])
    x, labels = _cache[name]
    if (name, metric) not in _cache:
        _cache[name, metric] = silhouette_fp64(x, labels, metric)
    return x, labels, _cache[name, metric]


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_inputs_are_the_recorded_ones(name):
    x, labels = draw(*GOLDEN_CASES[name])
    assert checksum(x, labels) == bytes(Z[name + "__checksum"]).decode()
    sizes = np.bincount(np.unique(labels, return_inverse=True)[1])
    assert labels.min() == -1 and (sizes == 1).sum() >= 3 and len(sizes) == GOLDEN_CASES[name][3]


@pytest.mark.parametrize("name,metric", CASES)
def test_fp64_function_equals_sklearn(name, metric):
    x, labels, ref = case(name, metric)
    d = np.abs(ref["s"] - Z["{}__{}__samples".format(name, metric)]).max()
    print(name, metric, "max |fp64 - sklearn| =", d)
    assert d <= 1e-12
    assert abs(ref["score"] - float(Z["{}__{}__score".format(name, metric)])) <= 1e-12


@pytest.mark.parametrize("name,metric", CASES)
def test_mirror_meets_the_derived_gate(name, metric):
    x, labels, ref = case(name, metric)
    m = silhouette_mirror(x, labels, metric)
    check_rows(m["s"], x, ref, metric, "{} {}".format(name, metric))
    check_mean(m["score"], x, ref, metric, "{} {}".format(name, metric))
    assert np.array_equal(m["nearest"], ref["nearest"])
    gate, gated = gates(x, ref, metric)
    assert np.abs(m["cluster_mean"] - ref["cluster_mean"]).max() <= gate[gated].max() and np.array_equal(m["cluster_label"], ref["cluster_label"])


def zero_row_case():
    """a zero row under cosine: the one place where the self term 1 - x^.x^ is 1 and not ~0"""
    x, labels = draw(211, 120, 16, 6, 0.3, singletons=0)
    x[7] = 0.0
    return x, labels


def tie_case():
    """clusters 10 and 20 hold the same rows: every row of cluster 0 is equally far from both, and the first must win"""
    rng = np.random.default_rng(5)
    a = rng.standard_normal((9, 8)).astype(np.float32)
    b = (rng.standard_normal((6, 8)) + 4).astype(np.float32)
    return np.concatenate([a, b, b]), np.array([0] * 9 + [10] * 6 + [20] * 6, np.int32)


@pytest.mark.parametrize("defect", DEFECTS)
def test_gate_catches_each_defect(defect):
    """the self term shows only where it is not ~0 (a zero row under cosine), the tie rule only in the nearest label of a tie; the
    other three move s by more than 1e-2 on every golden case"""
    if defect == "ties_last":
        x, labels = tie_case()
        for metric in METRICS:
            ref = silhouette_fp64(x, labels, metric)
            assert (ref["nearest"][:9] == 10).all()
            assert np.array_equal(silhouette_mirror(x, labels, metric)["nearest"], ref["nearest"])
            assert (silhouette_mirror(x, labels, metric, defect=defect)["nearest"][:9] == 20).all()
        return
    if defect == "self_kept":
        x, labels = zero_row_case()
        todo = [(x, labels, silhouette_fp64(x, labels, "cosine"), "cosine")]
    else:
        todo = [case(n, m) + (m,) for n, m in CASES]
    for x, labels, ref, metric in todo:
        check_rows(silhouette_mirror(x, labels, metric)["s"], x, ref, metric, "sound")
        with pytest.raises(AssertionError):
            check_rows(silhouette_mirror(x, labels, metric, defect=defect)["s"], x, ref, metric, defect)


# ---- the host driver through the NumPy provider ----

def test_input_forms_agree():
    from video_similarity_search_amd.clustering import silhouette_report, silhouette_samples, silhouette_score
    x, labels, ref = case("n300_d16_k7", "cosine")
    k = NumpySilhouetteKernels()
    s0 = silhouette_samples(x, labels, kernels=k)
    wide = torch.from_numpy(np.concatenate([x, x], 1))
    for a, b in ((x.astype(np.float64), labels.tolist()), (torch.from_numpy(x), torch.from_numpy(labels).long()),
                 (wide[:, :16], labels.astype(np.int64)), (x.tolist(), labels)):
        assert np.array_equal(silhouette_samples(a, b, kernels=k), s0)
    s, a, b, near = silhouette_samples(x, labels, return_parts=True, kernels=k)
    assert np.array_equal(s, s0) and np.array_equal(near, ref["nearest"]) and s.dtype == np.float32
    d = deltas(x, ref, "cosine")
    assert (np.abs(a - ref["a"]) <= 2 * d).all() and (np.abs(b - ref["b"]) <= d).all()
    rep = silhouette_report(x, labels, kernels=k)
    assert rep["score"] == silhouette_score(x, labels, kernels=k) and type(rep["score"]) is float
    assert rep["n_clusters"] == 7 and rep["n_rows"] == 300 and sorted(rep["per_cluster"]) == sorted(set(labels.tolist()))
    for lab, m in rep["per_cluster"].items():
        assert abs(m - ref["s"][labels == lab].mean()) <= gates(x, ref, "cosine")[0].max()


@pytest.mark.parametrize("name,metric", CASES)
def test_sample_size_follows_sklearn(name, metric):
    from video_similarity_search_amd.clustering import silhouette_score
    x, labels, _ = case(name, metric)
    got = silhouette_score(x, labels, metric=metric, sample_size=200, random_state=3, kernels=NumpySilhouetteKernels())
    idx = np.random.RandomState(3).permutation(len(x))[:200]
    ref = silhouette_fp64(x[idx], labels[idx], metric)
    assert abs(ref["score"] - float(Z["{}__{}__score200".format(name, metric)])) <= 1e-12       # the same subset as sklearn's
    check_mean(got, x[idx], ref, metric, "{} {} sample_size=200".format(name, metric))
    rs = np.random.RandomState(3)
    assert silhouette_score(x, labels, metric=metric, sample_size=200, random_state=rs, kernels=NumpySilhouetteKernels()) == got


def test_ignore_label_equals_removal():
    from video_similarity_search_amd.clustering import silhouette_report, silhouette_samples
    x, labels, _ = case("n517_d24_k30", "cosine")
    k = NumpySilhouetteKernels()
    keep = labels != -1
    assert 0 < (~keep).sum() < len(x)
    for metric in METRICS:
        s, a, b, near = silhouette_samples(x, labels, metric=metric, ignore_label=-1, return_parts=True, kernels=k)
        s1, a1, b1, near1 = silhouette_samples(x[keep], labels[keep], metric=metric, return_parts=True, kernels=k)
        assert np.isnan(s[~keep]).all() and np.isnan(a[~keep]).all() and np.isnan(b[~keep]).all() and (near[~keep] == -1).all()
        assert np.array_equal(s[keep], s1) and np.array_equal(a[keep], a1) and np.array_equal(b[keep], b1) and np.array_equal(near[keep], near1)
        r, r1 = (silhouette_report(x, labels, metric=metric, ignore_label=-1, kernels=k), silhouette_report(x[keep], labels[keep], metric=metric, kernels=k))
        assert r == r1 and -1 not in r["per_cluster"] and r["n_rows"] == keep.sum() and r["n_clusters"] == 29
    assert np.array_equal(silhouette_samples(x, labels, ignore_label=12345, kernels=k), silhouette_samples(x, labels, kernels=k))


def test_errors():
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.clustering import silhouette_samples, silhouette_score
    x, labels, _ = case("n300_d16_k7", "cosine")
    k = NumpySilhouetteKernels()
    with pytest.raises(NotImplementedError, match="N x N"):
        silhouette_score(x, labels, metric="euclidean", kernels=k)
    with pytest.raises(NotImplementedError):
        silhouette_score(x, labels, metric="precomputed", kernels=k)
    with pytest.raises(ValueError):
        silhouette_score(x, labels, metric="manhattan", kernels=k)
    with pytest.raises(ValueError, match=r"Number of labels is 1\. Valid values are 2 to n_samples - 1 \(inclusive\)"):
        silhouette_score(x, np.zeros(300, np.int32), kernels=k)
    with pytest.raises(ValueError, match=r"Number of labels is 300\. Valid values are 2 to n_samples - 1 \(inclusive\)"):
        silhouette_samples(x, np.arange(300), kernels=k)
    with pytest.raises(ValueError, match="Number of labels is 1"):                  # two labels, one of them ignored
        silhouette_score(x, np.where(np.arange(300) < 150, -1, 4), ignore_label=-1, kernels=k)
    with pytest.raises(ValueError, match="Number of labels is 2"):
        silhouette_score(x[:2], [0, 1], kernels=k)
    with pytest.raises(ValueError):
        silhouette_score(x, labels[:-1], kernels=k)
    with pytest.raises(ValueError):
        silhouette_score(x[0], labels, kernels=k)
    with pytest.raises(ValueError):
        silhouette_score(x, labels.astype(np.float32), kernels=k)
    with pytest.raises(ValueError):
        silhouette_score(x, labels, random_state="seed", sample_size=10, kernels=k)
    with pytest.raises(_lib.SlicError, match="max_clusters"):
        silhouette_score(x, labels, kernels=NumpySilhouetteKernels(max_clusters=5))


def test_no_device_raises():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.clustering import silhouette_report, silhouette_samples, silhouette_score
    from video_similarity_search_amd.clustering.metrics import HipSilhouetteKernels
    x, labels, _ = case("n300_d16_k7", "cosine")
    for f in (silhouette_samples, silhouette_score, silhouette_report):
        with pytest.raises(_lib.SlicError):
            f(x, labels)
    with pytest.raises(_lib.SlicError):
        HipSilhouetteKernels()


def test_workspace_query_states_the_limits():
    """host only: the query answers 0 for what the call rejects, and holds no N x K array"""
    from video_similarity_search_amd import _lib
    q = _lib.load().slic_silhouette_workspace_bytes
    assert q(3, 1, 2) > 0 and q(1 << 24, 512, 1000) > 0
    assert q(2, 8, 2) == 0 and q(100, 0, 5) == 0 and q(100, 513, 5) == 0 and q(100, 8, 1) == 0 and q(100, 8, 100) == 0
    assert q((1 << 24) + 1, 8, 5) == 0
    n, d, k = 240000, 128, 25000
    assert q(n, d, k) < 4 * n * (d + 64) + 4 * (k + 1) * d + (1 << 20) < 4 * n * k


# ---- the cluster step ----

def _providers():
    from cluster_metrics_cpu_kernels import NumpyClusterMetricsKernels
    from dbscan_cpu_kernels import NumpyDbscanKernels
    return dict(kmeans_kernels=NumpyDbscanKernels(), metrics_kernels=NumpyClusterMetricsKernels())


def test_cluster_step_opt_in_lines(tmp_path, capsys):
    x, y = step_inputs()
    labels, nmi, files = run_step(os.path.join(str(tmp_path), "on"), x, y, silhouette=True, silhouette_kernels=NumpySilhouetteKernels(),
                                  **_providers())
    out = capsys.readouterr().out
    assert (labels == -1).sum() == 10
    ref = silhouette_fp64(x, labels, "cosine", ignore_label=-1)
    line = "Silhouette (cosine) of the cluster assignments: {:.3f}".format(ref["score"])
    assert line in out and out.index("AMI between") < out.index(line) < out.index("Saved cluster labels")
    assert files["tnet_checkpoints/silhouettes.txt"] == "epoch:3 {:.3f}\n".format(ref["score"])
    assert files["tnet_checkpoints/NMIs.txt"] == "epoch:3 {:.3f}\n".format(nmi)


def test_cluster_step_undefined_score_does_not_stop(tmp_path, capsys):
    x, y = step_inputs()
    x[:] = x[0]                                                 # one DBSCAN cluster: no silhouette
    labels, nmi, files = run_step(os.path.join(str(tmp_path), "one"), x, y, silhouette=True, silhouette_kernels=NumpySilhouetteKernels(),
                                  **_providers())
    out = capsys.readouterr().out
    assert len(set(labels.tolist())) == 1
    assert "Silhouette (cosine) of the cluster assignments: undefined (Number of labels is 1." in out
    assert "tnet_checkpoints/silhouettes.txt" not in files and "vid_clusters.txt" in files


def test_cluster_step_sharded_route_refuses_the_flag(tmp_path, monkeypatch):
    from video_similarity_search_amd import online_train
    monkeypatch.setattr(online_train, "_cluster_sharded", lambda cfg: True)
    x, y = step_inputs()

    class NoLoader:
        dataset = list(range(60))

        def __iter__(self):
            raise AssertionError("the flag must be refused before the embeddings are computed")

    import types
    ns = types.SimpleNamespace
    cfg = ns(NUM_GPUS=2, OUTPUT_PATH=str(tmp_path), ITERCLUSTER=ns(METHOD='kmeans', K=4, L2_NORMALIZE=True, SHARDED=True, SILHOUETTE=True))
    with pytest.raises(NotImplementedError, match="SILHOUETTE"):
        online_train.iterative_cluster_step(None, cfg, torch.nn.Identity(), NoLoader(), epoch=0, cuda=False, device="cpu")


@pytest.mark.parametrize("flag", [None, False])
def test_cluster_step_without_the_flag_is_the_parent_commits(tmp_path, flag):
    """stdout, log files, labels and NMI of the step with the flag absent / false equal the record made before the lines existed"""
    rec = run_step_recorded(os.path.join(str(tmp_path), "off"), silhouette=flag)
    want = json.load(open(os.path.join(GOLDEN, "silhouette_cluster_step_parent.json")))
    assert rec["stdout"] == want["stdout"]
    assert rec["files"] == want["files"]
    assert rec["labels"] == want["labels"] and rec["nmi"] == want["nmi"]

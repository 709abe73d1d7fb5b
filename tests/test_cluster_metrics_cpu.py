"""CPU: the cluster-metrics host driver (clustering/metrics.py), its input forms and errors, and the cluster step's device route,
run against the float64 NumPy provider (tests/cluster_metrics_cpu_kernels.py) and the sklearn 1.7.2 goldens
(tests/golden/cluster_metrics.npz); the device path is test_cluster_metrics_gpu.py.

GATE: the provider restates the kernel's arithmetic and summation order; its largest absolute distance from sklearn over the
goldens, over MI, both entropies, EMI, NMI and AMI, was measured at 1.7e-11 (EMI of finch_like; 3.8e-12 on NMI / AMI).  That is
sklearn's own lgamma noise: it adds log-gamma values of ~N log N that cancel to ~10, the kernel's form of the same sum has no
such terms (include/slic_hip.h, rule 4).  The gate is ten times that, and by the project's rule never looser than 1e-9."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from cluster_metrics_cpu_kernels import NumpyClusterMetricsKernels, cluster_metrics_fp64

GATE = 1.7e-10
assert GATE <= 1e-9
KEYS = ("MI", "H_true", "H_pred", "EMI", "NMI", "AMI")


def golden_cases():
    z = np.load(os.path.join(GOLDEN, "cluster_metrics.npz"))
    names = sorted({k.split("__")[0] for k in z.files})
    return [(n, z[n + "__labels_true"], z[n + "__labels_pred"], z[n + "__rec"]) for n in names]


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_driver_reproduces_goldens(case):
    from video_similarity_search_amd.clustering import cluster_scores
    name, lt, lp, rec = case
    s = cluster_scores(lt, lp, kernels=NumpyClusterMetricsKernels())
    got = np.array([s[k] for k in KEYS])
    print(name, "max |provider - sklearn| =", np.abs(got - rec).max())
    assert np.abs(got - rec).max() <= GATE, (name, got, rec)
    assert all(type(s[k]) is float for k in KEYS)
    assert s["n_classes"] == len(np.unique(lt)) and s["n_clusters"] == len(np.unique(lp))


def test_goldens_cover_the_rules():
    c = {n: (lt, lp, rec) for n, lt, lp, rec in golden_cases()}
    assert c["one_and_one"][2][4] == 1.0 and c["one_and_one"][2][5] == 1.0 and c["n1"][2][4] == 1.0
    assert c["one_cluster"][2][4] == 0.0 and c["one_class"][2][5] == 0.0
    assert c["negative_ami"][2][5] < -0.1 and c["negative_ami"][2][4] == 0.0
    assert (c["with_noise_label"][1] == -1).any() and c["sparse_values"][0].min() == -2 ** 31
    assert len(np.unique(c["finch_like"][1])) > len(c["finch_like"][1]) // 5
    assert abs(c["identical"][2][5] - 1.0) < 1e-12 and abs(c["permuted_values"][2][4] - 1.0) < 1e-12
    assert len(c["n2_same"][0]) == 2


def test_agrees_with_sklearn_on_random_data():
    skm = pytest.importorskip("sklearn.metrics")
    from video_similarity_search_amd.clustering import adjusted_mutual_info_score, normalized_mutual_info_score
    k = NumpyClusterMetricsKernels()
    for seed in range(12):
        rng = np.random.default_rng(1000 + seed)
        n = int(rng.integers(50, 3000))
        lt = rng.integers(-3, int(rng.integers(2, 60)), n)
        lp = np.where(rng.random(n) < rng.random(), lt * 7 - 5, rng.integers(0, int(rng.integers(2, 200)), n))
        nmi, ami = normalized_mutual_info_score(lt, lp, kernels=k), adjusted_mutual_info_score(lt, lp, kernels=k)
        d = max(abs(nmi - skm.normalized_mutual_info_score(lt, lp)), abs(ami - skm.adjusted_mutual_info_score(lt, lp)))
        print(seed, n, "max |provider - sklearn| =", d)
        assert d <= GATE, seed


def test_input_forms_agree():
    from video_similarity_search_amd.clustering import cluster_scores
    _, lt, lp, _ = [c for c in golden_cases() if c[0] == "with_noise_label"][0]
    k = NumpyClusterMetricsKernels()
    ref = cluster_scores(lt, lp, kernels=k)
    wide = torch.from_numpy(np.stack([lt, lt + 1], 1).astype(np.int64))
    for a, b in ((lt.tolist(), lp.tolist()), (lt.astype(np.int64), lp.astype(np.int16)), (torch.from_numpy(lt), torch.from_numpy(lp).long()),
                 (wide[:, 0], lp)):
        assert cluster_scores(a, b, kernels=k) == ref


def test_value_errors():
    from video_similarity_search_amd.clustering import cluster_scores, normalized_mutual_info_score
    k = NumpyClusterMetricsKernels()
    with pytest.raises(ValueError):
        cluster_scores([0, 1, 2], [0, 1], kernels=k)                       # unequal lengths, as sklearn
    with pytest.raises(ValueError):
        cluster_scores([0, 2 ** 31], [0, 1], kernels=k)                    # outside int32
    with pytest.raises(ValueError):
        cluster_scores(np.array([0, -2 ** 31 - 1]), [0, 1], kernels=k)
    with pytest.raises(ValueError):
        normalized_mutual_info_score(torch.tensor([0, 2 ** 40]), torch.tensor([0, 1]), kernels=k)
    with pytest.raises(ValueError):
        cluster_scores(np.zeros((2, 2), np.int32), np.zeros((2, 2), np.int32), kernels=k)
    with pytest.raises(ValueError):
        cluster_scores([0.5, 1.0], [0, 1], kernels=k)
    with pytest.raises(ValueError):
        cluster_scores([], [], kernels=k)


def test_no_device_raises():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.clustering import adjusted_mutual_info_score, cluster_scores
    from video_similarity_search_amd.clustering.metrics import HipClusterMetricsKernels
    with pytest.raises(_lib.SlicError):
        cluster_scores([0, 1, 1], [1, 0, 0])
    with pytest.raises(_lib.SlicError):
        adjusted_mutual_info_score(np.arange(4), np.arange(4))
    with pytest.raises(_lib.SlicError):
        HipClusterMetricsKernels()


def test_workspace_query_states_the_limits():
    """host only: the query answers 0 for what the call rejects, and admits 400 x 65536"""
    from video_similarity_search_amd import _lib
    lib = _lib.load()
    q = lib.slic_cluster_metrics_workspace_bytes
    assert q(240000, 400 * 65536) >= 4 * 400 * 65536 + 52 * 240000
    assert q(1, 1) > 0
    assert q(0, 1) == 0 and q(10, 0) == 0 and q(10, (1 << 26) + 1) == 0 and q((1 << 24) + 1, 100) == 0
    assert q(1 << 24, 1 << 26) > 0


def test_provider_reports_the_table_limit():
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.clustering import cluster_scores
    n = 8200                                          # 8200 x 8200 distinct pairs of values: more than 2^26 cells
    with pytest.raises(_lib.SlicError):
        cluster_scores(np.arange(n), np.arange(n)[::-1], kernels=NumpyClusterMetricsKernels())


class _Loader:
    """an eval loader over rows x with true labels y, batches of 4 (the pattern of tests/test_dbscan_cpu.py::_Loader)"""

    def __init__(self, x, y):
        self.x, self.y = x, y
        self.dataset = list(range(len(x)))

    def __iter__(self):
        for s in range(0, len(self.x), 4):
            b = list(range(s, min(s + 4, len(self.x))))
            yield torch.from_numpy(self.x[b]), torch.from_numpy(self.y[b]), 0, torch.tensor(b)

    def __len__(self):
        return (len(self.x) + 3) // 4


def _step(tmp_path, sub, **kw):
    from dbscan_cpu_kernels import NumpyDbscanKernels
    from video_similarity_search_amd.online_train import iterative_cluster_step
    rng = np.random.default_rng(11)
    cen = rng.standard_normal((4, 8)) * 3
    y = rng.integers(0, 4, 60)
    x = (cen[y] + 0.05 * rng.standard_normal((60, 8))).astype(np.float32)
    x[50:] = 5 * rng.standard_normal((10, 8))                     # rows DBSCAN leaves as noise: a -1 cluster
    y[:6] = (y[:6] + 1) % 4                                       # some wrong true labels: NMI < 1
    out = os.path.join(str(tmp_path), sub)
    os.makedirs(out)
    ns = types.SimpleNamespace
    cfg = ns(NUM_GPUS=1, OUTPUT_PATH=out, DATASET=ns(POSITIVE_SAMPLING_P=0.2),
             ITERCLUSTER=ns(METHOD='DBSCAN', K=4, L2_NORMALIZE=True, FINCH_PARTITION=0, ADAPTIVEP=True, SHARDED=True))
    labels, nmi = iterative_cluster_step(None, cfg, torch.nn.Identity(), _Loader(x, y.astype(np.int64)), epoch=3, cuda=False,
                                         device="cpu", kmeans_kernels=NumpyDbscanKernels(), **kw)
    logs = os.path.join(out, "tnet_checkpoints")
    read = lambda n: open(os.path.join(logs, n)).read() if os.path.exists(os.path.join(logs, n)) else None
    return labels, nmi, cfg.DATASET.POSITIVE_SAMPLING_P, read("NMIs.txt"), read("AMIs.txt"), y


def test_cluster_step_device_route_equals_sklearn_route(tmp_path):
    pytest.importorskip("sklearn.metrics")
    host = _step(tmp_path, "host")
    dev = _step(tmp_path, "dev", metrics_kernels=NumpyClusterMetricsKernels())
    assert np.array_equal(host[0], dev[0]) and (host[0] == -1).any()
    assert host[3] == dev[3] and host[4] == dev[4] and host[3].startswith("epoch:3 0.")
    assert abs(host[1] - dev[1]) <= GATE and 0.0 < dev[1] < 1.0
    assert abs(host[2] - dev[2]) <= GATE and dev[2] == float(1.0 - dev[1])
    ref = cluster_metrics_fp64(host[5], host[0])
    assert dev[1] == ref[4]


def test_cluster_step_device_route_does_not_need_sklearn(tmp_path, monkeypatch, capsys):
    monkeypatch.setitem(sys.modules, 'sklearn.metrics', None)
    with pytest.raises(ImportError):
        import sklearn.metrics  # noqa: F401
    labels, nmi, p, nmis, amis, y = _step(tmp_path, "dev", metrics_kernels=NumpyClusterMetricsKernels())
    ref = cluster_metrics_fp64(y, labels)
    assert nmi == ref[4] and p == float(1.0 - nmi)
    assert nmis == "epoch:3 {:.3f}\n".format(ref[4]) and amis == "epoch:3 {:.3f}\n".format(ref[5])
    out = capsys.readouterr().out
    assert "NMI between true labels and cluster assignments: {:.3f}".format(ref[4]) in out
    assert "AMI between true labels and cluster assignments: {:.3f}\n".format(ref[5]) in out
    host = _step(tmp_path, "host")                    # the host route without sklearn: silent, as before
    assert host[1] is None and host[3] is None and host[2] == 0.2

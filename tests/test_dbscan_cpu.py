"""CPU: the DBSCAN host driver, fit_cluster's 'DBSCAN' method and vid_clusters.txt noise rows, run against the float64 NumPy
provider (tests/dbscan_cpu_kernels.py) and the sklearn goldens (tests/golden/dbscan.npz); the device path is test_dbscan_gpu.py."""
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from dbscan_cpu_kernels import NumpyDbscanKernels, dbscan_fp64


def golden_cases():
    z = np.load(os.path.join(GOLDEN, "dbscan.npz"))
    names = sorted({k.split("__")[0] for k in z.files})
    return [(n, z[n + "__X"], float(z[n + "__eps"]), int(z[n + "__min_samples"]), z[n + "__labels"], z[n + "__core"]) for n in names]


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_driver_reproduces_goldens(case):
    from video_similarity_search_amd.clustering.dbscan import DBSCAN
    name, X, eps, ms, labels, core = case
    m = DBSCAN(eps=eps, min_samples=ms, metric='cosine', kernels=NumpyDbscanKernels()).fit(X)
    assert m.labels_.dtype == np.int32 and m.labels_.shape == (len(X),)
    assert np.array_equal(m.labels_, labels), name
    assert np.array_equal(m.core_sample_indices_, core), name
    assert m.n_clusters_ == len(set(labels.tolist()) - {-1})


def test_goldens_cover_the_rules():
    cases = {c[0]: c for c in golden_cases()}
    _, X, eps, ms, labels, core = cases["border_ms4"]
    # row 6 reaches a core of both clusters; it is not core and takes the smaller cluster number (rule 4)
    assert 6 not in core and labels[6] == 0
    assert not np.any(np.all(cases["all_core_ms1"][1] == 0, axis=1) & (cases["all_core_ms1"][4] < 0))    # zero rows are core at ms 1
    assert len(cases["single_ms1"][1]) == 1 and cases["single_ms1"][4][0] == 0 and cases["single_ms2"][4][0] == -1
    assert np.all(cases["noise_ms2"][4] == -1)


def test_agrees_with_sklearn_on_random_data():
    sk = pytest.importorskip("sklearn.cluster")
    checked = 0
    for seed in range(12):
        rng = np.random.default_rng(seed)
        D = int(rng.choice([8, 16, 33]))
        cen = rng.standard_normal((5, D))
        X = (cen[rng.integers(0, 5, 300)] + 0.15 * rng.standard_normal((300, D))).astype(np.float32)
        eps, ms = float(rng.choice([0.02, 0.05, 0.1])), int(rng.choice([2, 3, 5]))
        d = np.concatenate([dd for _, dd in __import__("dbscan_cpu_kernels").distance_chunks(X)])
        off = ~np.eye(len(X), dtype=bool)
        if np.any(np.abs(d[off] - eps) < 1e-5):
            continue                                        # a pair in the float32 / float64 band: the two may disagree there
        ref = sk.DBSCAN(eps=eps, min_samples=ms, metric='cosine').fit(X)
        labels, core, counts, ncl = dbscan_fp64(X, eps, ms)
        assert np.array_equal(labels, ref.labels_), seed
        assert np.array_equal(np.flatnonzero(core), ref.core_sample_indices_), seed
        checked += 1
    assert checked >= 6


def test_fit_cluster_dbscan_prints_and_returns(capsys):
    from video_similarity_search_amd.clustering import fit_cluster
    name, X, eps, ms, labels, core = [c for c in golden_cases() if c[0] == "blobs16_ms2"][0]
    out = fit_cluster(torch.from_numpy(X), 'DBSCAN', kernels=NumpyDbscanKernels())
    assert isinstance(out, np.ndarray) and out.dtype == np.int32 and np.array_equal(out, labels)   # the golden is eps 0.14, ms 2
    n = len(set(labels.tolist()) - {-1})
    assert capsys.readouterr().out.splitlines() == ["Clustering with DBSCAN...", str((len(X),)),
                                                    "Fitted {} clusters with DBSCAN".format(n)]
    out = fit_cluster(X, 'DBSCAN', eps=0.05, min_samples=5, l2normalize=False, kernels=NumpyDbscanKernels())
    assert np.array_equal(out, dbscan_fp64(X, 0.05, 5)[0])


def test_other_methods_and_metrics_still_raise():
    from video_similarity_search_amd.clustering import fit_cluster
    from video_similarity_search_amd.clustering.dbscan import DBSCAN
    for m in ('Agglomerative', 'OPTICS'):
        with pytest.raises(NotImplementedError):
            fit_cluster(np.zeros((4, 3), np.float32), m)
    with pytest.raises(NotImplementedError):
        DBSCAN(metric='euclidean', kernels=NumpyDbscanKernels()).fit(np.ones((3, 2), np.float32))
    with pytest.raises(ValueError):
        DBSCAN(eps=-0.1, kernels=NumpyDbscanKernels()).fit(np.ones((3, 2), np.float32))


def test_no_device_raises():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.clustering import fit_cluster
    with pytest.raises(_lib.SlicError):
        fit_cluster(torch.randn(64, 8), 'DBSCAN')


class _Loader:
    """an eval loader that never yields slot `skip` (as drop_last would leave a slot unproduced)"""

    def __init__(self, x, skip):
        self.x = x
        self.dataset = list(range(len(x)))
        self.idx = [i for i in range(len(x)) if i != skip]

    def __iter__(self):
        for s in range(0, len(self.idx), 4):
            b = self.idx[s:s + 4]
            yield torch.from_numpy(self.x[b]), torch.zeros(len(b), dtype=torch.long), 0, torch.tensor(b)

    def __len__(self):
        return (len(self.idx) + 3) // 4


def test_iterative_cluster_step_writes_noise_as_minus_one(tmp_path):
    from video_similarity_search_amd.online_train import iterative_cluster_step
    rng = np.random.default_rng(4)
    cen = rng.standard_normal((3, 8)) * 3
    x = np.concatenate([cen[rng.integers(0, 3, 30)] + 0.05 * rng.standard_normal((30, 8)), 5 * rng.standard_normal((6, 8))])
    x = x.astype(np.float32)
    enc = torch.nn.Identity()
    ns = types.SimpleNamespace
    cfg = ns(NUM_GPUS=1, OUTPUT_PATH=str(tmp_path), DATASET=ns(POSITIVE_SAMPLING_P=0.2),
             ITERCLUSTER=ns(METHOD='DBSCAN', K=3, L2_NORMALIZE=True, FINCH_PARTITION=0, ADAPTIVEP=False, SHARDED=True))
    skip = 5
    labels, _ = iterative_cluster_step(None, cfg, enc, _Loader(x, skip), epoch=0, cuda=False, device="cpu",
                                       kmeans_kernels=NumpyDbscanKernels())
    ref = dbscan_fp64(np.delete(x, skip, axis=0), 0.14, 2)[0]
    assert (ref == -1).any() and (ref >= 0).any()
    exp = np.insert(ref, skip, -1)
    assert labels.dtype == np.int32 and np.array_equal(labels, exp)
    lines = open(os.path.join(str(tmp_path), "vid_clusters.txt")).read().splitlines()
    want = [str(v) for v in exp]
    want[skip] = "None"
    assert lines == want

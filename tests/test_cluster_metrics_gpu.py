"""GPU: NMI / AMI on the device (csrc/metrics.hip) against the sklearn goldens and the float64 NumPy provider
(tests/cluster_metrics_cpu_kernels.py, the kernel's arithmetic in the kernel's summation order) at the two working sizes,
bit-equal records across runs and input forms, the contingency-table limit, and the cluster step end to end.

The gate is test_cluster_metrics_cpu.GATE (ten times the provider's measured distance from sklearn over the goldens, never looser
than 1e-9): the device's order is the provider's, and the factor covers the device's lgamma / log / exp."""
import os
import types

import numpy as np
import pytest
import torch

from cluster_metrics_cpu_kernels import cluster_metrics_fp64
from test_cluster_metrics_cpu import GATE, KEYS, _Loader, golden_cases

pytestmark = pytest.mark.gpu


def _scores(lt, lp):
    from video_similarity_search_amd.clustering import cluster_scores
    return cluster_scores(lt, lp)


def working_size(which):
    """the two sizes of the cluster step: 240k videos in 400 classes against 1000 clusters; 100k in 101 classes against a
    FINCH-like first partition of about N / 4 clusters"""
    rng = np.random.default_rng(77 + which)
    if which == 0:
        N = 240000
        lt = rng.integers(0, 400, N)
        lp = np.where(rng.random(N) < 0.4, lt * 2 + rng.integers(0, 2, N), rng.integers(0, 1000, N))
    else:
        N = 100000
        lt = rng.integers(0, 101, N)
        lp = lt * 250 + rng.integers(0, 248, N)
    return lt.astype(np.int32), lp.astype(np.int32)


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_goldens(gpu, case):
    name, lt, lp, rec = case
    s = _scores(lt, lp)
    got = np.array([s[k] for k in KEYS])
    print(name, "max |device - sklearn| =", np.abs(got - rec).max(), "NMI", abs(got[4] - rec[4]), "AMI", abs(got[5] - rec[5]))
    assert np.abs(got - rec).max() <= GATE, (name, got, rec)
    assert s["n_classes"] == len(np.unique(lt)) and s["n_clusters"] == len(np.unique(lp))


@pytest.mark.parametrize("which", [0, 1], ids=["240k_400x1000", "100k_101x25k"])
def test_working_sizes_against_the_provider(gpu, which):
    lt, lp = working_size(which)
    s = _scores(torch.from_numpy(lt).cuda(), torch.from_numpy(lp).cuda())
    ref = cluster_metrics_fp64(lt, lp)
    got = np.array([s[k] for k in KEYS])
    print("classes", s["n_classes"], "clusters", s["n_clusters"], "device", got, "provider", ref[:6])
    print("max |device - provider| =", np.abs(got - ref[:6]).max(), "NMI", abs(got[4] - ref[4]), "AMI", abs(got[5] - ref[5]))
    assert (s["n_classes"], s["n_clusters"]) == (int(ref[6]), int(ref[7])) and ref[8] == 0
    assert s["n_classes"] == (400, 101)[which] and (s["n_clusters"] == 1000 if which == 0 else 20000 < s["n_clusters"] < 26000)
    assert np.abs(got - ref[:6]).max() <= GATE, (got, ref)


@pytest.mark.parametrize("N", [1, 2, 4095, 4096, 4097, 1023, 1024, 1025])
def test_scan_sizes_against_the_provider(gpu, N):
    """the one-workgroup array scan (1024 threads, runs of ceil(n / 1024) elements) on either side of 1024 elements: the radix histogram
    holds 16 * ceil(N / 64) counters (1024 at N = 4096), the head flags N"""
    rng = np.random.default_rng(1000 + N)
    lt = rng.integers(-3, 9, N).astype(np.int32)
    lp = np.where(rng.random(N) < 0.5, lt * 3 + rng.integers(0, 3, N), rng.integers(-40, 40, N)).astype(np.int32)
    s = _scores(torch.from_numpy(lt).cuda(), torch.from_numpy(lp).cuda())
    ref = cluster_metrics_fp64(lt, lp)
    got = np.array([s[k] for k in KEYS])
    print("N", N, "max |device - provider| =", np.abs(got - ref[:6]).max())
    assert (s["n_classes"], s["n_clusters"]) == (int(ref[6]), int(ref[7])) and ref[8] == 0
    assert (s["n_classes"], s["n_clusters"]) == (len(np.unique(lt)), len(np.unique(lp)))
    assert np.abs(got - ref[:6]).max() <= GATE, (got, ref)


def test_bit_identical_across_runs_and_input_forms(gpu):
    lt, lp = working_size(1)
    lt, lp = lt[:30000], lp[:30000] - 7000                                        # negative values too
    first = _scores(lt, lp)
    wide = torch.from_numpy(np.stack([lt, lp, lt], 1)).cuda()                      # columns: strided device views
    forms = [(lt, lp), (lt.tolist(), lp.tolist()), (torch.from_numpy(lt).cuda(), torch.from_numpy(lp).cuda()),
             (torch.from_numpy(lt).long().cuda(), torch.from_numpy(lp)), (wide[:, 0], wide[:, 1]), (wide[:, 2], lp.astype(np.int64))]
    for a, b in forms:
        assert _scores(a, b) == first
    assert not wide[:, 0].is_contiguous() and 0.0 < first["AMI"] < 1.0


def test_contingency_limit_raises(gpu):
    from video_similarity_search_amd import _lib
    n = 8200                                          # all values distinct on both sides: 8200 x 8200 > 2^26 cells
    with pytest.raises(_lib.SlicError):
        _scores(np.arange(n), np.arange(n)[::-1].copy())
    s = _scores(np.arange(8192), np.arange(8192)[::-1].copy())                     # exactly 2^26 cells: taken
    assert s["n_classes"] == 8192 and s["n_clusters"] == 8192 and abs(s["NMI"] - 1.0) < 1e-12
    ok = _scores([0, 0, 1, 1], [5, 5, -1, -1])                                     # the device is still sound after the refusal
    assert ok["NMI"] == 1.0 and ok["AMI"] == 1.0


def test_cluster_step_on_the_device(gpu, tmp_path, capsys):
    from video_similarity_search_amd.clustering import fit_cluster
    from video_similarity_search_amd.online_train import iterative_cluster_step
    rng = np.random.default_rng(5)
    cen = rng.standard_normal((6, 16)) * 3
    y = rng.integers(0, 6, 240)
    x = (cen[y] + 0.05 * rng.standard_normal((240, 16))).astype(np.float32)
    x[200:] = 5 * rng.standard_normal((40, 16))                                   # DBSCAN noise rows
    y[:20] = (y[:20] + 1) % 6
    ns = types.SimpleNamespace
    cfg = ns(NUM_GPUS=1, OUTPUT_PATH=str(tmp_path), DATASET=ns(POSITIVE_SAMPLING_P=0.2),
             ITERCLUSTER=ns(METHOD='DBSCAN', K=6, L2_NORMALIZE=True, FINCH_PARTITION=0, ADAPTIVEP=True, SHARDED=True))
    labels, nmi = iterative_cluster_step(None, cfg, torch.nn.Identity(), _Loader(x, y.astype(np.int64)), epoch=2, cuda=True,
                                         device="cuda")
    out = capsys.readouterr().out
    assert (labels == -1).any() and (labels >= 0).any()
    ref = cluster_metrics_fp64(y, labels)
    assert abs(nmi - ref[4]) <= GATE and 0.0 < nmi < 1.0
    assert cfg.DATASET.POSITIVE_SAMPLING_P == float(1.0 - nmi)
    logs = os.path.join(str(tmp_path), "tnet_checkpoints")
    assert open(os.path.join(logs, "NMIs.txt")).read() == "epoch:2 {:.3f}\n".format(ref[4])
    assert open(os.path.join(logs, "AMIs.txt")).read() == "epoch:2 {:.3f}\n".format(ref[5])
    assert "NMI between true labels and cluster assignments: {:.3f}".format(ref[4]) in out
    assert "AMI between true labels and cluster assignments: {:.3f}".format(ref[5]) in out


def test_max_cells_bounds_the_table(gpu):
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.clustering import cluster_scores
    rng = np.random.default_rng(9)
    lt, lp = rng.integers(0, 40, 20000), rng.integers(0, 100, 20000)
    ref = cluster_scores(lt, lp)
    assert cluster_scores(lt, lp, max_cells=4000) == ref                           # exactly 40 x 100 cells: taken
    with pytest.raises(_lib.SlicError):
        cluster_scores(lt, lp, max_cells=3999)
    with pytest.raises(ValueError):
        cluster_scores(lt, lp, max_cells=(1 << 26) + 1)
    assert cluster_scores(lt, lp) == ref

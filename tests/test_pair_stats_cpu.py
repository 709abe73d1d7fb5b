"""CPU: the host side of the pair statistics (video_similarity_search_amd/pairstats.py) — `separation` on hand-made histograms with
known answers, the argument errors, the summary through the NumPy provider (tests/pair_stats_cpu_kernels.py), and the cluster step's
opt-in lines; the device path is test_pair_stats_gpu.py."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from pair_stats_cases import clustered_rows, exact_rows, run_step_recorded
from pair_stats_cpu_kernels import NumpyPairStatsKernels, pair_stats_fp64


def _sep(hs, hd, **kw):
    from video_similarity_search_amd.pairstats import separation
    return separation({"hist_same": np.array(hs), "hist_diff": np.array(hd)}, **kw)


# ---- separation ----

def test_separation_disjoint_groups():
    s = _sep([5, 3, 0, 0, 0, 0, 0, 0], [0, 0, 0, 4, 4, 0, 0, 2])
    assert s["auc"] == 1.0 and s["auc_bounds"] == (1.0, 1.0)
    assert s["eer"] == 0.0 and s["eer_edge"] == 0.5              # the first edge with FAR = FRR = 0: above both same bins
    assert s["tar_at_far"] == {1e-3: 1.0, 1e-2: 1.0} and s["edge_at_far"] == {1e-3: 0.75, 1e-2: 0.75}
    assert s["d_at_precision"] == {0.9: 0.75, 0.99: 0.75}
    assert (s["n_same"], s["n_diff"]) == (8, 10)


def test_separation_identical_groups():
    s = _sep([1, 2, 3, 4, 0, 0, 0, 0], [1, 2, 3, 4, 0, 0, 0, 0])
    assert s["auc"] == 0.5
    lo, hi = s["auc_bounds"]
    assert lo == 35 / 100 and hi == 65 / 100 and lo <= s["auc"] <= hi      # ties: 1 + 4 + 9 + 16 = 30 of 100 couples
    assert s["d_at_precision"] == {0.9: None, 0.99: None}        # precision is 0.5 at every edge
    assert s["tar_at_far"][1e-3] == 0.0 and s["edge_at_far"][1e-3] == 0.0


def test_separation_hand_computed():
    """same [4, 3, 2, 1, 0 ..], diff [0, 1, 2, 3, 4, 0 ..]: edges 0, .25, .5, ...
    S = 0 4 7 9 10 10 .., F = 0 0 1 3 6 10 ..  lost = 4 * 10 + 3 * 9 + 2 * 7 + 1 * 4 = 85, ties = 3 + 4 + 3 = 10"""
    s = _sep([4, 3, 2, 1, 0, 0, 0, 0], [0, 1, 2, 3, 4, 0, 0, 0], far=(0.0, 0.1, 0.3, 0.5), precision=(1.0, 0.8, 0.75, 0.5))
    assert s["auc"] == (2 * 85 + 10) / 200 and s["auc_bounds"] == (0.85, 0.95)
    assert s["auc_bounds"][0] <= s["auc"] <= s["auc_bounds"][1]
    # FAR - FRR at k = 0 ..: -1, -.6, -.2, +.2, ... : |.| smallest first at k = 2 (FAR .1, FRR .3)
    assert s["eer_edge"] == 0.5 and s["eer"] == pytest.approx(0.2)
    assert s["tar_at_far"] == {0.0: 0.4, 0.1: 0.7, 0.3: 0.9, 0.5: 0.9}
    assert s["edge_at_far"] == {0.0: 0.25, 0.1: 0.5, 0.3: 0.75, 0.5: 0.75}
    # precision at k = 1 ..: 4/4, 7/8, 9/12, 10/16, 10/20 (and 10/20 up to the last edge)
    assert s["d_at_precision"] == {1.0: 0.25, 0.8: 0.5, 0.75: 0.75, 0.5: 2.0}


def test_separation_empty_group_and_bad_input():
    s = _sep([0] * 8, [1] * 8)
    assert math.isnan(s["auc"]) and math.isnan(s["eer"]) and s["d_at_precision"][0.9] is None
    from video_similarity_search_amd.pairstats import separation
    with pytest.raises(ValueError):
        separation({"hist_same": np.zeros(8), "hist_diff": np.zeros(16)})


# ---- the public functions through the NumPy provider ----

def test_summary_follows_the_oracle():
    from video_similarity_search_amd.pairstats import pair_statistics
    x, lab = clustered_rows(90, 8, 5, centres=4)
    lab[:7] = -1
    k = NumpyPairStatsKernels()
    st = pair_statistics(x, lab, bins=64, t=0.5, ignore_label=-1, kernels=k)
    o = pair_stats_fp64(x, lab, bins=64, t=0.5, ignore_label=-1)
    ds, dd = o["d"][1], o["d"][0]
    assert len(k.calls) == 1 and k.calls[0][5:] == (64, 0.5, -1)
    assert st["n_same"] == len(ds) and st["n_diff"] == len(dd) and st["n_same"] + st["n_diff"] == 83 * 82 // 2
    assert st["hist_same"].dtype == np.int64 and np.array_equal(st["hist_same"], o["hist"][1]) and np.array_equal(st["hist_diff"], o["hist"][0])
    assert np.array_equal(st["edges"], np.arange(65) / 32.0)
    assert st["mean_same"] == pytest.approx(ds.mean(), rel=1e-12) and st["std_diff"] == pytest.approx(dd.std(), rel=1e-9)
    assert st["mean_same"] < st["mean_diff"]
    assert st["uniformity"] == pytest.approx(math.log(np.exp(-np.concatenate([ds, dd])).mean()), rel=1e-12)      # 2 t = 1
    assert st["uniformity_diff"] == pytest.approx(math.log(np.exp(-dd).mean()), rel=1e-12)
    # no labels: one group, and NaN for the empty one
    st = pair_statistics(torch.from_numpy(x), kernels=k)
    assert st["n_same"] == 0 and st["n_diff"] == 90 * 89 // 2 and math.isnan(st["mean_same"]) and math.isnan(st["std_same"])
    assert st["hist_same"].shape == (256,) and st["bins"] == 256
    # one row: nothing is counted
    st = pair_statistics(x[:1], lab[:1], kernels=k)
    assert st["n_same"] == st["n_diff"] == 0 and math.isnan(st["uniformity"]) and math.isnan(st["uniformity_diff"])


def test_view_statistics():
    from video_similarity_search_amd.pairstats import separation, view_statistics
    x, _ = clustered_rows(40, 8, 6)
    z2 = (x + 0.1 * np.random.default_rng(1).standard_normal(x.shape)).astype(np.float32)
    k = NumpyPairStatsKernels()
    v = view_statistics(x, z2, bins=64, kernels=k)
    assert v["n_same"] == 40 and v["n_diff"] == 40 * 39
    a, b = x.astype(np.float64), z2.astype(np.float64)
    a, b = a / np.linalg.norm(a, axis=1)[:, None], b / np.linalg.norm(b, axis=1)[:, None]
    assert v["alignment"] == pytest.approx(((a - b) ** 2).sum(1).mean(), rel=1e-9)
    neg = ((a[:, None, :] - b[None, :, :]) ** 2).sum(2)[~np.eye(40, dtype=bool)]
    assert v["uniformity"] == pytest.approx(math.log(np.exp(-2.0 * neg).mean()), rel=1e-9)
    assert separation(v)["auc"] > 0.9
    assert view_statistics(x, x, kernels=k)["alignment"] <= 1e-12
    with pytest.raises(ValueError, match="one shape"):
        view_statistics(x, z2[:-1], kernels=k)


def test_argument_errors():
    from video_similarity_search_amd.pairstats import pair_statistics
    x = exact_rows(10, 1)
    lab = np.arange(10) % 3
    k = NumpyPairStatsKernels()
    for bins in (4, 8192, 100, 0, -8, 12, 2.0 ** 8, True):
        with pytest.raises(ValueError, match="bins"):
            pair_statistics(x, lab, bins=bins, kernels=k)
    for t in (0, -1.0, float("nan"), float("inf"), "2"):
        with pytest.raises(ValueError, match="t must"):
            pair_statistics(x, lab, t=t, kernels=k)
    with pytest.raises(ValueError, match="inconsistent"):
        pair_statistics(x, lab[:9], kernels=k)
    with pytest.raises(ValueError, match="inconsistent"):
        pair_statistics(x, lab, x[:5], lab, kernels=k)
    with pytest.raises(ValueError, match="both sides"):
        pair_statistics(x, lab, x, None, kernels=k)
    with pytest.raises(ValueError, match="both sides"):
        pair_statistics(x, None, x, lab, kernels=k)
    with pytest.raises(ValueError, match="y_labels without y"):
        pair_statistics(x, lab, None, lab, kernels=k)
    with pytest.raises(ValueError, match="2D"):
        pair_statistics(x[0], kernels=k)
    with pytest.raises(ValueError, match="2D"):
        pair_statistics(x, lab, torch.zeros(16), lab, kernels=k)
    with pytest.raises(ValueError, match="columns"):
        pair_statistics(x, lab, x[:, :8], lab, kernels=k)
    with pytest.raises(ValueError, match="1D"):
        pair_statistics(x, lab.reshape(5, 2), kernels=k)
    with pytest.raises(ValueError, match="ignore_label"):
        pair_statistics(x, lab, ignore_label=2 ** 31, kernels=k)
    assert k.calls == []


def test_reachable_from_evaluate_and_no_device_raises():
    from video_similarity_search_amd import _lib, evaluate, pairstats
    assert evaluate.pair_statistics is pairstats.pair_statistics and evaluate.view_statistics is pairstats.view_statistics
    assert evaluate.separation is pairstats.separation and evaluate.HipPairStatsKernels is pairstats.HipPairStatsKernels
    if not torch.cuda.is_available():
        with pytest.raises(_lib.SlicError):
            pairstats.pair_statistics(exact_rows(10, 1))


def test_workspace_query_states_the_limits():
    """host only: the query answers 0 for what the call rejects and holds no N x N array"""
    from video_similarity_search_amd import _lib
    q = _lib.load().slic_pair_stats_workspace_bytes
    assert q(1, 0, 1, 8) > 0 and q(1 << 20, 0, 512, 4096) > 0 and q(1 << 20, 1 << 20, 128, 256) > 0 and q(5, 300, 16, 8) > 0
    assert q(0, 0, 8, 8) == 0 and q((1 << 20) + 1, 0, 8, 8) == 0 and q(10, (1 << 20) + 1, 8, 8) == 0 and q(10, -1, 8, 8) == 0
    assert q(10, 0, 0, 8) == 0 and q(10, 0, 513, 8) == 0
    assert q(10, 0, 8, 4) == 0 and q(10, 0, 8, 8192) == 0 and q(10, 0, 8, 24) == 0
    n = 100000
    assert q(n, 0, 128, 256) < 4 * n * 128 + 8 * n + (1 << 22) < 8 * n * n


# ---- the cluster step ----

@pytest.mark.parametrize("flag", [None, 0])
def test_cluster_step_without_the_flag_is_the_parent_commits(tmp_path, flag):
    """provider calls, stdout, log files, labels and NMI of the step with the flag absent / 0 equal the record made before the lines existed"""
    k = NumpyPairStatsKernels()
    rec = run_step_recorded(os.path.join(str(tmp_path), "off"), pair_stats=flag, pairstats_kernels=k)
    want = json.load(open(os.path.join(GOLDEN, "pair_stats_cluster_step_parent.json")))
    assert rec == want and k.calls == []


def test_cluster_step_opt_in_lines(tmp_path):
    from silhouette_cases import step_inputs
    from video_similarity_search_amd.pairstats import separation
    k = NumpyPairStatsKernels()
    rec = run_step_recorded(os.path.join(str(tmp_path), "on"), pair_stats=64, pairstats_kernels=k)
    want = json.load(open(os.path.join(GOLDEN, "pair_stats_cluster_step_parent.json")))
    x, y = step_inputs()
    y[-3:] = -1
    o = pair_stats_fp64(x, y, bins=64, ignore_label=-1)
    assert o["record"][0] + o["record"][1] == 57 * 56 // 2            # the three unlabelled rows are in no pair
    ds, dd = o["d"][1], o["d"][0]
    sep = separation({"hist_same": o["hist"][1], "hist_diff": o["hist"][0]})
    assert sep["d_at_precision"][0.9] is None                   # six rows of the tight groups carry a wrong true label
    text = "intra {:.3f} +- {:.3f} inter {:.3f} +- {:.3f} AUC {:.3f} d(precision 0.9) none".format(
        ds.mean(), ds.std(), dd.mean(), dd.std(), sep["auc"])
    line = "Pair distances (cosine) under the true labels: " + text + "\n"
    # exactly one more print, after the NMI / AMI lines, and one more file
    assert rec["stdout"].replace(line, "", 1) == want["stdout"] and rec["stdout"].count("Pair distances") == 1
    assert rec["stdout"].index("AMI between") < rec["stdout"].index(line) < rec["stdout"].index("Saved cluster labels")
    extra = {n: t for n, t in rec["files"].items() if n not in want["files"]}
    assert extra == {"tnet_checkpoints/pair_stats.txt": "epoch:3 " + text + "\n"}
    assert {n: t for n, t in rec["files"].items() if n in want["files"]} == want["files"]
    assert rec["labels"] == want["labels"] and rec["nmi"] == want["nmi"]
    assert rec["calls"][:len(want["calls"])] == want["calls"]
    assert rec["calls"][len(want["calls"]):] == ["pairstats.resident_rows", "pairstats.resident_labels", "pairstats.pair_stats"]
    assert len(k.calls) == 1 and k.calls[0][1] == (60, 8) and k.calls[0][5:] == (64, 2.0, -1)


def test_cluster_step_line_names_the_threshold(tmp_path, capsys):
    """the line of the step on rows whose classes separate: the distance below which 0.9 of the pairs share a label is an edge"""
    import types
    from video_similarity_search_amd import online_train
    from video_similarity_search_amd.pairstats import separation
    x, lab = clustered_rows(80, 8, 9, centres=4, spread=0.2)
    cfg = types.SimpleNamespace(OUTPUT_PATH=str(tmp_path))
    online_train._pair_stats_lines(cfg, 7, torch.from_numpy(x), lab.astype(np.int64), 256, NumpyPairStatsKernels())
    o = pair_stats_fp64(x, lab, bins=256, ignore_label=-1)
    sep = separation({"hist_same": o["hist"][1], "hist_diff": o["hist"][0]})
    d90 = sep["d_at_precision"][0.9]
    assert d90 is not None and 0 < d90 < 1 and d90 * 128 == int(d90 * 128)
    text = "intra {:.3f} +- {:.3f} inter {:.3f} +- {:.3f} AUC {:.3f} d(precision 0.9) {:.4f}".format(
        o["d"][1].mean(), o["d"][1].std(), o["d"][0].mean(), o["d"][0].std(), sep["auc"], d90)
    assert capsys.readouterr().out == "Pair distances (cosine) under the true labels: " + text + "\n"
    assert open(os.path.join(str(tmp_path), "tnet_checkpoints", "pair_stats.txt")).read() == "epoch:7 " + text + "\n"


def test_cluster_step_sharded_route_refuses_the_flag(tmp_path, monkeypatch):
    import types
    from video_similarity_search_amd import online_train
    monkeypatch.setattr(online_train, "_cluster_sharded", lambda cfg: True)

    class NoLoader:
        dataset = list(range(60))

        def __iter__(self):
            raise AssertionError("the flag must be refused before the embeddings are computed")

    def no_collective(*a, **kw):
        raise AssertionError("the flag must be refused before any collective")

    for name in ("all_reduce", "all_gather", "barrier", "broadcast"):
        monkeypatch.setattr(torch.distributed, name, no_collective)
    ns = types.SimpleNamespace
    cfg = ns(NUM_GPUS=2, OUTPUT_PATH=str(tmp_path), ITERCLUSTER=ns(METHOD='kmeans', K=4, L2_NORMALIZE=True, SHARDED=True, PAIR_STATS=256))
    with pytest.raises(NotImplementedError, match="PAIR_STATS"):
        online_train.iterative_cluster_step(None, cfg, torch.nn.Identity(), NoLoader(), epoch=0, cuda=False, device="cpu")

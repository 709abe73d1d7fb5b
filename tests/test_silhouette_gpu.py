"""GPU: the silhouette call (csrc/silhouette.hip) against sklearn's goldens and the float64 reference under the derived gate of
test_silhouette_cpu.py, at the score kernel's edges (rows, columns and k that are no multiple of a tile, shares of the K-group split
with no tile, K = N - 1), and the call's contract: every output written, the workspace's end respected, bit-equal repeats, input
forms, ignore_label, the status paths, and the cluster step end to end.  Every case prints its worst error and slack."""
import ctypes
import os

import numpy as np
import pytest
import torch

from silhouette_cases import GOLDEN_CASES, METRICS, Loader, draw, run_step
from silhouette_cpu_kernels import check_mean, check_rows, deltas, gates, silhouette_fp64
from test_silhouette_cpu import CASES, Z, case, tie_case, zero_row_case

pytestmark = pytest.mark.gpu
GUARD = 4096


def raw_call(x, labels, metric, ignore_label=None, kmax=None):
    """slic_silhouette on device tensors with NaN-filled outputs and a guard pattern behind the workspace -> host arrays"""
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd._lib import call, ptr, stream
    N, D = x.shape
    kmax = N - 1 if kmax is None else kmax
    nbytes = _lib.load().slic_silhouette_workspace_bytes(N, D, kmax)
    assert nbytes > 0
    ws = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    f = torch.full((3, N), float("nan"), dtype=torch.float32, device="cuda")
    near = torch.full((N,), -777, dtype=torch.int32, device="cuda")
    rec = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
    cm = torch.full((kmax,), 123.0, dtype=torch.float64, device="cuda")
    cl = torch.full((kmax,), -777, dtype=torch.int32, device="cuda")
    call("slic_silhouette", ptr(x), N, D, x.stride(0), ptr(labels), {"cosine": 0, "sqeuclidean": 1}[metric], 0 if ignore_label is None else 1,
         ctypes.c_int32(0 if ignore_label is None else ignore_label), kmax, ptr(f[0]), ptr(f[1]), ptr(f[2]), ptr(near), ptr(rec), ptr(cm),
         ptr(cl), ptr(ws), stream())
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all()), "the call wrote past its workspace"
    fh = f.cpu().numpy()
    return dict(s=fh[0], a=fh[1], b=fh[2], nearest=near.cpu().numpy(), record=rec.cpu().numpy(), cluster_mean=cm.cpu().numpy(),
                cluster_label=cl.cpu().numpy())


def dev(x, labels):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()


def check_against(out, x, labels, metric, ref, what):
    """rows, mean, parts, nearest label, per-cluster means and the counts of a raw call against the float64 reference; the parts are
    held to the bound the row gate is derived from (a: 2 delta, b: delta)"""
    check_rows(out["s"], x, ref, metric, what)
    assert out["record"][3] == 0 and out["record"][1] == ref["n_clusters"] and out["record"][2] == ref["n_rows"]
    check_mean(float(out["record"][0]), x, ref, metric, what)
    scored = ~np.isnan(ref["s"])
    delta = deltas(x, ref, metric)
    assert np.array_equal(np.isnan(out["a"]), ~scored) and np.array_equal(np.isnan(out["b"]), ~scored)
    assert (np.abs(out["a"] - ref["a"])[scored] <= 2 * delta[scored]).all() and (np.abs(out["b"] - ref["b"])[scored] <= delta[scored]).all()
    # the nearest cluster is the reference's, or (a near-tie) one whose distance is within the bound of the reference's
    differ = np.flatnonzero(scored & (out["nearest"] != ref["nearest"]))
    assert len(differ) <= 0.01 * scored.sum(), differ[:5]
    K = ref["n_clusters"]
    assert np.array_equal(out["cluster_label"][:K], ref["cluster_label"])
    gate, gated = gates(x, ref, metric)
    if gated.sum() == scored.sum():                     # every row gated: a cluster's mean is within its rows' largest gate
        assert np.abs(out["cluster_mean"][:K] - ref["cluster_mean"]).max() <= gate[gated].max()
    assert np.isnan(out["cluster_mean"][K:]).all() and (out["cluster_label"][K:] == 0).all()


@pytest.mark.parametrize("name,metric", CASES)
def test_goldens(gpu, name, metric):
    x, labels, ref = case(name, metric)
    out = raw_call(*dev(x, labels), metric)
    check_against(out, x, labels, metric, ref, "{} {}".format(name, metric))
    gold = Z["{}__{}__samples".format(name, metric)]
    d = np.abs(out["s"] - gold).max()
    print(name, metric, "max |device - sklearn| =", d, " score: device", out["record"][0], "sklearn", float(Z["{}__{}__score".format(name, metric)]))
    assert np.abs(ref["s"] - gold).max() <= 1e-12                                 # so the gate against float64 is the gate against sklearn


# (N, D, K): rows 129 / 517 / 1000 (no multiple of the 128-row tile), D % 8 != 0 and D past one 32-wide k-tile and at the limit, K on both
# sides of the 64- and 128-column boundaries, more shares than cluster tiles (K = 2, 3), K = N - 1
EDGES = [(129, 8, 2), (129, 20, 3), (129, 24, 128), (517, 136, 127), (517, 24, 129), (517, 512, 300), (517, 20, 516), (1000, 8, 300),
         (1000, 136, 129), (1000, 20, 999), (517, 24, 128)]


@pytest.mark.parametrize("shape", EDGES, ids=lambda s: "n{}_d{}_k{}".format(*s))
@pytest.mark.parametrize("metric", METRICS)
def test_edges(gpu, shape, metric):
    N, D, K = shape
    x, labels = draw(1000 + N + D + K, N, D, K, 0.3, singletons=3 if K > 6 else 0)
    ref = silhouette_fp64(x, labels, metric)
    assert ref["n_clusters"] == K
    out = raw_call(*dev(x, labels), metric)
    check_against(out, x, labels, metric, ref, "n{} d{} k{} {}".format(N, D, K, metric))
    last = labels == labels.max()                     # K % 64 == 0: the rows whose own cluster is the last column of the last tile
    assert last.any() and np.array_equal(np.isnan(out["s"][last]), np.isnan(ref["s"][last]))


@pytest.mark.parametrize("shape,metric", [((1025, 8, 12), "cosine"), ((4097, 8, 40), "sqeuclidean")], ids=["n1025", "n4097"])
def test_label_scan_sizes(gpu, shape, metric):
    """the dense ids' one-workgroup array scan past 1024 elements: the head flags (N = 1025), the radix histogram (16 * ceil(N / 64) = 1040
    counters at N = 4097)"""
    N, D, K = shape
    x, labels = draw(1000 + N + D + K, N, D, K, 0.3, singletons=3)
    ref = silhouette_fp64(x, labels, metric)
    assert ref["n_clusters"] == K
    check_against(raw_call(*dev(x, labels), metric), x, labels, metric, ref, "n{} d{} k{} {}".format(N, D, K, metric))


@pytest.mark.parametrize("metric", METRICS)
def test_one_large_cluster(gpu, metric):
    x, labels = draw(31, 517, 24, 9, 0.3, singletons=0)
    big = np.arange(517) % 5 < 3                        # 311 of 517 rows in one cluster, spread over the other clusters' places
    labels = np.where(big, 1000, labels).astype(np.int32)
    ref = silhouette_fp64(x, labels, metric)
    assert (labels == 1000).sum() > 517 // 2
    gate_rows = np.maximum(ref["a"], ref["b"]) >= 0.05
    assert gate_rows.mean() >= 0.99
    check_against(raw_call(*dev(x, labels), metric), x, labels, metric, ref, "one large cluster " + metric)


def test_duplicates_and_zero_row(gpu):
    # exactly representable duplicates: two clusters of the same unit vector (cosine) / integer rows (sqeuclidean) -> a = b = 0 -> s = 0
    e = np.zeros((12, 8), np.float32)
    e[:8, 0] = 3.0
    e[8:, 1] = 2.0
    labels = np.array([5] * 4 + [7] * 4 + [9] * 4, np.int32)
    for metric in METRICS:
        out = raw_call(*dev(e, labels), metric)
        assert (out["a"][:8] == 0).all() and (out["b"][:8] == 0).all() and (out["s"][:8] == 0).all(), out
        assert (out["nearest"][:4] == 7).all() and (out["nearest"][4:8] == 5).all()
        assert (out["s"][8:] == 1.0).all() and (out["nearest"][8:] == 5).all()      # a tie between 5 and 7: the first wins
    x, labels = tie_case()
    for metric in METRICS:
        assert (raw_call(*dev(x, labels), metric)["nearest"][:9] == 10).all()
    x, labels = zero_row_case()
    ref = silhouette_fp64(x, labels, "cosine")
    out = raw_call(*dev(x, labels), "cosine")
    check_against(out, x, labels, "cosine", ref, "zero row")
    assert out["a"][7] == 1.0 and out["b"][7] == 1.0 and out["s"][7] == 0.0


def test_repeats_and_input_forms(gpu):
    from video_similarity_search_amd.clustering import silhouette_report, silhouette_samples, silhouette_score
    x, labels, ref = case("n1000_d128_k40", "cosine")
    for metric in METRICS:
        xd, ld = dev(x, labels)
        a, b = raw_call(xd, ld, metric), raw_call(xd, ld, metric)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
    first = silhouette_report(x, labels)
    wide = torch.from_numpy(np.concatenate([x, x], 1)).cuda()
    view = wide[:, :128]
    assert not view.is_contiguous()
    for form in (torch.from_numpy(x), torch.from_numpy(x).cuda(), view, x.astype(np.float64)):
        assert silhouette_report(form, labels) == first
    assert silhouette_report(view, torch.from_numpy(labels).cuda().long()) == first
    assert silhouette_score(x, labels) == first["score"]
    assert silhouette_score(view[::2], labels[::2]) == silhouette_score(np.ascontiguousarray(x[::2]), labels[::2])      # a row-strided view in place
    s = silhouette_samples(view, labels)
    check_rows(s, x, ref, "cosine", "public samples")
    got = silhouette_score(x, labels, sample_size=200, random_state=3)
    idx = np.random.RandomState(3).permutation(1000)[:200]
    check_mean(got, x[idx], silhouette_fp64(x[idx], labels[idx], "cosine"), "cosine", "sample_size=200")


@pytest.mark.parametrize("metric", METRICS)
def test_ignore_label_equals_removal(gpu, metric):
    x, labels, _ = case("n517_d24_k30", metric)
    keep = labels != -1
    out = raw_call(*dev(x, labels), metric, ignore_label=-1)
    sub = raw_call(*dev(x[keep], labels[keep]), metric)
    for k in ("s", "a", "b"):
        assert np.isnan(out[k][~keep]).all() and out[k][keep].tobytes() == sub[k].tobytes(), k
    assert (out["nearest"][~keep] == -1).all() and np.array_equal(out["nearest"][keep], sub["nearest"])
    assert out["record"].tobytes() == sub["record"].tobytes() and out["record"][1] == 29 and out["record"][2] == keep.sum()
    assert out["cluster_mean"][:29].tobytes() == sub["cluster_mean"][:29].tobytes()
    assert np.array_equal(out["cluster_label"][:29], sub["cluster_label"][:29]) and -1 not in out["cluster_label"][:29]
    absent = raw_call(*dev(x, labels), metric, ignore_label=4)               # a label nobody carries: nothing is ignored
    plain = raw_call(*dev(x, labels), metric)
    assert all(absent[k].tobytes() == plain[k].tobytes() for k in plain)


def test_status_paths_leave_the_device_sound(gpu):
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.clustering import silhouette_score
    from video_similarity_search_amd.clustering.metrics import HipSilhouetteKernels
    x, labels, ref = case("n300_d16_k7", "cosine")
    xd, ld = dev(x, labels)
    for bad, status, k in ((np.zeros(300, np.int32), 1, 1), (np.arange(300, dtype=np.int32) * 3 - 7, 1, 300)):
        out = raw_call(xd, torch.from_numpy(bad).cuda(), "cosine")
        assert out["record"][3] == status and out["record"][1] == k and np.isnan(out["record"][0])
        assert np.isnan(out["s"]).all() and np.isnan(out["a"]).all() and np.isnan(out["b"]).all() and (out["nearest"] == 0).all()
        assert np.isnan(out["cluster_mean"]).all()
        check_against(raw_call(xd, ld, "cosine"), x, labels, "cosine", ref, "after status {}".format(status))
    out = raw_call(xd, ld, "cosine", kmax=6)                                   # 7 clusters, room for 6
    assert out["record"][3] == 2 and np.isnan(out["s"]).all()
    check_against(raw_call(xd, ld, "cosine", kmax=7), x, labels, "cosine", ref, "kmax = K")
    with pytest.raises(ValueError, match="Number of labels is 1"):
        silhouette_score(x, np.zeros(300, np.int32))
    with pytest.raises(ValueError, match="Number of labels is 300"):
        silhouette_score(xd, np.arange(300))
    with pytest.raises(_lib.SlicError):
        silhouette_score(x, labels, kernels=HipSilhouetteKernels(max_clusters=6))
    check_mean(silhouette_score(x, labels, kernels=HipSilhouetteKernels(max_clusters=7)), x, ref, "cosine", "max_clusters = K")


def test_cluster_step_on_the_device(gpu, tmp_path, capsys):
    rng = np.random.default_rng(5)
    cen = rng.standard_normal((6, 16)) * 3
    y = rng.integers(0, 6, 240)
    x = (cen[y] + 0.05 * rng.standard_normal((240, 16))).astype(np.float32)
    x[200:] = 5 * rng.standard_normal((40, 16))                                   # DBSCAN noise rows
    labels, nmi, files = run_step(os.path.join(str(tmp_path), "on"), x, y.astype(np.int64), silhouette=True, cuda=True, device="cuda")
    out = capsys.readouterr().out
    assert (labels == -1).any() and (labels >= 0).any()
    ref = silhouette_fp64(x, labels, "cosine", ignore_label=-1)
    line = [l for l in out.splitlines() if l.startswith("Silhouette (cosine) of the cluster assignments: ")]
    gate, gated = gates(x, ref, "cosine")
    assert len(line) == 1 and abs(float(line[0].split(": ")[1]) - ref["score"]) <= 0.0005 + gate[gated].mean()      # three printed decimals
    assert files["tnet_checkpoints/silhouettes.txt"] == "epoch:3 " + line[0].split(": ")[1] + "\n"
    assert out.index("AMI between") < out.index(line[0])

"""The silhouette tests' inputs: the golden cases' recipe (tests/golden/make_goldens_silhouette.py stores sklearn's answers and a
checksum of what this draws) and the small cluster step of the opt-in lines."""
import hashlib
import os
import types

import numpy as np
import torch

# name: (seed, N, D, K, spread)
GOLDEN_CASES = {
    "n300_d16_k7": (101, 300, 16, 7, 0.3),
    "n1000_d128_k40": (102, 1000, 128, 40, 0.35),
    "n1000_d128_k40_tight": (103, 1000, 128, 40, 0.05),
    "n517_d24_k30": (104, 517, 24, 30, 1.0),
    "n700_d20_k129": (105, 700, 20, 129, 0.5),          # D % 8 != 0, K on both sides of a 128-column boundary
}
METRICS = ("cosine", "sqeuclidean")


def draw(seed, N, D, K, spread, singletons=3):
    """x = centre_z + spread * noise as fp32; labels 3 z - 1 (so -1 and gaps occur); the last `singletons` centres hold one row
    each, every other centre at least one"""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((K, D))
    z = np.concatenate([np.arange(K), rng.integers(0, K - singletons, N - K)])
    rng.shuffle(z)
    x = (cen[z] + spread * rng.standard_normal((N, D))).astype(np.float32)
    return x, (3 * z - 1).astype(np.int32)


def checksum(x, labels):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes() + np.ascontiguousarray(labels).tobytes()).hexdigest()


class Loader:
    """an eval loader over rows x with true labels y, batches of 4"""

    def __init__(self, x, y):
        self.x, self.y = x, y
        self.dataset = list(range(len(x)))

    def __iter__(self):
        for s in range(0, len(self.x), 4):
            b = list(range(s, min(s + 4, len(self.x))))
            yield torch.from_numpy(self.x[b]), torch.from_numpy(self.y[b]), 0, torch.tensor(b)

    def __len__(self):
        return (len(self.x) + 3) // 4


def step_inputs(n=60, d=8, noise=10, seed=11):
    """four tight groups and `noise` scattered rows DBSCAN (cosine, eps 0.14) leaves as -1"""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((4, d)) * 3
    y = rng.integers(0, 4, n)
    x = (cen[y] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    x[n - noise:] = 5 * rng.standard_normal((noise, d))
    y[:6] = (y[:6] + 1) % 4
    return x, y.astype(np.int64)


def run_step(out, x, y, *, silhouette=None, cuda=False, device="cpu", method="DBSCAN", **kw):
    """one iterative_cluster_step into directory `out`; -> (labels, NMI, {log file name: text})"""
    from video_similarity_search_amd.online_train import iterative_cluster_step
    os.makedirs(out)
    ns = types.SimpleNamespace
    it = ns(METHOD=method, K=4, L2_NORMALIZE=True, FINCH_PARTITION=0, ADAPTIVEP=True, SHARDED=True)
    if silhouette is not None:
        it.SILHOUETTE = silhouette
    cfg = ns(NUM_GPUS=1, OUTPUT_PATH=out, DATASET=ns(POSITIVE_SAMPLING_P=0.2), ITERCLUSTER=it)
    labels, nmi = iterative_cluster_step(None, cfg, torch.nn.Identity(), Loader(x, y), epoch=3, cuda=cuda, device=device, **kw)
    files = {}
    for d, _, names in os.walk(out):
        for n in names:
            files[os.path.relpath(os.path.join(d, n), out)] = open(os.path.join(d, n)).read()
    return labels, nmi, files


def normalise_step_output(text, out):
    """what differs between two runs of the same step: the output directory and the wall-clock times"""
    import re
    return re.sub(r"\d+\.\d+s", "<T>s", text.replace(out, "<OUT>"))


def run_step_recorded(out, **kw):
    """the recorded form of a step on step_inputs() with the NumPy DBSCAN and NMI / AMI providers: {'stdout', 'files', 'labels', 'nmi'}"""
    import contextlib
    import io
    from cluster_metrics_cpu_kernels import NumpyClusterMetricsKernels
    from dbscan_cpu_kernels import NumpyDbscanKernels
    x, y = step_inputs()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        labels, nmi, files = run_step(out, x, y, kmeans_kernels=NumpyDbscanKernels(), metrics_kernels=NumpyClusterMetricsKernels(), **kw)
    return {"stdout": normalise_step_output(buf.getvalue(), out), "files": {k: normalise_step_output(v, out) for k, v in sorted(files.items())},
            "labels": [int(v) for v in labels], "nmi": float(nmi)}

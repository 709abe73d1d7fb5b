"""The pair-statistics tests' inputs, and the small recorded cluster step of the opt-in lines (the step of tests/silhouette_cases.py with
every provider call logged; tests/golden/make_goldens_pair_stats_cluster_step.py stores the parent commit's record)."""
import contextlib
import io
import os
import types

import numpy as np
import torch

from silhouette_cases import Loader, normalise_step_output, step_inputs


def exact_rows(n, seed, D=16):
    """rows with four entries of +-0.5: ||x|| = 1 exactly, every dot product a multiple of 0.25, so every d is one of 0, 0.25 .. 2
    in float32 and in float64 alike.  Rows 1 and 2 repeat row 0, row 3 is its antipode (d = 0 and d = 2 occur from n = 4 on)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, D), dtype=np.float32)
    for i in range(n):
        x[i, rng.choice(D, 4, replace=False)] = rng.choice([-0.5, 0.5], 4)
    if n >= 4:
        x[1] = x[0]
        x[2] = x[0]
        x[3] = -x[0]
    return x


def clustered_rows(n, D, seed, centres=12, spread=0.5):
    """Gaussian rows around `centres` centres; -> (x fp32 [n, D], labels int32 [n])"""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((centres, D))
    z = rng.integers(0, centres, n)
    return (cen[z] + spread * rng.standard_normal((n, D))).astype(np.float32), z.astype(np.int32)


class Recorded:
    """a provider whose method calls are appended to `log` as 'name.method'"""

    def __init__(self, inner, name, log):
        self._inner, self._name, self._log = inner, name, log

    def __getattr__(self, attr):
        v = getattr(self._inner, attr)
        if not callable(v):
            return v

        def method(*a, **kw):
            self._log.append("{}.{}".format(self._name, attr))
            return v(*a, **kw)
        return method


def run_step(out, x, y, *, pair_stats=None, method="DBSCAN", **kw):
    """one iterative_cluster_step into directory `out`; -> (labels, NMI, {log file name: text})"""
    from video_similarity_search_amd.online_train import iterative_cluster_step
    os.makedirs(out)
    ns = types.SimpleNamespace
    it = ns(METHOD=method, K=4, L2_NORMALIZE=True, FINCH_PARTITION=0, ADAPTIVEP=True, SHARDED=True)
    if pair_stats is not None:
        it.PAIR_STATS = pair_stats
    cfg = ns(NUM_GPUS=1, OUTPUT_PATH=out, DATASET=ns(POSITIVE_SAMPLING_P=0.2), ITERCLUSTER=it)
    labels, nmi = iterative_cluster_step(None, cfg, torch.nn.Identity(), Loader(x, y), epoch=3, cuda=False, device="cpu", **kw)
    files = {}
    for d, _, names in os.walk(out):
        for n in names:
            files[os.path.relpath(os.path.join(d, n), out)] = open(os.path.join(d, n)).read()
    return labels, nmi, files


def run_step_recorded(out, pair_stats=None, pairstats_kernels=None):
    """the recorded form of a step on step_inputs() with the NumPy DBSCAN and NMI / AMI providers:
    {'calls', 'stdout', 'files', 'labels', 'nmi'}"""
    from cluster_metrics_cpu_kernels import NumpyClusterMetricsKernels
    from dbscan_cpu_kernels import NumpyDbscanKernels
    x, y = step_inputs()
    y = y.copy()
    y[-3:] = -1                                                 # three rows without a true label
    calls = []
    kw = dict(kmeans_kernels=Recorded(NumpyDbscanKernels(), "dbscan", calls),
              metrics_kernels=Recorded(NumpyClusterMetricsKernels(), "metrics", calls))
    if pairstats_kernels is not None:
        kw["pairstats_kernels"] = Recorded(pairstats_kernels, "pairstats", calls)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        labels, nmi, files = run_step(out, x, y, pair_stats=pair_stats, **kw)
    return {"calls": calls, "stdout": normalise_step_output(buf.getvalue(), out),
            "files": {k: normalise_step_output(v, out) for k, v in sorted(files.items())},
            "labels": [int(v) for v in labels], "nmi": float(nmi)}

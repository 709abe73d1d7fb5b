"""The rows the device k-means++ seeding picks, against tests/golden/kmeanspp_picks.npz (recorded from the library by
tests/golden/make_goldens_kmeanspp.py, which documents the cases): equal pick for pick on both distance paths, on blobs and on
unstructured data where the last bits of the sums decide, and every lock-step run equal to the single run from its first row."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "make_goldens_kmeanspp", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_goldens_kmeanspp.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "kmeanspp_picks.npz")))


def _inputs(golden, n, *case):
    X, T, u = mg.inputs(*case)
    assert np.array_equal(golden[n + "__sums"], [X.sum(dtype=np.float64), u.sum()]), "the generator's inputs drifted"
    return X, T, u


@pytest.mark.parametrize("kind", mg.KINDS)
@pytest.mark.parametrize("N,D,K", mg.SINGLE)
def test_single_run_picks(gpu, golden, N, D, K, kind):
    n = mg.name(N, D, K, kind)
    X, T, u = _inputs(golden, n, N, D, K, kind)
    dev = mg.Device(X)
    for path in ("valu", "mfma"):
        got = dev.single(mg.first_of(N), K, T, u, mfma=(path == "mfma"))
        assert got[0] == mg.first_of(N)
        assert np.array_equal(got, golden[n + "__" + path]), (path, int((got != golden[n + "__" + path]).sum()))


@pytest.mark.parametrize("kind", mg.KINDS)
@pytest.mark.parametrize("N,D,K,R", mg.BATCH)
def test_lock_step_picks(gpu, golden, N, D, K, R, kind):
    n = mg.name(N, D, K, kind, R)
    X, T, u = _inputs(golden, n, N, D, K, kind, R)
    dev = mg.Device(X)
    firsts = [mg.first_of(N, r) for r in range(R)]
    got = dev.batch(firsts, K, T, u)
    assert got.shape == (R, K)
    assert np.array_equal(got, golden[n + "__picks"]), int((got != golden[n + "__picks"]).sum())
    for r in range(R):                                              # run r == the single matrix-pipe run from firsts[r] with uniforms[r]
        assert np.array_equal(got[r], dev.single(firsts[r], K, T, u[r], mfma=True)), r

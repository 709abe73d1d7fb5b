"""GPU: pair_statistics on a workspace of EXACTLY slic_pair_stats_workspace_bytes(...) — guarded on both sides, poisoned inside with
0x00 and then 0xFF (tests/ws_guard.py), in the manner of test_workspace_contract_gpu.py: every guard byte intact, one request under the
tag `pair_stats` of the size the query returns, the two runs bit-equal (as test_pair_stats_gpu.test_two_calls_are_bit_equal asserts run
to run) and the 0xFF run held to the oracle under test_pair_stats_gpu's own checks."""
import numpy as np
import pytest

from ws_guard import run_both

pytestmark = pytest.mark.gpu


# (Nx, Ny or None, D, bins): one workgroup; ragged tiles of both sides; two slices of gallery tiles; the widest rows and table
CASES = [(1, None, 8, 8), (129, None, 20, 256), (2200, None, 8, 64), (130, 300, 40, 4096), (130, None, 512, 64)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "{}x{}_d{}_b{}".format(*c))
def test_pair_statistics_on_an_exact_workspace(gpu, monkeypatch, case):
    from pair_stats_cases import clustered_rows
    from pair_stats_cpu_kernels import pair_stats_fp64
    from test_pair_stats_gpu import check_sandwich, check_sums
    from test_workspace_contract_gpu import _only
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.pairstats import pair_statistics
    nx, ny, D, bins = case
    x, lx = clustered_rows(nx, D, 50 + nx)
    y, ly = (None, None) if ny is None else clustered_rows(ny, D, 60 + ny)
    want = _lib.load().slic_pair_stats_workspace_bytes(nx, ny or 0, D, bins)
    assert want > 0

    def run():
        st = pair_statistics(x, lx, y, ly, bins=bins)
        return np.stack([st["hist_diff"], st["hist_same"]]), st["record"]

    (a, wa), (b, wb) = run_both(monkeypatch, run)
    for ws in (wa, wb):
        _only(ws, "pair_stats", want)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    o = pair_stats_fp64(x, lx, y, ly, bins=bins)
    hist, rec = b
    assert rec[0] == o["record"][0] and rec[1] == o["record"][1] and rec[8] == 0
    what = "exact workspace {}".format(case)
    check_sandwich(hist, o, D, bins, what)
    if rec[0] + rec[1] > 0:
        check_sums(rec, o, D, 2.0, what)

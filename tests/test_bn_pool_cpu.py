"""CPU: the NumPy mirror of csrc/bn.hip (tests/bn_cpu_kernels.py) against float64 / torch's CPU kernels, the cases and gates of
tests/test_bn_pool_gpu.py run with the mirror in the device's place, the mutation table, and the host-side argument rules of the
bn.hip entry points (the library loads without a device).

Mutation table.  Each defect is switched on in the mirror alone, one at a time, and the GPU module's own check functions are run
on the mutated mirror: the listed case must raise (test_mutation_is_caught), and the unmutated mirror passes every one of them
(test_gpu_cases_pass_on_the_mirror), so each gate is both reachable in float32 and tight enough to see the defect.

  mutation       defect                                                   caught by (tests/test_bn_pool_gpu.py)              gate that breaks
  ragged_full    ragged last slab row counted as full                     check_stats R=17 rows=4 last=1 narrow              invstd (ulps)
  chain_order    sub-chains merged 0, 3, 2, 1                             check_row_order                                    mean == 1/64 exactly
  no_guard       `n_b > 0` guard removed                                  check_sync W=3, all-zero row with n = 0            finite outputs (0 / 0 -> NaN)
  swap_var       unbiased variance in invstd, biased in running_var       check_stats R=16 rows=4 last=3                     invstd (ulps), running_var
  swap_momentum  (1 - momentum) and momentum exchanged                    check_stats R=16 (running stats start non-trivial) running_mean / running_var
  rows_l         a level's rows_l not multiplied by 64                    check_stats R=65 rows=128 last=1 narrow            invstd (ulps)
  skip_tail      pass 1 drops the rows left after the unrolled loop       check_bwd M=700 C=8, integer data                  dgamma / dbeta bit-equality
  ge             `>=` in the ReLU mask and the max-pool comparison        check_bwd M=3 C=48 integer data; check_maxpool     g bit-equality; arg == torch's index
  border_clamp   border window position read clamped, not skipped         check_maxpool (5, 6, 9) C=3                        arg == torch's index
  stride_2axes   shortcut 'A' strides t and h only                        check_shortcut (2, 3, 7) stride 2                  bit-equality

Two remarks the table owes.  (1) Chan's merge is symmetric: merging the sub-chains in another order changes M2 in its last double
bits only (measured here: 2e-14 relative at most on the narrow data), which no float32 output can show, and the running `sum` is exact for any data a conv
epilogue emits.  What the order does decide is the documented contract "added in workgroup order, in double", and check_row_order
states it with sums whose double total is 1 in row order and 0 with a later chain first.  Inside the tree the `n_b > 0` guard is
arithmetically idle (chain 0 is never empty, and an empty chain adds d d n 0 / nn = 0); where it decides anything is the rank-order
merge, whose first row may have n = 0.  (2) For a window of 3, stride 2, padding 1 the clamped coordinate is always inside the
window already, so a kernel that clamps the coordinate and derives `arg` from the clamped one is correct; the defect is reading at
the clamped coordinate while `arg` is formed from the window's own coordinate, and the first-maximum rule then reports a position
outside the input."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_cpu_kernels as K
import test_bn_pool_gpu as G

F32 = np.float32


class Mirror:
    """tests/bn_cpu_kernels.py behind the interface of test_bn_pool_gpu.Device"""

    def __init__(self, *mut):
        self.mut = frozenset(mut)

    def finalize(self, slab, rows, M, eps, mom, gamma, beta, rm, rv):
        return K.bn_finalize(slab, rows, M, eps, mom, gamma, beta, rm, rv, self.mut)

    def merge_stats(self, slab, rows, M):
        return K.bn_merge_stats(slab, rows, M, self.mut)

    def finalize_sync(self, stats, C, eps, mom, gamma, beta, rm, rv):
        return K.bn_finalize_sync(stats, C, eps, mom, gamma, beta, rm, rv, self.mut)

    def bwd(self, dy, out, z, mean, invstd, gamma, g_given):
        g, dz, dg, db = K.bn_bwd(dy, out, z, mean, invstd, gamma, self.mut)
        return (g.copy() if g_given else None), dz, dg, db

    def bwd_sums(self, partial, dy, out, z, mean, invstd, M, C):
        g = None
        if partial is None:
            g, partial = K.bn_bwd_pass1(dy, out, z, mean, invstd, self.mut)
            g = g if out is not None else None
        a, b = K.sum_tree(partial)
        return g, np.concatenate([a, b]), b.astype(F32), a.astype(F32)

    def bwd_apply(self, g, z, mean, invstd, gamma, ka, kb):
        return K.bn_bwd_pass2(g, z, mean, invstd, gamma, ka, kb)

    def bwd_fused(self, partial, g, z, mean, invstd, gamma):
        a, b = K.sum_tree(partial)
        M = g.shape[0]
        return K.bn_bwd_pass2(g, z, mean, invstd, gamma, a / float(M), b / float(M)), b.astype(F32), a.astype(F32)

    def maxpool_fwd(self, x, with_arg=True):
        return K.maxpool3d_fwd(x, self.mut)

    def maxpool_bwd(self, dy, arg, dims):
        return K.maxpool3d_bwd(dy, arg, dims)

    def shortcut_a(self, x, stride, C_out):
        return K.shortcut_a(x, stride, C_out, self.mut)


STAT_IDS = [f"R{c[0]}-rows{c[1]}-C{c[2]}-last{c[3]}-{c[4]}" for c in G.STAT_CASES]


# ------------------------------------------------------------------ mirror against float64 / torch
@pytest.mark.parametrize("case", G.STAT_CASES, ids=STAT_IDS)
def test_mirror_tree_equals_flat_float64(case):
    """chained (tree) and flat forms of the same float64 sums of non-negative terms: mean and biased variance within 1e-12
    relative (measured: 4e-14 in variance at M = 16387, rows = 4, narrow data)"""
    R, rows, C, last, kind = case[:5]
    slab, M = G.make_slab(R, rows, C, last, kind)
    st = K.bn_merge_stats(slab, rows, M)
    mean, m2 = K.flat_stats(slab, rows, M)
    assert np.all(np.abs(st[:C] / M - mean) <= 1e-12 * np.abs(mean))
    assert np.all(np.abs(st[C:] - m2) <= 1e-12 * m2 + 1e-300)


def test_mirror_tree_on_the_measured_case():
    rng = np.random.default_rng(0)
    rows, M, C = 4, 16387, 8
    x = (100 + 0.05 * rng.standard_normal((M, C))).astype(F32).astype(np.float64)
    R = -(-M // rows)
    slab = np.zeros((R, 2, C))
    for r in range(R):
        b = x[r * rows:(r + 1) * rows]
        slab[r] = b.sum(0), ((b - b.mean(0)) ** 2).sum(0)
    slab = slab.astype(F32)
    st = K.bn_merge_stats(slab, rows, M)
    mean, m2 = K.flat_stats(slab, rows, M)
    assert np.abs(st[C:] / m2 - 1).max() < 1e-12 and np.abs(st[:C] / M / mean - 1).max() < 1e-12
    # ... and the float32 slab itself carries the variance of the data: 0.05^2 within the sampling error and the slab's rounding
    assert np.abs(m2 / M / x.var(0) - 1).max() < 1e-3


@pytest.mark.parametrize("dims", G.POOL_DIMS)
@pytest.mark.parametrize("C", [3, 8])
def test_mirror_maxpool_equals_torch(dims, C):
    """values bit-equal, indices equal, the gather-form backward bit-equal to autograd for integer-valued dy"""
    G.check_maxpool(Mirror(), dims, C)


@pytest.mark.parametrize("dims", G.POOL_DIMS)
@pytest.mark.parametrize("C,stride,wide", [(3, 1, 1), (3, 2, 2), (8, 2, 1)])
def test_mirror_shortcut_equals_torch(dims, C, stride, wide):
    G.check_shortcut(Mirror(), dims, C, stride, C * wide)


@pytest.mark.parametrize("M,C", [(77, 8), (1031, 48), (300, 2048), (8321, 200)])
def test_mirror_backward_equals_autograd(M, C):
    """float64 autograd of relu(batch_norm(z) + res), at the gates of test_bn_train_fwd_bwd"""
    rng = np.random.default_rng(4)
    z = torch.from_numpy((rng.standard_normal((M, C)) * 2 + 0.5).astype(F32))
    gam = torch.from_numpy((1 + 0.1 * rng.standard_normal(C)).astype(F32))
    bet = torch.from_numpy((0.1 * rng.standard_normal(C)).astype(F32))
    res = torch.from_numpy(rng.standard_normal((M, C)).astype(F32))
    dy = torch.from_numpy(rng.standard_normal((M, C)).astype(F32))
    z64 = z.double().requires_grad_(True)
    g64, b64, r64 = gam.double().requires_grad_(True), bet.double().requires_grad_(True), res.double().requires_grad_(True)
    y64 = F.relu(F.batch_norm(z64, None, None, g64, b64, True, 0.1, 1e-5) + r64)
    gz, gg, gb, gr = torch.autograd.grad(y64, [z64, g64, b64, r64], dy.double())
    R = (M + 127) // 128
    xp = np.zeros((R * 128, C))
    xp[:M] = z.numpy()
    n = np.minimum(128, M - 128 * np.arange(R))[:, None].astype(np.float64)
    s = xp.reshape(R, 128, C).sum(1)
    live = (np.arange(128)[None, :] < n)[:, :, None]
    m2 = (((xp.reshape(R, 128, C) - (s / n)[:, None]) ** 2) * live).sum(1)
    st = K.bn_finalize(np.stack([s, m2], 1).astype(F32), 128, M, 1e-5, 0.1, gam.numpy(), bet.numpy())
    y = np.maximum(z.numpy() * st["scale"] + st["shift"] + res.numpy(), F32(0))
    assert np.abs(y - y64.detach().numpy()).max() < 2e-5
    g, dz, dg, db = K.bn_bwd(dy.numpy(), y, z.numpy(), st["mean"], st["invstd"], gam.numpy())
    assert np.abs(g - gr.numpy()).max() < 1e-6
    assert np.abs(dz - gz.numpy()).max() < 2e-5 * max(1.0, gz.abs().max().item())
    assert np.abs(dg - gg.numpy()).max() < 1e-4 * max(1.0, gg.abs().max().item())
    assert np.abs(db - gb.numpy()).max() < 1e-4 * max(1.0, gb.abs().max().item())


# ------------------------------------------------------------------ the GPU module's cases on the mirror
@pytest.mark.parametrize("case", G.STAT_CASES, ids=STAT_IDS)
def test_gpu_statistics_cases_pass_on_the_mirror(case):
    G.check_stats(Mirror(), case)


def test_gpu_cases_pass_on_the_mirror():
    m = Mirror()
    G.check_stats_single_sample(m)
    G.check_row_order(m)
    for W, zero_at in [(1, 0), (3, 1), (8, -1)]:
        G.check_sync(m, W, zero_at)
    for M, C in G.BWD_SHAPES:
        G.check_bwd(m, M, C, True)
        G.check_bwd(m, M, C, False)
    for R, L, C in G.FUSED_SHAPES:
        G.check_bwd_slab(m, R, L, C, True)
        G.check_bwd_slab(m, R, L, C, False)
    for M in (2, 3, 4):
        for C in (512, 2048):
            G.check_bwd_small_batch(m, M, C)


def _stat_case(R, rows):
    return next(c for c in G.STAT_CASES if c[0] == R and c[1] == rows)


MUTATIONS = [
    ("ragged_full", "stats", lambda m: G.check_stats(m, _stat_case(17, 4))),
    ("chain_order", "row-order", lambda m: G.check_row_order(m)),
    ("no_guard", "sync", lambda m: G.check_sync(m, 3, 1)),
    ("swap_var", "stats", lambda m: G.check_stats(m, _stat_case(16, 4))),
    ("swap_momentum", "stats", lambda m: G.check_stats(m, _stat_case(16, 4))),
    ("rows_l", "stats", lambda m: G.check_stats(m, _stat_case(65, 128))),
    ("skip_tail", "bwd", lambda m: G.check_bwd(m, 700, 8, True)),
    ("ge", "relu-mask", lambda m: G.check_bwd(m, 3, 48, True)),
    ("ge", "maxpool", lambda m: G.check_maxpool(m, (5, 6, 9), 3)),
    ("border_clamp", "maxpool", lambda m: G.check_maxpool(m, (5, 6, 9), 3)),
    ("stride_2axes", "shortcut", lambda m: G.check_shortcut(m, (2, 3, 7), 3, 2, 6)),
]


@pytest.mark.parametrize("mut,where,case", MUTATIONS, ids=[f"{m}-{w}" for m, w, _ in MUTATIONS])
def test_mutation_is_caught(mut, where, case):
    case(Mirror())                                        # the case passes on the mirror as it is ...
    with pytest.raises(AssertionError):                   # ... and fails with the one defect
        case(Mirror(mut))


@pytest.mark.parametrize("name,M,C", [("skip_tail", 257, 48), ("skip_tail", 700, 200), ("skip_tail", 259, 1024), ("ge", 700, 64)])
def test_backward_mutations_are_caught_at_other_shapes(name, M, C):
    with pytest.raises(AssertionError):
        G.check_bwd(Mirror(name), M, C, True)


# ------------------------------------------------------------------ host argument rules (no device needed)
def test_host_argument_rules():
    from video_similarity_search_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                 # never read: every call below is refused before any launch

    def refused(name, *args):
        assert getattr(lib, name)(*args, None) != 0, name
        assert name.encode() in lib.slic_last_error(), (name, lib.slic_last_error())

    # R rows of `rows` samples must cover M, and the last row must not be empty
    for R, rows, M in [(3, 4, 13), (3, 4, 8), (1, 4, 5), (2, 1, 1)]:
        refused("slic_bn_finalize", p, R, rows, 8, M, 1e-5, 0.1, p, p, p, p, p, p, p, p, p)
        refused("slic_bn_merge_stats", p, R, rows, 8, M, p, p)
    # running statistics come in pairs
    refused("slic_bn_finalize", p, 3, 4, 8, 12, 1e-5, 0.1, p, p, p, p, p, p, p, None, p)
    refused("slic_bn_finalize", p, 3, 4, 8, 12, 1e-5, 0.1, p, p, p, p, p, p, None, p, p)
    refused("slic_bn_finalize_sync", p, 2, 8, 1e-5, 0.1, p, p, p, p, p, p, p, None)
    refused("slic_bn_finalize_sync", p, 2, 8, 1e-5, 0.1, p, p, p, p, p, p, None, p)
    # C % 4 == 0
    for C in (6, 1, 2047):
        refused("slic_bn_apply", p, p, p, p, 1, 4, C, p)
        refused("slic_bn_bwd", p, p, p, p, p, p, 4, C, p, p, p, p, p)
        refused("slic_bn_bwd_sums", None, 0, p, p, p, p, p, 4, C, p, p, p, p, p)
        refused("slic_bn_bwd_apply", p, p, p, p, p, p, p, 4, C, p)
        refused("slic_bn_bwd_fused", p, 1, p, p, p, p, p, 4, C, p, p, p, p)
        refused("slic_avgpool_fwd", p, 2, 3, C, p)
        refused("slic_avgpool_bwd", p, 2, 3, C, p)
    # slic_bn_bwd_sums: neither a slab nor dy / z / mean / invstd; a ReLU mask without a place for the masked gradient
    refused("slic_bn_bwd_sums", None, 0, None, None, None, None, None, 4, 8, None, p, p, p, p)
    refused("slic_bn_bwd_sums", None, 0, p, None, p, p, None, 4, 8, None, p, p, p, p)
    refused("slic_bn_bwd_sums", p, 0, None, None, None, None, None, 4, 8, None, p, p, p, p)
    refused("slic_bn_bwd_sums", None, 0, p, p, p, p, p, 4, 8, None, p, p, p, p)
    # arg is an int32 position
    refused("slic_maxpool3d_fwd", p, 1, 2048, 1024, 1024, 1, p, p)
    refused("slic_maxpool3d_fwd", p, 1, 1 << 11, 1 << 10, 1 << 10, 4, p, None)
    # shortcut 'A'
    refused("slic_shortcut_a", p, 1, 2, 2, 2, 4, 0, 8, p)
    refused("slic_shortcut_a", p, 1, 2, 2, 2, 8, 2, 4, p)
    assert lib.slic_bn_bwd_rows_per_partial() == K.BNB_RB

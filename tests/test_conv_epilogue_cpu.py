"""No GPU: the float64 reference of the gather-GEMM epilogue (tests/conv_epilogue_ref.py) against float64 torch, and the properties of
its cases that test_conv_epilogue_gpu.py leans on — every quantity it compares bit for bit IS a float32 number whatever the order of the
additions, the one inexact quantity (sum (v - mean_blk)^2) stays inside its derived bound in a float32 evaluation, and no case is
trivial (ReLU and mask each act on 25 % .. 75 % of the elements, no statistic or backward-sum column is all zero)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_epilogue_ref as R

FWD_CASES = sorted({(C, M, N, R.TILE_M[v]) for v, C in R.KERNEL_C.items() for M, N, _ in R.SHAPES} |
                   {(R.TAIL_C, M, N, t) for M, N, _ in R.TAIL_SHAPES for t in (64, 128)})
DGRAD_CASES = [(kind, nout) for kind in R.DGRAD_KINDS for nout in (32, 16)]


def _t(a):
    return torch.from_numpy(R.f64(a))


def test_shape_list_covers_what_it_promises():
    pairs = {(M, N) for M, N, _ in R.SHAPES}
    assert all(sum((M, N) in pairs for N in R.NS) >= 2 for M in R.MS)
    assert all(sum((M, N) in pairs for M in R.MS) >= 2 for N in R.NS)
    wide = {(M, N) for M, N, ldo in R.SHAPES if ldo == N + 12}
    assert len(wide) == 3 and all((M, N, N) in R.SHAPES for M, N in wide)
    assert len(R.OPERAND_SETS) == 17 and len({n for n, _ in R.OPERAND_SETS}) == 17


@pytest.mark.parametrize("C,M,N,tile_m", [(16, 65, 36, 64), (64, 129, 68, 128), (32, 581, 132, 64)])
def test_reference_matches_torch_forward(C, M, N, tile_m):
    """F.linear and a 1x1x1 F.conv3d + affine + residual + ReLU, and the block statistics as torch's sum / biased variance"""
    c = R.make_case(C, M, N)
    out, stat, _ = R.case_ref(c, ("stat",) + R.ALL5, tile_m)
    x, W, b = _t(c["x"]), _t(c["W"]), _t(c["bias"])
    lin = F.linear(x, W, b)
    conv = F.conv3d(x.t().reshape(1, C, M, 1, 1), W.reshape(N, C, 1, 1, 1), b).reshape(N, M).t()
    assert torch.equal(lin, conv)
    want = F.relu(lin * _t(c["scale"]) + _t(c["shift"]) + _t(c["addend"]))
    assert np.array_equal(out, want.numpy())
    for i, r0 in enumerate(range(0, M, tile_m)):
        blk = lin[r0:r0 + tile_m]
        assert np.array_equal(stat[i, 0], blk.sum(0).numpy())
        assert np.allclose(stat[i, 1], (blk.var(0, unbiased=False) * blk.shape[0]).numpy(), rtol=1e-12, atol=1e-12)
    # the statistics are those of acc + bias: the other operands do not move them
    assert np.array_equal(stat, R.case_ref(c, ("stat", "bias"), tile_m)[1])


@pytest.mark.parametrize("kind,nout", DGRAD_CASES)
def test_reference_matches_torch_data_gradient(kind, nout):
    """conv_transpose3d + addend + where(mask > 0) and the two column sums: the slab rows of all classes and blocks add up to them (in
    float64 these sums of small binary fractions are exact, so equality is exact)"""
    c = R.dgrad_case(kind, nout)
    dx, slab = R.dgrad_ref(c, True)
    x64 = _t(np.zeros((c["B"], c["cin"]) + c["dims"])).requires_grad_(True)
    y = F.conv3d(x64, _t(c["W"]), None, 2, c["pad"])
    g, = torch.autograd.grad(y, [x64], _t(c["dz"]).permute(0, 4, 1, 2, 3))
    full = g.permute(0, 2, 3, 4, 1).reshape(-1, c["cin"])
    assert np.array_equal(c["full"], full.numpy()), "conv_transpose3d is not the gradient of conv3d"
    want = torch.where(_t(c["mask"]) > 0, full + _t(c["addend"]), torch.zeros_like(full))
    assert np.array_equal(dx, want.numpy())
    xhat = (_t(c["z"]) - _t(c["mean"])) * _t(c["invstd"])
    assert np.array_equal(slab[:, 0].sum(0), want.sum(0).numpy())
    assert np.array_equal(slab[:, 1].sum(0), (want * xhat).sum(0).numpy())
    plain, none = R.dgrad_ref(c, False)
    assert none is None and np.array_equal(plain, full.numpy())
    # launch order and class geometry: eight classes of unequal grids that tile the positions (dgrad_ref asserts the cover)
    assert len(c["classes"]) == 8 and len({dc["grid"] for dc in c["classes"]}) == 8
    assert [dc["nchunks"] for dc in c["classes"]] == sorted((dc["nchunks"] for dc in c["classes"]), reverse=True)
    assert sum(dc["ntaps"] == 0 for dc in c["classes"]) == (7 if kind == "1x1x1" else 0)


def _assert_exact(trace, what):
    for name, a in trace["pointwise"]:
        assert R.is_f32(a), f"{what}: '{name}' is not a float32 number"
    for name, terms, starts in trace["sums"]:
        assert R.sums_exact(terms, starts), f"{what}: a partial sum of '{name}' may round in float32"


@pytest.mark.parametrize("C", sorted({c[0] for c in FWD_CASES}))
def test_forward_cases_are_exact_in_float32_and_not_trivial(C):
    for C_, M, N, tile_m in FWD_CASES:
        if C_ != C:
            continue
        c = R.make_case(C, M, N)
        assert R.caps_violations(c, tile_m) == [], (C, M, N, tile_m)
        assert (np.abs(c["acc"]) % 2 == 1).all(), "acc is a sum of an odd number of +-1"
        off = c["mask"][~(c["mask"] > 0)]
        if off.size >= 64:
            assert np.isnan(off).any() and (off < 0).any() and (np.signbit(off) & (off == 0)).any() and (~np.signbit(off) & (off == 0)).any()
        for name, ops in R.OPERAND_SETS:
            tr = {}
            R.case_ref(c, ops, tile_m, tr)
            _assert_exact(tr, f"C={C} M={M} N={N} tile {tile_m} {name}")


@pytest.mark.parametrize("kind,nout", DGRAD_CASES)
def test_data_gradient_cases_are_exact_in_float32_and_not_trivial(kind, nout):
    c = R.dgrad_case(kind, nout)
    assert R.dgrad_caps_violations(c) == []
    for fused in (True, False):
        traces = []
        R.dgrad_ref(c, fused, traces)
        for dc, tr in zip(c["classes"], traces):
            _assert_exact(tr, f"{kind} {nout} class {dc['cls']} fused={fused}")


@pytest.mark.parametrize("C", sorted({c[0] for c in FWD_CASES}))
def test_m2_bound_holds_in_float32(C):
    """a float32 evaluation of the kernel's two-pass formula stays inside m2_bound for every case, with and without the bias (the bound
    is derived in conv_epilogue_ref.py; this shows the factor there did not have to be widened)"""
    worst = 0.0
    for C_, M, N, tile_m in FWD_CASES:
        if C_ != C:
            continue
        c = R.make_case(C, M, N)
        _, cnt = R.block_starts(M, tile_m)
        for ops in (("stat",), ("stat", "bias")):
            ref = R.case_ref(c, ops, tile_m)[1][:, 1]
            got = R.m2_float32(c["acc"] + (c["bias"] if "bias" in ops else 0.0), tile_m).astype(np.float64)
            bound = R.m2_bound(cnt[:, None], ref)
            assert (np.abs(got - ref) <= bound).all(), (C, M, N, tile_m, ops)
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, np.nanmax(np.where(ref > 0, np.abs(got - ref) / ((cnt[:, None] + 8.0) * 2.0 ** -24 * ref), 0.0)))
    print(f"C = {C}: largest |float32 - float64| / ((rows + 8) 2^-24 ref) = {worst:.3f} (allowed: {R.M2_FACTOR})")
    assert worst <= R.M2_FACTOR

"""The references of tests/conv_operand_ref.py and the host tables of models/conv_plan.py mean what they say (no GPU): the gather-GEMM
emulated in float64 from nothing but the documented operands — chunk / tap tables, packed weights, transposed clips, Winograd operands —
equals F.conv3d and its autograd in float64 on float32-valued inputs.  Both sides work in float64 on at most 1372 products per output,
so the tolerance is 1e-10 * max(1, max |ref|): far below any float32 effect, far above float64 rounding.

test_conv_operands_gpu.py then compares the device entry points with the same references."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_operand_ref as R
from video_similarity_search_amd.models.conv_plan import ConvPlan

B = 2
# (C, N, kernel, stride, pad, dims, wrun)
FWD_CASES = [
    (3, 8, (7, 7, 7), (1, 2, 2), (3, 3, 3), (4, 9, 10), False),
    (3, 8, (7, 7, 7), (1, 2, 2), (3, 3, 3), (4, 9, 10), True),
    (2, 8, (3, 7, 7), (1, 2, 2), (1, 3, 3), (3, 7, 9), True),
    (3, 16, (3, 5, 3), (1, 1, 1), (1, 2, 1), (2, 5, 6), True),
    (8, 16, (3, 3, 3), (2, 2, 2), (1, 1, 1), (5, 7, 6), False),
    (8, 16, (1, 1, 1), (2, 2, 2), (0, 0, 0), (4, 5, 6), False),
    (32, 32, (3, 3, 3), (1, 1, 1), (1, 1, 1), (2, 3, 5), False),
]
DGRAD_CASES = [c for c in FWD_CASES if not c[6]]


def _close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(got, np.float64) - ref).max()
    assert err <= 1e-10 * max(1.0, np.abs(ref).max()), f"{what}: max error {err:.3e}"


_CONV = {}


def _conv(C, N, k, s, p, dims):
    """(x, w, dy float32 numpy; y, dx float64 numpy, channels-first) of one case — computed once, never modified"""
    key = (C, N, k, s, p, dims)
    if key not in _CONV:
        rng = np.random.default_rng(1000 * C + N + sum(dims))
        x = rng.standard_normal((B, C) + dims).astype(np.float32)
        w = (rng.standard_normal((N, C) + k) / np.sqrt(C * np.prod(k))).astype(np.float32)
        x64 = torch.from_numpy(x).double().requires_grad_(True)
        y64 = F.conv3d(x64, torch.from_numpy(w).double(), None, s, p)
        dy = rng.standard_normal(tuple(y64.shape)).astype(np.float32)
        dx64, = torch.autograd.grad(y64, [x64], torch.from_numpy(dy).double())
        out = (x, w, dy, y64.detach().numpy(), dx64.numpy())
        for a in out:
            a.setflags(write=False)
        _CONV[key] = out
    return _CONV[key]


def _cl(a):
    """channels-first [B, C, T, H, W] -> channels-last [B, T, H, W, C]"""
    return np.ascontiguousarray(np.einsum("bcthw->bthwc", a))


def _forward(case, taps=False, mutate=None):
    C, N, k, s, p, dims, wrun = case
    x, w, _, y, _ = _conv(C, N, k, s, p, dims)
    plan = ConvPlan(C, N, k, s, p, dims, "cpu", wrun=wrun, wino=False)
    assert plan.wrun == wrun
    T, H, W = dims
    if wrun:
        src = R.ref_ncdhw_to_ndhwc_wpad(x.reshape(B, C, T * H, W), p[2], plan.src_dims[2])
        wp = R.ref_pack_fwd_runs(w, plan.run_len, plan.run_px, plan.Kp)
    else:
        src = R.ref_ncdhw_to_ndhwc(x.reshape(B, C, T * H * W), plan.Cs)
        wp = R.ref_pack_fwd(w, plan.Cs, plan.Kp, 0.0)
    g = R.fwd_geometry(plan, B)
    assert src.size == B * g.Ts * g.Hs * g.Ws * g.Cs
    if mutate is not None:
        g.tab, wp = g.tab.copy(), wp.copy()
        g.tap_tab = None if g.tap_tab is None else g.tap_tab.copy()
        mutate(g, wp)
    dst = (R.emulate_gemm_taps if taps else R.emulate_gemm)(g, src, wp)
    assert dst.shape == (g.M, N) and not np.isnan(dst).any()
    _close(dst.reshape((B,) + plan.out_dims + (N,)), _cl(y), f"forward {case}")


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_from_chunk_table(case):
    _forward(case)


def test_forward_from_tap_table():
    _forward(FWD_CASES[6], taps=True)


def _dgrad(case, taps=False, mutate=None):
    C, N, k, s, p, dims, _ = case
    _, w, dy, _, dx = _conv(C, N, k, s, p, dims)
    plan = ConvPlan(C, N, k, s, p, dims, "cpu", wrun=False, wino=False)
    wd = R.ref_pack_dgrad(w, plan.Cs, plan.Kd, 0.0)
    src = _cl(dy)
    T, H, W = dims
    dst = np.full((B * T * H * W, plan.Cs), np.nan)
    hits = np.zeros(B * T * H * W, np.int64)
    ran = 0
    for dc in plan.dgrad_classes:
        g = R.dgrad_geometry(plan, dc, B)
        if taps:
            if g.tap_tab is None:
                continue
            R.emulate_gemm_taps(g, src, wd, dst, hits)
        else:
            if mutate is not None:
                g.tab = g.tab.copy()
                mutate(g)
            R.emulate_gemm(g, src, wd, dst, hits)
        ran += 1
    assert ran > 0
    if not taps or ran == len(plan.dgrad_classes):
        assert (hits == 1).all(), "every element of dx must be written exactly once"
    ref = np.zeros((B, T, H, W, plan.Cs))
    ref[..., :C] = _cl(dx)
    got = dst.reshape(ref.shape)
    written = hits.reshape(B, T, H, W) > 0
    _close(got[written], ref[written], f"dgrad {case}")
    return ran


@pytest.mark.parametrize("case", DGRAD_CASES)
def test_dgrad_parity_classes_cover_dx_once(case):
    n = _dgrad(case)
    assert n == (8 if case[3] == (2, 2, 2) else 4 if case[3] == (1, 2, 2) else 1)


def test_dgrad_from_tap_tables():
    assert _dgrad(FWD_CASES[6], taps=True) == 1


# ---- Winograd -----------------------------------------------------------------------------------------------------------------------
WINO_DIMS = [(2, 3, 7), (3, 2, 8)]
WINO2_DIMS = [(2, 4, 8), (2, 5, 7), (1, 1, 1)]


@pytest.mark.parametrize("dims", WINO_DIMS + WINO2_DIMS)
@pytest.mark.parametrize("C,N,dgrad", [(8, 64, 0), (64, 64, 0), (64, 8, 1)])
def test_winograd_operands_give_the_convolution(C, N, dgrad, dims):
    x, w, dy, y, dx = _conv(C, N, (3, 3, 3), (1, 1, 1), (1, 1, 1), dims)
    src, ref = (_cl(dy), _cl(dx)) if dgrad else (_cl(x), _cl(y))
    if dims in WINO_DIMS:
        U, bound = R.ref_pack_wino(w, dgrad)
        got = R.emulate_wino(U, src)
    else:
        U, bound = R.ref_pack_wino2(w, dgrad)
        got = R.emulate_wino2(U, src)
    assert U.shape == bound.shape and (np.abs(U) <= bound * (1 + 1e-12)).all()
    _close(got, ref, f"winograd C={C} N={N} dgrad={dgrad} dims={dims}")


# ---- tables against brute force -----------------------------------------------------------------------------------------------------
def _row_geometries():
    mk = lambda C, N, k, s, p, dims, wrun, b: R.fwd_geometry(ConvPlan(C, N, k, s, p, dims, "cpu", wrun=wrun, wino=False), b)
    out = [mk(8, 8, (3, 3, 3), (1, 1, 1), (1, 1, 1), (3, 5, 7), False, 2),
           mk(8, 16, (3, 3, 3), (2, 2, 2), (1, 1, 1), (5, 7, 9), False, 2),
           mk(8, 8, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), False, 5),
           mk(8, 8, (3, 3, 3), (1, 1, 1), (1, 1, 1), (2, 4, 1), False, 2),
           mk(3, 8, (7, 7, 7), (1, 2, 2), (3, 3, 3), (4, 9, 10), True, 2)]
    plan = ConvPlan(8, 16, (3, 3, 3), (2, 2, 2), (1, 1, 1), (5, 7, 9), "cpu", wrun=False, wino=False)
    out.append(R.dgrad_geometry(plan, plan.dgrad_classes[3], 2))
    return out


def test_row_table_bits_against_brute_force():
    for g in _row_geometries():
        tab = R.ref_row_table(g)
        assert tab.dtype == np.uint32 and tab.shape == (g.M, 2)
        m = 0
        for b in range(g.M // (g.Ga * g.Gb * g.Gc)):
            for ga, gb, gc in itertools.product(range(g.Ga), range(g.Gb), range(g.Gc)):
                co = (ga * g.sa, gb * g.sb, gc * g.sc)
                pixel = ((b * g.Ts + co[0]) * g.Hs + co[1]) * g.Ws + co[2]
                assert int(tab[m, 0]) == pixel * g.Cs * 4
                for dim, size in enumerate((g.Ts, g.Hs, g.Ws)):
                    for o in range(-3, 4):
                        assert bool(int(tab[m, 1]) >> (7 * dim + o + 3) & 1) == (0 <= co[dim] + o < size), (m, dim, o)
                assert int(tab[m, 1]) >> 21 == 0
                m += 1
        assert m == g.M


TILE_DIMS = [(1, 1, 1), (3, 5, 7), (2, 4, 8), (2, 3, 14), (2, 5, 7)]


@pytest.mark.parametrize("dims", TILE_DIMS)
@pytest.mark.parametrize("batch", [1, 3])
def test_tile_tables_against_brute_force(batch, dims):
    T, H, W = dims
    g = R.same_size_geometry(batch, dims)
    tab, tab2 = R.ref_wino_tile_table(g), R.ref_wino2_tile_table(g)
    Wq, Hq = (W + 3) // 4, (H + 1) // 2
    assert tab.shape == (batch * T * H * Wq, 2) and tab2.shape == (batch * T * Hq * Wq, 2) and tab.dtype == tab2.dtype == np.uint32
    i = i2 = 0
    for b, t in itertools.product(range(batch), range(T)):
        for h, wt in itertools.product(range(H), range(Wq)):
            bits = [0 <= t + o - 1 < T for o in range(3)] + [0 <= h + o - 1 < H for o in range(3)]
            bits += [0 <= 4 * wt - 1 + a < W for a in range(6)] + [4 * wt + o < W for o in range(4)]
            assert int(tab[i, 0]) == ((b * T + t) * H + h) * W + 4 * wt
            assert int(tab[i, 1]) == sum(int(v) << n for n, v in enumerate(bits)), (b, t, h, wt)
            i += 1
        for h2, wt in itertools.product(range(Hq), range(Wq)):
            out = [not (0 <= 2 * h2 - 1 + a < H and 0 <= 4 * wt - 1 + c < W) for a in range(4) for c in range(6)]
            out += [not (0 <= t - 1 + kt < T) for kt in range(3)] + [True]
            assert int(tab2[i2, 0]) == ((b * T + t) * H + 2 * h2) * W + 4 * wt
            assert int(tab2[i2, 1]) == sum(int(v) << n for n, v in enumerate(out)), (b, t, h2, wt)
            i2 += 1
    assert i == len(tab) and i2 == len(tab2)


def test_tile_m_counts_real_outputs_of_64_tiles():
    """variant 31: a block of 64 consecutive tiles must hold the same number of real outputs wherever it starts, else 0"""
    for dims in TILE_DIMS + [(2, 6, 10), (1, 4, 14), (2, 7, 7)]:
        T, H, W = dims
        g = R.same_size_geometry(64, dims)
        Wq, Hq = (W + 3) // 4, (H + 1) // 2
        real = np.array([min(2, H - 2 * h2) * min(4, W - 4 * wt) for h2 in range(Hq) for wt in range(Wq)] * (64 * T))
        blocks = real[:len(real) // 64 * 64].reshape(-1, 64).sum(1)
        want = int(blocks[0]) if (blocks == blocks[0]).all() else 0
        assert R.ref_tile_m(g, 31) == want, dims
        assert R.ref_tile_m(g, 30) == (128 if W % 4 == 0 else 128 // (4 * Wq) * W)
        assert (R.ref_tile_m(g, 0), R.ref_tile_m(g, 20), R.ref_tile_m(g, 22)) == (64, 64, 128)


# ---- the emulators must not pass silently -------------------------------------------------------------------------------------------
def test_a_flipped_record_bit_or_swapped_pack_columns_fail():
    """One bit of one record — the W bound in the tap mask of the first tap (offset -1 along W) of the per-tap table, bit 2 of a source
    delta in a per-chunk table — and one swapped pair of packed weight columns, each on a copy: the cases that pass above must now
    fail, and fail in the comparison with conv3d ('max error'), not in a consistency check on the way."""
    case = FWD_CASES[6]

    def drop_w_bound(g, wp):
        g.tap_tab[0, 1] ^= 1 << (14 + -1 + 3)

    def swap_columns(g, wp):
        wp[:, [5, 6]] = wp[:, [6, 5]]

    _forward(case)
    _forward(case, taps=True)
    with pytest.raises(AssertionError, match="max error"):
        _forward(case, taps=True, mutate=drop_w_bound)
    with pytest.raises(AssertionError, match="max error"):
        _forward(case, mutate=swap_columns)

    def flip_delta(g):
        g.tab[0, 0] ^= 4

    _dgrad(FWD_CASES[4])
    with pytest.raises(AssertionError, match="max error"):
        _dgrad(FWD_CASES[4], mutate=flip_delta)

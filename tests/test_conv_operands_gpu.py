"""The operand packers, layout transposes and row / tile tables of the gather-GEMM (csrc/conv.hip, csrc/conv_wino2.hip), each called
directly through the C ABI and compared with the numpy references of tests/conv_operand_ref.py (proved against conv3d in
test_conv_operands_cpu.py).

Every destination lies between the guard bands of tests/ws_guard.py and is pre-filled with SENTINEL, a finite non-zero float32 bit
pattern (1e30) that neither the seeded inputs nor any record can contain: a packer that skips a real element, writes its padding, or a
transpose that leaves a pad channel unwritten shows.  Data movement is compared as uint32 bit patterns; the two Winograd packs against
float64 within 8 * 2^-24 * (|G| . |w| resp. |Gh| . |w| . |Gw|^T) — the 1-D pack does at most four roundings per element (rounded
constant, sum, product / fma), the 2-D pack at most eight, each relative 2^-24 of a partial sum no larger than that bound."""
import ctypes
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_operand_ref as R
from ws_guard import GuardedWorkspace

pytestmark = pytest.mark.gpu

SENTINEL = 0x7149F2CA          # float32 1e30
EPS8 = 8.0 * 2.0 ** -24


def _pad8(n):
    return (n + 7) // 8 * 8


class _Bufs:
    """sentinel-filled destinations inside guard bands"""

    def __init__(self):
        self.ws = GuardedWorkspace(0xFF)
        self.n = 0

    def dst(self, nwords, skip=0):
        """int32 device view of `nwords` words, every word = SENTINEL; skip: start that many words behind the 16-byte aligned start"""
        self.n += 1
        whole = self.ws(4 * (nwords + skip), "cuda", f"dst{self.n}").view(torch.int32)
        whole.fill_(SENTINEL)
        self.last_whole = whole
        return whole[skip:]

    def check(self):
        self.ws.check()


@pytest.fixture
def bufs(gpu):
    b = _Bufs()
    yield b
    b.check()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _f32bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sentinel_array(shape):
    return np.full(shape, SENTINEL, np.uint32).view(np.float32)


def _dev(a, skip=0):
    """float32 numpy -> device tensor (skip: offset by that many floats from an aligned allocation)"""
    a = np.ascontiguousarray(a, np.float32)
    assert not (a.view(np.uint32) == SENTINEL).any()
    if not skip:
        return torch.from_numpy(a).cuda()
    whole = torch.empty(a.size + skip, dtype=torch.float32, device="cuda")
    whole[skip:].copy_(torch.from_numpy(a.reshape(-1)))
    return whole[skip:]


def _call(name, *args):
    from video_similarity_search_amd import _lib
    _lib.call(name, *args, _lib.stream())
    torch.cuda.synchronize()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _weights(seed, N, C, kernel):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, C) + tuple(kernel)).astype(np.float32)


# ---- slic_pack_weight_fwd -----------------------------------------------------------------------------------------------------------
PACK_FWD = [  # N, C, kernel, Cs, Kp (None: the plan's _pad8 value)
    (8, 3, (7, 7, 7), 4, None),
    (4, 40, (7, 7, 7), 40, None),        # 343 taps: channel tile 12288 / 343 = 35, two chunks (c0 = 0, 35)
    (4, 64, (3, 3, 3), 64, None),
    (4, 72, (3, 3, 3), 72, None),        # the 64-channel fast path, then a ragged chunk of 8
    (8, 130, (1, 1, 1), 132, None),
    (16, 3, (3, 5, 3), 4, None),
    (4, 8, (1, 1, 1), 8, 32),            # three quarters of each row is padding
]


@pytest.mark.parametrize("N,C,kernel,Cs,Kp", PACK_FWD)
def test_pack_weight_fwd(bufs, N, C, kernel, Cs, Kp):
    ntaps = int(np.prod(kernel))
    Kp = Kp or _pad8(ntaps * Cs // 4) * 4
    W = _weights(N * 131 + C, N, C, kernel)
    dst = bufs.dst(N * Kp)
    Wdev = _dev(W)
    _call("slic_pack_weight_fwd", _p(Wdev), N, C, ntaps, Cs, Kp, _p(dst))
    ref = R.ref_pack_fwd(W, Cs, Kp, _sentinel_array((N, Kp)))
    got = _bits(dst).reshape(N, Kp)
    col = np.arange(Kp)
    real = np.broadcast_to((col < ntaps * Cs) & (col % Cs < C), (N, Kp))
    assert np.array_equal(got[real], _f32bits(ref)[real]), "a real element differs"
    assert (got[~real] == SENTINEL).all(), "the padding was written"


# ---- slic_pack_weight_dgrad ---------------------------------------------------------------------------------------------------------
PACK_DGRAD = [  # N, C, ntaps, Cs, Kd, W offset, Wd offset (floats from a 16-byte boundary)
    (68, 20, 27, 20, None, 0, 0),
    (64, 64, 27, 64, None, 0, 0),
    (8, 3, 343, 4, None, 0, 0),
    (4, 4, 1, 4, 32, 0, 0),
    (68, 20, 27, 20, None, 1, 0),        # the alignment fallback (one thread per element) must give the same bits
    (68, 20, 27, 20, None, 0, 1),
]


@pytest.mark.parametrize("N,C,ntaps,Cs,Kd,woff,doff", PACK_DGRAD)
def test_pack_weight_dgrad(bufs, N, C, ntaps, Cs, Kd, woff, doff):
    Kd = Kd or _pad8(ntaps * N // 4) * 4
    W = _weights(N * 17 + C + ntaps, N, C, (ntaps,))
    Wd_ = _dev(W, skip=woff)
    dst = bufs.dst(Cs * Kd, skip=doff)
    assert Wd_.data_ptr() % 16 == 4 * woff and dst.data_ptr() % 16 == 4 * doff
    _call("slic_pack_weight_dgrad", _p(Wd_), N, C, ntaps, Cs, Kd, _p(dst))
    ref = R.ref_pack_dgrad(W, Cs, Kd, _sentinel_array((Cs, Kd)))
    got = _bits(dst).reshape(Cs, Kd)
    assert np.array_equal(got[:C, :ntaps * N], _f32bits(ref)[:C, :ntaps * N]), "a real element differs"
    assert (got[C:] == SENTINEL).all() and (got[:, ntaps * N:] == SENTINEL).all(), "rows C..Cs / columns ntaps*N..Kd were written"
    assert np.array_equal(got, _f32bits(ref))
    assert (_bits(bufs.last_whole)[:doff] == SENTINEL).all(), "the words in front of an offset destination were written"


# ---- slic_pack_weight_fwd_runs ------------------------------------------------------------------------------------------------------
PACK_RUNS = [  # C, kernel, extra _pad8 steps of Kp — the W-run stems of test_encoder_gpu.CONV_CASES at N = 8
    (3, (7, 7, 7), 0),
    (2, (3, 7, 7), 0),
    (3, (3, 5, 3), 0),
    (3, (7, 7, 7), 1),
]


@pytest.mark.parametrize("C,kernel,extra", PACK_RUNS)
def test_pack_weight_fwd_runs(bufs, C, kernel, extra):
    N, ntaps, run_px = 8, int(np.prod(kernel)), kernel[2]
    run_len = (run_px * C + 3) // 4 * 4
    Kp = (_pad8(kernel[0] * kernel[1] * run_len // 4) + 8 * extra) * 4
    W = _weights(C * 7 + ntaps, N, C, kernel)
    dst = bufs.dst(N * Kp)
    Wdev = _dev(W)
    _call("slic_pack_weight_fwd_runs", _p(Wdev), N, C, ntaps, run_len, run_px, Kp, _p(dst))
    assert np.array_equal(_bits(dst).reshape(N, Kp), _f32bits(R.ref_pack_fwd_runs(W, run_len, run_px, Kp)))


# ---- transposes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,S,Cp", [(2, 3, 5 * 7 * 9, 4), (1, 1, 257, 4), (3, 4, 256, 4), (2, 5, 33, 8)])
def test_ncdhw_to_ndhwc(bufs, B, C, S, Cp):
    x = np.random.default_rng(S + C).standard_normal((B, C, S)).astype(np.float32)
    dst = bufs.dst(B * S * Cp)
    xdev = _dev(x)
    _call("slic_ncdhw_to_ndhwc", _p(xdev), B, C, S, Cp, _p(dst))
    got = _bits(dst).reshape(B, S, Cp)
    assert not (got == SENTINEL).any(), "an element of the destination was left unwritten"
    assert np.array_equal(got, _f32bits(R.ref_ncdhw_to_ndhwc(x, Cp)))


@pytest.mark.parametrize("B,C,Rr,W,pad,Wp", [(2, 3, 6, 9, 3, 17), (1, 2, 5, 15, 3, 21), (2, 3, 4, 8, 0, 8), (1, 3, 300, 7, 1, 9)])
def test_ncdhw_to_ndhwc_wpad(bufs, B, C, Rr, W, pad, Wp):
    x = np.random.default_rng(Rr + W).standard_normal((B, C, Rr, W)).astype(np.float32)
    dst = bufs.dst(B * Rr * Wp * C)
    xdev = _dev(x)
    _call("slic_ncdhw_to_ndhwc_wpad", _p(xdev), B, C, Rr, W, pad, Wp, _p(dst))
    got = _bits(dst).reshape(B, Rr, Wp, C)
    assert not (got == SENTINEL).any(), "an element of the destination was left unwritten"
    assert np.array_equal(got, _f32bits(R.ref_ncdhw_to_ndhwc_wpad(x, pad, Wp)))


# ---- Winograd packs -----------------------------------------------------------------------------------------------------------------
def _check_wino_pack(got_bits, U, bound):
    assert not (got_bits == SENTINEL).any(), "an element of the operand was left unwritten (it has no padding)"
    got = got_bits.view(np.float32).astype(np.float64).reshape(U.shape)
    bad = np.abs(got - U) > EPS8 * bound
    assert not bad.any(), f"{bad.sum()} elements beyond 8 * 2^-24 * bound, the first at {np.argwhere(bad)[0]}"
    return got


def _wino_conv_check(got_U, bound, W, dgrad, dims, emulate):
    """the DEVICE operand, run through the float64 emulation of the kernel, gives the convolution / its data gradient: within the
    operand's own error bound pushed through the same transforms in absolute values"""
    N, C = W.shape[:2]
    rng = np.random.default_rng(11)
    x = rng.standard_normal((1, C) + dims).astype(np.float32)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    y64 = F.conv3d(x64, torch.from_numpy(W).double(), None, 1, 1)
    if dgrad:
        dy = rng.standard_normal(tuple(y64.shape)).astype(np.float32)
        ref, = torch.autograd.grad(y64, [x64], torch.from_numpy(dy).double())
        src = dy
    else:
        ref, src = y64.detach(), x
    cl = lambda a: np.einsum("bcthw->bthwc", np.asarray(a, np.float64))
    got = emulate(got_U, cl(src))
    tol = emulate(EPS8 * bound, np.abs(cl(src)), absolute=True) + 1e-10
    assert (np.abs(got - cl(ref.numpy())) <= tol).all()


@pytest.mark.parametrize("N,C,dgrad", [(64, 8, 0), (128, 24, 0), (64, 64, 0), (8, 64, 1), (64, 128, 1)])
def test_pack_weight_wino(bufs, N, C, dgrad):
    W = _weights(N + 3 * C + dgrad, N, C, (3, 3, 3))
    dst = bufs.dst(54 * N * C)
    Wdev = _dev(W)
    _call("slic_pack_weight_wino", _p(Wdev), N, C, dgrad, _p(dst))
    U, bound = R.ref_pack_wino(W, dgrad)
    got = _check_wino_pack(_bits(dst), U, bound)
    if (N, C) in ((64, 8), (8, 64)):
        _wino_conv_check(got, bound, W, dgrad, (2, 3, 7), R.emulate_wino)


@pytest.mark.parametrize("N,C,dgrad", [(64, 64, 0), (64, 64, 1), (128, 64, 0), (64, 128, 1)])
def test_pack_weight_wino2(bufs, N, C, dgrad):
    """slic_pack_weight_wino2 takes N % 64 == 0 and C % 64 == 0 in both directions"""
    W = _weights(2 * N + C + dgrad, N, C, (3, 3, 3))
    dst = bufs.dst(72 * N * C)
    Wdev = _dev(W)
    _call("slic_pack_weight_wino2", _p(Wdev), N, C, dgrad, _p(dst))
    U, bound = R.ref_pack_wino2(W, dgrad)
    got = _check_wino_pack(_bits(dst), U, bound)
    if N == C:
        _wino_conv_check(got, bound, W, dgrad, (2, 5, 7), R.emulate_wino2)


# ---- row and tile tables ------------------------------------------------------------------------------------------------------------
def _to_args(g):
    from video_similarity_search_amd._lib import SlicConvArgs
    a = SlicConvArgs()
    for f in R.GEOM_INT_FIELDS:
        setattr(a, f, int(getattr(g, f)))
    return a


def _plan_args(C, N, k, s, p, dims, wrun, B):
    """(SlicConvArgs from ConvPlan._fwd_args, the reference's geometry) — their integer fields must agree"""
    from video_similarity_search_amd.models.conv_plan import ConvPlan
    plan = ConvPlan(C, N, k, s, p, dims, "cuda", wrun=wrun, wino=False)
    x = torch.zeros((B,) + plan.src_dims + (plan.Cs,), dtype=torch.float32, device="cuda")
    a = plan._fwd_args(x, B)
    g = R.fwd_geometry(plan, B)
    assert all(int(getattr(a, f)) == int(getattr(g, f)) for f in R.GEOM_INT_FIELDS)
    return plan, a, g, x


ROW_PLANS = [
    (8, 8, (3, 3, 3), (1, 1, 1), (1, 1, 1), (3, 5, 7), False, 2),
    (8, 16, (3, 3, 3), (2, 2, 2), (1, 1, 1), (5, 7, 9), False, 2),
    (8, 8, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), False, 5),
    (8, 8, (3, 3, 3), (1, 1, 1), (1, 1, 1), (2, 4, 1), False, 2),
    (3, 8, (7, 7, 7), (1, 2, 2), (3, 3, 3), (4, 9, 10), True, 2),       # the W-run stem: Cs = 3, padded width
]


def _row_cases():
    out = []
    for spec in ROW_PLANS:
        plan, a, g, x = _plan_args(*spec)
        out.append((a, g, x))
    plan = _plan_args(*ROW_PLANS[1])[0]                                  # one stride-2 data-gradient parity class
    g = R.dgrad_geometry(plan, next(dc for dc in plan.dgrad_classes if dc["cls"] == (1, 0, 1)), 2)
    out.append((_to_args(g), g, None))
    return out


TILE_DIMS = [(1, 1, 1), (3, 5, 7), (2, 4, 8), (2, 3, 14)]


def test_conv_row_table(bufs):
    for a, g, _ in _row_cases():
        dst = bufs.dst(2 * g.M)
        _call("slic_conv_row_table", ctypes.byref(a), _p(dst))
        assert np.array_equal(_bits(dst).reshape(g.M, 2), R.ref_row_table(g)), vars(g)


@pytest.mark.parametrize("dims", TILE_DIMS)
@pytest.mark.parametrize("B", [1, 3])
def test_conv_wino_tile_table(bufs, B, dims):
    g = R.same_size_geometry(B, dims)
    ref = R.ref_wino_tile_table(g)
    dst = bufs.dst(ref.size)
    _call("slic_conv_wino_tile_table", ctypes.byref(_to_args(g)), _p(dst))
    assert np.array_equal(_bits(dst).reshape(ref.shape), ref)


@pytest.mark.parametrize("dims", TILE_DIMS + [(2, 5, 7)])
@pytest.mark.parametrize("B", [1, 3])
def test_conv_wino2_tile_table(bufs, B, dims):
    g = R.same_size_geometry(B, dims)
    ref = R.ref_wino2_tile_table(g)
    dst = bufs.dst(ref.size)
    _call("slic_conv_wino2_tile_table", ctypes.byref(_to_args(g)), _p(dst))
    assert np.array_equal(_bits(dst).reshape(ref.shape), ref)


def test_conv_tile_m(gpu):
    geoms = [(a, g) for a, g, _ in _row_cases()]
    for B, dims in itertools.product((1, 3), TILE_DIMS + [(2, 5, 7)]):
        g = R.same_size_geometry(B, dims)
        geoms.append((_to_args(g), g))
    zero = 0
    for a, g in geoms:
        for variant in (0, 20, 22, 30, 31):
            want = R.ref_tile_m(g, variant)
            assert gpu.slic_conv_tile_m(ctypes.byref(a), variant) == want, (vars(g), variant)
            zero += variant == 31 and want == 0
    assert R.ref_tile_m(R.same_size_geometry(1, (3, 5, 7)), 31) == 0 and zero > 0      # 3 x 2 tiles per frame do not divide 64


# ---- error paths --------------------------------------------------------------------------------------------------------------------
def test_violated_requirements_are_refused(gpu, bufs):
    """one call per entry point that breaks a documented requirement: non-zero return, slic_last_error set, destination untouched
    (slic_conv_tile_m has no error return: it is a pure function of the geometry)"""
    from video_similarity_search_amd import _lib
    srcdev = _dev(np.ones(4096, np.float32))
    src = _p(srcdev)
    dst = bufs.dst(4096)
    d = _p(dst)
    st = _lib.stream()
    same = R.same_size_geometry(1, (2, 4, 8))
    not_same = R.same_size_geometry(1, (2, 4, 8))
    not_same.Gc = 4
    ragged_m = R.same_size_geometry(1, (2, 4, 8))
    ragged_m.M += 1
    calls = [
        ("slic_pack_weight_fwd", (src, 4, 8, 1, 4, 32, d, st)),                       # Cs < C
        ("slic_pack_weight_fwd", (src, 4, 8, 27, 8, 208, d, st)),                     # Kp < ntaps * Cs
        ("slic_pack_weight_fwd_runs", (src, 4, 3, 49, 24, 7, 160, d, st)),            # Kp < 7 runs of 24
        ("slic_pack_weight_fwd_runs", (src, 4, 3, 49, 20, 7, 168, d, st)),            # run_px * C > run_len
        ("slic_pack_weight_dgrad", (src, 4, 8, 1, 4, 32, d, st)),                     # Cs < C
        ("slic_pack_weight_dgrad", (src, 8, 4, 27, 4, 208, d, st)),                   # Kd < ntaps * N
        ("slic_pack_weight_wino", (src, 32, 8, 0, d, st)),                            # N_ % 64 != 0
        ("slic_pack_weight_wino", (src, 64, 4, 0, d, st)),                            # C_ % 8 != 0
        ("slic_pack_weight_wino", (src, 64, 8, 1, d, st)),                            # dgrad: N_ = C = 8
        ("slic_pack_weight_wino2", (src, 32, 64, 0, d, st)),                          # N % 64 != 0
        ("slic_pack_weight_wino2", (src, 64, 8, 1, d, st)),                           # C % 64 != 0
        ("slic_ncdhw_to_ndhwc", (src, 2, 5, 16, 4, d, st)),                           # Cp < C
        ("slic_ncdhw_to_ndhwc_wpad", (src, 1, 3, 4, 8, 3, 10, d, st)),                # Wp < W + pad_left
        ("slic_conv_row_table", (ctypes.byref(_to_args(ragged_m)), d, st)),           # M is not batch * grid
        ("slic_conv_wino_tile_table", (ctypes.byref(_to_args(not_same)), d, st)),     # not a same-size geometry
        ("slic_conv_wino2_tile_table", (ctypes.byref(_to_args(not_same)), d, st)),
    ]
    assert gpu.slic_conv_wino_tile_table(ctypes.byref(_to_args(same)), d, st) == 0    # the geometry itself is fine ...
    torch.cuda.synchronize()
    dst.fill_(SENTINEL)                                                               # ... and the destination poisoned again
    for name, args in calls:
        rc = getattr(gpu, name)(*args)
        msg = gpu.slic_last_error().decode()
        assert rc != 0, f"{name}{args[1:-2]} was accepted"
        assert name in msg, (name, msg)
    torch.cuda.synchronize()
    assert (_bits(dst) == SENTINEL).all(), "a refused call wrote to its destination"

"""GPU: every entry point of csrc/bn.hip called directly and compared with float64 — the statistics tree and its finalisation, the
SyncBatchNorm halves, the eval affine, apply, the two-pass and the slab-fed backward, the pools, shortcut 'A' and slic_colsum.

The cases and gates are functions of a backend: `Device` calls the library; tests/test_bn_pool_cpu.py runs the same functions with
the NumPy mirror (tests/bn_cpu_kernels.py) in the device's place, unmutated (every gate can be met in float32) and with one defect
at a time (every gate that matters is tight enough to notice).  Every workspace is the first `*_workspace_bytes` bytes of a larger
buffer whose 4096-byte tail must come back unchanged, every output starts as NaN, and every statistics / backward call runs
twice into fresh outputs that must be bit-equal."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_cpu_kernels as K

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4096


def f32(a):
    return np.ascontiguousarray(a, dtype=F32)


def ulps(a, b):
    """distance in float32 steps (signed zeros coincide)"""
    def key(x):
        i = f32(x).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def bits_equal(a, b):
    a, b = f32(a), f32(b)
    return a.shape == b.shape and bool(np.all((a == b) | ((a != a) & (b != b))))


# ------------------------------------------------------------------ the device backend
class Device:
    def __init__(self, lib):
        from video_similarity_search_amd import _lib
        self.lib, self._lib = lib, _lib
        self.pattern = (torch.arange(GUARD) % 251).to(torch.uint8).cuda()

    # -- plumbing
    def up(self, a, dtype=F32):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()

    def nan(self, *shape):
        return torch.full(shape, float("nan"), device="cuda")

    def ws(self, nbytes):
        buf = torch.empty(int(nbytes) + GUARD, dtype=torch.uint8, device="cuda")
        buf[int(nbytes):] = self.pattern
        return buf, int(nbytes)

    def run(self, name, *args, guards=()):
        p = self._lib.ptr
        self._lib.call(name, *[p(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], self._lib.stream())
        torch.cuda.synchronize()
        for buf, n in guards:
            assert torch.equal(buf[n:], self.pattern), f"{name} wrote past its workspace of {n} bytes"

    # -- statistics
    def _stat_out(self, C, rm, rv):
        o = dict(mean=self.nan(C), invstd=self.nan(C), scale=self.nan(C), shift=self.nan(C))
        return o, self.up(rm), self.up(rv)

    def _stat_np(self, o, rm, rv):
        r = {k: v.cpu().numpy() for k, v in o.items()}
        if rm is not None:
            r["running_mean"], r["running_var"] = rm.cpu().numpy(), rv.cpu().numpy()
        return r

    def finalize(self, slab, rows, M, eps, mom, gamma, beta, rm, rv):
        R, _, C = slab.shape
        o, rm, rv = self._stat_out(C, rm, rv)
        w = self.ws(self.lib.slic_bn_finalize_workspace_bytes(R, C))
        self.run("slic_bn_finalize", self.up(slab), R, rows, C, M, eps, mom, self.up(gamma), self.up(beta), o["mean"], o["invstd"],
                 o["scale"], o["shift"], rm, rv, w[0], guards=[w])
        return self._stat_np(o, rm, rv)

    def merge_stats(self, slab, rows, M):
        R, _, C = slab.shape
        st = torch.full((2 * C + 1,), float("nan"), dtype=torch.float64, device="cuda")
        w = self.ws(self.lib.slic_bn_finalize_workspace_bytes(R, C))
        self.run("slic_bn_merge_stats", self.up(slab), R, rows, C, M, st, w[0], guards=[w])
        assert torch.isnan(st[2 * C]).item(), "slic_bn_merge_stats wrote past its 2 C doubles"
        return st[:2 * C].cpu().numpy()

    def finalize_sync(self, stats, C, eps, mom, gamma, beta, rm, rv):
        o, rm, rv = self._stat_out(C, rm, rv)
        self.run("slic_bn_finalize_sync", self.up(stats, np.float64), stats.shape[0], C, eps, mom, self.up(gamma), self.up(beta),
                 o["mean"], o["invstd"], o["scale"], o["shift"], rm, rv)
        return self._stat_np(o, rm, rv)

    # -- backward
    def bwd(self, dy, out, z, mean, invstd, gamma, g_given):
        M, C = dy.shape
        g = self.nan(M, C) if g_given else None
        dz, dg, db = self.nan(M, C), self.nan(C), self.nan(C)
        w = self.ws(self.lib.slic_bn_bwd_workspace_bytes(M, C, int(out is not None and not g_given)))
        self.run("slic_bn_bwd", self.up(dy), self.up(out), self.up(z), self.up(mean), self.up(invstd), self.up(gamma), M, C, g, dz,
                 dg, db, w[0], guards=[w])
        return (None if g is None else g.cpu().numpy()), dz.cpu().numpy(), dg.cpu().numpy(), db.cpu().numpy()

    def bwd_sums(self, partial, dy, out, z, mean, invstd, M, C):
        R = 0 if partial is None else partial.shape[0]
        g = self.nan(M, C) if (partial is None and out is not None) else None
        sums = torch.full((2 * C,), float("nan"), dtype=torch.float64, device="cuda")
        dg, db = self.nan(C), self.nan(C)
        w = self.ws(self.lib.slic_bn_bwd_sums_workspace_bytes(M, C, R))
        self.run("slic_bn_bwd_sums", self.up(partial), R, self.up(dy), self.up(out), self.up(z), self.up(mean), self.up(invstd), M, C, g,
                 sums, dg, db, w[0], guards=[w])
        return (None if g is None else g.cpu().numpy()), sums.cpu().numpy(), dg.cpu().numpy(), db.cpu().numpy()

    def bwd_apply(self, g, z, mean, invstd, gamma, ka, kb):
        M, C = g.shape
        dz = self.nan(M, C)
        self.run("slic_bn_bwd_apply", self.up(g), self.up(z), self.up(mean), self.up(invstd), self.up(gamma), self.up(ka, np.float64),
                 self.up(kb, np.float64), M, C, dz)
        return dz.cpu().numpy()

    def bwd_fused(self, partial, g, z, mean, invstd, gamma):
        M, C = g.shape
        R = partial.shape[0]
        dz, dg, db = self.nan(M, C), self.nan(C), self.nan(C)
        w = self.ws(self.lib.slic_bn_bwd_fused_workspace_bytes(R, C))
        self.run("slic_bn_bwd_fused", self.up(partial), R, self.up(g), self.up(z), self.up(mean), self.up(invstd), self.up(gamma), M, C,
                 dz, dg, db, w[0], guards=[w])
        return dz.cpu().numpy(), dg.cpu().numpy(), db.cpu().numpy()

    # -- pools, shortcut
    def maxpool_fwd(self, x, with_arg=True):
        B, T, H, W, C = x.shape
        shp = (B, K._odim(T), K._odim(H), K._odim(W), C)
        y = self.nan(*shp)
        arg = torch.full(shp, -7, dtype=torch.int32, device="cuda") if with_arg else None
        self.run("slic_maxpool3d_fwd", self.up(x), B, T, H, W, C, y, arg)
        return y.cpu().numpy(), (arg.cpu().numpy() if with_arg else None)

    def maxpool_bwd(self, dy, arg, dims):
        B, C = dy.shape[0], dy.shape[-1]
        dx = self.nan(B, *dims, C)
        self.run("slic_maxpool3d_bwd", self.up(dy), self.up(arg, np.int32), B, *dims, C, dx)
        return dx.cpu().numpy()

    def shortcut_a(self, x, stride, C_out):
        B, T, H, W, C = x.shape
        y = self.nan(B, K._odim(T, stride), K._odim(H, stride), K._odim(W, stride), C_out)
        self.run("slic_shortcut_a", self.up(x), B, T, H, W, C, stride, C_out, y)
        return y.cpu().numpy()


@pytest.fixture(scope="module")
def dev(gpu):
    return Device(gpu)


def twice(fn):
    """two runs into fresh outputs, bit-equal"""
    a, b = fn(), fn()
    fa = a.values() if isinstance(a, dict) else a
    fb = b.values() if isinstance(b, dict) else b
    for u, v in zip(fa, fb):
        assert (u is None and v is None) or np.array_equal(u.view(np.uint8), v.view(np.uint8)), "two runs differ"
    return a


# ------------------------------------------------------------------ a) statistics
def make_slab(R, rows, C, last, kind, seed=0):
    """the conv epilogue's slab, built in float64 from float32-representable data and rounded to float32: row r holds (sum,
    sum (x - mean_r)^2) of `rows` samples, the last row of `last`.  kind 'wide' = 0.5 + 2 N(0, 1); 'narrow' = 100 + 0.05 N(0, 1)
    (variance 2.5e-3 against E[x^2] = 1e4: E[x^2] - E[x]^2 in float32 is off by a quarter).  The last channel is constant."""
    M = (R - 1) * rows + last
    rng = np.random.default_rng(seed + 7 * R + rows)
    a, b = (0.5, 2.0) if kind == "wide" else (100.0, 0.05)
    x = (a + b * rng.standard_normal((M, C))).astype(F32)
    if M > 1:
        x[:, C - 1] = F32(100.25)
    xp = np.zeros((R * rows, C))
    xp[:M] = x
    xp = xp.reshape(R, rows, C)
    n = np.full((R, 1), float(rows))
    n[-1] = last
    s = xp.sum(1)
    live = (np.arange(rows)[None, :] < n)[:, :, None]
    m2 = (((xp - (s / n)[:, None]) ** 2) * live).sum(1)
    return np.stack([s, m2], 1).astype(F32), M


def stat_params(C, affine, running, seed):
    rng = np.random.default_rng(100 + seed)
    gamma = (1 + 0.3 * rng.standard_normal(C)).astype(F32) if affine else None
    beta = (0.2 * rng.standard_normal(C)).astype(F32) if affine else None
    rm = (0.7 * rng.standard_normal(C)).astype(F32) if running else None
    rv = (0.5 + rng.random(C)).astype(F32) if running else None
    return gamma, beta, rm, rv


def stats_reference(slab, rows, M, eps, mom, gamma, beta, rm, rv):
    """flat float64 statistics of the float32 slab; eps and momentum are the float32 values the ABI carries"""
    mean, m2 = K.flat_stats(slab, rows, M)
    C = mean.shape[0]
    var = m2 / M
    unb = var * M / (M - 1) if M > 1 else var
    inv = 1.0 / np.sqrt(var + np.float64(F32(eps)))
    g = np.ones(C) if gamma is None else gamma.astype(np.float64)
    b = np.zeros(C) if beta is None else beta.astype(np.float64)
    ref = dict(mean=mean, invstd=inv, scale=g * inv, beta=b)
    ref["shift"] = b - mean * ref["scale"]
    if rm is not None:
        m = np.float64(F32(mom))
        ref["run"] = {"running_mean": ((1 - m) * rm.astype(np.float64), m * mean),
                      "running_var": ((1 - m) * rv.astype(np.float64), m * unb)}
    return ref


def gate_stats(res, ref, what):
    """mean, invstd, scale: 2 float32 steps from the rounded float64 value (the device merges in double; the outputs are one or two
    float32 roundings of that).  shift: 2^-22 (|beta| + |mean scale|).  running statistics: 2^-22 (|(1 - m) old| + |m new|)."""
    for k in ("mean", "invstd", "scale"):
        assert np.all(np.isfinite(res[k])), (what, k)
        d = ulps(res[k], ref[k].astype(F32))
        assert d.max() <= 2, (what, k, int(d.max()), int(d.argmax()))
    err = np.abs(res["shift"].astype(np.float64) - ref["shift"])
    assert np.all(err <= 2.0 ** -22 * (np.abs(ref["beta"]) + np.abs(ref["mean"] * ref["scale"]))), (what, "shift", err.max())
    for k, (old, new) in ref.get("run", {}).items():
        err = np.abs(res[k].astype(np.float64) - (old + new))
        assert np.all(err <= 2.0 ** -22 * (np.abs(old) + np.abs(new))), (what, k, err.max())
    if "run" not in ref:
        assert "running_mean" not in res


# (R, rows, C, last, kind, affine, running, (eps, momentum))
E0, E1 = (1e-5, 0.1), (1e-3, 0.25)
STAT_CASES = [
    (1, 4, 8, 1, "wide", True, True, E0), (16, 4, 8, 3, "narrow", True, True, E1), (17, 4, 8, 1, "narrow", False, True, E0),
    (33, 128, 8, 127, "wide", True, False, E0), (48, 4, 4, 1, "narrow", True, True, E0), (49, 1, 8, 1, "wide", True, True, E1),
    (63, 192, 8, 191, "narrow", True, True, E0), (64, 4, 68, 3, "narrow", False, False, E1),
    (65, 128, 68, 1, "narrow", True, True, E0), (65, 4, 200, 3, "wide", True, True, E1), (4096, 4, 4, 1, "narrow", True, True, E0),
    (4097, 4, 8, 3, "narrow", True, True, E0), (4097, 1, 200, 1, "wide", False, True, E1), (17, 192, 200, 1, "narrow", True, True, E0),
    (33, 4, 2048, 1, "narrow", True, True, E1), (129, 4, 2048, 3, "wide", True, False, E0),
    (64 ** 3 + 1, 1, 4, 1, "narrow", True, True, E0),
]


def check_stats(be, case):
    R, rows, C, last, kind, affine, running, (eps, mom) = case
    slab, M = make_slab(R, rows, C, last, kind)
    gamma, beta, rm, rv = stat_params(C, affine, running, R)
    res = twice(lambda: be.finalize(slab, rows, M, eps, mom, gamma, beta, rm, rv))
    gate_stats(res, stats_reference(slab, rows, M, eps, mom, gamma, beta, rm, rv), case)
    if M > 1:                                            # the constant channel: variance 0 (rows = 192 rounds its sums: below eps / 1e5)
        assert abs(res["invstd"][C - 1] * np.sqrt(np.float64(F32(eps))) - 1) < 1e-5


def check_stats_single_sample(be):
    """M = 1: variance 0, everything finite, the running variance moves toward 0 by exactly its (1 - momentum) share"""
    slab, M = make_slab(1, 4, 8, 1, "wide")
    assert M == 1 and not slab[:, 1].any()
    gamma, beta, rm, rv = stat_params(8, True, True, 1)
    res = twice(lambda: be.finalize(slab, 4, 1, 1e-5, 0.1, gamma, beta, rm, rv))
    gate_stats(res, stats_reference(slab, 4, 1, 1e-5, 0.1, gamma, beta, rm, rv), "M=1")
    assert np.all(res["running_var"] < rv) and np.all(res["running_var"] > 0)


def check_row_order(be):
    """The contract in bn.hip's header: partial sums are added in workgroup order, in double.  Rows 0..15 hold 2^80, rows 16..31 hold
    -2^80, row 32 holds 1, the rest 0 (one sample a row).  Added in row order, under any grouping that keeps the order, the sum is
    exactly 1 and the mean 1 / 64; a merge that takes a later group first absorbs the 1 into 2^80 and answers 0."""
    C = 4
    slab = np.zeros((64, 2, C), F32)
    slab[:16, 0], slab[16:32, 0], slab[32, 0] = 2.0 ** 80, -2.0 ** 80, 1.0
    res = twice(lambda: be.finalize(slab, 1, 64, 1e-5, 0.1, None, None, None, None))
    assert np.array_equal(res["mean"], np.full(C, 1 / 64, F32)), res["mean"]
    st = twice(lambda: [be.merge_stats(slab, 1, 64)])[0]
    assert np.array_equal(st[:C], np.ones(C)), st[:C]


SYNC_SHARDS = {1: [100], 3: [70, 1, 29], 8: [65, 1, 3, 5, 7, 2, 9, 8]}


def check_sync(be, W, zero_at):
    """the rows of one slab dealt to W unequal shards (one beyond BN_MG rows, one of a single row), each merged by slic_bn_merge_stats
    with its own count in stats[2 C] as models/resnet.py writes it, an all-zero row with n = 0 injected at `zero_at`, finalised in
    one process: the statistics of the union, at the gates of the plain path"""
    R, rows, C, eps, mom = 100, 4, 68, 1e-5, 0.1
    slab, M = make_slab(R, rows, C, 1, "narrow")
    gamma, beta, rm, rv = stat_params(C, True, True, W)
    stats, r0 = [], 0
    for n in SYNC_SHARDS[W]:
        part = slab[r0:r0 + n]
        Mw = min(M - r0 * rows, n * rows)
        row = twice(lambda: [be.merge_stats(part, rows, Mw)])[0]
        stats.append(np.concatenate([row, [float(Mw)]]))
        r0 += n
    assert r0 == R
    stats.insert(zero_at if zero_at >= 0 else len(stats), np.zeros(2 * C + 1))
    stats = np.stack(stats)
    res = twice(lambda: be.finalize_sync(stats, C, eps, mom, gamma, beta, rm, rv))
    gate_stats(res, stats_reference(slab, rows, M, eps, mom, gamma, beta, rm, rv), ("sync", W))
    res = be.finalize_sync(stats, C, eps, mom, None, None, None, None)
    gate_stats(res, stats_reference(slab, rows, M, eps, mom, None, None, None, None), ("sync plain", W))


@pytest.mark.parametrize("case", STAT_CASES, ids=lambda c: f"R{c[0]}-rows{c[1]}-C{c[2]}-last{c[3]}-{c[4]}")
def test_statistics_tree(dev, case):
    check_stats(dev, case)


def test_statistics_single_sample(dev):
    check_stats_single_sample(dev)


def test_statistics_row_order(dev):
    check_row_order(dev)


@pytest.mark.parametrize("W,zero_at", [(1, 0), (3, 1), (8, -1)])
def test_sync_halves_equal_the_union(dev, W, zero_at):
    check_sync(dev, W, zero_at)


# ------------------------------------------------------------------ b) eval affine, apply
@pytest.mark.parametrize("C", [4, 68, 2048])
@pytest.mark.parametrize("affine", [True, False])
def test_eval_affine(dev, C, affine):
    """scale within 2^-21 relative (the float32 add, sqrt, divide and multiply), shift within 2^-22 (|beta| + |mean scale|)"""
    gamma, beta, rm, rv = stat_params(C, affine, True, C)
    rv[0], rv[1] = 0.0, 1e-8
    for eps in (1e-5, 1e-3):
        scale, shift = dev.nan(C), dev.nan(C)
        dev.run("slic_bn_eval_affine", dev.up(gamma), dev.up(beta), dev.up(rm), dev.up(rv), eps, C, scale, shift)
        g = np.ones(C) if gamma is None else gamma.astype(np.float64)
        b = np.zeros(C) if beta is None else beta.astype(np.float64)
        sc = g / np.sqrt(rv.astype(np.float64) + np.float64(F32(eps)))
        assert np.all(np.abs(scale.cpu().numpy() - sc) <= 2.0 ** -21 * np.abs(sc))
        ref = b - rm.astype(np.float64) * sc
        assert np.all(np.abs(shift.cpu().numpy() - ref) <= 2.0 ** -22 * (np.abs(b) + np.abs(rm * sc)))


@pytest.mark.parametrize("M,C", [(77, 12), (1, 4), (1031, 200), (2097184, 8)])
def test_apply(dev, M, C):
    """y = relu?(z scale + shift (+ res)) within 2^-23 (|z scale| + |shift| + |res|) of float64 (two roundings, or three with the
    product contracted into an FMA), all four (res, relu) forms; M C / 4 is no multiple of 256, and 16384 * 256 + 64 in the last
    case, just past the grid cap, where every thread takes a second element"""
    assert (M * C // 4) % 256 and (M < 10 ** 6 or M * C // 4 == 16384 * 256 + 64)
    rng = np.random.default_rng(M)
    z, res = f32(rng.standard_normal((M, C)) * 2 + 0.5), f32(rng.standard_normal((M, C)))
    scale, shift = f32(1 + 0.3 * rng.standard_normal(C)), f32(rng.standard_normal(C))
    zd, rd, sd, hd = dev.up(z), dev.up(res), dev.up(scale), dev.up(shift)
    base = z.astype(np.float64) * scale + shift
    mag = np.abs(z.astype(np.float64) * scale) + np.abs(shift.astype(np.float64))
    for with_res in (False, True):
        for relu in (0, 1):
            y = dev.nan(M, C)
            dev.run("slic_bn_apply", zd, sd, hd, rd if with_res else None, relu, M, C, y)
            y = y.cpu().numpy()
            ref = base + res if with_res else base
            tol = 2.0 ** -23 * (mag + np.abs(res) if with_res else mag)
            if relu:
                assert y.min() >= 0
                ref = np.maximum(ref, 0)
            assert np.all(np.abs(y - ref) <= tol), (with_res, relu, float(np.max(np.abs(y - ref) - tol)))


# ------------------------------------------------------------------ c) backward
def bwd_reference(dy, out, z, mean, invstd, gamma):
    """float64, the float32 mean / invstd taken as exact numbers; the mask comes from the very `out` the kernel reads"""
    d = lambda a: np.asarray(a, np.float64)
    g = d(dy) * (np.asarray(out) > 0) if out is not None else d(dy)
    xh = (d(z) - d(mean)) * d(invstd)
    M = dy.shape[0]
    s1, s2 = g.sum(0), (g * xh).sum(0)
    gi = np.abs(d(gamma) * d(invstd))
    return dict(g=g, xh=xh, s1=s1, s2=s2, gi=gi, dz=d(gamma) * d(invstd) * (g - s1 / M - xh * s2 / M))


def data_exact(M, C, seed=0):
    """integer-valued: every float32 product and partial sum is exact, so a dropped, repeated or mis-addressed row shows as a unit"""
    rng = np.random.default_rng(seed + M + C)
    z, dy = f32(rng.integers(-3, 4, (M, C))), f32(rng.integers(-3, 4, (M, C)))
    out = f32(np.array([-1.0, -0.0, 0.0, 1.0])[rng.integers(0, 4, (M, C))])
    gamma = f32(np.array([0.5, 1.0, 2.0])[rng.integers(0, 3, C)])
    return dy, out, z, np.zeros(C, F32), np.ones(C, F32), gamma


def data_random(be, M, C, seed=0):
    """random floats; mean / invstd are what the statistics path gives for z (one slab row)"""
    rng = np.random.default_rng(seed + M + C)
    z, dy = f32(0.5 + 2 * rng.standard_normal((M, C))), f32(rng.standard_normal((M, C)))
    out = f32(rng.standard_normal((M, C)))
    out[rng.random((M, C)) < 0.1] = 0.0
    gamma = f32(1 + 0.3 * rng.standard_normal(C))
    s = z.astype(np.float64).sum(0)
    slab = np.stack([s, ((z - s / M) ** 2).sum(0)])[None].astype(F32)
    st = be.finalize(slab, M, M, 1e-5, 0.1, None, None, None, None)
    return dy, out, z, st["mean"], st["invstd"], gamma


def gate_exact(ref, g, dz, dgamma, dbeta, what):
    """g, dgamma, dbeta bit for bit; dz within one float32 step of the float64 value.  Where the bracket g - s1/M - xhat s2/M
    cancels to nothing (g = 0, s1 = -xhat s2) the float64 value is 0 or a last-bit residue of the three double terms and a
    distance in steps of IT says nothing: the double bracket is granted 2^-50 of its terms on top of the one float32 step."""
    if g is not None:
        assert bits_equal(g, ref["g"] + 0.0), (what, "g")          # + 0.0: a masked -x * 0 is +0 on the device (a select, not a product)
    assert bits_equal(dgamma, ref["s2"]) and bits_equal(dbeta, ref["s1"]), what
    M = ref["g"].shape[0]
    terms = np.abs(ref["g"]) + np.abs(ref["s1"] / M) + np.abs(ref["xh"] * ref["s2"] / M)
    step = np.spacing(np.abs(ref["dz"]).astype(F32)).astype(np.float64)
    err = np.abs(dz - ref["dz"])
    assert np.all(err <= step + 2.0 ** -50 * ref["gi"] * terms), (what, "dz", float(err.max()))


def gate_random(ref, g, dz, dgamma, dbeta, what):
    """the project's gates (test_bn_train_fwd_bwd)"""
    if g is not None:
        assert np.abs(g - ref["g"]).max() < 1e-6, what
    assert np.abs(dz - ref["dz"]).max() < 2e-5 * max(1.0, np.abs(ref["dz"]).max()), what
    assert np.abs(dgamma - ref["s2"]).max() < 1e-4 * max(1.0, np.abs(ref["s2"]).max()), what
    assert np.abs(dbeta - ref["s1"]).max() < 1e-4 * max(1.0, np.abs(ref["s1"]).max()), what


# (out given, g_out given)
MODES = [(True, True), (True, False), (False, False), (False, True)]
BWD_SHAPES = ([(M, 48) for M in (1, 2, 3, 4, 255, 256, 257, 16384, 16385)] +
              [(700, C) for C in (8, 48, 64, 200, 1028, 1200, 2048)] +
              [(259, 1024)])        # one row a thread-step (RL = 1) and 3 rows in the last block: the loop after the unrolled one alone


def check_bwd(be, M, C, exact):
    """slic_bn_bwd in its four modes; then slic_bn_bwd_sums + slic_bn_bwd_apply from dy / out / z with k = sums / M: the same bits"""
    dy, out, z, mean, invstd, gamma = data_exact(M, C) if exact else data_random(be, M, C)
    gate = gate_exact if exact else gate_random
    for has_out, has_g in MODES:
        o = out if has_out else None
        ref = bwd_reference(dy, o, z, mean, invstd, gamma)
        g, dz, dg, db = twice(lambda: be.bwd(dy, o, z, mean, invstd, gamma, has_g))
        assert (g is not None) == has_g
        if has_g and not has_out:
            assert bits_equal(g, dy)
        gate(ref, g, dz, dg, db, (M, C, has_out, has_g))
        if has_g != has_out:
            continue                                      # the sums entry point writes g exactly when it masks
        g2, sums, dg2, db2 = twice(lambda: be.bwd_sums(None, dy, o, z, mean, invstd, M, C))
        if exact:
            assert np.array_equal(sums, np.concatenate([ref["s1"], ref["s2"]]))
        gin = g2 if has_out else dy
        dz2 = be.bwd_apply(gin, z, mean, invstd, gamma, sums[:C] / M, sums[C:] / M)
        assert bits_equal(dz2, dz) and bits_equal(dg2, dg) and bits_equal(db2, db) and (g2 is None or bits_equal(g2, g))
        # the frozen case: k = 0, dz = gamma invstd g (one rounding of a double product)
        dz0 = be.bwd_apply(gin, z, mean, invstd, gamma, np.zeros(C), np.zeros(C))
        assert ulps(dz0, (gamma.astype(np.float64) * invstd.astype(np.float64) * ref["g"]).astype(F32)).max() <= 1


def host_slab(g, xh, R, L):
    """what a dgrad epilogue emits (ConvPlan.dgrad(..., bwd=...)): R rows of (sum g, sum g xhat) over L samples each, float32"""
    M, C = g.shape
    gp, pp = np.zeros((R * L, C)), np.zeros((R * L, C))
    gp[:M], pp[:M] = g, g * xh
    return np.stack([gp.reshape(R, L, C).sum(1), pp.reshape(R, L, C).sum(1)], 1).astype(F32)


FUSED_SHAPES = [(1, 5, 8), (64, 3, 48), (65, 3, 200), (4097, 3, 8), (65, 7, 1028)]      # (R, slab row length, C)


def check_bwd_slab(be, R, L, C, exact):
    """slic_bn_bwd_fused, and slic_bn_bwd_sums (+ apply) in its slab form, from a host-built slab of R rows of L samples"""
    M = R * L - (L - 1 if R > 1 else 0)
    dy, out, z, mean, invstd, gamma = data_exact(M, C, 1) if exact else data_random(be, M, C, 1)
    g = f32(np.where(out > 0, dy, 0))
    ref = bwd_reference(g, None, z, mean, invstd, gamma)
    xh32 = ((z - mean) * invstd).astype(np.float64)           # the float32 xhat of the epilogue
    slab = host_slab(g.astype(np.float64), xh32, R, L)
    gate = gate_exact if exact else gate_random
    dz, dg, db = twice(lambda: be.bwd_fused(slab, g, z, mean, invstd, gamma))
    gate(ref, None, dz, dg, db, ("fused", R, L, C))
    g2, sums, dg2, db2 = twice(lambda: be.bwd_sums(slab, None, None, None, None, None, M, C))
    assert g2 is None and bits_equal(dg2, dg) and bits_equal(db2, db)
    if exact:
        assert np.array_equal(sums, np.concatenate([ref["s1"], ref["s2"]]))
    dz2 = be.bwd_apply(g, z, mean, invstd, gamma, sums[:C] / M, sums[C:] / M)
    assert bits_equal(dz2, dz)


def check_bwd_small_batch(be, M, C):
    """the BatchNorm1d head: M = 2..4 samples a channel, where the bracket cancels.  Elementwise
    |dz - ref| <= 2^-20 gamma invstd (|g| + mean|g| + |xhat| mean|g xhat|): two float32 roundings in xhat, float32 sums of at most
    four terms, the final rounding."""
    dy, _, z, mean, invstd, gamma = data_random(be, M, C, 2)
    ref = bwd_reference(dy, None, z, mean, invstd, gamma)
    _, dz, dg, db = twice(lambda: be.bwd(dy, None, z, mean, invstd, gamma, False))
    g, xh = np.abs(ref["g"]), np.abs(ref["xh"])
    tol = 2.0 ** -20 * np.abs(gamma * invstd.astype(np.float64)) * (g + g.mean(0) + xh * (g * xh).mean(0))
    assert np.all(np.abs(dz - ref["dz"]) <= tol), float(np.max(np.abs(dz - ref["dz"]) / tol))
    gate_random(ref, None, dz, dg, db, ("small", M, C))


@pytest.mark.parametrize("M,C", BWD_SHAPES)
def test_bwd_integer_data_is_exact(dev, M, C):
    check_bwd(dev, M, C, True)


@pytest.mark.parametrize("M,C", BWD_SHAPES)
def test_bwd_random_data(dev, M, C):
    check_bwd(dev, M, C, False)


@pytest.mark.parametrize("R,L,C", FUSED_SHAPES)
@pytest.mark.parametrize("exact", [True, False])
def test_bwd_from_a_slab(dev, R, L, C, exact):
    check_bwd_slab(dev, R, L, C, exact)


@pytest.mark.parametrize("M", [2, 3, 4])
@pytest.mark.parametrize("C", [512, 2048])
def test_bwd_small_batch(dev, M, C):
    check_bwd_small_batch(dev, M, C)


def test_rows_per_partial(gpu):
    assert gpu.slic_bn_bwd_rows_per_partial() == K.BNB_RB == 256


# ------------------------------------------------------------------ d) pools, shortcut, column sum
POOL_DIMS = [(1, 1, 1), (1, 5, 4), (2, 3, 7), (5, 6, 9), (4, 8, 8)]


def pool_input(dims, C, B=2):
    """small integers (many ties), one all-zero channel, one NaN"""
    rng = np.random.default_rng(sum(dims) + C)
    x = f32(rng.integers(-2, 3, (B, *dims, C)))
    x[..., C - 1] = 0
    x[B - 1, dims[0] // 2, dims[1] // 2, dims[2] // 2, 0] = np.nan
    return x


def ncdhw(a):
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(a, -1, 1)))


def ndhwc(t):
    return np.ascontiguousarray(np.moveaxis(t.numpy(), 1, -1))


def check_maxpool(be, dims, C):
    x = pool_input(dims, C)
    xt = ncdhw(x).requires_grad_(True)
    yt, it = F.max_pool3d(xt, 3, 2, 1, return_indices=True)
    y, arg = be.maxpool_fwd(x)
    assert bits_equal(y, ndhwc(yt.detach())), "values"
    assert np.array_equal(arg, ndhwc(it)), "indices"
    if isinstance(be, Device):
        y2, none = be.maxpool_fwd(x, with_arg=False)
        assert none is None and bits_equal(y2, y)
    dy = f32(np.random.default_rng(C).integers(-3, 4, y.shape))
    (dxt,) = torch.autograd.grad(yt, xt, ncdhw(dy))
    assert bits_equal(be.maxpool_bwd(dy, arg, dims), ndhwc(dxt)), "dx"


def check_shortcut(be, dims, C, stride, C_out):
    x = f32(np.random.default_rng(C + stride).standard_normal((2, *dims, C)))
    yt = F.avg_pool3d(ncdhw(x), 1, stride)
    ref = np.zeros((*ndhwc(yt).shape[:-1], C_out), F32)
    ref[..., :C] = ndhwc(yt)
    assert bits_equal(be.shortcut_a(x, stride, C_out), ref)


@pytest.mark.parametrize("dims", POOL_DIMS)
@pytest.mark.parametrize("C", [3, 8, 64])
def test_maxpool(dev, dims, C):
    check_maxpool(dev, dims, C)


@pytest.mark.parametrize("dims", POOL_DIMS)
@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("wide", [1, 2])
def test_shortcut_a(dev, dims, C, stride, wide):
    check_shortcut(dev, dims, C, stride, C * wide)


@pytest.mark.parametrize("S", [1, 3, 49, 784])
@pytest.mark.parametrize("B,C", [(3, 20), (5, 132)])
def test_avgpool(dev, S, B, C):
    assert (B * C // 4) % 64                              # 15 lanes of one block; 165 = two blocks and 37 lanes of a third
    rng = np.random.default_rng(S)
    inv = F32(1) / F32(S)
    # integer-valued x: the float32 sum is exact; sum * float32(1 / S) is two roundings from the float64 mean
    x = f32(rng.integers(-8, 9, (B, S, C)))
    y = dev.nan(B, C)
    dev.run("slic_avgpool_fwd", dev.up(x), B, S, C, y)
    assert ulps(y.cpu().numpy(), x.astype(np.float64).mean(1).astype(F32)).max() <= 2
    # random x: S 2^-24 mean|x| for the S - 1 float32 additions and the product
    x = f32(rng.standard_normal((B, S, C)))
    dev.run("slic_avgpool_fwd", dev.up(x), B, S, C, y)
    err = np.abs(y.cpu().numpy() - x.astype(np.float64).mean(1))
    assert np.all(err <= S * 2.0 ** -24 * np.abs(x.astype(np.float64)).mean(1))
    dy = f32(rng.standard_normal((B, C)))
    dx = dev.nan(B, S, C)
    dev.run("slic_avgpool_bwd", dev.up(dy), B, S, C, dx)
    assert bits_equal(dx.cpu().numpy(), np.broadcast_to((dy * inv)[:, None, :], (B, S, C)))


@pytest.mark.parametrize("M", [1, 7, 4096])
@pytest.mark.parametrize("C", [1, 5, 64, 130])
def test_colsum(dev, M, C):
    """within one float32 step of the float64 column sum, plus 1e-12 sum|x| for the double accumulation"""
    x = f32(np.random.default_rng(M * C).standard_normal((M, C)) * 3)
    out = dev.nan(C)
    dev.run("slic_colsum", dev.up(x), M, C, out)
    ref = x.astype(np.float64).sum(0)
    got = out.cpu().numpy().astype(np.float64)
    step = np.spacing(np.abs(ref).astype(F32)).astype(np.float64)
    assert np.all(np.abs(got - ref) <= step + 1e-12 * np.abs(x.astype(np.float64)).sum(0))

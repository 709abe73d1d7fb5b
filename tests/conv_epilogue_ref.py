"""The fused epilogue of the gather-GEMM kernels (csrc/conv_epilogue.h; the contract is SlicConvArgs in include/slic_hip.h) as ONE plain
numpy float64 function, and the cases test_conv_epilogue_cpu.py / test_conv_epilogue_gpu.py run it on.

    v      = acc + bias
    stat   = per block of tile_m consecutive GEMM rows: (sum v, sum (v - mean_blk)^2)             -- of acc + bias, NOT of the stored value
    out    = v * scale + shift + addend;  out = where(mask > 0, out, 0);  out = max(out, 0) if relu
    bwd    = per block: (sum out, sum out * (z - mean) * invstd)                                    -- of the STORED value
    dst[row(m)] = out[m];  addend / mask / z are addressed like dst;  a missing scale is 1, a missing bias / shift / addend is 0

Exact data.  The cases hold small integers and binary fractions (the pattern of test_bwd_integer_data_is_exact in test_bn_pool_gpu.py): every
product, sum and PARTIAL sum of the epilogue, in whatever order a kernel adds them, is a float32 number, so the device result has to
equal the float64 one bit for bit.  test_conv_epilogue_cpu.py proves that per case from the `trace` the reference fills: pointwise
intermediates equal their own float32 rounding (is_f32), and the terms of every sum are multiples of one power of two q with
sum |terms| <= 2^24 q per block and column (sums_exact) -- then no order of additions, and no fused multiply-add, can round.

  * forward-type cases (make_case): x, W in {-1, +1} with the last input channel of x zero, so acc is a sum of an ODD number of +-1: an odd
    integer, never 0.  bias and addend are odd multiples of 1/4 (acc + bias and acc + addend are never 0 either), shift a multiple of 1/4,
    scale a non-zero multiple of 1/2 of either sign, z and mean multiples of 1/2, invstd a power of two.
  * data-gradient cases (dgrad_case): dz, W in {-1, 0, 1}; at most 8 taps x 32 channels, so |acc| <= 256 and the 64-row sums of
    out * xhat stay below 2^24 sixteenths.

The one quantity that cannot be exact is sum (v - mean_blk)^2: 1 / rows is no float32 number for a ragged block and the squares of
v - mean need more than 24 bits.  It alone is held to the derived bound m2_bound() instead.

Masks hold +0.0, -0.0, negative values and NaN (all of them zero the element) beside positive values.  For the sets with the backward
sums the mask is mask_bwd: the same, except that every column of every block of 64 rows that has at least two rows keeps one positive
row -- a column whose rows are all masked has backward sums (0, 0) by definition, which would hide a slab row that was never written.
In a ONE-row block (M = 1, 65, 129) the masked columns are meant to be (0, 0): the mask is left as drawn there."""
import functools
import itertools

import numpy as np

# |got - ref| <= M2_FACTOR * (rows + 8) * 2^-24 * ref for sum (v - mean_blk)^2 over a block of `rows` real rows.  Derivation: the float32
# mean differs from the true one by at most 2 ulp, which moves the sum by rows * delta^2 (the cross term vanishes) -- far below one ulp
# of it; each term (v - mean)^2 carries three roundings (difference, product, its addition: 3 * 2^-24 relative) and the at most 128
# non-negative terms are added in some order with at most rows - 1 further roundings of a partial sum that never exceeds the total:
# (rows + 2) * 2^-24 relative in first order.  rows + 8 and the factor 2 leave room for the second-order terms.  The factor was NOT widened:
# test_conv_epilogue_cpu.py::test_m2_bound_holds_in_float32 shows a float32 evaluation of the two-pass formula inside it for every case.
M2_FACTOR = 2.0


def m2_bound(rows, ref):
    return M2_FACTOR * (np.asarray(rows, np.float64) + 8.0) * 2.0 ** -24 * np.asarray(ref, np.float64)


def f64(a):
    return np.asarray(a, np.float64)


def is_f32(a):
    """every element equals its own float32 rounding"""
    a = f64(a)
    return bool(np.array_equal(a.astype(np.float32).astype(np.float64), a))


def block_starts(M, tile_m):
    starts = np.arange(0, M, tile_m)
    return starts, np.minimum(tile_m, M - starts)


def sums_exact(terms, starts):
    """every partial sum of a block's terms, in ANY order and grouping, is a float32 number: the terms are multiples of one power of
    two q = 2^-k and the block's sum of |terms| is at most 2^24 q"""
    t = f64(terms)
    for k in range(13):
        s = t * 2.0 ** k
        if np.array_equal(np.round(s), s):
            return bool((np.add.reduceat(np.abs(s), starts, axis=0) <= 2.0 ** 24).all())
    return False


def dst_row_map(B, G, D, d, e):
    """GEMM row m = ((b Ga + ga) Gb + gb) Gc + gc  ->  dst row ((b Da + ga da + ea) Db + gb db + eb) Dc + gc dc + ec"""
    b, ga, gb, gc = np.meshgrid(np.arange(B), np.arange(G[0]), np.arange(G[1]), np.arange(G[2]), indexing="ij")
    return ((((b * D[0] + ga * d[0] + e[0]) * D[1] + gb * d[1] + e[1]) * D[2]) + gc * d[2] + e[2]).reshape(-1)


def epilogue_ref(acc, tile_m, bias=None, scale=None, shift=None, addend=None, mask=None, relu=False, bwd=None, rows=None, trace=None):
    """acc [M, N] -> (out [M, N], stat [R, 2, N], bwd sums [R, 2, N] or None), all float64; R = ceil(M / tile_m).
    addend, mask and z = bwd[0] are [dst rows, N] in dst addressing; rows[m] = dst row of GEMM row m (None: dst row = m), and out[m] is
    what dst[rows[m]] receives.  bwd = (z, mean [N], invstd [N]).  trace: a dict that receives the intermediates, for the exactness proof:
    trace["pointwise"] = [(name, array)], trace["sums"] = [(name, terms [M, N], block starts)]."""
    acc = f64(acc)
    M, N = acc.shape
    rows = np.arange(M) if rows is None else np.asarray(rows)
    starts, cnt = block_starts(M, tile_m)
    v = acc + (0.0 if bias is None else f64(bias))
    s = np.add.reduceat(v, starts, axis=0)
    dev = v - np.repeat(s / cnt[:, None], cnt, axis=0)
    stat = np.stack([s, np.add.reduceat(dev * dev, starts, axis=0)], axis=1)
    t_scale = v * (1.0 if scale is None else f64(scale))
    t_shift = t_scale + (0.0 if shift is None else f64(shift))
    t_add = t_shift + (0.0 if addend is None else f64(addend)[rows])
    out = t_add
    if mask is not None:
        out = np.where(f64(mask)[rows] > 0, out, 0.0)          # False for +0.0, -0.0, negatives and NaN
    if relu:
        out = np.maximum(out, 0.0)
    out = out + 0.0                                             # the kernel always adds shift and addend (0 when absent): no -0.0 survives
    if trace is not None:
        trace["pointwise"] = [("acc", acc), ("acc + bias", v), ("v * scale", t_scale), ("+ shift", t_shift), ("+ addend", t_add), ("out", out)]
        trace["sums"] = [("sum v", v, starts)]
    bsum = None
    if bwd is not None:
        z, mean, invstd = bwd
        centred = f64(z)[rows] - f64(mean)
        xhat = centred * f64(invstd)
        prod = out * xhat
        # + 0.0: a sum starts from +0.0, so a block whose only terms are 0 * (negative xhat) = -0.0 still adds up to +0.0
        bsum = np.stack([np.add.reduceat(out, starts, axis=0), np.add.reduceat(prod, starts, axis=0)], axis=1) + 0.0
        if trace is not None:
            trace["pointwise"] += [("z - mean", centred), ("xhat", xhat), ("out * xhat", prod)]
            trace["sums"] += [("sum out", out, starts), ("sum out * xhat", prod, starts)]
    return out, stat, bsum


def m2_float32(v, tile_m):
    """sum (v - mean_blk)^2 per block by the kernel's two-pass formula in float32: mean = sum * (1.0f / rows), squares added row by row"""
    v = np.asarray(v, np.float32)
    starts, cnt = block_starts(v.shape[0], tile_m)
    out = np.zeros((len(starts), v.shape[1]), np.float32)
    for i, (r0, n) in enumerate(zip(starts, cnt)):
        blk = v[r0:r0 + n]
        t = np.zeros(v.shape[1], np.float32)
        for r in range(n):
            t = t + blk[r]
        mean = t * (np.float32(1.0) / np.float32(n))
        q = np.zeros(v.shape[1], np.float32)
        for r in range(n):
            d = blk[r] - mean
            q = q + d * d
        out[i] = q
    return out


# ---- operand sets -------------------------------------------------------------------------------------------------------------------
ALL5 = ("bias", "scale", "shift", "addend", "relu")
OPERAND_SETS = [
    ("none", ()),
    ("bias", ("bias",)),
    ("scale", ("scale",)),
    ("shift", ("shift",)),
    ("scale+shift", ("scale", "shift")),
    ("addend", ("addend",)),
    ("relu", ("relu",)),
    ("addend=dst", ("addend", "alias")),
    ("all5", ALL5),
    ("stat", ("stat",)),
    ("stat+bias", ("stat", "bias")),
    ("stat+all5", ("stat",) + ALL5),
    ("mask", ("mask",)),
    ("mask+addend", ("mask", "addend")),
    ("mask+relu", ("mask", "relu")),
    ("bwd+mask+addend", ("bwd", "mask", "addend")),
    ("bwd", ("bwd",)),
]

# ---- shapes -------------------------------------------------------------------------------------------------------------------------
MS = (1, 63, 64, 65, 127, 128, 129, 581)      # 581: ten 64-row (five 128-row) blocks, so the DMA launches' grids of 16 (8) hold empty blocks
NS = (4, 8, 36, 64, 68, 104, 132)
# (M, N, ldo): every M at N = 36 and 68, every N at M = 65 and 129, ldo = N + 12 at three pairs
SHAPES = ([(M, N, N) for M in MS for N in (36, 68)] + [(M, N, N) for N in NS if N not in (36, 68) for M in (65, 129)] +
          [(65, 36, 48), (129, 132, 144), (581, 68, 80)])
KERNEL_C = {0: 16, 20: 32, 22: 64}            # launch variant -> input channels of its cases
TILE_M = {0: 64, 20: 64, 22: 128}
TAIL_C = 128                                   # four k-tiles of 32
TAIL_SHAPES = [(129, 36, 36), (129, 68, 80), (581, 132, 144)]
TAIL_PLANS = ("(0, 2)", "(1, 3)", "last")     # (nfull_rb, splits); "last": every row block but the last whole, the last cut in two

MASK_POS = np.array([1.0, 0.5, 3.0], np.float32)
MASK_OFF = np.array([0.0, -0.0, -1.0, -0.25, np.nan], np.float32)


def draw_mask(rng, shape):
    """a third of the elements is zeroed: by +0.0, -0.0, a negative value or NaN in equal shares"""
    off = rng.random(shape) < 1.0 / 3.0
    return np.where(off, rng.choice(MASK_OFF, shape), rng.choice(MASK_POS, shape)).astype(np.float32)


def keep_one_row(mask, starts, cnt):
    """mask with one positive row in every column of every block of at least two rows"""
    mask = mask.copy()
    for r0, n in zip(starts, cnt):
        if n >= 2:
            dead = ~(mask[r0:r0 + n] > 0).any(axis=0)
            mask[r0, dead] = 1.0
    return mask


def odd_quarters(rng, lim, shape):
    return ((2 * rng.integers(-lim, lim, shape) + 1) / 4.0).astype(np.float32)


def _draw_case(C, M, N, seed):
    rng = np.random.default_rng(seed)
    x = rng.choice(np.array([-1.0, 1.0], np.float32), (M, C))
    x[:, C - 1] = 0.0
    c = dict(C=C, M=M, N=N, seed=seed, x=x, W=rng.choice(np.array([-1.0, 1.0], np.float32), (N, C)))
    c["bias"] = odd_quarters(rng, 4, N)
    c["scale"] = rng.choice(np.array([-2.0, -1.5, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0], np.float32), N)
    c["shift"] = (rng.integers(-8, 9, N) / 4.0).astype(np.float32)
    c["addend"] = odd_quarters(rng, 4 * int(np.sqrt(C)), (M, N))
    c["mask"] = draw_mask(rng, (M, N))
    c["mask_bwd"] = keep_one_row(c["mask"], *block_starts(M, 64))
    c["z"] = (rng.integers(-4, 5, (M, N)) / 2.0).astype(np.float32)
    c["mean"] = (rng.integers(-2, 3, N) / 2.0).astype(np.float32)
    c["invstd"] = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), N)
    c["acc"] = f64(x) @ f64(c["W"]).T
    return c


def case_ref(c, ops, tile_m, trace=None):
    """the reference on a forward-type case (dst row = GEMM row) for one operand set"""
    mask = None
    if "mask" in ops:
        mask = c["mask_bwd"] if "bwd" in ops else c["mask"]
    return epilogue_ref(c["acc"], tile_m, bias=c["bias"] if "bias" in ops else None, scale=c["scale"] if "scale" in ops else None,
                        shift=c["shift"] if "shift" in ops else None, addend=c["addend"] if "addend" in ops else None, mask=mask,
                        relu="relu" in ops, bwd=(c["z"], c["mean"], c["invstd"]) if "bwd" in ops else None, trace=trace)


def one_row_masked(mask, M, tile_m):
    """[R, N]: True where a block has ONE row and the mask zeroes it in that column (backward sums (0, 0) by definition)"""
    starts, cnt = block_starts(M, tile_m)
    return (cnt == 1)[:, None] & ~(mask[starts] > 0)


def caps_violations(c, tile_m):
    """the conditions that keep a forward-type case from being trivial -> list of violations (empty: all hold)"""
    bad = []
    for name, ops in OPERAND_SETS:
        tr = {}
        out, stat, bsum = case_ref(c, ops, tile_m, tr)
        pre = dict(tr["pointwise"])["+ addend"]
        if "mask" in ops:
            m = c["mask_bwd"] if "bwd" in ops else c["mask"]
            share = 1.0 - (m > 0).mean()
            if "bwd" not in ops and not 0.25 <= share <= 0.75:
                bad.append(f"{name}: the mask zeroes {share:.0%}")
            pre = np.where(m > 0, pre, 0.0)
        if "relu" in ops:
            share = (pre < 0).mean()
            if not 0.25 <= share <= 0.75:
                bad.append(f"{name}: ReLU clips {share:.0%}")
        if "stat" in ops and ((stat[:, 0] == 0) & (stat[:, 1] == 0)).any():
            bad.append(f"{name}: a column of a block has statistics (0, 0)")
        if "bwd" in ops:
            zero = (bsum[:, 0] == 0) & (bsum[:, 1] == 0)
            if "mask" in ops:
                zero &= ~one_row_masked(c["mask_bwd"], c["M"], tile_m)
            if zero.any():
                bad.append(f"{name}: a column of a block has backward sums (0, 0)")
    return bad


@functools.lru_cache(maxsize=None)
def make_case(C, M, N):
    """the forward-type case of (C, M, N): the first seed of a fixed sequence whose draw meets caps_violations at both tile sizes (the caps
    are conditions on the inputs; nothing here looks at a device result)"""
    for k in range(64):
        c = _draw_case(C, M, N, 1000003 * k + 4099 * C + 131 * M + N)
        if not caps_violations(c, 64) and not caps_violations(c, 128):
            return c
    raise AssertionError(f"no seed meets the caps at C={C} M={M} N={N}")


# ---- the stride-2 data gradient ---------------------------------------------------------------------------------------------------------
DGRAD_DIMS, DGRAD_B, DGRAD_CIN = (3, 5, 7), 2, 12          # odd sizes: the parity classes have grids of unequal size
DGRAD_KINDS = {"3x3x3": ((3, 3, 3), (1, 1, 1)), "1x1x1": ((1, 1, 1), (0, 0, 0))}      # kernel, pad; stride 2 in every dimension


def _pad8(n):
    return (n + 7) // 8 * 8


def dgrad_classes(kernel, pad, in_dims, nout, stride=(2, 2, 2)):
    """the parity classes of the data gradient in LAUNCH order (descending nchunks, ties in product order): dicts cls, grid, ntaps, nchunks"""
    out = []
    for cls in itertools.product(*[range(s) for s in stride]):
        grid = tuple((d - p + s - 1) // s for d, p, s in zip(in_dims, cls, stride))
        if min(grid) <= 0:
            continue
        ntaps = int(np.prod([sum((cls[i] + pad[i] - d) % stride[i] == 0 for d in range(kernel[i])) for i in range(3)]))
        out.append(dict(cls=cls, grid=grid, ntaps=ntaps, nchunks=_pad8(ntaps * (nout // 4)) if ntaps else 0))
    return sorted(out, key=lambda d: -d["nchunks"])


@functools.lru_cache(maxsize=None)
def dgrad_case(kind, nout):
    kernel, pad = DGRAD_KINDS[kind]
    B, dims, cin = DGRAD_B, DGRAD_DIMS, DGRAD_CIN
    odims = tuple((i + 2 * p - k) // 2 + 1 for i, p, k in zip(dims, pad, kernel))
    classes = dgrad_classes(kernel, pad, dims, nout)
    P = B * int(np.prod(dims))
    for k in range(64):
        rng = np.random.default_rng(7919 * k + 31 * nout + kernel[0])
        ints = np.array([-1.0, 0.0, 1.0], np.float32)
        c = dict(kind=kind, kernel=kernel, pad=pad, dims=dims, odims=odims, B=B, cin=cin, nout=nout, classes=classes,
                 dz=rng.choice(ints, (B,) + odims + (nout,)), W=rng.choice(ints, (nout, cin) + kernel))
        c["addend"] = odd_quarters(rng, 12, (P, cin))
        mask = draw_mask(rng, (P, cin))
        for dc in classes:                                  # one positive row per column of every block of every class
            rows = class_rows(c, dc)
            sub = keep_one_row(mask[rows], *block_starts(len(rows), 64))
            mask[rows] = sub
        c["mask"] = mask
        c["z"] = (rng.integers(-4, 5, (P, cin)) / 2.0).astype(np.float32)
        c["mean"] = (rng.integers(-2, 3, cin) / 2.0).astype(np.float32)
        c["invstd"] = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), cin)
        c["full"] = dgrad_full(c)
        if not dgrad_caps_violations(c):
            return c
    raise AssertionError(f"no seed meets the caps for the {kind} data gradient at {nout} channels")


def class_rows(c, dc):
    return dst_row_map(c["B"], dc["grid"], c["dims"], (2, 2, 2), dc["cls"])


def dgrad_full(c):
    """float64 conv_transpose3d of dz: [B T H W, cin], rows in NDHWC order"""
    import torch
    import torch.nn.functional as F
    dz = torch.from_numpy(f64(c["dz"])).permute(0, 4, 1, 2, 3)
    full = F.conv_transpose3d(dz, torch.from_numpy(f64(c["W"])), None, 2, c["pad"])
    assert tuple(full.shape[2:]) == c["dims"]
    return full.permute(0, 2, 3, 4, 1).reshape(-1, c["cin"]).numpy()


def dgrad_ref(c, fused, trace=None):
    """-> (dx [B T H W, cin] float64, bwd slab [sum of the classes' blocks, 2, cin] in launch order or None); fused: addend + mask + bwd.
    trace: a list that receives one trace dict per class"""
    dx = np.full(c["full"].shape, np.nan)
    slabs = []
    for dc in c["classes"]:
        rows = class_rows(c, dc)
        tr = {} if trace is not None else None
        kw = dict(addend=c["addend"], mask=c["mask"], bwd=(c["z"], c["mean"], c["invstd"])) if fused else {}
        out, _, bsum = epilogue_ref(c["full"][rows], 64, rows=rows, trace=tr, **kw)
        dx[rows] = out
        if fused:
            slabs.append(bsum)
        if trace is not None:
            trace.append(tr)
    assert not np.isnan(dx).any(), "the classes cover every position once"
    return dx, (np.concatenate(slabs) if fused else None)


def dgrad_caps_violations(c):
    bad = []
    share = 1.0 - (c["mask"] > 0).mean()
    if not 0.25 <= share <= 0.75:
        bad.append(f"the mask zeroes {share:.0%}")
    r0 = 0
    _, slab = dgrad_ref(c, True)
    for dc in c["classes"]:
        r = -(-c["B"] * int(np.prod(dc["grid"])) // 64)
        blk = slab[r0:r0 + r]
        r0 += r
        if ((blk[:, 0] == 0) & (blk[:, 1] == 0)).any():
            bad.append(f"class {dc['cls']}: a column of a block has backward sums (0, 0)")
    if c["kind"] == "3x3x3" and any(dc["ntaps"] == 0 for dc in c["classes"]):
        bad.append("a 3x3x3 class without a tap")
    return bad

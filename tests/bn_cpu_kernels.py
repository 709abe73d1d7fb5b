"""NumPy restatement of csrc/bn.hip for the tests (not a product fallback): the BatchNorm statistics tree, the rank-order merge of
SyncBatchNorm, the two backward passes, the stem max-pool (forward and gather-form backward) and shortcut 'A' in the device's own
order of operations and number formats (float32 where the kernel holds a float, float64 where it holds a double), plus the flat
float64 reference of the statistics.  What a compiler may contract into an FMA on the device (g * xhat + s2, z * scale + shift,
the double bracket of pass 2) is written here as a product and a sum: the two differ by one rounding of the product.

Every function takes `mut`, a set of names of deliberate defects (tests/test_bn_pool_cpu.py: the mutation table); the product code
has none of them and the default is the empty set:
  ragged_full   the ragged last slab row counted as a full one
  chain_order   the sub-chains of a group merged 0, 3, 2, 1
  no_guard      the `n_b > 0` guard of the Chan merges removed
  swap_var      unbiased variance into invstd, biased into the running update
  swap_momentum (1 - momentum) and momentum exchanged
  rows_l        a level's rows_l not multiplied by BN_MG
  skip_tail     pass 1 without the loop that takes the last r1 - r rows after the four-way unrolled one
  ge            `>=` for `>` in the ReLU mask and in the max-pool comparison
  border_clamp  a max-pool window position outside the input read at the clamped position instead of skipped
  stride_2axes  shortcut 'A' striding t and h only"""
import itertools

import numpy as np

BN_MG = 64                    # slab rows per merge group
BN_MQ = 4                     # sub-chains per group
SUB = BN_MG // BN_MQ
BNB_RB = 256                  # rows per pass-1 workgroup (slic_bn_bwd_rows_per_partial)
F32 = np.float32


# ------------------------------------------------------------------ statistics
def _chan(st, nb, mb, m2b, sb, on):
    """one Chan update of (n, mean, M2, sum) with a block (nb, mean mb, M2 m2b, sum sb), where `on`"""
    n, mean, m2, s = st
    with np.errstate(all="ignore"):
        d = mb - mean
        nn = n + nb
        m2n = m2 + (m2b + d * d * n * nb / nn)
        meann = mean + d * nb / nn
    return np.where(on, nn, n), np.where(on, meann, mean), np.where(on, m2n, m2), np.where(on, s + sb, s)


def _merge_groups(x, rows_in, M, mut):
    """bn_merge_level / the merge part of bn_merge_final: x [R, 2, C] -> per group (n, mean, M2, sum), each [G, C] float64"""
    R, _, C = x.shape
    G = -(-R // BN_MG)
    pad = np.zeros((G * BN_MG, 2, C), np.float64)
    pad[:R] = x
    r = np.arange(G * BN_MG, dtype=np.int64)
    nb = np.minimum(rows_in, M - r * rows_in).astype(np.float64)
    if "ragged_full" in mut:
        nb[:] = rows_in
    valid = (r < R).reshape(G, BN_MQ, SUB, 1)
    nb = nb.reshape(G, BN_MQ, SUB, 1)
    pad = pad.reshape(G, BN_MQ, SUB, 2, C)
    st = tuple(np.zeros((G, BN_MQ, C)) for _ in range(4))
    for j in range(SUB):                                  # the BN_MQ chains of every group advance together, rows in order
        sb = pad[:, :, j, 0]
        with np.errstate(all="ignore"):
            mb = sb / nb[:, :, j]
        st = _chan(st, nb[:, :, j], mb, pad[:, :, j, 1], sb, valid[:, :, j])
    acc = tuple(a[:, 0] for a in st)
    for u in ((3, 2, 1) if "chain_order" in mut else (1, 2, 3)):
        nbu = st[0][:, u]
        on = np.ones_like(nbu, bool) if "no_guard" in mut else nbu > 0.0
        acc = _chan(acc, nbu, st[1][:, u], st[2][:, u], st[3][:, u], on)
    return acc


def _levels(slab, rows, M, mut):
    """run_merge<true>: levels until at most BN_MG rows are left (float at level 0, double above)"""
    x = np.asarray(slab, F32)
    rows_l = int(rows)
    while x.shape[0] > BN_MG:
        _, _, m2, s = _merge_groups(x, rows_l, M, mut)
        x = np.stack([s, m2], 1)
        if "rows_l" not in mut:
            rows_l *= BN_MG
    return x, rows_l


def _finish(mu, m2, n, eps, momentum, gamma, beta, running_mean, running_var, mut):
    eps, momentum = F32(eps), F32(momentum)
    var = np.maximum(m2 / n, 0.0) if n > 0 else np.zeros_like(m2)
    unb = var * (n / (n - 1.0)) if n > 1 else var
    if "swap_var" in mut:
        var, unb = unb, var
    C = mu.shape[0]
    inv = (1.0 / np.sqrt(var + np.float64(eps))).astype(F32)
    g = np.ones(C, F32) if gamma is None else np.asarray(gamma, F32)
    b = np.zeros(C, F32) if beta is None else np.asarray(beta, F32)
    sc = g * inv
    out = dict(mean=mu.astype(F32), invstd=inv, scale=sc, shift=b - mu.astype(F32) * sc)
    if running_mean is not None:
        keep, new = (momentum, F32(1) - momentum) if "swap_momentum" in mut else (F32(1) - momentum, momentum)
        out["running_mean"] = keep * np.asarray(running_mean, F32) + new * mu.astype(F32)
        out["running_var"] = keep * np.asarray(running_var, F32) + new * unb.astype(F32)
    return out


def bn_finalize(slab, rows, M, eps, momentum, gamma=None, beta=None, running_mean=None, running_var=None, mut=()):
    """slic_bn_finalize: slab [R, 2, C] float32 of (sum, M2) over `rows` samples a row, the last row ragged"""
    x, rows_l = _levels(slab, rows, M, mut)
    _, _, m2, s = _merge_groups(x, rows_l, M, mut)
    return _finish(s[0] / float(M), m2[0], float(M), eps, momentum, gamma, beta, running_mean, running_var, mut)


def bn_merge_stats(slab, rows, M, mut=()):
    """slic_bn_merge_stats: the slab merged to one row, [2 C] float64 = (sum, M2)"""
    x, rows_l = _levels(slab, rows, M, mut)
    _, _, m2, s = _merge_groups(x, rows_l, M, mut)
    return np.concatenate([s[0], m2[0]])


def bn_finalize_sync(stats, C, eps, momentum, gamma=None, beta=None, running_mean=None, running_var=None, mut=()):
    """slic_bn_finalize_sync: stats [W, 2 C + 1] float64 = (sum, M2, n) per rank, merged in rank order; rows with n = 0 are passed over"""
    st = tuple(np.zeros(C) for _ in range(4))
    for row in np.asarray(stats, np.float64):
        nb = row[2 * C]
        on = True if "no_guard" in mut else nb > 0.0
        with np.errstate(all="ignore"):
            mb = row[:C] / nb
        st = _chan(st, nb, mb, row[C:2 * C], row[:C], on)
    n, mean, m2, _ = st
    n = float(np.max(n))
    return _finish(mean, m2, n, eps, momentum, gamma, beta, running_mean, running_var, mut)


def flat_stats(slab, rows, M):
    """float64 reference of the same slab: mean = sum_r sum_r / M, M2 = sum_r m2_r + sum_r n_r (sum_r / n_r - mean)^2"""
    x = np.asarray(slab, np.float64)
    R = x.shape[0]
    n = np.minimum(rows, M - np.arange(R, dtype=np.int64) * rows).astype(np.float64)[:, None]
    mean = x[:, 0].sum(0) / M
    m2 = x[:, 1].sum(0) + (n * (x[:, 0] / n - mean) ** 2).sum(0)
    return mean, m2


# ------------------------------------------------------------------ backward
def bn_bwd_pass1(dy, out, z, mean, invstd, mut=()):
    """bn_bwd_reduce_kernel: g = dy * (out > 0), partial [ceil(M / 256), 2, C] float32 of (sum g, sum g xhat).  Thread (rl, channel
    group) adds its rows rl, rl + RL, ... in float32; the RL thread sums are then added in order."""
    dy, z = np.asarray(dy, F32), np.asarray(z, F32)
    M, C = dy.shape
    g = dy
    if out is not None:
        keep = (np.asarray(out) >= 0) if "ge" in mut else (np.asarray(out) > 0)
        g = np.where(keep, dy, F32(0))
    xh = (z - np.asarray(mean, F32)) * np.asarray(invstd, F32)
    p = g * xh
    C4 = C // 4
    CG = min(C4, 256)
    RL = 256 // CG
    nblk = -(-M // BNB_RB)
    K = -(-BNB_RB // RL)
    k = np.arange(K)[:, None]
    i = k * RL + np.arange(RL)[None, :]                                   # row within the block of thread rl at step k
    idx = np.arange(nblk, dtype=np.int64)[:, None, None] * BNB_RB + i     # [nblk, K, RL]
    valid = (i < BNB_RB)[None] & (idx < M)
    if "skip_tail" in mut:
        cnt = valid.sum(1)
        valid = valid & (k[None] < 4 * (cnt // 4)[:, None, :])
    idx = np.minimum(idx, M - 1)
    s = np.zeros((2, nblk, RL, C), F32)
    for kk in range(K):
        v = valid[:, kk, :, None]
        s[0] = s[0] + np.where(v, g[idx[:, kk]], F32(0))
        s[1] = s[1] + np.where(v, p[idx[:, kk]], F32(0))
    acc = np.zeros((2, nblk, C), F32)
    for u in range(RL):
        acc = acc + s[:, :, u]
    return g, np.ascontiguousarray(acc.transpose(1, 0, 2))


def sum_tree(partial):
    """run_merge<false> + sum_merge_final: [R, 2, C] float32 -> [2, C] float64, groups of BN_MG rows as BN_MQ chains in row order"""
    x = np.asarray(partial, F32).astype(np.float64)
    while True:
        R, _, C = x.shape
        G = -(-R // BN_MG)
        pad = np.zeros((G * BN_MG, 2, C))
        pad[:R] = x
        pad = pad.reshape(G, BN_MQ, SUB, 2, C)
        ch = np.zeros((G, BN_MQ, 2, C))
        for j in range(SUB):
            ch = ch + pad[:, :, j]
        x = ch[:, 0]
        for u in range(1, BN_MQ):
            x = x + ch[:, u]
        if G == 1:
            return x[0]


def bn_bwd_pass2(g, z, mean, invstd, gamma, ka, kb):
    """bn_bwd_apply_kernel: dz = gamma invstd (g - ka - xhat kb), float32 xhat, the bracket and the products in double"""
    inv = np.asarray(invstd, F32)
    xh = (np.asarray(z, F32) - np.asarray(mean, F32)) * inv
    br = np.asarray(g, F32).astype(np.float64) - ka - xh.astype(np.float64) * kb
    return (np.asarray(gamma, F32).astype(np.float64) * inv.astype(np.float64) * br).astype(F32)


def bn_bwd(dy, out, z, mean, invstd, gamma, mut=()):
    """slic_bn_bwd -> g, dz, dgamma, dbeta"""
    g, part = bn_bwd_pass1(dy, out, z, mean, invstd, mut)
    a, b = sum_tree(part)
    M = dy.shape[0]
    return g, bn_bwd_pass2(g, z, mean, invstd, gamma, a / float(M), b / float(M)), b.astype(F32), a.astype(F32)


# ------------------------------------------------------------------ pools, shortcut
def _odim(n, s=2):
    return (n - 1) // s + 1


def maxpool3d_fwd(x, mut=()):
    """MaxPool3d(3, 2, 1) on NDHWC x [B, T, H, W, C]: windows scanned in (t, h, w) order, the first maximum wins, a NaN is taken
    and kept, arg = (t H + h) W + w of the winner -> y, arg [B, To, Ho, Wo, C]"""
    x = np.asarray(x, F32)
    B, T, H, W, C = x.shape
    To, Ho, Wo = _odim(T), _odim(H), _odim(W)
    best = np.full((B, To, Ho, Wo, C), -np.inf, F32)
    bi = np.full((B, To, Ho, Wo, C), -1, np.int32)
    for dt, dh, dw in itertools.product(range(3), repeat=3):
        t, h, w = 2 * np.arange(To) - 1 + dt, 2 * np.arange(Ho) - 1 + dh, 2 * np.arange(Wo) - 1 + dw
        ok = (((t >= 0) & (t < T))[:, None, None] & ((h >= 0) & (h < H))[None, :, None] & ((w >= 0) & (w < W))[None, None, :])
        if "border_clamp" in mut:
            ok = np.ones_like(ok)
        v = x[:, np.clip(t, 0, T - 1)][:, :, np.clip(h, 0, H - 1)][:, :, :, np.clip(w, 0, W - 1)]
        pos = ((t[:, None, None] * H + h[None, :, None]) * W + w[None, None, :]).astype(np.int32)[None, ..., None]
        with np.errstate(invalid="ignore"):
            better = (v >= best) if "ge" in mut else (v > best)
        take = ok[None, ..., None] & ((bi < 0) | better | (v != v))
        best = np.where(take, v, best)
        bi = np.where(take, pos, bi)
    return best, bi


def maxpool3d_bwd(dy, arg, dims):
    """gather form: dx[pos] = sum of dy over the (at most eight) windows that cover pos and chose it, windows in (t, h, w) order"""
    dy, arg = np.asarray(dy, F32), np.asarray(arg)
    T, H, W = dims
    B, To, Ho, Wo, C = dy.shape
    t, h, w = np.arange(T), np.arange(H), np.arange(W)
    pos = ((t[:, None, None] * H + h[None, :, None]) * W + w[None, None, :])[None, ..., None]
    dx = np.zeros((B, T, H, W, C), F32)
    for at, ah, aw in itertools.product(range(2), repeat=3):
        sel = []
        for p, a, no in ((t, at, To), (h, ah, Ho), (w, aw, Wo)):
            o = (p + a) >> 1                                   # a = 0: p >> 1; a = 1: (p + 1) >> 1, a second window only where it differs
            sel.append((np.minimum(o, no - 1), (o < no) & ((a == 0) | (o != p >> 1))))
        (ot, vt), (oh, vh), (ow, vw) = sel
        ok = (vt[:, None, None] & vh[None, :, None] & vw[None, None, :])[None, ..., None]
        a_ = arg[:, ot][:, :, oh][:, :, :, ow]
        d_ = dy[:, ot][:, :, oh][:, :, :, ow]
        dx = dx + np.where(ok & (a_ == pos), d_, F32(0))
    return dx


def shortcut_a(x, stride, C_out, mut=()):
    """F.avg_pool3d(x, 1, stride) — every stride-th position — then zero channels up to C_out; NDHWC"""
    x = np.asarray(x, F32)
    B, T, H, W, C = x.shape
    sw = 1 if "stride_2axes" in mut else stride
    to, ho, wo = np.arange(_odim(T, stride)) * stride, np.arange(_odim(H, stride)) * stride, np.arange(_odim(W, stride)) * sw
    y = np.zeros((B, len(to), len(ho), len(wo), C_out), F32)
    y[..., :C] = x[:, to][:, :, ho][:, :, :, wo]
    return y

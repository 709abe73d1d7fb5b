"""NumPy restatement of csrc/loss.hip and csrc/nce.hip for the tests (not a product fallback).

The three selection entry points are restated in the device's own order (64-column chunks, one column a lane, ballots as boolean
rows, the lowest index on ties), because their integer outputs are compared exactly.  Everything else is plain float32 NumPy
(float32 products, NumPy's own summation order) where the kernel holds a float and float64 where it holds a double: a different
order of the same float32 sums is what shows that a gate of tests/test_loss_kernels_gpu.py can be met by float32 arithmetic.

Every function takes `mut`, a set of names of deliberate defects (tests/test_loss_kernels_cpu.py: the mutation table); the product
code has none of them and the default is the empty set:
  sel_seen            the rank search restarts `seen` at each 64-column chunk
  sel_tie_last        ties of the arg-max / arg-min go to the higher index
  sel_ge              candidate test `>= 0`
  sel_fallback_row    the fallback returns the row, not the position in the negatives list
  sel_fallback_chunk  the fallback position counts the negatives of the first chunk only
  sel_label32         labels compared in their low 32 bits
  sel_anchor_label    the cross form takes col_labels[anchor_row]
  selk_no_skip        draws do not skip the positions taken already
  selk_no_topup       L = cnt_c, no top-up to K
  selk_status_all     one short pair blanks the whole call
  row_tail            `for (k = lane; k < D; k += 64)` loops stop at the last multiple of 64
  pd_eps_out          euclidean eps added outside the norm
  pd_clamp_prod       cosine clamp on the product of the norms
  hinge_ge            hinge active at v == 0
  gscale_ignored      a backward ignores gscale
  mean_n              a loss mean divides by n + 1
  ntx_diag_inf        NT-Xent diagonal dropped from the denominator
  ntx_target          target i + n/2 for i < n/2, i - n/2 beyond (the pair formula, no wrap): differs at odd n
  ntx_ld              lde / ldd taken as D
  eucl_dup            euclidean NT-Xent backward guards j != i instead of dist > 0
  eucl_256            euclidean NT-Xent sums exp over the first 256 columns only
  infonce_pos_twice   the positive counted among the negatives too
  nce_k_tail          the loop after the four-way unrolled one dropped (scores_bwd, fused_bwd)
  nce_d_slice         columns >= 128 of D dropped
  nce_grid_stride     scores_fwd writes the first 512 columns only
  nce_side            the two sides' features exchanged
  nce_idle_part       an idle part's (max, sum) formed and merged without the -inf guards
  nce_dup_first       fused update: the first of duplicate labels wins
  ce0_no_shift        log-sum-exp without the max shift"""
import numpy as np

F32 = np.float32
NONE = frozenset()
NCE_PARTS = 16
INFONCE_MAXY = 8
TSK_MAX = 8
CLAMP = F32(1e-8)


def _sum(a):
    return a.sum(-1, dtype=F32)


def _dk(D, mut):
    return D // 64 * 64 if "row_tail" in mut else D


def _mean(v, mut):
    """mean_serial: a double accumulator, one float32 rounding"""
    n = len(v) + (1 if "mean_n" in mut else 0)
    return F32(np.asarray(v, np.float64).sum() / n)


def _gs(gscale, mut):
    return F32(1) if gscale is None or "gscale_ignored" in mut else F32(gscale)


# ------------------------------------------------------------------ selection (the device's order)
def _labels(labels, mut):
    lab = np.asarray(labels, np.int64)
    return lab.astype(np.int32).astype(np.int64) if "sel_label32" in mut else lab


def _nth_set(mask, k):
    """index of the k-th set entry of a ballot"""
    return int(np.flatnonzero(mask)[k])


def triplet_select(Dm, labels, anc, anc_label, pos, margin, mode, u, mut=NONE):
    """triplet_select_kernel; anc_label None = slic_triplet_select, given = slic_triplet_select_cross"""
    Dm = np.asarray(Dm, F32)
    n = Dm.shape[1]
    lab = _labels(labels, mut)
    P = len(anc)
    neg = np.full(P, -7, np.int32)
    lanes = np.arange(64)
    last = "sel_tie_last" in mut
    for pr in range(P):
        a = int(anc[pr])
        if anc_label is None or "sel_anchor_label" in mut:
            la = lab[a]
        else:
            la = _labels(anc_label, mut)[pr]
        row = Dm[a]
        thr = F32(row[int(pos[pr])] + F32(margin))
        cnt_neg = cnt_c = 0
        best_loss, best_d = np.full(64, -np.inf, F32), np.full(64, np.inf, F32)
        best_loss_j, best_d_j = np.full(64, -1), np.full(64, -1)
        for j0 in range(0, n, 64):
            j = j0 + lanes
            ok = j < n
            jj = np.minimum(j, n - 1)
            isneg = ok & (lab[jj] != la)
            d = np.where(isneg, row[jj], F32(0))
            los = thr - d
            c = isneg & ((los >= 0) if "sel_ge" in mut else (los > 0))
            cnt_neg += int(isneg.sum())
            cnt_c += int(c.sum())
            up = isneg & ((los >= best_loss) if last else (los > best_loss))
            best_loss, best_loss_j = np.where(up, los, best_loss), np.where(up, j, best_loss_j)
            up = isneg & ((d <= best_d) if last else (d < best_d))
            best_d, best_d_j = np.where(up, d, best_d), np.where(up, j, best_d_j)

        def across(val, idx, sign):
            """the xor butterfly: the better value, on a tie the lower (mutant: higher) index"""
            have = idx >= 0
            if not have.any():
                return -1
            v = sign * val[have]
            tied = idx[have][v == v.max()]
            return int(tied.max() if last else tied.min())
        bl_j, bd_j = across(best_loss, best_loss_j, 1), across(best_d, best_d_j, -1)
        result = -1
        want = cnt_neg if mode == 0 else cnt_c
        if mode == 3:
            pass
        elif mode == 2:
            if cnt_c > 0:
                result = bl_j
        elif want > 0:
            rsel = min(int(F32(u[pr]) * F32(want)), want - 1)
            seen = 0
            for j0 in range(0, n, 64):
                j = j0 + lanes
                ok = j < n
                jj = np.minimum(j, n - 1)
                isneg = ok & (lab[jj] != la)
                los = thr - row[jj]
                c = isneg if mode == 0 else isneg & ((los >= 0) if "sel_ge" in mut else (los > 0))
                pc = int(c.sum())
                if seen + pc > rsel:
                    result = j0 + _nth_set(c, rsel - seen)
                    break
                seen = 0 if "sel_seen" in mut else seen + pc
        if result < 0:
            if "sel_fallback_row" in mut:
                result = bd_j
            else:
                stop = min(bd_j, 64) if "sel_fallback_chunk" in mut else bd_j
                result = int((lab[:max(stop, 0)] != la).sum())
        neg[pr] = result
    return neg


def triplet_select_k(Dm, labels, anc, pos, margin, K, u, mut=NONE):
    """triplet_select_k_kernel -> (neg [P, K], status)"""
    Dm = np.asarray(Dm, F32)
    n = Dm.shape[1]
    lab = _labels(labels, mut)
    P = len(anc)
    u = np.asarray(u, F32).reshape(P, K)
    neg = np.full((P, K), -7, np.int32)
    status = 0
    for pr in range(P):
        a = int(anc[pr])
        la = lab[a]
        row = Dm[a]
        thr = F32(row[int(pos[pr])] + F32(margin))
        isneg = lab != la
        los = thr - row
        cnt_neg = int(isneg.sum())
        cnt_c = int((isneg & ((los >= 0) if "sel_ge" in mut else (los > 0))).sum())
        if cnt_neg < K:
            status = 1
            neg[pr] = -1
            continue
        L = cnt_c if "selk_no_topup" in mut else max(cnt_c, K)
        taken = []
        chosen = []
        for t in range(K):
            rsel = min(int(u[pr, t] * F32(L - t)), L - t - 1)
            if "selk_no_skip" not in mut:
                for q in sorted(taken):
                    if rsel >= q:
                        rsel += 1
            chosen.append(rsel)
            taken.append(rsel)
        seen = 0
        for j0 in range(0, n, 64):                        # position in the negatives list -> row, chunk by chunk
            m = isneg[j0:j0 + 64]
            pc = int(m.sum())
            for t in range(K):
                rk = chosen[t] - seen
                if 0 <= rk < pc:
                    neg[pr, t] = j0 + _nth_set(m, rk)
            seen += pc
    if status and "selk_status_all" in mut:
        neg[:] = -1
    return neg, status


# ------------------------------------------------------------------ rowwise distances
def _pd(x, y, euclid, eps, mut):
    """distance along the last axis (broadcasting): slic_pd_step / _wave_sum / _finish"""
    k = _dk(x.shape[-1], mut)
    x, y = x[..., :k], y[..., :k]
    if euclid:
        if "pd_eps_out" in mut:
            d = x - y
            return np.sqrt(_sum(d * d)) + F32(eps)
        d = x - y + F32(eps)
        return np.sqrt(_sum(d * d))
    a, b, c = _sum(x * y), _sum(x * x), _sum(y * y)
    if "pd_clamp_prod" in mut:
        den = np.maximum(np.sqrt(b) * np.sqrt(c), CLAMP)
    else:
        den = np.maximum(np.sqrt(b), CLAMP) * np.maximum(np.sqrt(c), CLAMP)
    return F32(1) - a / den


def pair_distance(X, Y, euclid, mut=NONE):
    return _pd(X, Y, euclid, 1e-6, mut)


def pdist2(X, Y, eps, euclid, mut=NONE):
    return _pd(X[:, None, :], Y[None, :, :], euclid, eps, mut)


def pdist(V, eps, euclid, mut=NONE):
    return pdist2(V, V, eps, euclid, mut)


def pair_distance_bwd(X, Y, G, euclid, mut=NONE):
    n, D = X.shape
    k = _dk(D, mut)
    dX, dY = np.full((n, D), np.nan, F32), np.full((n, D), np.nan, F32)
    x, y = X[:, :k], Y[:, :k]
    with np.errstate(all="ignore"):
        if euclid:
            d = x - y if "pd_eps_out" in mut else x - y + F32(1e-6)
            dn = np.sqrt(_sum(d * d))
            inv = np.where(dn > 0, G / dn, F32(0)).astype(F32)
            v = d * inv[:, None]
            dX[:, :k], dY[:, :k] = v, -v
            return dX, dY
        a, b, c = _sum(x * y), _sum(x * x), _sum(y * y)
        rx, ry = np.sqrt(b), np.sqrt(c)
        nx, ny = np.maximum(rx, CLAMP), np.maximum(ry, CLAMP)
        inv = F32(1) / (np.maximum(rx * ry, CLAMP) if "pd_clamp_prod" in mut else nx * ny)
        cx = np.where(rx > CLAMP, a * inv / (nx * nx), F32(0)).astype(F32)
        cy = np.where(ry > CLAMP, a * inv / (ny * ny), F32(0)).astype(F32)
    g = G[:, None]
    dX[:, :k] = -g * (y * inv[:, None] - cx[:, None] * x)
    dY[:, :k] = -g * (x * inv[:, None] - cy[:, None] * y)
    return dX, dY


# ------------------------------------------------------------------ margin terms
def _active(v, mut):
    return ((v >= 0) if "hinge_ge" in mut else (v > 0)).astype(F32)


def margin_fwd(X, Y, Z, margin, euclid, mut=NONE):
    """-> state [n, 8] (the slots the kernel leaves alone stay NaN), rowloss [n], loss"""
    n, D = X.shape
    k = _dk(D, mut)
    x, y, z = X[:, :k], Y[:, :k], Z[:, :k]
    st = np.full((n, 8), np.nan, F32)
    if euclid:
        dy, dz = x - y + F32(1e-6), x - z + F32(1e-6)
        d1, d2 = np.sqrt(_sum(dy * dy)), np.sqrt(_sum(dz * dz))
        v = d1 - d2 + F32(margin)
        st[:, 0], st[:, 1] = d1, d2
    else:
        nx, ny, nz = (np.maximum(np.sqrt(_sum(t * t)), CLAMP) for t in (x, y, z))
        c1, c2 = _sum(x * y) / (nx * ny), _sum(x * z) / (nx * nz)
        v = (F32(1) - c1) - (F32(1) - c2) + F32(margin)
        st[:, 0], st[:, 1], st[:, 2], st[:, 3], st[:, 4] = c1, c2, nx, ny, nz
    st[:, 5] = _active(v, mut)
    rowloss = np.maximum(v, F32(0))
    return st, rowloss, _mean(rowloss, mut)


def margin_bwd(X, Y, Z, st, gscale, euclid, mut=NONE):
    n, D = X.shape
    k = _dk(D, mut)
    x, y, z = X[:, :k], Y[:, :k], Z[:, :k]
    out = [np.full((n, D), np.nan, F32) for _ in range(3)]
    g = (st[:, 5] * _gs(gscale, mut) / F32(n))[:, None]
    with np.errstate(all="ignore"):
        if euclid:
            d1, d2 = st[:, 0:1], st[:, 1:2]
            i1 = np.where(d1 > 0, g / d1, F32(0)).astype(F32)
            i2 = np.where(d2 > 0, g / d2, F32(0)).astype(F32)
            uy, uz = (x - y + F32(1e-6)) * i1, (x - z + F32(1e-6)) * i2
            out[0][:, :k], out[1][:, :k], out[2][:, :k] = uy - uz, -uy, uz
        else:
            c1, c2, nx, ny, nz = (st[:, i:i + 1] for i in range(5))
            dc1 = y / (nx * ny) - c1 * x / (nx * nx)
            dc2 = z / (nx * nz) - c2 * x / (nx * nx)
            out[0][:, :k] = g * (-dc1 + dc2)
            out[1][:, :k] = g * -(x / (nx * ny) - c1 * y / (ny * ny))
            out[2][:, :k] = g * (x / (nx * nz) - c2 * z / (nz * nz))
    return tuple(out)


# ------------------------------------------------------------------ InfoNCE over gathered rows
def infonce_rows_fwd(X, Y, T, mut=NONE):
    """X [P, D], Y [P, NY, D] -> state [P, 18], rowloss [P], loss"""
    P, NY, D = Y.shape
    k = _dk(D, mut)
    x, y = X[:, None, :k], Y[:, :, :k]
    inv_t = F32(1) / F32(T)
    st = np.full((P, 2 * INFONCE_MAXY + 2), np.nan, F32)
    nx = np.maximum(np.sqrt(_sum(x * x)), CLAMP)                      # [P, 1]
    ny = np.maximum(np.sqrt(_sum(y * y)), CLAMP)                      # [P, NY]
    c = _sum(x * y) / (nx * ny)
    e = np.exp((F32(1) - (F32(1) - c)) * inv_t)
    an = e[:, 1:].sum(-1, dtype=F32) + (e[:, 0] if "infonce_pos_twice" in mut else F32(0))
    Zs = an + e[:, 0]
    st[:, :NY], st[:, INFONCE_MAXY:INFONCE_MAXY + NY] = c, ny
    st[:, 2 * INFONCE_MAXY], st[:, 2 * INFONCE_MAXY + 1] = nx[:, 0], Zs
    rowloss = -np.log(e[:, 0] / Zs)
    return st, rowloss, _mean(rowloss, mut)


def infonce_rows_bwd(X, Y, st, T, gscale, mut=NONE):
    P, NY, D = Y.shape
    k = _dk(D, mut)
    x, y = X[:, None, :k], Y[:, :, :k]
    inv_t = F32(1) / F32(T)
    c, ny = st[:, :NY, None], st[:, INFONCE_MAXY:INFONCE_MAXY + NY, None]
    nx, Zs = st[:, 2 * INFONCE_MAXY, None, None], st[:, 2 * INFONCE_MAXY + 1, None, None]
    g = _gs(gscale, mut) / F32(P)
    pj = np.exp((F32(1) - (F32(1) - c)) * inv_t) / Zs
    pj[:, 0] -= F32(1)
    w = g * inv_t * pj
    dX, dY = np.full((P, D), np.nan, F32), np.full((P, NY, D), np.nan, F32)
    dX[:, :k] = (w * (y / (nx * ny) - c * x / (nx * nx))).sum(1, dtype=F32)
    dY[:, :, :k] = w * (x / (nx * ny) - c * y / (ny * ny))
    return dX, dY


# ------------------------------------------------------------------ NT-Xent, cosine
def _target(n, mut):
    i = np.arange(n)
    if "ntx_target" in mut:
        return np.where(i < n // 2, i + n // 2, i - n // 2)
    return (n // 2 + i) % n


def ntxent(Eflat, n, D, lde, T, gscale, ldd, mut=NONE):
    """slic_ntxent_fwd + slic_ntxent_bwd on a flat input of row stride lde -> loss, dE [n, ldd] (padding left NaN)"""
    if "ntx_ld" in mut:
        lde_r, ldd_w = D, D
    else:
        lde_r, ldd_w = lde, ldd
    E = np.stack([Eflat[i * lde_r:i * lde_r + D] for i in range(n)]).astype(F32)
    invT = F32(1) / F32(T)
    nrm = np.maximum(np.sqrt(_sum(E * E)), CLAMP)
    rn = F32(1) / nrm
    Eh = E / nrm[:, None]
    S = (Eh @ Eh.T).astype(F32)
    s = F32(1) - (F32(1) - S)
    np.fill_diagonal(s, F32(0))
    s = s * invT
    ex = np.exp(s - invT)
    if "ntx_diag_inf" in mut:
        np.fill_diagonal(ex, F32(0))
    lse = invT + np.log(_sum(ex))
    tgt = _target(n, mut)
    i = np.arange(n)
    rowloss = lse - s[i, tgt]
    loss = _mean(rowloss, mut)
    # backward
    onehot = np.zeros((n, n), F32)
    onehot[i, tgt] = 1
    Pm = np.exp(s - lse[:, None])
    H = (Pm - onehot) + (Pm.T - onehot.T)
    np.fill_diagonal(H, F32(0))
    gs = _gs(gscale, mut) * invT / F32(n)
    dh = (H @ Eh).astype(F32) * gs
    dot = _sum(dh * Eh)
    d = (dh - Eh * dot[:, None]) * rn[:, None]
    flat = np.full(n * ldd, np.nan, F32)
    for r in range(n):
        flat[r * ldd_w:r * ldd_w + D] = d[r]
    return loss, flat.reshape(n, ldd)


# ------------------------------------------------------------------ NT-Xent, euclidean
def ntxent_euclid_fwd(E, T, mut=NONE):
    """-> dist [n, n], wm [n, n], rowloss [n], loss"""
    n, D = E.shape
    invT = F32(1) / F32(T)
    diff = E[:, None, :] - E[None, :, :]
    dist = np.sqrt(_sum(diff * diff))
    sc = (F32(1) - dist) * invT
    np.fill_diagonal(sc, F32(0))
    m = sc.max(1)
    ex = np.exp(sc - m[:, None])
    if "eucl_256" in mut:
        ex = ex[:, :256]
    lse = m + np.log(_sum(ex))
    tgt = _target(n, mut)
    i = np.arange(n)
    rowloss = lse - sc[i, tgt]
    pj = np.exp(sc - lse[:, None])
    pj[i, tgt] -= F32(1)
    wm = -pj * invT
    np.fill_diagonal(wm, F32(0))
    return dist, wm.astype(F32), rowloss, _mean(rowloss, mut)


def ntxent_euclid_bwd(E, dist, wm, gscale, mut=NONE):
    n, D = E.shape
    g = _gs(gscale, mut) / F32(n)
    with np.errstate(all="ignore"):
        q = g * (wm + wm.T) / dist
    live = ~np.eye(n, dtype=bool) if "eucl_dup" in mut else dist > 0
    cf = np.where(live, q, F32(0)).astype(F32)
    diff = E[:, None, :] - E[None, :, :]
    with np.errstate(invalid="ignore"):
        return (cf[:, :, None] * diff).sum(1, dtype=F32)


# ------------------------------------------------------------------ memory-bank NCE
def _dn(D, mut):
    return min(D, 128) if "nce_d_slice" in mut else D


def _unrolled(K1, groups, mut):
    """the j a kernel visits: all, or (mutant) only those of the four-way unrolled loop of each of `groups` groups"""
    if "nce_k_tail" not in mut:
        return np.arange(K1)
    keep = []
    for sub in range(groups):
        j = sub
        while j + 3 * groups < K1:
            keep += [j, j + groups, j + 2 * groups, j + 3 * groups]
            j += 4 * groups
    return np.array(sorted(keep), dtype=np.int64)


def nce_scores_fwd(bank, idx, f, T, gather, mut=NONE):
    """-> out [B, K1], gathered [B, K1, D] or None"""
    B, K1 = idx.shape
    D = bank.shape[1]
    k = _dn(D, mut)
    invT = F32(1) / F32(T)
    rows = bank[idx]
    out = np.full((B, K1), np.nan, F32)
    lim = min(K1, 512) if "nce_grid_stride" in mut else K1
    out[:, :lim] = (_sum(rows[..., :k] * f[:, None, :k]) * invT)[:, :lim]
    g = None
    if gather:
        g = np.full((B, K1, D), np.nan, F32)
        g[:, :lim, :k] = rows[:, :lim, :k]
    return out, g


def nce_scores_bwd(bank, idx, dout, T, mut=NONE):
    B, K1 = idx.shape
    D = bank.shape[1]
    k = _dn(D, mut)
    invT = F32(1) / F32(T)
    js = _unrolled(K1, 8, mut)
    df = np.full((B, D), np.nan, F32)
    df[:, :k] = (bank[idx[:, js]][..., :k] * dout[:, js, None]).sum(1, dtype=F32) * invT
    return df


def _updated(bank, y, f, momentum, first, mut):
    """rows y of `bank` after the momentum update, every row computed from the bank as it was"""
    k = _dk(bank.shape[1], mut)
    mom = F32(momentum)
    old = bank.copy()
    order = range(len(y) - 1, -1, -1) if first else range(len(y))
    for b in order:                                       # a later write wins
        v = old[y[b]] * mom + f[b] * (F32(1) - mom)
        nrm = np.sqrt(_sum(v[:k] * v[:k]))
        bank[y[b], :k] = (v / nrm)[:k]
    return bank


def nce_bank_update(bank, y, f, momentum, mut=NONE):
    return _updated(bank.copy(), y, f, momentum, False, mut)


def softmax_ce0_fwd(x, mut=NONE):
    """-> lse [B], rowloss [B], loss"""
    with np.errstate(all="ignore"):
        if "ce0_no_shift" in mut:
            lse = np.log(_sum(np.exp(x)))
        else:
            m = x.max(1)
            lse = m + np.log(_sum(np.exp(x - m[:, None])))
    rowloss = lse - x[:, 0]
    return lse.astype(F32), rowloss.astype(F32), _mean(rowloss, mut)


def softmax_ce0_bwd(x, lse, gscale, mut=NONE):
    B = x.shape[0]
    g = _gs(gscale, mut) / F32(B)
    p = np.exp(x - lse[:, None])
    p[:, 0] -= F32(1)
    return p * g


def nce_fused_fwd(bank_l, bank_ab, f_l, f_ab, idx, T, mut=NONE):
    """-> scores [2, B, K1], rows [2, B, K1, D], part [2, B, NCE_PARTS, 2]"""
    B, K1 = idx.shape
    D = bank_l.shape[1]
    k = _dn(D, mut)
    invT = F32(1) / F32(T)
    feats = (f_l, f_ab) if "nce_side" in mut else (f_ab, f_l)
    scores, rows = np.zeros((2, B, K1), F32), np.zeros((2, B, K1, D), F32)
    part = np.zeros((2, B, NCE_PARTS, 2), F32)
    cl = -(-K1 // NCE_PARTS)
    for side, (bank, f) in enumerate(zip((bank_l, bank_ab), feats)):
        rows[side] = bank[idx]
        if k < D:
            rows[side][..., k:] = np.nan
        scores[side] = _sum(rows[side][..., :k] * f[:, None, :k]) * invT
        for c in range(NCE_PARTS):
            v = scores[side][:, c * cl:min(K1, (c + 1) * cl)]
            if v.shape[1] == 0:
                part[side, :, c] = (-np.inf, np.nan if "nce_idle_part" in mut else 0.0)
                continue
            m = v.max(1)
            part[side, :, c, 0], part[side, :, c, 1] = m, _sum(np.exp(v - m[:, None]))
    return scores, rows, part


def nce_fused_update(bank_l, bank_ab, y, f_l, f_ab, momentum, part, scores, mut=NONE):
    """-> bank_l, bank_ab, lse [2, B], rowloss [2, B], loss (the last three None without `part`)"""
    first = "nce_dup_first" in mut
    bl = _updated(bank_l.copy(), y, f_l, momentum, first, mut)
    bab = _updated(bank_ab.copy(), y, f_ab, momentum, first, mut)
    if part is None:
        return bl, bab, None, None, None
    M, S = part[..., 0], part[..., 1]
    top = M.max(-1)
    with np.errstate(all="ignore"):
        w = S * np.exp(M - top[..., None])
        if "nce_idle_part" not in mut:
            w = np.where(M > -np.inf, w, F32(0))
        lse = (top + np.log(_sum(w.astype(F32)))).astype(F32)
    rowloss = lse - scores[:, :, 0]
    B = rowloss.shape[1]
    n = B + (1 if "mean_n" in mut else 0)
    loss = F32(F32(rowloss[0].astype(np.float64).sum() / n) + F32(rowloss[1].astype(np.float64).sum() / n))
    return bl, bab, lse, rowloss.astype(F32), loss


def nce_fused_bwd(rows, scores, lse, T, gscale, mut=NONE):
    """-> df [2, B, D]"""
    _, B, K1, D = rows.shape
    k = _dn(D, mut)
    invT = F32(1) / F32(T)
    g = _gs(gscale, mut) / F32(B)
    p = np.exp(scores - lse[..., None])
    p[..., 0] -= F32(1)
    p = p * g
    js = _unrolled(K1, 32, mut)
    df = np.full((2, B, D), np.nan, F32)
    df[..., :k] = (rows[:, :, js, :k] * p[:, :, js, None]).sum(2, dtype=F32) * invT
    return df

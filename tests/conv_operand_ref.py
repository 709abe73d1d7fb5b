"""Plain numpy references for the operands of the gather-GEMM (csrc/conv.hip, csrc/conv_wino2.hip): packed weights, layout
transposes, per-row / per-tile records, and float64 emulators of what the kernels compute FROM those operands.

Written from the layouts documented in include/slic_hip.h (and, for the two tile tables and the Winograd matrices, the comments above
the kernels), not from the kernels' index arithmetic: arrays are built with einsum / transpose / reshape over named axes, so a wrong
stride in a kernel is not reproduced here.  No torch device, no `_lib`.  tests/test_conv_operands_cpu.py proves these references
against F.conv3d; tests/test_conv_operands_gpu.py compares the device entry points with them.

A "geometry" is any object with the integer fields of `SlicConvArgs` (M, N, nchunks, Cs, Ts, Hs, Ws, Ga, Gb, Gc, sa, sb, sc, ldw, ldo,
dst_strided, Da .. ec, k_run_len, k_run_px): `fwd_geometry` / `dgrad_geometry` build one from a ConvPlan the way ConvPlan._fwd_args /
ConvPlan.dgrad fill the struct."""
import types

import numpy as np

# ---- Winograd matrices (comments above pack_w_wino / pack_w_wino2, wino_common.h, the output transforms) ---------------------------
G43 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                [0, 0, 1]], np.float64)
BT43 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                 [0, 4, 0, -5, 0, 1]], np.float64)
AT43 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)
# F(2, 3) along H as the two-dimensional kernel runs it: H-point 2 is formed as d1 - d2 (the textbook row is d2 - d1), and row 2 of
# Gh is negated in the packed operand to match; the product of the two is the textbook one, so Ah^T is the textbook matrix
GH23 = np.array([[1, 0, 0], [1 / 2, 1 / 2, 1 / 2], [-1 / 2, 1 / 2, -1 / 2], [0, 0, 1]], np.float64)
BHT23 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, 1, -1, 0], [0, 1, 0, -1]], np.float64)
AHT23 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)


# ---- weight packs -------------------------------------------------------------------------------------------------------------------
def _w3(W):
    W = np.asarray(W)
    return W.reshape(W.shape[0], W.shape[1], -1)                     # [n, c, tap]


def _filled(fill, shape):
    out = np.empty(shape, np.float32)
    out[...] = fill                                                  # a scalar or the destination's earlier content
    return out


def ref_pack_fwd(W, Cs, Kp, fill):
    """Wp[n][tap * Cs + c] = W[n][c][tap] for c < C; channels C..Cs and columns ntaps * Cs..Kp keep `fill`"""
    w = _w3(W)
    N, C, ntaps = w.shape
    out = _filled(fill, (N, Kp))
    real = out[:, :ntaps * Cs].reshape(N, ntaps, Cs)                 # a view: [n, tap, channel slot]
    real[:, :, :C] = np.einsum("nct->ntc", w)
    return out


def ref_pack_dgrad(W, Cs, Kd, fill):
    """Wd[c][tap * N + n] = W[n][c][tap] (Cs rows, Kd columns); rows C..Cs and columns ntaps * N..Kd keep `fill`"""
    w = _w3(W)
    N, C, ntaps = w.shape
    out = _filled(fill, (Cs, Kd))
    real = out[:C, :ntaps * N].reshape(C, ntaps, N)
    real[...] = np.einsum("nct->ctn", w)
    return out


def ref_pack_fwd_runs(W, run_len, run_px, Kp):
    """Wp[n][run * run_len + px * C + c] = W[n][c][run * run_px + px], zero elsewhere (every element of [N][Kp] is specified)"""
    w = _w3(W)
    N, C, ntaps = w.shape
    nruns = -(-ntaps // run_px)
    taps = np.zeros((N, C, nruns * run_px), np.float32)
    taps[:, :, :ntaps] = w
    runs = np.zeros((N, nruns, run_len), np.float32)
    runs[:, :, :run_px * C] = np.einsum("ncrp->nrpc", taps.reshape(N, C, nruns, run_px)).reshape(N, nruns, run_px * C)
    out = np.zeros((N, Kp), np.float32)
    out[:, :nruns * run_len] = runs.reshape(N, nruns * run_len)
    return out


def _wino_w(W, dgrad):
    """w(n, c, kt, kh, kw) of the two Winograd packs: the weight itself, or W[c][n][2 - kt][2 - kh][2 - kw] for the data gradient"""
    w = np.asarray(W, np.float64)
    assert w.ndim == 5 and w.shape[2:] == (3, 3, 3)
    if dgrad:
        w = np.einsum("cnthw->ncthw", w)[:, :, ::-1, ::-1, ::-1]
    return w


def ref_pack_wino(W, dgrad):
    """-> (U, bound) float64, both of shape [tap9 = 9, C_/8, N_/64, p = 6, h = 2, nl = 64, j = 4]:
    U[tap9, cc, nb, p, h, nl, j] = sum_kw G[p][kw] w(n = 64 nb + nl, c = 8 cc + 4 h + j, kt, kh, kw), bound = |G| . |w|"""
    w = _wino_w(W, dgrad)
    N_, C_ = w.shape[:2]
    assert N_ % 64 == 0 and C_ % 8 == 0

    def lay(Gm, wm):
        u = np.einsum("pk,ncthk->ncthp", Gm, wm)
        u = u.reshape(N_ // 64, 64, C_ // 8, 2, 4, 3, 3, 6)           # nb nl cc h j kt kh p
        return np.ascontiguousarray(np.einsum("bleHjthp->thebpHlj", u)).reshape(9, C_ // 8, N_ // 64, 6, 2, 64, 4)
    return lay(G43, w), lay(np.abs(G43), np.abs(w))


def ref_pack_wino2(W, dgrad):
    """-> (U2, bound) float64 of shape [kt 3, C_/4, N_/64, Hpoint 4, Wpoint 6, column half 2, channel pair 2, n 32, 2 ch]:
    U2 = Gh w Gw^T with n = 64 nb + 32 half + n32, c = 4 cc + 2 pair + ch, row 2 of Gh negated; bound = |Gh| . |w| . |Gw|^T"""
    w = _wino_w(W, dgrad)
    N_, C_ = w.shape[:2]
    assert N_ % 64 == 0 and C_ % 4 == 0

    def lay(Gh, Gw, wm):
        u = np.einsum("jh,pk,ncthk->nctjp", Gh, Gw, wm)
        u = u.reshape(N_ // 64, 2, 32, C_ // 4, 2, 2, 3, 4, 6)        # nb half n32 cc pair ch kt j p
        return np.ascontiguousarray(np.einsum("bHlePctjp->tebjpHPlc", u))
    return lay(GH23, G43, w), lay(np.abs(GH23), np.abs(G43), np.abs(w))


# ---- layout transposes --------------------------------------------------------------------------------------------------------------
def ref_ncdhw_to_ndhwc(x, Cp):
    """[B, C, S] -> [B, S, Cp], channels zero-padded to Cp (every element specified)"""
    x = np.asarray(x, np.float32)
    B, C, S = x.shape
    y = np.zeros((B, S, Cp), np.float32)
    y[:, :, :C] = np.einsum("bcs->bsc", x)
    return y


def ref_ncdhw_to_ndhwc_wpad(x, pad_left, Wp):
    """[B, C, R, W] -> [B, R, Wp, C]: column w lands at w + pad_left, the other columns are zero"""
    x = np.asarray(x, np.float32)
    B, C, R, W = x.shape
    y = np.zeros((B, R, Wp, C), np.float32)
    y[:, :, pad_left:pad_left + W, :] = np.einsum("bcrw->brwc", x)
    return y


# ---- geometries ---------------------------------------------------------------------------------------------------------------------
GEOM_INT_FIELDS = ("M", "N", "nchunks", "Cs", "Ts", "Hs", "Ws", "Ga", "Gb", "Gc", "sa", "sb", "sc", "ldw", "ldo", "dst_strided",
                   "Da", "Db", "Dc", "da", "db", "dc", "ea", "eb", "ec", "k_run_len", "k_run_px")


def make_geometry(**kw):
    g = types.SimpleNamespace(**{f: 0 for f in GEOM_INT_FIELDS})
    g.tab = g.tap_tab = None
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def fwd_geometry(plan, B):
    """what ConvPlan._fwd_args puts into SlicConvArgs for a batch of B (tables as numpy arrays)"""
    T, H, W = plan.src_dims
    To, Ho, Wo = plan.out_dims
    return make_geometry(M=B * To * Ho * Wo, N=plan.N, nchunks=plan.nchunks_fwd, Cs=plan.Cs, Ts=T, Hs=H, Ws=W, Ga=To, Gb=Ho, Gc=Wo,
                         sa=plan.stride[0], sb=plan.stride[1], sc=plan.stride[2], ldw=plan.Kp, ldo=plan.N,
                         k_run_len=plan.run_len, k_run_px=plan.run_px, tab=plan.tab_fwd.cpu().numpy(),
                         tap_tab=None if plan.tap_fwd is None else plan.tap_fwd.cpu().numpy())


def dgrad_geometry(plan, dc, B):
    """what ConvPlan.dgrad puts into SlicConvArgs for the parity class record `dc` of plan.dgrad_classes"""
    T, H, W = plan.in_dims
    To, Ho, Wo = plan.out_dims
    ga, gb, gc = dc["grid"]
    return make_geometry(M=B * ga * gb * gc, N=plan.Cs, nchunks=dc["nchunks"], Cs=plan.N, Ts=To, Hs=Ho, Ws=Wo, Ga=ga, Gb=gb, Gc=gc,
                         sa=1, sb=1, sc=1, ldw=plan.Kd, ldo=plan.Cs, dst_strided=int(plan.stride != (1, 1, 1)),
                         Da=T, Db=H, Dc=W, da=plan.stride[0], db=plan.stride[1], dc=plan.stride[2],
                         ea=dc["cls"][0], eb=dc["cls"][1], ec=dc["cls"][2], tab=dc["tab"].cpu().numpy(),
                         tap_tab=None if dc["tap"] is None else dc["tap"].cpu().numpy())


def same_size_geometry(B, dims, Cs=64, N=64):
    """the stride-1 same-size geometry of the 3 x 3 x 3 / pad 1 layers (the Winograd variants and their tile tables)"""
    T, H, W = dims
    return make_geometry(M=B * T * H * W, N=N, Cs=Cs, Ts=T, Hs=H, Ws=W, Ga=T, Gb=H, Gc=W, sa=1, sb=1, sc=1, ldo=N)


# ---- per-row and per-tile records ---------------------------------------------------------------------------------------------------
def _rows(g):
    """(b, source coordinates a0, b0, c0) of the M rows: m -> (b, ga, gb, gc), coordinate = g * s"""
    per = g.Ga * g.Gb * g.Gc
    assert g.M % per == 0
    b, ga, gb, gc = np.unravel_index(np.arange(g.M, dtype=np.int64), (g.M // per, g.Ga, g.Gb, g.Gc))
    return b, ga * g.sa, gb * g.sb, gc * g.sc


def _inside_mask(coords, sizes):
    """bit (7 * dim + o + 3) set iff coordinate + o is inside the source, o in -3..3"""
    mk = np.zeros(coords[0].shape, np.int64)
    for dim, (x, n) in enumerate(zip(coords, sizes)):
        for o in range(-3, 4):
            mk |= ((x + o >= 0) & (x + o < n)).astype(np.int64) << (7 * dim + o + 3)
    return mk


def ref_row_table(g):
    """uint32 [M, 2]: {(((b * Ts + ga * sa) * Hs + gb * sb) * Ws + gc * sc) * Cs * 4, in-bounds mask}"""
    b, a0, b0, c0 = _rows(g)
    off = (((b * g.Ts + a0) * g.Hs + b0) * g.Ws + c0) * g.Cs * 4
    return np.stack([off & 0xFFFFFFFF, _inside_mask((a0, b0, c0), (g.Ts, g.Hs, g.Ws))], 1).astype(np.uint32)


def ref_wino_tile_table(g):
    """uint32 [(M / Ws) * ceil(Ws / 4), 2], tiles in (b, t, h, wt) order: {pixel index of (b, t, h, 4 wt); bits 0-2: t - 1, t, t + 1
    inside; 3-5: h - 1, h, h + 1 inside; 6-11: pixel 4 wt - 1 + a inside the row, a = 0..5; 12-15: output 4 wt + o inside the row}"""
    Wq = -(-g.Ws // 4)
    B = g.M // (g.Ts * g.Hs * g.Ws)
    b, t, h, wt = np.unravel_index(np.arange(B * g.Ts * g.Hs * Wq, dtype=np.int64), (B, g.Ts, g.Hs, Wq))
    mk = np.zeros(b.shape, np.int64)
    for o in range(3):
        mk |= ((t + o - 1 >= 0) & (t + o - 1 < g.Ts)).astype(np.int64) << o
        mk |= ((h + o - 1 >= 0) & (h + o - 1 < g.Hs)).astype(np.int64) << (3 + o)
    for a in range(6):
        mk |= ((4 * wt - 1 + a >= 0) & (4 * wt - 1 + a < g.Ws)).astype(np.int64) << (6 + a)
    for o in range(4):
        mk |= (4 * wt + o < g.Ws).astype(np.int64) << (12 + o)
    pix = ((b * g.Ts + t) * g.Hs + h) * g.Ws + 4 * wt
    return np.stack([pix, mk], 1).astype(np.uint32)


def ref_wino2_tile_table(g):
    """uint32 [(M / (Hs Ws)) * ceil(Hs / 2) * ceil(Ws / 4), 2], tiles in (b, t, h2, wt) order: {pixel index of (b, t, 2 h2, 4 wt);
    bit a * 6 + b (0-23): patch pixel (2 h2 - 1 + a, 4 wt - 1 + b) is OUTSIDE the frame; bits 24-26: frame t - 1 + kt is outside the
    clip; bit 27: always set}"""
    Wq, Hq = -(-g.Ws // 4), -(-g.Hs // 2)
    B = g.M // (g.Ts * g.Hs * g.Ws)
    b, t, h2, wt = np.unravel_index(np.arange(B * g.Ts * Hq * Wq, dtype=np.int64), (B, g.Ts, Hq, Wq))
    mk = np.full(b.shape, 1 << 27, np.int64)
    for a in range(4):
        for c in range(6):
            y, x = 2 * h2 - 1 + a, 4 * wt - 1 + c
            inside = (y >= 0) & (y < g.Hs) & (x >= 0) & (x < g.Ws)
            mk |= (~inside).astype(np.int64) << (a * 6 + c)
    for kt in range(3):
        mk |= ((t - 1 + kt < 0) | (t - 1 + kt >= g.Ts)).astype(np.int64) << (24 + kt)
    pix = ((b * g.Ts + t) * g.Hs + 2 * h2) * g.Ws + 4 * wt
    return np.stack([pix, mk], 1).astype(np.uint32)


def ref_tile_m(g, variant):
    """rows per workgroup tile (include/slic_hip.h, slic_conv_tile_m and the variant-30 / variant-31 paragraphs)"""
    if variant in (0, 20):
        return 64
    if variant == 22:
        return 128
    if variant == 30:                                                # 128 GEMM rows, or 128 / Wp * Ws on a ragged width (Wp = 4 ceil(Ws / 4))
        return 128 if g.Ws % 4 == 0 else 128 // (-(-g.Ws // 4) * 4) * g.Ws
    assert variant == 31
    # real outputs of a block of 64 tiles of 2 x 4, or 0 when the blocks do not all hold the same number
    Wq, Hq = -(-g.Ws // 4), -(-g.Hs // 2)
    if g.Hs % 2 == 0 and g.Ws % 4 == 0:
        return 64 * 8
    if g.Hs % 2 == 0 and 64 % Wq == 0:
        return (64 // Wq) * 2 * g.Ws                                 # 64 / Wq whole tile rows of two image rows
    if 64 % (Hq * Wq) == 0:
        return (64 // (Hq * Wq)) * g.Hs * g.Ws                       # whole frames
    return 0


# ---- the gather-GEMM in float64 -----------------------------------------------------------------------------------------------------
def _gather(src, idx):
    """range-checked loads: an element offset outside the source tensor reads zero"""
    ok = (idx >= 0) & (idx < src.size)
    return np.where(ok, src[np.clip(idx, 0, src.size - 1)], 0.0)


def _dst_rows(g):
    b, ga, gb, gc = np.unravel_index(np.arange(g.M, dtype=np.int64), (g.M // (g.Ga * g.Gb * g.Gc), g.Ga, g.Gb, g.Gc))
    if not g.dst_strided:
        return np.arange(g.M, dtype=np.int64)
    return ((b * g.Da + ga * g.da + g.ea) * g.Db + gb * g.db + g.eb) * g.Dc + gc * g.dc + g.ec


def _emulate(g, src, wgt, records, width, dst, hits, check_packed):
    src = np.asarray(src, np.float64).reshape(-1)
    wgt = np.asarray(wgt, np.float64)
    if dst is None:
        nrows = g.M // (g.Ga * g.Gb * g.Gc) * g.Da * g.Db * g.Dc if g.dst_strided else g.M
        dst, hits = np.full((nrows, g.ldo), np.nan), np.zeros(nrows, np.int64)
    assert wgt.shape == (g.N, g.ldw) and dst.shape[1] == g.ldo and g.ldo >= g.N
    b, a0, b0, c0 = _rows(g)
    origin = (((b * g.Ts + a0) * g.Hs + b0) * g.Ws + c0) * g.Cs
    rmask = _inside_mask((a0, b0, c0), (g.Ts, g.Hs, g.Ws))
    Y = np.zeros((g.M, g.N), np.float64)
    lane = np.arange(width, dtype=np.int64)
    for delta, tmask, col, packed in np.asarray(records, np.int64):
        if tmask == -1:                                              # all-zero chunk
            continue
        ok = (rmask & tmask) == tmask                                # the 21-bit in-bounds rule
        if check_packed:                                             # the packed tap offsets must say the same as the mask
            oa, ob, oc = (packed & 255) - 128, ((packed >> 8) & 255) - 128, ((packed >> 16) & 255) - 128
            direct = ((a0 + oa >= 0) & (a0 + oa < g.Ts) & (b0 + ob >= 0) & (b0 + ob < g.Hs) & (c0 + oc >= 0) & (c0 + oc < g.Ws))
            assert np.array_equal(ok, direct), "tap mask and packed tap offsets of a chunk disagree"
        vals = _gather(src, origin[ok, None] + delta + lane[None, :])
        Y[ok] += vals @ wgt[:, col:col + width].T
    rows = _dst_rows(g)
    dst[rows, :g.N] = Y
    np.add.at(hits, rows, 1)
    return dst


def emulate_gemm(g, src, wgt, dst=None, hits=None):
    """dst = gather(src) x wgt^T from the per-chunk table g.tab ([nchunks][4]): each chunk is four consecutive floats of the source
    at (row origin + delta) times four consecutive weight columns, taken only where the row's in-bounds mask contains the chunk's tap
    mask.  -> dst, float64 [rows, ldo] (NaN where nothing was written), written at the rows `dst_strided` addressing gives.  Several
    launches into one destination (the parity classes of a data gradient) pass `dst` and `hits` along; hits[row] counts the writes."""
    assert g.nchunks % 8 == 0 and g.tab.shape[0] >= g.nchunks and g.tab.shape[1] == 4
    if g.k_run_len > 0:
        # W-run operand: any Cs; runs of k_run_len floats hold k_run_px pixels x Cs channels, the rest of a run has zero weights
        assert g.k_run_len % 4 == 0 and g.k_run_px > 0 and g.k_run_px * g.Cs <= g.k_run_len and g.tap_tab is None
        w = np.asarray(wgt)
        nruns = (g.nchunks * 4) // g.k_run_len
        tail = w[:, :nruns * g.k_run_len].reshape(g.N, nruns, g.k_run_len)[:, :, g.k_run_px * g.Cs:]
        assert not tail.any() and not w[:, nruns * g.k_run_len:].any(), "the padding floats of a run must carry zero weights"
    else:
        assert g.Cs % 4 == 0
    return _emulate(g, src, wgt, g.tab[:g.nchunks], 4, dst, hits, True)


def emulate_gemm_taps(g, src, wgt, dst=None, hits=None):
    """the same product from the per-TAP table g.tap_tab ([ntaps][4] = {delta, tap mask, weight column base, 0}): Cs consecutive
    floats per tap, K = ntaps * Cs exactly"""
    assert g.tap_tab is not None and g.Cs % 32 == 0 and g.k_run_len == 0
    assert g.tap_tab.shape[0] * g.Cs == g.nchunks * 4, "K must be ntaps * Cs exactly"
    assert not g.tap_tab[:, 3].any()
    return _emulate(g, src, wgt, g.tap_tab, g.Cs, dst, hits, False)


# ---- the Winograd variants in float64 -----------------------------------------------------------------------------------------------
def _windows(xp, axis, n, size, step):
    """n windows of `size` at stride `step` along `axis` -> a new axis right behind it"""
    idx = (np.arange(n) * step)[:, None] + np.arange(size)[None, :]
    return np.take(xp, idx, axis=axis)


def emulate_wino(U, x, absolute=False):
    """Y = A^T [U . (B^T d)] per W-tile, d[a] = x[t + kt - 1, h + kh - 1, 4 wt - 1 + a, c] (zero outside): x [B, T, H, W, C_] ->
    [B, T, H, W, N_].  U in the documented layout [9, C_/8, N_/64, 6, 2, 64, 4].  absolute=True: every matrix by its absolute values
    (an element-wise error bound when U is an error bound and x the input's magnitudes)."""
    x = np.asarray(x, np.float64)
    B, T, H, W, C = x.shape
    U = np.asarray(U, np.float64)
    assert U.shape[0] == 9 and U.shape[1] == C // 8 and U.shape[3:] == (6, 2, 64, 4)
    N = U.shape[2] * 64
    u = np.einsum("thebpHlj->thpeHjbl", U.reshape(3, 3, C // 8, N // 64, 6, 2, 64, 4)).reshape(3, 3, 6, C, N)   # kt kh p c n
    BT, AT = (np.abs(BT43), np.abs(AT43)) if absolute else (BT43, AT43)
    Wq = -(-W // 4)
    xp = np.zeros((B, T + 2, H + 2, 4 * Wq + 2, C))
    xp[:, 1:T + 1, 1:H + 1, 1:W + 1] = x
    d = _windows(xp, 3, Wq, 6, 4)                                    # b t' h' wt a c
    V = np.einsum("pa,bthwac->bthwpc", BT, d)
    M = np.zeros((B, T, H, Wq, 6, N))
    for kt in range(3):
        for kh in range(3):
            M += np.einsum("bthwpc,pcn->bthwpn", V[:, kt:kt + T, kh:kh + H], u[kt, kh])
    Y = np.einsum("op,bthwpn->bthwon", AT, M).reshape(B, T, H, 4 * Wq, N)
    return Y[:, :, :, :W]


def emulate_wino2(U2, x, absolute=False):
    """Y = Ah^T [U2 . (Bh^T d Bw)] Aw per tile of 2 x 4 outputs, d the 4 x 6 patch at (2 h2 - 1, 4 wt - 1) of frame t + kt - 1, with
    H-point 2 formed as d1 - d2.  U2 in the documented layout [3, C_/4, N_/64, 4, 6, 2, 2, 32, 2]."""
    x = np.asarray(x, np.float64)
    B, T, H, W, C = x.shape
    U2 = np.asarray(U2, np.float64)
    assert U2.shape[0] == 3 and U2.shape[1] == C // 4 and U2.shape[3:] == (4, 6, 2, 2, 32, 2)
    N = U2.shape[2] * 64
    u = np.einsum("tebjpHPlc->tjpePcbHl", U2).reshape(3, 4, 6, C, N)  # kt j p c n
    BH, BT, AH, AT = (np.abs(m) if absolute else m for m in (BHT23, BT43, AHT23, AT43))
    Wq, Hq = -(-W // 4), -(-H // 2)
    xp = np.zeros((B, T + 2, 2 * Hq + 2, 4 * Wq + 2, C))
    xp[:, 1:T + 1, 1:H + 1, 1:W + 1] = x
    d = _windows(_windows(xp, 3, Wq, 6, 4), 2, Hq, 4, 2)              # b t' h2 a wt b6 c
    V = np.einsum("ja,pq,bthawqc->bthwjpc", BH, BT, d)
    M = np.zeros((B, T, Hq, Wq, 4, 6, N))
    for kt in range(3):
        M += np.einsum("bthwjpc,jpcn->bthwjpn", V[:, kt:kt + T], u[kt])
    Y = np.einsum("rj,op,bthwjpn->bthrwon", AH, AT, M).reshape(B, T, 2 * Hq, 4 * Wq, N)
    return Y[:, :, :H, :W]

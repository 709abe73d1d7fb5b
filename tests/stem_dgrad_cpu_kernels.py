"""float64 NumPy restatement of csrc/stem_dgrad.hip — the stem's data gradient with respect to the clip — for the tests
(not a product fallback).  Same algorithm as the device code: one GEMM row per coarse position (b, t, hc = h // 2, wc = w // 2),
one column per (channel, h parity, w parity) padded to 16, K = taps dt x 4 x 4 (h, w) offsets into dz x N channels, a weight
operand that is zero where a parity class has no tap, built from the same offset table as the device packer
(stem_dgrad_pack_kernel).  t is not folded: a row's t is the fine t and only the taps dt with (t + pt - dt) % st == 0 whose dz
plane exists are executed."""
import itertools

import numpy as np

COLS = 16                     # C x 2 x 2 columns, padded to the MFMA's width
KH = KW = 7                   # the stem's spatial kernel; stride 2, pad 3


def offset_table(k, s, p):
    """offsets o into dz along one axis of a (kernel k, stride s, pad p) convolution's data gradient: input position
    s * coarse + q receives dz[coarse + o] through tap d = q + p - s * o, for every parity q and tap d"""
    return sorted({(q + p - d) // s for q in range(s) for d in range(k) if (q + p - d) % s == 0})


def tap_of(q, o, k, s, p):
    """tap index of parity q at offset o, or None where that parity class has no tap there"""
    d = q + p - s * o
    return d if 0 <= d < k else None


def slot_counts(kernel, stride, pad):
    """(real, total) tap slots of the coarse formulation with every strided axis folded into parity columns:
    total = #offset triples x #parity classes, real = those that hold a tap"""
    offs = [offset_table(k, s, p) for k, s, p in zip(kernel, stride, pad)]
    real = total = 0
    for o in itertools.product(*offs):
        for q in itertools.product(*[range(s) for s in stride]):
            total += 1
            real += all(tap_of(qq, oo, k, s, p) is not None for qq, oo, k, s, p in zip(q, o, kernel, stride, pad))
    return real, total


def executed_slots(kt, st):
    """(real, executed) slots of the device kernel over one period of st output frames: t stays a fine row index, so a frame
    executes only its own taps dt (every one of them real along t) x the 4 x 4 offsets x the 2 x 2 parities"""
    oh = offset_table(KH, 2, 3)
    per_dt_real = sum(tap_of(qh, a, KH, 2, 3) is not None and tap_of(qw, b, KW, 2, 3) is not None
                      for a in oh for b in oh for qh in range(2) for qw in range(2))
    ndt = sum(1 for t in range(st) for dt in range(kt) if (t + kt // 2 - dt) % st == 0)
    return per_dt_real * ndt, len(oh) * len(oh) * 4 * ndt


def pack_weight(w):
    """w [N, C, kt, 7, 7] -> Wop [kt, 16 offsets (4 (oh + 1) + (ow + 1)), N, 16 columns (4 c + 2 qh + qw)], zero-padded"""
    N, C, kt = w.shape[:3]
    assert w.shape[3:] == (KH, KW) and C * 4 <= COLS
    offs = offset_table(KH, 2, 3)
    assert offs == [-1, 0, 1, 2]
    wop = np.zeros((kt, 16, N, COLS), np.float64)
    for (ia, oh), (ib, ow) in itertools.product(enumerate(offs), enumerate(offs)):
        for c, qh, qw in itertools.product(range(C), range(2), range(2)):
            dh, dw = tap_of(qh, oh, KH, 2, 3), tap_of(qw, ow, KW, 2, 3)
            if dh is not None and dw is not None:
                wop[:, 4 * ia + ib, :, 4 * c + 2 * qh + qw] = w[:, c, :, dh, dw].T
    return wop


def device_pack_order(wop):
    """the flat operand as slic_pack_weight_stem_dgrad lays it out: [dt][off][n // 8][kq][column][m], n = 8 g + 2 kq + m"""
    kt, _, N, _ = wop.shape
    return wop.reshape(kt, 16, N // 8, 4, 2, COLS).transpose(0, 1, 2, 3, 5, 4).reshape(-1)


def stem_dgrad(dz, w, dims, st):
    """dz [B, To, Ho, Wo, N] (NDHWC), w [N, C, kt, 7, 7], dims = (T, H, W), t-stride st -> dx [B, C, T, H, W] in float64"""
    dz, w = np.asarray(dz, np.float64), np.asarray(w, np.float64)
    B, To, Ho, Wo, N = dz.shape
    C, kt = w.shape[1], w.shape[2]
    T, H, W = dims
    pt = kt // 2
    assert (To, Ho, Wo) == ((T - 1) // st + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    wop = pack_weight(w)
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    # zero frame: offsets -1 .. 2 around every coarse position
    dzp = np.zeros((B, To, Hc + 3, Wc + 3, N), np.float64)
    dzp[:, :, 1:1 + Ho, 1:1 + Wo] = dz
    out = np.zeros((B, T, Hc, Wc, COLS), np.float64)             # GEMM rows x columns
    for t in range(T):
        for dt in range(kt):
            num = t + pt - dt
            if num < 0 or num % st or num // st >= To:
                continue
            plane = dzp[:, num // st]
            for off in range(16):
                a, b = off >> 2, off & 3
                out[:, t] += plane[:, a:a + Hc, b:b + Wc] @ wop[dt, off]
    # column 4 c + 2 qh + qw of coarse (hc, wc) is dx[c, 2 hc + qh, 2 wc + qw]
    full = out[..., :4 * C].reshape(B, T, Hc, Wc, C, 2, 2).transpose(0, 4, 1, 2, 5, 3, 6).reshape(B, C, T, 2 * Hc, 2 * Wc)
    return np.ascontiguousarray(full[:, :, :, :H, :W])

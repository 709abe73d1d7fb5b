"""GPU: every entry point of csrc/loss.hip and csrc/nce.hip called directly through the C ABI and compared with float64.

Entry points called by at least one case (18 of loss.hip, 8 of nce.hip):
  slic_triplet_select, slic_triplet_select_cross, slic_triplet_select_k, slic_pair_distance, slic_pair_distance_bwd,
  slic_margin_cos_fwd, slic_margin_cos_bwd, slic_margin_euclid_fwd, slic_margin_euclid_bwd, slic_infonce_rows_fwd,
  slic_infonce_rows_bwd, slic_pdist, slic_pdist2, slic_ntxent_workspace_bytes, slic_ntxent_fwd, slic_ntxent_bwd,
  slic_ntxent_euclid_fwd, slic_ntxent_euclid_bwd;
  slic_nce_scores_fwd, slic_nce_scores_bwd, slic_nce_bank_update, slic_softmax_ce0_fwd, slic_softmax_ce0_bwd, slic_nce_fused_fwd,
  slic_nce_fused_update, slic_nce_fused_bwd.

The cases and gates are functions of a backend: `Device` calls the library; tests/test_loss_kernels_cpu.py runs the same functions
with the NumPy mirror (tests/loss_cpu_kernels.py) in the device's place, unmutated (every gate can be met in float32 by another
summation order, with a factor 4 to spare) and with one defect at a time (every gate is tight enough to notice).  Importing this
module does not touch the device.

Hygiene: every output starts as NaN (-7 for int32), every output, state and workspace is the front of a larger buffer whose
4096-byte tail must come back unchanged, and every call runs twice into fresh outputs that must be bit-equal.

Selection outputs are compared exactly with a list-based reference written from the header comment (negatives list, candidate list,
floor(u * count)); the distance matrices hold multiples of 1/16 in [0, 2] and the margins are multiples of 1/16, so every
d(a,p) + margin - d(a,j) is exact in float32 and float64.

Float outputs are gated as |got - float64| <= coef * 2^-24 * scale: `scale` comes from the float64 reference (the sum of the
absolute terms of the sum that made the output), `coef` counts the roundings of the kernel's own arithmetic and is derived beside
each gate.  steps(D) = ceil(D / 64) + 6 is the chain of a one-wave row sum: a lane's fused steps plus the six butterfly adds.  The
worst error / gate ratio of each named gate is kept in RATIOS."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4096
U = 2.0 ** -24
EPS6 = float(F32(1e-6))
CLAMP = float(F32(1e-8))
TWO32 = 1 << 32
RATIOS = {}


def f32(a):
    return np.ascontiguousarray(a, dtype=F32)


def f64(a):
    return np.asarray(a, np.float64)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def steps(D):
    return -(-D // 64) + 6


def cc(D):
    """a cosine x.y / (nx ny) in units of 2^-24 x.|y| / (nx ny): steps(D) for the dot, steps(D) / 2 + 1 for each norm (the square
    root halves the relative error of the sum and rounds once), one product, one division, two to spare"""
    return 2 * steps(D) + 6


def c_euclid(D):
    """|x - y + eps|_2 in units of 2^-24 of itself: each difference rounds twice (4 units on its square), steps(D) for the sum,
    4 for sqrtf; the halving of the sum's relative error by the root is not claimed"""
    return steps(D) + 8


def gate(name, got, ref, scale, coef, what=""):
    """finite, and |got - ref| <= coef 2^-24 scale elementwise (a zero scale demands the reference's value exactly, up to float32's
    underflow: below 2^-126 a float32 result has no relative precision, and an expf of -200 is 0)"""
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (name, what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), (name, what, "not finite")
    tol = coef * U * np.broadcast_to(f64(scale), ref.shape)
    err = np.abs(got - ref)
    err = np.where(err <= 2.0 ** -126, 0.0, err)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / tol)
    worst = float(r.max()) if r.size else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), worst)
    assert worst <= 1.0, (name, what, worst)


def twice(fn):
    """two runs into fresh outputs, bit-equal"""
    a, b = fn(), fn()
    for u, v in zip(a, b):
        assert (u is None and v is None) or bits_equal(np.asarray(u), np.asarray(v)), "two runs differ"
    return a


# ------------------------------------------------------------------ the device backend
class Device:
    def __init__(self, lib):
        from video_similarity_search_amd import _lib
        self.lib, self._lib = lib, _lib
        self.pattern = (torch.arange(GUARD) % 251).to(torch.uint8).cuda()
        self._guards = []

    # -- plumbing
    def up(self, a, dtype=F32):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()

    def out(self, shape, dtype=torch.float32, data=None):
        """NaN / -7 (or `data`) in front of a guard tail"""
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape)) * 4
        buf = torch.empty(n + GUARD, dtype=torch.uint8, device="cuda")
        buf[n:] = self.pattern
        v = buf[:n].view(dtype).view(shape)
        if data is not None:
            v.copy_(torch.from_numpy(np.ascontiguousarray(data)).view(shape))
        else:
            v.fill_(float("nan") if dtype == torch.float32 else -7)
        self._guards.append((buf, n))
        return v

    def ws(self, nbytes):
        buf = torch.empty(int(nbytes) + GUARD, dtype=torch.uint8, device="cuda")
        buf[int(nbytes):] = self.pattern
        self._guards.append((buf, int(nbytes)))
        return buf

    def run(self, name, *args, keep=False):
        p = self._lib.ptr
        self._lib.call(name, *[p(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], self._lib.stream())
        torch.cuda.synchronize()
        for buf, n in self._guards:
            assert torch.equal(buf[n:], self.pattern), f"{name} wrote past a buffer of {n} bytes"
        if not keep:
            self._guards = []

    @staticmethod
    def np(*ts):
        return tuple(None if t is None else t.cpu().numpy() for t in ts)

    def scalar(self, g):
        return None if g is None else self.up([g])

    # -- selection
    def select(self, Dm, labels, anc, pos, margin, mode, u):
        neg = self.out((len(anc),), torch.int32)
        self.run("slic_triplet_select", self.up(Dm), self.up(labels, np.int64), Dm.shape[1], self.up(anc, np.int32),
                 self.up(pos, np.int32), len(anc), float(margin), mode, self.up(u), neg)
        return neg.cpu().numpy()

    def select_cross(self, Dm, col_labels, anc, anc_labels, pos, margin, mode, u):
        neg = self.out((len(anc),), torch.int32)
        self.run("slic_triplet_select_cross", self.up(Dm), self.up(col_labels, np.int64), Dm.shape[1], self.up(anc, np.int32),
                 self.up(anc_labels, np.int64), self.up(pos, np.int32), len(anc), float(margin), mode, self.up(u), neg)
        return neg.cpu().numpy()

    def select_k(self, Dm, labels, anc, pos, margin, K, u):
        neg = self.out((len(anc), K), torch.int32)
        status = self.out((1,), torch.int32, data=np.zeros(1, np.int32))            # caller-zeroed
        self.run("slic_triplet_select_k", self.up(Dm), self.up(labels, np.int64), Dm.shape[1], self.up(anc, np.int32),
                 self.up(pos, np.int32), len(anc), float(margin), K, self.up(u), neg, status)
        return neg.cpu().numpy(), int(status.item())

    # -- rowwise
    def pair_distance(self, X, Y, euclid):
        out = self.out((X.shape[0],))
        self.run("slic_pair_distance", self.up(X), self.up(Y), *X.shape, euclid, out)
        return out.cpu().numpy()

    def pair_distance_bwd(self, X, Y, G, euclid):
        dX, dY = self.out(X.shape), self.out(X.shape)
        self.run("slic_pair_distance_bwd", self.up(X), self.up(Y), self.up(G), *X.shape, euclid, dX, dY)
        return self.np(dX, dY)

    def pdist(self, V, eps, euclid):
        n = V.shape[0]
        out = self.out((n, n))
        self.run("slic_pdist", self.up(V), *V.shape, float(eps), euclid, out)
        return out.cpu().numpy()

    def pdist2(self, X, Y, eps, euclid):
        out = self.out((X.shape[0], Y.shape[0]))
        self.run("slic_pdist2", self.up(X), X.shape[0], self.up(Y), Y.shape[0], X.shape[1], float(eps), euclid, out)
        return out.cpu().numpy()

    def margin_fwd(self, X, Y, Z, margin, euclid):
        n, D = X.shape
        st, rl, loss = self.out((n, 8)), self.out((n,)), self.out((1,))
        self.run("slic_margin_euclid_fwd" if euclid else "slic_margin_cos_fwd", self.up(X), self.up(Y), self.up(Z), n, D,
                 float(margin), st, rl, loss)
        st, rl, loss = self.np(st, rl, loss)
        return st, rl, loss[0]

    def margin_bwd(self, X, Y, Z, st, gscale, euclid):
        n, D = X.shape
        dX, dY, dZ = self.out((n, D)), self.out((n, D)), self.out((n, D))
        self.run("slic_margin_euclid_bwd" if euclid else "slic_margin_cos_bwd", self.up(X), self.up(Y), self.up(Z), self.up(st), n, D,
                 self.scalar(gscale), dX, dY, dZ)
        return self.np(dX, dY, dZ)

    def infonce_fwd(self, X, Y, T):
        P, NY, D = Y.shape
        st, rl, loss = self.out((P, 18)), self.out((P,)), self.out((1,))
        self.run("slic_infonce_rows_fwd", self.up(X), self.up(Y), P, NY, D, float(T), st, rl, loss)
        st, rl, loss = self.np(st, rl, loss)
        return st, rl, loss[0]

    def infonce_bwd(self, X, Y, st, T, gscale):
        P, NY, D = Y.shape
        dX, dY = self.out((P, D)), self.out((P, NY, D))
        self.run("slic_infonce_rows_bwd", self.up(X), self.up(Y), self.up(st), P, NY, D, float(T), self.scalar(gscale), dX, dY)
        return self.np(dX, dY)

    # -- NT-Xent
    def ntxent(self, Eflat, n, D, lde, T, gscale, ldd):
        w = self.ws(self.lib.slic_ntxent_workspace_bytes(n, D))
        loss, dE = self.out((1,)), self.out((n, ldd))
        self.run("slic_ntxent_fwd", self.up(Eflat), n, D, lde, float(T), loss, w, keep=True)
        self.run("slic_ntxent_bwd", w, n, D, float(T), self.scalar(gscale), dE, ldd)
        loss, dE = self.np(loss, dE)
        return loss[0], dE

    def ntxent_euclid_fwd(self, E, T):
        n, D = E.shape
        dist, wm, rl, loss = self.out((n, n)), self.out((n, n)), self.out((n,)), self.out((1,))
        self.run("slic_ntxent_euclid_fwd", self.up(E), n, D, float(T), dist, wm, rl, loss)
        dist, wm, rl, loss = self.np(dist, wm, rl, loss)
        return dist, wm, rl, loss[0]

    def ntxent_euclid_bwd(self, E, dist, wm, gscale):
        n, D = E.shape
        dE = self.out((n, D))
        self.run("slic_ntxent_euclid_bwd", self.up(E), self.up(dist), self.up(wm), n, D, self.scalar(gscale), dE)
        return dE.cpu().numpy()

    # -- memory-bank NCE
    def nce_scores_fwd(self, bank, idx, f, T, gather):
        B, K1 = idx.shape
        D = bank.shape[1]
        out = self.out((B, K1))
        g = self.out((B, K1, D)) if gather else None
        self.run("slic_nce_scores_fwd", self.up(bank), self.up(idx, np.int64), self.up(f), B, K1, D, float(T), out, g)
        return self.np(out, g)

    def nce_scores_bwd(self, bank, idx, dout, T):
        B, K1 = idx.shape
        D = bank.shape[1]
        df = self.out((B, D))
        self.run("slic_nce_scores_bwd", self.up(bank), self.up(idx, np.int64), self.up(dout), B, K1, D, float(T), df)
        return df.cpu().numpy()

    def nce_bank_update(self, bank, y, f, momentum):
        b = self.out(bank.shape, data=bank)
        self.run("slic_nce_bank_update", b, self.up(y, np.int64), self.up(f), len(y), bank.shape[1], float(momentum))
        return b.cpu().numpy()

    def ce0_fwd(self, x):
        B, K1 = x.shape
        lse, rl, loss = self.out((B,)), self.out((B,)), self.out((1,))
        self.run("slic_softmax_ce0_fwd", self.up(x), B, K1, lse, rl, loss)
        lse, rl, loss = self.np(lse, rl, loss)
        return lse, rl, loss[0]

    def ce0_bwd(self, x, lse, gscale):
        B, K1 = x.shape
        dx = self.out((B, K1))
        self.run("slic_softmax_ce0_bwd", self.up(x), self.up(lse), B, K1, self.scalar(gscale), dx)
        return dx.cpu().numpy()

    def fused_fwd(self, bank_l, bank_ab, f_l, f_ab, idx, T):
        B, K1 = idx.shape
        D = bank_l.shape[1]
        sc, rows, part = self.out((2, B, K1)), self.out((2, B, K1, D)), self.out((2, B, 16, 2))
        self.run("slic_nce_fused_fwd", self.up(bank_l), self.up(bank_ab), self.up(f_l), self.up(f_ab), self.up(idx, np.int64), B, K1, D,
                 float(T), sc, rows, part)
        return self.np(sc, rows, part)

    def fused_update(self, bank_l, bank_ab, y, f_l, f_ab, momentum, part, scores):
        """with part None the loss outputs are passed all the same and must stay NaN"""
        B, D = f_l.shape
        bl, bab = self.out(bank_l.shape, data=bank_l), self.out(bank_ab.shape, data=bank_ab)
        lse, rl, loss = self.out((2, B)), self.out((2, B)), self.out((1,))
        K1 = 1 if scores is None else scores.shape[2]
        self.run("slic_nce_fused_update", bl, bab, self.up(y, np.int64), self.up(f_l), self.up(f_ab), B, D, float(momentum),
                 self.up(part), self.up(scores), K1, lse, rl, loss)
        bl, bab, lse, rl, loss = self.np(bl, bab, lse, rl, loss)
        if part is None:
            assert np.isnan(lse).all() and np.isnan(rl).all() and np.isnan(loss).all(), "update without part touched a loss output"
            return bl, bab, None, None, None
        return bl, bab, lse, rl, loss[0]

    def fused_bwd(self, rows, scores, lse, T, gscale):
        _, B, K1, D = rows.shape
        df = self.out((2, B, D))
        self.run("slic_nce_fused_bwd", self.up(rows), self.up(scores), self.up(lse), B, K1, D, float(T), self.scalar(gscale), df)
        return df.cpu().numpy()


@pytest.fixture(scope="module")
def dev(gpu):
    return Device(gpu)


# ------------------------------------------------------------------ a) selection: exact
def sixteenths(rng, shape, lo=0, hi=33):
    return f32(rng.integers(lo, hi, shape) / 16.0)


def u_for(rank, count):
    """a uniform whose float32 product with `count` floors to `rank`; 'first' = 0, 'last' = the largest float32 below 1"""
    if rank == "first" or count <= 0:
        return F32(0)
    if rank == "last":
        return np.nextafter(F32(1), F32(0))
    u = F32((rank + 0.5) / count)
    assert int(u * F32(count)) == rank
    return u


def ref_lists(c, pr):
    """the negatives list and the candidate list of pair pr (Python integers: labels compare as 64-bit)"""
    Dm, lab = c["Dm"], [int(v) for v in c["labels"]]
    a = int(c["anc"][pr])
    la = int(c["anc_labels"][pr]) if c.get("anc_labels") is not None else lab[a]
    negs = [j for j in range(len(lab)) if lab[j] != la]
    dap = float(Dm[a, int(c["pos"][pr])]) + float(c["margin"])
    loss = {j: dap - float(Dm[a, j]) for j in negs}
    cand = negs if c["mode"] == 0 else [j for j in negs if loss[j] > 0]
    return a, negs, cand, loss


def ref_select(c):
    out = []
    for pr in range(len(c["anc"])):
        a, negs, cand, loss = ref_lists(c, pr)
        res = None
        if c["mode"] in (0, 1) and cand:
            res = cand[min(int(F32(c["u"][pr]) * F32(len(cand))), len(cand) - 1)]
        elif c["mode"] == 2 and cand:
            best = max(loss[j] for j in cand)
            res = min(j for j in cand if loss[j] == best)
        if res is None:                                   # hardest easy: the POSITION of the closest negative in the negatives list
            res = 0
            if negs:
                dmin = min(float(c["Dm"][a, j]) for j in negs)
                res = negs.index(min(j for j in negs if float(c["Dm"][a, j]) == dmin))
        out.append(res)
    return np.array(out, np.int32)


def set_u(c, ranks):
    """ranks[pr]: an integer rank (taken modulo the set's size), 'first' or 'last'"""
    u = []
    for pr, r in enumerate(ranks):
        n = len(ref_lists(c, pr)[2])
        u.append(u_for(r % n if isinstance(r, int) and n else r, n))
    c["u"] = f32(u)
    return c


def sel_random(n, P, mode, seed, cross=False):
    rng = np.random.default_rng(1000 * n + 10 * P + mode + seed)
    rows = 6 if cross else n
    labels = rng.integers(-1 if cross else 0, 4, n).astype(np.int64)
    if n == 2:
        labels[:] = [0, 1]
    anc = rng.integers(0, rows, P).astype(np.int32)
    c = dict(Dm=sixteenths(rng, (rows, n)), labels=labels, anc=anc, margin=float(rng.integers(0, 9)) / 16, mode=mode)
    if cross:
        c["anc_labels"] = np.array([(max(int(labels[a]), 0) + 1 + pr % 3) % 4 for pr, a in enumerate(anc)], np.int64)
        assert all(int(c["anc_labels"][pr]) != int(labels[a]) for pr, a in enumerate(anc))
        la = c["anc_labels"]
    else:
        la = labels[anc]
    pos = []
    for pr in range(P):
        same = np.flatnonzero(labels == la[pr])
        pos.append(int(same[rng.integers(0, len(same))]) if len(same) else int(rng.integers(0, n)))
    c["pos"] = np.array(pos, np.int32)
    kinds = [3, "last", "first", 70, 1, 141, 64, "last", 17]
    return set_u(c, kinds[:P])


@functools.lru_cache(maxsize=None)
def sel_case(name):
    """the named situations; each builder asserts that its situation really occurs"""
    rng = np.random.default_rng(sum(map(ord, name)))
    chunk = lambda res: [int(r) // 64 for r in res]
    if name in ("rank_chunks_m0", "rank_chunks_m1"):      # the drawn rank falls in the 2nd, 3rd, 4th chunk; column n - 1; rank 0
        n, mode = 200, int(name[-1])
        labels = rng.integers(0, 4, n).astype(np.int64)
        labels[n - 1] = 77
        Dm = sixteenths(rng, (n, n))
        Dm[:, n - 1] = 0
        c = dict(Dm=Dm, labels=labels, anc=np.arange(5, dtype=np.int32), pos=np.arange(5, dtype=np.int32), margin=2.0, mode=mode)
        ranks = []
        for pr, want in enumerate([64, 128, 192]):
            cand = ref_lists(c, pr)[2]
            ranks.append(next(i for i, j in enumerate(cand) if j >= want))
        set_u(c, ranks + ["last", "first"])
        res = ref_select(c)
        assert chunk(res[:3]) == [1, 2, 3] and res[3] == n - 1 and res[4] < 64
        return c
    if name in ("first_chunk_empty", "last_chunk_only_129", "last_chunk_only_200_m1", "last_chunk_only_200_m2"):
        n = 129 if "129" in name or name == "first_chunk_empty" else 200
        P = {"first_chunk_empty": 4, "last_chunk_only_129": 1}.get(name, 9)
        start = 64 if name == "first_chunk_empty" else n - n % 64
        labels = rng.integers(1, 4, n).astype(np.int64)
        labels[:P + 1] = 0                                # the anchors 0 .. P-1 and the positive column P
        Dm = np.full((n, n), 2.0, F32)
        Dm[:, start:] = sixteenths(rng, (n, n - start), 0, 16)      # below thr = 1
        Dm[:, P] = 0.5
        c = dict(Dm=Dm, labels=labels, anc=np.arange(P, dtype=np.int32), pos=np.full(P, P, np.int32), margin=0.5,
                 mode=2 if name.endswith("m2") else 1)
        set_u(c, [0, "last", 5, "first", 2, 3, 4, 6, 1][:P])
        for pr in range(P):
            cand = ref_lists(c, pr)[2]
            assert cand and min(cand) >= start
        return c
    if name == "mode2_ties":                              # the lowest index wins across lanes, across chunks of one lane, and both
        n = 129
        labels = np.ones(n, np.int64)
        labels[:5] = 0
        Dm = np.ones((n, n), F32)
        Dm[:, 4] = 0.5
        for a, (j1, j2) in enumerate([(70, 90), (5, 69), (64, 128), (127, 128)]):
            Dm[a, j1] = Dm[a, j2] = 0.25
        c = dict(Dm=Dm, labels=labels, anc=np.arange(4, dtype=np.int32), pos=np.full(4, 4, np.int32), margin=0.25, mode=2,
                 u=np.zeros(4, F32))
        assert list(ref_select(c)) == [70, 5, 64, 127]
        return c
    if name in ("zero_loss_m1", "zero_loss_m2"):          # loss exactly 0 is no candidate
        n, mode = 40, int(name[-1])
        labels = rng.integers(1, 4, n).astype(np.int64)
        labels[:6] = 0
        Dm = np.ones((n, n), F32)
        Dm[:, 5] = 0.75                                   # thr = 1: every negative of anchors 0 .. 2 has loss 0 -> fallback
        Dm[3, 6], Dm[3, 9], Dm[3, 20], Dm[3, 33] = 1.0, 0.5, 0.25, 0.5      # anchor 3: column 6 at loss 0, three candidates
        Dm[3, 7:] = np.where(Dm[3, 7:] == 1.0, 2.0, Dm[3, 7:])
        c = dict(Dm=Dm, labels=labels, anc=np.arange(4, dtype=np.int32), pos=np.full(4, 5, np.int32), margin=0.25, mode=mode)
        set_u(c, [0, 1, "last", 0])
        res = ref_select(c)
        assert list(res[:3]) == [0, 0, 0] and ref_lists(c, 3)[2] == [9, 20, 33] and res[3] == (9 if mode == 1 else 20)
        return c
    if name in ("fallback_m1", "fallback_m2", "fallback_cross_m3"):
        # no candidate; the closest negative sits in the 3rd chunk, tied with a later one; position != row; 64-bit labels
        n, P = 200, 5
        labels = rng.integers(1, 4, n).astype(np.int64)
        labels[[0, 1, 2, 3, 4, 10, 70]] = 5
        labels[130] = 5 + TWO32
        Dm = np.full((6 if "cross" in name else n, n), 2.0, F32)
        Dm[:, 10] = 0.0
        Dm[:, 130] = Dm[:, 150] = 1.0
        c = dict(Dm=Dm, labels=labels, anc=np.arange(P, dtype=np.int32), pos=np.full(P, 10, np.int32), margin=0.5,
                 mode=int(name[-1]), u=np.full(P, 0.5, F32))
        if "cross" in name:
            labels[0:5] = [1, 2, 3, 1, 2]                 # the queue's own labels at the anchors' row numbers: not the anchors' labels
            c["anc_labels"] = np.full(P, 5, np.int64)
            assert list(ref_select(c)) == [128] * P
        else:
            assert list(ref_select(c)) == [123] * P
        return c
    if name.startswith("cross_"):                         # cross_<ncols>_<P>_m<mode>
        _, n, P, m = name.split("_")
        c = sel_random(int(n), int(P), int(m[1:]), 5, cross=True)
        assert (c["labels"] == -1).any() and c["Dm"].shape[0] != c["Dm"].shape[1]
        return c
    raise KeyError(name)


SEL_NAMED = ["rank_chunks_m0", "rank_chunks_m1", "first_chunk_empty", "last_chunk_only_129", "last_chunk_only_200_m1",
             "last_chunk_only_200_m2", "mode2_ties", "zero_loss_m1", "zero_loss_m2", "fallback_m1", "fallback_m2", "fallback_cross_m3",
             "cross_129_5_m0", "cross_200_9_m1", "cross_65_4_m2", "cross_200_1_m3", "cross_40_9_m0"]
SEL_RANDOM = [(n, P, mode) for n, P in [(2, 1), (40, 4), (64, 5), (65, 9), (128, 4), (129, 5), (200, 9)] for mode in (0, 1, 2)]


def check_select(be, c):
    c = sel_case(c) if isinstance(c, str) else c
    ref = ref_select(c)
    if c.get("anc_labels") is not None:
        (got,) = twice(lambda: [be.select_cross(c["Dm"], c["labels"], c["anc"], c["anc_labels"], c["pos"], c["margin"], c["mode"], c["u"])])
    else:
        (got,) = twice(lambda: [be.select(c["Dm"], c["labels"], c["anc"], c["pos"], c["margin"], c["mode"], c["u"])])
    assert got.dtype == np.int32 and np.array_equal(got, ref), (got, ref)


def ref_select_k(c):
    P, K = c["u"].shape
    out, status = np.full((P, K), -1, np.int32), 0
    for pr in range(P):
        a, negs, cand, _ = ref_lists(c, pr)
        if len(negs) < K:
            status = 1
            continue
        avail = list(range(max(K, len(cand))))
        for t in range(K):
            r = min(int(F32(c["u"][pr, t]) * F32(len(avail))), len(avail) - 1)
            out[pr, t] = negs[avail.pop(r)]
    return out, status


@functools.lru_cache(maxsize=None)
def selk_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "topup":                                   # cnt_c = 2 < K = 5: the first five negatives, in draw order
        n, P, K = 40, 4, 5
        labels = rng.integers(1, 4, n).astype(np.int64)
        labels[:5] = 0
        Dm = np.full((n, n), 2.0, F32)
        Dm[:, 4] = 0.5
        Dm[:, 20] = Dm[:, 30] = 0.25
        c = dict(Dm=Dm, labels=labels, anc=np.arange(P, dtype=np.int32), pos=np.full(P, 4, np.int32), margin=0.25, mode=1)
        ranks = [[0] * 5, ["last"] * 5, [2, 2, 0, 1, 0], [4, 0, 2, 0, 0]]
        c["u"] = f32([[u_for(r, K - t) for t, r in enumerate(row)] for row in ranks])
        res, st = ref_select_k(c)
        first = [j for j in range(n) if labels[j] != 0][:K]
        assert st == 0 and all(sorted(r) == first for r in res.tolist()) and res[0].tolist() == first and res[1].tolist() == first[::-1]
        return c
    if name in ("three_chunks", "k1", "short"):
        n, P, K = {"three_chunks": (200, 5, 8), "k1": (65, 9, 1), "short": (64, 5, 5)}[name]
        labels = rng.integers(0, 4, n).astype(np.int64)
        if name == "short":                               # anchor 7 (label 9) has three negatives; anchors 1, 2, 3 have 61 or more
            labels[:] = 9
            labels[[1, 2, 3]] = [1, 2, 3]
            anc = np.array([1, 7, 2, 3, 1], np.int32)
        else:
            anc = rng.integers(0, n, P).astype(np.int32)
        c = dict(Dm=sixteenths(rng, (n, n)), labels=labels, anc=anc, pos=anc.copy(), margin=2.0, mode=1)
        u = np.zeros((P, K), F32)
        for pr in range(P):
            L = max(K, len(ref_lists(c, pr)[2]))
            for t in range(K):
                r = [0, L - t - 1, (L - t) // 2, 0, 70, 130, 1, (L - t) // 3][(t + pr) % 8] % (L - t)
                u[pr, t] = u_for(["first", "last", r][(pr + t) % 3] if pr == 0 else r, L - t)
        c["u"] = u
        res, st = ref_select_k(c)
        assert st == (name == "short")
        if name == "short":
            assert (res[1] == -1).all() and (np.delete(res, 1, 0) >= 0).all()
        if name == "three_chunks":
            assert min(len(ref_lists(c, pr)[2]) for pr in range(P)) > 128 + K and len({j // 64 for j in res.ravel()}) >= 3
        for row in res.tolist():
            assert row[0] == -1 or len(set(row)) == K
        return c
    raise KeyError(name)


SELK_NAMED = ["topup", "three_chunks", "k1", "short"]


def check_select_k(be, name):
    c = selk_case(name)
    ref, rst = ref_select_k(c)
    K = c["u"].shape[1]
    got, st = twice(lambda: be.select_k(c["Dm"], c["labels"], c["anc"], c["pos"], c["margin"], K, c["u"]))
    assert np.array_equal(got, ref), (got, ref)
    assert int(st) == rst


@pytest.mark.parametrize("name", SEL_NAMED)
def test_select_named(dev, name):
    check_select(dev, name)


@pytest.mark.parametrize("n,P,mode", SEL_RANDOM)
def test_select_random(dev, n, P, mode):
    check_select(dev, sel_random(n, P, mode, 0))


@pytest.mark.parametrize("name", SELK_NAMED)
def test_select_k(dev, name):
    check_select_k(dev, name)


# ------------------------------------------------------------------ b) one wave per row
def t64(a):
    return torch.from_numpy(np.array(a, np.float64)).requires_grad_(True)


def cos64(x, y, formula=False):
    """F.cosine_similarity, or (where a norm is below the clamp) x.y / (clamp(|x|, 1e-8) clamp(|y|, 1e-8)) spelled out, with the
    float32 value of the 1e-8 the kernels hold"""
    if not formula:
        return F.cosine_similarity(x, y, dim=-1, eps=1e-8)
    nx = torch.linalg.vector_norm(x, dim=-1).clamp_min(CLAMP)
    ny = torch.linalg.vector_norm(y, dim=-1).clamp_min(CLAMP)
    return (x * y).sum(-1) / (nx * ny)


def cos_parts(X, Y):
    """float64: clamped norms and A' = sum |x y| / (nx ny), the scale of a cosine"""
    X, Y = f64(X), f64(Y)
    nx = np.maximum(np.sqrt((X * X).sum(-1)), CLAMP)
    ny = np.maximum(np.sqrt((Y * Y).sum(-1)), CLAMP)
    return nx, ny, np.abs(X * Y).sum(-1) / (nx * ny)


ROW_SHAPES = [(1, 1), (3, 2), (5, 63), (9, 64), (3, 65), (5, 130), (9, 200)]


def check_pair_distance(be, n, D, euclid, kind="plain"):
    """slic_pair_distance and its backward.  kind 'dup': one row of Y equals X's (euclidean: the distance is sqrt(D) 1e-6, the
    gradient finite); kind 'zero': one all-zero row of X (cosine: the per-norm clamp)"""
    rng = np.random.default_rng(100 * n + D + euclid)
    X, Y, G = f32(rng.standard_normal((n, D))), f32(rng.standard_normal((n, D))), f32(rng.standard_normal(n))
    if kind == "dup":
        Y[n // 2] = X[n // 2]
    if kind == "zero":
        X[0] = 0
    (out,) = twice(lambda: [be.pair_distance(X, Y, euclid)])
    x, y = t64(X), t64(Y)
    what = (n, D, euclid, kind)
    if euclid:
        d = F.pairwise_distance(x, y, eps=EPS6)
        dn = d.detach().numpy()
        gate("pair_distance.euclid", out, dn, dn, c_euclid(D), what)
        if kind == "dup":
            assert abs(out[n // 2] / (np.sqrt(D) * EPS6) - 1) < 1e-5
    else:
        d = 1 - cos64(x, y, kind == "zero")
        dn = d.detach().numpy()
        A = cos_parts(X, Y)[2]
        gate("pair_distance.cos", out, dn, A + np.abs(dn), cc(D) + 1, what)            # cc(D) on the cosine, one for 1 - c
    gx, gy = torch.autograd.grad(d, [x, y], torch.from_numpy(f64(G)))
    dX, dY = twice(lambda: be.pair_distance_bwd(X, Y, G, euclid))
    g = np.abs(f64(G))[:, None]
    if euclid:
        dk = np.abs(f64(X) - f64(Y) + EPS6)
        s = g * dk / dn[:, None]
        # (x - y + eps) * (g / d): two roundings in the difference, the distance's c_euclid(D), the division, the product
        for name, got, ref in (("dX", dX, gx), ("dY", dY, gy)):
            gate("pair_distance_bwd.euclid." + name, got, ref.numpy(), s, c_euclid(D) + 7, what)
    else:
        nx, ny, A = cos_parts(X, Y)
        nx, ny, A = nx[:, None], ny[:, None], A[:, None]
        # inv = 1 / (nx ny): steps(D) + 4; c / nx^2 with c's own cc(D) A': together below cc(D) + 8 of the absolute terms
        gate("pair_distance_bwd.cos.dX", dX, gx.numpy(), g * (np.abs(f64(Y)) / (nx * ny) + A * np.abs(f64(X)) / nx ** 2), cc(D) + 8, what)
        gate("pair_distance_bwd.cos.dY", dY, gy.numpy(), g * (np.abs(f64(X)) / (nx * ny) + A * np.abs(f64(Y)) / ny ** 2), cc(D) + 8, what)


def check_pdist(be, n, m, D, euclid, eps):
    """slic_pdist (m None) or slic_pdist2: the gates of slic_pair_distance; on the diagonal of pdist the euclidean distance is
    sqrt(D) eps from the eps inside the norm"""
    rng = np.random.default_rng(n + D + euclid)
    X = f32(rng.standard_normal((n, D)))
    Y = X if m is None else f32(rng.standard_normal((m, D)))
    (out,) = twice(lambda: [be.pdist(X, eps, euclid) if m is None else be.pdist2(X, Y, eps, euclid)])
    x, y = f64(X)[:, None, :], f64(Y)[None, :, :]
    if euclid:
        ref = np.sqrt(((x - y + float(F32(eps))) ** 2).sum(-1))
        gate("pdist.euclid", out, ref, ref, c_euclid(D), (n, m, D))
    else:
        nx, ny, A = cos_parts(x, y)
        ref = 1 - (x * y).sum(-1) / (nx * ny)
        gate("pdist.cos", out, ref, A + np.abs(ref), cc(D) + 1, (n, m, D))


def margin_data(n, D, euclid, margin):
    rng = np.random.default_rng(10 * n + D + euclid)
    X, Y, Z = (f32(rng.standard_normal((n, D))) for _ in range(3))
    if n >= 3:                                            # row 0: hinge inactive
        Y[0] = X[0]
        Z[0] = X[0] + 3 if euclid else -X[0]
    if margin == 0:                                       # last row: v exactly 0
        Z[n - 1] = Y[n - 1]
    return X, Y, Z


def check_margin(be, n, D, euclid, margin, gscale):
    """slic_margin_cos / slic_margin_euclid, forward and backward against autograd of mean(relu(d1 - d2 + margin))"""
    X, Y, Z = margin_data(n, D, euclid, margin)
    st, rl, loss = twice(lambda: be.margin_fwd(X, Y, Z, margin, euclid))
    x, y, z = t64(X), t64(Y), t64(Z)
    if euclid:
        d1, d2 = F.pairwise_distance(x, y, eps=EPS6), F.pairwise_distance(x, z, eps=EPS6)
    else:
        d1, d2 = 1 - cos64(x, y), 1 - cos64(x, z)
    v = d1 - d2 + margin
    vn = v.detach().numpy()
    if margin == 0:
        assert vn[n - 1] == 0 and rl[n - 1] == 0
    quiet = np.abs(vn) > 1e-3
    quiet[n - 1] |= margin == 0
    assert quiet.all(), "a hinge too close to 0 to compare gradients"
    ref_rl = F.relu(v)
    ref_loss = ref_rl.mean()
    d1n, d2n = d1.detach().numpy(), d2.detach().numpy()
    what = (n, D, euclid, margin, gscale)
    if euclid:
        s_row, coef = d1n + d2n + abs(margin) + np.abs(vn), c_euclid(D) + 2              # two distances, the two adds
    else:
        (nx, ny, A1), (_, nz, A2) = cos_parts(X, Y), cos_parts(X, Z)
        s_row, coef = A1 + A2 + np.abs(d1n) + np.abs(d2n) + abs(margin) + np.abs(vn), cc(D) + 3      # two cosines, the three adds
    kind = "euclid" if euclid else "cos"
    gate(f"margin_{kind}.rowloss", rl, ref_rl.detach().numpy(), s_row, coef, what)
    gate(f"margin_{kind}.loss", loss, ref_loss.item(), s_row.mean() + abs(ref_loss.item()), coef + 1, what)
    gs = 1.0 if gscale is None else gscale
    gx, gy, gz = torch.autograd.grad(ref_loss * gs, [x, y, z])
    dX, dY, dZ = twice(lambda: be.margin_bwd(X, Y, Z, st, gscale, euclid))
    g0 = ((vn > 0) * gs / n)[:, None]
    aX, aY, aZ = np.abs(f64(X)), np.abs(f64(Y)), np.abs(f64(Z))
    if euclid:
        ky, kz = np.abs(f64(X) - f64(Y) + EPS6) / d1n[:, None], np.abs(f64(X) - f64(Z) + EPS6) / d2n[:, None]
        sc = (g0 * (ky + kz), g0 * ky, g0 * kz)
        coef = c_euclid(D) + 8                            # as slic_pair_distance_bwd, and g = active gscale / n
    else:
        nx, ny, nz, A1, A2 = (t[:, None] for t in (nx, ny, nz, A1, A2))
        sc = (g0 * (aY / (nx * ny) + aZ / (nx * nz) + (A1 + A2) * aX / nx ** 2), g0 * (aX / (nx * ny) + A1 * aY / ny ** 2),
              g0 * (aX / (nx * nz) + A2 * aZ / nz ** 2))
        coef = cc(D) + 10                                 # as slic_pair_distance_bwd, g = active gscale / n, the sum of two terms
    for name, got, ref, s in zip("XYZ", (dX, dY, dZ), (gx, gy, gz), sc):
        gate(f"margin_{kind}_bwd.d{name}", got, ref.numpy(), s, coef, what)
        assert not got[vn <= 0].any(), "an inactive row has a gradient"


INFONCE_T = 0.25


def check_infonce_rows(be, P, NY, D, gscale):
    """slic_infonce_rows_fwd / _bwd against autograd of mean(logsumexp(cos / T) - cos_0 / T); state is [P][18]"""
    rng = np.random.default_rng(P + 10 * NY + D)
    X, Y = f32(rng.standard_normal((P, D))), f32(rng.standard_normal((P, NY, D)))
    Y[:, 0] = X + f32(0.5 * rng.standard_normal((P, D)))
    st, rl, loss = twice(lambda: be.infonce_fwd(X, Y, INFONCE_T))
    assert st.shape == (P, 18)
    x, y = t64(X), t64(Y)
    invT = 1.0 / float(F32(INFONCE_T))
    s = cos64(x[:, None, :], y) * invT
    ref_rl = torch.logsumexp(s, 1) - s[:, 0]
    ref_loss = ref_rl.mean()
    rn = ref_rl.detach().numpy()
    cs = invT * (cc(D) + 3)             # a logit: the cosine (A' <= 1), 1 - (1 - c), the product with 1 / T
    coef = int(2 * cs) + NY + 8         # exp and log carry the logits' error; NY adds, four transcendental calls and a division
    what = (P, NY, D, gscale)
    gate("infonce_rows.rowloss", rl, rn, 1 + np.abs(rn), coef, what)
    gate("infonce_rows.loss", loss, ref_loss.item(), 1 + abs(ref_loss.item()), coef + 1, what)
    gs = 1.0 if gscale is None else gscale
    gx, gy = torch.autograd.grad(ref_loss * gs, [x, y])
    dX, dY = twice(lambda: be.infonce_bwd(X, Y, st, INFONCE_T, gscale))
    p = torch.softmax(s, 1).detach().numpy()
    t = np.zeros_like(p)
    t[:, 0] = 1
    W = (gs / P * invT * (p + np.abs(p - t)))[:, :, None]
    nx, ny, A = cos_parts(f64(X)[:, None, :], Y)
    nx, ny, A = nx[:, :, None], ny[:, :, None], A[:, :, None]
    aX, aY = np.abs(f64(X))[:, None, :], np.abs(f64(Y))
    sY = W * (aX / (nx * ny) + A * aY / ny ** 2)
    sX = (W * (aY / (nx * ny) + A * aX / nx ** 2)).sum(1)
    coef = int(cs) + NY + 12 + cc(D) + 6                  # the softmax weight (one logit, Z, exp, divisions) times a cosine gradient
    gate("infonce_rows_bwd.dY", dY, gy.numpy(), sY, coef, what)
    gate("infonce_rows_bwd.dX", dX, gx.numpy(), sX, coef + NY, what)


@pytest.mark.parametrize("n,D", ROW_SHAPES)
@pytest.mark.parametrize("euclid", [0, 1])
def test_pair_distance(dev, n, D, euclid):
    check_pair_distance(dev, n, D, euclid)


@pytest.mark.parametrize("D", [2, 65, 200])
def test_pair_distance_identical_rows(dev, D):
    check_pair_distance(dev, 5, D, 1, "dup")


@pytest.mark.parametrize("D", [2, 63, 130])
def test_pair_distance_zero_row(dev, D):
    check_pair_distance(dev, 3, D, 0, "zero")


@pytest.mark.parametrize("m", [None, 7])
@pytest.mark.parametrize("D", [63, 130])
@pytest.mark.parametrize("euclid,eps", [(0, 0.0), (1, 0.25), (1, 0.0)])
def test_pdist(dev, m, D, euclid, eps):
    check_pdist(dev, 9 if m is None else 3, m, D, euclid, eps)


MARGIN_CASES = [(1, 2, 0.25, None), (3, 1, 0.25, 1.5), (5, 63, 0.0, None), (9, 64, 0.25, 1.5), (3, 65, 0.0, 1.5), (5, 130, 0.25, None),
                (9, 200, 0.0, 1.5)]


@pytest.mark.parametrize("n,D,margin,gscale", MARGIN_CASES)
@pytest.mark.parametrize("euclid", [0, 1])
def test_margin(dev, n, D, margin, gscale, euclid):
    check_margin(dev, n, D, euclid, margin, gscale)


INFONCE_CASES = [(1, 2, 1, None), (5, 6, 63, 1.5), (5, 8, 64, None), (1, 8, 65, 1.5), (5, 2, 130, None), (5, 6, 200, 1.5)]


@pytest.mark.parametrize("P,NY,D,gscale", INFONCE_CASES)
def test_infonce_rows(dev, P, NY, D, gscale):
    check_infonce_rows(dev, P, NY, D, gscale)


# ------------------------------------------------------------------ c) NT-Xent
NTX_T = 0.25


def check_ntxent(be, n, D, gscale, tiny=False):
    """slic_ntxent_fwd + _bwd on an input of row stride D + 3 (padding NaN: never read) into an output of row stride D + 5
    (padding NaN afterwards), against autograd of the header's formula.  In units of 2^-24:
      cs = (D + steps(D) + 7) / T   a logit: D MFMA accumulations of entries below 1, the two normalisations, 1 - (1 - S), / T
      cl = cs + ceil(n / 64) + 10   a row's log-sum-exp: the logits, the chain of adds, expf and logf
      loss, on 1 + |loss|:          cs + cl + 2
      dE: p_ij carries cs + cl + 4 relatively; H e_hat adds n fused steps (one thread, j ascending); the projection and the
          division by the norm add steps(D) + 10"""
    rng = np.random.default_rng(n + D)
    lde, ldd = D + 3, D + 5
    E = f32(rng.standard_normal((n, D)))
    h = n // 2
    E[h:2 * h] = E[:h] + f32(0.3 * rng.standard_normal((h, D)))
    if tiny:
        E[1] *= F32(1e-30)
    pad = np.full((n, lde), np.nan, F32)
    pad[:, :D] = E
    loss, dE = twice(lambda: be.ntxent(pad.ravel(), n, D, lde, NTX_T, gscale, ldd))
    assert dE.shape == (n, ldd) and np.isnan(dE[:, D:]).all(), "padding columns of dE written"
    e = t64(E)
    invT = 1.0 / float(F32(NTX_T))
    eh = e / torch.linalg.vector_norm(e, dim=1, keepdim=True).clamp_min(CLAMP)
    eye = torch.eye(n, dtype=torch.bool)
    s = (eh @ eh.T).masked_fill(eye, 0.0) * invT
    tgt = (n // 2 + torch.arange(n)) % n
    lse = torch.logsumexp(s, 1)
    ref_loss = (lse - s[torch.arange(n), tgt]).mean()
    gs = 1.0 if gscale is None else gscale
    (ge,) = torch.autograd.grad(ref_loss * gs, [e])
    cs = invT * (D + steps(D) + 7)
    cl = cs + -(-n // 64) + 10
    what = (n, D, gscale, tiny)
    gate("ntxent.loss", loss, ref_loss.item(), 1 + abs(ref_loss.item()), int(cs + cl) + 2, what)
    p = torch.softmax(s, 1).detach().numpy()
    t = np.zeros((n, n))
    t[np.arange(n), tgt.numpy()] = 1
    Habs = p + p.T + t + t.T
    np.fill_diagonal(Habs, 0)
    ehn = np.abs(eh.detach().numpy())
    rn = 1.0 / np.maximum(np.sqrt((f64(E) ** 2).sum(1)), CLAMP)
    Babs = gs * invT / n * (Habs @ ehn)
    scale = rn[:, None] * (Babs + ehn * (Babs * ehn).sum(1, keepdims=True))
    gate("ntxent.dE", dE[:, :D], ge.numpy(), scale, int(cs + cl) + 4 + n + steps(D) + 10, what)


NTX_CASES = [(2, 2, None, False), (6, 6, 1.5, False), (33, 66, None, False), (66, 6, 1.5, False), (130, 66, 1.5, False),
             (130, 2, None, False), (8, 6, None, True)]


@pytest.mark.parametrize("n,D,gscale,tiny", NTX_CASES)
def test_ntxent(dev, n, D, gscale, tiny):
    check_ntxent(dev, n, D, gscale, tiny)


EUCL_T = 0.5


def check_ntxent_euclid(be, n, D, gscale):
    """slic_ntxent_euclid_fwd / _bwd against autograd of the header's formula; rows 0 and n - 1 are identical (n >= 4): their
    distance is 0, the pair contributes nothing to dE, everything stays finite.  With s = (1 - d) / T a logit carries
    about c_euclid(D) (1 + d) / T units (the distance, 1 - d, the product): folded into the scales as amp = 1 + (1 + d) / T."""
    rng = np.random.default_rng(n + D)
    E = f32(0.3 * rng.standard_normal((n, D)))
    if n >= 4:
        E[n - 1] = E[0]
    dist, wm, rl, loss = twice(lambda: be.ntxent_euclid_fwd(E, EUCL_T))
    e = t64(E)
    invT = 1.0 / float(F32(EUCL_T))
    d = torch.linalg.vector_norm(e[:, None, :] - e[None, :, :], dim=-1)
    eye = torch.eye(n, dtype=torch.bool)
    s = ((1 - d) * invT).masked_fill(eye, 0.0)
    tgt = (n // 2 + torch.arange(n)) % n
    ref_rl = torch.logsumexp(s, 1) - s[torch.arange(n), tgt]
    ref_loss = ref_rl.mean()
    dn = d.detach().numpy()
    what = (n, D, gscale)
    if n >= 4:
        assert dist[0, n - 1] == 0 and dist[n - 1, 0] == 0
    gate("ntxent_euclid.dist", dist, dn, dn, c_euclid(D) - 2, what)                   # as c_euclid, one rounding a difference (no eps)
    p = torch.softmax(s, 1).detach().numpy()
    amp = 1 + (1 + dn) * invT
    rn = ref_rl.detach().numpy()
    s_row = 1 + np.abs(rn) + (p * amp).sum(1) + amp[np.arange(n), tgt.numpy()]
    coef = steps(D) + -(-n // 256) + 24                   # two logits' worth, the chain of adds, expf, logf, max shift
    gate("ntxent_euclid.rowloss", rl, rn, s_row, coef, what)
    gate("ntxent_euclid.loss", loss, ref_loss.item(), s_row.mean(), coef + 1, what)
    gs = 1.0 if gscale is None else gscale
    (ge,) = torch.autograd.grad(ref_loss * gs, [e])
    dE = twice(lambda: [be.ntxent_euclid_bwd(E, dist, wm, gscale)])[0]
    t = np.zeros((n, n))
    t[np.arange(n), tgt.numpy()] = 1
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(dn > 0, gs / n * invT * (p + p.T + t + t.T) * (amp + np.abs(np.log(p)) + np.abs(np.log(p)).T) / dn, 0.0)
    np.fill_diagonal(w, 0)
    scale = (w[:, :, None] * np.abs(f64(E)[:, None, :] - f64(E)[None, :, :])).sum(1)
    # p = exp(s - lse): its argument's error (amp, |s - lse| once rounded) is in the scale; then n fused steps of one thread
    gate("ntxent_euclid.dE", dE, ge.numpy(), scale, coef + n + 6, what)


EUCL_CASES = [(2, 3, None), (8, 70, 1.5), (258, 3, 1.5), (260, 70, None), (258, 70, None)]


@pytest.mark.parametrize("n,D,gscale", EUCL_CASES)
def test_ntxent_euclid(dev, n, D, gscale):
    check_ntxent_euclid(dev, n, D, gscale)


# ------------------------------------------------------------------ d) memory-bank NCE
NCE_T = 0.07
NBANK = 50


def unit_rows(rng, shape):
    a = rng.standard_normal(shape)
    return f32(a / np.sqrt((a * a).sum(-1, keepdims=True)))


def nce_idx(rng, B, K1):
    idx = rng.integers(0, NBANK, (B, K1)).astype(np.int64)
    if K1 > 1:
        idx[0, K1 - 1] = idx[0, 0]                        # a repeat even where K1 is small
    return idx


def c_dot4(D):
    """a 32-lane row dot: four fused steps per 128 columns, five butterfly adds, 1 / T and the product with it"""
    return 4 * -(-D // 128) + 7


def check_nce_scores_fwd(be, B, K1, D, gather):
    rng = np.random.default_rng(B + K1 + D)
    bank, f, idx = unit_rows(rng, (NBANK, D)), unit_rows(rng, (B, D)), nce_idx(rng, B, K1)
    out, g = twice(lambda: be.nce_scores_fwd(bank, idx, f, NCE_T, gather))
    invT = 1.0 / float(F32(NCE_T))
    terms = f64(bank)[idx] * f64(f)[:, None, :]
    gate("nce_scores_fwd", out, terms.sum(-1) * invT, np.abs(terms).sum(-1) * invT, c_dot4(D), (B, K1, D))
    assert (g is not None) == bool(gather)
    if gather:
        assert bits_equal(g, bank[idx]), "gathered rows are not bank[idx]"


def check_nce_scores_bwd(be, B, K1, D):
    rng = np.random.default_rng(B + K1 + D)
    bank, idx, dout = unit_rows(rng, (NBANK, D)), nce_idx(rng, B, K1), f32(rng.standard_normal((B, K1)))
    (df,) = twice(lambda: [be.nce_scores_bwd(bank, idx, dout, NCE_T)])
    invT = 1.0 / float(F32(NCE_T))
    terms = f64(bank)[idx] * f64(dout)[:, :, None]
    # a 32-lane group adds ceil(K1 / 8) products (two roundings each), eight groups are summed, 1 / T and the product
    gate("nce_scores_bwd", df, terms.sum(1) * invT, np.abs(terms).sum(1) * invT, 2 * -(-K1 // 8) + 10, (B, K1, D))


def updated64(bank, y, f, mom):
    """float64 rows and scales of the momentum update, each row from the bank as it was; the last of duplicate labels wins"""
    ref, scale = f64(bank).copy(), np.zeros(bank.shape)
    m = float(F32(mom))
    for b in range(len(y)):
        a, c = f64(bank)[y[b]] * m, f64(f)[b] * (1 - m)
        v, V = a + c, np.abs(a) + np.abs(c)
        nrm = np.sqrt((v * v).sum())
        ref[y[b]] = v / nrm
        scale[y[b]] = (V + np.abs(v) * (V * np.abs(v)).sum() / nrm ** 2) / nrm
    return ref, scale


def gate_bank(name, got, bank, y, f, mom, D, what):
    """v = m row + (1 - m) f: three roundings on |m row| + |(1 - m) f| =: V; the norm carries 3 sum(V |v|) / |v|^2 from those and
    steps(D) / 2 + 1 of its own; one division.  Rows not named by y keep their bits."""
    ref, scale = updated64(bank, y, f, mom)
    rows = np.unique(y)
    gate(name, got[rows], ref[rows], scale[rows], steps(D) // 2 + 6, what)
    rest = np.setdiff1d(np.arange(len(bank)), rows)
    assert bits_equal(got[rest], bank[rest]), "an untouched bank row changed"


def check_nce_bank_update(be, B, D):
    rng = np.random.default_rng(B + D)
    bank, f = unit_rows(rng, (NBANK, D)), unit_rows(rng, (B, D))
    y = rng.permutation(NBANK)[:B].astype(np.int64)       # distinct: the unfused update documents a race on duplicates
    (got,) = twice(lambda: [be.nce_bank_update(bank, y, f, 0.5)])
    gate_bank("nce_bank_update", got, bank, y, f, 0.5, D, (B, D))


def ce0_scale(x):
    """float64 log-sum-exp of the rows of x and the scale of its float32 evaluation: 1 + |lse| + sum_j p_j |x_j - max| (the rounding
    of each shifted logit enters its exponential relatively)"""
    x = f64(x)
    m = x.max(-1, keepdims=True)
    lse = m[..., 0] + np.log(np.exp(x - m).sum(-1))
    p = np.exp(x - lse[..., None])
    return lse, p, 1 + np.abs(lse) + (p * np.abs(x - m)).sum(-1)


def check_ce0(be, B, K1, gscale):
    """slic_softmax_ce0_fwd, and _bwd fed the float32-rounded float64 log-sum-exp; row 0 holds +100 and -100"""
    rng = np.random.default_rng(B + K1)
    x = f32(3 * rng.standard_normal((B, K1)))
    x[0, 0::2], x[0, 1::2] = 100, -100
    lse, rl, loss = twice(lambda: be.ce0_fwd(x))
    ref, p, s = ce0_scale(x)
    coef = -(-K1 // 256) + 14                             # a thread's adds, six butterfly adds and three of the waves, expf, logf, the shift
    what = (B, K1, gscale)
    gate("softmax_ce0.lse", lse, ref, s, coef, what)
    gate("softmax_ce0.rowloss", rl, ref - f64(x)[:, 0], s + np.abs(f64(x)[:, 0]), coef + 1, what)
    gate("softmax_ce0.loss", loss, (ref - f64(x)[:, 0]).mean(), (s + np.abs(f64(x)[:, 0])).mean(), coef + 2, what)
    lse32 = f32(ref)
    xt = t64(x)
    gs = 1.0 if gscale is None else gscale
    (gx,) = torch.autograd.grad((torch.logsumexp(xt, 1) - xt[:, 0]).mean() * gs, [xt])
    (dx,) = twice(lambda: [be.ce0_bwd(x, lse32, gscale)])
    t = np.zeros_like(p)
    t[:, 0] = 1
    arg = np.abs(f64(x) - ref[:, None]) + np.abs(ref)[:, None]
    # x - lse rounds once and lse itself was rounded (both enter p relatively: in the scale); expf, the subtraction, g = gscale / B, the product
    gate("softmax_ce0_bwd", dx, gx.numpy(), gs / B * (p * (1 + arg) + np.abs(p - t)), 6, what)


def fused_data(B, K1, D, dup=True):
    rng = np.random.default_rng(B + K1 + D)
    bl, bab = unit_rows(rng, (NBANK, D)), unit_rows(rng, (NBANK, D))
    fl, fab = unit_rows(rng, (B, D)), unit_rows(rng, (B, D))
    y = rng.permutation(NBANK)[:B].astype(np.int64)
    if dup and B >= 3:
        y[B - 1] = y[0]                                   # a duplicated label: the last row wins
    return bl, bab, fl, fab, nce_idx(rng, B, K1), y


def c_lse(K1, D):
    """the fused log-sum-exp: the scores' own c_dot4(D); an online step is two expf, a product and an add (8 units) over
    ceil(K1 / 128) steps a group; 8 groups and 16 parts merged with an expf and a fused step each (3 units); logf and the shift"""
    return c_dot4(D) + 8 * -(-K1 // 128) + 3 * 24 + 4


def check_nce_fused(be, B, K1, D, gscale):
    """slic_nce_fused_fwd -> _update -> _bwd as the training step chains them, against float64 and autograd of
    sum over the two sides of mean_b(logsumexp(scores) - scores[:, 0]); side 0 is feature ab against memory_l"""
    bl, bab, fl, fab, idx, y = fused_data(B, K1, D)
    sc, rows, part = twice(lambda: be.fused_fwd(bl, bab, fl, fab, idx, NCE_T))
    assert bits_equal(rows[0], bl[idx]) and bits_equal(rows[1], bab[idx]), "rows are not the gathered bank rows"
    invT = 1.0 / float(F32(NCE_T))
    tfl, tfab = t64(fl), t64(fab)
    r0, r1 = torch.from_numpy(f64(bl)[idx]), torch.from_numpy(f64(bab)[idx])
    s = torch.stack([(r0 * tfab[:, None, :]).sum(-1), (r1 * tfl[:, None, :]).sum(-1)]) * invT
    s_abs = (torch.stack([(r0 * tfab[:, None, :]).abs().sum(-1), (r1 * tfl[:, None, :]).abs().sum(-1)]) * invT).detach().numpy()
    what = (B, K1, D, gscale)
    gate("nce_fused_fwd.scores", sc, s.detach().numpy(), s_abs, c_dot4(D), what)
    nbl, nbab, lse, rl, loss = twice(lambda: be.fused_update(bl, bab, y, fl, fab, 0.5, part, sc))
    gate_bank("nce_fused_update.bank_l", nbl, bl, y, fl, 0.5, D, what)
    gate_bank("nce_fused_update.bank_ab", nbab, bab, y, fab, 0.5, D, what)
    ref_lse, p, s0 = ce0_scale(s.detach().numpy())
    s_lse = s0 + (p * s_abs).sum(-1)                      # each score's own error enters the log-sum-exp with weight p_j
    coef = c_lse(K1, D)
    gate("nce_fused_update.lse", lse, ref_lse, s_lse, coef, what)
    ref_rl = ref_lse - s.detach().numpy()[:, :, 0]
    gate("nce_fused_update.rowloss", rl, ref_rl, s_lse + s_abs[:, :, 0], coef + 1, what)
    gate("nce_fused_update.loss", loss, ref_rl.mean(1).sum(), (s_lse + s_abs[:, :, 0]).mean(1).sum(), coef + 3, what)
    # without `part`: the same banks, no loss output touched
    b2l, b2ab, none1, none2, none3 = be.fused_update(bl, bab, y, fl, fab, 0.5, None, None)
    assert bits_equal(b2l, nbl) and bits_equal(b2ab, nbab) and none1 is None and none2 is None and none3 is None
    gs = 1.0 if gscale is None else gscale
    ref_loss = (torch.logsumexp(s, 2) - s[:, :, 0]).mean(1).sum()
    gab, gl = torch.autograd.grad(ref_loss * gs, [tfab, tfl])
    (df,) = twice(lambda: [be.fused_bwd(rows, sc, lse, NCE_T, gscale)])
    assert df.shape == (2, B, D)
    t = np.zeros_like(p)
    t[:, :, 0] = 1
    sn = s.detach().numpy()
    # p_j = exp(score_j - lse): the errors of both (in units of their own scales) enter relatively
    amp = 1 + np.abs(sn - ref_lse[..., None]) + s_abs + s_lse[..., None]
    w = gs / B * invT * (p * amp + np.abs(p - t))
    scale = (w[..., None] * np.abs(np.stack([f64(bl)[idx], f64(bab)[idx]]))).sum(2)
    # a group adds ceil(K1 / 32) products (two roundings each), 32 groups are summed; g, 1 / T; p_j's relative error is c_lse
    gate("nce_fused_bwd.chain", df, np.stack([gab.numpy(), gl.numpy()]), scale, 2 * -(-K1 // 32) + 36 + coef, what)


def check_nce_fused_bwd(be, B, K1, D, gscale):
    """slic_nce_fused_bwd alone, fed float32 scores, rows and the float32-rounded float64 log-sum-exp of those scores"""
    rng = np.random.default_rng(B + K1 + D)
    rows, sc = unit_rows(rng, (2, B, K1, D)), f32(3 * rng.standard_normal((2, B, K1)))
    ref_lse, p, _ = ce0_scale(sc)
    lse32 = f32(ref_lse)
    (df,) = twice(lambda: [be.fused_bwd(rows, sc, lse32, NCE_T, gscale)])
    st = t64(sc)
    gs = 1.0 if gscale is None else gscale
    (gsc,) = torch.autograd.grad((torch.logsumexp(st, 2) - st[:, :, 0]).mean(1).sum() * gs, [st])
    invT = 1.0 / float(F32(NCE_T))
    ref = (gsc.numpy()[..., None] * f64(rows)).sum(2) * invT
    t = np.zeros_like(p)
    t[:, :, 0] = 1
    amp = 1 + np.abs(f64(sc) - ref_lse[..., None]) + np.abs(ref_lse)[..., None]
    w = gs / B * invT * (p * amp + np.abs(p - t))
    scale = (w[..., None] * np.abs(f64(rows))).sum(2)
    # expf of a once-rounded argument (in the scale), the subtraction, g = gscale / B; ceil(K1 / 32) products of two roundings a
    # group, 32 groups summed, 1 / T
    gate("nce_fused_bwd", df, ref, scale, 2 * -(-K1 // 32) + 40, (B, K1, D, gscale))


SCORES_FWD_CASES = [(1, 1, 4, 0), (3, 7, 64, 1), (1, 9, 132, 1), (3, 515, 260, 0), (1, 515, 132, 1), (3, 9, 260, 1), (3, 7, 4, 0)]
SCORES_BWD_CASES = [(B, K1, D) for K1, B, D in [(1, 1, 4), (8, 3, 132), (25, 1, 260), (32, 3, 4), (33, 1, 132), (57, 3, 260), (70, 3, 132),
                                               (70, 1, 4)]]
FUSED_CASES = [(1, 1, 4, None), (3, 15, 132, 1.5), (3, 17, 260, None), (1, 130, 132, 1.5), (3, 130, 4, None), (3, 1, 260, 1.5)]
FUSED_BWD_CASES = [(1, 1, 132, None), (3, 32, 4, 1.5), (1, 97, 260, None), (3, 129, 132, 1.5), (3, 260, 260, None), (1, 260, 4, 1.5)]


@pytest.mark.parametrize("B,K1,D,gather", SCORES_FWD_CASES)
def test_nce_scores_fwd(dev, B, K1, D, gather):
    check_nce_scores_fwd(dev, B, K1, D, gather)


@pytest.mark.parametrize("B,K1,D", SCORES_BWD_CASES)
def test_nce_scores_bwd(dev, B, K1, D):
    check_nce_scores_bwd(dev, B, K1, D)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("D", [4, 65, 130])
def test_nce_bank_update(dev, B, D):
    check_nce_bank_update(dev, B, D)


@pytest.mark.parametrize("K1", [1, 2, 255, 257, 600])
@pytest.mark.parametrize("B,gscale", [(1, None), (3, 1.5)])
def test_softmax_ce0(dev, B, K1, gscale):
    check_ce0(dev, B, K1, gscale)


@pytest.mark.parametrize("B,K1,D,gscale", FUSED_CASES)
def test_nce_fused_chain(dev, B, K1, D, gscale):
    check_nce_fused(dev, B, K1, D, gscale)


@pytest.mark.parametrize("B,K1,D,gscale", FUSED_BWD_CASES)
def test_nce_fused_bwd(dev, B, K1, D, gscale):
    check_nce_fused_bwd(dev, B, K1, D, gscale)

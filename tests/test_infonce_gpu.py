"""GPU: the rank of the best positive (slic_moco_topk_hits, slic_mask_topk_hits) against the float64 NumPy provider
(tests/infonce_cpu_kernels.py), and the InfoNCE / UberNCE models (models/infoNCE.py) against the reference's goldens
(tests/golden/infonce.npz).

Ranks are integers, compared for equality.  A device logit is within the logit gate of tests/test_moco_gpu.py of its float64 value,
so a row whose saturated float64 rank changes when its positives move by +- that gate has no single right answer: such rows are
skipped, at most 5 % of a case, never all.  Rows with planted bit-equal logits have one: the lower column goes first."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import infonce_cpu_kernels as ref
import moco_cpu_kernels as ref64
from test_moco_gpu import SHAPES, T, dev, gate, unit

pytestmark = pytest.mark.gpu
TOPKS = [(1, 5), (1, 2, 8)]


def kernels():
    from video_similarity_search_amd.models.infoNCE import HipInfoNCEKernels
    return HipInfoNCEKernels()


def mixed_queries(rng, k, D, K):
    """unit rows a_b k_b + sqrt(1 - a_b^2) u_b with <q_b, k_b> = a_b spread around the largest of K random dot products (standard
    deviation 1 / sqrt(D), largest about sqrt(2 ln K) of them): column 0 lands anywhere between about tenth and first"""
    B = k.shape[0]
    top = np.sqrt(2 * np.log(K))
    u = unit(rng, B, D).astype(np.float64)
    u -= (u * k).sum(1, keepdims=True) * k
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a = rng.permutation(np.linspace(top - 1.8, top + 0.1, B) if B > 1 else np.array([top]))[:, None] / np.sqrt(D)
    a = np.minimum(a, 0.95)
    return (a * k + np.sqrt(1 - a * a) * u).astype(np.float32)


def labels_for(rng, B, K):
    """about two positives per class in the queue, empty slots, a label the queue does not hold, a query without a label"""
    ql = rng.integers(0, max(K // 2, 1), K).astype(np.int64)
    ql[rng.choice(K, K // 8, replace=False)] = -1
    ql[ql == 3] = 4
    kl = rng.integers(0, max(K // 2, 1), B).astype(np.int64)
    kl[0] = 3                                                # absent from the queue
    if B > 1:
        kl[1] = -1                                           # no label: column 0 only, although the queue has -1 slots
    return kl, ql


def logit_gate(q, k, mem):
    x64 = ref64.logits(*(a.astype(np.float64) for a in (q, k, mem)), T)
    qt, kt, mt = (torch.from_numpy(a) for a in (q, k, mem))
    x32 = (torch.cat(((qt * kt).sum(1, keepdim=True), qt @ mt.t()), 1) / T).numpy()
    return x64, gate("logits", q.shape[1], np.abs(x32 - x64).max())


def sat_rank(x64, mask, shift, kmax):
    return np.minimum(ref.rank_of_best(x64 + shift * mask, mask), kmax)


_cases = {}
SEED = 20         # chosen so that the float64 ranks alone meet the test's own conditions (coverage of 0 .. kmax, ambiguity cap)


def case(B, D, K, lab):
    """inputs, float64 logits and gate of one shape, built once"""
    key = (B, D, K, lab)
    if key not in _cases:
        rng = np.random.default_rng(B * 1000 + D + (7 if lab else 0) + SEED)
        k, mem = unit(rng, B, D), unit(rng, K, D)
        q = mixed_queries(rng, k.astype(np.float64), D, K)
        kl, ql = labels_for(rng, B, K) if lab else (None, None)
        x64, g = logit_gate(q, k, mem)
        _cases[key] = (q, k, mem, kl, ql, x64, g, ref64.positives(B, K, kl, ql))
    return _cases[key]


@pytest.mark.parametrize("top_ks", TOPKS)
@pytest.mark.parametrize("lab", [False, True])
@pytest.mark.parametrize("B,D,K", SHAPES)
def test_moco_topk_hits_against_float64(gpu, B, D, K, lab, top_ks):
    q, k, mem, kl, ql, x64, g, mask = case(B, D, K, lab)
    kmax = top_ks[-1]
    want = sat_rank(x64, mask, 0.0, kmax)
    clear = (want == sat_rank(x64, mask, g, kmax)) & (want == sat_rank(x64, mask, -g, kmax))
    if lab:
        assert kl[0] not in ql and (ql == -1).any() and (B == 1 or kl[1] == -1)
    if (B, K) in ((130, 16384),):                            # the two largest shapes: every rank 0 .. kmax occurs
        assert set(want.tolist()) == set(range(kmax + 1)), sorted(set(want.tolist()))
    rank, hits = kernels().topk_hits(dev(q), dev(k), dev(mem), T, None if kl is None else dev(kl), None if ql is None else dev(ql), top_ks)
    rank2, hits2 = kernels().topk_hits(dev(q), dev(k), dev(mem), T, None if kl is None else dev(kl), None if ql is None else dev(ql), top_ks)
    rank, hits = rank.cpu().numpy(), hits.cpu().numpy()
    print((B, D, K), "labels" if lab else "plain", top_ks, "gate", g, "ambiguous", int((~clear).sum()), "of", B, "ranks", np.bincount(want, minlength=kmax + 1).tolist(),
          "mismatches", int((rank != want)[clear].sum()))
    assert (~clear).sum() <= 0.05 * B and clear.any()
    assert np.array_equal(rank[clear], want[clear])
    assert np.array_equal(hits, ref.hits_of(rank, top_ks))                    # hits is the count derived from rank
    assert np.array_equal(rank2.cpu().numpy(), rank) and np.array_equal(hits2.cpu().numpy(), hits)      # two runs: the same bits


@pytest.mark.parametrize("D", [128, 101, 512])
def test_moco_topk_hits_planted_ties(gpu, D):
    """a positive queue row duplicated bit for bit as a non-positive row at a lower and at a higher column: the lower one is ahead,
    the higher one is not"""
    rng = np.random.default_rng(31 + D)
    B, K = 40, 1000
    k, mem = unit(rng, B, D), unit(rng, K, D)
    q = unit(rng, B, D)
    ql = np.full(K, 5, np.int64)
    kl = np.full(B, 9, np.int64)
    want = np.zeros(B, np.int64)
    for b in range(B):                                       # query b is its positive row itself: logit 1 / T, the largest of the row
        pos = 20 + 24 * b
        mem[pos] = q[b]
        ql[pos] = 100 + b
        kl[b] = 100 + b
        if b % 4 in (1, 3):
            mem[pos - 7 - b % 5] = q[b]                      # the same bits at a lower column, another label: ahead
            want[b] += 1
        if b % 4 in (2, 3):
            mem[pos + 5 + b % 3] = q[b]                      # and at a higher column: behind
        if b % 8 == 7:
            mem[pos - 17] = q[b]                             # two lower copies
            want[b] += 1
    x64 = ref64.logits(*(a.astype(np.float64) for a in (q, k, mem)), T)
    assert np.array_equal(ref.rank_of_best(x64, ref64.positives(B, K, kl, ql)), want) and set(want.tolist()) == {0, 1, 2}
    rank, hits = kernels().topk_hits(dev(q), dev(k), dev(mem), T, dev(kl), dev(ql), (1, 2, 8))
    assert np.array_equal(rank.cpu().numpy(), want)
    assert np.array_equal(hits.cpu().numpy(), ref.hits_of(want, (1, 2, 8)))


def test_moco_topk_hits_label_edge_cases_and_arguments(gpu):
    from video_similarity_search_amd import _lib
    rng = np.random.default_rng(41)
    B, D, K = 26, 128, 2048
    k, mem = unit(rng, B, D), unit(rng, K, D)
    q = mixed_queries(rng, k.astype(np.float64), D, K)
    kern = kernels()
    plain_rank, plain_hits = kern.topk_hits(dev(q), dev(k), dev(mem), T, None, None, (1, 5))
    # an all -1 queue, labels absent from the queue, k_label -1 against -1 slots: column 0 is the only positive
    for kl, ql in ((np.arange(B), np.full(K, -1)), (np.arange(B) + 5000, rng.integers(0, 100, K)), (np.full(B, -1), np.full(K, -1))):
        rank, hits = kern.topk_hits(dev(q), dev(k), dev(mem), T, dev(kl.astype(np.int64)), dev(ql.astype(np.int64)), (1, 5))
        assert torch.equal(rank, plain_rank) and torch.equal(hits, plain_hits)
    lib = _lib.load()
    hits = torch.zeros(8, dtype=torch.int32, device="cuda")
    ws = torch.empty(257 * B * 8, dtype=torch.uint8, device="cuda")
    qd, kd, md, kld = dev(q), dev(k), dev(mem), dev(np.arange(B).astype(np.int64))

    def rc(top_ks, n=None, k_label=None, queue_label=None, D_=D):
        ks = (ctypes.c_int32 * 8)(*top_ks)
        return lib.slic_moco_topk_hits(_lib.ptr(qd), _lib.ptr(kd), _lib.ptr(md), B, K, D_, T, _lib.ptr(k_label), _lib.ptr(queue_label), ks,
                                       len(top_ks) if n is None else n, None, _lib.ptr(hits), _lib.ptr(ws), None)
    assert rc((1, 5)) == 0
    torch.cuda.synchronize()
    assert hits[:2].tolist() == plain_hits.tolist()
    for bad in ((5, 1), (1, 1), (0, 1), (1, 9)):
        assert rc(bad) != 0
    assert rc((1,), n=0) != 0 and rc((1, 2, 3, 4, 5, 6, 7, 8), n=9) != 0
    assert rc((1, 5), k_label=kld) != 0                       # labels come together
    assert rc((1, 5), D_=513) != 0
    assert b"slic_moco_topk_hits" in lib.slic_last_error()


def np_mask_rank(x, mask):
    """the definition, row by row: sort by (-logit, column), find the first masked column"""
    out = []
    for xr, mr in zip(x, mask):
        order = np.lexsort((np.arange(len(xr)), -xr))
        pos = np.nonzero(mr[order])[0]
        out.append(pos[0] if len(pos) else len(xr))
    return np.array(out)


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("C", [1, 63, 64, 2049])
def test_mask_topk_hits(gpu, B, C):
    rng = np.random.default_rng(100 * B + C)
    ld, ldm = C + 3, C + 5
    x = rng.integers(-4, 5, (B, ld)).astype(np.float32)       # few distinct values: exact ties in every row
    x[B // 2] = rng.standard_normal(ld)                       # and one row without
    mask = (rng.random((B, ldm)) < min(0.5, 3.0 / C)).astype(np.uint8)
    if B > 1:
        mask[3] = 0                                           # a row without a positive
        mask[4] = 1
    mask[0, :C] = 0
    mask[0, C - 1] = 1                                        # only the last column
    want = np_mask_rank(x[:, :C], mask[:, :C] != 0)
    assert np.array_equal(want, ref.rank_of_best(x[:, :C].astype(np.float64), mask[:, :C] != 0))
    top_ks = tuple(k for k in (1, 5, 64) if k <= C)
    rank, hits = kernels().mask_hits(dev(x)[:, :C], dev(mask)[:, :C], top_ks)
    assert np.array_equal(rank.cpu().numpy(), want)
    assert np.array_equal(hits.cpu().numpy(), ref.hits_of(want, top_ks))
    if B > 1:
        assert want[3] == C and want[4] == 0


def test_calc_mask_accuracy_is_the_reference_counting(gpu):
    """calc_mask_accuracy against the reference's topk + scatter formulation written in torch, on logits without ties"""
    from video_similarity_search_amd.online_train import calc_mask_accuracy
    rng = np.random.default_rng(5)
    B, C = 65, 301
    out = torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32)).cuda()
    mask = torch.from_numpy(rng.random((B, C)) < 0.02).cuda()
    mask[:, 0] = True
    _, pred = out.topk(5, 1, True, True)
    want = [(mask.gather(1, pred[:, :k]).sum(1) >= 1).float().mean() for k in (1, 5)]
    got = calc_mask_accuracy(out, mask, (1, 5))
    assert [float(g) for g in got] == [float(w) for w in want] and got[0].dim() == 0 and got[0].is_cuda
    assert float(calc_mask_accuracy(out, mask, (5,))[0]) == float(want[1])
    with pytest.raises(ValueError):
        calc_mask_accuracy(out, mask[:, :5], (1,))
    with pytest.raises(ValueError):
        calc_mask_accuracy(out, mask, (0,))


# ---------------------------------------------------------------------------------------------------------------------------------
# the projection head and the models
# ---------------------------------------------------------------------------------------------------------------------------------
import sys                                                      # noqa: E402
import torch.nn.functional as F                                 # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_goldens_infonce as gen                              # noqa: E402  (draw_case and the golden shapes)

GM = np.load(os.path.join(ROOT, "tests", "golden", "infonce.npz"))


def mgate(name):
    """4 x the reference's own fp32 deviation from float64 on the golden inputs"""
    return 4.0 * float(GM["dev_" + name])


@pytest.mark.parametrize("B", [1, 5, 70])
def test_head_against_float64(gpu, B):
    rng = np.random.default_rng(50 + B)
    Fw, N = 64, 32
    feat = rng.standard_normal((B, Fw)).astype(np.float32)
    w1 = (rng.standard_normal((Fw, Fw, 1, 1, 1)) * np.sqrt(2.0 / Fw)).astype(np.float32)
    w2 = (rng.standard_normal((N, Fw, 1, 1, 1)) / np.sqrt(Fw)).astype(np.float32)
    b1, b2 = (0.1 * rng.standard_normal(Fw)).astype(np.float32), (0.1 * rng.standard_normal(N)).astype(np.float32)
    dy = rng.standard_normal((B, N)).astype(np.float32)
    args64 = [a.astype(np.float64) for a in (feat, w1, b1, w2, b2)]
    y64 = ref.head(*args64)[0]
    g64 = ref.head_grads(dy.astype(np.float64), *args64)
    # the same op sequence in fp32 torch on the CPU: its deviation from float64 sets the gate (floor: a few ulp of unit-scale values)
    t = [torch.from_numpy(a).requires_grad_(True) for a in (feat, w1, b1, w2, b2)]
    y32 = F.normalize(torch.relu(t[0] @ t[1].view(Fw, Fw).t() + t[2]) @ t[3].view(N, Fw).t() + t[4], dim=1)
    g32 = torch.autograd.grad(y32, t, torch.from_numpy(dy))
    kern = kernels()
    y, saved = kern.head_fwd(*(dev(a) for a in (feat, w1, b1, w2, b2)))
    grads = kern.head_bwd(dev(dy), y, saved, dev(w1), dev(w2), True)
    gy = 4 * max(np.abs(y32.detach().numpy() - y64).max(), 2.0 ** -23)
    assert np.abs(y.cpu().numpy() - y64).max() <= gy
    for got, w64, w32 in zip(grads, g64, g32):
        scale = np.abs(w64).max()
        gg = 4 * max(np.abs(w32.numpy().reshape(w64.shape) - w64).max() / scale, 2.0 ** -23)
        assert np.abs(got.cpu().numpy().reshape(w64.shape) - w64).max() <= gg * scale
    # a zero row goes through the eps clamp: y = 0, a finite gradient
    z = torch.zeros(3, N, device="cuda")
    yz, inv = torch.empty_like(z), torch.empty(3, device="cuda")
    from video_similarity_search_amd._lib import call, ptr, stream
    call("slic_l2normalize_fwd", ptr(z), 3, N, 1e-12, ptr(yz), ptr(inv), stream())
    dz = torch.empty_like(z)
    call("slic_l2normalize_bwd", ptr(torch.ones_like(z)), ptr(yz), ptr(inv), 3, N, ptr(dz), stream())
    assert (yz == 0).all() and torch.isfinite(dz).all()


def golden_model(tag):
    from video_similarity_search_amd.models import generate_model, infoNCE
    import contextlib
    import io
    labelled = tag == "uber"
    sd, blocks = gen.draw_case(211 if tag == "info" else 223, labelled)
    assert np.allclose(gen.checksum(sd, blocks), GM[tag + "/check"], rtol=1e-12)
    with contextlib.redirect_stdout(io.StringIO()):
        m = getattr(infoNCE, "UberNCE" if labelled else "InfoNCE")(lambda: generate_model(10, **gen.TRUNK_KW), gen.DIM, gen.K, gen.M, gen.T)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m.cuda().train(), blocks


def acc_bounds(logits64, mask, ks, g):
    """the accuracies the golden logits allow when the positives move by +- the logit gate (equal bounds: one right answer)"""
    lo = [np.mean(ref.rank_of_best(logits64 - g * mask, mask) < k) for k in ks]
    hi = [np.mean(ref.rank_of_best(logits64 + g * mask, mask) < k) for k in ks]
    return lo, hi


def masked_loss(logits, target):
    return (-(F.log_softmax(logits, dim=1) * target).sum(1) / target.sum(1)).mean()


def check_grads(m, tag, it):
    for n, p in m.encoder_q.named_parameters():
        want = GM[f"{tag}/grad{it}/{n}"]
        got = gen.strided(p.grad.cpu().numpy())
        assert np.abs(got - want).max() <= mgate("grad") * max(np.abs(want).max(), 1e-30), (n, it)


@pytest.mark.parametrize("path", ["forward", "contrast"])
@pytest.mark.parametrize("tag", ["info", "uber"])
def test_golden_steps(gpu, tag, path):
    from video_similarity_search_amd.loss import calc_topk_accuracy
    from video_similarity_search_amd.online_train import calc_mask_accuracy
    labelled = tag == "uber"
    m, blocks = golden_model(tag)
    for it in range(gen.STEPS):
        train = it < gen.STEPS - 1
        blk = dev(blocks[it])
        lab = dev(gen.LABELS[it]) if labelled else None
        w_logits, w_target, w_loss = GM[f"{tag}/logits{it}"], GM[f"{tag}/target{it}"], float(GM[f"{tag}/loss{it}"])
        mask = w_target.astype(bool) if labelled else np.arange(gen.K + 1)[None, :] == np.zeros((gen.B, 1), int)
        lo, hi = acc_bounds(w_logits.astype(np.float64), mask, (1, 5), mgate("logits"))
        m.zero_grad(set_to_none=True)
        with torch.set_grad_enabled(train):
            if path == "forward":
                logits, target = m(blk, lab) if labelled else m(blk)
                assert np.abs(logits.detach().cpu().numpy() - w_logits).max() <= mgate("logits")
                assert np.array_equal(target.cpu().numpy(), w_target)
                loss = masked_loss(logits, target) if labelled else F.cross_entropy(logits, target)
                accs = (calc_mask_accuracy if labelled else calc_topk_accuracy)(logits.detach(), target, (1, 5))
            else:
                # step 3 of the labelled golden has no -1 label, so contrast()'s positives are the reference's
                loss, accs = m.contrast(blk, lab, (1, 5))
        accs = [float(a) for a in accs]
        print(tag, path, it, "loss", loss.item(), w_loss, "acc", accs, GM[f"{tag}/acc{it}"].tolist(), "bounds", lo, hi)
        assert abs(loss.item() - w_loss) <= mgate("loss") * abs(w_loss)
        assert all(l <= a <= h for l, a, h in zip(lo, accs, hi))
        if lo == hi:
            assert accs == GM[f"{tag}/acc{it}"].tolist()
        if train:
            loss.backward()
            check_grads(m, tag, it)
        assert int(m.queue_ptr) == int(GM[f"{tag}/ptr{it}"])
        assert np.abs(m.queue.cpu().numpy() - GM[f"{tag}/queue{it}"]).max() <= mgate("queue")
        if labelled:
            assert np.array_equal(m.queue_label.cpu().numpy(), GM[f"{tag}/queue_label{it}"])
    for n, v in m.state_dict().items():
        if n.startswith("encoder_k."):
            want = GM[f"{tag}/final/{n}"]
            got = gen.strided(v.cpu().numpy())
            if want.dtype.kind == "f":
                assert np.abs(got - want).max() <= mgate("key") * max(np.abs(want).max(), 1e-30), n
            else:
                assert np.array_equal(got, want), n


def test_contrast_agrees_with_forward_and_gradient_is_that_of_the_queue_as_scored(gpu):
    a, blocks = golden_model("uber")
    b, _ = golden_model("uber")
    first = None
    for it in range(3):
        blk, lab = dev(blocks[it]), dev(gen.LABELS[it])
        logits, target = a(blk, lab)
        la = masked_loss(logits, target)
        lb, _ = b.contrast(blk, lab)
        assert abs(la.item() - lb.item()) <= mgate("loss") * abs(la.item())
        assert torch.equal(a.queue, b.queue) and torch.equal(a.queue_label, b.queue_label) and torch.equal(a.queue_ptr, b.queue_ptr)
        if it == 0:
            first = (la, lb)
    # two steps later the queue has been overwritten; the first step's gradient is still that of the queue it scored
    for m, loss in zip((a, b), first):
        m.zero_grad(set_to_none=True)
        loss.backward()
        for n in ("2.weight", "2.bias", "4.weight", "4.bias"):
            want = GM[f"uber/grad0/{n}"]
            got = gen.strided(dict(m.encoder_q.named_parameters())[n].grad.cpu().numpy())
            assert np.abs(got - want).max() <= mgate("grad") * np.abs(want).max(), n

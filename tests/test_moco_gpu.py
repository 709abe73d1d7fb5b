"""GPU: loss.NCE_loss.MemoryMoCo / NCEAverage_intra_neg on the device (csrc/moco.hip) against the reference's goldens
(tests/golden/moco.npz) and against the float64 NumPy provider (tests/moco_cpu_kernels.py).

Tolerance.  The scale is the reference's own error: the generator ran the reference (fp32 torch) and the float64 provider on the golden
inputs and stored the deviation — logits 2.2e-6 max abs, exp outputs 2.2e-6 max rel, loss 8.1e-8 rel, dq 6.4e-7 (softmax mode) /
1.6e-6 (exp mode) of max |dq|.  The gate is 4 x that deviation (the summation order differs across k-tiles and K-slices), with
D 2^-24 / T as the floor for logits of unit-norm rows.  At the other shapes of this file (D up to 512, K up to 16384) the error of
any fp32 evaluation grows with D and K, so there the same fp32 torch op sequence is run on the CPU on the test's own inputs and the
gate is 4 x the larger of its deviation from float64 and the stored one.  Enqueue is a copy: written rows and `index` are compared
for equality."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
import moco_cpu_kernels as ref64

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(ROOT, "tests", "golden", "moco.npz"))
T, NDATA = 0.07, 1000


def gate(name, D=0, measured=0.0):
    d = max(float(G["dev_" + name]), measured)
    return 4.0 * (d if d > 0 else D * 2.0 ** -24 / T)


def unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def module(K, D, memory, soft=True, labels=None):
    from video_similarity_search_amd.loss.NCE_loss import MemoryMoCo
    m = MemoryMoCo(D, NDATA, K, T, use_softmax=soft, labels=labels is not None).cuda()
    m.memory.copy_(dev(memory))
    if labels is not None:
        m.queue_label.copy_(dev(labels))
    return m


def torch32(q, k, mem, k_label=None, queue_label=None):
    """the reference's op sequence (NCE_loss.py:211-221 + NCESoftmaxLoss, or the multi-positive loss) in fp32 on the CPU"""
    B = q.shape[0]
    qt, kt, mt = torch.from_numpy(q).requires_grad_(True), torch.from_numpy(k), torch.from_numpy(mem)
    l_pos = torch.bmm(qt.view(B, 1, -1), kt.view(B, -1, 1)).view(B, 1)
    out = torch.div(torch.cat((l_pos, torch.mm(mt, qt.transpose(1, 0)).transpose(0, 1)), dim=1), T)
    if k_label is None:
        loss = F.cross_entropy(out, torch.zeros(B, dtype=torch.long))
    else:
        mask = torch.from_numpy(k_label).unsqueeze(1) == torch.from_numpy(queue_label).unsqueeze(0)
        mask = torch.cat([torch.ones((B, 1), dtype=torch.bool), mask], dim=1)
        loss = (-(F.log_softmax(out, dim=1) * mask).sum(1) / mask.sum(1)).mean()
    loss.backward()
    return out.detach().numpy(), loss.item(), qt.grad.numpy()


def gates_at(q, k, mem, k_label=None, queue_label=None):
    """(float64 logits, loss, dq) and the gates (logits abs, loss rel, dq of max) for these inputs"""
    q64, k64, m64 = (a.astype(np.float64) for a in (q, k, mem))
    x64 = ref64.logits(q64, k64, m64, T)
    l64, dq64, _ = ref64.ce(q64, k64, m64, T, k_label, queue_label)
    x32, l32, dq32 = torch32(q, k, mem, k_label, queue_label)
    g = (gate("logits", q.shape[1], np.abs(x32 - x64).max()), gate("loss", 0, abs(l32 - l64) / abs(l64)),
         gate("dq", 0, np.abs(dq32 - dq64).max() / np.abs(dq64).max()))
    return (x64, l64, dq64), g


@pytest.mark.parametrize("case", ["c0", "c1"])
@pytest.mark.parametrize("soft", [True, False])
def test_goldens_on_device(case, soft):
    from video_similarity_search_amd.loss.NCE_loss import NCESoftmaxLoss
    K, D, B = (int(v) for v in G[case + "_shape"])
    m = module(K, D, G[case + "_memory0"], soft)
    tag = case + ("_soft" if soft else "_exp")
    expect = G[case + "_memory0"].copy()
    index = 0
    for it in range(3):
        q = dev(G[f"{case}_q{it}"]).requires_grad_(True)
        out = m(q, dev(G[f"{case}_k{it}"]))
        loss = NCESoftmaxLoss()(out)
        loss.backward()
        want = G[f"{tag}_out{it}"]
        err = np.abs(out.detach().cpu().numpy() - want)
        wl, dq = float(G[f"{tag}_loss{it}"]), G[f"{tag}_dq{it}"]
        dq_err = np.abs(q.grad.cpu().numpy() - dq).max() / np.abs(dq).max()
        print(tag, it, "out", err.max() if soft else (err / want).max(), "loss", abs(loss.item() - wl) / wl, "dq", dq_err)
        assert tuple(out.shape) == (B, K + 1)
        if soft:
            assert err.max() <= gate("logits", D)
        else:
            assert (err / want).max() <= gate("exp")
        assert abs(loss.item() - wl) <= gate("loss") * wl
        assert dq_err <= gate("dq" if soft else "dq_exp")
        expect[(index + np.arange(B)) % K] = G[f"{case}_k{it}"]
        index = (index + B) % K
        assert m.index == int(G[f"{case}_index{it}"])
        assert np.array_equal(m.memory.cpu().numpy(), expect)                     # bit-equal: enqueue is a copy
        if f"{case}_memory_after{it}" in G:
            assert np.array_equal(expect, G[f"{case}_memory_after{it}"])
    if not soft:
        assert m.params.tolist() == G[case + "_Z"].tolist()


# each of B in {1, 26, 130}, D in {100, 128, 512}, K in {1000, 2048, 16384} at least once, (130, 512, 16384) once; 101 / 3: rows the
# LDS DMA cannot address (the 32-query engine's forward); 200: the 8-k-tile instantiation
SHAPES = [(1, 100, 1000), (26, 128, 2048), (130, 512, 16384), (26, 101, 1000), (5, 3, 130), (40, 200, 1000), (130, 128, 16384)]


@pytest.mark.parametrize("B,D,K", SHAPES)
def test_against_float64_fused_and_unfused(B, D, K):
    from video_similarity_search_amd.loss.NCE_loss import NCESoftmaxLoss
    rng = np.random.default_rng(B * 1000 + D)
    q, k, mem = unit(rng, B, D), unit(rng, B, D), unit(rng, K, D)
    (x64, l64, dq64), (g_x, g_l, g_dq) = gates_at(q, k, mem)
    ma, mb = module(K, D, mem), module(K, D, mem)
    ma.index = mb.index = K - B // 2 if B > 1 else K - 1            # the enqueue wraps (B > 1: in the middle of the batch)
    qa, qb = dev(q).requires_grad_(True), dev(q).requires_grad_(True)
    out = ma(qa, dev(k))
    la = NCESoftmaxLoss()(out)
    la.backward()
    lb = mb.softmax_loss(qb, dev(k))
    lb.backward()
    e_x = np.abs(out.detach().cpu().numpy() - x64).max()
    e_dqa = np.abs(qa.grad.cpu().numpy() - dq64).max() / np.abs(dq64).max()
    e_dqb = np.abs(qb.grad.cpu().numpy() - dq64).max() / np.abs(dq64).max()
    print((B, D, K), "logits", e_x, "/", g_x, "loss", abs(la.item() - l64) / l64, abs(lb.item() - l64) / l64, "/", g_l,
          "dq", e_dqa, e_dqb, "/", g_dq)
    assert e_x <= g_x
    assert abs(la.item() - l64) <= g_l * l64 and abs(lb.item() - l64) <= g_l * l64
    assert e_dqa <= g_dq and e_dqb <= g_dq
    # fused and unfused leave the same queue
    assert ma.index == mb.index == (K - (B // 2 if B > 1 else 1) + B) % K
    assert torch.equal(ma.memory, mb.memory)
    expect = mem.copy()
    expect[((K - (B // 2 if B > 1 else 1)) + np.arange(B)) % K] = k
    assert np.array_equal(ma.memory.cpu().numpy(), expect)


@pytest.mark.parametrize("fused", [True, False])
def test_gradient_is_that_of_the_queue_as_scored(fused):
    from video_similarity_search_amd.loss.NCE_loss import NCESoftmaxLoss
    rng = np.random.default_rng(7)
    K, D, B = 256, 64, 128
    mem = unit(rng, K, D)
    q1, k1, q2, k2, k3 = (unit(rng, B, D) for _ in range(5))
    (_, l64, dq64), (_, g_l, g_dq) = gates_at(q1, k1, mem)
    m = module(K, D, mem)
    step = (lambda q, k: m.softmax_loss(q, k)) if fused else (lambda q, k: NCESoftmaxLoss()(m(q, k)))
    qa = dev(q1).requires_grad_(True)
    loss1 = step(qa, dev(k1))                      # scores rows 0 .. 255, overwrites 0 .. 127
    step(dev(q2).requires_grad_(True), dev(k2))    # overwrites 128 .. 255
    step(dev(q2), dev(k3))                         # and 0 .. 127 again
    loss1.backward()
    assert abs(loss1.item() - l64) <= g_l * l64
    assert np.abs(qa.grad.cpu().numpy() - dq64).max() <= g_dq * np.abs(dq64).max()


def test_multi_positive():
    rng = np.random.default_rng(11)
    # the golden (1, 2 and 25 positives, -1 slots), then 130 x 64 x 2048 with > 100 positives per row of label 0, then an all -1 queue
    cases = [(G["mp_q"], G["mp_k"], G["mp_memory"], G["mp_k_label"], G["mp_queue_label"])]
    K, D, B = 2048, 64, 130
    ql = rng.integers(1, 40, K).astype(np.int64)
    ql[rng.choice(K, 300, replace=False)] = -1
    ql[rng.choice(K, 150, replace=False)] = 0
    ql[ql == 5] = 6
    ql[77] = 5
    kl = rng.integers(0, 45, B).astype(np.int64)                      # labels 40 .. 44: not in the queue
    kl[:3] = (0, 5, 44)
    cases.append((unit(rng, B, D), unit(rng, B, D), unit(rng, K, D), kl, ql))
    cases.append((unit(rng, 26, D), unit(rng, 26, D), unit(rng, 1000, D), kl[:26].copy(), np.full(1000, -1, np.int64)))
    for q, k, mem, kl, ql in cases:
        B, (K, D) = q.shape[0], mem.shape
        (_, l64, dq64), (_, g_l, g_dq) = gates_at(q, k, mem, kl, ql)
        npos = 1 + ((kl[:, None] == ql[None, :]) & (ql[None, :] >= 0)).sum(1)
        m = module(K, D, mem, labels=ql)
        qa = dev(q).requires_grad_(True)
        loss = m.softmax_loss(qa, dev(k), dev(kl))
        loss.backward()
        e_dq = np.abs(qa.grad.cpu().numpy() - dq64).max() / np.abs(dq64).max()
        print((B, D, K), "npos", npos.min(), npos.max(), "loss", abs(loss.item() - l64) / l64, "/", g_l, "dq", e_dq, "/", g_dq)
        assert abs(loss.item() - l64) <= g_l * l64 and e_dq <= g_dq
        want = ql.copy()
        want[:B] = kl
        assert np.array_equal(m.queue_label.cpu().numpy(), want) and m.index == B % K
    assert npos.max() == 1                                             # the last case: the first training step
    assert float(G["mp_npos"].max()) == 25 and (cases[1][3][0], cases[1][3][1]) == (0, 5)


def test_extreme_logits():
    from video_similarity_search_amd.loss.NCE_loss import NCESoftmaxLoss
    rng = np.random.default_rng(13)
    K, D, B = 1000, 128, 26
    mem = unit(rng, K, D)
    q, k = unit(rng, B, D), unit(rng, B, D)
    q[0] = k[0] = mem[400]                        # logit 1 / 0.07 = 14.3 at columns 0 and 401
    q[1] = 50.0 * mem[999]                        # logits up to 714: exp overflows fp32 without the running maximum
    q[2] = -50.0 * mem[0]
    (x64, l64, dq64), (g_x, g_l, g_dq) = gates_at(q, k, mem)
    assert abs(x64[0, 0] - 1 / T) < 1e-4 and x64[1].max() > 700
    ma, mb = module(K, D, mem), module(K, D, mem)
    qa, qb = dev(q).requires_grad_(True), dev(q).requires_grad_(True)
    out = ma(qa, dev(k))
    la = NCESoftmaxLoss()(out)
    la.backward()
    lb = mb.softmax_loss(qb, dev(k))
    lb.backward()
    for t in (out, la, lb, qa.grad, qb.grad):
        assert torch.isfinite(t).all()
    # logits of the scaled rows carry the scale in their error: relative to the row's largest logit
    scale = np.maximum(1.0, np.abs(x64).max(1, keepdims=True) * T)
    assert (np.abs(out.detach().cpu().numpy() - x64) / scale).max() <= g_x
    assert abs(la.item() - l64) <= g_l * l64 and abs(lb.item() - l64) <= g_l * l64
    for g in (qa.grad, qb.grad):
        assert np.abs(g.cpu().numpy() - dq64).max() <= g_dq * np.abs(dq64).max()


def test_two_runs_are_bit_equal():
    from video_similarity_search_amd.loss.NCE_loss import NCESoftmaxLoss
    rng = np.random.default_rng(17)
    K, D, B = 16384, 128, 130
    q, k, mem = unit(rng, B, D), unit(rng, B, D), unit(rng, K, D)
    runs = []
    for _ in range(2):
        ma, mb = module(K, D, mem), module(K, D, mem)
        qa, qb = dev(q).requires_grad_(True), dev(q).requires_grad_(True)
        out = ma(qa, dev(k))
        la = NCESoftmaxLoss()(out)
        la.backward()
        lb = mb.softmax_loss(qb, dev(k))
        lb.backward()
        runs.append([t.detach().clone() for t in (out, la, qa.grad, lb, qb.grad)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_input_forms():
    from video_similarity_search_amd.loss.NCE_loss import NCESoftmaxLoss
    rng = np.random.default_rng(19)
    K, D, B = 1000, 100, 26
    q, k, mem = unit(rng, B, D), unit(rng, B, D), unit(rng, K, D)
    m0 = module(K, D, mem)
    q0 = dev(q).requires_grad_(True)
    l0 = m0.softmax_loss(q0, dev(k))
    l0.backward(retain_graph=True)
    g1 = q0.grad.clone()
    q0.grad = None
    l0.backward()                                                  # retain_graph: the second backward gives the same gradient
    assert torch.equal(q0.grad, g1)
    # a column slice of a wider tensor; k that requires grad gets None
    wide = torch.zeros(B, D + 28, device="cuda")
    wide[:, 7:7 + D] = dev(q)
    wide.requires_grad_(True)
    kk = dev(k).requires_grad_(True)
    for fused in (True, False):
        m = module(K, D, mem)
        qs = wide[:, 7:7 + D]
        assert not qs.is_contiguous()
        loss = m.softmax_loss(qs, kk) if fused else NCESoftmaxLoss()(m(qs, kk))
        loss.backward()
        assert kk.grad is None
        assert torch.equal(loss, l0) if fused else abs(loss.item() - l0.item()) <= gate("loss") * l0.item()
        if fused:
            assert torch.equal(wide.grad[:, 7:7 + D], g1) and wide.grad[:, :7].abs().max().item() == 0
        wide.grad = None
    # no_grad keeps nothing
    m = module(K, D, mem)
    with torch.no_grad():
        loss = m.softmax_loss(dev(q).requires_grad_(True), dev(k))
        out = m(dev(q).requires_grad_(True), dev(k))
    assert loss.grad_fn is None and out.grad_fn is None and not loss.requires_grad and m.index == 2 * B
    assert torch.equal(loss, l0)
    from video_similarity_search_amd import _lib
    with pytest.raises(_lib.SlicError):
        m(torch.from_numpy(q), torch.from_numpy(k))
    with pytest.raises(ValueError):
        module(8, D, mem[:8])(dev(q), dev(k))


@pytest.mark.parametrize("soft", [True, False])
def test_intra_neg_goldens_on_device(soft):
    from video_similarity_search_amd.loss.NCE_loss import NCEAverage_intra_neg, NCECriterion, NCESoftmaxLoss
    B, D = G["in_l0"].shape
    K, ndata = G["in_idx0"].shape[1] - 1, G["in_memory_l0"].shape[0]
    tag = "in_soft" if soft else "in_exp"
    nce = NCEAverage_intra_neg(D, ndata, K, T, 0.5, use_softmax=soft).cuda()
    assert list(nce.state_dict().keys()) == ["params", "memory_l", "memory_ab", "memory_neg"]
    for n in ("memory_l", "memory_ab", "memory_neg"):
        getattr(nce, n).copy_(dev(G[f"in_{n}0"]))
    crit = NCESoftmaxLoss() if soft else NCECriterion(ndata)
    for it in range(2):
        l, ab = dev(G[f"in_l{it}"]).requires_grad_(True), dev(G[f"in_ab{it}"]).requires_grad_(True)
        o_l, o_ab = nce(l, ab, dev(G[f"in_neg{it}"]), dev(G[f"in_y{it}"]), dev(G[f"in_idx{it}"]))
        tot = crit(o_l) + crit(o_ab)
        tot.backward()
        assert tuple(o_l.shape) == tuple(o_ab.shape) == (B, 2 * (K + 1), 1)
        for got, name in ((o_l, "out_l"), (o_ab, "out_ab")):
            want = G[f"{tag}_{name}{it}"]
            err = np.abs(got.detach().cpu().numpy() - want)
            assert err.max() <= gate("logits", D) if soft else (err / want).max() <= gate("exp")
        wl = float(G[f"{tag}_loss{it}"])
        assert abs(tot.item() - wl) <= gate("loss") * abs(wl) * (1 if soft else 8)       # NCECriterion sums B (2K + 2) logs: not a mean
        for got, name in ((l.grad, "grad_l"), (ab.grad, "grad_ab")):
            want = G[f"{tag}_{name}{it}"]
            assert np.abs(got.cpu().numpy() - want).max() <= gate("dq" if soft else "dq_exp") * np.abs(want).max()
    for n in ("memory_l", "memory_ab", "memory_neg"):
        assert np.abs(getattr(nce, n).cpu().numpy() - G[f"{tag}_{n}2"]).max() <= 4 * 2.0 ** -23          # unit rows, a few ulp
    assert np.allclose(nce.params.cpu().numpy(), G[f"{tag}_params"], rtol=gate("exp"), atol=0)
    # idx=None: column 0 of the drawn idx is y -> the positive's score sits in column 0 and column K + 1
    y = dev(G["in_y0"])
    l = dev(G["in_l0"])
    bank_ab, bank_neg = nce.memory_ab.clone(), nce.memory_neg.clone()
    o_l, o_ab = nce(l, dev(G["in_ab0"]), dev(G["in_neg0"]), y)
    assert tuple(o_l.shape) == (B, 2 * (K + 1), 1)
    Zl = 1.0 if soft else float(nce.params[2].item())
    want0 = (bank_ab[y] * l).sum(1) / T
    want1 = (bank_neg[y] * l).sum(1) / T
    got0, got1 = o_l[:, 0, 0], o_l[:, K + 1, 0]
    if not soft:
        got0, got1 = torch.log(got0 * Zl), torch.log(got1 * Zl)
    assert (got0 - want0).abs().max().item() <= 1e-4 and (got1 - want1).abs().max().item() <= 1e-4

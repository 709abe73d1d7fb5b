"""CPU: the host logic of loss.NCE_loss.MemoryMoCo against the reference's goldens (tests/golden/moco.npz), driven through the
float64 NumPy provider (tests/moco_cpu_kernels.py) — queue index and wrap, Z, prints, state_dict, argument errors — and the
no-device behaviour of the product path.

Tolerances: the golden is the reference's fp32 output; the generator measured its deviation from the float64 provider on the golden
inputs (stored as dev_*: logits 2.2e-6 abs, exp outputs 2.2e-6 rel, loss 8.1e-8 rel, dq 6.4e-7 / 1.6e-6 of max |dq|).  The gate is
4 x that deviation, with D 2^-24 / T as the floor for logits."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from moco_cpu_kernels import NumpyMoCoKernels
import moco_cpu_kernels as ref64

G = np.load(os.path.join(ROOT, "tests", "golden", "moco.npz"))
T, NDATA = 0.07, 1000


def gate(name, D=0):
    d = float(G["dev_" + name])
    return 4.0 * (d if d > 0 else D * 2.0 ** -24 / T)


def _module(case, soft, **kw):
    from video_similarity_search_amd.loss.NCE_loss import MemoryMoCo
    K, D, B = (int(v) for v in G[case + "_shape"])
    m = MemoryMoCo(D, NDATA, K, T, use_softmax=soft, kernels=NumpyMoCoKernels(), **kw).double()
    m.memory.copy_(torch.from_numpy(G[case + "_memory0"]))
    return m, K, D, B


@pytest.mark.parametrize("case", ["c0", "c1"])
@pytest.mark.parametrize("soft", [True, False])
def test_driver_reproduces_goldens(case, soft, capsys):
    from video_similarity_search_amd.loss.NCE_loss import NCESoftmaxLoss
    m, K, D, B = _module(case, soft)
    assert "using queue shape: ({},{})".format(K, D) in capsys.readouterr().out
    tag = case + ("_soft" if soft else "_exp")
    expect = np.array(G[case + "_memory0"], np.float64)
    index = 0
    for it in range(3):
        q = torch.from_numpy(G[f"{case}_q{it}"]).double().requires_grad_(True)
        k = torch.from_numpy(G[f"{case}_k{it}"]).double().requires_grad_(True)
        out = m(q, k)
        assert tuple(out.shape) == (B, K + 1)
        x = torch.nn.functional.cross_entropy(out, torch.zeros(B, dtype=torch.long))       # NCESoftmaxLoss, on the CPU
        x.backward()
        assert k.grad is None
        want = G[f"{tag}_out{it}"]
        if soft:
            assert np.abs(out.detach().numpy() - want).max() <= gate("logits", D)
        else:
            assert (np.abs(out.detach().numpy() - want) / want).max() <= gate("exp")
        assert abs(x.item() - float(G[f"{tag}_loss{it}"])) <= gate("loss") * abs(float(G[f"{tag}_loss{it}"]))
        dq = G[f"{tag}_dq{it}"]
        assert np.abs(q.grad.numpy() - dq).max() <= gate("dq" if soft else "dq_exp") * np.abs(dq).max()
        ids = (index + np.arange(B)) % K
        expect[ids] = G[f"{case}_k{it}"]
        index = (index + B) % K
        assert m.index == int(G[f"{case}_index{it}"]) == index
        assert np.array_equal(m.memory.numpy(), expect)
        if f"{case}_memory_after{it}" in G:
            assert np.array_equal(m.memory.numpy().astype(np.float32), G[f"{case}_memory_after{it}"])
    printed = capsys.readouterr().out
    if soft:
        assert "normalization constant" not in printed and m.params.tolist() == [-1]
    else:
        assert m.params.tolist() == G[case + "_Z"].tolist()
        assert printed.count("normalization constant Z is set to {:.1f}".format(int(G[case + "_Z"][0]))) == 1


def test_golden_wraps_in_the_middle_of_a_batch():
    K, D, B = (int(v) for v in G["c1_shape"])
    before, after = int(G["c1_index1"]), int(G["c1_index2"])
    assert before + B > K and 0 < after < B and after == (before + B) % K


def test_state_dict_keys_and_attributes(capsys):
    from video_similarity_search_amd.loss.NCE_loss import MemoryMoCo
    m = MemoryMoCo(16, 1000, 64, kernels=NumpyMoCoKernels())
    assert list(m.state_dict().keys()) == ["params", "memory"]
    assert (m.outputSize, m.inputSize, m.queueSize, m.T, m.index, m.use_softmax) == (1000, 16, 64, 0.07, 0, False)
    assert m.params.dtype == torch.int64 and m.params.tolist() == [-1]
    stdv = 1.0 / np.sqrt(16 / 3)
    assert tuple(m.memory.shape) == (64, 16) and m.memory.abs().max().item() <= stdv and m.memory.std().item() > 0.4 * stdv
    ml = MemoryMoCo(16, 1000, 64, labels=True, kernels=NumpyMoCoKernels())
    assert list(ml.state_dict().keys()) == ["params", "memory", "queue_label"]
    assert ml.queue_label.dtype == torch.int64 and ml.queue_label.tolist() == [-1] * 64
    assert capsys.readouterr().out.count("using queue shape: (64,16)") == 2


def test_argument_errors():
    from video_similarity_search_amd.loss.NCE_loss import MemoryMoCo
    m = MemoryMoCo(16, 1000, 8, use_softmax=True, kernels=NumpyMoCoKernels()).double()
    q = torch.randn(9, 16).double()
    with pytest.raises(ValueError):
        m(q, q)
    with pytest.raises(ValueError):
        m.softmax_loss(q, q)
    with pytest.raises(ValueError):
        m.softmax_loss(q[:4], q[:4], k_label=torch.zeros(4, dtype=torch.long))          # built without labels=True
    with pytest.raises(ValueError):
        m(q[:4, :8], q[:4, :8])
    assert m.index == 0
    with pytest.raises(NotImplementedError):
        MemoryMoCo(16, 1000, 8, use_softmax=False, kernels=NumpyMoCoKernels()).softmax_loss(q[:4], q[:4])


def test_fused_step_equals_forward_plus_loss():
    """softmax_loss == cross-entropy of forward()'s logits with the same queue update; a second forward before the first backward
    leaves the first gradient that of the queue as scored"""
    ma, K, D, B = _module("c1", True)
    mb, _, _, _ = _module("c1", True)
    qs = [torch.from_numpy(G[f"c1_q{it}"]).double().requires_grad_(True) for it in range(3)]
    losses = [ma.softmax_loss(qs[it], torch.from_numpy(G[f"c1_k{it}"]).double()) for it in range(3)]      # all forwards first
    for it in range(3):
        losses[it].backward()
        assert abs(losses[it].item() - float(G[f"c1_soft_loss{it}"])) <= gate("loss") * abs(float(G[f"c1_soft_loss{it}"]))
        dq = G[f"c1_soft_dq{it}"]
        assert np.abs(qs[it].grad.numpy() - dq).max() <= gate("dq") * np.abs(dq).max()
        mb(torch.from_numpy(G[f"c1_q{it}"]).double(), torch.from_numpy(G[f"c1_k{it}"]).double())
    assert ma.index == mb.index == int(G["c1_index2"]) and torch.equal(ma.memory, mb.memory)
    with torch.no_grad():
        assert ma.softmax_loss(qs[0], qs[1]).grad_fn is None


def test_multi_positive_golden():
    from video_similarity_search_amd.loss.NCE_loss import MemoryMoCo
    K, D = G["mp_memory"].shape
    m = MemoryMoCo(D, NDATA, K, T, use_softmax=True, labels=True, kernels=NumpyMoCoKernels()).double()
    m.memory.copy_(torch.from_numpy(G["mp_memory"]))
    m.queue_label.copy_(torch.from_numpy(G["mp_queue_label"]))
    q = torch.from_numpy(G["mp_q"]).double().requires_grad_(True)
    k_label = torch.from_numpy(G["mp_k_label"])
    loss = m.softmax_loss(q, torch.from_numpy(G["mp_k"]).double(), k_label)
    loss.backward()
    assert abs(loss.item() - float(G["mp_loss"])) <= 1e-12 * float(G["mp_loss"])
    assert np.abs(q.grad.numpy() - G["mp_dq"]).max() <= 1e-12 * np.abs(G["mp_dq"]).max()
    B = q.shape[0]
    assert m.index == B and m.queue_label[:B].tolist() == k_label.tolist()
    assert np.array_equal(m.queue_label[B:].numpy(), G["mp_queue_label"][B:])


def test_goldens_cover_the_label_rules():
    ql, kl, npos = G["mp_queue_label"], G["mp_k_label"], G["mp_npos"]
    assert (ql == -1).sum() > 0 and kl.min() >= 0                       # empty slots exist, and no row's label can match one
    assert np.array_equal(npos, 1 + (kl[:, None] == ql[None, :]).sum(1))
    assert 1 in npos and 2 in npos and npos.max() >= 20
    # a row with n_pos == 1 carries the plain cross-entropy against column 0
    q, k, mem = (G[n].astype(np.float64) for n in ("mp_q", "mp_k", "mp_memory"))
    x = ref64.logits(q, k, mem, T)
    plain = np.log(np.exp(x - x.max(1, keepdims=True)).sum(1)) + x.max(1) - x[:, 0]
    rows = np.flatnonzero(npos == 1)
    assert len(rows) >= 1 and np.abs(G["mp_rowloss"][rows] - plain[rows]).max() <= 1e-12 * plain[rows].max()


def test_no_device_raises():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.loss.NCE_loss import MemoryMoCo, NCEAverage_intra_neg
    m = MemoryMoCo(16, 1000, 64, use_softmax=True)
    q = torch.randn(4, 16)
    with pytest.raises(_lib.SlicError):
        m(q, q)
    with pytest.raises(_lib.SlicError):
        m.softmax_loss(q, q)
    assert m.index == 0
    with pytest.raises(_lib.SlicError):
        NCEAverage_intra_neg(16, 50, 8)(q, q, q, torch.arange(4))

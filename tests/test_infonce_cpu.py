"""CPU: the host logic of models/infoNCE.py (InfoNCE, UberNCE), online_train.UberNCE_train_epoch / calc_mask_accuracy and
model_utils.model_selector, driven with the float64 NumPy provider (tests/infonce_cpu_kernels.py).  Against the reference's goldens
(tests/golden/infonce.npz): state-dict keys and shapes, and the golden steps of forward / contrast with the golden weights, the
trunk run by oracle.encoder.encoder_forward (the CPU restatement of the 3D ResNet).  Against a float64 torch restatement of the step
written here, on a small torch trunk: steps with a weight update between them (the EMA moves), the epoch, the error paths."""
import contextlib
import io
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import GOLDEN
from infonce_cpu_kernels import NumpyInfoNCEKernels, hits_of, rank_of_best
sys.path.insert(0, GOLDEN)
import make_goldens_infonce as gen                              # noqa: E402  (draw_case, the golden shapes)

G = np.load(os.path.join(GOLDEN, "infonce.npz"))
ns = types.SimpleNamespace
CLIP = (3, 2, 6, 6)
FEAT, DIM, K, B, T, M = 8, 12, 16, 4, 0.07, 0.9


class TinyTrunk(nn.Module):
    feature_size = FEAT

    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(int(np.prod(CLIP)), FEAT)

    def forward(self, x):
        return torch.tanh(self.lin(x.reshape(x.shape[0], -1).to(self.lin.weight.dtype)))


def make(cls_name, K_=K, seed=0):
    from video_similarity_search_amd.models import infoNCE
    torch.manual_seed(seed)
    return getattr(infoNCE, cls_name)(TinyTrunk, DIM, K_, M, T, kernels=NumpyInfoNCEKernels()).double()


def blocks(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((B, 2) + CLIP, generator=g).double() for _ in range(n)]


LABELS = [torch.tensor(v) for v in ([0, 1, 2, 0], [1, 1, 0, 3], [2, 0, 0, 1], [0, 2, 1, -1])]


class Restated:
    """the step in float64 torch, from the behaviour: EMA, two encoders, logits against the queue, loss, enqueue"""

    def __init__(self, model, labelled, empty_slots_match=True):
        self.empty_slots_match = empty_slots_match              # forward(): the reference's plain ==; contrast(): -1 is never a positive
        sd = {k: v.detach().clone().double() for k, v in model.state_dict().items()}
        self.q = {k[len("encoder_q."):]: v.requires_grad_(True) for k, v in sd.items() if k.startswith("encoder_q.")}
        self.k = {k[len("encoder_k."):]: v for k, v in sd.items() if k.startswith("encoder_k.")}
        self.queue, self.ptr = sd["queue"].clone(), 0
        self.qlabel = sd["queue_label"].clone().long() if labelled else None

    @staticmethod
    def encode(p, x):
        f = torch.tanh(x.reshape(x.shape[0], -1).double() @ p["0.lin.weight"].t() + p["0.lin.bias"])
        h = torch.relu(f @ p["2.weight"].reshape(FEAT, FEAT).t() + p["2.bias"])
        return F.normalize(h @ p["4.weight"].reshape(DIM, FEAT).t() + p["4.bias"], dim=1)

    def step(self, block, label, train=True):
        for v in self.q.values():
            v.grad = None
        q = self.encode(self.q, block[:, 0])
        with torch.no_grad():
            if train:
                for n in self.k:
                    self.k[n] = self.k[n] * M + self.q[n].detach() * (1. - M)
            k = self.encode(self.k, block[:, 1])
        logits = torch.cat([(q * k).sum(1, keepdim=True), q @ self.queue], 1) / T
        if self.qlabel is None:
            mask = torch.zeros(B, logits.shape[1], dtype=torch.bool)
            mask[:, 0] = True
        else:
            same = label[:, None] == self.qlabel[None, :]
            if not self.empty_slots_match:
                same &= self.qlabel[None, :] >= 0
            mask = torch.cat([torch.ones(B, 1, dtype=torch.bool), same], 1)
        loss = (-(F.log_softmax(logits, 1) * mask).sum(1) / mask.sum(1)).mean()
        if train:
            loss.backward()
            self.queue[:, self.ptr:self.ptr + B] = k.t()
            if self.qlabel is not None:
                self.qlabel[self.ptr:self.ptr + B] = label
            self.ptr = (self.ptr + B) % self.queue.shape[1]
        return logits.detach(), mask, loss.detach()


def close(a, b, tol=1e-5):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("tag,cls", [("info", "InfoNCE"), ("uber", "UberNCE")])
def test_state_dict_is_the_references(tag, cls):
    from video_similarity_search_amd.models import generate_model, infoNCE
    with contextlib.redirect_stdout(io.StringIO()):
        m = getattr(infoNCE, cls)(lambda: generate_model(10, **gen.TRUNK_KW), gen.DIM, gen.K, gen.M, gen.T, kernels=NumpyInfoNCEKernels())
    sd = m.state_dict()
    assert sorted(sd) == G[tag + "/keys"].tolist()
    assert [",".join(map(str, sd[k].shape)) for k in sorted(sd)] == G[tag + "/shapes"].tolist()
    assert sd["queue_ptr"].dtype == torch.int64 and m.queue.t().is_contiguous() and m.param == {"feature_size": gen.FEAT}
    assert close(m.queue.norm(dim=0), torch.ones(gen.K)) and int(sd["queue_ptr"]) == 0
    assert all(not p.requires_grad for p in m.encoder_k.parameters()) and all(p.requires_grad for p in m.encoder_q.parameters())
    for pq, pk in zip(m.encoder_q.parameters(), m.encoder_k.parameters()):
        assert torch.equal(pq, pk)
    if tag == "uber":
        assert sd["queue_label"].dtype == torch.int64 and (sd["queue_label"] == -1).all()
    # a reference-shaped state dict loads, and the queue keeps its row storage
    ref_sd, blk = gen.draw_case(211 if tag == "info" else 223, tag == "uber")
    assert np.allclose(gen.checksum(ref_sd, blk), G[tag + "/check"], rtol=1e-12)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in ref_sd.items()})
    assert torch.equal(m.queue, torch.as_tensor(ref_sd["queue"])) and m._rows().is_contiguous()
    assert torch.equal(m.encoder_k[4].weight, torch.as_tensor(ref_sd["encoder_k.4.weight"]))


def test_networks():
    from video_similarity_search_amd.models.infoNCE import InfoNCE
    with pytest.raises(NotImplementedError, match="DESIGN"):
        InfoNCE('s3d')
    with pytest.raises(ValueError):
        InfoNCE('vgg')
    with contextlib.redirect_stdout(io.StringIO()):
        m = InfoNCE('resnet10', K=8)
    assert m.param == {"feature_size": 512} and tuple(m.encoder_q[2].weight.shape) == (512, 512, 1, 1, 1)
    assert tuple(m.encoder_k[4].weight.shape) == (128, 512, 1, 1, 1) and tuple(m.queue.shape) == (128, 8)
    from video_similarity_search_amd import _lib
    with pytest.raises(_lib.SlicError):
        m(torch.zeros(2, 2, 3, 4, 8, 8))                          # no device: no fallback


@pytest.mark.parametrize("cls", ["InfoNCE", "UberNCE"])
@pytest.mark.parametrize("path", ["forward", "contrast"])
def test_steps_against_the_restated_model(cls, path):
    labelled = cls == "UberNCE"
    m = make(cls)
    want = Restated(m, labelled, empty_slots_match=path == "forward")
    m.train()
    for it, blk in enumerate(blocks(4)):
        train = it < 3
        lab = LABELS[it] if labelled else None
        for p in m.parameters():
            p.grad = None
        w_logits, w_mask, w_loss = want.step(blk, lab, train)
        w_rank = rank_of_best(w_logits.numpy(), w_mask.numpy())
        with torch.set_grad_enabled(train):
            if path == "forward":
                logits, target = m(blk, lab) if labelled else m(blk)
                assert tuple(logits.shape) == (B, K + 1) and close(logits, w_logits)
                if labelled:
                    assert target.dtype == torch.bool and torch.equal(target, w_mask)
                    loss = (-(F.log_softmax(logits, 1) * target).sum(1) / target.sum(1)).mean()
                else:
                    assert target.dtype == torch.int64 and torch.equal(target, torch.zeros(B, dtype=torch.long))
                    loss = F.cross_entropy(logits, target)
            else:
                loss, accs = m.contrast(blk, lab, (1, 5))
                assert [float(a) for a in accs] == (hits_of(w_rank, (1, 5)) / B).tolist() and accs[0].dim() == 0
        assert close(loss, w_loss)
        assert loss.requires_grad == train
        if train:
            loss.backward()
            for n, p in m.encoder_q.named_parameters():
                assert close(p.grad, want.q[n].grad, 1e-4), n
            with torch.no_grad():                                # a plain SGD step on both sides: the EMA has something to move
                for n, p in m.encoder_q.named_parameters():
                    p -= 0.5 * p.grad
                    want.q[n].data -= 0.5 * want.q[n].grad
        assert int(m.queue_ptr) == want.ptr and close(m.queue, want.queue, 1e-6)
        for n, p in m.encoder_k.named_parameters():
            assert close(p, want.k[n], 1e-6), n
        if labelled:
            assert torch.equal(m.queue_label, want.qlabel)
    assert want.ptr == (3 * B) % K


def test_contrast_and_forward_leave_the_same_state():
    a, b = make("UberNCE", seed=3), make("UberNCE", seed=3)
    a.train(), b.train()
    for it, blk in enumerate(blocks(3, seed=9)):
        logits, mask = a(blk, LABELS[it])
        la = (-(F.log_softmax(logits, 1) * mask).sum(1) / mask.sum(1)).mean()
        lb, accs = b.contrast(blk, LABELS[it])
        assert close(la, lb, 1e-6) and all(0.0 <= float(x) <= 1.0 for x in accs)
        assert torch.equal(a.queue, b.queue) and torch.equal(a.queue_label, b.queue_label) and torch.equal(a.queue_ptr, b.queue_ptr)
    with pytest.raises(TypeError):
        a(blocks(1)[0])                                           # UberNCE.forward(block, k_label), as in the reference
    with pytest.raises(ValueError):
        a.contrast(blocks(1)[0])                                  # and contrast needs them too
    with pytest.raises(ValueError):
        make("InfoNCE")(blocks(1)[0], LABELS[0])
    with pytest.raises(ValueError):
        make("InfoNCE")(torch.zeros((B, 3) + CLIP))


def test_queue_size_must_be_a_multiple_of_the_batch():
    m = make("InfoNCE", K_=10).train()
    with pytest.raises(ValueError, match="multiple"):
        m(blocks(1)[0])
    with torch.no_grad():
        m(blocks(1)[0])                                           # no enqueue without a gradient: nothing to refuse


@pytest.mark.parametrize("world", [1, 2, 4])
def test_shuffle_index_functions(world):
    from video_similarity_search_amd.models.infoNCE import shuffle_rows_of_rank, unshuffle_rows_of_rank
    per = 3
    g = torch.Generator().manual_seed(world)
    perm = torch.randperm(world * per, generator=g)
    x = torch.arange(world * per) * 10                            # the gathered batch
    shuffled = torch.cat([x[shuffle_rows_of_rank(perm, world, r)] for r in range(world)])       # what the ranks encode, gathered
    assert torch.equal(shuffled, x[perm])
    for r in range(world):
        assert torch.equal(shuffled[unshuffle_rows_of_rank(perm, world, r)], x[r * per:(r + 1) * per])


def test_single_process_draws_the_permutation_and_does_not_apply_it():
    m = make("InfoNCE")
    x = torch.arange(12.).view(4, 3)
    torch.manual_seed(77)
    y, idx = m._batch_shuffle_ddp(x)
    after = torch.rand(1)
    torch.manual_seed(77)
    torch.randperm(4)
    assert torch.equal(after, torch.rand(1)) and idx is None and y is x and m._batch_unshuffle_ddp(y, idx) is y


class Loader(list):
    def __init__(self, items, n):
        super().__init__(items)
        self.dataset = range(n)


def epoch_cfg(arch, out):
    return ns(MODEL=ns(ARCH=arch), DATA=ns(SAMPLE_DURATION=CLIP[1]), LOSS=ns(FEAT_DIM=CLIP[2]), NUM_GPUS=1, TRAIN=ns(LOG_INTERVAL=2),
              OUTPUT_PATH=out)


def loader(n_steps):
    items = []
    for it, blk in enumerate(blocks(n_steps, seed=21)):
        # the dataset's two views, [B, 3, T, S, S] each; concatenated on the channel axis and reshaped by the epoch
        six = blk.transpose(1, 2).reshape(B, 6, *CLIP[1:])
        items.append(([six[:, :3].numpy(), six[:, 3:].numpy()], [LABELS[it % 3], LABELS[it % 3]], torch.arange(B)))
    return Loader(items, n_steps * B)


@pytest.mark.parametrize("arch,cls", [("info_nce", "InfoNCE"), ("uber_nce", "UberNCE")])
def test_epoch_prints_logs_and_returns(arch, cls, tmp_path):
    from video_similarity_search_amd.online_train import UberNCE_train_epoch
    results = {}
    for fused in ((True, False) if arch == "uber_nce" else (True,)):      # unfused info_nce: calc_topk_accuracy is a device call
        m = make(cls, seed=5)
        opt = torch.optim.SGD(m.encoder_q.parameters(), lr=0.1)
        out = str(tmp_path / ("f" if fused else "u"))
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res = UberNCE_train_epoch(loader(4), m, nn.CrossEntropyLoss(), opt, 7, epoch_cfg(arch, out), False, "cpu", True, fused=fused)
        lines = buf.getvalue().splitlines()
        logs = [l for l in lines if l.startswith("Train Epoch: 7 [")]
        assert len(logs) == 2 and m.training
        assert re.fullmatch(r"Train Epoch: 7 \[8/16 \| 50\.0%\]\tLoss: \d+\.\d{4} \(\d+\.\d{4}\)  Top1:\d\.\d+ Top5:\d\.\d+", logs[0]), logs[0]
        assert logs[1].startswith("Train Epoch: 7 [16/16 | 100.0%]")
        assert any(re.fullmatch(r"Train set: Average loss: \d+\.\d{4}", l) for l in lines)
        assert any(l.startswith("epoch:7 runtime:") for l in lines) and lines[-1] == f"saved to file:{out}/tnet_checkpoints/train_loss_and_acc.txt"
        log = open(os.path.join(out, "tnet_checkpoints", "train_loss_and_acc.txt")).read()
        assert re.fullmatch(r"epoch:7 runtime:\d+\.\d+ \d+\.\d{4}\n", log), log
        assert len(res) == 2 and all(0.0 <= r <= 1.0 for r in res) and int(m.queue_ptr) == (4 * B) % K
        results[fused] = (res, log.split()[-1], [p.detach().clone() for p in m.encoder_q.parameters()])
    if len(results) == 2:
        assert results[True][:2] == results[False][:2]
        for a, b in zip(results[True][2], results[False][2]):
            assert close(a, b, 1e-5)
    with pytest.raises(ValueError):
        UberNCE_train_epoch(loader(1), make(cls), None, None, 0, epoch_cfg("3dresnet", None), False, "cpu")


def test_calc_mask_accuracy_host_logic():
    from video_similarity_search_amd.online_train import calc_mask_accuracy
    out = torch.tensor([[3., 1., 2., 2.], [0., 5., 5., 1.], [1., 2., 3., 4.]])
    mask = torch.tensor([[0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 0]]).bool()      # ranks 1, 1 (the tie goes to column 1), 4 (no positive)
    acc = calc_mask_accuracy(out, mask, (2, 1), kernels=NumpyInfoNCEKernels())
    assert [float(a) for a in acc] == [float(np.float32(2) / np.float32(3)), 0.0] and acc[0].dim() == 0
    with pytest.raises(ValueError):
        calc_mask_accuracy(out, mask, (5,), kernels=NumpyInfoNCEKernels())


def test_model_selector():
    from video_similarity_search_amd.models.infoNCE import InfoNCE, UberNCE
    from video_similarity_search_amd.models.model_utils import model_selector
    with contextlib.redirect_stdout(io.StringIO()):
        a = model_selector(ns(MODEL=ns(ARCH="info_nce"), RESNET=ns(MODEL_DEPTH=10)))
        b = model_selector(ns(MODEL=ns(ARCH="uber_nce"), RESNET=ns(MODEL_DEPTH=10)))
    assert type(a) is InfoNCE and type(b) is UberNCE and (a.dim, a.K, a.m, a.T) == (128, 2048, 0.999, 0.07)
    assert tuple(b.queue_label.shape) == (2048,) and len(a.encoder_q[0].layer1) == 1
    with pytest.raises(NotImplementedError):
        model_selector(ns(MODEL=ns(ARCH="slowfast")))


# ---------------------------------------------------------------------------------------------------------------------------------
# the golden steps on the CPU: golden weights, the trunk through the oracle's torch restatement, everything else the module's own
# host logic on the NumPy provider, in float64.  Gates: 4 x the reference's fp32 deviation from float64, as on the GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def oracle_trunk():
    from oracle import encoder as oe
    from video_similarity_search_amd.models import generate_model
    net = generate_model(10, **gen.TRUNK_KW)                    # the parameter / buffer container with the reference's names

    def forward(x):
        sd = dict(net.named_parameters())
        sd.update(net.named_buffers())
        return oe.encoder_forward(sd, x.to(net.conv1.weight.dtype), net.training, projection_head=False)
    net.forward = forward
    return net


def mgate(name):
    return 4.0 * float(G["dev_" + name])


@pytest.mark.parametrize("path", ["forward", "contrast"])
@pytest.mark.parametrize("tag", ["info", "uber"])
def test_golden_steps_on_the_cpu(tag, path):
    from video_similarity_search_amd.models import infoNCE
    labelled = tag == "uber"
    sd, blks = gen.draw_case(211 if tag == "info" else 223, labelled)
    with contextlib.redirect_stdout(io.StringIO()):
        m = getattr(infoNCE, "UberNCE" if labelled else "InfoNCE")(oracle_trunk, gen.DIM, gen.K, gen.M, gen.T, kernels=NumpyInfoNCEKernels())
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    m = m.double().train()
    for it in range(gen.STEPS):
        train = it < gen.STEPS - 1
        blk = torch.from_numpy(blks[it]).double()
        lab = torch.from_numpy(gen.LABELS[it]) if labelled else None
        w_logits, w_target, w_loss = G[f"{tag}/logits{it}"].astype(np.float64), G[f"{tag}/target{it}"], float(G[f"{tag}/loss{it}"])
        mask = w_target.astype(bool) if labelled else np.arange(gen.K + 1)[None, :] == np.zeros((gen.B, 1), int)
        lo = [np.mean(rank_of_best(w_logits - mgate("logits") * mask, mask) < k) for k in (1, 5)]
        hi = [np.mean(rank_of_best(w_logits + mgate("logits") * mask, mask) < k) for k in (1, 5)]
        m.zero_grad(set_to_none=True)
        with torch.set_grad_enabled(train):
            if path == "forward":
                logits, target = m(blk, lab) if labelled else m(blk)
                assert np.abs(logits.detach().numpy() - w_logits).max() <= mgate("logits")
                assert np.array_equal(target.numpy(), w_target)
                loss = (-(F.log_softmax(logits, 1) * target).sum(1) / target.sum(1)).mean() if labelled else F.cross_entropy(logits, target)
                accs = None
            else:
                loss, accs = m(blk, lab, fused=True) if labelled else m(blk, fused=True)
                accs = [float(a) for a in accs]
                assert all(l <= a <= h for l, a, h in zip(lo, accs, hi))
                if lo == hi:
                    assert accs == G[f"{tag}/acc{it}"].tolist()
        assert abs(loss.item() - w_loss) <= mgate("loss") * abs(w_loss)
        if train:
            loss.backward()
            for n, p in m.encoder_q.named_parameters():
                want = G[f"{tag}/grad{it}/{n}"]
                assert np.abs(gen.strided(p.grad.numpy()) - want).max() <= mgate("grad") * max(np.abs(want).max(), 1e-30), (n, it)
        assert int(m.queue_ptr) == int(G[f"{tag}/ptr{it}"])
        assert np.abs(m.queue.numpy() - G[f"{tag}/queue{it}"]).max() <= mgate("queue")
        if labelled:
            assert np.array_equal(m.queue_label.numpy(), G[f"{tag}/queue_label{it}"])
    for n, v in m.state_dict().items():
        if n.startswith("encoder_k."):
            want = G[f"{tag}/final/{n}"]
            if v.dtype.is_floating_point:
                assert np.abs(gen.strided(v.numpy()) - want).max() <= mgate("key") * max(np.abs(want).max(), 1e-30), n
            else:
                assert np.array_equal(gen.strided(v.numpy()), want), n          # num_batches_tracked: the key encoder ran in train mode

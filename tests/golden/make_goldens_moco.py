"""
Generates tests/golden/moco.npz in the BUILD container by importing the reference's loss/NCE_loss.py (MemoryMoCo :188-241,
NCEAverage_intra_neg :91-184, NCESoftmaxLoss, NCECriterion) with the oracle-only .cuda() shim.
    python tests/golden/make_goldens_moco.py
Inputs come from numpy's PCG64 and are stored, so the GPU box regenerates nothing.

Also measured here and stored (dev_*): how far the reference itself, fp32 torch on the CPU, is from the float64 provider
(tests/moco_cpu_kernels.py) on these inputs.  The tests gate at 4 x these numbers.
"""
import os
import sys
sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
torch.Tensor.cuda = lambda self, *a, **k: self              # oracle-only shim for hard-coded .cuda()
nn.Module.cuda = lambda self, *a, **k: self
from loss.NCE_loss import MemoryMoCo, NCEAverage_intra_neg, NCECriterion, NCESoftmaxLoss      # noqa: E402  (the reference)
import moco_cpu_kernels as ref64                                                              # noqa: E402

rng = np.random.default_rng(97)
out = {}
T, NDATA = 0.07, 1000
dev = dict(logits=0.0, exp=0.0, loss=0.0, dq=0.0, dq_exp=0.0)


def unit(n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


# ---- MemoryMoCo: three consecutive calls, both use_softmax modes.  c1 (K=60, B=26): index 0 -> 26 -> 52 -> 18, the third call wraps
for name, (K, D, B) in (("c0", (64, 16, 8)), ("c1", (60, 128, 26))):
    qs, ks = [unit(B, D) for _ in range(3)], [unit(B, D) for _ in range(3)]
    for it in range(3):
        out[f"{name}_q{it}"], out[f"{name}_k{it}"] = qs[it], ks[it]
    out[f"{name}_shape"] = np.array([K, D, B], np.int64)
    for soft in (True, False):
        tag = f"{name}_{'soft' if soft else 'exp'}"
        torch.manual_seed(5)
        m = MemoryMoCo(D, NDATA, K, T, use_softmax=soft)
        out[f"{name}_memory0"] = m.memory.clone().numpy()
        for it in range(3):
            mem_before = m.memory.clone().double().numpy()
            q = torch.from_numpy(qs[it]).requires_grad_(True)
            o = m(q, torch.from_numpy(ks[it]))
            loss = NCESoftmaxLoss()(o)
            loss.backward()
            out[f"{tag}_out{it}"], out[f"{tag}_loss{it}"], out[f"{tag}_dq{it}"] = o.detach().numpy(), loss.detach().numpy(), q.grad.numpy().copy()
            out[f"{name}_index{it}"] = np.int64(m.index)
            if name == "c0" or it == 2:
                out[f"{name}_memory_after{it}"] = m.memory.clone().numpy()
            # the same call in float64
            q64, k64 = qs[it].astype(np.float64), ks[it].astype(np.float64)
            x64 = ref64.logits(q64, k64, mem_before, T)
            if soft:
                l64, dq64, _ = ref64.ce(q64, k64, mem_before, T)
                dev["logits"] = max(dev["logits"], np.abs(o.detach().numpy() - x64).max())
                dev["loss"] = max(dev["loss"], abs(float(loss) - l64) / abs(l64))
                dev["dq"] = max(dev["dq"], np.abs(q.grad.numpy() - dq64).max() / np.abs(dq64).max())
            else:
                Z = float(m.params[0].item())
                qt = torch.from_numpy(q64).requires_grad_(True)
                xt = torch.cat(((qt * torch.from_numpy(k64)).sum(1, keepdim=True), qt @ torch.from_numpy(mem_before).t()), 1) / T
                ot = torch.exp(xt) / Z
                lt = F.cross_entropy(ot, torch.zeros(B, dtype=torch.long))
                lt.backward()
                dev["exp"] = max(dev["exp"], (np.abs(o.detach().numpy() - ot.detach().numpy()) / ot.detach().numpy()).max())
                dev["loss"] = max(dev["loss"], abs(float(loss) - float(lt)) / abs(float(lt)))
                dev["dq_exp"] = max(dev["dq_exp"], np.abs(q.grad.numpy() - qt.grad.numpy()).max() / np.abs(qt.grad.numpy()).max())
        if not soft:
            out[f"{name}_Z"] = m.params.clone().numpy()
        print(tag, "index", [int(out[f"{name}_index{i}"]) for i in range(3)], "loss", [float(out[f"{tag}_loss{i}"]) for i in range(3)],
              "Z", int(m.params[0]))

# ---- the multi-positive loss (models/infoNCE.py:281-283 mask, online_train.py:96-97), torch float64
K, D, B = 64, 16, 8
mem = unit(K, D)
q, k = unit(B, D), unit(B, D)
queue_label = rng.integers(3, 9, K).astype(np.int64)
queue_label[rng.choice(K, 12, replace=False)] = -1          # empty slots
queue_label[queue_label == 1] = 3
queue_label[5] = 1                                           # label 1: once in the queue -> 2 positives; label 0: never -> 1
queue_label[np.arange(20, 44)] = 2                           # label 2: 24 times -> 25 positives
k_label = np.array([0, 1, 2, 2, 0, 4, 1, 7], np.int64)
qt = torch.from_numpy(q.astype(np.float64)).requires_grad_(True)
logit = torch.cat(((qt * torch.from_numpy(k.astype(np.float64))).sum(1, keepdim=True), qt @ torch.from_numpy(mem.astype(np.float64)).t()), 1) / T
mask = torch.from_numpy(k_label).unsqueeze(1) == torch.from_numpy(queue_label).unsqueeze(0)
mask = torch.cat([torch.ones((B, 1), dtype=torch.long).bool(), mask], dim=1)
rows = - (F.log_softmax(logit, dim=1) * mask).sum(1) / mask.sum(1)
lt = rows.mean()
lt.backward()
out.update(mp_memory=mem, mp_q=q, mp_k=k, mp_queue_label=queue_label, mp_k_label=k_label, mp_loss=lt.detach().numpy(),
           mp_rowloss=rows.detach().numpy(), mp_dq=qt.grad.numpy().copy(), mp_npos=mask.sum(1).numpy().astype(np.int64))
print("multi-positive: n_pos", mask.sum(1).tolist(), "loss", float(lt))

# ---- NCEAverage_intra_neg: two calls with a fixed idx, both modes (use_softmax=False: Z as written at :145-159)
B, D, K, ndata = 4, 16, 8, 50
ins = []
for it in range(2):
    y = rng.choice(ndata, B, replace=False).astype(np.int64)
    idx = rng.integers(0, ndata, (B, K + 1)).astype(np.int64)
    idx[:, 0] = y
    ins.append((unit(B, D), unit(B, D), unit(B, D), y, idx))
    for nm, a in zip(("l", "ab", "neg", "y", "idx"), ins[-1]):
        out[f"in_{nm}{it}"] = a
for soft in (True, False):
    tag = "in_soft" if soft else "in_exp"
    torch.manual_seed(13)
    nce = NCEAverage_intra_neg(D, ndata, K, T, 0.5, use_softmax=soft)
    out["in_memory_l0"], out["in_memory_ab0"], out["in_memory_neg0"] = (b.clone().numpy() for b in (nce.memory_l, nce.memory_ab, nce.memory_neg))
    crit = NCESoftmaxLoss() if soft else NCECriterion(ndata)
    for it, (l, ab, neg, y, idx) in enumerate(ins):
        lt_, abt = torch.from_numpy(l).requires_grad_(True), torch.from_numpy(ab).requires_grad_(True)
        o_l, o_ab = nce(lt_, abt, torch.from_numpy(neg), torch.from_numpy(y), torch.from_numpy(idx).clone())
        tot = crit(o_l) + crit(o_ab)
        tot.backward()
        out.update({f"{tag}_out_l{it}": o_l.detach().numpy(), f"{tag}_out_ab{it}": o_ab.detach().numpy(), f"{tag}_loss{it}": tot.detach().numpy(),
                    f"{tag}_grad_l{it}": lt_.grad.numpy().copy(), f"{tag}_grad_ab{it}": abt.grad.numpy().copy()})
    out[f"{tag}_memory_l2"], out[f"{tag}_memory_ab2"], out[f"{tag}_memory_neg2"] = (b.clone().numpy() for b in (nce.memory_l, nce.memory_ab, nce.memory_neg))
    out[f"{tag}_params"] = nce.params.detach().numpy().copy()
    print(tag, "loss", float(tot), "params", nce.params.tolist())

for n, v in dev.items():
    out[f"dev_{n}"] = np.float64(v)
print("reference (fp32) vs float64 provider:", {n: float(v) for n, v in dev.items()})
np.savez_compressed(os.path.join(HERE, "moco.npz"), **out)
print("moco goldens:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "moco.npz")), "bytes")

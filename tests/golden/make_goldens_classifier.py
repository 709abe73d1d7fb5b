"""
Generates tests/golden/classifier.npz in the BUILD container from the reference's models/resnet.py with classifier=True
(:192-201, 247-252, 305-307) and coclr_utils/utils.py calc_topk_accuracy (:55-75), in the style of make_goldens_encoder_options.py:
    python tests/golden/make_goldens_classifier.py
The reference's head is nn.Linear(512, C), so the models are full width: depth 10, clips [3, 3, 8, 16, 16] (small enough
that no ReLU input sits within rounding noise of zero — RELU_MARGIN below).  Weights and clips are
NOT stored — `draw_model` / `draw_logits` below (numpy PCG64 through oracle.encoder.make_state_dict, the generator of the other
encoder goldens; tests/golden/r3d_weights.py draws R3DNet's keys, not this model's) regenerate them, a checksum is stored — and
a backbone gradient is stored as at most 4096 evenly strided elements.

Model cases (`<tag>/...`):
    plain   projection_head=False, dropout=None: eval logits; train logits, CE loss, gradients of linear.* and of three backbone tensors
    proj    projection_head=True:  train logits, bn_proj's running statistics and counter after the pass, the parameters left with grad None
    drop    dropout=0.5 in eval mode (keys linear.1.*): logits
    probe   plain's weights, everything but linear.* frozen, model.eval(): logits, loss, gradients of linear.*
    <tag>/keys: the sorted state_dict keys
Loss cases (`ce/<name>/...`, LOSS_CASES): torch's CPU fp32 F.cross_entropy, the fp64 value, the fp32 gradient's largest deviation from
the fp64 gradient, and the reference's calc_topk_accuracy for (1, 5) (top-5 where C >= 5).  The maker asserts that no row has two
of its six largest logits closer than 1e-4 (relative to the case's scale), so the top-k order is unambiguous.
"""
import os
import sys
import types
sys.dont_write_bytecode = True
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from oracle import encoder as oe                          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NUM_CLASSES, HIDDEN, OUT_DIM = 11, 64, 32
CLIP = (3, 3, 8, 16, 16)
MODEL_SEED = 71
# Conditioning of the train-mode gradients.  A ReLU whose input is within rounding noise of zero takes either branch in any fp32
# arithmetic, and ONE flipped branch in the stem moves a channel of conv1.weight's gradient by ~1 % (it is a sum with cancellation
# over a few thousand positions: measured on the fp64 oracle with clips of [3, 3, 8, 32, 32], a 1e-6 relative perturbation of the
# clips moved it by 2.5e-2, and none of 129 seeds at that size kept its 1.5 M ReLU inputs further than 2.4e-6 rms from zero).
# fp32 accumulation over K = 1029 ... 13824 terms in another order differs by ~1e-6 of an activation's rms, so the clips are
# 16 x 16 (0.2 M ReLU inputs) and the maker demands that no ReLU input of the reference's train pass is closer to zero than
# RELU_MARGIN x the rms of its layer.
RELU_MARGIN = 5e-6
MODEL_CASES = (("plain", False, None), ("proj", True, None), ("drop", False, 0.5))      # tag, projection_head, dropout
GRAD_KEYS = ("conv1.weight", "layer2.0.downsample.0.weight", "layer4.0.conv2.weight", "layer4.0.bn2.weight")

LOSS_SEED = 2024
LOSS_CASES = [(f"n{B}x{C}", B, C, 1.0, C, "rand") for B in (1, 2, 33, 257) for C in (1, 2, 5, 63, 64, 65, 101, 129, 1000)]
LOSS_CASES += [("strided", 33, 101, 1.0, 108, "rand"), ("scaled33", 33, 101, 1e4, 101, "rand"), ("scaled257", 257, 1000, 1e4, 1000, "rand"),
               ("first", 33, 65, 1.0, 65, "first"), ("last", 33, 65, 1.0, 65, "last")]      # name, B, C, scale, row stride, targets


def draw_model(projection_head, dropout):
    """state_dict (reference init rules; BatchNorm affine and running statistics perturbed, `linear` drawn wide enough to matter)
    and the clip batch + targets of one model case"""
    rng = np.random.default_rng(MODEL_SEED)
    sd = oe.make_state_dict(rng, layers=(1, 1, 1, 1), widen=1.0, hidden=HIDDEN, out_dim=OUT_DIM, projection_head=projection_head)
    for k in sorted(sd):
        if ".bn" in k or k.startswith(("bn1.", "bn_proj.")) or ".downsample.1." in k:
            if k.endswith(".weight"):
                sd[k] = (1.0 + 0.1 * rng.standard_normal(sd[k].shape)).astype(np.float32)
            elif k.endswith((".bias", ".running_mean")):
                sd[k] = (0.1 * rng.standard_normal(sd[k].shape)).astype(np.float32)
            elif k.endswith(".running_var"):
                sd[k] = (1.0 + 0.2 * rng.random(sd[k].shape)).astype(np.float32)
    pre = "linear.1" if (dropout is not None and dropout > 0) else "linear"
    sd[pre + ".weight"] = (0.05 * rng.standard_normal((NUM_CLASSES, 512))).astype(np.float32)
    sd[pre + ".bias"] = (0.1 * rng.standard_normal(NUM_CLASSES)).astype(np.float32)
    x = rng.standard_normal(CLIP).astype(np.float32)
    y = rng.integers(0, NUM_CLASSES, CLIP[0]).astype(np.int64)
    return sd, x, y


def draw_logits(name):
    """(logits [B, C] fp32 — a view with row stride ld of a wider array when ld > C —, targets [B] int64) of one loss case;
    no row has two of its six largest logits closer than 1e-4 x the case's scale (top_gap_ok), so no row is ever skipped"""
    idx = [c[0] for c in LOSS_CASES].index(name)
    _, B, C, scale, ld, tmode = LOSS_CASES[idx]
    for attempt in range(64):          # redrawn (a deterministic sequence) until the top-k order of every row is unambiguous
        rng = np.random.default_rng([LOSS_SEED, idx, attempt])
        base = (rng.standard_normal((B, ld)) * scale).astype(np.float32)
        t = {"rand": rng.integers(0, C, B), "first": np.zeros(B), "last": np.full(B, C - 1)}[tmode].astype(np.int64)
        if top_gap_ok(base[:, :C], scale):
            return base[:, :C], t
    raise AssertionError(f"{name}: no draw with a 1e-4 gap between a row's six largest logits")


def top_gap_ok(logits, scale, gap=1e-4):
    """no row has two of its (up to) six largest logits closer than gap * scale"""
    s = -np.sort(-logits.astype(np.float64), axis=1)[:, :6]
    return s.shape[1] < 2 or float(np.min(s[:, :-1] - s[:, 1:])) >= gap * scale


def strided(a, limit=4096):
    """at most ~limit evenly strided elements; the step is kept coprime with 27 (a multiple of 3 would walk one tap of a 3 x 3 x 3 filter)"""
    a = np.asarray(a).reshape(-1)
    step = max(1, -(-a.size // limit))
    while step > 1 and step % 3 == 0:
        step += 1
    return a[::step].copy()


def checksum(sd, x):
    return np.array([float(np.sum(x, dtype=np.float64)), float(sum(np.sum(v, dtype=np.float64) for v in sd.values()))])


def main():
    tv = types.ModuleType("torchvision")                      # oracle-only shim: coclr_utils/utils.py imports it for its transforms
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tv.transforms)
    sys.path.insert(0, "/root/reference")
    from models.resnet import generate_model                  # the reference
    from coclr_utils.utils import calc_topk_accuracy
    import torch.nn.functional as F
    out = {}

    def build(proj, dropout):
        sd, x, y = draw_model(proj, dropout)
        m = generate_model(10, hidden_layer=HIDDEN, out_dim=OUT_DIM, num_classes=NUM_CLASSES, n_input_channels=3, shortcut_type='B',
                           conv1_t_size=7, conv1_t_stride=1, no_max_pool=True, widen_factor=1.0, projection_head=proj,
                           predict_temporal_ds=False, spatio_temporal_attention=False, classifier=True, dropout=dropout)
        assert sorted(m.state_dict()) == sorted(sd), set(m.state_dict()) ^ set(sd)
        m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
        return m, sd, torch.from_numpy(x), torch.from_numpy(y)

    for tag, proj, dropout in MODEL_CASES:
        m, sd, x, y = build(proj, dropout)
        out[f"{tag}/keys"] = np.array(sorted(m.state_dict()))
        out[f"{tag}/check"] = checksum(sd, x.numpy())
        m.eval()
        with torch.no_grad():
            out[f"{tag}/eval_logits"] = m(x).numpy()
        if tag == "drop":
            continue
        m.train()
        margins = []
        hooks = [mod.register_forward_pre_hook(lambda _m, inp: margins.append(float(inp[0].detach().abs().min() / inp[0].detach().pow(2).mean().sqrt())))
                 for mod in m.modules() if isinstance(mod, torch.nn.ReLU)]
        logits = m(x)
        for h in hooks:
            h.remove()
        print(f"  {tag}: smallest |ReLU input| / rms over {len(margins)} ReLU calls: {min(margins):.2e}")
        assert min(margins) >= RELU_MARGIN, f"{tag}: a ReLU input within {RELU_MARGIN} rms of zero — raise MODEL_SEED"
        loss = torch.nn.CrossEntropyLoss()(logits, y)
        loss.backward()
        out[f"{tag}/train_logits"], out[f"{tag}/loss"] = logits.detach().numpy(), loss.detach().numpy()
        print(tag, "loss", float(loss), "top1/top5", [float(v) for v in calc_topk_accuracy(logits, y, (1, 5))])
        if tag == "plain":
            # the fp64 run of the same graph: how far the reference's own fp32 gradients are from exact (the test's tolerance must sit above it)
            m64, _, _, _ = build(proj, dropout)
            m64 = m64.double().train()
            torch.nn.CrossEntropyLoss()(m64(x.double()), y).backward()
            g64 = dict((k, p.grad) for k, p in m64.named_parameters())
            for k, p in m.named_parameters():
                if k in GRAD_KEYS or k.startswith("linear"):
                    out[f"{tag}/grad/{k}"] = strided(p.grad.numpy())
                    dev = float((p.grad.double() - g64[k]).abs().max() / g64[k].abs().max())
                    print(f"  grad {k}: fp32 vs fp64 max-norm deviation {dev:.2e}")
                    assert dev < 1e-4, "the reference's fp32 gradient is not a usable yardstick at 5e-4 here"
        if tag == "proj":
            out[f"{tag}/grad_none"] = np.array(sorted(k for k, p in m.named_parameters() if p.grad is None))
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                out[f"{tag}/after/bn_proj.{k}"] = m.state_dict()["bn_proj." + k].numpy().copy()
            print("  grad None:", list(out[f"{tag}/grad_none"]))

    # linear probe (coclr_classify.py:172-179, 406-407): everything but linear.* frozen, model.eval()
    m, sd, x, y = build(False, None)
    for k, p in m.named_parameters():
        p.requires_grad_(k.startswith("linear"))
    m.eval()
    logits = m(x)
    loss = torch.nn.CrossEntropyLoss()(logits, y)
    loss.backward()
    out["probe/logits"], out["probe/loss"] = logits.detach().numpy(), loss.detach().numpy()
    out["probe/grad/linear.weight"], out["probe/grad/linear.bias"] = m.linear.weight.grad.numpy(), m.linear.bias.grad.numpy()
    assert all(p.grad is None for k, p in m.named_parameters() if not k.startswith("linear"))
    print("probe loss", float(loss))

    for name, B, C, scale, ld, tmode in LOSS_CASES:
        lg, t = draw_logits(name)
        assert top_gap_ok(lg, scale), f"{name}: two of a row's six largest logits are closer than 1e-4 — change LOSS_SEED"
        x32 = torch.from_numpy(np.ascontiguousarray(lg)).requires_grad_(True)
        x64 = x32.detach().double().requires_grad_(True)
        tt = torch.from_numpy(t)
        l32, l64 = F.cross_entropy(x32, tt), F.cross_entropy(x64, tt)
        l32.backward()
        l64.backward()
        ks = (1, 5) if C >= 5 else (1,)
        acc = calc_topk_accuracy(x32.detach(), tt, ks)
        out[f"ce/{name}/loss32"], out[f"ce/{name}/loss64"] = np.float32(l32.item()), np.float64(l64.item())
        out[f"ce/{name}/grad_err32"] = np.float64((x32.grad.double() - x64.grad).abs().max().item())
        out[f"ce/{name}/topk"] = np.array([float(a) for a in acc])
        out[f"ce/{name}/check"] = np.float64(np.sum(lg, dtype=np.float64) + np.sum(t))
    np.savez_compressed(os.path.join(HERE, "classifier.npz"), **out)
    print("classifier goldens:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "classifier.npz")), "bytes")


if __name__ == "__main__":
    main()

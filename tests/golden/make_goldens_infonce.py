"""
Generates tests/golden/infonce.npz in the BUILD container by running the reference's own models/infoNCE.py InfoNCE and UberNCE, with
the loss and accuracies of the reference's UberNCE_train_epoch (online_train.py:43-57, 88-98; coclr_utils/utils.py:55-75).
    python tests/golden/make_goldens_infonce.py /path/to/reference
`select_backbone` is replaced by the reference's tiny-width generate_model trunk (depth 10, widen 0.125, projection_head=False, its
pooled output reshaped to [B, F, 1, 1, 1]); the process group is one gloo process; hard-coded .cuda() calls are the identity.
Three consecutive train steps (K = 12, B = 4: the third enqueue wraps to the start) and one no_grad step.

Kept small: the weights and the clips are NOT stored.  `draw_case` below (numpy PCG64, oracle.encoder.make_state_dict) regenerates
them in the test; a checksum is stored.  Gradients and the key encoder's final parameters are stored as at most 1024 evenly strided
elements per tensor.  dev_*: how far the reference in fp32 is from the same classes run in float64 on the same inputs; the tests
gate at 4 x these.
"""
import importlib.abc
import importlib.machinery
import os
import sys
import tempfile
import types
sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from oracle import encoder as oe                          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
WIDEN, FEAT, DIM, K, B, T, M = 0.125, 64, 32, 12, 4, 0.07, 0.999
CLIP = (3, 8, 32, 32)
STEPS = 4                                                  # three train steps, one no_grad step
TRUNK_KW = dict(n_input_channels=3, shortcut_type='B', conv1_t_size=7, conv1_t_stride=1, no_max_pool=True, widen_factor=WIDEN,
                projection_head=False)
LABELS = np.array([[0, 1, 2, 0], [1, 1, 0, 3], [2, 0, 0, 1], [0, 2, 1, 1]], np.int64)       # k_label of step i (UberNCE)


def strided(a, limit=1024):
    a = np.asarray(a).reshape(-1)
    step = max(1, -(-a.size // limit))
    while step > 1 and step % 3 == 0:
        step += 1
    return a[::step].copy()


def draw_case(seed, labelled):
    """(initial state dict of the model, clip blocks [STEPS, B, 2, C, T, H, W]) in the generator's draw order"""
    rng = np.random.default_rng(seed)
    trunk = oe.make_state_dict(rng, layers=(1, 1, 1, 1), widen=WIDEN, hidden=8, out_dim=8)
    trunk = {k: v for k, v in trunk.items() if not k.startswith(("fc1.", "fc2.", "bn_proj."))}
    for k in trunk:
        if k.endswith(("bn1.weight", "bn2.weight", "downsample.1.weight")):
            trunk[k] = (1.0 + 0.1 * rng.standard_normal(trunk[k].shape)).astype(np.float32)
        if k.endswith(("bn1.bias", "bn2.bias", "downsample.1.bias")):
            trunk[k] = (0.1 * rng.standard_normal(trunk[k].shape)).astype(np.float32)
    head = {"2.weight": (rng.standard_normal((FEAT, FEAT, 1, 1, 1)) * np.sqrt(2.0 / FEAT)).astype(np.float32),
            "2.bias": (0.1 * rng.standard_normal(FEAT)).astype(np.float32),
            "4.weight": (rng.standard_normal((DIM, FEAT, 1, 1, 1)) * np.sqrt(1.0 / FEAT)).astype(np.float32),
            "4.bias": (0.1 * rng.standard_normal(DIM)).astype(np.float32)}
    sd = {}
    for enc in ("encoder_q", "encoder_k"):
        for k, v in trunk.items():
            sd[f"{enc}.0.{k}"] = v.copy()
        for k, v in head.items():
            sd[f"{enc}.{k}"] = v.copy()
    queue = rng.standard_normal((DIM, K)).astype(np.float32)
    sd["queue"] = (queue / np.linalg.norm(queue, axis=0, keepdims=True)).astype(np.float32)
    sd["queue_ptr"] = np.zeros(1, np.int64)
    if labelled:
        sd["queue_label"] = np.full(K, -1, np.int64)
    blocks = rng.standard_normal((STEPS, B, 2) + CLIP).astype(np.float32)
    return sd, blocks


def checksum(sd, blocks):
    return np.array([float(np.sum(blocks, dtype=np.float64)), float(sum(np.sum(v, dtype=np.float64) for v in sd.values()))])


class _Any:
    """stands in for every name of a replaced module"""

    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Any()

    def __call__(self, *a, **k):
        return a[0] if len(a) == 1 and not k and callable(a[0]) else _Any()


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Any


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """modules the reference's training script imports and this generator never calls"""
    STUBS = ("torchvision", "cv2", "fvcore", "PIL", "matplotlib", "seaborn", "datasets", "spatial_transforms", "temporal_transforms",
             "config", "simplejson", "iopath", "psutil", "tensorboard", "kornia", "av", "pandas", "h5py", "skimage", "slowfast", "spherecluster",
             "finch", "faiss", "hdbscan", "umap")

    def find_spec(self, fullname, path, target=None):
        if fullname.split(".")[0] in self.STUBS:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        return _Stub(spec.name)

    def exec_module(self, module):
        pass


def main(reference):
    sys.meta_path.insert(0, _StubFinder())
    sys.path.insert(0, reference)
    torch.Tensor.cuda = lambda self, *a, **k: self            # oracle-only shim for hard-coded .cuda()
    nn.Module.cuda = lambda self, *a, **k: self
    from models.resnet import generate_model                  # noqa: E402  (the reference)
    import models.infoNCE as ref_nce                          # noqa: E402
    from coclr_utils.utils import calc_topk_accuracy          # noqa: E402

    def tiny_backbone(network):
        net = generate_model(10, **TRUNK_KW)
        inner = net.forward
        net.forward = lambda x: inner(x).view(x.shape[0], FEAT, 1, 1, 1)
        return net, {'feature_size': FEAT}
    ref_nce.select_backbone = tiny_backbone

    from online_train import calc_mask_accuracy as mask_accuracy      # noqa: E402

    with tempfile.TemporaryDirectory() as d:
        torch.distributed.init_process_group("gloo", init_method="file://" + os.path.join(d, "pg"), rank=0, world_size=1)
        out, dev = {}, dict(logits=0.0, loss=0.0, grad=0.0, queue=0.0, key=0.0)
        for tag, cls, seed in (("info", ref_nce.InfoNCE, 211), ("uber", ref_nce.UberNCE, 223)):
            labelled = tag == "uber"
            sd, blocks = draw_case(seed, labelled)
            out[f"{tag}/check"] = checksum(sd, blocks)
            out[f"{tag}/keys"] = np.array(sorted(sd))
            out[f"{tag}/shapes"] = np.array([",".join(map(str, sd[k].shape)) for k in sorted(sd)])
            runs = {}
            for dt in (torch.float32, torch.float64):
                torch.manual_seed(3)
                m = cls('s3d', dim=DIM, K=K, m=M, T=T)
                assert sorted(m.state_dict()) == sorted(sd), set(m.state_dict()) ^ set(sd)
                m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
                if dt == torch.float64:
                    m = m.double()
                m.train()
                torch.manual_seed(5)                            # the batch shuffle draws from the global generator
                rec = []
                for it in range(STEPS):
                    x = torch.from_numpy(blocks[it]).to(dt)
                    lab = torch.from_numpy(LABELS[it])
                    for p in m.parameters():
                        p.grad = None
                    with torch.set_grad_enabled(it < STEPS - 1):
                        if labelled:
                            logits, target = m(x, lab)
                            loss = (-(F.log_softmax(logits, dim=1) * target).sum(1) / target.sum(1)).mean()
                            acc = mask_accuracy(logits.detach(), target, (1, 5))
                        else:
                            logits, target = m(x)
                            loss = F.cross_entropy(logits, target)
                            acc = calc_topk_accuracy(logits.detach(), target, (1, 5))
                    if it < STEPS - 1:
                        loss.backward()
                    rec.append(dict(logits=logits.detach().numpy().copy(), target=target.numpy().copy(), loss=float(loss),
                                    acc=np.array([float(a) for a in acc]),
                                    grads={k: p.grad.numpy().copy() for k, p in m.encoder_q.named_parameters() if p.grad is not None},
                                    queue=m.queue.numpy().copy(), ptr=int(m.queue_ptr),
                                    qlabel=m.queue_label.numpy().copy() if labelled else None))
                runs[dt] = (rec, {k: v.numpy().copy() for k, v in m.state_dict().items()})
            rec32, final32 = runs[torch.float32]
            rec64, final64 = runs[torch.float64]
            for it, (a, b) in enumerate(zip(rec32, rec64)):
                out[f"{tag}/logits{it}"], out[f"{tag}/target{it}"] = a["logits"], a["target"]
                out[f"{tag}/loss{it}"], out[f"{tag}/acc{it}"] = np.float64(a["loss"]), a["acc"]
                out[f"{tag}/queue{it}"], out[f"{tag}/ptr{it}"] = a["queue"], np.int64(a["ptr"])
                if labelled:
                    out[f"{tag}/queue_label{it}"] = a["qlabel"]
                assert np.array_equal(a["target"], b["target"]) and a["ptr"] == b["ptr"]
                dev["logits"] = max(dev["logits"], np.abs(a["logits"] - b["logits"]).max())
                dev["loss"] = max(dev["loss"], abs(a["loss"] - b["loss"]) / abs(b["loss"]))
                dev["queue"] = max(dev["queue"], np.abs(a["queue"] - b["queue"]).max())
                for k, g in a["grads"].items():
                    out[f"{tag}/grad{it}/{k}"] = strided(g)
                    dev["grad"] = max(dev["grad"], np.abs(g - b["grads"][k]).max() / max(np.abs(b["grads"][k]).max(), 1e-30))
                print(tag, it, "loss", a["loss"], "acc", a["acc"].tolist(), "ptr", a["ptr"], "positives", a["target"].sum() if labelled else B)
            for k, v in final32.items():
                if k.startswith("encoder_k."):
                    out[f"{tag}/final/{k}"] = strided(v)
                    if v.dtype.kind == "f":
                        dev["key"] = max(dev["key"], np.abs(v - final64[k]).max() / max(np.abs(final64[k]).max(), 1e-30))
        torch.distributed.destroy_process_group()
    for n, v in dev.items():
        out[f"dev_{n}"] = np.float64(v)
    print("reference fp32 vs the reference in float64:", {n: float(v) for n, v in dev.items()})
    path = os.path.join(HERE, "infonce.npz")
    np.savez_compressed(path, **out)
    print("infonce goldens:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))

"""Generates tests/golden/linear_sites_parent.json on a gfx950 device: what the library's linear layers computed, and which entry points
they called, on the commit BEFORE the five hand-written copies of the 1x1x1-convolution recipe moved onto LinearPlan (HipLinear, the
InfoNCE head, the classifier head, the projection head).  tests/test_linear_sites_gpu.py imports the cases from here, re-runs them on the
tree and demands the same bits and the same calls.

    python tests/golden/make_goldens_linear_sites.py --commit ID [--out FILE]      # writes the record (run it on the parent commit)
    python tests/golden/make_goldens_linear_sites.py --check                       # the tree against the committed record

Per case the record holds, for every output tensor, its shape and the SHA-256 of its bytes (null for a gradient that was not asked for),
and the multiset name -> count of the library entry points called during the case's pass (slic_last_error and the *_workspace_bytes
queries included).  Calls are counted by putting a proxy in the place of `video_similarity_search_amd._lib._lib`, the object load()
returns, for the length of the pass: its __getattr__ counts the name and hands back the real function.  The record is a multiset, not
a sequence: HipLinear's backward launched its data gradient first before the move and launches it last after.

Every case builds its objects fresh (plans build their tables on first use, so the counts include those) and runs ONE pass.  Inputs
and weights are drawn from the numpy.random.default_rng seeds below; the upstream gradient is drawn too and handed to backward(), so no
loss kernel and no torch reduction enters.
    linear_*    HipLinear(12, 20): B = 3, B = 70 (two 64-row tiles), no bias, input without a gradient          -> y, dx, dW, db
    nce_*       HipInfoNCEKernels().head_fwd / head_bwd at F = 64, dim = 32: B = 1, 5, 70, and B = 5 with need_dx=False
                                                                                                                 -> y, inv, five gradients
    cls*_*      generate_model(10, classifier=True, projection_head=False) at full width, 2 clips of [3, 8, 16, 16], 8 classes (no padding)
                and 101 (padded to 104): a training pass, the linear-probe pass (trunk frozen, eval mode), a training pass with
                linear.weight frozen                              -> logits, gradients of linear.weight / linear.bias and of bn1.weight
    proj_*      generate_model(10, projection_head=True) at widen 0.125, hidden 64, out 32, 4 clips of [3, 8, 32, 32], training pass; and
                the same with fc2.bias frozen                     -> embedding, gradients of fc1.* / bn_proj.* / fc2.* and of bn1.weight
"""
import contextlib
import hashlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "linear_sites_parent.json")

# the tiny keyword sets of tests/test_classifier_gpu.py (KW) and of the encoder golden (make_goldens_encoder.tiny_model)
CLS_KW = dict(hidden_layer=64, out_dim=32, n_input_channels=3, shortcut_type='B', conv1_t_size=7, conv1_t_stride=1, no_max_pool=True,
              widen_factor=1.0, predict_temporal_ds=False, spatio_temporal_attention=False, classifier=True, projection_head=False,
              dropout=None)
PROJ_KW = dict(hidden_layer=64, out_dim=32, num_classes=101, n_input_channels=3, shortcut_type='B', conv1_t_size=7, conv1_t_stride=1,
               no_max_pool=True, widen_factor=0.125, projection_head=True, predict_temporal_ds=False, spatio_temporal_attention=False,
               classifier=False, dropout=None)
CLS_CLIP, PROJ_CLIP = (2, 3, 8, 16, 16), (4, 3, 8, 32, 32)
LIN_IN, LIN_OUT = 12, 20
NCE_F, NCE_DIM = 64, 32

# name -> (kind, parameters, seed)
_CASES = {
    "linear_b3": ("linear", dict(B=3, bias=True, x_grad=True), 101),
    "linear_b70": ("linear", dict(B=70, bias=True, x_grad=True), 102),
    "linear_nobias_b3": ("linear", dict(B=3, bias=False, x_grad=True), 103),
    "linear_b3_no_dx": ("linear", dict(B=3, bias=True, x_grad=False), 104),
    "nce_b1": ("nce", dict(B=1, need_dx=True), 201),
    "nce_b5": ("nce", dict(B=5, need_dx=True), 202),
    "nce_b70": ("nce", dict(B=70, need_dx=True), 203),
    "nce_b5_no_dx": ("nce", dict(B=5, need_dx=False), 204),
    "cls8_train": ("cls", dict(num_classes=8, mode="train"), 301),
    "cls101_train": ("cls", dict(num_classes=101, mode="train"), 302),
    "cls8_probe": ("cls", dict(num_classes=8, mode="probe"), 303),
    "cls101_probe": ("cls", dict(num_classes=101, mode="probe"), 304),
    "cls8_weight_frozen": ("cls", dict(num_classes=8, mode="weight_frozen"), 305),
    "cls101_weight_frozen": ("cls", dict(num_classes=101, mode="weight_frozen"), 306),
    "proj_train": ("proj", dict(frozen=()), 401),
    "proj_fc2_bias_frozen": ("proj", dict(frozen=("fc2.bias",)), 402),
}
CASES = tuple(_CASES)


class _Counting:
    """stands where load()'s library object stands: counts every attribute asked of it and hands back the library's own"""

    def __init__(self, real, counts):
        self._real, self._counts = real, counts

    def __getattr__(self, name):
        self._counts[name] = self._counts.get(name, 0) + 1
        return getattr(self._real, name)


@contextlib.contextmanager
def counting():
    from video_similarity_search_amd import _lib
    real = _lib.load()
    counts = {}
    _lib._lib = _Counting(real, counts)
    try:
        yield counts
    finally:
        _lib._lib = real


def digest(t):
    if t is None:
        return None
    a = t.detach().cpu().contiguous().numpy()
    return {"shape": list(a.shape), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def fill(model, rng):
    """every floating tensor of the state dict from rng, in the state dict's order: He-scaled weights, BatchNorm affine around (1, 0),
    biases and running means 0.1 sigma, running variances in [1, 1.2)"""
    import torch
    new = {}
    for k, v in model.state_dict().items():
        if not v.dtype.is_floating_point:
            continue
        shape = tuple(v.shape)
        if k.endswith("running_var"):
            a = 1.0 + 0.2 * rng.random(shape)
        elif k.endswith(("running_mean", ".bias")):
            a = 0.1 * rng.standard_normal(shape)
        elif v.dim() == 1:
            a = 1.0 + 0.1 * rng.standard_normal(shape)
        else:
            a = rng.standard_normal(shape) * np.sqrt(2.0 / int(np.prod(shape[1:])))
        new[k] = torch.from_numpy(f32(a))
    model.load_state_dict(new, strict=False)


def _model(kw, rng):
    from video_similarity_search_amd.models import generate_model
    with contextlib.redirect_stdout(io.StringIO()):
        m = generate_model(10, **kw)
    fill(m, rng)
    return m.cuda()


def _linear(rng, B, bias, x_grad):
    import torch
    from video_similarity_search_amd.models.r3d import HipLinear
    lin = HipLinear(LIN_IN, LIN_OUT, bias=bias)
    fill(lin, rng)
    lin = lin.cuda()
    x = torch.from_numpy(f32(rng.standard_normal((B, LIN_IN)))).cuda().requires_grad_(x_grad)
    dy = torch.from_numpy(f32(rng.standard_normal((B, LIN_OUT)))).cuda()

    def step():
        y = lin(x)
        y.backward(dy)
        return {"y": y, "dx": x.grad, "dW": lin.weight.grad, "db": lin.bias.grad if bias else None}
    return step


def _nce(rng, B, need_dx):
    import torch
    from video_similarity_search_amd.models.infoNCE import HipInfoNCEKernels
    Fw, N = NCE_F, NCE_DIM
    feat = rng.standard_normal((B, Fw))
    w1 = rng.standard_normal((Fw, Fw, 1, 1, 1)) * np.sqrt(2.0 / Fw)
    w2 = rng.standard_normal((N, Fw, 1, 1, 1)) / np.sqrt(Fw)
    b1, b2 = 0.1 * rng.standard_normal(Fw), 0.1 * rng.standard_normal(N)
    dy = rng.standard_normal((B, N))
    feat, w1, b1, w2, b2, dy = (torch.from_numpy(f32(a)).cuda() for a in (feat, w1, b1, w2, b2, dy))
    kern = HipInfoNCEKernels()

    def step():
        y, saved = kern.head_fwd(feat, w1, b1, w2, b2)
        dfeat, gw1, gb1, gw2, gb2 = kern.head_bwd(dy, y, saved, w1, w2, need_dx)
        return {"y": y, "inv": saved[2], "dfeat": dfeat, "dW1": gw1, "db1": gb1, "dW2": gw2, "db2": gb2}
    return step


def _cls(rng, num_classes, mode):
    import torch
    m = _model(dict(CLS_KW, num_classes=num_classes), rng)
    x = torch.from_numpy(f32(rng.standard_normal(CLS_CLIP))).cuda()
    dy = torch.from_numpy(f32(rng.standard_normal((CLS_CLIP[0], num_classes)))).cuda()
    m.train()
    if mode == "probe":                        # tests/test_classifier_gpu.py::_probe_state
        for k, p in m.named_parameters():
            p.requires_grad_(k.startswith("linear"))
        m.eval()
    elif mode == "weight_frozen":
        m.linear.weight.requires_grad_(False)

    def step():
        logits = m(x)
        logits.backward(dy)
        return {"logits": logits, "linear.weight.grad": m.linear.weight.grad, "linear.bias.grad": m.linear.bias.grad,
                "bn1.weight.grad": m.bn1.weight.grad}
    return step


def _proj(rng, frozen):
    import torch
    m = _model(PROJ_KW, rng)
    x = torch.from_numpy(f32(rng.standard_normal(PROJ_CLIP))).cuda()
    dy = torch.from_numpy(f32(rng.standard_normal((PROJ_CLIP[0], PROJ_KW["out_dim"])))).cuda()
    m.train()
    params = dict(m.named_parameters())
    for k in frozen:
        params[k].requires_grad_(False)

    def step():
        emb = m(x)
        emb.backward(dy)
        out = {"emb": emb}
        for k in ("fc1.weight", "fc1.bias", "bn_proj.weight", "bn_proj.bias", "fc2.weight", "fc2.bias", "bn1.weight"):
            out[k + ".grad"] = params[k].grad
        return out
    return step


_BUILD = {"linear": _linear, "nce": _nce, "cls": _cls, "proj": _proj}


def run_case(name):
    """-> {"outputs": {tensor name: {"shape", "sha256"} or None}, "calls": {entry point: count}}"""
    import torch
    kind, params, seed = _CASES[name]
    step = _BUILD[kind](np.random.default_rng(seed), **params)
    torch.cuda.synchronize()
    with counting() as calls:
        out = step()
        torch.cuda.synchronize()
    return {"outputs": {k: digest(v) for k, v in out.items()}, "calls": dict(sorted(calls.items()))}


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    args = sys.argv[1:]
    cases = {name: run_case(name) for name in CASES}
    for name, rec in cases.items():
        print("{:22s} {:2d} tensors, {:4d} calls of {:2d} entry points".format(
            name, sum(v is not None for v in rec["outputs"].values()), sum(rec["calls"].values()), len(rec["calls"])))
    if "--check" in args:
        old = json.load(open(OUT))["cases"]
        bad = [n for n in CASES if cases[n] != old[n]]
        assert not bad, "differs from {}: {}".format(OUT, bad)
        print("every case reproduces", OUT)
        return
    commit = args[args.index("--commit") + 1]
    assert len(commit) == 40, "--commit takes the full 40-digit id"
    path = args[args.index("--out") + 1] if "--out" in args else OUT
    with open(path, "w") as f:
        f.write('{"recorded_from_commit": %s,\n "cases": {\n' % json.dumps(commit))
        f.write(",\n".join("  %s: %s" % (json.dumps(n), json.dumps(rec, sort_keys=True)) for n, rec in cases.items()))
        f.write("\n }}\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

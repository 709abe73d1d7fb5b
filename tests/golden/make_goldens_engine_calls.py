"""Generates tests/golden/engine_entry_sequence.json: the ordered names of the int-returning slic_* entry points one pass of the encoder
ENGINE (the host side, models/resnet.py::_Engine) calls, per case, on a gfx950 device.  A name carries the suffix "@side" when the call's
last argument is the engine's side-stream handle (weight gradients and weight packs go there): the stream a launch goes to is part of the
sequence.  torch's own kernels (copy_, _foreach_add_) are no entry points and are not recorded.  The committed file was recorded from
the resnet.py of the commit it names (the parent of the engine's split into one routine per segment kind); the tree's engine must make
the same calls in the same order on the same streams (tests/test_engine_calls_gpu.py imports the cases from here; the recorder is
make_goldens_kmeans_calls.recording):

    python tests/golden/make_goldens_engine_calls.py --commit ID [--engine FILE]      # writes the file
    python tests/golden/make_goldens_engine_calls.py --check                          # the tree's own engine against the file

--engine FILE loads another revision of resnet.py (`git show ID:video_similarity_search_amd/models/resnet.py > FILE`) as a sibling
module of the package's, so that its relative imports resolve; without it the tree's engine is recorded.

Every case builds a fresh model, runs its pass once unrecorded (plans build their tables on first use) and records the second.  The
first four run on the clip and weights of encoder_tiny.npz ([4, 3, 8, 32, 32], widen 0.125, hidden 64, out 32); the others on drawn
clips and torch's initialisation at the shapes the tests of that configuration use.  The loss is torch arithmetic (no entry point).
    r18_train               R3D-18, shortcut B, no max-pool, training step
    r18_train_unfused       the same with SLIC_BN_FUSE=0
    r18_train_wgrad_main    the same with SLIC_WGRAD_STREAM=0
    r18_train_wgrad_auto    the same with SLIC_WGRAD_STREAM=auto: layer1 on the main stream, the rest on the side
    r18_maxpool_shortcut_a  max-pool behind the stem and shortcut type A
    r50_train               Bottleneck blocks (conv3 path, 1x1x1 downsample with the sparse parity-class hand-over)
    r18_eval_backward       model.eval() with gradients enabled (frozen statistics)
    r18_eval_nograd         eval under no_grad (BatchNorm folded into the epilogues)
    r18_two_views           two forwards, one loss, one backward (two live passes)
    r18_engine_backward     eng.forward(x, True, True) then eng.backward(ctxs, dy): the whole-pass entry
    r18_input_grad_frozen   the clip requires a gradient, every parameter frozen
    r18_no_head             projection_head=False
    cls_finetune            classifier=True, 101 classes (padded to 104), dropout 0.5, training (projection head present: fc1 + statistics)
    cls_probe               classifier=True, everything but `linear` frozen, model.eval(): the probe pass
"""
import contextlib
import ctypes
import importlib.util
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_goldens_kmeans_calls", os.path.join(HERE, "make_goldens_kmeans_calls.py"))
_kc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_kc)
recording = _kc.recording          # the one recorder of both entry-sequence goldens

OUT = os.path.join(HERE, "engine_entry_sequence.json")
TINY = dict(hidden_layer=64, out_dim=32, num_classes=101, n_input_channels=3, shortcut_type='B', conv1_t_size=7, conv1_t_stride=1,
            no_max_pool=True, widen_factor=0.125, projection_head=True, predict_temporal_ds=False, spatio_temporal_attention=False,
            classifier=False, dropout=None)
CLS = dict(TINY, widen_factor=1.0, classifier=True)            # the classifier needs a pooled width of 512: depth 10 at full width
CLIP, CLS_CLIP = (4, 3, 8, 32, 32), (3, 3, 8, 16, 16)
GOLDEN_CASES = ("r18_train", "r18_train_unfused", "r18_train_wgrad_main", "r18_train_wgrad_auto")
# name -> (depth, constructor keywords, environment switches, kind of pass)
_CASES = {
    "r18_train": (18, TINY, {}, "train"),
    "r18_train_unfused": (18, TINY, {"SLIC_BN_FUSE": "0"}, "train"),
    "r18_train_wgrad_main": (18, TINY, {"SLIC_WGRAD_STREAM": "0"}, "train"),
    "r18_train_wgrad_auto": (18, TINY, {"SLIC_WGRAD_STREAM": "auto"}, "train"),
    "r18_maxpool_shortcut_a": (18, dict(TINY, no_max_pool=False, shortcut_type='A'), {}, "train"),
    "r50_train": (50, TINY, {}, "train"),
    "r18_eval_backward": (18, TINY, {}, "eval_backward"),
    "r18_eval_nograd": (18, TINY, {}, "eval_nograd"),
    "r18_two_views": (18, TINY, {}, "two_views"),
    "r18_engine_backward": (18, TINY, {}, "engine_backward"),
    "r18_input_grad_frozen": (18, TINY, {}, "input_grad_frozen"),
    "r18_no_head": (18, dict(TINY, projection_head=False), {}, "train"),
    "cls_finetune": (10, dict(CLS, dropout=0.5), {}, "train"),
    "cls_probe": (10, dict(CLS, projection_head=False), {}, "probe"),
}
CASES = tuple(_CASES)
SWITCHES = {"SLIC_BN_FUSE": "1", "SLIC_WGRAD_STREAM": "1", "SLIC_PROBE": "1"}        # their defaults, unless the case sets them


def build(rn, name):
    """-> (model on the device, clip, step): step() is the case's pass, zero arguments; rn = the resnet module under test"""
    import torch
    depth, kw, _, kind = _CASES[name]
    torch.manual_seed(sum(map(ord, name)))
    with contextlib.redirect_stdout(io.StringIO()):
        m = rn.generate_model(depth, **kw)
    if name in GOLDEN_CASES:
        enc = np.load(os.path.join(HERE, "encoder_tiny.npz"))
        m.load_state_dict({k[3:]: torch.as_tensor(enc[k]) for k in enc.files if k.startswith("sd/")})
        x = torch.from_numpy(enc["x"]).cuda()
    else:
        x = torch.randn(CLS_CLIP if kw["classifier"] else CLIP).cuda()
    assert tuple(x.shape) == (CLS_CLIP if kw["classifier"] else CLIP)
    m = m.cuda().train(kind in ("train", "two_views", "engine_backward", "input_grad_frozen"))
    if kind == "input_grad_frozen":
        for p in m.parameters():
            p.requires_grad_(False)
        x.requires_grad_(True)
    if kind == "probe":
        for k, p in m.named_parameters():
            p.requires_grad_(k.startswith("linear."))

    def step():
        """-> (output, loss or None); the gradients are left in .grad"""
        if kind == "eval_nograd":
            with torch.no_grad():
                return m(x), None
        if kind == "engine_backward":
            eng = m._engine(x)
            with torch.no_grad():
                y, ctxs = eng.forward(x, True, True)
                for p, g in eng.backward(ctxs, torch.ones_like(y)).items():
                    p.grad = g
            return y, None
        y = m(x)
        loss = (y * m(x.flip(0))).sum() if kind == "two_views" else y.square().sum()
        loss.backward()
        return y, loss
    return m, x, step


def run_case(rn, name):
    import torch
    m, x, one_pass = build(rn, name)

    def step():
        one_pass()
        m.zero_grad(set_to_none=True)
        x.grad = None

    def label(n, args):
        s = args[-1] if args else None
        if isinstance(s, ctypes.c_void_p) and s.value is not None:
            for eng in m._engines.values():
                side = getattr(eng, "_side", None)
                if side is not None and side.cuda_stream == s.value:
                    return n + "@side"
        return n
    with recording(dict(SWITCHES, **_CASES[name][2]), label) as seq:
        step()
        torch.cuda.synchronize()
        del seq[:]
        step()
    torch.cuda.synchronize()
    return list(seq)


def load_engine(path, name="_resnet_parent"):
    """another revision of models/resnet.py as a sibling module of the package's own"""
    spec = importlib.util.spec_from_file_location("video_similarity_search_amd.models." + name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    args = sys.argv[1:]
    if "--engine" in args:
        rn = load_engine(args[args.index("--engine") + 1])
    else:
        from video_similarity_search_amd.models import resnet as rn
    seqs = {name: run_case(rn, name) for name in CASES}
    for name, s in seqs.items():
        print("{:24s} {:4d} calls, {:3d} on the side stream".format(name, len(s), sum(n.endswith("@side") for n in s)))
    if "--check" in args:
        old = json.load(open(OUT))["sequences"]
        bad = [n for n in CASES if seqs[n] != old[n]]
        assert not bad, "differs from {}: {}".format(OUT, bad)
        print("every case reproduces", OUT)
    else:
        commit = args[args.index("--commit") + 1]
        assert len(commit) == 40, "--commit takes the full 40-digit id"
        assert any(n.endswith("_wgrad@side") for n in seqs["r18_train"]) and not any(n.endswith("_wgrad@side") for n in seqs["r18_train_wgrad_main"])
        with open(OUT, "w") as f:
            f.write('{"recorded_from_commit": %s,\n "sequences": {\n' % json.dumps(commit))
            f.write(",\n".join("  %s: %s" % (json.dumps(n), json.dumps(s)) for n, s in seqs.items()))
            f.write("\n }}\n")
        print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

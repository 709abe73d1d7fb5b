"""GPU: the gradient with respect to the input clip — slic_conv_stem_dgrad / ConvPlan.input_grad against float64 conv3d autograd,
and x.grad of the encoders (ResNet in train / eval / frozen, with the stem max-pool, R3DNet, several live passes, a non-leaf and
a float64 clip) against the float64 oracle on the device's ReLU branches.

Kernel gate: the forward formula of test_conv_fwd_dgrad_wgrad at the gradient's reduction length,
(2e-6 sqrt(N prod(kernel) / prod(stride)) + 1e-6) max(1, |g|max) — 5e-5 at N = 8.
Model gate (test_tiny_encoder_ragged_sizes_vs_oracle): max-norm relative to the largest entry <= max(1e-3, 3 x the fp32 CPU
oracle's own distance from the fp64 run)."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

import stem_dgrad_cpu_kernels as sk
from test_input_grad_cpu import SHAPES, make_case
from test_encoder_gpu import R3D18_KW, _load_into

pytestmark = pytest.mark.gpu

TINY = dict(R3D18_KW, widen_factor=0.125, hidden_layer=64, out_dim=32)
REFUSED = (3, 16, (3, 5, 3), (1, 1, 1), 1, (3, 9, 11))           # CONV_CASES[2]: not a 7 x 7 / stride-2 stem


# ------------------------------------------------------------------------------------------------ kernel
def _gate(N, kernel, stride, gx):
    return (2e-6 * np.sqrt(N * np.prod(kernel) / np.prod(stride)) + 1e-6) * max(1.0, gx.abs().max().item())


_KCACHE = {}


def _kernel_case(shape, seed):
    """(plan inputs on the device, float64 reference), computed once per shape and left unchanged"""
    if shape not in _KCACHE:
        C, N, kernel, stride, B, dims = shape
        w, dz, gx = make_case(*shape, seed=seed, dtype=torch.float32)
        nd = dz.permute(0, 2, 3, 4, 1).contiguous()
        buf = torch.full((nd.numel() + 128,), float("nan"), dtype=torch.float32, device="cuda")
        view = buf[64:64 + nd.numel()].view(nd.shape)             # the middle of a NaN-filled buffer: a read before or after dz shows
        view.copy_(nd)
        _KCACHE[shape] = (w.cuda().contiguous(), view, gx, buf)
    return _KCACHE[shape]


def _input_grad(shape, wd, dzv):
    from video_similarity_search_amd.models.conv_plan import ConvPlan
    C, N, kernel, stride, B, dims = shape
    plan = ConvPlan(C, N, kernel, stride, tuple(k // 2 for k in kernel), dims, "cuda")
    out = torch.full((B, C) + tuple(dims), float("nan"), dtype=torch.float32, device="cuda")
    got = plan.input_grad(dzv, wd, B, out=out)
    assert got.data_ptr() == out.data_ptr()
    return out.cpu()


@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_kernel_and_fallback_vs_fp64(gpu, monkeypatch, case):
    from video_similarity_search_amd.models import resnet
    shape = SHAPES[case]
    C, N, kernel, stride, B, dims = shape
    wd, dzv, gx, _ = _kernel_case(shape, case)
    tol = _gate(N, kernel, stride, gx)
    c0 = resnet.COUNTS["stem_dgrad"]
    fast = _input_grad(shape, wd, dzv)
    assert resnet.COUNTS["stem_dgrad"] == c0 + 1
    assert not torch.isnan(fast).any(), "an element of dx was not written (or a NaN outside dz was read)"
    e_fast = (fast.double() - gx).abs().max().item()
    monkeypatch.setenv("SLIC_STEM_DGRAD", "0")
    slow = _input_grad(shape, wd, dzv)
    assert resnet.COUNTS["stem_dgrad"] == c0 + 1
    assert not torch.isnan(slow).any()
    e_slow = (slow.double() - gx).abs().max().item()
    e_pair = (fast - slow).abs().max().item()
    print(f"case {case}: fast {e_fast:.3g} fallback {e_slow:.3g} fast-vs-fallback {e_pair:.3g} gate {tol:.3g}")
    assert e_fast <= tol and e_slow <= tol and e_pair <= tol


def test_refused_shape_arrives_through_the_fallback(gpu):
    from video_similarity_search_amd.models import resnet
    from video_similarity_search_amd.models.conv_plan import ConvPlan
    C, N, kernel, stride, B, dims = REFUSED
    wd, dzv, gx, _ = _kernel_case(REFUSED, 17)
    plan = ConvPlan(C, N, kernel, stride, (1, 2, 1), dims, "cuda")
    assert plan.wrun and not plan.stem_dgrad_ok()
    c0 = resnet.COUNTS["stem_dgrad"]
    got = _input_grad(REFUSED, wd, dzv)
    assert resnet.COUNTS["stem_dgrad"] == c0
    assert not torch.isnan(got).any()
    assert (got.double() - gx).abs().max().item() <= _gate(N, kernel, stride, gx)
    with pytest.raises(Exception):
        plan.pack_dgrad(wd)                                       # the W-run plan itself still has no transposed operand


def test_device_packer_equals_numpy_packer(gpu):
    from video_similarity_search_amd._lib import call, ptr, stream
    for C, N, kt in ((3, 8, 7), (2, 16, 3), (4, 64, 5)):
        w = torch.randn(N, C, kt, 7, 7, generator=torch.Generator().manual_seed(kt))
        wp = torch.full((kt * 16 * N * 16,), float("nan"), dtype=torch.float32, device="cuda")
        call("slic_pack_weight_stem_dgrad", ptr(w.cuda()), N, C, kt, ptr(wp), stream())
        ref = sk.device_pack_order(sk.pack_weight(w.double().numpy()))
        assert np.array_equal(wp.cpu().numpy().astype(np.float64), ref)


def test_batch_chunks_equal_single_launch(gpu, monkeypatch):
    from video_similarity_search_amd.models.conv_plan import ConvPlan
    C, N, kernel, stride, B, dims = 3, 8, (7, 7, 7), (1, 2, 2), 16, (2, 6, 7)
    w, dz, gx = make_case(C, N, kernel, stride, B, dims, seed=5, dtype=torch.float32)
    wd, dzd = w.cuda().contiguous(), dz.permute(0, 2, 3, 4, 1).contiguous().cuda()
    plan = ConvPlan(C, N, kernel, stride, (3, 3, 3), dims, "cuda")
    one = plan.input_grad(dzd, wd, B).clone()
    per = max(int(np.prod(plan.src_dims)), int(np.prod(plan.in_dims)), int(np.prod(plan.out_dims))) * max(plan.Cs, plan.N) * 4
    monkeypatch.setenv("SLIC_CONV_MAX_BYTES", str(per * 8 + per // 2))
    assert plan._chunks(B) == [(0, 8), (8, 16)]
    two = plan.input_grad(dzd, wd, B, out=torch.full_like(one, float("nan")))
    assert torch.equal(one, two)
    assert (one.cpu().double() - gx).abs().max().item() <= _gate(N, kernel, stride, gx)


# ------------------------------------------------------------------------------------------------ models
def _masks(eng, xc, training):
    """the branch every ReLU of the HIP encoder takes on clip batch xc in the given mode, as the oracle's relu_masks
    (test_encoder_gpu._gpu_relu_masks, for either mode and for engines of both encoders)"""
    masks = {}

    def ncdhw(t):
        return (t > 0).permute(0, 4, 1, 2, 3).contiguous().cpu()

    with torch.no_grad():
        eng.prepack(with_dgrad=False)
        a = xc
        for si in range(eng.N_SEG):
            a, ctx = eng.seg_forward(si, a, training, True)
            if si == 0:
                masks["stem"] = ncdhw(ctx["a0"])
            elif si <= 4:
                for b, blk in enumerate(ctx["blocks"]):
                    masks[f"layer{si}.{b}.a1"] = ncdhw(blk["a1"])
                    masks[f"layer{si}.{b}"] = ncdhw(blk["out"])
            elif "ah" in ctx:
                masks["head"] = (ctx["ah"] > 0).view(xc.shape[0], -1).cpu()
            del ctx
    torch.cuda.synchronize()
    return masks


def _tiny(seed, **over):
    from oracle import encoder as oe
    from video_similarity_search_amd.models import generate_model
    sd = oe.make_state_dict(np.random.default_rng(seed), widen=0.125, hidden=64, out_dim=32)
    rng = np.random.default_rng(seed + 1)
    for k in list(sd):                                            # non-trivial running statistics for the eval-mode passes
        if k.endswith("running_mean"):
            sd[k] = (0.3 * rng.standard_normal(np.asarray(sd[k]).shape)).astype(np.float32)
        elif k.endswith("running_var"):
            sd[k] = (0.5 + rng.random(np.asarray(sd[k]).shape)).astype(np.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        m = generate_model(18, **dict(TINY, **over))
    _load_into(m, sd)
    return m.cuda(), sd


def _oracle_xgrads(sd, xs, masks, training, loss_of=None, **kw):
    """{dtype: [x.grad per clip batch]} of the oracle on the imposed ReLU branches (one mask set per batch), fp64 and fp32;
    the fp64 run's mask report must be benign"""
    from oracle import encoder as oe
    out = {}
    for dt in (torch.float64, torch.float32):
        t = oe.to_torch(sd, dtype=dt)
        leaves = [x.detach().cpu().to(dt).clone().requires_grad_(True) for x in xs]
        embs = []
        for x, mk in zip(leaves, masks):
            rep = {}
            embs.append(oe.encoder_forward(t, x, training=training, relu_masks=mk, mask_report=rep, **kw))
            if dt == torch.float64:
                print("imposed ReLU branches differ from the fp64 run's own in (elements, of)", oe.assert_masks_benign(rep))
        loss = oe.ntxent_loss(torch.cat(embs)) if loss_of is None else loss_of(embs)
        out[dt] = list(torch.autograd.grad(loss, leaves))
    return out


def _assert_close(got, ref, what):
    g64, g32 = ref
    scale = g64.abs().max().clamp_min(1e-30).item()
    d_gpu = (got.detach().cpu().double() - g64).abs().max().item() / scale
    d_cpu = (g32.double() - g64).abs().max().item() / scale
    print(f"{what}: device {d_gpu:.3g}, fp32 CPU oracle {d_cpu:.3g} of the largest entry")
    assert d_gpu <= max(1e-3, 3 * d_cpu), (what, d_gpu, d_cpu)


def _clip(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).cuda()


@pytest.mark.parametrize("shape", [(3, 3, 9, 36, 44), (2, 3, 8, 32, 32)])
def test_train_mode_clip_gradient_vs_oracle(gpu, shape):
    from video_similarity_search_amd.models import resnet
    from video_similarity_search_amd.loss.triplet_loss import ntxent_loss
    m, sd = _tiny(sum(shape))
    m.train()
    xc = _clip(shape, 7)
    masks = _masks(m._engine(xc), xc, True)
    _load_into(m, sd)
    c0 = resnet.COUNTS["stem_dgrad"]
    x = xc.clone().requires_grad_(True)
    ntxent_loss(m(x)).backward()
    assert resnet.COUNTS["stem_dgrad"] == c0 + 1
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == torch.float32
    ref = _oracle_xgrads(sd, [xc], [masks], True)
    _assert_close(x.grad, (ref[torch.float64][0], ref[torch.float32][0]), f"x.grad {shape}")
    with_x = {k: p.grad.clone() for k, p in m.named_parameters()}
    # the same step without the clip's gradient: no launch, and the parameter gradients are the same bits
    m.zero_grad(set_to_none=True)
    _load_into(m, sd)
    c1 = resnet.COUNTS["stem_dgrad"]
    ntxent_loss(m(xc)).backward()
    assert resnet.COUNTS["stem_dgrad"] == c1
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, with_x[k]), k


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_frozen_encoder_clip_gradient(gpu, mode):
    from video_similarity_search_amd.models import resnet
    from video_similarity_search_amd.loss.triplet_loss import ntxent_loss
    m, sd = _tiny(61)
    for p in m.parameters():
        p.requires_grad_(False)
    training = mode == "train"
    m.train(training)
    xc = _clip((2, 3, 8, 32, 32), 8)
    masks = _masks(m._engine(xc), xc, training)
    _load_into(m, sd)
    c0 = dict(resnet.COUNTS)
    x = xc.clone().requires_grad_(True)
    emb = m(x)                                                    # no exception
    assert emb.requires_grad
    ntxent_loss(emb).backward()
    assert resnet.COUNTS["wgrad"] == c0["wgrad"], "a frozen weight launched a weight gradient"
    assert resnet.COUNTS["stem_dgrad"] == c0["stem_dgrad"] + 1
    assert all(p.grad is None for p in m.parameters())
    ref = _oracle_xgrads(sd, [xc], [masks], training)
    _assert_close(x.grad, (ref[torch.float64][0], ref[torch.float32][0]), f"frozen / {mode}")


def test_stem_max_pool_clip_gradient(gpu):
    from video_similarity_search_amd.loss.triplet_loss import ntxent_loss
    m, sd = _tiny(71, no_max_pool=False)
    m.train()
    # 48 x 48: behind the pool layer4 still has 4 x 1 x 2 x 2 = 16 samples per channel — at (2, 3, 8, 32, 32) its BatchNorm would see
    # two, and the fp32 oracle's own distance (8 % there) would open the gate to anything
    xc = _clip((4, 3, 8, 48, 48), 9)
    masks = _masks(m._engine(xc), xc, True)
    _load_into(m, sd)
    x = xc.clone().requires_grad_(True)
    ntxent_loss(m(x)).backward()
    assert x.grad is not None
    ref = _oracle_xgrads(sd, [xc], [masks], True, max_pool=True)
    _assert_close(x.grad, (ref[torch.float64][0], ref[torch.float32][0]), "max-pool")


def test_r3dnet_eval_clip_gradient(gpu):
    """eval mode: train-mode BatchNorm over 2 samples at 1 x 1 x 1 is ill-posed"""
    from oracle import encoder as oe
    from video_similarity_search_amd.models import R3DNet
    from video_similarity_search_amd.loss.triplet_loss import ntxent_loss
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from r3d_weights import r3d_weights
    raw = r3d_weights(np.random.default_rng(23))
    m = R3DNet(layer_sizes=(1, 1, 1, 1))
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in raw.items()})
    m = m.cuda().eval()
    xc = _clip((2, 3, 4, 32, 32), 10)
    with torch.no_grad():
        m(xc)                                                     # builds the module view and the engine of this shape
    masks = _masks(m._engines[(tuple(xc.shape), str(xc.device))], xc, False)
    x = xc.clone().requires_grad_(True)
    ntxent_loss(m(x)).backward()
    assert x.grad is not None
    ref = _oracle_xgrads(oe.r3d_to_resnet_keys(raw), [xc], [masks], False, projection_head=False)
    _assert_close(x.grad, (ref[torch.float64][0], ref[torch.float32][0]), "R3DNet eval")


def test_two_live_passes_clip_gradients(gpu):
    from video_similarity_search_amd.loss.triplet_loss import ntxent_loss
    m, sd = _tiny(81)
    m.train()
    xcs = [_clip((4, 3, 8, 32, 32), 11), _clip((4, 3, 8, 32, 32), 12)]
    masks = [_masks(m._engine(xc), xc, True) for xc in xcs]
    _load_into(m, sd)
    xs = [xc.clone().requires_grad_(True) for xc in xcs]
    embs = [m(x) for x in xs]                                     # both passes alive: one backward of the summed loss
    (ntxent_loss(embs[0]) + 0.5 * ntxent_loss(embs[1])).backward()
    from oracle import encoder as oe
    ref = _oracle_xgrads(sd, xcs, masks, True, loss_of=lambda e: oe.ntxent_loss(e[0]) + 0.5 * oe.ntxent_loss(e[1]))
    for i, x in enumerate(xs):
        assert x.grad is not None, i
        _assert_close(x.grad, (ref[torch.float64][i], ref[torch.float32][i]), f"pass {i}")


def test_non_leaf_input_and_float64_clip(gpu):
    from video_similarity_search_amd.loss.triplet_loss import ntxent_loss
    m, sd = _tiny(91)
    m.train()
    clip = _clip((2, 3, 8, 32, 32), 13)
    s0 = torch.tensor([1.0, 0.8, 1.2], device="cuda").view(1, 3, 1, 1, 1)
    xc = (clip * s0).detach()
    masks = _masks(m._engine(xc), xc, True)
    _load_into(m, sd)
    # a learnable module in front of the encoder: x = clip * s is no leaf, the gradient must reach s
    s = torch.nn.Parameter(s0.clone())
    ntxent_loss(m(clip * s)).backward()
    assert s.grad is not None and s.grad.shape == s.shape
    ref = _oracle_xgrads(sd, [xc], [masks], True)
    want = tuple((ref[dt][0] * clip.cpu().to(dt)).sum((0, 2, 3, 4)) for dt in (torch.float64, torch.float32))
    _assert_close(s.grad.view(3), want, "s.grad")
    # a float64 clip gets a float64 gradient of its own shape (the values are those of the fp32 pass)
    _load_into(m, sd)
    x64 = xc.double().requires_grad_(True)
    ntxent_loss(m(x64)).backward()
    assert x64.grad is not None and x64.grad.dtype == torch.float64 and x64.grad.shape == x64.shape
    _assert_close(x64.grad, (ref[torch.float64][0], ref[torch.float32][0]), "float64 clip")

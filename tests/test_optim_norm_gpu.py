"""GPU: the norm pass, the fold, the LARS update and the scale launch (csrc/optim.hip) through optim.LARS, optim.clip_grad_norm_ and
optim.grad_norm.

Norms are compared against float64 NumPy norms of the same fp32 values at 2^-23 relative: a double sum of at most 2^21 squares of
fp32 values is exact to far below fp32's half-ulp, and one rounding of the square root then gives at most one ulp.  The inf-norm is
exact.  Updates are gated per quantity by the project's rule (optim_cpu_kernels.gates): 4 x the largest deviation of the float32 CPU
restatement from its float64 run, at least one fp32 half-ulp of the quantity's largest magnitude.  Every figure is printed before it
is asserted."""
import contextlib
import io
import math

import numpy as np
import pytest
import torch

from optim_cpu_kernels import gates, lengths_for, make_data, worst
from optim_norm_cpu_kernels import (LARS_KW, LARS_LRS, clip_reference, lars_groups, lars_quantities, lars_reference, lars_trajectory,
                                    step_grads)

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 8, 1234.5
NORM_GATE = 2.0 ** -23
NORM_TYPES = [2.0, math.inf]


def _so():
    from video_similarity_search_amd import optim as so
    return so


def _report(what, got, gate):
    for key in got:
        print(f"{what}: {key}: worst {got[key]:.3e} gate {gate[key]:.3e}")
    for key in got:
        assert got[key] <= gate[key], (what, key, got[key], gate[key])


@pytest.fixture(scope="module")
def lengths(gpu):
    """1, the n % 4 tails, an item shorter than one float4 pass, exactly one pass, the chunk boundary on both sides, and one tensor whose
    fold covers more items than a workgroup of the norm pass has threads"""
    chunk = gpu.slic_multi_tensor_chunk()
    return lengths_for(chunk, extra=(255, 256, 257)) + [300 * chunk + 3]


@pytest.fixture(scope="module")
def grads32(lengths):
    rng = np.random.default_rng(21)
    return [(0.01 * rng.standard_normal(n)).astype(np.float32) for n in lengths]


def _params_with(grads, scale=1.0):
    ps = [torch.nn.Parameter(torch.zeros(g.size, device="cuda")) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = torch.tensor(g, device="cuda") * scale
    return ps


def _np_norm(a, norm_type):
    a = a.astype(np.float64)
    return float(np.abs(a).max()) if norm_type == math.inf else float(np.sqrt((a * a).sum()))


@pytest.mark.parametrize("norm_type", NORM_TYPES)
def test_norms_against_float64(norm_type, gpu, grads32):
    so = _so()
    ps = _params_with(grads32)
    per = so.grad_norm(ps, norm_type, per_tensor=True)
    total = so.grad_norm(ps, norm_type)
    assert per.shape == (len(ps),) and per.dtype == torch.float32 and per.is_cuda and total.dim() == 0 and total.is_cuda
    want = np.array([_np_norm(g, norm_type) for g in grads32])
    want_total = float(want.max()) if norm_type == math.inf else float(np.sqrt((want * want).sum()))
    rel = np.abs(per.double().cpu().numpy() - want) / want
    rel_total = abs(float(total.double()) - want_total) / want_total
    print(f"norm_type {norm_type}: per tensor worst relative {rel.max():.3e}, total {rel_total:.3e}, gate {NORM_GATE:.3e}")
    if norm_type == math.inf:
        assert rel.max() == 0.0 and rel_total == 0.0
    assert rel.max() <= NORM_GATE and rel_total <= NORM_GATE
    again, again_total = so.grad_norm(ps, norm_type, per_tensor=True), so.grad_norm(ps, norm_type)
    assert torch.equal(again, per) and torch.equal(again_total, total)          # the same bits
    assert all(torch.equal(p.grad.cpu(), torch.tensor(g)) for p, g in zip(ps, grads32))      # read-only


# ---------------------------------------------------------------------------------------------------------------------------------
# LARS

@pytest.fixture(scope="module")
def data(lengths):
    p0, grads = make_data(lengths)
    return p0, step_grads(grads, len(p0))


@pytest.fixture(scope="module")
def lars_refs(data):
    """the definition in torch ops on the CPU, once: (float64 quantities, gates, float64 ratios per step, the ratios' gate)"""
    groups = lars_groups(len(data[0]))
    r64, r32 = lars_reference(*data, groups, torch.float64), lars_reference(*data, groups, torch.float32)
    q64, q32 = r64.pop("ratio"), r32.pop("ratio")
    dev = max(abs(q64[0][i] - q32[0][i]) for i in q64[0])
    qgate = max(4.0 * dev, 0.5 * float(np.spacing(np.float32(max(q64[0].values())))))
    return r64, gates(r64, r32), q64, qgate


def test_lars_ragged_set_five_steps(gpu, data, lars_refs):
    """two groups (one adapt=False, weight_decay=0), fresh gradient allocations every step, a None gradient in step 2, a frozen
    parameter, a late group; the trust ratios the first step's update read"""
    so = _so()
    r64, gate, q64, qgate = lars_refs
    seen = {}

    def ratios(s, opt):
        if s == 0:
            live, q = opt.trust_ratios()
            seen.update({id(p): x for p, x in zip(live, q.double().cpu().tolist())})

    params, opt = lars_trajectory(lambda groups, **kw: so.LARS(groups, lr=LARS_LRS[0], **kw), *data, torch.float32, device="cuda",
                                  after_step=ratios)
    _report("LARS", worst(lars_quantities(params, opt), r64), gate)
    qworst = max(abs(seen[id(params[i])] - q) for i, q in q64[0].items())
    print(f"LARS: ratio after step 1: worst {qworst:.3e} gate {qgate:.3e} over {len(q64[0])} adaptive tensors")
    assert qworst <= qgate


def test_lars_without_adaptation_is_sgd_bit_for_bit(gpu, data):
    so = _so()
    groups = [dict(g, adapt=False) for g in lars_groups(len(data[0]))]
    pa, oa = lars_trajectory(lambda gs, **kw: so.LARS(gs, lr=LARS_LRS[0], **kw), *data, torch.float32, device="cuda", groups=groups)
    pb, ob = lars_trajectory(lambda gs, **kw: so.SGD(gs, lr=LARS_LRS[0], momentum=kw["momentum"], weight_decay=kw["weight_decay"]),
                             *data, torch.float32, device="cuda", groups=groups)
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        assert ("momentum_buffer" in oa.state.get(a, {})) == ("momentum_buffer" in ob.state.get(b, {}))
        if a in oa.state:
            assert torch.equal(oa.state[a]["momentum_buffer"], ob.state[b]["momentum_buffer"])


# ---------------------------------------------------------------------------------------------------------------------------------
# views one element past a 16-byte boundary

def _guarded(arr, shift, flats):
    """a view of `arr`'s values at `shift` elements past a 16-byte boundary inside a flat buffer full of sentinels"""
    n = arr.size
    flat = torch.full((n + 2 * GUARD + 1,), SENTINEL, dtype=torch.float32, device="cuda")
    view = flat[GUARD + shift:GUARD + shift + n]
    view.copy_(torch.tensor(arr, dtype=torch.float32))
    assert view.data_ptr() % 16 == 4 * shift
    flats.append((flat, GUARD + shift, n))
    return view


@pytest.mark.parametrize("which", ["param", "grad", "state"])
def test_one_element_offset_views_keep_their_guards(which, gpu):
    """three LARS steps and one clipping call on tensors 4 bytes past a 16-byte boundary: the element path, nothing read into the
    result from outside the view and nothing written outside it"""
    so = _so()
    chunk = gpu.slic_multi_tensor_chunk()
    lens = [1, 3, 4, 5, 255, 257, chunk + 1]
    rng = np.random.default_rng(11)
    p0 = [0.2 * rng.standard_normal(n) for n in lens]
    grads = [[0.01 * rng.standard_normal(n) for n in lens] for _ in range(3)]
    groups = [dict(idx=list(range(0, len(lens), 2)), lr=LARS_LRS[0]),
              dict(idx=list(range(1, len(lens), 2)), lr=LARS_LRS[1], adapt=False, weight_decay=0)]

    def restated(dtype):
        out = lars_reference(p0, grads, groups, dtype)
        out.pop("ratio")
        total, clipped = clip_reference(grads[2], 0.5 * math.sqrt(sum(float((g * g).sum()) for g in grads[2])), 2.0, dtype)
        out["clipped"] = [c.double().numpy() for c in clipped]
        return out

    r64, r32 = restated(torch.float64), restated(torch.float32)
    flats = []
    place = lambda what, a: _guarded(a, 1 if what == which else 0, flats)
    params = [torch.nn.Parameter(place("param", a)) for a in p0]
    opt = so.LARS([dict(params=[params[i] for i in g["idx"]], **{k: v for k, v in g.items() if k != "idx"}) for g in groups],
                  lr=LARS_LRS[0], **LARS_KW)
    for p in params:                          # a buffer of zeros from the start: momentum * 0 + v is the first step's v
        opt.state[p]["momentum_buffer"] = place("state", np.zeros(p.numel()))
    for s in range(3):
        for p, g in zip(params, grads[s]):
            p.grad = place("grad", g)
        opt.step()
    max_norm = 0.5 * math.sqrt(sum(float((g * g).sum()) for g in grads[2]))
    so.clip_grad_norm_(params, max_norm)
    torch.cuda.synchronize()
    for flat, lo, n in flats:
        assert (flat[:lo] == SENTINEL).all() and (flat[lo + n:] == SENTINEL).all(), "a guard element changed"
    got = lars_quantities(params, opt)
    got["clipped"] = [p.grad.double().cpu().numpy() for p in params]
    _report(f"LARS + clip / {which} shifted", worst(got, r64), gates(r64, r32))


# ---------------------------------------------------------------------------------------------------------------------------------
# clipping

def _cpu_coef(total, max_norm):
    """torch's own fp32 arithmetic on the returned total"""
    return torch.clamp(max_norm / (total.cpu() + 1e-6), max=1.0)


@pytest.mark.parametrize("norm_type", NORM_TYPES)
def test_clipping(norm_type, gpu, grads32):
    so = _so()
    full = _np_norm(np.concatenate(grads32), norm_type)
    # the total is about 10 x max_norm: every gradient is g_in * coef, bit for bit
    max_norm = 0.1 * full
    ps = _params_with(grads32)
    total = so.clip_grad_norm_(ps, max_norm, norm_type)
    assert total.dim() == 0 and total.is_cuda and total.dtype == torch.float32
    rel = abs(float(total.double()) - full) / full
    print(f"clip, norm_type {norm_type}: total relative {rel:.3e} gate {NORM_GATE:.3e}")
    assert rel <= NORM_GATE
    coef = _cpu_coef(total, max_norm)
    assert 0.09 < float(coef) < 0.11
    for p, g in zip(ps, grads32):
        assert torch.equal(p.grad.cpu(), torch.tensor(g) * coef)
    # max_norm above the total: nothing is touched
    ps = _params_with(grads32)
    total = so.clip_grad_norm_(ps, 2.0 * full, norm_type)
    assert abs(float(total.double()) - full) / full <= NORM_GATE
    for p, g in zip(ps, grads32):
        assert torch.equal(p.grad.cpu(), torch.tensor(g))
    # one inf element: the total is inf, that element becomes nan and every other element of every tensor 0, as torch's on the CPU
    ps = _params_with(grads32)
    ps[5].grad[100] = math.inf
    ref = [torch.nn.Parameter(torch.zeros(g.size)) for g in grads32]
    for r, p in zip(ref, ps):
        r.grad = p.grad.cpu().clone()
    want = torch.nn.utils.clip_grad_norm_(ref, max_norm, norm_type)
    total = so.clip_grad_norm_(ps, max_norm, norm_type)
    assert math.isinf(float(total)) and math.isinf(float(want))
    for p, r in zip(ps, ref):
        assert torch.allclose(p.grad.cpu(), r.grad, rtol=0, atol=0, equal_nan=True)
    assert math.isnan(float(ps[5].grad[100])) and float(ps[5].grad.nan_to_num(0.0).abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="non-finite"):
        so.clip_grad_norm_(ps, max_norm, norm_type, error_if_nonfinite=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# a real step

def _tiny():
    from test_train_loop_gpu import TINY
    from video_similarity_search_amd.models import generate_model
    with contextlib.redirect_stdout(io.StringIO()):
        return generate_model(18, **TINY)


def test_real_step_on_the_tiny_encoder(gpu):
    """gradients written by the engine's own backward, clipped to half their norm, then two LARS steps (conv and linear weights adaptive,
    everything one-dimensional not) against the float64 restatement on CPU clones; then one more forward / backward / step"""
    so = _so()
    from video_similarity_search_amd.loss import OnlineTripletLoss
    torch.manual_seed(0)
    m = _tiny().cuda().train()
    x = torch.randn(4, 3, 8, 32, 32, device="cuda")
    labels = torch.arange(2).repeat(2).cuda()
    crit = OnlineTripletLoss(0.2, 'cosine')

    def fwd_bwd():
        loss, _ = crit(m(x), labels, sampling_strategy='noise_contrastive')
        loss.backward()
        return loss

    fwd_bwd()
    live = [p for p in m.parameters() if p.grad is not None]
    assert len(live) > 50
    p0 = [p.detach().cpu().double().numpy().reshape(-1) for p in live]
    g0 = [p.grad.detach().cpu().clone().reshape(-1) for p in live]
    total64 = float(torch.linalg.vector_norm(torch.cat(g0).double()))
    max_norm = 0.5 * total64
    wide = [i for i, p in enumerate(live) if p.dim() > 1]
    flat = [i for i, p in enumerate(live) if p.dim() <= 1]
    assert wide and flat
    groups = [dict(idx=wide, lr=0.1), dict(idx=flat, lr=0.1, adapt=False, weight_decay=0)]

    def restated(dtype):
        _, clipped = clip_reference(g0, max_norm, 2.0, dtype)
        clipped = [c.numpy() for c in clipped]
        out = lars_reference(p0, [clipped, clipped], groups, dtype)
        out.pop("ratio")
        out["clipped"] = [c.astype(np.float64) for c in clipped]
        return out

    r64, r32 = restated(torch.float64), restated(torch.float32)
    total = so.clip_grad_norm_(m.parameters(), max_norm)
    rel = abs(float(total.double()) - total64) / total64
    print(f"tiny encoder: total norm relative {rel:.3e} gate {NORM_GATE:.3e}")
    assert rel <= NORM_GATE
    opt = so.LARS([dict(params=[live[i] for i in wide]), dict(params=[live[i] for i in flat], adapt=False, weight_decay=0)], lr=0.1, **LARS_KW)
    opt.step()
    opt.step()
    got = {"param": [p.detach().double().cpu().numpy().reshape(-1) for p in live],
           "momentum_buffer": [opt.state[p]["momentum_buffer"].double().cpu().numpy().reshape(-1) for p in live],
           "clipped": [p.grad.double().cpu().numpy().reshape(-1) for p in live]}
    _report("tiny encoder, clip and two LARS steps", worst(got, r64), gates(r64, r32))
    opt.zero_grad()
    loss = fwd_bwd()
    so.clip_grad_norm_(m.parameters(), max_norm)
    opt.step()
    assert torch.isfinite(loss).item() and all(torch.isfinite(p).all().item() for p in live)

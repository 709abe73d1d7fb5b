"""CPU: the host side of video_similarity_search_amd.optim (tables, staging ring, upload decisions, torch semantics, state dicts,
errors) through the float64 NumPy provider of tests/optim_cpu_kernels.py, against torch.optim in float64."""
import numpy as np
import pytest
import torch

from optim_cpu_kernels import CASES, STEPS, CpuOptimKernels, lengths_for, make_data, quantities, trajectory, worst

from video_similarity_search_amd import _lib
from video_similarity_search_amd import optim as so

F64 = torch.float64
TOL = 1e-13          # float64 against float64: the same formulas, |values| < 1; only the association of a few products differs


def _ours(kern):
    return (lambda groups, **kw: so.SGD(groups, kernels=kern, **kw)), (lambda groups, **kw: so.Adam(groups, kernels=kern, **kw))


TORCH = (torch.optim.SGD, torch.optim.Adam)


@pytest.fixture(scope="module")
def data():
    return make_data(lengths_for(48))


@pytest.fixture(scope="module")
def torch64(data):
    out = {}
    for case in CASES:
        params, opt = trajectory(case, *TORCH, *data, F64)
        out[case] = (quantities(case, params, opt), opt, params)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_trajectory_matches_torch_float64(case, data, torch64):
    """five steps: a gradient that is None in step 2 only, a requires_grad=False parameter, a parameter added after step 1, per-group
    learning rates, the rate halved between steps 2 and 3 (adam_2g_halved)"""
    kern = CpuOptimKernels()
    params, opt = trajectory(case, *_ours(kern), *data, F64)
    ref, ref_opt, ref_params = torch64[case]
    for key, w in worst(quantities(case, params, opt), ref).items():
        assert w < TOL, (case, key, w)
    assert kern.launches == STEPS                      # one launch per step, whatever the number of groups
    n = len(data[0]) - 3
    if CASES[case]["kind"] == "adam":
        steps = [float(opt.state[p]["step"]) if p in opt.state else None for p in params]
        assert steps == [float(ref_opt.state[p]["step"]) if p in ref_opt.state else None for p in ref_params]
        assert float(opt.state[params[n]]["step"]) == STEPS - 1         # skipped once
        assert float(opt.state[params[n + 2]]["step"]) == STEPS - 1     # joined after step 1
        st = opt.state[params[0]]["step"]
        assert st.device.type == "cpu" and st.dtype == ref_opt.state[next(iter(ref_opt.state))]["step"].dtype
    assert params[n + 1] not in opt.state              # the frozen parameter has no state
    assert np.array_equal(params[n + 1].detach().numpy(), data[0][n + 1])


@pytest.mark.parametrize("case", ["sgd_2g_dampening", "sgd_2g_nesterov", "adam_2g_halved"])
@pytest.mark.parametrize("first", ["ours", "torch"])
def test_state_dict_interchange(case, first, data, torch64):
    """three steps with one implementation, load_state_dict into the other, two more: the five uninterrupted torch steps"""
    kern = CpuOptimKernels()
    a, b = (_ours(kern), TORCH) if first == "ours" else (TORCH, _ours(kern))
    kind = 0 if CASES[case]["kind"] == "sgd" else 1
    params, opt = trajectory(case, *a, *data, F64, swap_at=3, swap_to=b[kind], extras=False)
    ref_params, ref_opt = trajectory(case, *TORCH, *data, F64, extras=False)
    assert type(opt).__module__.startswith("torch") == (first == "ours")
    for key, w in worst(quantities(case, params, opt), quantities(case, ref_params, ref_opt)).items():
        assert w < TOL, (case, key, w)
    if kind == 1:
        n = len(data[0]) - 3
        assert float(opt.state[params[n]]["step"]) == STEPS - 1 and float(opt.state[params[0]]["step"]) == STEPS
    assert sorted(opt.state_dict()["param_groups"][0]) == sorted(ref_opt.state_dict()["param_groups"][0])


def test_closure_and_scheduler():
    kern = CpuOptimKernels()
    w = torch.nn.Parameter(torch.tensor([1.0, -2.0, 3.0], dtype=F64))
    opt = so.SGD([w], lr=0.1, kernels=kern)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    seen = []

    def closure():
        assert torch.is_grad_enabled()
        opt.zero_grad()
        loss = (w * w).sum()
        loss.backward()
        seen.append(loss.item())
        return loss

    with torch.no_grad():
        loss = opt.step(closure)                       # enable_grad around the closure even under no_grad
    assert loss.item() == seen[0] == 14.0
    np.testing.assert_allclose(w.detach().numpy(), [0.8, -1.6, 2.4], rtol=1e-15)
    sched.step()
    opt.step(closure)                                  # lr 0.05 now: read from param_groups at every step
    np.testing.assert_allclose(w.detach().numpy(), [0.72, -1.44, 2.16], rtol=1e-15)


# ---------------------------------------------------------------------------------------------------------------------------------
# tables

def test_chunk_map_covers_every_element_once():
    chunk = _lib.load().slic_multi_tensor_chunk()      # the library's own chunk length: answers without a device
    assert chunk > 0 and chunk % 4 == 0
    lens = lengths_for(chunk) + [1] * 1000
    cmap = so.build_chunk_map(lens, chunk)
    assert cmap.dtype == np.int32 and cmap.shape[1] == 2
    hits = [np.zeros(n, dtype=np.int32) for n in lens]
    for t, c in cmap:
        lo = int(c) * chunk
        assert 0 <= t < len(lens) and 0 <= lo < lens[t]            # an item lies inside ONE tensor
        hits[t][lo:min(lo + chunk, lens[t])] += 1
    assert all((h == 1).all() for h in hits)
    assert cmap.shape[0] == sum(-(-n // chunk) for n in lens) == 1000 + 4 + 1 + 1 + 2 + 3
    with pytest.raises(ValueError):
        so.build_chunk_map([4, 0], chunk)


def test_descriptors_flag_vector_access_only_when_every_pointer_is_aligned():
    base = 0x7F0000001000
    p = [base, base + 4, base, base, base, base + 8]
    g = [base + 64, base + 64, base + 68, base + 64, base + 64, base + 64]
    s1 = [base + 128, base + 128, base + 128, base + 132, base + 128, 0]
    s2 = [base + 256, base + 256, base + 256, base + 256, base + 268, 0]
    d = so.build_descriptors(p, g, s1, s2, [5] * 6, [(0.1, 0.9)] * 6, [0, so.NESTEROV, 0, so.FIRST, so.VEC, 0])
    assert d.dtype.itemsize == 128 and d.nbytes == 6 * 128
    assert [int(f) & so.VEC for f in d["flags"]] == [so.VEC, 0, 0, 0, 0, 0]
    assert [int(f) & ~so.VEC for f in d["flags"]] == [0, so.NESTEROV, 0, so.FIRST, 0, 0]
    assert d["h"][0, 0] == 0.1 and d["h"][0, 1] == 0.9 and (d["h"][:, 2:] == 0).all()      # doubles, not rounded to fp32
    assert list(d["n"]) == [5] * 6 and list(d["s2"]) == s2
    # per item: the flag of the item's tensor
    chunk = 8
    cmap = so.build_chunk_map([5] * 6, chunk)
    for t, c in cmap:
        aligned = all(a % 16 == 0 for a in (p[t], g[t], s1[t], s2[t]))
        assert bool(d["flags"][t] & so.VEC) == aligned


# ---------------------------------------------------------------------------------------------------------------------------------
# uploads and the staging ring

def _model(lens, seed=3):
    rng = np.random.default_rng(seed)
    return [torch.nn.Parameter(torch.tensor(0.2 * rng.standard_normal(n), dtype=F64)) for n in lens]


def test_fresh_gradients_upload_every_step_and_never_rewrite_a_busy_slot():
    """the device runs five steps behind the host: every step's table must survive until its launch runs"""
    lens = lengths_for(48)
    rng = np.random.default_rng(5)
    grads = [[0.01 * rng.standard_normal(n) for n in lens] for _ in range(6)]
    kern = CpuOptimKernels(deferred=True)
    ps, rs = _model(lens), _model(lens)
    opt, ref = so.SGD(ps, lr=0.1, momentum=0.5, kernels=kern), torch.optim.SGD(rs, lr=0.1, momentum=0.5)
    keep = []
    for s in range(5):
        for p, g in zip(ps, grads[s]):
            p.grad = torch.tensor(g, dtype=F64)        # zero_grad(set_to_none=True): a new allocation, a new address
            keep.append(p.grad)
        opt.step()
    assert kern.uploads == 5 and kern.launches == 5 and kern.map_uploads == 1
    assert kern.slots_made == 5                        # nothing was consumed: no slot could be used twice (write() asserts it too)
    assert kern.upload_bytes == 5 * len(lens) * 128    # O(tensors) per step
    kern.drain()
    for s in range(5):
        for p, g in zip(rs, grads[s]):
            p.grad = torch.tensor(g, dtype=F64)
        ref.step()
    for p, r in zip(ps, rs):
        assert (p - r).abs().max().item() < TOL
        assert (opt.state[p]["momentum_buffer"] - ref.state[r]["momentum_buffer"]).abs().max().item() < TOL
    for p, g in zip(ps, grads[5]):
        p.grad = torch.tensor(g, dtype=F64)
    opt.step()
    assert kern.uploads == 6 and kern.slots_made == 5  # consumed slots are used again
    # launch 6 has not run: steps 7 and 8 must leave its slot alone and take consumed ones (write() asserts that none is busy)
    for _ in range(2):
        for p, g in zip(ps, grads[0]):
            p.grad = torch.tensor(g, dtype=F64)
            keep.append(p.grad)
        opt.step()
    assert kern.slots_made == 5 and kern.uploads == 8 and len(kern.queue) == 3
    assert len({id(q[3]) for q in kern.queue}) == 3
    kern.drain()


def test_stable_gradient_views_upload_once():
    lens = lengths_for(48)
    kern = CpuOptimKernels()
    ps, rs = _model(lens), _model(lens)
    flat = torch.zeros(sum(lens), dtype=F64)           # a DDP bucket: gradients are views at 8-byte granularity
    views = list(flat.split(lens))
    opt = so.SGD([dict(params=ps[:4], lr=1e-3), dict(params=ps[4:], lr=1e-4)], lr=1e-3, momentum=0.9, weight_decay=1e-3, kernels=kern)
    ref = torch.optim.SGD([dict(params=rs[:4], lr=1e-3), dict(params=rs[4:], lr=1e-4)], lr=1e-3, momentum=0.9, weight_decay=1e-3)
    rng = np.random.default_rng(6)
    for p, v in zip(ps, views):
        p.grad = v

    def step():
        flat.copy_(torch.tensor(0.01 * rng.standard_normal(flat.numel())))
        for r, v in zip(rs, views):
            r.grad = v.clone()
        opt.step()
        ref.step()

    for _ in range(4):
        step()
    assert kern.uploads == 1 and kern.launches == 4 and kern.map_uploads == 1      # step 2 is not a change either
    for g in opt.param_groups + ref.param_groups:
        g["lr"] = g["lr"] * 0.5
    step()
    step()
    assert kern.uploads == 2 and kern.launches == 6
    opt.zero_grad(set_to_none=False)                   # keeps the views
    step()
    assert kern.uploads == 2
    for p, r in zip(ps, rs):
        assert (p - r).abs().max().item() < TOL


def test_adam_uploads_every_step_one_launch():
    kern = CpuOptimKernels()
    ps = _model([3, 50, 101])
    opt = so.Adam(ps, lr=1e-3, weight_decay=1e-5, kernels=kern)
    for p in ps:
        p.grad = torch.full_like(p, 0.01)
    for _ in range(3):
        opt.step()
    assert kern.launches == 3 and kern.uploads == 3 and kern.map_uploads == 1      # the bias corrections change every step


# ---------------------------------------------------------------------------------------------------------------------------------
# errors: raised with a reason before the provider is entered

def _p(*shape, dtype=torch.float32):
    return torch.nn.Parameter(torch.zeros(*shape, dtype=dtype))


def test_unsupported_options_raise():
    kern = CpuOptimKernels(dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        so.Adam([_p(3)], amsgrad=True, kernels=kern)
    with pytest.raises(NotImplementedError, match="maximize"):
        so.Adam([_p(3)], maximize=True, kernels=kern)
    with pytest.raises(NotImplementedError, match="maximize"):
        so.SGD([_p(3)], lr=0.1, maximize=True, kernels=kern)
    with pytest.raises(ValueError, match="[Nn]esterov"):
        so.SGD([_p(3)], lr=0.1, nesterov=True, kernels=kern)
    for opt, key in ((so.SGD([_p(3)], lr=0.1, kernels=kern), "maximize"), (so.Adam([_p(3)], kernels=kern), "amsgrad"),
                     (so.Adam([_p(3)], kernels=kern), "decoupled_weight_decay")):
        opt.param_groups[0]["params"][0].grad = torch.zeros(3)
        opt.param_groups[0][key] = True                # as a loaded state dict could
        with pytest.raises(NotImplementedError, match=key):
            opt.step()
    assert kern.calls == 0


@pytest.mark.parametrize("cls", [so.SGD, so.Adam])
def test_bad_tensors_raise_before_any_launch(cls):
    kern = CpuOptimKernels(dtype=torch.float32)
    with pytest.raises(TypeError, match="float64"):
        cls([_p(3, dtype=torch.float64)], lr=0.1, kernels=kern)
    with pytest.raises(TypeError, match="float16"):
        cls([_p(3, dtype=torch.float16)], lr=0.1, kernels=kern)
    with pytest.raises(ValueError, match="non-contiguous"):
        cls([torch.nn.Parameter(torch.zeros(4, 6).t())], lr=0.1, kernels=kern)
    with pytest.raises(ValueError, match="more than one device"):
        cls([_p(3), torch.nn.Parameter(torch.zeros(3, device="meta"))], lr=0.1, kernels=kern)
    # the same at step(), for a parameter that add_param_group brought in
    opt = cls([_p(3)], lr=0.1, kernels=kern)
    opt.add_param_group(dict(params=[_p(3, dtype=torch.float64)]))
    for g in opt.param_groups:
        g["params"][0].grad = torch.zeros_like(g["params"][0])
    with pytest.raises(TypeError, match="float64"):
        opt.step()
    # sparse gradient
    emb = torch.nn.Embedding(5, 3, sparse=True)
    opt = cls(emb.parameters(), lr=0.1, kernels=kern)
    emb(torch.tensor([1, 2])).sum().backward()
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()
    assert kern.calls == 0
    if cls is so.Adam:
        assert "step" not in opt.state[emb.weight] or float(opt.state[emb.weight]["step"]) == 0


def test_non_contiguous_gradient_is_copied_for_the_step():
    kern = CpuOptimKernels()
    p, r = _p(4, 6, dtype=F64), _p(4, 6, dtype=F64)
    g = torch.arange(24, dtype=F64).reshape(6, 4).t() * 0.01
    assert not g.is_contiguous()
    p.grad, r.grad = g, g.clone()
    so.SGD([p], lr=0.1, momentum=0.5, kernels=kern).step()
    torch.optim.SGD([r], lr=0.1, momentum=0.5).step()
    assert (p - r).abs().max().item() < TOL and p.grad is g


def test_product_path_needs_the_device():
    """no CPU fallback: fp32 CPU tensors through the default provider raise SlicError"""
    for opt in (so.SGD([_p(5)], lr=0.1, momentum=0.5), so.Adam([_p(5)])):
        opt.param_groups[0]["params"][0].grad = torch.ones(5)
        with pytest.raises(_lib.SlicError):
            opt.step()
    with pytest.raises(_lib.SlicError):
        so.momentum_update([_p(5)], [_p(5)], 0.999)


# ---------------------------------------------------------------------------------------------------------------------------------
# momentum_update

def _net(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(7, 50), torch.nn.BatchNorm1d(50), torch.nn.Linear(50, 3)).double()


def test_momentum_update_matches_the_reference_loop():
    kern = CpuOptimKernels()
    key, query = _net(1), _net(2)
    key[1].running_mean.fill_(0.25)
    m = 0.999
    want = [k.detach().clone() * m + q.detach().clone() * (1. - m) for k, q in zip(key.parameters(), query.parameters())]
    before_q = [q.detach().clone() for q in query.parameters()]
    so.momentum_update(key, query, m, kernels=kern)
    for k, w in zip(key.parameters(), want):
        assert (k - w).abs().max().item() < 1e-15
    assert all(torch.equal(q, b) for q, b in zip(query.parameters(), before_q))
    assert (key[1].running_mean == 0.25).all()         # buffers are not parameters
    so.momentum_update(list(key.parameters()), query.parameters(), m, kernels=kern)        # iterables; stable pointers, same m
    assert kern.launches == 2 and kern.uploads == 1


def test_momentum_update_refuses_mismatched_structures():
    kern = CpuOptimKernels()
    key, query = _net(1), _net(2)
    with pytest.raises(ValueError, match="parameters"):
        so.momentum_update(key, list(query.parameters())[:-1], 0.9, kernels=kern)
    other = torch.nn.Sequential(torch.nn.Linear(7, 50), torch.nn.BatchNorm1d(50), torch.nn.Linear(50, 4)).double()
    with pytest.raises(ValueError, match="key .* against query"):
        so.momentum_update(key, other, 0.9, kernels=kern)
    with pytest.raises(ValueError, match="outside"):
        so.momentum_update(key, query, 1.5, kernels=kern)
    with pytest.raises(TypeError):
        so.momentum_update(key, _net(3).float(), 0.9, kernels=kern)
    assert kern.calls == 0

"""The float64 NumPy provider of tests/optim_cpu_kernels.py grown by the four launches that LARS, clip_grad_norm_ and grad_norm need, and
the plain-torch restatements the CPU and GPU tests of those share.

The provider is driven from the same two tables by address, as its parent is: the norm pass goes item by item of the chunk map into a
partials array [n_items][2], the fold finds a tensor's items by the running sum of ceil(n / chunk) and adds them in item order, the LARS
update reads its ratios and the scale launch its coefficient from the array the fold wrote.  With `deferred=True` the launches queue up
behind one another as the parent's do."""
import math

import numpy as np
import torch

from optim_cpu_kernels import STEPS, CpuOptimKernels, _view

from video_similarity_search_amd import optim as so


def _nanmax(a, b):
    return math.nan if a != a or b != b else max(a, b)


class NormCpuOptimKernels(CpuOptimKernels):
    def new_partials(self, n_items, device):
        self.calls += 1
        return np.zeros((n_items, 2), dtype=np.float64)

    def new_norms(self, n_tensors, device):
        self.calls += 1
        return torch.full((2 + 3 * n_tensors,), math.nan, dtype=torch.float64)

    def _enqueue(self, op, cmap, n_items, slot, n_tensors, upload, extra):
        """what the parent's launch() does, with the operation's own arguments where the parent carries all_first"""
        self.calls += 1
        self.launches += 1
        if upload:
            self.uploads += 1
            self.upload_bytes += n_tensors * so.DESC.itemsize
        slot.pending += 1
        self.queue.append((op, cmap, n_items, slot, n_tensors, upload, extra))
        if not self.deferred:
            self.drain()

    def launch_norm(self, mode, cmap, n_items, slot, n_tensors, upload, partials):
        self._enqueue("norm", cmap, n_items, slot, n_tensors, upload, (mode, partials))

    def launch_fold(self, mode, slot, n_tensors, n_items, partials, max_norm, norms):
        self._enqueue("fold", None, n_items, slot, n_tensors, False, (mode, partials, max_norm, norms))

    def launch_lars(self, cmap, n_items, slot, n_tensors, upload, all_first, norms):
        self._enqueue("lars", cmap, n_items, slot, n_tensors, upload, (all_first, norms))

    def launch_scale(self, cmap, n_items, slot, n_tensors, upload, norms):
        self._enqueue("scale", cmap, n_items, slot, n_tensors, upload, norms)

    def _items(self, cmap, n_items, desc):
        assert cmap.shape == (n_items, 2)
        for item, (t, c) in enumerate(cmap):
            d = desc[t]
            lo = int(c) * self._chunk
            hi = min(lo + self._chunk, int(d["n"]))
            assert 0 <= lo < hi
            yield item, int(t), d, lo, hi

    def _kernel(self, op, cmap, n_items, desc, extra):
        T = desc.shape[0]
        if op == "norm":
            mode, partials = extra
            assert partials.shape == (n_items, 2)
            for item, t, d, lo, hi in self._items(cmap, n_items, desc):
                g = _view(d["g"], lo, hi)
                if mode == "lars":
                    p, wd = _view(d["p"], lo, hi), d["h"][3]
                    u = g + wd * p if wd != 0 else g
                    partials[item] = (p @ p, u @ u)
                else:
                    partials[item] = (0.0, g @ g if mode == "l2" else np.max(np.abs(g)))
        elif op == "fold":
            mode, partials, max_norm, norms = extra
            out, first, tot = norms.numpy(), 0, 0.0
            for t in range(T):
                nch = -(-int(desc[t]["n"]) // self._chunk)
                a0 = a1 = 0.0
                for item in range(first, first + nch):         # in item order
                    a0 += partials[item, 0]
                    a1 = _nanmax(a1, float(partials[item, 1])) if mode == "inf" else a1 + partials[item, 1]
                first += nch
                wn, un = math.sqrt(a0), a1 if mode == "inf" else math.sqrt(a1)
                out[2 + t], out[2 + T + t] = wn, un
                out[2 + 2 * T + t] = desc[t]["h"][2] * wn / un if mode == "lars" and wn > 0 and un > 0 else 1.0
                if mode != "lars":                             # in tensor order
                    tot = _nanmax(tot, a1) if mode == "inf" else tot + a1
            assert first == n_items
            if mode != "lars":
                total = math.sqrt(tot) if mode == "l2" else tot
                x = total + 1e-6
                coef = (1.0 / x if x != 0 else math.inf) * max_norm
                out[0], out[1] = total, 1.0 if coef > 1.0 else coef
        elif op == "lars":
            all_first, norms = extra
            for item, t, d, lo, hi in self._items(cmap, n_items, desc):
                p, g = _view(d["p"], lo, hi), _view(d["g"], lo, hi)
                lr, mom, _, wd = d["h"][:4]
                u = g + wd * p if wd != 0 else g.copy()
                if d["flags"] & so.ADAPT:
                    u = float(norms[2 + 2 * T + t]) * u
                if mom != 0:
                    buf = _view(d["s1"], lo, hi)
                    buf[:] = u if (all_first or d["flags"] & so.FIRST) else mom * buf + u
                    u = buf
                p -= lr * u
        elif op == "scale":
            c = float(extra[1])
            if c >= 1.0:
                return
            for item, t, d, lo, hi in self._items(cmap, n_items, desc):
                g = _view(d["g"], lo, hi)
                with np.errstate(invalid="ignore"):            # inf * 0 is the nan torch makes too
                    g *= c
        else:
            super()._kernel(op, cmap, n_items, desc, extra)


# ---------------------------------------------------------------------------------------------------------------------------------
# LARS: the case the CPU and GPU tests share, and its restatement in plain torch ops

LARS_KW = dict(momentum=0.9, weight_decay=1e-3, trust_coefficient=0.001)
LARS_LRS = (0.1, 0.01)


def lars_groups(n_tensors):
    """the two groups of the ragged-set tests over make_data's tensors (the last three: skip, frozen, late): even positions adaptive,
    odd ones adapt=False and weight_decay=0; `late` joins after step 1 as a group of its own with the defaults.  The frozen tensor is
    listed (it has no gradient in any step)."""
    n = n_tensors - 3
    body = list(range(n)) + [n, n + 1]
    return [dict(idx=body[0::2], lr=LARS_LRS[0]),
            dict(idx=body[1::2], lr=LARS_LRS[1], adapt=False, weight_decay=0),
            dict(idx=[n + 2], lr=0.5 * LARS_LRS[0], from_step=1)]


def step_grads(grads, n_tensors):
    """make_data's gradients as lars_reference takes them: None where the tensor has none in that step (skip in step 2, frozen always)"""
    n = n_tensors - 3
    return [[None if i == n + 1 or (i == n and s == 1) else g for i, g in enumerate(gs)] for s, gs in enumerate(grads)]


def lars_reference(p0, grads, groups, dtype):
    """LARS by its definition in plain torch ops in `dtype`, norms from torch.linalg.vector_norm.
    p0: arrays; grads[step][i]: an array, or None (the tensor is skipped in that step); groups: dicts with `idx` and optionally lr,
    momentum, weight_decay, trust_coefficient, adapt (defaults: LARS_KW, adapt=True) and from_step (the group joins then).
    -> {'param': [arrays], 'momentum_buffer': [arrays of the tensors that have one], 'ratio': [{i: q} per step]}, float64"""
    ps = [torch.tensor(a, dtype=dtype) for a in p0]
    bufs = [None] * len(ps)
    ratios = []
    for s, gs in enumerate(grads):
        r = {}
        for grp in groups:
            if s < grp.get("from_step", 0):
                continue
            kw = {**LARS_KW, "adapt": True, **{k: v for k, v in grp.items() if k not in ("idx", "from_step")}}
            lr, mom, wd, tc = kw["lr"], kw["momentum"], kw["weight_decay"], kw["trust_coefficient"]
            for i in grp["idx"]:
                if gs[i] is None:
                    continue
                w, g = ps[i], torch.tensor(gs[i], dtype=dtype)
                u = g + wd * w if wd != 0 else g
                if kw["adapt"]:
                    wn, un = torch.linalg.vector_norm(w), torch.linalg.vector_norm(u)
                    q = torch.where((wn > 0) & (un > 0), tc * wn / un, torch.ones_like(wn))
                    r[i] = float(q)
                    u = q * u
                if mom != 0:
                    bufs[i] = u.clone() if bufs[i] is None else mom * bufs[i] + u
                    u = bufs[i]
                ps[i] = w - lr * u
        ratios.append(r)
    return {"param": [p.double().numpy() for p in ps], "momentum_buffer": [b.double().numpy() for b in bufs if b is not None],
            "ratio": ratios}


def lars_trajectory(make, p0, grads, dtype, device="cpu", wrap=None, steps=STEPS, groups=None, after_step=None):
    """the steps lars_reference restates (the same p0, grads with their Nones, groups), through an optimizer:
    make(param groups, **LARS_KW) -> (parameters, optimizer).  Gradients are fresh allocations every step.  wrap(i, array) -> the tensor to use for parameter i.  after_step(s, optimizer)."""
    groups = lars_groups(len(p0)) if groups is None else groups
    mk = wrap or (lambda i, a: torch.tensor(a, dtype=dtype, device=device))
    params = [torch.nn.Parameter(mk(i, a)) for i, a in enumerate(p0)]
    sg = grads
    for i in range(len(p0)):
        if all(gs[i] is None for gs in sg):
            params[i].requires_grad_(False)

    def group(grp):
        return dict(params=[params[i] for i in grp["idx"]], **{k: v for k, v in grp.items() if k not in ("idx", "from_step")})

    opt = make([group(grp) for grp in groups if grp.get("from_step", 0) == 0], **LARS_KW)
    keep = []
    for s in range(steps):
        for grp in groups:
            if grp.get("from_step", 0) == s and s > 0:
                opt.add_param_group(group(grp))
        for i, p in enumerate(params):
            if not p.requires_grad:
                continue
            if sg[s][i] is None:
                p.grad = None
                continue
            p.grad = torch.tensor(sg[s][i], dtype=dtype, device=device).reshape(p.shape)
            keep.append(p.grad)
        opt.step()
        if after_step is not None:
            after_step(s, opt)
    return params, opt


def lars_quantities(params, opt):
    return {"param": [p.detach().double().cpu().numpy() for p in params],
            "momentum_buffer": [opt.state[p]["momentum_buffer"].detach().double().cpu().numpy() for p in params
                                if "momentum_buffer" in opt.state.get(p, {})]}


# ---------------------------------------------------------------------------------------------------------------------------------
# clipping

def clip_reference(grads, max_norm, norm_type, dtype):
    """torch.nn.utils.clip_grad_norm_ restated in plain torch ops in `dtype` -> (total norm, the clipped gradients), 0-dim / tensors"""
    gs = [torch.as_tensor(g).to(dtype) for g in grads]
    norms = torch.stack([torch.linalg.vector_norm(g, norm_type) for g in gs])
    total = torch.linalg.vector_norm(norms, norm_type)
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    return total, [g * coef for g in gs]

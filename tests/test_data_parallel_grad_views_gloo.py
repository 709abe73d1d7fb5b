"""CPU over gloo, worlds 1 and 2: misc.distributed_helper.data_parallel hands each parameter's bucket view to the engine, which writes the
weight gradient into it (models/resnet.py: _grad_out).  A view may only be written when nothing else is accumulated into it: once per
backward, and only while the parameter has no .grad.  Every backward pattern of a training loop is run here for several SGD-momentum steps
under data_parallel and under plain DistributedDataParallel on an identical model, and gradients, weights and buffers must be bit-equal:

  one_fwd            one forward, zero_grad() after it (the reference's order): the views must still be written (counted)
  two_fwd            two forwards, one backward (contrastive_train_epoch)
  three_fwd          three forwards, one backward (Tripletnet)
  zero_not_none      zero_grad(set_to_none=False) before the backward
  no_sync            two micro-batches under ddp.no_sync(), then a synced third
  zero_before_fwd    zero_grad() before the forward (the common PyTorch order: nothing is handed over, every gradient is copied)

The encoder needs a GPU, so a stand-in takes its place: a module with `_engines` (what data_parallel looks for) whose one-matrix
autograd.Function routes its weight and bias gradients through the real resnet._grad_out exactly as seg_backward does, followed by a
BatchNorm (flat-buffer path) and a plain Linear.  A further test makes DistributedDataParallel's constructor raise and checks that
data_parallel leaves the model as it found it."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

PATTERNS = ["one_fwd", "two_fwd", "three_fwd", "zero_not_none", "no_sync", "zero_before_fwd"]
STEPS = 5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _MatFn(torch.autograd.Function):
    """y = x W^T + b; the backward writes dW and db where seg_backward writes its weight gradients"""

    @staticmethod
    def forward(ctx, x, w, b, module):
        ctx.save_for_backward(x, w)
        ctx.module = module
        return torch.addmm(b, x, w.t())

    @staticmethod
    def backward(ctx, g):
        from video_similarity_search_amd.models import resnet as rn
        x, w = ctx.saved_tensors
        rn._GRAD_VIEWS[0] = getattr(ctx.module, "_slic_grad_views", None)
        gw, gb = rn._grad_out(w), rn._grad_out(ctx.module.b)
        torch.matmul(g.t(), x, out=gw)
        torch.sum(g, 0, out=gb)
        return g @ w, gw, gb, None


class _Engine(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(8, 6) * 0.5)
        self.b = torch.nn.Parameter(torch.randn(8) * 0.1)
        self._engines = {}

    def forward(self, x):
        return _MatFn.apply(x, self.w, self.b, self)


class _BatchNorm(torch.nn.Module):
    """training-mode BatchNorm whose running statistics are updated outside autograd, as the engine's kernels do (torch's own CPU
    BatchNorm saves them for its backward, so a second forward before the backward trips autograd's version check)"""

    def __init__(self, C):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(C))
        self.bias = torch.nn.Parameter(torch.zeros(C))
        self.register_buffer("running_mean", torch.zeros(C))
        self.register_buffer("running_var", torch.ones(C))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))

    def forward(self, x):
        mean, var = x.mean(0), x.var(0, unbiased=False)
        with torch.no_grad():
            self.running_mean.mul_(0.9).add_(0.1 * mean)
            self.running_var.mul_(0.9).add_(0.1 * var * x.shape[0] / (x.shape[0] - 1))
            self.num_batches_tracked.add_(1)
        return (x - mean) * torch.rsqrt(var + 1e-5) * self.weight + self.bias


def _model():
    torch.manual_seed(5)
    return torch.nn.Sequential(_Engine(), _BatchNorm(8), torch.nn.ReLU(), torch.nn.Linear(8, 4))


def _x(rank, step, k):
    g = torch.Generator().manual_seed(1000 * step + 100 * k + rank)           # every rank, step and pass its own data
    return torch.randn(6, 6, generator=g)


def _loss(*ys):
    # a loss that mixes the passes, so that each pass's gradient depends on the others
    if len(ys) == 1:
        return ys[0].square().mean()
    return sum((a * b).mean() for a, b in zip(ys, ys[1:] + ys[:1])) + ys[0].square().mean()


def _step(pattern, ddp, opt, rank, step):
    """one training step's gradient computation (everything before opt.step())"""
    if pattern == "one_fwd":
        loss = _loss(ddp(_x(rank, step, 0)))
        opt.zero_grad()
        loss.backward()
    elif pattern in ("two_fwd", "three_fwd"):
        ys = [ddp(_x(rank, step, k)) for k in range(2 if pattern == "two_fwd" else 3)]
        loss = _loss(*ys)
        opt.zero_grad()
        loss.backward()
    elif pattern == "zero_not_none":
        loss = _loss(ddp(_x(rank, step, 0)))
        opt.zero_grad(set_to_none=False)
        loss.backward()
    elif pattern == "no_sync":
        with ddp.no_sync():
            loss = _loss(ddp(_x(rank, step, 0)))
            opt.zero_grad()
            loss.backward()
            _loss(ddp(_x(rank, step, 1))).backward()
        _loss(ddp(_x(rank, step, 2))).backward()
    elif pattern == "zero_before_fwd":
        opt.zero_grad()
        _loss(ddp(_x(rank, step, 0))).backward()
    else:
        raise ValueError(pattern)


WRITES = []          # parameters whose gradient _grad_out placed in a handed-over bucket view, in call order


def _count_view_writes():
    from video_similarity_search_amd.models import resnet as rn
    inner = rn._grad_out

    def counted(p):
        gv = rn._GRAD_VIEWS[0]
        v = gv.get(p) if gv else None
        out = inner(p)
        if v is not None and out.untyped_storage().data_ptr() == v.untyped_storage().data_ptr():
            WRITES.append(p)
        return out

    rn._grad_out = counted


def _views_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from video_similarity_search_amd.misc.distributed_helper import data_parallel
    torch.distributed.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    torch.set_num_threads(1)
    _count_view_writes()
    res = {}
    for pattern in PATTERNS:
        ref = _model()
        if rank == 1:                                                   # rank 0's running statistics must win
            ref[1].running_mean.add_(1.0)
        fast = _model()
        fast.load_state_dict(ref.state_dict())
        plain = torch.nn.parallel.DistributedDataParallel(ref)
        wrapped = data_parallel(fast)
        assert wrapped.slic_ddp["flat_buffers"] and wrapped.slic_ddp["buffers_flattened"] == 3
        opt_r = torch.optim.SGD(plain.parameters(), lr=0.1, momentum=0.5)
        opt_f = torch.optim.SGD(wrapped.parameters(), lr=0.1, momentum=0.5)
        grad_bad, weight_bad, buf_bad, worst, written = [], [], [], [], []
        for step in range(STEPS):
            _step(pattern, plain, opt_r, rank, step)
            n0 = len(WRITES)
            _step(pattern, wrapped, opt_f, rank, step)
            written.append(sum(int(p is fast[0].w or p is fast[0].b) for p in WRITES[n0:]))
            g_r = [p.grad for p in ref.parameters()]
            g_f = [p.grad for p in fast.parameters()]
            grad_bad.append(sum(int(not torch.equal(a, b)) for a, b in zip(g_r, g_f)))
            worst.append(max(float((a - b).abs().max()) for a, b in zip(g_r, g_f)))
            opt_r.step()
            opt_f.step()
            weight_bad.append(sum(int(not torch.equal(a, b)) for a, b in zip(ref.parameters(), fast.parameters())))
            buf_bad.append(sum(int(not torch.equal(a, b)) for a, b in zip(ref.buffers(), fast.buffers())))
        res[pattern + "/grad_bad"] = np.array(grad_bad)
        res[pattern + "/weight_bad"] = np.array(weight_bad)
        res[pattern + "/buf_bad"] = np.array(buf_bad)
        res[pattern + "/worst"] = np.array(worst)
        res[pattern + "/written"] = np.array(written)
        res[pattern + "/w"] = fast[0].w.detach().numpy().copy()
        del plain, wrapped
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), **res)
    torch.distributed.destroy_process_group()


@pytest.fixture(scope="module", params=[1, 2], ids=["w1", "w2"])
def views_run(request, tmp_path_factory):
    world = request.param
    out = str(tmp_path_factory.mktemp(f"views_w{world}"))
    mp.spawn(_views_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    return world, [dict(np.load(os.path.join(out, f"r{r}.npz"))) for r in range(world)]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_data_parallel_grad_views_match_plain_ddp(views_run, pattern):
    """every step's gradients, the weights after every SGD-momentum step and the buffers: bit-equal to plain DistributedDataParallel"""
    world, res = views_run
    for rk, r in enumerate(res):
        assert r[pattern + "/grad_bad"].tolist() == [0] * STEPS, (rk, r[pattern + "/worst"].tolist())
        assert r[pattern + "/weight_bad"].tolist() == [0] * STEPS, rk
        assert r[pattern + "/buf_bad"].tolist() == [0] * STEPS, rk
        assert np.array_equal(r[pattern + "/w"], res[0][pattern + "/w"])                # replicas identical
    wr = [r[pattern + "/written"].tolist() for r in res]
    for w in wr:
        # a view is written at most once per parameter and step (two routed parameters)
        assert all(0 <= n <= 2 for n in w), wr
    if pattern == "one_fwd":
        # the reference's order keeps the zero-copy path: nothing is handed over at step 1, and from step 2 on both routed gradients are
        # written into their bucket views
        assert all(w[0] == 0 and w[1:] == [2] * (STEPS - 1) for w in wr), wr
    elif pattern == "zero_before_fwd":
        # .grad is None when the forward runs, so no view is handed over and every gradient is copied (the baseline of a later change)
        assert all(w == [0] * STEPS for w in wr), wr


def _rollback_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from torch.nn.parallel import DistributedDataParallel as DDP
    from video_similarity_search_amd.misc.distributed_helper import data_parallel
    torch.distributed.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    torch.set_num_threads(1)
    m = _model()
    m[1].running_mean.add_(float(rank))                                 # rank 1 starts from different statistics
    m[1].running_var.mul_(1.0 + rank)
    before = [b.clone() for b in m.buffers()]
    orig_init = DDP.__init__

    def failing_init(self, *a, **k):
        raise RuntimeError("construction failed")

    DDP.__init__ = failing_init
    try:
        data_parallel(m)
        raised = False
    except RuntimeError as e:
        raised = "construction failed" in str(e)
    finally:
        DDP.__init__ = orig_init
    ignore_left = bool(getattr(m, "_ddp_params_and_buffers_to_ignore", None)) or any(getattr(b, "_ddp_ignored", False) for b in m.buffers())
    ptrs = [b.untyped_storage().data_ptr() for b in m.buffers()]
    values_kept = all(torch.equal(a, b) for a, b in zip(before, m.buffers()))
    views_left = any(hasattr(mod, "_slic_grad_views") for mod in m.modules())
    # the fallback bench.py takes: plain DistributedDataParallel on the same model must broadcast rank 0's statistics
    ddp = DDP(m)
    ddp(_x(0, 0, 0)).square().mean().backward()                         # the same data on every rank: statistics stay equal
    flat = torch.cat([b.double().reshape(-1) for b in m.buffers()])
    allb = [torch.empty_like(flat) for _ in range(world)]
    torch.distributed.all_gather(allb, flat)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), raised=raised, ignore_left=ignore_left, n_buffers=len(ptrs),
             n_storages=len(set(ptrs)), values_kept=values_kept, views_left=views_left,
             buffers_equal=all(torch.equal(allb[0], b) for b in allb))
    torch.distributed.destroy_process_group()


def test_data_parallel_failure_leaves_model_untouched(tmp_path):
    """DistributedDataParallel's constructor raises inside data_parallel: the error reaches the caller, the ignore list is gone, every
    buffer has storage of its own again with its values kept, and plain DistributedDataParallel on the same model then broadcasts rank 0's
    running statistics (bench.py's fallback)"""
    world = 2
    mp.spawn(_rollback_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for rk in range(world):
        r = dict(np.load(os.path.join(tmp_path, f"r{rk}.npz")))
        assert bool(r["raised"]), rk
        assert not bool(r["ignore_left"]), rk
        assert int(r["n_storages"]) == int(r["n_buffers"]) == 3, rk
        assert bool(r["values_kept"]) and not bool(r["views_left"]), rk
        assert bool(r["buffers_equal"]), rk

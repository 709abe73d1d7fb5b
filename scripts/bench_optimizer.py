"""The optimizer step of the headline model (full-width R3D-18 + projection head) through video_similarity_search_amd.optim (one
multi-tensor launch) against torch.optim on the same device, and momentum_update against the reference's per-parameter loop.

    python scripts/bench_optimizer.py [--reps 30] [--warmup 5] [--out profiles/optimizer.txt]
    python scripts/bench_optimizer.py --only norms --out profiles/optim_norms.txt

Configurations: SGD(lr 0.1, momentum 0.5) (online_train.py:543) and Adam(lr 1e-3, weight_decay 1e-5) (online_train.py:541); torch at
its default (foreach) and at fused=True where the installed torch offers it.  Every variant owns a copy of the parameters; the
gradients are shared and either kept in place (stable pointers: our SGD uploads nothing) or re-allocated before every step as
zero_grad(set_to_none=True) makes them ("fresh": our SGD uploads its 128 bytes per tensor).  The variants alternate inside one
repetition loop, so they share whatever else the machine is doing.  One JSON line per variant:
  gpu_ms / gpu_ms_min    device events around one step whose launches were all enqueued while the stream was held busy by a
                         spin kernel: the device's time for the step, free of the host's enqueue time; median and minimum
  host_us / host_us_min  host clock around the step() call alone (it returns before the device has run anything)
  bytes, hbm_share       bytes the update must move (4 bytes x elements x streams: 5 for momentum SGD, 7 for Adam, 3 for the EMA)
                         over gpu_ms_min, as a share of the 6.29 TB/s a float4 copy reaches on this part
--only norms measures, by the same method, what needs a norm: clip_grad_norm_ (clipping: max_norm = total / 10, the gradients restored
before every call; not clipping: max_norm = 10 x total) against torch.nn.utils.clip_grad_norm_ at its default and at foreach=True,
grad_norm against the same torch call with max_norm=inf, and a LARS step (weights of two and more dimensions adaptive, the rest
adapt=False without decay) against the same update written as torch ops per tensor and against optim.SGD.  Bytes there: one read of
the gradients for a norm, two more streams for the scale only when it clips, 2 + 5 streams for LARS, 5 for SGD.
A machine without a device fails here: nothing is measured on the CPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from video_similarity_search_amd import optim as so  # noqa: E402

HBM_COPY_RATE = 6.29e12
SPIN_CYCLES = 6_000_000            # a few ms: longer than any variant's host time


def clone_params(params):
    return [torch.nn.Parameter(p.detach().clone()) for p in params]


def variants(kind, params):
    """name -> (optimizer, its parameters)"""
    if kind == "sgd":
        tcls, ocls, kw = torch.optim.SGD, so.SGD, dict(lr=0.1, momentum=0.5)
    else:
        tcls, ocls, kw = torch.optim.Adam, so.Adam, dict(lr=1e-3, weight_decay=1e-5)
    out = {}
    ps = clone_params(params)
    out[f"torch.optim.{tcls.__name__} (default)"] = (tcls(ps, **kw), ps)
    try:
        ps = clone_params(params)
        out[f"torch.optim.{tcls.__name__} (fused=True)"] = (tcls(ps, fused=True, **kw), ps)
    except (RuntimeError, TypeError, ValueError) as e:
        print(f"# torch.optim.{tcls.__name__}(fused=True) not offered here: {e}", flush=True)
    ps = clone_params(params)
    out[f"optim.{ocls.__name__}"] = (ocls(ps, **kw), ps)
    return out


def measure(fns, reps, warmup):
    """fns: name -> (prepare, step): prepare runs untimed before every step.  -> name -> (gpu ms list, host us list)"""
    for _ in range(warmup):
        for prep, fn in fns.values():
            prep()
            fn()
    torch.cuda.synchronize()
    res = {name: ([], []) for name in fns}
    for _ in range(reps):
        for name, (prep, fn) in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            prep()
            torch.cuda.synchronize()
            torch.cuda._sleep(SPIN_CYCLES)
            e0.record()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            res[name][0].append(e0.elapsed_time(e1))
            res[name][1].append((t1 - t0) * 1e6)
    return res


def rows_for(what, res, nbytes, extra):
    """nbytes: one figure for every variant, or name -> bytes"""
    rows, per = [], nbytes if isinstance(nbytes, dict) else None
    for name, (gpu, host) in res.items():
        if per is not None:
            nbytes = per[name]
        rows.append(dict(what=what, variant=name, gpu_ms=round(statistics.median(gpu), 4), gpu_ms_min=round(min(gpu), 4),
                         gpu_ms_max=round(max(gpu), 4), host_us=round(statistics.median(host), 1), host_us_min=round(min(host), 1),
                         bytes=int(nbytes), hbm_share=round(nbytes / (min(gpu) * 1e-3) / HBM_COPY_RATE, 3), **extra))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def bench_optimizer(kind, params, grads, fresh, reps, warmup):
    vs = variants(kind, params)
    fns = {}
    for name, (opt, ps) in vs.items():
        def prep(ps=ps):
            if fresh:
                for p, g in zip(ps, grads):
                    p.grad = g.clone()                     # a new allocation at a new address, as after zero_grad(set_to_none=True)
        for p, g in zip(ps, grads):
            p.grad = g
        fns[name] = (prep, opt.step)
    res = measure(fns, reps, warmup)
    n = sum(p.numel() for p in params)
    streams = 5 if kind == "sgd" else 7
    what = f"{kind} step, {'fresh' if fresh else 'stable'} gradient pointers"
    return rows_for(what, res, 4 * n * streams, dict(tensors=len(params), elements=n))


def bench_ema(model, reps, warmup):
    key_a, key_b = clone_params(model.parameters()), clone_params(model.parameters())
    query = list(model.parameters())
    m = 0.999

    def loop():
        with torch.no_grad():
            for k, q in zip(key_a, query):                 # models/infoNCE.py:87-90
                k.data = k.data * m + q.data * (1. - m)

    res = measure({"reference loop (torch ops per parameter)": (lambda: None, loop),
                   "optim.momentum_update": (lambda: None, lambda: so.momentum_update(key_b, query, m))}, reps, warmup)
    n = sum(p.numel() for p in query)
    return rows_for("momentum_update, m = 0.999", res, 4 * n * 3, dict(tensors=len(query), elements=n))


def bench_clip(params, grads, reps, warmup):
    n = sum(p.numel() for p in params)
    total = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads])))
    torch_clip = torch.nn.utils.clip_grad_norm_
    rows = []
    for what, max_norm, streams in (("clip_grad_norm_, clipping (max_norm = total / 10)", 0.1 * total, 3),
                                    ("clip_grad_norm_, not clipping (max_norm = 10 x total)", 10.0 * total, 1),
                                    ("grad_norm (torch: clip_grad_norm_ with max_norm=inf)", float("inf"), 1)):
        fns = {}
        for name, call in (("torch.nn.utils.clip_grad_norm_ (default)", lambda ps: torch_clip(ps, max_norm)),
                           ("torch.nn.utils.clip_grad_norm_ (foreach=True)", lambda ps: torch_clip(ps, max_norm, foreach=True)),
                           ("optim.grad_norm" if max_norm == float("inf") else "optim.clip_grad_norm_",
                            (lambda ps: so.grad_norm(ps)) if max_norm == float("inf") else (lambda ps: so.clip_grad_norm_(ps, max_norm)))):
            ps = clone_params(params)
            for p, g in zip(ps, grads):
                p.grad = g.clone()

            def prep(ps=ps):
                for p, g in zip(ps, grads):                # a clipped gradient no longer clips: every call starts from the same values
                    p.grad.copy_(g)
            fns[name] = (prep, lambda ps=ps, call=call: call(ps))
        rows += rows_for(what, measure(fns, reps, warmup), 4 * n * streams, dict(tensors=len(params), elements=n))
        del fns
        torch.cuda.empty_cache()
    return rows


def bench_lars(params, grads, reps, warmup):
    n = sum(p.numel() for p in params)
    lr, mom, wd, tc = 0.1, 0.9, 1e-6, 1e-3
    adaptive = [p.dim() > 1 for p in params]

    def split(ps):
        return [dict(params=[p for p, a in zip(ps, adaptive) if a]),
                dict(params=[p for p, a in zip(ps, adaptive) if not a], adapt=False, weight_decay=0)]

    ps_t, ps_l, ps_s = clone_params(params), clone_params(params), clone_params(params)
    for ps in (ps_t, ps_l, ps_s):
        for p, g in zip(ps, grads):
            p.grad = g
    bufs = [torch.zeros_like(p) for p in ps_t]
    one = torch.ones((), device=grads[0].device)

    @torch.no_grad()
    def torch_ops():                                       # the float32 restatement of the tests, per tensor
        for p, buf, a in zip(ps_t, bufs, adaptive):
            u = p.grad
            if a:
                u = u + wd * p
                wn, un = torch.linalg.vector_norm(p), torch.linalg.vector_norm(u)
                u = torch.where((wn > 0) & (un > 0), tc * wn / un, one) * u
            buf.mul_(mom).add_(u)
            p.add_(buf, alpha=-lr)

    lars = so.LARS(split(ps_l), lr=lr, momentum=mom, weight_decay=wd, trust_coefficient=tc)
    sgd = so.SGD(ps_s, lr=lr, momentum=mom, weight_decay=wd)
    fns = {"LARS as torch ops per tensor": (lambda: None, torch_ops), "optim.LARS": (lambda: None, lars.step),
           "optim.SGD": (lambda: None, sgd.step)}
    nbytes = {"LARS as torch ops per tensor": 4 * n * 7, "optim.LARS": 4 * n * 7, "optim.SGD": 4 * n * 5}
    return rows_for("LARS step (momentum 0.9), stable gradient pointers", measure(fns, reps, warmup), nbytes,
                    dict(tensors=len(params), adaptive_tensors=sum(adaptive), elements=n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("steps", "norms"), default="steps", help="steps: SGD / Adam / EMA; norms: clip, grad_norm, LARS")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optimizer.py needs a gfx950 device: nothing is measured on the CPU")
    torch.cuda.set_device(0)
    model, _ = bench.build_model()
    model = model.cuda()
    params = [p for p in model.parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)
    print(f"# R3D-18 + projection head: {len(params)} parameter tensors, {n} parameters", flush=True)
    g = torch.Generator(device="cuda").manual_seed(3)
    grads = [1e-3 * torch.randn(p.shape, device="cuda", generator=g) for p in params]
    rows = []
    if a.only == "norms":
        rows += bench_clip(params, grads, a.reps, a.warmup)
        rows += bench_lars(params, grads, a.reps, a.warmup)
    else:
        for kind in ("sgd", "adam"):
            for fresh in (False, True):
                rows += bench_optimizer(kind, params, grads, fresh, a.reps, a.warmup)
                torch.cuda.empty_cache()
        rows += bench_ema(model, a.reps, a.warmup)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# scripts/bench_optimizer.py --only {} --reps {} --warmup {} on {}: {} parameter tensors, {} parameters\n".format(
                a.only, a.reps, a.warmup, torch.cuda.get_device_name(0), len(params), n))
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

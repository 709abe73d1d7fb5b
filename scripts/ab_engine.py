"""The encoder engine (models/resnet.py::_Engine, host code around an unchanged library) against another revision of it, in one process
on one gfx950 device: bits, peak memory and host time (table and verdicts: profiles/engine_segments_refactor.txt):

    git show REV:video_similarity_search_amd/models/resnet.py > resnet_parent.py
    python scripts/ab_engine.py resnet_parent.py REV [OUT.txt]

Three engines: the parent revision, the tree's, and a second copy of the parent (an A/A control: what a condition says about the parent).
  bits    every case of tests/golden/make_goldens_engine_calls.py that has a backward, and the bench configuration (R3D-18, B = 32,
          [3, 16, 112, 112], NT-Xent): one pass from identical weights and clip; output, loss, every parameter gradient, the clip's
          gradient and every buffer (running statistics, counters) afterwards, torch.equal against the parent's.
  memory  torch.cuda.max_memory_allocated() over one bench-configuration step (third step of a fresh model).
  time    the bench configuration's step at B = 32 and at B = 8: the engines alternate, three repeats each, per repeat a fresh model
          and the median of 10 timed steps after 5 warm-up steps; condition per row: median over the repeats <= the parent's median
          + the parent's own spread (its slowest repeat - its fastest)."""
import contextlib
import gc
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_goldens_engine_calls as mg  # noqa: E402
from video_similarity_search_amd import _lib  # noqa: E402
from video_similarity_search_amd.loss import OnlineTripletLoss  # noqa: E402
from video_similarity_search_amd.models import resnet as new_engine  # noqa: E402

R3D18_KW = dict(mg.TINY, widen_factor=1.0, hidden_layer=2048, out_dim=128)         # bench.py's model

ENGINES = (("parent", mg.load_engine(sys.argv[1], "_resnet_parent")), ("new", new_engine),
           ("control", mg.load_engine(sys.argv[1], "_resnet_parent_again")))
OUT = sys.argv[3] if len(sys.argv) > 3 else os.devnull
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


@contextlib.contextmanager
def switches(over):
    old = {k: os.environ.get(k) for k in over}
    os.environ.update(over)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def snapshot(m, x, out, loss):
    snap = {"output": out, "loss": loss, "clip.grad": x.grad}
    snap.update({"grad/" + k: p.grad for k, p in m.named_parameters()})
    snap.update({"buffer/" + k: b for k, b in m.named_buffers()})
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in snap.items() if v is not None}


def bench_model(rn, B):
    """model, clip and step of bench.py's headline at batch B"""
    torch.manual_seed(7)
    with contextlib.redirect_stdout(io.StringIO()):
        m = rn.generate_model(18, **R3D18_KW).cuda().train()
    x = torch.from_numpy(np.random.default_rng(7).standard_normal((B, 3, 16, 112, 112)).astype(np.float32)).cuda()
    labels = torch.arange(B // 2).repeat(2).cuda()
    crit = OnlineTripletLoss(0.2, 'cosine')
    opt = torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.5)

    def step(update=True):
        emb = m(x)
        loss, _ = crit(emb, labels, sampling_strategy='noise_contrastive')
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if update:
            opt.step()
        return emb, loss
    return m, x, step


def one_pass(rn, name):
    if name == "bench_b32":
        m, x, step = bench_model(rn, 32)
        return snapshot(m, x, *step(update=False))
    with switches(dict(mg.SWITCHES, **mg._CASES[name][2])):
        m, x, step = mg.build(rn, name)
        return snapshot(m, x, *step())


def bits():
    say("bits: one pass from identical weights and clip; tensors compared with torch.equal against the parent's")
    for name in [n for n in mg.CASES if mg._CASES[n][3] != "eval_nograd"] + ["bench_b32"]:
        snaps = {who: one_pass(rn, name) for who, rn in ENGINES}
        gc.collect()
        ref = snaps["parent"]
        res = {}
        for who in ("control", "new"):
            assert sorted(snaps[who]) == sorted(ref), (name, who)
            res[who] = [k for k in ref if not torch.equal(snaps[who][k], ref[k])]
        verdict = ("control not deterministic: " + ", ".join(res["control"][:4])) if res["control"] else \
            ("bit-equal" if not res["new"] else "DIFFERS: " + ", ".join(res["new"][:4]))
        say("  {:24s} {:3d} tensors ({} gradients)   control {:3d} differ | new {:3d} differ -> {}".format(
            name, len(ref), sum(k.startswith("grad/") or k == "clip.grad" for k in ref), len(res["control"]), len(res["new"]), verdict))


def fresh():
    """every engine starts from the same allocations: the previous model is collected, and so are the library's grow-only workspaces
    (kept per stream, and every engine has a side stream of its own)"""
    gc.collect()
    _lib._ws_cache.clear()


def memory():
    say("peak memory: torch.cuda.max_memory_allocated() over the third bench-configuration step (B = 32) of a fresh model")
    for who, rn in ENGINES:
        fresh()
        m, x, step = bench_model(rn, 32)
        step()
        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        say("  {:8s} peak {:13d} bytes   (allocated before the step {:13d})".format(who, torch.cuda.max_memory_allocated(), before))
        del m, x, step


def timing(B, warm=5, timed=10):
    res = {who: [] for who, _ in ENGINES}
    for rep in range(3):
        for who, rn in ENGINES:
            # a fresh model per repeat, in the place the previous one left: a model's step time depends on where its tensors lie by more
            # than the engines differ (three models kept alive side by side: a copy of the parent 8 % slower than the parent at B = 8)
            fresh()
            m, x, step = bench_model(rn, B)
            for _ in range(warm):
                step()
            vals = []
            for _ in range(timed):
                torch.cuda.synchronize()
                t0 = time.time()
                step()
                torch.cuda.synchronize()
                vals.append((time.time() - t0) * 1e3)
            res[who].append(statistics.median(vals))
            del m, x, step
    p = res["parent"]
    pm, spread = statistics.median(p), max(p) - min(p)
    for who in ("new", "control"):
        nm = statistics.median(res[who])
        say("  step B = {:2d} [ms]   parent {} med {:.4f} | {:7s} {} med {:.4f} | bound {:.4f} ms -> {}".format(
            B, " ".join("%.4f" % v for v in p), pm, who, " ".join("%.4f" % v for v in res[who]), nm, pm + spread,
            "inside" if nm <= pm + spread else "OUTSIDE"))


def main():
    say("encoder engine: parent (%s) vs the tree's, control = a second copy of the parent" % sys.argv[2])
    say("device: " + torch.cuda.get_device_name(0))
    bits()
    memory()
    say("time: the engines alternate, 3 repeats each; per repeat the median of 10 timed steps of a fresh model (5 warm-up steps before them)")
    say("condition per row: median <= parent median + (parent slowest - parent fastest)")
    timing(32)
    timing(8)
    say("done")


if __name__ == "__main__":
    main()

"""Generates tests/golden/kmeans_entry_sequence.json: the ordered names of the int-returning slic_* entry points one KMeans.fit() calls,
per case, recorded from a k-means DRIVER (the host side, clustering/kmeans_hip.py) on a gfx950 device.  The committed file was recorded
from the driver of the commit it names (the parent of the driver's rewrite into two iteration forms); the rewritten driver must make
the same calls in the same order (tests/test_kmeans_calls_gpu.py imports the cases and the recorder from here):

    python tests/golden/make_goldens_kmeans_calls.py --commit ID [--driver FILE]      # writes the file
    python tests/golden/make_goldens_kmeans_calls.py --check                          # the tree's own driver against the file

--driver FILE loads another revision of kmeans_hip.py (for instance `git show ID:video_similarity_search_amd/clustering/kmeans_hip.py`
saved to a file) as a sibling module of the package's, so that its relative imports resolve; without it the tree's driver is recorded.

Cases (explicit `precision`, so SLIC_KMEANS_BF16 does not move them; rows and inits of the committed kmeans_*.npz goldens):
    a_explicit_fp32     unstructured, explicit init, trace          the fused step, iteration after iteration
    b_explicit_bf16     the same with precision='bf16'              the bf16 image, the bf16 fused step, the bf16 relabelling
    c_relocation        clustered_empty                             relocation, redo of finalize, speculative relaunch
    d_kpp_lockstep      unstructured rows, n_init=3, seed 0         k-means++ of all runs in lock-step, then three Lloyd runs
    e_kpp_run_by_run    SLIC_KPP_BATCH=0, n_init=2                  k-means++ run by run
    f_max_iter_1 / _0   explicit init                               one iteration / none (the plain E-step relabels)
    g_spherical         unit-norm init, spherical=True              row normalisation instead of centring
    sharded_kpp_w1[_bf16]   the k-means++ fit of tests/dist_gpu_worker.py:case_kmeans on a one-rank process group, SLIC_KMEANS_BF16 0 / 1
"""
import contextlib
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "kmeans_entry_sequence.json")
CASES = ("a_explicit_fp32", "b_explicit_bf16", "c_relocation", "d_kpp_lockstep", "e_kpp_run_by_run", "f_max_iter_1", "f_max_iter_0",
         "g_spherical")


def _golden(name):
    return dict(np.load(os.path.join(HERE, f"kmeans_{name}.npz")))


def case(name):
    """-> (KMeans keyword arguments, rows, environment switches)"""
    g = _golden("clustered_empty" if name == "c_relocation" else "unstructured")
    X, init = g["X"], g["init"]
    kw = dict(n_clusters=init.shape[0], init=init, n_init=1, precision="fp32")
    env = {"SLIC_KPP_BATCH": "1"}
    if name in ("a_explicit_fp32", "c_relocation"):
        kw.update(trace=True)
    elif name == "b_explicit_bf16":
        kw.update(trace=True, precision="bf16")
    elif name == "d_kpp_lockstep":
        kw.update(init="k-means++", n_init=3, random_state=0)
    elif name == "e_kpp_run_by_run":
        kw.update(init="k-means++", n_init=2, random_state=0)
        env = {"SLIC_KPP_BATCH": "0"}
    elif name in ("f_max_iter_1", "f_max_iter_0"):
        kw.update(max_iter=int(name[-1]))
    else:
        assert name == "g_spherical", name
        kw.update(init=init / np.linalg.norm(init, axis=1, keepdims=True), spherical=True)
    return kw, X, env


@contextlib.contextmanager
def recording(env=None, label=None):
    """for the duration of the block every int-returning entry point of the loaded library appends its name to the yielded list
    (_lib.call and the direct callers all look the names up on that one library object); `env` is set for the block too.
    label(name, args), when given, returns what is appended instead of the bare name"""
    from video_similarity_search_amd import _lib
    lib = _lib.load()
    seq = []
    orig = {n: getattr(lib, n) for n, (res, _) in _lib.SIGNATURES.items() if res is _lib.c_int}
    old_env = {k: os.environ.get(k) for k in (env or {})}

    def wrapper(n, f):
        def w(*a):
            seq.append(n if label is None else label(n, a))
            return f(*a)
        return w
    try:
        os.environ.update(env or {})
        for n, f in orig.items():
            setattr(lib, n, wrapper(n, f))
        yield seq
    finally:
        for n, f in orig.items():
            setattr(lib, n, f)
        for k, v in old_env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def run_case(KMeans, name):
    import torch
    kw, X, env = case(name)
    with recording(env) as seq:
        KMeans(**kw).fit(torch.from_numpy(X).cuda())
    return list(seq)


def sharded_kpp_fit(KMeans, rank, world):
    """the k-means++ fit of tests/dist_gpu_worker.py:case_kmeans: every rank must pick the same rows of the GLOBAL matrix (needs an
    initialised process group; precision is left to SLIC_KMEANS_BF16, as that fit has always been)"""
    import torch
    X = _golden("d128")["X"]
    per = (len(X) + world - 1) // world
    shard = torch.from_numpy(X[rank * per:(rank + 1) * per]).cuda()
    return KMeans(n_clusters=12, n_init=2, random_state=5, process_group=torch.distributed.group.WORLD).fit(shard)


def sharded_key(world):
    return f"sharded_kpp_w{world}" + ("_bf16" if os.environ.get("SLIC_KMEANS_BF16", "0") == "1" else "")


def load_driver(path):
    """another revision of clustering/kmeans_hip.py as a sibling module of the package's own"""
    spec = importlib.util.spec_from_file_location("video_similarity_search_amd.clustering._kmeans_parent", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def generate(KMeans):
    import torch
    import torch.distributed as dist
    seqs = {name: run_case(KMeans, name) for name in CASES}
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29641", RANK="0", WORLD_SIZE="1")
    dist.init_process_group("nccl")
    torch.cuda.set_device(0)
    try:
        for bf in ("0", "1"):
            with recording({"SLIC_KMEANS_BF16": bf}) as seq:
                key = sharded_key(1)
                sharded_kpp_fit(KMeans, 0, 1)
            seqs[key] = list(seq)
    finally:
        dist.destroy_process_group()
    return seqs


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    args = sys.argv[1:]
    if "--driver" in args:
        KMeans = load_driver(args[args.index("--driver") + 1]).KMeans
    else:
        from video_similarity_search_amd.clustering.kmeans_hip import KMeans
    seqs = generate(KMeans)
    for name, s in seqs.items():
        print("{:20s} {:4d} calls".format(name, len(s)))
    if "--check" in args:
        old = json.load(open(OUT))["sequences"]
        bad = [n for n in CASES if seqs[n] != old[n]]
        assert not bad, "differs from {}: {}".format(OUT, bad)
        print("the unsharded cases reproduce", OUT)
    else:
        commit = args[args.index("--commit") + 1]
        with open(OUT, "w") as f:
            f.write('{"recorded_from_commit": %s,\n "sequences": {\n' % json.dumps(commit))
            f.write(",\n".join("  %s: %s" % (json.dumps(n), json.dumps(s)) for n, s in seqs.items()))
            f.write("\n }}\n")
        print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

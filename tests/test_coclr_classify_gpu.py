"""GPU: slic_segment_mean against float64 and against the reference's own fp32 arithmetic, and coclr_classify's functions end to end
on generate_model(10, classifier=True).

Kernel cases (both modes): C in {5, 51, 101, 400, 513} x pitch in {C, ceil4(C) + 4}; segment lengths {1, 2, 7, 37, 130} as V = 1
each, V = 3 and V = 33 (the lengths in turn); table rows in scrambled order; Gaussian logits, rows with entries at +-80 and at 1e4,
all-equal rows, a -inf beside a finite maximum; a table pre-filled with a NaN canary whose unaddressed rows and pitch columns must
come back bit-identical; two runs bit-equal; ten accumulating calls.

Accuracy gate, per case: the device's error against the float64 mirror (tests/segmean_cpu_kernels.py) is at most 4 x the worst error,
against the same float64, of the reference's fp32 arithmetic on the CPU — torch F.softmax(x, -1).mean(0) per view, stack, .mean(0)
(mode 0: feature.mean(0)) — plus one fp32 ulp of the value.  The factor 4 covers a different, equally valid summation order and a
1-2 ulp expf.  Every case prints both worst errors (run with -s).  Measured on an MI355X (profiles/coclr_classify.txt):
worst absolute error over all single-call cases of a C, device / reference (both pitches give the same figures) —
    mode 1 (probabilities):  C = 5: 7.58e-8 / 9.04e-8,  51: 5.11e-8 / 5.11e-8,  101: 1.25e-7 / 6.56e-8,  400: 1.03e-7 / 4.56e-8,
                             513: 8.15e-8 / 7.29e-8;  ten accumulating calls (C = 513, values near 10): 9.78e-7 / 9.78e-7
    mode 0 (rows, values up to 1e4):  5: 2.92e-4 / 2.92e-4,  51: 3.14e-4 / 2.88e-4,  101: 3.70e-4 / 1.94e-4,  400: 2.72e-4 / 3.09e-4,
                             513: 3.20e-4 / 2.97e-4

Integer outcomes — the rank of every target in the table and the top-1 / top-5 counts (slic_softmax_ce_fwd on the table) — must equal
the float64 mirror outright.  Targets are drawn so that the target's mean probability is at least 1e-3 (relative) away from EVERY
other class (all-equal rows: exact ties on both sides, the index rule decides); the generator is checked on the CPU below and drops
no case.
"""
import contextlib
import copy
import functools
import io
import json
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from segmean_cpu_kernels import segment_mean64, softmax64, target_ranks, topk64      # noqa: E402

ns = types.SimpleNamespace
gpu_test = pytest.mark.gpu
CANARY = 0x7FC0BEEF                       # a quiet NaN with a payload no arithmetic produces
LENGTHS = [1, 2, 7, 37, 130]
CONFIGS = [[n] for n in LENGTHS] + [[130, 1, 37], [LENGTHS[i % 5] for i in range(33)]]
KINDS = ("gauss", "extreme", "equal", "neginf")
KERNEL_CASES = [(mode, C, pitch) for mode in (0, 1) for C in (5, 51, 101, 400, 513) for pitch in ("dense", "pitched")]
MARGIN = 1e-3


def n_views(n):
    """how a segment of n rows splits into equal views for the reference's mean of means"""
    return 10 if n % 10 == 0 else 2 if n % 2 == 0 else 1


def hot_groups(n, G):
    """n rows split into at most G groups of DISTINCT sizes (1, 2, 4, .. and the rest): the rows of a group are one-hot on one class,
    so the classes' mean probabilities are k / n with distinct k — no ties between them for the ranks to hang on"""
    sizes, left, s = [], n, 1
    while left and len(sizes) < G - 1:
        sizes.append(min(s, left))
        left -= sizes[-1]
        s *= 2
    if left:
        sizes.append(left)
    if len(sizes) > 1 and sizes[-1] in sizes[:-1]:
        last = sizes.pop()
        sizes[-1] += last
    assert len(set(sizes)) == len(sizes) and sum(sizes) == n
    return sizes


def draw(kind, R, C, rng, seg_off):
    x = (rng.standard_normal((R, C)) * 3).astype(np.float32)
    if kind == "extreme":                 # softmax -> one-hot, or nearly: +80 / -80 on two classes, or 1e4 on one
        for v in range(len(seg_off) - 1):
            cols = rng.permutation(C)
            r = int(seg_off[v])
            for k, size in enumerate(hot_groups(int(seg_off[v + 1] - seg_off[v]), min(C, 8))):
                for _ in range(size):
                    if r % 2 == 0:
                        x[r, cols[k]], x[r, cols[(k + 1) % C]] = 80.0, -80.0
                    else:
                        x[r, cols[k]] = 1e4
                    r += 1
    elif kind == "equal":
        x[:] = (rng.standard_normal((R, 1)) * 3).astype(np.float32)
    elif kind == "neginf":
        for r in range(R):
            cols = [c for c in rng.choice(C, 2, replace=False) if c != int(np.argmax(x[r]))]
            x[r, cols[0]] = -np.inf
    return x


def choose_targets(p):
    """one target per row of the float64 table p [V, C]: the class nearest the wanted rank (0, 4, 5, 1, last in turn) whose
    probability is a normal fp32 number (>= 1e-36: two one-hot rows of an 'extreme' segment tie at 0.5 to 1e-35, and the classes
    below them sit near 1e-35) and at least MARGIN (relative) away from every other class; rows of exactly equal values take class v % C
    (exact ties on the device too: the index rule decides).  Raises when a row has no such class: no case is dropped."""
    V, C = p.shape
    out = []
    for v in range(V):
        if p[v].max() == p[v].min():
            out.append(v % C)
            continue
        order = np.argsort(-p[v], kind="stable")
        want = (0, 4, 5, 1, C - 1)[v % 5] % C
        for pos in sorted(range(C), key=lambda q: abs(q - want)):
            t = order[pos]
            gap = np.abs(np.delete(p[v], t) - p[v, t])
            if p[v, t] >= 1e-36 and (gap >= MARGIN * np.maximum(np.delete(p[v], t), p[v, t])).all():
                out.append(int(t))
                break
        else:
            raise AssertionError("no class with a margin in row %d" % v)
    return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def kernel_case(mode, C):
    """every (segment configuration, data kind) of one (mode, C), computed once: inputs, the float64 mirror, the reference's fp32
    arithmetic, and (mode 1) targets with their float64 ranks"""
    out = []
    for ci, lens in enumerate(CONFIGS):
        V = len(lens)
        seg_off = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.int64)             # three rows in front belong to no segment
        R = int(seg_off[-1]) + 2                                                           # and two behind
        rows = np.random.default_rng(100 + ci).permutation(V + 3)[:V]                      # scrambled, with unaddressed rows between
        w = [1.0 / n for n in lens]
        for kind in KINDS:
            rng = np.random.default_rng([mode, C, ci, KINDS.index(kind)])
            x = draw(kind, R, C, rng, seg_off)
            f64 = segment_mean64(x, seg_off, rows, w, np.zeros((V + 3, C)), mode, 0)[rows]
            xt = torch.from_numpy(x)
            ref = []
            for v, n in enumerate(lens):
                seg = xt[seg_off[v]:seg_off[v + 1]]
                if mode == 1:
                    ref.append(torch.stack([F.softmax(view, dim=-1).mean(0) for view in seg.view(n_views(n), -1, C)], 0).mean(0))
                else:
                    ref.append(seg.mean(0))
            case = dict(lens=lens, kind=kind, x=x, seg_off=seg_off, rows=rows, w=w, f64=f64, ref32=torch.stack(ref).numpy())
            if mode == 1:
                case["targets"] = choose_targets(f64)
                case["ranks"] = target_ranks(f64, case["targets"])
            out.append(case)
    return out


def gate(dev, f64, ref32):
    """(device's worst error, the reference's worst error, whether every element is inside 4 x that + one fp32 ulp of the value);
    non-finite values must sit in the same places with the same value"""
    fin = np.isfinite(f64)
    same = np.array_equal(np.isfinite(dev), fin) and np.array_equal(dev[~fin].astype(np.float64), f64[~fin], equal_nan=True)
    if not fin.any():
        return 0.0, 0.0, same
    ref_err = np.abs(ref32.astype(np.float64)[fin] - f64[fin]).max()
    err = np.abs(dev.astype(np.float64)[fin] - f64[fin])
    ulp = np.spacing(np.abs(f64[fin]).astype(np.float32)).astype(np.float64)
    return float(err.max()), float(ref_err), bool(same and (err <= 4 * ref_err + ulp).all())


def test_generator_gives_every_case_targets_with_a_margin():
    """CPU: choose_targets finds a class for every table row of every case (it raises otherwise), and the ranks it implies are
    spread over the decisions that matter: first, inside the first five, outside them"""
    seen = set()
    for C in (5, 51, 101, 400, 513):
        cases = kernel_case(1, C)
        assert len(cases) == len(CONFIGS) * len(KINDS)
        for case in cases:
            assert case["targets"].shape == (len(case["lens"]),) and ((case["targets"] >= 0) & (case["targets"] < C)).all()
            p, t = case["f64"], case["targets"]
            if case["kind"] != "equal":
                for v in range(len(t)):
                    others = np.delete(p[v], t[v])
                    assert (np.abs(others - p[v, t[v]]) >= MARGIN * np.maximum(others, p[v, t[v]])).all()
            seen.update(("first" if r == 0 else "five" if r < 5 else "out") for r in case["ranks"])
    assert seen == {"first", "five", "out"}


def run_segments(case, C, ldt, x_dev, mode, calls=1):
    """the table after `calls` calls (the first writes, the others add) as (float32 [T, ldt] on the host, its bits)"""
    from video_similarity_search_amd.coclr_classify import HipClassifyKernels
    K = HipClassifyKernels()
    T = len(case["lens"]) + 3
    table = torch.full((T, ldt), float("nan"), dtype=torch.float32, device="cuda")
    table.view(torch.int32).fill_(CANARY)
    for i in range(calls):
        K.segment_mean(x_dev, case["seg_off"], case["rows"], case["w"], table[:, :C], mode, int(i > 0))
    host = table.cpu()
    return host.numpy(), host.view(torch.int32).numpy(), table


@gpu_test
@pytest.mark.parametrize("mode,C,pitch", KERNEL_CASES)
def test_segment_mean_kernel(gpu, mode, C, pitch):
    from video_similarity_search_amd.coclr_classify import HipClassifyKernels
    ld = C if pitch == "dense" else (C + 3) // 4 * 4 + 4
    worst = [0.0, 0.0]
    for case in kernel_case(mode, C):
        x, rows, V = case["x"], case["rows"], len(case["lens"])
        buf = torch.full((x.shape[0], ld), 7.0, dtype=torch.float32, device="cuda")       # pitch columns that would show in a sum
        buf[:, :C] = torch.from_numpy(x).cuda()
        x_dev = buf[:, :C]
        assert x_dev.stride(0) == ld
        got, bits, table = run_segments(case, C, ld, x_dev, mode)
        # untouched: the rows no segment addresses and the pitch columns of every row
        other = np.setdiff1d(np.arange(V + 3), rows)
        assert (bits[other] == CANARY).all() and (bits[:, C:] == CANARY).all(), (case["lens"], case["kind"])
        dev_err, ref_err, ok = gate(got[rows, :C], case["f64"], case["ref32"])
        print("segment_mean mode %d C %d ld %d lens %s %s: device %.3e reference %.3e" % (
            mode, C, ld, case["lens"] if V < 4 else "33 x", case["kind"], dev_err, ref_err))
        assert ok, (case["lens"], case["kind"], dev_err, ref_err)
        worst = [max(worst[0], dev_err), max(worst[1], ref_err)]
        assert np.array_equal(run_segments(case, C, ld, x_dev, mode)[1], bits), "two runs differ"
        if mode == 1:
            if case["kind"] == "neginf":
                assert (got[rows, :C][~(case["f64"] > 0)] == 0).all()                      # a -inf beside a finite maximum adds exactly 0
            addressed = table[torch.from_numpy(rows).cuda(), :C].contiguous()             # segment v's row, in segment order
            hits = HipClassifyKernels().target_hits(addressed, torch.from_numpy(case["targets"]).cuda()).cpu().numpy()
            assert hits[0] == 0 and np.array_equal(hits[3:], case["ranks"]), (case["lens"], case["kind"], hits[3:], case["ranks"])
            assert hits[1] == (case["ranks"] == 0).sum() and hits[2] == (case["ranks"] < 5).sum()
        if case["lens"] == [130, 1, 37]:
            got10, bits10, _ = run_segments(case, C, ld, x_dev, mode, calls=10)
            ref10 = torch.from_numpy(case["ref32"]).clone()
            for _ in range(9):
                ref10 = ref10 + torch.from_numpy(case["ref32"])
            d10, r10, ok10 = gate(got10[rows, :C], 10 * case["f64"], ref10.numpy())
            print("   ten accumulating calls: device %.3e reference %.3e" % (d10, r10))
            assert ok10 and (bits10[other] == CANARY).all() and (bits10[:, C:] == CANARY).all(), (case["kind"], d10, r10)
            assert np.array_equal(run_segments(case, C, ld, x_dev, mode, calls=10)[1], bits10)
    print("segment_mean mode %d C %d ld %d WORST: device %.3e reference %.3e" % (mode, C, ld, worst[0], worst[1]))


# ---------------------------------------------------------------------------------------------------- end to end

SEQ, IMG, FRAME, NCLS = 8, 32, 40, 21
MODEL_KW = dict(hidden_layer=64, out_dim=32, n_input_channels=3, shortcut_type='B', conv1_t_size=7, conv1_t_stride=1, no_max_pool=True,
                widen_factor=1.0, projection_head=False, classifier=True, num_classes=NCLS)


def new_model(seed):
    from video_similarity_search_amd.models import generate_model
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        m = generate_model(10, **MODEL_KW)
    torch.nn.init.normal_(m.linear.weight, mean=0.0, std=0.05)
    return m.cuda()


class Videos(object):
    def __init__(self, S_list, seed):
        rng = np.random.default_rng(seed)
        self.clips = [torch.from_numpy(rng.integers(0, 256, (S * SEQ, FRAME, FRAME, 3), dtype=np.uint8)) for S in S_list]
        self.targets = [int(t) for t in rng.integers(0, 4, len(S_list))]
        self.names = ['cls%d/v_%03d/frames' % (t, i) for i, t in enumerate(self.targets)]

    def __len__(self):
        return len(self.clips)

    def __getitem__(self, i):
        return self.clips[i], (self.targets[i], self.names[i])


class Subset(object):
    def __init__(self, data, keep):
        self.data, self.keep = data, list(keep)

    def __len__(self):
        return len(self.keep)

    def __getitem__(self, i):
        return self.data[self.keep[i]]


class Recorder(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net, self.outputs = net, []

    def forward(self, x):
        y = self.net(x)
        self.outputs.append(y.detach().clone())
        return y


def normalise5():
    from video_similarity_search_amd.coclr_utils import transforms as T
    return T.Compose([T.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], channel=1)])


def view_clips(video, chain, tf):
    """the reference's per-view pass for one video: its S clips [S, 3, SEQ, IMG, IMG] under one chain"""
    S = video.shape[0] // SEQ
    return tf(chain(video.cuda())[None]).view(3, S, 1, SEQ, IMG, IMG).permute(1, 2, 0, 3, 4, 5).squeeze(1).contiguous()


@gpu_test
def test_test_10crop_packed_against_ten_passes(gpu, tmp_path, capsys):
    """the packed protocol against the reference's shape — ten passes, a forward per video, float64 softmax / mean of the device
    logits.  delta = the largest difference between a clip's logits in its per-video batch and in the packed batch (batch-size
    dependent kernels: existing behaviour on both sides); the mean probabilities may differ by delta / 2 (the Jacobian of softmax has
    infinity-norm <= 1/2) plus the kernel gate; counts are compared on the videos whose margin exceeds that.
    Measured on an MI355X: delta 4.0e-7; device against the ten passes 2.1e-8 / 1.1e-8 / 8.2e-9 (center / five / ten), the fp32
    reference on the packed logits against float64 7.6e-9 / 6.8e-9 / 7.6e-9."""
    from video_similarity_search_amd import coclr_classify as cc
    from video_similarity_search_amd.coclr_utils import transforms as T
    S_list = [1, 2, 3, 3, 2, 1]
    data = Videos(S_list, 31)
    model = new_model(32).eval()
    tf = normalise5()
    chains = T.ten_crop_views(IMG, IMG)
    with torch.no_grad():
        alone = [[model(view_clips(v, chains[n], tf)).double().cpu().numpy() for v in data.clips] for n in range(10)]      # [view][video] -> [S, C]
    ref = {t: np.stack([np.mean([softmax64(alone[n][i]).mean(0) for n in range(nv)], axis=0) for i in range(len(S_list))])
           for t, nv in cc.TITLES}
    # targets: per video the class with the widest margin over the three tables
    marg =np.array([[min(np.min(np.abs(np.delete(ref[t][i], c) - ref[t][i][c])) for t, _ in cc.TITLES) for c in range(NCLS)]
                     for i in range(len(S_list))])
    order = np.argsort(-ref['ten'], axis=1, kind="stable")
    data.targets = []
    for i in range(len(S_list)):
        cand = order[i][[0, 3, 6][i % 3]:][:6]            # near rank 0 / 3 / 6 of the ten-crop table: hits and misses of both kinds
        data.targets.append(int(cand[np.argmax(marg[i][cand])]))

    rec = Recorder(model)
    args = ns(num_seq=1, seq_len=SEQ, img_dim=IMG, crop_size=IMG, clips_per_forward=16, ten_crop=True,
              checkpoint_path=str(tmp_path / "epoch3.pth.tar"))
    K = cc.HipClassifyKernels()
    res = cc.test_10crop(data, rec, None, tf, "cuda", 3, args, kernels=K)
    assert list(res) == ['center', 'five', 'ten'] and K.reads == 3
    total = 10 * sum(S_list)
    assert [o.shape[0] for o in rec.outputs] == [16] * (total // 16) + ([total % 16] if total % 16 else [])
    packed = torch.cat(rec.outputs).double().cpu().numpy()
    base = np.concatenate([[0], np.cumsum([10 * S for S in S_list])])
    delta = max(np.abs(packed[base[i] + n * S:base[i] + (n + 1) * S] - alone[n][i]).max() for i, S in enumerate(S_list) for n in range(10))
    packed32 = torch.cat(rec.outputs).float().cpu()
    for t, nv in cc.TITLES:
        f64 = np.stack([softmax64(packed[base[i]:base[i] + nv * S]).mean(0) for i, S in enumerate(S_list)])
        r32 = torch.stack([torch.stack([F.softmax(packed32[base[i] + n * S:base[i] + (n + 1) * S], dim=-1).mean(0) for n in range(nv)]).mean(0)
                           for i, S in enumerate(S_list)]).numpy()
        ref_err = np.abs(r32.astype(np.float64) - f64).max()
        stat = json.load(open(args.checkpoint_path + '-prob-%s.json' % t))
        dev = np.array([stat[v]['mean_prob'][0] for v in data.names])
        bound = delta / 2 + 4 * ref_err + np.spacing(ref[t].astype(np.float32)).astype(np.float64)
        err = np.abs(dev - ref[t])
        with capsys.disabled():
            print("test_10crop %s: delta %.3e, device vs ten passes %.3e, fp32 reference on the packed logits %.3e" % (t, delta, err.max(), ref_err))
        assert (err <= bound).all(), (t, err.max(), delta, ref_err)
        sure = [marg[i][data.targets[i]] > 2 * bound[i].max() for i in range(len(S_list))]
        rank = target_ranks(ref[t], data.targets)
        for k, got in ((1, res[t][0]), (5, res[t][1])):
            lo = sum(1 for i in range(len(S_list)) if sure[i] and rank[i] < k)
            hi = lo + sum(1 for s in sure if not s)
            assert lo <= round(got * len(S_list)) <= hi and abs(got * len(S_list) - round(got * len(S_list))) < 1e-9, (t, k, got, lo, hi)
        assert sum(sure) >= len(S_list) // 2, "the generator's margins do not exceed the bound: %r" % (sure,)
    out = capsys.readouterr().out
    assert out.count('-crop result:\nMean: Acc@1: ') == 3


@gpu_test
def test_test_retrieval_against_float64_sort(gpu, tmp_path, capsys):
    """features of 60 train and 6 test videos -> centring, normalising and a full sort in float64 on the saved features.  The train
    set is cut to 56 videos for which every test video's k-th and (k + 1)-th similarities, k in {1, 5, 10, 20, 50}, differ by more
    than 1e-4 (searched with 2e-4 on the first run's features, verified on the second's): the hits must then be equal."""
    from video_similarity_search_amd import coclr_classify as cc
    rng = np.random.default_rng(41)
    pool = Videos([int(s) for s in rng.choice([1, 2, 3], 60)], 42)
    test = Videos([1, 2, 3, 3, 2, 1], 43)
    model = new_model(44).eval()
    tf = normalise5()
    args = ns(num_seq=1, seq_len=SEQ, img_dim=IMG, crop_size=IMG, clips_per_forward=32, checkpoint_path=str(tmp_path / "ck.pth.tar"),
              dataset='hmdb51', dirname='pool')

    def gaps_and_hits(ftest, ftrain, ytest, ytrain):
        q, g = ftest.astype(np.float64), ftrain.astype(np.float64)
        q, g = q - q.mean(0), g - g.mean(0)
        q, g = q / np.linalg.norm(q, axis=1, keepdims=True), g / np.linalg.norm(g, axis=1, keepdims=True)
        sim = -np.sort(-(q @ g.T), axis=1)
        gap = min((sim[:, k - 1] - sim[:, k]).min() for k in cc.RETRIEVAL_KS if k < sim.shape[1])
        idx = topk64(q, g, 50)
        hit = np.asarray(ytrain)[idx] == np.asarray(ytest)[:, None]
        return gap, [int(hit[:, :k].any(1).sum()) for k in cc.RETRIEVAL_KS]

    cc.test_retrieval(model, None, tf, "cuda", 0, args, train_dataset=pool, test_dataset=test)
    root = tmp_path / "pool"
    ftest = torch.load(root / 'hmdb51_test_feature.pth.tar').cpu().numpy()
    ftrain = torch.load(root / 'hmdb51_train_feature.pth.tar').cpu().numpy()
    assert ftest.shape == (6, NCLS) and ftrain.shape == (60, NCLS) and not os.path.exists(root / 'hmdb51_sim.pth.tar')
    for start in range(0, 57):
        keep = [i for i in range(60) if not start <= i < start + 4]
        if gaps_and_hits(ftest, ftrain[keep], test.targets, [pool.targets[i] for i in keep])[0] > 2e-4:
            break
    else:
        raise AssertionError("no train subset separates the k-th from the (k + 1)-th neighbour")

    args.dirname = 'cut'
    K = cc.HipClassifyKernels()
    capsys.readouterr()
    acc = cc.test_retrieval(model, None, tf, "cuda", 0, args, train_dataset=Subset(pool, keep), test_dataset=test, kernels=K)
    out = capsys.readouterr().out
    root = tmp_path / "cut"
    ftest2 = torch.load(root / 'hmdb51_test_feature.pth.tar').cpu().numpy()
    ftrain2 = torch.load(root / 'hmdb51_train_feature.pth.tar').cpu().numpy()
    assert torch.load(root / 'hmdb51_train_label.pth.tar').tolist() == [pool.targets[i] for i in keep]
    gap, hits = gaps_and_hits(ftest2, ftrain2, test.targets, [pool.targets[i] for i in keep])
    print("test_retrieval: smallest gap between the k-th and (k + 1)-th similarity %.3e, hits %s" % (gap, hits))
    assert gap > 1e-4
    assert acc == [float(np.float32(h) / np.float32(6)) for h in hits] and K.reads == 1
    assert out.splitlines()[-5:] == ['%dNN acc = %.4f' % (k, a) for k, a in zip(cc.RETRIEVAL_KS, acc)]
    # the features are the per-video means of the model's outputs (checked on the test videos, a forward per video)
    from video_similarity_search_amd.coclr_utils import transforms as T
    centre = T.ten_crop_views(IMG, IMG)[0]
    with torch.no_grad():
        want = np.stack([model(view_clips(v, centre, tf)).double().cpu().numpy().mean(0) for v in test.clips])
    np.testing.assert_allclose(ftest2, want, rtol=0, atol=1e-4 * max(1.0, np.abs(want).max()))


def epoch_batches(sizes, seed):
    rng = np.random.default_rng(seed)
    return [(torch.from_numpy(rng.standard_normal((b, 3, SEQ, IMG, IMG)).astype(np.float32)),
             torch.from_numpy(rng.integers(0, NCLS, b).astype(np.int64))) for b in sizes]


@gpu_test
@pytest.mark.parametrize("train_what", ["last", "ft"])
def test_train_one_epoch_against_the_literal_loop(gpu, capsys, train_what):
    """4 steps on the probe path (train_what 'last': eval mode, only `linear` trains) and on the fine-tune path against the
    reference's loop written out — three .item() per step — on a deep copy: the same kernels in the same order, only the read-back
    moved.  Returned averages equal to 1e-6 relative; parameters and buffers bit-equal after the epoch."""
    from video_similarity_search_amd import coclr_classify as cc
    from video_similarity_search_amd import optim
    from video_similarity_search_amd.coclr_utils import transforms as T
    from video_similarity_search_amd.coclr_utils.utils import AverageMeter
    from video_similarity_search_amd.loss import CrossEntropyLoss, calc_topk_accuracy
    from video_similarity_search_amd.models.resnet import COUNTS
    model = new_model(51)
    if train_what == 'last':
        for name, p in model.named_parameters():
            if 'linear' not in name:
                p.requires_grad = False
    ref = copy.deepcopy(model)
    loader = epoch_batches((4, 4, 4, 3), 52)
    tf = T.Compose([T.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], channel=1)])

    def opt(m):
        return optim.SGD([p for p in m.parameters() if p.requires_grad], lr=0.01, momentum=0.9, weight_decay=1e-3)

    # the reference's loop
    crit, o = CrossEntropyLoss(), opt(ref)
    ref.eval() if train_what == 'last' else ref.train()
    losses, top1_meter = AverageMeter('Loss', ':.4f'), AverageMeter('acc@1', ':.4f')
    for x, y in loader:
        B = x.size(0)
        x, y = x.cuda(), y.cuda()
        logit = ref(tf(x).view(B, 3, 1, SEQ, IMG, IMG).transpose(1, 2).contiguous().squeeze(1))
        loss = crit(logit, y)
        top1, top5 = calc_topk_accuracy(logit, y, (1, 5))
        losses.update(loss.item(), B)
        top1_meter.update(top1.item(), B)
        o.zero_grad()
        loss.backward()
        o.step()

    K = cc.HipClassifyKernels()
    probes = COUNTS["probe_pass"]
    args = ns(train_what=train_what, final_bn=False, print_freq=2, num_seq=1, seq_len=SEQ, img_dim=IMG, iteration=1)
    got = cc.train_one_epoch(loader, model, CrossEntropyLoss(), opt(model), tf, "cuda", 0, args, kernels=K)
    assert model.training == (train_what != 'last') and COUNTS["probe_pass"] - probes == (4 if train_what == 'last' else 0)
    assert K.reads == 3                                   # progress lines after steps 0 and 2, the rest at the end
    assert got[0] == pytest.approx(losses.avg, rel=1e-6) and got[1] == pytest.approx(top1_meter.avg, rel=1e-6, abs=1e-12)
    for (n, p), (_, q) in zip(model.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(p, q), n
    assert capsys.readouterr().out.count('Epoch:[0]') == 2


@gpu_test
def test_validate_one_read_back(gpu, capsys):
    from video_similarity_search_amd import coclr_classify as cc
    from video_similarity_search_amd.coclr_utils import transforms as T
    from video_similarity_search_amd.loss import CrossEntropyLoss
    model = new_model(61)
    loader = epoch_batches((4, 3), 62)
    tf = T.Compose([T.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], channel=1)])
    K = cc.HipClassifyKernels()
    loss, top1 = cc.validate(loader, model, CrossEntropyLoss(), tf, "cuda", 5, ns(num_seq=1, seq_len=SEQ, img_dim=IMG), kernels=K)
    crit, tot, hit = CrossEntropyLoss(), 0.0, 0
    with torch.no_grad():
        for x, y in loader:
            logit = model(tf(x.cuda()))
            tot += crit(logit, y.cuda()).item() * x.shape[0]
            hit += int((logit.argmax(1).cpu() == y).sum())
    assert K.reads == 1 and not model.training
    assert loss == pytest.approx(tot / 7, rel=1e-6) and top1 == pytest.approx(hit / 7, rel=1e-6, abs=1e-12)
    assert capsys.readouterr().out.startswith('Epoch: [5]\tLoss: %.4f Acc@1: %.4f' % (loss, top1))

"""CPU: the host logic of coclr_classify — the meter arithmetic and print cadence of train_one_epoch / validate against a literal
per-step loop, one read-back per interval, the view-major packing of test_10crop (a video split across forwards), its three tables,
summarize_probability's file, test_retrieval's files and cache, and the argument rules of slic_segment_mean (host checks: they
answer without a device) — driven with the NumPy provider of tests/segmean_cpu_kernels.py and a Flatten + Linear stand-in model.
The same functions on the HIP kernels: tests/test_coclr_classify_gpu.py."""
import copy
import ctypes
import json
import os
import pickle
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ns = types.SimpleNamespace
L, HW, C = 2, 4, 7                       # frames per window, frame side, classes


class Loader(list):
    pass


class Log(object):
    def __init__(self):
        self.lines = []

    def log(self, s):
        self.lines.append(s)


class Plotter(object):
    def __init__(self):
        self.data = []

    def add_data(self, tag, value, step):
        self.data.append((tag, float(value), step))


def stand_in(n_in, n_out, seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(n_in, n_out))


def batches(sizes, seed):
    rng = np.random.default_rng(seed)
    ld = Loader()
    for b in sizes:
        ld.append((torch.from_numpy(rng.standard_normal((b, 3, L, HW, HW)).astype(np.float32)),
                   torch.from_numpy(rng.integers(0, C, b).astype(np.int64))))
    return ld


def scale(x):
    return x * 0.5 + 0.25


def epoch_args(**kw):
    return ns(train_what='ft', final_bn=False, print_freq=3, num_seq=1, seq_len=L, img_dim=HW, iteration=11, **kw)


def ref_topk(logit, target, ks):
    """coclr_utils/utils.py's calc_topk_accuracy, in the test's own words: the share of rows whose target is among the k largest"""
    order = logit.detach().argsort(dim=1, descending=True, stable=True)
    return [float((order[:, :k] == target[:, None]).any(1).float().sum().mul_(1 / target.shape[0]).item()) for k in ks]


def literal_epoch(loader, model, optimizer, print_freq, epoch, train):
    """the reference's loop, step by step, with the meters written out: -> (stdout lines, local averages at the print points, returned pair)"""
    crit = torch.nn.CrossEntropyLoss()
    keys = ('Loss', 'acc@1', 'acc@5')
    s = {k: dict(val=0, sum=0, count=0, avg=0, last=[]) for k in keys}
    lines, local = [], []
    digits = len(str(len(loader)))
    for idx, (x, y) in enumerate(loader):
        B = x.shape[0]
        logit = model(scale(x).view(B, 3, 1, L, HW, HW).transpose(1, 2).contiguous().squeeze(1))
        loss = crit(logit, y)
        vals = (loss.item(),) + tuple(ref_topk(logit, y, (1, 5)))
        for k, v in zip(keys, vals):
            m = s[k]
            m['val'] = v
            m['sum'] += v * B
            m['count'] += B
            m['avg'] = m['sum'] / m['count']
            m['last'] = (m['last'] + [v])[-5:]
        if train:
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            if idx % print_freq == 0:
                head = 'Epoch:[%d][%*d/%*d]' % (epoch, digits, idx, digits, len(loader))
                lines.append('\t'.join([head, 'Time 0.00 (0.00)', 'Data 0.00 (0.00)'] +
                                       ['%s %.4f (%.4f)' % (k, s[k]['val'], s[k]['avg']) for k in keys]))
                local.append(tuple(sum(s[k]['last']) / len(s[k]['last']) for k in keys))
    return lines, local, (s['Loss']['avg'], s['acc@1']['avg']), s


def test_average_meter_and_progress_meter(capsys):
    from video_similarity_search_amd.coclr_utils.utils import AverageMeter, ProgressMeter
    m = AverageMeter('acc@1', ':.3f')
    vals = [0.5, 0.25, 1.0, 0.0, 0.75, 0.125, 0.375]
    ns_ = [4, 4, 0, 3, 1, 2, 5]
    tot = cnt = 0
    last, avg = [], 0
    for v, n in zip(vals, ns_):
        m.update(v, n, history=(n == 4))
        tot, cnt = tot + v * n, cnt + n
        if n:
            avg = tot / cnt
            last = (last + [v])[-5:]
        assert (m.val, m.sum, m.count, m.avg) == (v, tot, cnt, avg)
        assert m.local_avg == pytest.approx(sum(last) / len(last), abs=1e-15) and len(m.local_history) == len(last)
    assert m.history == [0.5, 0.25] and len(m) == cnt
    assert str(m) == 'acc@1 %.3f (%.3f)' % (vals[-1], avg)
    m.update(9.0, 1, step=0)                           # step = 0 leaves the local window alone
    assert list(m.local_history) == last
    d = AverageMeter()
    assert (d.name, str(d)) == ('null', 'null 0.0000 (0.0000)')
    ProgressMeter(120, [m, d], prefix='Epoch:[3]').display(7)
    assert capsys.readouterr().out == 'Epoch:[3][  7/120]\t%s\t%s\n' % (str(m), str(d))


def test_utils_reexports_and_neq_load(capsys):
    from video_similarity_search_amd.coclr_utils import utils
    from video_similarity_search_amd.loss.classification import calc_topk_accuracy
    from video_similarity_search_amd.online_train import calc_mask_accuracy
    assert utils.calc_topk_accuracy is calc_topk_accuracy and utils.calc_mask_accuracy is calc_mask_accuracy
    a, b = torch.nn.Linear(3, 2), torch.nn.Linear(3, 2)
    sd = {'weight': b.weight.detach().clone(), 'extra.bias': torch.zeros(1)}
    keep_bias = a.bias.detach().clone()
    assert utils.neq_load_customized(a, sd, verbose=True) is a
    out = capsys.readouterr().out
    assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, keep_bias)
    assert 'Weights not used from pretrained file:\nextra.bias\n' in out and 'Weights not loaded into new model:\nbias\n' in out


@pytest.mark.parametrize("sizes,print_freq", [((4, 4, 4, 4, 3), 3), ((5, 5, 2), 1), ((3, 3, 3, 1), 5)])
def test_train_one_epoch_is_the_literal_loop(capsys, monkeypatch, sizes, print_freq):
    from video_similarity_search_amd import coclr_classify as cc
    from segmean_cpu_kernels import NumpyClassifyKernels
    monkeypatch.setattr(cc.time, "time", lambda: 100.0)
    loader = batches(sizes, 1)
    model = stand_in(3 * L * HW * HW, C, 2)
    ref = copy.deepcopy(model)
    lines, local, want, _ = literal_epoch(loader, ref, torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9), print_freq, 4, True)
    K = NumpyClassifyKernels()
    args = epoch_args(train_plotter=Plotter(), logger=Log())
    args.print_freq = print_freq
    capsys.readouterr()
    got = cc.train_one_epoch(loader, model, torch.nn.CrossEntropyLoss(), torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9), scale,
                             "cpu", 4, args, kernels=K)
    out = capsys.readouterr().out
    tail = 'Epoch: [4][%d/%d]\tT-epoch:0.00\t' % (len(sizes) - 1, len(sizes))
    assert out == ''.join(ln + '\n' for ln in lines + [tail])
    assert got == want and model.training
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.equal(p, q)
    # one read-back per progress line, one more at the end when steps are still pending
    n_print = len([i for i in range(len(sizes)) if i % print_freq == 0])
    assert K.reads == n_print + ((len(sizes) - 1) % print_freq != 0)
    assert [c for c, _ in K.calls if c == "read"] == ["read"] * K.reads
    # the plotter got the local averages at the print points, at the running iteration, then the epoch averages
    loc = [d for d in args.train_plotter.data if d[0].startswith('local/')]
    assert [d[0] for d in loc] == ['local/loss', 'local/top1', 'local/top5'] * n_print
    assert [d[1] for d in loc] == pytest.approx([v for t in local for v in t], abs=1e-12)
    assert [d[2] for d in loc[::3]] == [11 + i for i in range(len(sizes)) if i % print_freq == 0] and args.iteration == 11 + len(sizes)
    assert [d[0] for d in args.train_plotter.data[-3:]] == ['global/loss', 'global/top1', 'global/top5']
    assert args.train_plotter.data[-3][1:] == (want[0], 4) and args.logger.lines == ['train ' + tail]


def test_train_what_last_puts_the_model_in_eval_and_works_without_plotter_or_logger(capsys, monkeypatch):
    from video_similarity_search_amd import coclr_classify as cc
    from segmean_cpu_kernels import NumpyClassifyKernels
    model = stand_in(3 * L * HW * HW, C, 2)
    args = ns(train_what='last', print_freq=2, num_seq=1, seq_len=L, img_dim=HW)
    cc.train_one_epoch(batches((3, 2), 5), model, torch.nn.CrossEntropyLoss(), torch.optim.SGD(model.parameters(), lr=0.1), scale, "cpu", 0,
                       args, kernels=NumpyClassifyKernels())
    assert not model.training and args.iteration == 3


def test_validate_reads_back_once(capsys):
    from video_similarity_search_amd import coclr_classify as cc
    from segmean_cpu_kernels import NumpyClassifyKernels
    sizes = (4, 4, 4, 3)
    loader = batches(sizes, 3)
    model = stand_in(3 * L * HW * HW, C, 4)
    before = copy.deepcopy(model.state_dict())
    _, _, want, s = literal_epoch(loader, copy.deepcopy(model).eval(), None, 1, 2, False)
    K = NumpyClassifyKernels()
    args = epoch_args(val_plotter=Plotter(), logger=Log())
    capsys.readouterr()
    got = cc.validate(loader, model.train(), torch.nn.CrossEntropyLoss(), scale, "cpu", 2, args, kernels=K)
    line = 'Epoch: [2]\tLoss: %.4f Acc@1: %.4f Acc@5: %.4f\t' % (s['Loss']['avg'], s['acc@1']['avg'], s['acc@5']['avg'])
    assert capsys.readouterr().out == line + '\n' and args.logger.lines == ['val ' + line]
    assert got == want and not model.training and K.reads == 1
    assert K.calls[-1] == ("read", (len(sizes), 3))
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    assert [d[0] for d in args.val_plotter.data] == ['global/loss', 'global/top1', 'global/top5']


def test_adjust_learning_rate():
    from video_similarity_search_amd.coclr_classify import adjust_learning_rate
    opt = torch.optim.SGD([{'params': [torch.nn.Parameter(torch.zeros(1))], 'lr': 0.5}, {'params': [torch.nn.Parameter(torch.zeros(1))]}], lr=0.25)
    adjust_learning_rate(opt, 3, ns(schedule=[2, 4]))
    assert [g['lr'] for g in opt.param_groups] == [0.5, 0.25]
    adjust_learning_rate(opt, 4, ns(schedule=[2, 4]))
    assert [g['lr'] for g in opt.param_groups] == [0.5 * 0.1, 0.25 * 0.1]


# ---------------------------------------------------------------------------------------------- views, packing, tables

FRAME, CROP, IMG = 12, 8, 6


class Videos(object):
    """(clip uint8 [S * L, FRAME, FRAME, 3], (target, vname)) per video; `reads` counts how often each video was fetched"""

    def __init__(self, S_list, seed, n_classes=C):
        rng = np.random.default_rng(seed)
        self.clips = [torch.from_numpy(rng.integers(0, 256, (S * L, FRAME, FRAME, 3), dtype=np.uint8)) for S in S_list]
        self.targets = [int(t) for t in rng.integers(0, n_classes, len(S_list))]
        self.names = ['cls%d/v_%03d/frames' % (t, i) for i, t in enumerate(self.targets)]
        self.reads = [0] * len(S_list)

    def __len__(self):
        return len(self.clips)

    def __getitem__(self, i):
        self.reads[i] += 1
        return self.clips[i], (torch.tensor(self.targets[i]), self.names[i])


class Counting(torch.nn.Module):
    def __init__(self, net, as_tuple=False):
        super().__init__()
        self.net, self.as_tuple, self.batches = net, as_tuple, []

    def forward(self, x):
        self.batches.append(x.shape[0])
        y = self.net(x)
        return (None, y) if self.as_tuple else y


def normalise5(kernels):
    from video_similarity_search_amd.coclr_utils import transforms as T
    return T.Compose([T.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], channel=1)], kernels=kernels)


def view_clips(video, chain, tf):
    """the reference's per-view pass for one video: its S clips [S, 3, L, IMG, IMG] under one of the ten chains"""
    x = tf(chain(video)[None])
    S = video.shape[0] // L
    return x.view(3, S, 1, L, IMG, IMG).permute(1, 2, 0, 3, 4, 5).squeeze(1)


def test_five_crop_windows_and_forced_flips():
    from video_similarity_search_amd.coclr_utils import transforms as T
    h, w = 10, 14
    win = {k: T.FiveCrop((4, 6), k).window(h, w) for k in range(1, 6)}
    assert win == {1: (0, 0, 4, 6), 2: (0, 8, 4, 6), 3: (6, 0, 4, 6), 4: (4, 8, 6, 6), 5: (3, 4, 4, 6)}       # 4: the reference's h - tw
    assert T.FiveCrop(5).size == (5, 5)
    with pytest.raises(ValueError, match="bigger than input size"):
        T.FiveCrop((11, 4), 1).window(h, w)
    with pytest.raises(ValueError):
        T.FiveCrop(4, 6)
    assert (T.RandomHorizontalFlip(command='left').p, T.RandomHorizontalFlip(command='right').p, T.RandomHorizontalFlip().p) == (0, 1, 0.5)
    with pytest.raises(ValueError):
        T.RandomHorizontalFlip(command='up')


def test_multi_view_is_one_launch_of_ten_records_on_one_source():
    from video_similarity_search_amd.coclr_utils import transforms as T
    from clip_transforms_cpu_kernels import NumpyClipKernels
    kern = NumpyClipKernels()
    video = Videos([2], 7).clips[0]
    chains = T.ten_crop_views(CROP, IMG, kernels=kern)
    seen = []
    run = kern.run
    kern.run = lambda groups, *a: (seen.append([g.src.data_ptr() for g in groups]), run(groups, *a))[1]
    views = T.multi_view(video, chains)
    assert views.shape == (10, 3, 2 * L, IMG, IMG) and views.dtype == torch.float32 and views.is_contiguous()
    assert len(seen) == 1 and seen[0] == [video.data_ptr()] * 10 and kern.launches == [("apply",)]
    # view by view it is the chain applied on its own: centre, the corners in the reference's numbering, then the same flipped
    f = video.permute(3, 0, 1, 2).float() / 255
    for n, where in enumerate((5, 1, 2, 3, 4)):
        one = T.Compose(chains[n].transforms, kernels=NumpyClipKernels())(video)
        assert torch.equal(views[n], one)
        flipped = T.Compose(chains[n + 5].transforms, kernels=NumpyClipKernels())(video)
        assert torch.equal(views[n + 5], flipped)
        i, j, th, tw = T.FiveCrop(CROP, where).window(FRAME, FRAME)
        plain = T.Compose([T.Resize((IMG, IMG))], kernels=NumpyClipKernels())
        assert torch.allclose(views[n], plain(f[:, :, i:i + th, j:j + tw].contiguous()), rtol=0, atol=1e-6)
        assert torch.allclose(views[n + 5], plain(f.flip(-1)[:, :, i:i + th, j:j + tw].contiguous()), rtol=0, atol=1e-6)
    same = T.ten_crop_views(CROP, CROP)
    assert all(len(c.transforms) == 3 for c in same) and all(len(c.transforms) == 4 for c in chains)
    with pytest.raises(ValueError):
        T.multi_view(video, [])


@pytest.mark.parametrize("flag,limit", [("ten_crop", 16), ("ten_crop", 64), ("five_crop", 7), ("center_crop", 3)])
def test_test_10crop_packs_and_averages(tmp_path, capsys, flag, limit):
    from video_similarity_search_amd import coclr_classify as cc
    from video_similarity_search_amd.coclr_utils import transforms as T
    from segmean_cpu_kernels import NumpyClassifyKernels, softmax64, target_ranks
    S_list = [1, 2, 5, 2, 1]
    data = Videos(S_list, 11)
    net = stand_in(3 * L * IMG * IMG, C, 12)
    with torch.no_grad():
        net[1].weight.mul_(10)                    # probabilities away from uniform, so that ranks mean something
    model = Counting(net)
    K = NumpyClassifyKernels()
    tf = normalise5(K.clip)
    ckpt = str(tmp_path / "epoch9.pth.tar")
    args = ns(num_seq=1, seq_len=L, img_dim=IMG, crop_size=CROP, clips_per_forward=limit, checkpoint_path=ckpt, logger=Log(),
              **{flag: True})
    capsys.readouterr()
    res = cc.test_10crop(data, model.train(), None, tf, "cpu", 9, args, kernels=K)
    out = capsys.readouterr().out

    n_views = dict(cc.TITLES)[flag.split('_')[0]]
    titles = ['center', 'five', 'ten'] if flag == "ten_crop" else [flag.split('_')[0]]
    assert list(res) == titles and not model.training and data.reads == [1] * len(S_list)            # every video read once
    total = n_views * sum(S_list)
    assert model.batches == [limit] * (total // limit) + ([total % limit] if total % limit else [])
    assert any(n_views * S > limit for S in S_list) or limit == 64                                   # a video split across forwards
    seg_calls = [d for c, d in K.calls if c == "segment_mean"]
    assert all(d["mode"] == 1 and d["accumulate"] == 1 for d in seg_calls) and len(seg_calls) <= len(titles) * len(model.batches)
    assert len({id(d["table"]) for d in seg_calls}) == len(titles) and K.reads == len(titles)

    # the reference's shape: one pass per view, a forward per video, softmax / mean per view, then the mean over the views — in float64
    chains = T.ten_crop_views(CROP, IMG, kernels=K.clip)
    per_view = np.zeros((10, len(S_list), C))
    with torch.no_grad():
        for n in range(10):
            for i in range(len(S_list)):
                per_view[n, i] = softmax64(net(view_clips(data.clips[i], chains[n], tf)).numpy()).mean(0)
    lines = [{'center_crop': 'Test using center crop', 'five_crop': 'Test using 5 crop', 'ten_crop': 'Test using 10 crop'}[flag]]
    logs = [{'center_crop': 'Test using center_crop\n', 'five_crop': 'Test using 5_crop\n', 'ten_crop': 'Test using 10_crop\n'}[flag]]
    for t in titles:
        want = per_view[:dict(cc.TITLES)[t]].mean(0)
        stat = json.load(open(ckpt + '-prob-%s.json' % t))
        assert list(stat) == data.names
        got = np.array([stat[v]['mean_prob'] for v in data.names])
        assert got.shape == (len(S_list), 1, C)
        np.testing.assert_allclose(got[:, 0], want, rtol=0, atol=2e-6)
        rank = target_ranks(got[:, 0].astype(np.float32), data.targets)
        acc = ((rank == 0).mean(), (rank < 5).mean())
        assert res[t] == acc
        lines += ['%s-crop result:' % t, 'Mean: Acc@1: %.4f Acc@5: %.4f' % acc]
        logs += ['%s-crop:' % t, 'test Epoch: [9]\tMean: Acc@1: %.4f Acc@5: %.4f' % acc]
    assert out == ''.join(ln + '\n' for ln in lines) and args.logger.lines == logs


def test_test_10crop_argument_errors(tmp_path):
    from video_similarity_search_amd import coclr_classify as cc
    from segmean_cpu_kernels import NumpyClassifyKernels
    K = NumpyClassifyKernels()
    net = stand_in(3 * L * IMG * IMG, C, 12)
    base = dict(num_seq=1, seq_len=L, img_dim=IMG, crop_size=CROP, checkpoint_path=str(tmp_path / "m.pth.tar"))
    with pytest.raises(ValueError, match="center_crop / five_crop / ten_crop"):
        cc.test_10crop(Videos([1], 1), net, None, normalise5(K.clip), "cpu", 0, ns(**base), kernels=K)
    with pytest.raises(ValueError, match="whole number of windows"):
        cc.test_10crop(Videos([1], 1), net, None, normalise5(K.clip), "cpu", 0, ns(**dict(base, seq_len=3), ten_crop=True), kernels=K)
    with pytest.raises(ValueError, match="bigger than input size"):
        cc.test_10crop(Videos([1], 1), net, None, normalise5(K.clip), "cpu", 0, ns(**dict(base, crop_size=FRAME + 1), ten_crop=True), kernels=K)


def test_summarize_probability_reports_a_bad_target(tmp_path):
    from video_similarity_search_amd import coclr_classify as cc
    from segmean_cpu_kernels import NumpyClassifyKernels
    table = torch.full((2, C), 1.0 / C)
    with pytest.raises(ValueError, match="outside"):
        cc.summarize_probability(table, [0, C], ['a', 'b'], 'ten', ns(checkpoint_path=str(tmp_path / "m")), kernels=NumpyClassifyKernels())
    with pytest.raises(ValueError, match="2 targets and 1 names"):
        cc.summarize_probability(table, [0, 1], ['a'], 'ten', ns(checkpoint_path=str(tmp_path / "m")), kernels=NumpyClassifyKernels())


def test_test_retrieval_files_cache_and_accuracies(tmp_path, capsys):
    from video_similarity_search_amd import coclr_classify as cc
    from video_similarity_search_amd.coclr_utils import transforms as T
    from segmean_cpu_kernels import NumpyClassifyKernels, topk64
    D = 10
    rng = np.random.default_rng(21)
    train = Videos([int(s) for s in rng.choice([1, 2, 5], 53)], 22, n_classes=4)
    test = Videos([1, 2, 5, 2, 1, 5, 2], 23, n_classes=4)
    net = stand_in(3 * L * IMG * IMG, D, 24)
    model = Counting(net, as_tuple=True)
    K = NumpyClassifyKernels()
    tf = normalise5(K.clip)
    args = ns(num_seq=1, seq_len=L, img_dim=IMG, crop_size=CROP, clips_per_forward=8, checkpoint_path=str(tmp_path / "ck.pth.tar"),
              dataset='ucf101', dirname=None, logger=Log())
    capsys.readouterr()
    acc = cc.test_retrieval(model.train(), None, tf, "cpu", 0, args, train_dataset=train, test_dataset=test, kernels=K)
    out = capsys.readouterr().out
    assert not model.training and test.reads == [1] * len(test) and train.reads == [1] * len(train)
    n_clips = sum(c.shape[0] // L for c in test.clips), sum(c.shape[0] // L for c in train.clips)
    assert model.batches == sum(([8] * (n // 8) + ([n % 8] if n % 8 else []) for n in n_clips), [])
    assert all(d["mode"] == 0 for c, d in K.calls if c == "segment_mean") and K.reads == 1

    # float64, the reference's shape: a forward per video, the mean over its windows, centring, normalising, a full sort
    centre = T.ten_crop_views(CROP, IMG, kernels=K.clip)[0]
    with torch.no_grad():
        f = {n: np.stack([net(view_clips(v, centre, tf)).double().numpy().mean(0) for v in d.clips]) for n, d in (("test", test), ("train", train))}
    root = tmp_path / "feature"
    for n, d in (("test", test), ("train", train)):
        np.testing.assert_allclose(torch.load(root / ('ucf101_%s_feature.pth.tar' % n)).numpy(), f[n], rtol=0, atol=1e-5)
        assert torch.load(root / ('ucf101_%s_label.pth.tar' % n)).tolist() == d.targets
        assert pickle.load(open(root / ('ucf101_%s_vname.pkl' % n), 'rb')) == d.names
    assert sorted(os.listdir(root)) == sorted('ucf101_%s_%s' % (n, w) for n in ("test", "train") for w in ("feature.pth.tar", "label.pth.tar", "vname.pkl"))
    idx = topk64(f["test"] - f["test"].mean(0), f["train"] - f["train"].mean(0), 50)
    lab = np.array(train.targets)[idx] == np.array(test.targets)[:, None]
    want = [float(np.float32(lab[:, :k].any(1).sum()) / np.float32(len(test))) for k in cc.RETRIEVAL_KS]
    assert acc == want
    text = ['%dNN acc = %.4f' % (k, a) for k, a in zip(cc.RETRIEVAL_KS, want)]
    assert out == ''.join(s + '\n' for s in ['train dataset size: 53', 'test dataset size: 7', 'Computing test set feature ... ',
                                            'torch.Size([7, 10])', 'Computing train set feature ... ', 'torch.Size([53, 10])'] + text)
    assert args.logger.lines == ['NN-Retrieval on ucf101:'] + ['\t' + s for s in text]

    # a second run finds the files and runs no forward
    model.batches = []
    acc2 = cc.test_retrieval(model, None, tf, "cpu", 0, args, train_dataset=train, test_dataset=test, kernels=K)
    out2 = capsys.readouterr().out
    assert acc2 == acc and model.batches == [] and test.reads == [1] * len(test)
    assert out2.splitlines()[2] == str(root / 'ucf101_test_feature.pth.tar') + ' exists' and 'Computing' not in out2

    small = Videos([1] * 49, 25, n_classes=4)
    args.dirname = 'other'
    with pytest.raises(ValueError, match="top-50"):
        cc.test_retrieval(model, None, tf, "cpu", 0, args, train_dataset=small, test_dataset=test, kernels=K)


# ---------------------------------------------------------------------------------------------- the entry point's host checks

def seg_call(lib, R, C, seg_off, rows, w, table_rows, ld=None, ldt=None, mode=1, accumulate=0):
    """slic_segment_mean with a host table and pointers that are never followed: every case here must be refused before a launch"""
    from video_similarity_search_amd import coclr_classify as cc
    host = cc.pack_segments(seg_off, rows, w)
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(dummy))
    rc = lib.slic_segment_mean(p, C if ld is None else ld, R, C, p, ctypes.c_void_p(host.data_ptr()), len(rows), mode, accumulate, p,
                               C if ldt is None else ldt, table_rows, None)
    return rc, lib.slic_last_error().decode()


BAD_SEGMENTS = [
    ("descending offsets", dict(R=10, C=5, seg_off=[0, 4, 3, 6], rows=[0, 1, 2], w=[1, 1, 1], table_rows=3), "not ascending"),
    ("negative first offset", dict(R=10, C=5, seg_off=[-1, 4], rows=[0], w=[1], table_rows=3), "leave"),
    ("offsets past R", dict(R=10, C=5, seg_off=[0, 4, 11], rows=[0, 1], w=[1, 1], table_rows=3), "leave"),
    ("empty segment", dict(R=10, C=5, seg_off=[0, 4, 4, 6], rows=[0, 1, 2], w=[1, 1, 1], table_rows=3), "empty"),
    ("repeated row", dict(R=10, C=5, seg_off=[0, 4, 5, 6], rows=[2, 1, 2], w=[1, 1, 1], table_rows=3), "two segments"),
    ("row past the table", dict(R=10, C=5, seg_off=[0, 4], rows=[3], w=[1], table_rows=3), "table of 3"),
    ("negative row", dict(R=10, C=5, seg_off=[0, 4], rows=[-1], w=[1], table_rows=3), "table of 3"),
    ("C = 0", dict(R=10, C=0, seg_off=[0, 4], rows=[0], w=[1], table_rows=3), "outside [1, 4096]"),
    ("C = 4097", dict(R=10, C=4097, seg_off=[0, 4], rows=[0], w=[1], table_rows=3), "outside [1, 4096]"),
    ("input pitch below C", dict(R=10, C=5, seg_off=[0, 4], rows=[0], w=[1], table_rows=3, ld=4), "pitches"),
    ("table pitch below C", dict(R=10, C=5, seg_off=[0, 4], rows=[0], w=[1], table_rows=3, ldt=4), "pitches"),
    ("mode 2", dict(R=10, C=5, seg_off=[0, 4], rows=[0], w=[1], table_rows=3, mode=2), "mode"),
]


@pytest.mark.parametrize("name,kw,text", BAD_SEGMENTS, ids=[b[0] for b in BAD_SEGMENTS])
def test_segment_mean_refuses_bad_arguments_on_the_host(name, kw, text):
    from video_similarity_search_amd import _lib
    from segmean_cpu_kernels import check_segments
    lib = _lib.load()
    rc, msg = seg_call(lib, **kw)
    assert rc == -1 and msg.startswith("slic_segment_mean:") and text in msg, (rc, msg)
    if kw.get("mode", 1) in (0, 1):
        with pytest.raises(ValueError):              # the mirror's rules are the entry point's
            check_segments(kw["R"], kw["C"], kw["seg_off"], kw["rows"], kw["w"], kw["table_rows"], kw.get("ld"), kw.get("ldt"))


def test_segment_mean_null_pointers_and_the_mirrors_agree():
    from video_similarity_search_amd import _lib
    from segmean_cpu_kernels import check_segments, segment_mean32, segment_mean64
    lib = _lib.load()
    assert lib.slic_segment_mean(None, 5, 10, 5, None, None, 1, 1, 0, None, 5, 3, None) == -1
    assert b"slic_segment_mean" in lib.slic_last_error()
    # float32 in the kernel's order against the float64 definition: both modes, accumulate, scrambled rows, a -inf beside a finite maximum
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((23, 101)) * 3).astype(np.float32)
    x[1, 7] = -np.inf                                  # row 1 is segment 0 on its own, which writes table row 4
    seg_off, rows, w = [1, 2, 9, 23], [4, 0, 2], [0.5, 1 / 7, 1 / 14]
    check_segments(23, 101, seg_off, rows, w, 5)
    for mode in (0, 1):
        t32 = np.full((5, 101), 0.25, dtype=np.float32)
        t64 = segment_mean64(x, seg_off, rows, w, segment_mean64(x, seg_off, rows, w, t32, mode, 0), mode, 1)
        segment_mean32(x, seg_off, rows, w, segment_mean32(x, seg_off, rows, w, t32, mode, 0), mode, 1)
        assert np.array_equal(t32[[1, 3]], np.full((2, 101), 0.25, dtype=np.float32))
        np.testing.assert_allclose(t32, t64, rtol=0, atol=1e-5 if mode == 0 else 2e-7)
        if mode == 1:
            assert t32[4, 7] == 0.0

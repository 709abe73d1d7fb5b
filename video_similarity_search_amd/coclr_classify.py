"""
Drop-in for the loops of the reference's coclr_classify.py — the downstream action-recognition protocol (linear probe / fine-tune
epochs, the multi-crop test, nearest-neighbour retrieval):

    train_one_epoch(data_loader, model, criterion, optimizer, transforms_cuda, device, epoch, args)     <- :395-463
    validate(data_loader, model, criterion, transforms_cuda, device, epoch, args)                       <- :466-509
    test_10crop(dataset, model, criterion, transforms_cuda, device, epoch, args)                        <- :512-610
    summarize_probability(prob_table, targets, vnames, title, args)                                     <- :613-635
    test_retrieval(model, criterion, transforms_cuda, device, epoch, args, *, train_dataset, test_dataset)   <- :638-822
    adjust_learning_rate(optimizer, epoch, args)                                                        <- :825-830

`args` is any object with the reference's attribute names (train_what, final_bn, print_freq, num_seq, seq_len, img_dim, iteration,
center_crop / five_crop / ten_crop, checkpoint_path, dataset, dirname); train_plotter / val_plotter / logger are used when present.
Two more are read when present: clips_per_forward (default 64) and crop_size (default 224, the reference's constant).  Every
function takes `kernels=`: another provider with HipClassifyKernels' methods (the CPU suite drives the host logic with a NumPy one).

What changes is where the arithmetic runs and when the host looks at it.

Epochs.  One forward, the criterion, top-1 / top-5 from the criterion's own pass when it is this package's CrossEntropyLoss (else
calc_topk_accuracy).  The three scalars of a step stay on the device in a pending list; the list is read back as ONE tensor when a
progress line is due (idx % print_freq == 0) and at the end of the epoch — validate: once — and replayed through AverageMeter in batch
order, so every printed and returned number is the reference's.  The reference reads three .item() per step.

test_10crop.  The dataset yields (clip, (target, vname)): the undecorated uint8 [N, H, W, 3] frames of ALL windows of a video,
N = S * num_seq * seq_len.  The video is read once; transforms.multi_view makes its 1 / 5 / 10 views in one launch; transforms_cuda
and the reference's reshaping turn them into views * S clips, view-major (centre, the four corners, then the five flipped).  Clips of
consecutive videos are packed into forwards of clips_per_forward (a video may straddle two forwards).  After each forward
slic_segment_mean (mode 1, accumulate) adds w * sum of softmax(logits) into the device tables 'center', 'five' and 'ten' — the same
logits under three segment lists, w = 1 / (views * S) — so a table row ends as the mean probability of its video ('ten' covers every
row of a batch; the rows 'center' and 'five' use are gathered first when a batch holds several videos, because the kernel takes
consecutive segments).  The reference
runs the loader ten times at batch = one video's windows.  summarize_probability: the rank of the target in every row from one
slic_softmax_ce_fwd pass on the table (ranks do not change under the positive scale w), one read-back (table + the three counters)
for the accuracies and <checkpoint>-prob-<title>.json.
Differences: the reference takes the mean per view and then over views; with the same S in every view that is the same real number
as the flat mean here, to rounding.  Its 'Aug type' lines are not printed (there are no passes), the final file of a five- or
centre-crop run carries its own title (the reference names it 'ten' whatever ran), the function returns {'center': (acc1, acc5), ..}
for the titles it ran and does not call sys.exit.  Views: see transforms.ten_crop_views (bilinear resample, no test-time jitter).

test_retrieval.  Centre-crop view, packed forwards; the features are the model's output, or the last element when it returns a
tuple; slic_segment_mean (mode 0) writes the per-video mean into a [V, D] table.  Features, labels and names are cached in the
reference's files.  Then slic_col_stats + slic_sub_rowvec (centring), cosine_topk(k = 50), which normalises (slic_normalize_rows), and
slic_topk_label_hits at ks = [1, 5, 10, 20, 50].  The [N_test, N_train] similarity matrix is never built and `<dataset>_sim.pth.tar`
is not written.  Returns the five accuracies; no sys.exit.  Both datasets are arguments (the LMDB readers are out of scope).
"""
import json
import os
import pickle
import time

import numpy as np
import torch

from . import _lib
from .coclr_utils import transforms as T
from .coclr_utils.utils import AverageMeter, ProgressMeter
from .loss.classification import HITS_HEAD, CrossEntropyLoss

CROP_SIZE = 224                         # FiveCrop / CenterCrop size of the reference's test transforms
CLIPS_PER_FORWARD = 64
RETRIEVAL_KS = [1, 5, 10, 20, 50]
TITLES = (('center', 1), ('five', 5), ('ten', 10))


def pack_segments(seg_off, rows, w):
    """the segment table of slic_segment_mean — int32 seg_off[V + 1], int32 rows[V], float32 w[V] — as one pinned byte tensor"""
    seg_off, rows = np.asarray(seg_off, dtype=np.int32).reshape(-1), np.asarray(rows, dtype=np.int32).reshape(-1)
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    V = rows.shape[0]
    if seg_off.shape[0] != V + 1 or w.shape[0] != V:
        raise ValueError("segments: %d offsets, %d rows, %d weights (V + 1, V, V expected)" % (seg_off.shape[0], V, w.shape[0]))
    raw = np.concatenate([seg_off.view(np.uint8), rows.view(np.uint8), w.view(np.uint8)])
    host = torch.empty(raw.shape[0], dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    host.numpy()[:] = raw
    return host


class HipClassifyKernels(object):
    """the device side of this module.  `reads` counts read(): the host synchronisations these loops add.  `clip`: the provider the
    clip transforms run on (None: their HIP kernels)."""
    clip = None

    def __init__(self):
        if not torch.cuda.is_available():
            raise _lib.SlicError("coclr_classify needs a gfx950 device (no CPU fallback)")
        _lib.load()
        self.reads = 0

    def segment_mean(self, x, seg_off, rows, w, table, mode, accumulate):
        """table[rows[v]] (+)= w[v] * sum over rows seg_off[v] .. seg_off[v + 1] of x (mode 0) or of their softmax (mode 1)"""
        x = x.detach()
        if x.dim() != 2 or table.dim() != 2 or table.shape[1] != x.shape[1]:
            raise ValueError("segment_mean: x [R, C] and table [V, C] expected, got %s and %s" % (tuple(x.shape), tuple(table.shape)))
        if x.dtype != torch.float32 or x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
            x = x.float().contiguous()
        if table.dtype != torch.float32 or table.stride(1) != 1:
            raise ValueError("segment_mean: the table is fp32 with unit column stride")
        _lib.require_device(x, table)
        R, C = x.shape
        host = pack_segments(seg_off, rows, w)
        dev = host.to(x.device, non_blocking=True)
        _lib.call("slic_segment_mean", _lib.ptr(x), x.stride(0) if R > 1 else max(C, x.stride(0)), R, C, _lib.ptr(dev),
                  _lib.c_void_p(host.data_ptr()), len(rows), int(mode), int(accumulate), _lib.ptr(table),
                  table.stride(0) if table.shape[0] > 1 else max(C, table.stride(0)), table.shape[0], _lib.stream())

    def target_hits(self, table, targets):
        """int32 [3 + V] on the device: {targets outside [0, C), rows whose target ranks first, rows whose target is in the first
        five, the rank of every row's target} (slic_softmax_ce_fwd on the table; nothing is read back here)"""
        _lib.require_device(table, targets)
        V, C = table.shape
        dev = table.device
        lse = torch.empty(V, 2, dtype=torch.float32, device=dev)
        rowloss = torch.empty(V, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        hits = torch.empty(HITS_HEAD + V, dtype=torch.int32, device=dev)
        _lib.call("slic_softmax_ce_fwd", _lib.ptr(table), table.stride(0) if V > 1 else max(C, table.stride(0)), V, C,
                  _lib.ptr(targets.contiguous()), _lib.ptr(lse), _lib.ptr(rowloss), _lib.ptr(loss), _lib.ptr(hits), _lib.stream())
        return hits

    def topk_accuracy(self, logit, target, topk):
        from .loss.classification import calc_topk_accuracy
        return calc_topk_accuracy(logit, target, topk)

    def centre(self, feat):
        """feat - its column mean (column sums in double, slic_col_stats; slic_sub_rowvec works on columns in fours)"""
        _lib.require_device(feat)
        N, D = feat.shape
        Dp = (D + 3) // 4 * 4
        x = feat.detach()
        if Dp != D or x.dtype != torch.float32 or not x.is_contiguous():
            x = torch.zeros(N, Dp, dtype=torch.float32, device=feat.device)
            x[:, :D] = feat
        cs = torch.empty(2, Dp, dtype=torch.float64, device=x.device)
        ws = _lib.workspace(_lib.load().slic_col_stats_workspace_bytes(N, Dp), x.device, "classify_cs")
        _lib.call("slic_col_stats", _lib.ptr(x), N, Dp, Dp, _lib.ptr(cs[0]), _lib.ptr(cs[1]), _lib.ptr(ws), _lib.stream())
        mean = (cs[0] / N).to(torch.float32)
        out = torch.empty_like(x)
        _lib.call("slic_sub_rowvec", _lib.ptr(x), N, Dp, Dp, _lib.ptr(mean), _lib.ptr(out), Dp, _lib.stream())
        return out[:, :D]

    def topk(self, q, g, k):
        """[Nq, k] int32: the k gallery rows of largest cosine similarity, best first (rows are normalised by the search)"""
        from .evaluate import cosine_topk
        return cosine_topk(q, g, k=k)[0]

    def label_hits(self, idx, q_labels, g_labels, top_ks):
        from .evaluate import _label_hits
        return _label_hits(idx, q_labels, g_labels, top_ks)

    def read(self, t):
        self.reads += 1
        return t.detach().cpu().numpy()


def _kernels(kernels):
    return HipClassifyKernels() if kernels is None else kernels      # raises SlicError without a gfx950 device


def _log(args, text):
    logger = getattr(args, 'logger', None)
    if logger is not None:
        logger.log(text)


def _plot(plotter, tag, value, step):
    if plotter is not None:
        plotter.add_data(tag, value, step)


def _batch_tr(transforms_cuda, args):
    def tr(x):      # transformation on tensor
        B = x.size(0)
        return transforms_cuda(x).view(B, 3, args.num_seq, args.seq_len, args.img_dim, args.img_dim).transpose(1, 2).contiguous()
    return tr


def _step_record(K, criterion, logit, target, loss, B):
    """float32 [3] on the device: (loss, top-1, top-5) of one step, each the value the reference's .item() would read"""
    if isinstance(criterion, CrossEntropyLoss) and criterion.hits is not None:
        top1, top5 = criterion.top1_hits.float().mul_(1 / B), criterion.top5_hits.float().mul_(1 / B)
    else:
        top1, top5 = K.topk_accuracy(logit.detach(), target, (1, 5))
    return torch.stack([loss.detach().float().reshape(()), top1.reshape(()), top5.reshape(())])


class _Pending(object):
    """per-step records kept on the device until a read-back replays them through the meters in batch order"""

    def __init__(self, K, meters):
        self.K, self.meters, self.items = K, meters, []

    def add(self, rec, B):
        self.items.append((rec, B))

    def flush(self):
        if not self.items:
            return
        host = self.K.read(torch.stack([r for r, _ in self.items]))
        for row, (_, B) in zip(host, self.items):
            for m, v in zip(self.meters, row):
                m.update(float(v), B)
        self.items = []


def train_one_epoch(data_loader, model, criterion, optimizer, transforms_cuda, device, epoch, args, *, kernels=None):
    K = _kernels(kernels)
    batch_time = AverageMeter('Time', ':.2f')
    data_time = AverageMeter('Data', ':.2f')
    losses = AverageMeter('Loss', ':.4f')
    top1_meter = AverageMeter('acc@1', ':.4f')
    top5_meter = AverageMeter('acc@5', ':.4f')
    progress = ProgressMeter(len(data_loader), [batch_time, data_time, losses, top1_meter, top5_meter], prefix='Epoch:[{}]'.format(epoch))
    pending = _Pending(K, (losses, top1_meter, top5_meter))
    plotter = getattr(args, 'train_plotter', None)

    if args.train_what == 'last':
        model.eval()    # totally freeze BN in backbone: the linear-probe pass of models/resnet.py
    else:
        model.train()
    if getattr(args, 'final_bn', False):
        model.module.final_bn.train()

    end = time.time()
    tic = time.time()
    tr = _batch_tr(transforms_cuda, args)
    if not hasattr(args, 'iteration'):
        args.iteration = 1

    for idx, (input_seq, target) in enumerate(data_loader):
        data_time.update(time.time() - end)
        B = input_seq.size(0)
        input_seq = tr(input_seq.to(device, non_blocking=True))
        target = target.to(device, non_blocking=True)

        input_seq = input_seq.squeeze(1)    # num_seq is always 1
        logit = model(input_seq)
        loss = criterion(logit, target)
        pending.add(_step_record(K, criterion, logit, target, loss, B), B)

        optimizer.zero_grad()
        loss.backward()
        optimizer.step()

        batch_time.update(time.time() - end)
        end = time.time()

        if idx % args.print_freq == 0:
            pending.flush()
            progress.display(idx)
            _plot(plotter, 'local/loss', losses.local_avg, args.iteration)
            _plot(plotter, 'local/top1', top1_meter.local_avg, args.iteration)
            _plot(plotter, 'local/top5', top5_meter.local_avg, args.iteration)

        args.iteration += 1

    pending.flush()
    print('Epoch: [{0}][{1}/{2}]\t'
          'T-epoch:{t:.2f}\t'.format(epoch, idx, len(data_loader), t=time.time() - tic))
    _plot(plotter, 'global/loss', losses.avg, epoch)
    _plot(plotter, 'global/top1', top1_meter.avg, epoch)
    _plot(plotter, 'global/top5', top5_meter.avg, epoch)
    _log(args, 'train Epoch: [{0}][{1}/{2}]\t'
               'T-epoch:{t:.2f}\t'.format(epoch, idx, len(data_loader), t=time.time() - tic))
    return losses.avg, top1_meter.avg


def validate(data_loader, model, criterion, transforms_cuda, device, epoch, args, *, kernels=None):
    K = _kernels(kernels)
    batch_time = AverageMeter()
    losses = AverageMeter()
    top1_meter = AverageMeter('acc@1', ':.4f')
    top5_meter = AverageMeter('acc@5', ':.4f')
    pending = _Pending(K, (losses, top1_meter, top5_meter))
    plotter = getattr(args, 'val_plotter', None)

    model.eval()
    tr = _batch_tr(transforms_cuda, args)
    with torch.no_grad():
        end = time.time()
        for idx, (input_seq, target) in enumerate(data_loader):
            B = input_seq.size(0)
            input_seq = tr(input_seq.to(device, non_blocking=True))
            target = target.to(device, non_blocking=True)

            input_seq = input_seq.squeeze(1)    # num_seq is always 1
            logit = model(input_seq)
            loss = criterion(logit, target)
            pending.add(_step_record(K, criterion, logit, target, loss, B), B)
            batch_time.update(time.time() - end)
            end = time.time()
    pending.flush()       # the epoch's one read-back

    print('Epoch: [{0}]\t'
          'Loss: {loss.avg:.4f} Acc@1: {top1.avg:.4f} Acc@5: {top5.avg:.4f}\t'
          .format(epoch, loss=losses, top1=top1_meter, top5=top5_meter))
    _plot(plotter, 'global/loss', losses.avg, epoch)
    _plot(plotter, 'global/top1', top1_meter.avg, epoch)
    _plot(plotter, 'global/top5', top5_meter.avg, epoch)
    _log(args, 'val Epoch: [{0}]\t'
               'Loss: {loss.avg:.4f} Acc@1: {top1.avg:.4f} Acc@5: {top5.avg:.4f}\t'
               .format(epoch, loss=losses, top1=top1_meter, top5=top5_meter))
    return losses.avg, top1_meter.avg


class _PackedForwards(object):
    """clips of consecutive videos queued in order and run through the model `limit` at a time.  on_output(output, pieces) follows each
    forward; pieces: (video, position of the piece's first clip within the video, number of clips, first row in the batch)."""

    def __init__(self, model, limit, on_output):
        if limit < 1:
            raise ValueError("clips_per_forward must be at least 1, got %r" % (limit,))
        self.model, self.limit, self.on_output = model, int(limit), on_output
        self.chunks, self.total, self.forwards = [], 0, 0

    def add(self, video, clips):
        self.chunks.append((clips, video, 0))
        self.total += clips.shape[0]
        while self.total >= self.limit:
            self._run(self.limit)

    def finish(self):
        if self.total:
            self._run(self.total)

    def _run(self, n):
        parts, pieces, at = [], [], 0
        while at < n:
            clips, video, pos = self.chunks[0]
            take = min(n - at, clips.shape[0])
            parts.append(clips[:take])
            pieces.append((video, pos, take, at))
            at += take
            if take == clips.shape[0]:
                self.chunks.pop(0)
            else:
                self.chunks[0] = (clips[take:], video, pos + take)
        self.total -= n
        out = self.model(parts[0] if len(parts) == 1 else torch.cat(parts))
        self.forwards += 1
        self.on_output(out, pieces)


def _video_clips(clip, chains, transforms_cuda, device, args):
    """(the views * S clips of one video, view-major, float32 [views * S, 3, seq_len, img_dim, img_dim]; S)"""
    if args.num_seq != 1:
        raise ValueError("num_seq is always 1 in this protocol (the reference squeezes that axis), got %r" % (args.num_seq,))
    N = clip.shape[0]
    S = N // (args.seq_len * args.num_seq)
    if S < 1 or S * args.seq_len * args.num_seq != N:
        raise ValueError("a video of %d frames is not a whole number of windows of %d" % (N, args.seq_len * args.num_seq))
    views = T.multi_view(clip.to(device, non_blocking=True), chains)
    nv = views.shape[0]
    x = transforms_cuda(views).view(nv, 3, S, args.num_seq, args.seq_len, args.img_dim, args.img_dim).permute(0, 2, 3, 1, 4, 5, 6)
    return x.reshape(nv * S, 3, args.seq_len, args.img_dim, args.img_dim), S


def _sample(dataset, i):
    clip, (target, vname) = dataset[i]
    if isinstance(vname, (list, tuple)):
        vname = vname[0]
    return clip, int(target), vname


def test_10crop(dataset, model, criterion, transforms_cuda, device, epoch, args, *, kernels=None):
    K = _kernels(kernels)
    model.eval()

    title = None
    if getattr(args, 'center_crop', False):
        print('Test using center crop')
        _log(args, 'Test using center_crop\n')
        title = 'center'
    if getattr(args, 'five_crop', False):
        print('Test using 5 crop')
        _log(args, 'Test using 5_crop\n')
        title = 'five'
    if getattr(args, 'ten_crop', False):
        print('Test using 10 crop')
        _log(args, 'Test using 10_crop\n')
        title = 'ten'
    if title is None:
        raise ValueError("test_10crop: one of args.center_crop / five_crop / ten_crop must be set")
    n_views = dict(TITLES)[title]
    titles = [(t, n) for t, n in TITLES if t == title or title == 'ten']          # a ten-crop run also reports the other two
    chains = T.ten_crop_views(getattr(args, 'crop_size', CROP_SIZE), args.img_dim, kernels=K.clip)[:n_views]

    V = len(dataset)
    tables, S_of, targets, vnames = {}, [], [], []

    def on_output(out, pieces):
        logit = out[0] if isinstance(out, tuple) else out
        if not tables:
            for t, _ in titles:
                tables[t] = torch.zeros(V, logit.shape[1], dtype=torch.float32, device=logit.device)
        for t, n in titles:
            off, rows, w = [], [], []
            for video, pos, take, at in pieces:
                upto = n * S_of[video]                   # view-major: this title's clips are the first n * S of the video
                hi = min(pos + take, upto)
                if hi > pos:
                    off.append((at, at + hi - pos))
                    rows.append(video)
                    w.append(1.0 / upto)
            if not rows:
                continue
            # slic_segment_mean takes consecutive segments.  'ten' covers every row of the batch; 'center' and 'five' leave the rows of
            # the other views between two videos out, so with several videos in the batch their rows are gathered first
            seg_off, keep = _as_offsets(off)
            x = logit if keep is None else logit.index_select(0, torch.as_tensor(keep, dtype=torch.int64, device=logit.device))
            K.segment_mean(x, seg_off, rows, w, tables[t], 1, 1)

    packed = _PackedForwards(model, getattr(args, 'clips_per_forward', CLIPS_PER_FORWARD), on_output)
    with torch.no_grad():
        for i in range(V):
            clip, target, vname = _sample(dataset, i)
            clips, S = _video_clips(clip, chains, transforms_cuda, device, args)
            S_of.append(S)
            targets.append(target)
            vnames.append(vname)
            packed.add(i, clips)
        packed.finish()

    result = {}
    for t, _ in titles:
        print('%s-crop result:' % t)
        result[t] = summarize_probability(tables[t], targets, vnames, t, args, epoch=epoch, kernels=K)
    return result


def _as_offsets(ranges):
    """[(a0, b0), (a1, b1), ..] ascending and disjoint -> (seg_off, None) when they abut, else (seg_off over the gathered rows, the
    row indices to gather): slic_segment_mean takes consecutive segments"""
    if all(ranges[i][1] == ranges[i + 1][0] for i in range(len(ranges) - 1)):
        return [ranges[0][0]] + [b for _, b in ranges], None
    keep, seg_off = [], [0]
    for a, b in ranges:
        keep.extend(range(a, b))
        seg_off.append(len(keep))
    return seg_off, keep


def summarize_probability(prob_table, targets, vnames, title, args, *, epoch=None, kernels=None):
    """Acc@1 / Acc@5 of the [V, C] table of mean probabilities against `targets`, and <checkpoint>-prob-<title>.json
    ({vname: {'mean_prob': [[..]]}}, the reference's nesting); with `epoch` the two lines the reference's caller logs are logged"""
    K = _kernels(kernels)
    V, C = prob_table.shape
    if len(targets) != V or len(vnames) != V:
        raise ValueError("summarize_probability: %d targets and %d names for %d rows" % (len(targets), len(vnames), V))
    if V >= 1 << 24:
        raise ValueError("summarize_probability: more than 2^24 videos")       # the counters travel as fp32 beside the table
    tgt = torch.as_tensor(np.asarray(targets, dtype=np.int64)).to(prob_table.device)
    hits = K.target_hits(prob_table, tgt)
    host = K.read(torch.cat([prob_table.reshape(-1), hits[:HITS_HEAD].to(torch.float32)]))
    bad, top1, top5 = (int(v) for v in host[V * C:])
    if bad:
        raise ValueError("summarize_probability: %d target(s) outside [0, %d)" % (bad, C))
    probs = host[:V * C].reshape(V, C)
    acc1, acc5 = top1 / V, top5 / V          # AverageMeter over V updates of 0. / 1.
    print('Mean: Acc@1: {:.4f} Acc@5: {:.4f}'.format(acc1, acc5))
    stat = {vname: {'mean_prob': [probs[i].tolist()]} for i, vname in enumerate(vnames)}
    with open(os.path.join(os.path.dirname(args.checkpoint_path),
                           '%s-prob-%s.json' % (os.path.basename(args.checkpoint_path), title)), 'w') as fp:
        json.dump(stat, fp)
    if epoch is not None:
        _log(args, '%s-crop:' % title)
        _log(args, 'test Epoch: [{0}]\t'
                   'Mean: Acc@1: {1:.4f} Acc@5: {2:.4f}'.format(epoch, acc1, acc5))
    return acc1, acc5


def _video_features(dataset, model, transforms_cuda, device, args, K):
    """([V, D] per-video mean features on the device, int64 [V] labels on the device, names)"""
    crop = getattr(args, 'crop_size', CROP_SIZE)
    chains = T.ten_crop_views(crop, args.img_dim, kernels=K.clip)[:1]
    V = len(dataset)
    state = {}
    S_of, labels, vnames = [], [], []

    def on_output(out, pieces):
        feature = out[-1] if isinstance(out, tuple) else out
        feature = feature.reshape(feature.shape[0], -1)
        if not state:
            state['table'] = torch.zeros(V, feature.shape[1], dtype=torch.float32, device=feature.device)
        seg_off = [pieces[0][3]] + [at + take for _, _, take, at in pieces]
        K.segment_mean(feature, seg_off, [v for v, _, _, _ in pieces], [1.0 / S_of[v] for v, _, _, _ in pieces], state['table'], 0, 1)

    packed = _PackedForwards(model, getattr(args, 'clips_per_forward', CLIPS_PER_FORWARD), on_output)
    for i in range(V):
        clip, target, vname = _sample(dataset, i)
        clips, S = _video_clips(clip, chains, transforms_cuda, device, args)
        S_of.append(S)
        labels.append(target)
        vnames.append(vname)
        packed.add(i, clips)
    packed.finish()
    table = state['table']
    return table, torch.as_tensor(np.asarray(labels, dtype=np.int64)).to(table.device), vnames


def test_retrieval(model, criterion, transforms_cuda, device, epoch, args, *, train_dataset, test_dataset, kernels=None):
    K = _kernels(kernels)
    model.eval()
    dirname = 'feature' if getattr(args, 'dirname', None) is None else args.dirname
    root = os.path.join(os.path.dirname(args.checkpoint_path), dirname)

    def path(split, what):
        return os.path.join(root, '%s_%s_%s' % (args.dataset, split, what))

    with torch.no_grad():
        print('train dataset size: %d' % len(train_dataset))
        print('test dataset size: %d' % len(test_dataset))
        feats = {}
        for split, dataset in (('test', test_dataset), ('train', train_dataset)):
            if os.path.exists(path(split, 'feature.pth.tar')):
                if split == 'test':
                    print(path(split, 'feature.pth.tar'), 'exists')
                feature = torch.load(path(split, 'feature.pth.tar')).to(device)
                label = torch.load(path(split, 'label.pth.tar')).to(device)
            else:
                os.makedirs(root, exist_ok=True)
                print('Computing %s set feature ... ' % split)
                feature, label, vname = _video_features(dataset, model, transforms_cuda, device, args, K)
                print(feature.size())
                torch.save(feature, path(split, 'feature.pth.tar'))
                torch.save(label, path(split, 'label.pth.tar'))
                with open(path(split, 'vname.pkl'), 'wb') as fp:
                    pickle.dump(vname, fp)
            feats[split] = (feature, label)

        (test_feature, test_label), (train_feature, train_label) = feats['test'], feats['train']
        ks = RETRIEVAL_KS
        if train_feature.shape[0] < ks[-1]:
            raise ValueError("test_retrieval: top-%d needs at least that many train videos, got %d" % (ks[-1], train_feature.shape[0]))
        # centering, then the search (which normalises the rows) and the label count; no similarity matrix
        idx = K.topk(K.centre(test_feature), K.centre(train_feature), ks[-1])
        hits = K.read(K.label_hits(idx, test_label, train_label, ks))
        NN_acc = [float(np.float32(h) / np.float32(test_feature.shape[0])) for h in hits]
        for k, acc in zip(ks, NN_acc):
            print('%dNN acc = %.4f' % (k, acc))

        _log(args, 'NN-Retrieval on %s:' % args.dataset)
        for k, acc in zip(ks, NN_acc):
            _log(args, '\t%dNN acc = %.4f' % (k, acc))
    return NN_acc


def adjust_learning_rate(optimizer, epoch, args):
    '''Decay the learning rate based on schedule'''
    ratio = 0.1 if epoch in args.schedule else 1.
    for param_group in optimizer.param_groups:
        param_group['lr'] = param_group['lr'] * ratio

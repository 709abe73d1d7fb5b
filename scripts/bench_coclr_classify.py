"""The ten-crop test protocol per video: packed (coclr_classify.test_10crop) against the reference's shape, same model, same device.

    python scripts/bench_coclr_classify.py [--runs 20] [--videos 64] [--out FILE.txt]

Setting: one MI355X, generate_model(18, classifier=True), C = 101, 64 synthetic videos of S = 5 windows of [16, 128, 171] uint8 frames,
views cropped to 112 x 112 (= img_dim, so no resample on either side).
(a) reference-shaped: ten passes over the test set, one per (flip, crop); in each the video is fetched and uploaded again, its view
    made, a forward of its S clips, torch softmax(-1).mean(0); then per video stack / mean / top-k / two .item(), after the centre
    pass, the unflipped passes and all ten (three summaries), each with its JSON file — coclr_classify.py:512-635 in this
    package's transforms and model.
(b) packed: test_10crop — each video fetched once, its ten views from one launch, forwards of 64 clips, slic_segment_mean into
    the three tables, one rank pass and one read-back per table, the same three JSON files.
Time: each side one WHOLE protocol run over the videos, host clock with a device synchronise before and after, divided by the number
of videos; the sides alternate run by run after one warm-up run each; median, min and max over --runs runs of each, and the ratio of the
medians.  The two sides' ten-crop probabilities are compared once (largest difference) so that the times are of the same result.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_similarity_search_amd import coclr_classify as cc  # noqa: E402
from video_similarity_search_amd.coclr_utils import transforms as T  # noqa: E402
from video_similarity_search_amd.models import generate_model  # noqa: E402

SEQ, S, H, W, CROP, NCLS = 16, 5, 128, 171, 112, 101
DEV = "cuda"


class Videos(object):
    def __init__(self, n, seed):
        rng = np.random.default_rng(seed)
        self.clips = [torch.from_numpy(rng.integers(0, 256, (S * SEQ, H, W, 3), dtype=np.uint8)) for _ in range(n)]
        if torch.cuda.is_available():
            self.clips = [c.pin_memory() for c in self.clips]
        self.targets = [int(t) for t in rng.integers(0, NCLS, n)]
        self.names = ['cls%03d/v_%04d/frames' % (t, i) for i, t in enumerate(self.targets)]

    def __len__(self):
        return len(self.clips)

    def __getitem__(self, i):
        return self.clips[i], (self.targets[i], self.names[i])


def topk_accuracy(output, target, topk):
    """coclr_utils/utils.py's calc_topk_accuracy in torch ops, as the reference runs it on the device"""
    _, pred = output.topk(max(topk), 1, True, True)
    correct = pred.t().eq(target.view(1, -1))
    return [correct[:k].reshape(-1).float().sum(0).mul_(1 / target.size(0)) for k in topk]


def reference_shaped(data, model, tf, chains, ckpt):
    """ten passes, a forward per video, per-video host arithmetic: -> {title: (acc1, acc5)} and the ten-crop mean probabilities"""
    prob, res, last = {}, {}, None

    def summarize(title):
        hits, stat = [0.0, 0.0], {}
        for i, (vname, item) in enumerate(prob.items()):
            mean_prob = torch.stack(item, 0).mean(0)
            top1, top5 = topk_accuracy(mean_prob, torch.LongTensor([data.targets[i]]).to(DEV), (1, 5))
            stat[vname] = {'mean_prob': mean_prob.tolist()}
            hits[0] += top1.item()
            hits[1] += top5.item()
        with open(ckpt + '-prob-%s.json' % title, 'w') as fp:
            json.dump(stat, fp)
        return hits[0] / len(prob), hits[1] / len(prob), stat

    with torch.no_grad():
        for n, chain in enumerate(chains):
            for i in range(len(data)):
                clip, (_, vname) = data[i]
                x = tf(chain(clip.to(DEV, non_blocking=True))[None])
                x = x.view(3, S, 1, SEQ, CROP, CROP).permute(1, 2, 0, 3, 4, 5).squeeze(1).contiguous()
                prob.setdefault(vname, []).append(F.softmax(model(x), dim=-1).mean(0, keepdim=True))
            if n in (0, 4, 9):
                title = {0: 'center', 4: 'five', 9: 'ten'}[n]
                a1, a5, last = summarize(title)
                res[title] = (a1, a5)
    return res, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = generate_model(18, hidden_layer=64, out_dim=32, n_input_channels=3, shortcut_type='B', conv1_t_size=7, conv1_t_stride=1,
                               no_max_pool=True, widen_factor=1.0, projection_head=False, classifier=True, num_classes=NCLS)
    torch.nn.init.normal_(model.linear.weight, std=0.05)
    model = model.cuda().eval()
    data = Videos(a.videos, 1)
    tf = T.Compose([T.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], channel=1)])
    chains = T.ten_crop_views(CROP, CROP)
    tmp = tempfile.mkdtemp()
    ckpt = {side: os.path.join(tmp, side, "epoch0.pth.tar") for side in ("ref", "packed")}
    for p in ckpt.values():
        os.makedirs(os.path.dirname(p))
    args = types.SimpleNamespace(num_seq=1, seq_len=SEQ, img_dim=CROP, crop_size=CROP, clips_per_forward=64, ten_crop=True,
                                 checkpoint_path=ckpt["packed"])

    def packed():
        with contextlib.redirect_stdout(io.StringIO()):
            return cc.test_10crop(data, model, None, tf, "cuda", 0, args)

    def ref():
        return reference_shaped(data, model, tf, chains, ckpt["ref"])

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / len(data), out

    (_, (res_ref, stat)), (_, res_new) = timed(ref), timed(packed)              # warm-up: every shape of both sides
    new = json.load(open(ckpt["packed"] + '-prob-ten.json'))
    diff = max(np.abs(np.array(stat[v]['mean_prob']) - np.array(new[v]['mean_prob'])).max() for v in data.names)
    t_ref, t_new = [], []
    for r in range(a.runs):
        t_ref.append(timed(ref)[0])
        t_new.append(timed(packed)[0])
        print("run %2d: reference-shaped %8.2f ms / video, packed %8.2f ms / video" % (r, t_ref[-1], t_new[-1]), flush=True)
    m_ref, m_new = statistics.median(t_ref), statistics.median(t_new)
    lines = [
        "ten-crop test protocol, %s, depth 18, C = %d, %d videos of S = %d windows of [%d, %d, %d] -> %d x %d, %d runs of each side, alternating"
        % (torch.cuda.get_device_name(0), NCLS, len(data), S, SEQ, H, W, CROP, CROP, a.runs),
        "ms per video (whole protocol run / videos; host clock between device synchronisations)",
        "%-18s %10s %10s %10s" % ("side", "median", "min", "max"),
        "%-18s %10.2f %10.2f %10.2f" % ("reference-shaped", m_ref, min(t_ref), max(t_ref)),
        "%-18s %10.2f %10.2f %10.2f" % ("packed", m_new, min(t_new), max(t_new)),
        "ratio of the medians (reference-shaped / packed): %.3f" % (m_ref / m_new),
        "same result: largest difference of a ten-crop mean probability %.3e; accuracies reference-shaped %s, packed %s"
        % (diff, {k: tuple(round(x, 4) for x in v) for k, v in res_ref.items()}, {k: tuple(round(x, 4) for x in v) for k, v in res_new.items()}),
    ]
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

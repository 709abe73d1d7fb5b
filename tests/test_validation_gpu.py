"""GPU: the validation pass on the HIP kernels — slic_triplet_val_batch and slic_topk_label_hits against the float64 rules
(tests/validate_cpu_kernels.py) and against slic_pair_distance bit for bit; validate() end to end against the same loop written
from the package's older public pieces; the reference's golden runs (tests/golden/validation.npz) through the real kernels."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
ns = types.SimpleNamespace


def _val_batch(ex, ey, ez, euclid, margin):
    from video_similarity_search_amd._lib import call, ptr, stream
    B, D = ex.shape
    da, db = (torch.full((B,), float("nan"), device="cuda") for _ in range(2))
    rec = torch.full((5,), float("nan"), device="cuda")
    call("slic_triplet_val_batch", ptr(ex), ptr(ey), ptr(ez), B, D, int(euclid), float(margin), ptr(da), ptr(db), ptr(rec), stream())
    return da, db, rec


@pytest.mark.parametrize("euclid", [0, 1])
@pytest.mark.parametrize("D", [128, 512, 130])
@pytest.mark.parametrize("B", [1, 7, 80, 300])
def test_triplet_val_batch(gpu, B, D, euclid):
    """distances bit-equal to slic_pair_distance and within its test's tolerances of float64 (atol 1e-6 cosine, 1e-5 euclidean, on
    unit-scale rows); acc equal; loss within 1e-6 relative of the float64 mean of the device's own float32 hinge terms.
    D = 130: the scalar path (rows not 16-byte aligned).  Rows with a zero vector (the norm clamp) and with ey == ez included."""
    from video_similarity_search_amd.models.triplet_net import pair_distance
    from validate_cpu_kernels import val_batch64
    rng = np.random.default_rng(1000 * B + 2 * D + euclid)
    ex, ey, ez = (torch.from_numpy((rng.standard_normal((B, D)) / np.sqrt(D)).astype(np.float32)) for _ in range(3))
    if B >= 7:
        ex[1] = 0
        ey[2] = 0
        ez[4] = ey[4]
        ex[5], ey[5] = 0, 0
    margin = 0.2
    ex, ey, ez = ex.cuda(), ey.cuda(), ez.cuda()
    da, db, rec = _val_batch(ex, ey, ez, euclid, margin)
    metric = 'euclidean' if euclid else 'cosine'
    assert torch.equal(da, pair_distance(ex, ey, metric)) and torch.equal(db, pair_distance(ex, ez, metric))
    da64, db64, _, acc64 = val_batch64(ex, ey, ez, euclid, margin)
    atol = 1e-5 if euclid else 1e-6
    print("B %d D %d %s: max |dist - fp64| = %.3g" % (B, D, metric, max(np.abs(da.cpu().numpy() - da64).max(), np.abs(db.cpu().numpy() - db64).max())))
    assert torch.allclose(da.cpu().double(), torch.from_numpy(da64), atol=atol, rtol=0)
    assert torch.allclose(db.cpu().double(), torch.from_numpy(db64), atol=atol, rtol=0)
    rec = rec.cpu().numpy()
    assert rec[1] == np.float32(acc64) and rec[2] == B and np.isnan(rec[3]) and np.isnan(rec[4])
    hinge = torch.clamp((da - db) + margin, min=0)                          # float32, from the device's own distances
    want = hinge.double().mean().item()
    print("   loss %.9g, float64 mean of the float32 terms %.9g" % (rec[0], want))
    assert abs(float(rec[0]) - want) <= 1e-6 * want
    # NULL distance outputs: same record; the views of a larger matrix (row pointers 16-byte aligned or not) too
    from video_similarity_search_amd._lib import call, ptr, stream
    rec2 = torch.zeros(5, device="cuda")
    call("slic_triplet_val_batch", ptr(ex), ptr(ey), ptr(ez), B, D, euclid, margin, None, None, ptr(rec2), stream())
    assert np.array_equal(rec2.cpu().numpy()[:3], rec[:3])


def test_triplet_val_batch_refuses_bad_sizes(gpu):
    from video_similarity_search_amd import _lib
    x = torch.zeros(4, 8, device="cuda")
    rec = torch.zeros(5, device="cuda")
    for B, D in ((0, 8), (4, 0), (-1, 8)):
        assert gpu.slic_triplet_val_batch(_lib.ptr(x), _lib.ptr(x), _lib.ptr(x), B, D, 0, 0.2, None, None, _lib.ptr(rec), _lib.stream()) != 0
        assert b"slic_triplet_val_batch" in gpu.slic_last_error()


@pytest.mark.parametrize("Nq,Ng,k,top_ks,pad", [(1, 30, 1, [1], False), (257, 1000, 20, [1, 5, 10, 20], False), (5000, 400, 50, [1, 2, 3, 5, 10, 20, 30, 50], True),
                                                (333, 50, 20, [1, 5, 10, 20], True), (64, 21, 20, [20], False)])
def test_topk_label_hits(gpu, Nq, Ng, k, top_ks, pad):
    """exactly the host's _acc_from_indices * Nq; -1 padding and indices >= Ng never hit; labels beyond 2^31 compare in full"""
    from video_similarity_search_amd.evaluate import _acc_from_indices, _label_hits
    from validate_cpu_kernels import label_hits
    rng = np.random.default_rng(Nq + Ng + k)
    idx = rng.integers(0, Ng, (Nq, k)).astype(np.int32)
    base = np.int64(1) << 40
    g_lab = base + rng.integers(0, 12, Ng).astype(np.int64)
    q_lab = base + rng.integers(0, 14, Nq).astype(np.int64)
    q_lab[::7] -= base                   # equal to a gallery label in the low 32 bits only: no hit
    if pad:
        idx[rng.random((Nq, k)) < 0.3] = -1
        idx[::5, k // 2:] = -1
    first = torch.full((Nq,), -7, dtype=torch.int32, device="cuda")
    hits = _label_hits(torch.from_numpy(idx).cuda(), q_lab, torch.from_numpy(g_lab).cuda(), top_ks, first_hit=first)
    host_idx = np.where(idx < 0, Ng, idx)                                   # the host rule has no padding: send it to a label nobody has
    want = _acc_from_indices(host_idx, q_lab, np.append(g_lab, np.int64(-1)), top_ks) * Nq
    assert hits.dtype == torch.int32 and np.array_equal(hits.cpu().numpy(), np.rint(want).astype(np.int64))
    f, h = label_hits(idx, q_lab, g_lab, top_ks)
    assert np.array_equal(first.cpu().numpy(), f) and np.array_equal(hits.cpu().numpy(), h)
    # written, not accumulated; first_hit optional; an index past the gallery is no hit
    idx2 = idx.copy()
    idx2[:, 0] = Ng + 3
    hits2 = _label_hits(torch.from_numpy(idx2).cuda(), q_lab, g_lab, top_ks)
    assert np.array_equal(hits2.cpu().numpy(), label_hits(idx2, q_lab, g_lab, top_ks)[1])


def test_topk_acc_device_matches_get_topk_acc(gpu, golden_dir):
    from video_similarity_search_amd.evaluate import topk_acc_device
    g = dict(np.load(os.path.join(golden_dir, "validation.npz")))
    for dm in ("cosine", "euclidean"):
        acc = topk_acc_device(g["knn_test"], g["knn_test_labels"].tolist(), torch.from_numpy(g["knn_train"]), torch.from_numpy(g["knn_train_labels"]),
                              dist_metric=dm)
        assert acc.dtype == np.float64 and np.array_equal(acc, g["knn_%s/acc" % dm])


# ---------------------------------------------------------------------------------------------------------------------------
class _Loader(list):
    dataset = None


def _meter():
    from video_similarity_search_amd.online_train import AverageMeter
    return AverageMeter()


def _parent_loop(loader, net, margin, epoch, cfg):
    """validation.py:12-151 written over Tripletnet + torch.nn.MarginRankingLoss + the accuracy formula + get_distance_matrix +
    get_topk_acc, with the reference's per-batch .item() reads"""
    from video_similarity_search_amd.evaluate import get_distance_matrix, get_topk_acc
    crit = torch.nn.MarginRankingLoss(margin=margin)
    losses, accs, top1, top5 = _meter(), _meter(), _meter(), _meter()
    embs, labs, rows = [], [], []
    net.eval()
    with torch.no_grad():
        for (a, p, n), (ta, tp, tn), _ in loader:
            dista, distb, ex, ey, ez = net(a.cuda(), p.cuda(), n.cuda())
            loss = crit(dista, distb, torch.full_like(dista, -1))
            acc = ((distb - dista) > 0).sum() * 1.0 / dista.size()[0]
            row = [loss.item(), acc.item(), a.size(0), None, None]
            if cfg.VAL.METRIC == 'global':
                embs.append(ex.flatten(1).cpu())
                labs.append(ta)
            else:
                e = torch.cat((ex.flatten(1).cpu(), ey.flatten(1).cpu()), dim=0)
                t = get_topk_acc(get_distance_matrix(e, dist_metric=cfg.LOSS.DIST_METRIC), torch.cat((ta, tp)).tolist())
                top1.update(t[0])
                top5.update(t[1])
                row[3:] = [t[0], t[1]]
            accs.update(acc.item(), a.size(0))
            losses.update(loss.item(), a.size(0))
            rows.append(row)
    if cfg.VAL.METRIC == 'global':
        t = get_topk_acc(get_distance_matrix(torch.cat(embs), dist_metric=cfg.LOSS.DIST_METRIC), torch.cat(labs).tolist())
        top1.update(t[0])
        top5.update(t[1])
        rows[-1][3:] = [t[0], t[1]]
    line = 'epoch:{} {:.4f} {:.2f}'.format(epoch, losses.avg, accs.avg*100.) + ' {:.2f} {:.2f}'.format(100.*top1.avg, 100.*top5.avg) + '\n'
    return rows, accs.avg, line


@pytest.mark.parametrize("metric", ["global", "local_batch"])
@pytest.mark.parametrize("dm", ["cosine", "euclidean"])
def test_validate_end_to_end_vs_the_older_pieces(gpu, tmp_path, metric, dm):
    from test_encoder_gpu import R3D18_KW
    from video_similarity_search_amd.models import generate_model, Tripletnet
    from video_similarity_search_amd.validation import validate, HipValidationKernels
    torch.manual_seed(3)
    m = generate_model(18, **dict(R3D18_KW, widen_factor=0.125, hidden_layer=64, out_dim=32)).cuda().eval()
    net = Tripletnet(m, dm)
    rng = np.random.default_rng(77)
    loader = _Loader()
    sizes = [12, 11, 12]
    loader.dataset = range(sum(sizes))
    for b in sizes:
        clips = [torch.from_numpy((rng.standard_normal((b, 3, 8, 32, 32)) * rng.uniform(0.3, 3.0, (b, 1, 1, 1, 1))).astype(np.float32)) for _ in range(3)]
        ta = torch.from_numpy(rng.integers(0, 4, b))
        loader.append((tuple(clips), (ta, ta.clone(), torch.from_numpy(rng.integers(0, 4, b))), torch.arange(b)))
    cfg = ns(NUM_GPUS=1, OUTPUT_PATH=str(tmp_path), VAL=ns(METRIC=metric, LOG_INTERVAL=2), LOSS=ns(DIST_METRIC=dm), DATASET=ns(MODALITY=False),
             MODEL=ns(ARCH='3dresnet'))
    rows, acc_avg, line = _parent_loop(loader, net, 0.2, 5, cfg)

    class Keeps(HipValidationKernels):
        def read_record(self, rec):
            self.host = super().read_record(rec)
            return self.host

    K = Keeps()
    ret = validate(loader, net, torch.nn.MarginRankingLoss(margin=0.2), 5, cfg, True, torch.device("cuda"), True, kernels=K)
    assert K.reads == 2
    for r, h in zip(rows, K.host):
        print("parent loop", r, "record", h.tolist())
        assert abs(h[0] - r[0]) <= 1e-6 and abs(h[1] - r[1]) <= 1e-6 and h[2] == r[2]
    n_rows = {"global": [sum(sizes)] * len(sizes), "local_batch": [2 * b for b in sizes]}[metric]
    for r, h, n in zip(rows, K.host, n_rows):
        if r[3] is not None:
            assert int(np.rint(h[3] * n)) == int(np.rint(r[3] * n)) and int(np.rint(h[4] * n)) == int(np.rint(r[4] * n))
    assert abs(ret - acc_avg) <= 1e-6
    assert open(os.path.join(str(tmp_path), "tnet_checkpoints", "val_loss_and_acc.txt")).read() == line


@pytest.mark.parametrize("metric", ["global", "local_batch"])
@pytest.mark.parametrize("dm", ["cosine", "euclidean"])
def test_golden_runs_through_the_kernels(gpu, golden_dir, tmp_path, capsys, metric, dm):
    from test_validation_cpu import cfg_for, encoder, golden, loader, val_file
    from video_similarity_search_amd.models import Tripletnet
    from video_similarity_search_amd.validation import validate
    g = golden(golden_dir)
    tag = "%s_%s" % (metric, dm)
    capsys.readouterr()
    ret = validate(loader(g), Tripletnet(encoder(g).cuda(), dm), torch.nn.MarginRankingLoss(margin=float(g["margin"])), int(g["epoch"]),
                   cfg_for(str(tmp_path), metric, dm, g), True, torch.device("cuda"), True)
    assert capsys.readouterr().out == str(g[tag + "/stdout"])
    assert val_file(str(tmp_path)) == str(g[tag + "/file"])
    assert abs(ret - float(g[tag + "/return"])) <= 1e-6

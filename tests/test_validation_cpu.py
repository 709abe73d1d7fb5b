"""CPU: the host logic of validation.validate and evaluate.k_nearest_embeddings — loader contract, the device-resident epoch record
and its replay into the reference's AverageMeter arithmetic, prints, files, the one collective per read-back — driven with the
float64 NumPy provider (tests/validate_cpu_kernels.py) against goldens produced by the reference's own validate
(tests/golden/make_goldens_validation.py).  The same cases on the HIP kernels: tests/test_validation_gpu.py."""
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ns = types.SimpleNamespace
CASES = [(m, d) for m in ("global", "local_batch") for d in ("cosine", "euclidean")]


def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "validation.npz")))


def encoder(g):
    m = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(g["enc_weight"].shape[1], g["enc_weight"].shape[0]))
    with torch.no_grad():
        m[1].weight.copy_(torch.from_numpy(g["enc_weight"]))
        m[1].bias.copy_(torch.from_numpy(g["enc_bias"]))
    return m


class Loader(list):
    dataset = None


def rank_rows(s, b, rank, world):
    """rows of the batch at s .. s + b that rank `rank` sees: equal parts, the last one wrapping round to the batch's first rows when b
    is not a multiple of the world size (the padding of DistributedSampler: every collective needs equal shapes)"""
    h = (b + world - 1) // world
    return s + (np.arange(h) + rank * h) % b


def loader(g, rank=0, world=1):
    """the golden's batches; with world > 1 rank r gets its own part of every batch"""
    ld, s = Loader(), 0
    ld.dataset = range(int(g["sizes"].sum()))
    for b in g["sizes"]:
        rows = rank_rows(s, int(b), rank, world)
        ld.append((tuple(torch.from_numpy(g["clips"][i, rows]) for i in range(3)),
                   tuple(torch.from_numpy(g["targets"][i, rows]) for i in range(3)), torch.from_numpy(rows)))
        s += b
    return ld


def cfg_for(out_dir, metric, dm, g, world=1, log_interval=None, modality=False, arch='3dresnet'):
    return ns(NUM_GPUS=world, OUTPUT_PATH=out_dir, VAL=ns(METRIC=metric, LOG_INTERVAL=int(g["log_interval"]) if log_interval is None else log_interval),
              LOSS=ns(DIST_METRIC=dm), DATASET=ns(MODALITY=modality), MODEL=ns(ARCH=arch))


class TorchTripletnet(torch.nn.Module):
    """models/triplet_net.py:7-34 in torch ops, for the module-by-module route on the CPU"""

    def __init__(self, embeddingnet, dist_metric):
        super().__init__()
        self.embeddingnet, self.dist_metric = embeddingnet, dist_metric

    def forward(self, x, y, z):
        ex, ey, ez = self.embeddingnet(x), self.embeddingnet(y), self.embeddingnet(z)
        if self.dist_metric == 'euclidean':
            return F.pairwise_distance(ex, ey, 2), F.pairwise_distance(ex, ez, 2), ex, ey, ez
        return 1 - F.cosine_similarity(ex, ey, dim=1), 1 - F.cosine_similarity(ex, ez, dim=1), ex, ey, ez


def val_file(out_dir):
    return open(os.path.join(out_dir, "tnet_checkpoints", "val_loss_and_acc.txt")).read()


@pytest.mark.parametrize("metric,dm", CASES)
def test_validate_reproduces_the_reference_run(golden_dir, tmp_path, capsys, metric, dm):
    from video_similarity_search_amd.validation import validate
    from validate_cpu_kernels import NumpyValidationKernels
    g = golden(golden_dir)
    tag = "%s_%s" % (metric, dm)
    K = NumpyValidationKernels()
    capsys.readouterr()
    ret = validate(loader(g), TorchTripletnet(encoder(g), dm), torch.nn.MarginRankingLoss(margin=float(g["margin"])), int(g["epoch"]),
                   cfg_for(str(tmp_path), metric, dm, g), False, "cpu", True, kernels=K)
    out = capsys.readouterr().out
    assert out == str(g[tag + "/stdout"])
    assert val_file(str(tmp_path)) == str(g[tag + "/file"])
    assert abs(ret - float(g[tag + "/return"])) <= 1e-6
    # no per-batch synchronisation: the record is read at the log points and once at the end
    n_log = sum(1 for b in range(len(g["sizes"])) if (b + 1) % int(g["log_interval"]) == 0)
    assert n_log >= 2 and len(g["sizes"]) % int(g["log_interval"]) != 0
    assert K.reads == n_log + 1


@pytest.mark.parametrize("metric,dm", CASES)
def test_other_criterion_goes_module_by_module(golden_dir, tmp_path, capsys, metric, dm):
    from video_similarity_search_amd.validation import validate
    from validate_cpu_kernels import NumpyValidationKernels
    g = golden(golden_dir)
    tag = "%s_%s" % (metric, dm)
    margin = float(g["margin"])
    calls = []

    def hinge(dista, distb, target):
        calls.append(dista.shape[0])
        assert torch.equal(target, torch.full_like(dista, -1))
        return torch.clamp(dista - distb + margin, min=0).mean()

    class Refuses(NumpyValidationKernels):
        def val_batch(self, *a):
            raise AssertionError("the fused step was taken for a criterion that is not MarginRankingLoss")

    capsys.readouterr()
    ret = validate(loader(g), TorchTripletnet(encoder(g), dm), hinge, int(g["epoch"]), cfg_for(str(tmp_path), metric, dm, g), False, "cpu",
                   True, kernels=Refuses())
    assert calls == list(g["sizes"])
    assert capsys.readouterr().out == str(g[tag + "/stdout"])
    assert val_file(str(tmp_path)) == str(g[tag + "/file"])
    assert abs(ret - float(g[tag + "/return"])) <= 1e-6
    # MarginRankingLoss with another reduction is not the fused kernel's loss either
    with pytest.raises(AssertionError, match="fused"):
        class Fused(NumpyValidationKernels):
            def val_batch(self, *a):
                raise AssertionError("fused")
        validate(loader(g), TorchTripletnet(encoder(g), dm), torch.nn.MarginRankingLoss(margin=margin), 0, cfg_for(None, metric, dm, g),
                 False, "cpu", False, kernels=Fused())
    validate(loader(g), TorchTripletnet(encoder(g), dm), torch.nn.MarginRankingLoss(margin=margin, reduction='sum'), 0,
             cfg_for(None, metric, dm, g), False, "cpu", False, kernels=Refuses())


def test_unknown_metric_prints_the_reference_message(golden_dir, tmp_path, capsys):
    from video_similarity_search_amd.validation import validate
    from validate_cpu_kernels import NumpyValidationKernels
    g = golden(golden_dir)
    capsys.readouterr()
    validate(loader(g), TorchTripletnet(encoder(g), 'cosine'), torch.nn.MarginRankingLoss(margin=float(g["margin"])), 3,
             cfg_for(str(tmp_path), 'nearest', 'cosine', g), False, "cpu", True, kernels=NumpyValidationKernels())
    out = capsys.readouterr().out
    assert out.count('Metric type:nearest is not implemented\n') == len(g["sizes"])
    assert 'Top1' not in out
    ref = str(g["global_cosine/file"]).split()
    assert val_file(str(tmp_path)) == ' '.join(ref[:3]) + '\n'           # no top-k fields


def test_what_is_out_of_scope_raises(golden_dir):
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.validation import validate
    from video_similarity_search_amd.evaluate import k_nearest_embeddings, topk_acc_device
    from validate_cpu_kernels import NumpyValidationKernels
    g = golden(golden_dir)
    net, crit = TorchTripletnet(encoder(g), 'cosine'), torch.nn.MarginRankingLoss(margin=0.2)
    with pytest.raises(NotImplementedError, match="MODALITY"):
        validate(loader(g), net, crit, 0, cfg_for(None, 'global', 'cosine', g, modality=True), False, "cpu", kernels=NumpyValidationKernels())
    with pytest.raises(NotImplementedError, match="SlowFast"):
        validate(loader(g), net, crit, 0, cfg_for(None, 'global', 'cosine', g, arch='slowfast'), False, "cpu", kernels=NumpyValidationKernels())
    short = loader(g)
    for i, (inp, tgt, idx) in enumerate(short):                              # 10 triplets: 20 rows to search, one too few
        short[i] = (tuple(t[:10] for t in inp), tuple(t[:10] for t in tgt), idx[:10])
    with pytest.raises(ValueError, match="more than 20 rows"):
        validate(short, net, crit, 0, cfg_for(None, 'local_batch', 'cosine', g), False, "cpu", kernels=NumpyValidationKernels())
    del short[1:]
    with pytest.raises(ValueError, match="more than 20 rows"):
        validate(short, net, crit, 0, cfg_for(None, 'global', 'cosine', g), False, "cpu", kernels=NumpyValidationKernels())
    with pytest.raises(NotImplementedError, match="plot=False"):
        k_nearest_embeddings(None, net.embeddingnet, False, "cpu", [], [], None, None, cfg_for(None, 'global', 'cosine', g))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.SlicError):
            validate(loader(g), net, crit, 0, cfg_for(None, 'global', 'cosine', g), False, "cpu")
        with pytest.raises(_lib.SlicError):
            topk_acc_device(g["knn_test"], g["knn_test_labels"], g["knn_train"], g["knn_train_labels"])


def embedding_loader(x, labels, batch):
    return [(torch.from_numpy(x[s:s + batch]), torch.from_numpy(labels[s:s + batch]), 0, torch.arange(s, min(s + batch, len(x))))
            for s in range(0, len(x), batch)]


@pytest.mark.parametrize("dm", ["cosine", "euclidean"])
def test_k_nearest_embeddings_vs_golden(golden_dir, tmp_path, capsys, dm):
    from video_similarity_search_amd.evaluate import k_nearest_embeddings
    from validate_cpu_kernels import NumpyValidationKernels
    g = golden(golden_dir)
    cfg = ns(OUTPUT_PATH=str(tmp_path), LOSS=ns(DIST_METRIC=dm), NUM_GPUS=1)
    train_loader = embedding_loader(g["knn_train"], g["knn_train_labels"], 32)
    test_loader = embedding_loader(g["knn_test"], g["knn_test_labels"], 16)
    capsys.readouterr()
    acc = k_nearest_embeddings(None, torch.nn.Identity(), False, "cpu", train_loader, test_loader, None, None, cfg, plot=False,
                               epoch=int(g["knn_epoch"]), kernels=NumpyValidationKernels())
    out = capsys.readouterr().out
    assert isinstance(acc, np.ndarray) and acc.dtype == np.float64 and np.array_equal(acc, g["knn_%s/acc" % dm])
    assert out == 'Getting embeddings...\nComputing top1/5/10/20 Acc...\n' + str(g["knn_%s/print" % dm]) + '\n'
    assert open(os.path.join(str(tmp_path), "tnet_checkpoints", "global_retrieval_acc.txt")).read() == str(g["knn_%s/file" % dm])
    # elsewhere than on the master: no search, no file, []
    acc = k_nearest_embeddings(None, torch.nn.Identity(), False, "cpu", train_loader, test_loader, None, None, cfg, plot=False,
                               epoch=8, is_master_proc=False, out_filename='other', kernels=NumpyValidationKernels())
    assert acc == [] and not os.path.exists(os.path.join(str(tmp_path), "tnet_checkpoints", "other.txt"))


# ---------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


GLOO_LOG_INTERVAL = 4          # world 2: log lines after batches 2 and 4, the fifth batch is read at the end


def _worker(rank, world, port, out_dir, golden_dir):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.distributed.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", world_size=world, rank=rank)
    try:
        from video_similarity_search_amd.validation import validate
        from video_similarity_search_amd.misc import distributed_helper as du_helper
        from validate_cpu_kernels import NumpyValidationKernels
        g = golden(golden_dir)
        reduces = []
        plain = du_helper.all_reduce
        du_helper.all_reduce = lambda tensors, avg=True: (reduces.append(len(tensors)), plain(tensors, avg=avg))[1]
        K = NumpyValidationKernels()
        d = os.path.join(out_dir, "rank%d" % rank)
        ret = validate(loader(g, rank, world), TorchTripletnet(encoder(g), 'cosine'), torch.nn.MarginRankingLoss(margin=float(g["margin"])),
                       int(g["epoch"]), cfg_for(d, 'global', 'cosine', g, world=world, log_interval=GLOO_LOG_INTERVAL), False, "cpu",
                       rank == 0, kernels=K)
        np.savez(os.path.join(out_dir, "res%d.npz" % rank), ret=ret, reads=K.reads, reduces=np.array(reduces))
    finally:
        torch.distributed.destroy_process_group()


def test_world_size_2_one_collective_per_read_back(golden_dir, tmp_path):
    g = golden(golden_dir)
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), golden_dir), nprocs=world, join=True)
    res = [dict(np.load(os.path.join(str(tmp_path), "res%d.npz" % r))) for r in range(world)]
    # the reference's arithmetic (validation.py:89-103) from the per-rank parts of the golden distances: per batch the mean over the
    # ranks of each rank's float32 loss / accuracy, weighted with the summed batch size
    margin = np.float32(g["margin"])
    da, db = g["global_cosine/dist_a"], g["global_cosine/dist_b"]
    s, loss_sum, acc_sum, n, gathered = 0, 0.0, 0.0, 0, []
    for b in g["sizes"]:
        parts = [rank_rows(s, int(b), r, world) for r in range(world)]
        l = [np.float32(np.maximum(da[p] - db[p] + margin, np.float32(0)).astype(np.float64).mean()) for p in parts]
        a = [np.float32((db[p] - da[p] > 0).sum() / np.float32(len(p))) for p in parts]
        bw = sum(len(p) for p in parts)
        loss_sum += float(np.float32(np.sum(l, dtype=np.float32) * np.float32(1.0 / world))) * bw
        acc_sum += float(np.float32(np.sum(a, dtype=np.float32) * np.float32(1.0 / world))) * bw
        n += bw
        gathered.extend(np.concatenate(parts))
        s += b
    assert abs(float(res[0]["ret"]) - acc_sum / n) <= 1e-6 and abs(float(res[1]["ret"]) - acc_sum / n) <= 1e-6
    # top-1 / top-5 over the gathered anchors (rank order within a batch), by the float64 provider's own rules
    from validate_cpu_kernels import topk64, label_hits
    with torch.no_grad():
        emb = encoder(g)(torch.from_numpy(g["clips"][0, gathered])).numpy()
    lab = g["targets"][0, gathered]
    hits = label_hits(topk64(emb, None, 20, 'cosine'), lab, lab, [1, 5, 10, 20])[1]
    top = [float(np.float32(h) / np.float32(len(lab))) for h in hits[:2]]
    assert val_file(os.path.join(str(tmp_path), "rank0")) == 'epoch:{} {:.4f} {:.2f} {:.2f} {:.2f}\n'.format(
        int(g["epoch"]), loss_sum / n, 100. * acc_sum / n, 100. * top[0], 100. * top[1])
    assert not os.path.exists(os.path.join(str(tmp_path), "rank1"))
    n_log = sum(1 for bi in range(len(g["sizes"])) if ((bi + 1) * world) % GLOO_LOG_INTERVAL == 0)
    for r in res:
        assert int(r["reads"]) == n_log + 1
        assert list(r["reduces"]) == [1] * (n_log + 1)          # ONE tensor, one collective per read-back

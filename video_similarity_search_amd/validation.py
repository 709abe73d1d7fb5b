"""
Drop-in for the reference's validation.py:12-151 — the per-epoch validation pass of online_train.py:730:

    validate(val_loader, tripletnet, criterion, epoch, cfg, cuda, device, is_master_proc=True, *, kernels=None)

Same loader contract ((anchor, positive, negative), (anchor_target, positive_target, negative_target), idx), eval() + no_grad,
the same printed lines at the same moments, the same line in tnet_checkpoints/val_loss_and_acc.txt, the same return value.

What changes is where the per-batch arithmetic runs and when the host looks at it.  After the three encoder passes ONE launch
(csrc/validate.hip: slic_triplet_val_batch) writes (loss, acc, B) into row `batch_idx` of a device-resident epoch record
[n_batches, 5] = (loss, acc, B, top1, top5).  VAL.METRIC 'local_batch' adds a device top-k search on cat(embedded_x, embedded_y) and
slic_topk_label_hits, whose counts become columns 3-4 of the row; 'global' keeps the anchor embeddings and labels on the device and runs
one search after the loop, whose result takes columns 3-4 of the LAST row.  The record is read back at a log point and once at the end;
the reference's AverageMeter arithmetic is then replayed on the host in batch order, so every printed number is the reference's.  With
cfg.NUM_GPUS > 1 the rows not yet reduced are all-reduced once per read-back (loss, acc, top1, top5 as mean, B as sum) instead of three
collectives per batch.

Two-view inputs (DATASET.MODALITY) and SlowFast inputs raise NotImplementedError.
"""
import torch

from . import _lib
from .misc import distributed_helper as du_helper
from .online_train import AverageMeter, _append_log

TOP_KS = [1, 5, 10, 20]                 # get_topk_acc's default: its np.argpartition(.., 20) needs more than 20 gallery rows
REC_LOSS, REC_ACC, REC_B, REC_TOP1, REC_TOP5 = range(5)


class HipValidationKernels(object):
    """the device side of validate(): `validate(kernels=)` takes another provider with the same four methods (the CPU suite drives the
    host logic with a float64 NumPy one).  `reads` counts read_record calls: the host synchronisations of an epoch."""

    def __init__(self):
        if not torch.cuda.is_available():
            raise _lib.SlicError("validate needs a gfx950 device (no CPU fallback)")
        _lib.load()
        self.reads = 0

    def val_batch(self, ex, ey, ez, euclid, margin, rec_row):
        """rec_row[0:3] = (MarginRankingLoss(margin) of the two rowwise distances, triplet accuracy, B)"""
        ex, ey, ez = (t.detach().float().contiguous() for t in (ex, ey, ez))
        _lib.require_device(ex, ey, ez, rec_row)
        _lib.call("slic_triplet_val_batch", _lib.ptr(ex), _lib.ptr(ey), _lib.ptr(ez), ex.shape[0], ex.shape[1], int(euclid),
                  float(margin), None, None, _lib.ptr(rec_row), _lib.stream())

    def topk(self, x, y, k, dist_metric):
        """[Nq, k] int32 indices of the k nearest rows of y (None: of x itself, diagonal excluded), on the device"""
        from .evaluate import _topk_search
        return _topk_search(dist_metric)(x, y, k=k)[0]

    def label_hits(self, idx, q_labels, g_labels, top_ks):
        """int32 [len(top_ks)] on the device: the number of query rows with a same-label gallery row among their first top_ks[i]"""
        from .evaluate import _label_hits
        return _label_hits(idx, q_labels, g_labels, top_ks)

    def read_record(self, rec):
        self.reads += 1
        return rec.cpu().numpy()


def _unwrap(embedded):
    return embedded[0] if isinstance(embedded, tuple) else embedded


def validate(val_loader, tripletnet, criterion, epoch, cfg, cuda, device, is_master_proc=True, *, kernels=None):
    metric = cfg.VAL.METRIC
    if cfg.DATASET.MODALITY == True:    # noqa: E712 (the reference's comparison)
        raise NotImplementedError("validate: two-view inputs (DATASET.MODALITY) are out of scope (DESIGN.md section 7)")
    if cfg.MODEL.ARCH == 'slowfast':
        raise NotImplementedError("validate: SlowFast multi-pathway inputs are out of scope (DESIGN.md section 7)")
    K = HipValidationKernels() if kernels is None else kernels       # raises SlicError without a gfx950 device

    losses = AverageMeter()
    accs = AverageMeter()
    top1_accs = AverageMeter()
    top5_accs = AverageMeter()
    embeddings, labels = [], []

    world_size = du_helper.get_world_size()
    net = getattr(tripletnet, "module", tripletnet)
    fused = isinstance(criterion, torch.nn.MarginRankingLoss) and criterion.reduction == 'mean'
    n_batches = len(val_loader)
    rec = torch.zeros(max(n_batches, 1), 5, dtype=torch.float32, device=device if cuda else "cpu")
    replayed = 0            # rows already all-reduced and fed to the meters

    def reduce_rows(upto):
        """the reference's per-batch all-reduces (validation.py:89-96) for rows replayed .. upto-1 as ONE collective"""
        if cfg.NUM_GPUS > 1 and upto > replayed:
            rows = rec[replayed:upto]
            du_helper.all_reduce([rows], avg=False)
            rows[:, [REC_LOSS, REC_ACC, REC_TOP1, REC_TOP5]] *= 1.0 / world_size

    def read_back(upto):
        """one device-to-host copy, then the reference's meter updates for rows replayed .. upto-1 in batch order"""
        nonlocal replayed
        host = K.read_record(rec)
        for r in host[replayed:upto]:
            batch_size_world = int(round(float(r[REC_B])))
            accs.update(float(r[REC_ACC]), batch_size_world)
            losses.update(float(r[REC_LOSS]), batch_size_world)
            if metric == 'local_batch':
                top1_accs.update(float(r[REC_TOP1]))
                top5_accs.update(float(r[REC_TOP5]))
        replayed = upto
        return host

    tripletnet.eval()
    with torch.no_grad():
        for batch_idx, (inputs, targets, idx) in enumerate(val_loader):
            (anchor, positive, negative) = inputs
            (anchor_target, positive_target, negative_target) = targets
            if cuda:
                anchor, positive, negative = anchor.to(device), positive.to(device), negative.to(device)
                anchor_target = anchor_target.to(device)
            row = rec[batch_idx]
            if fused:
                # Tripletnet.forward's three passes, then the distances, the loss and the accuracy in one launch
                embedded_x = _unwrap(net.embeddingnet(anchor)).flatten(1)
                embedded_y = _unwrap(net.embeddingnet(positive)).flatten(1)
                embedded_z = _unwrap(net.embeddingnet(negative)).flatten(1)
                euclid = getattr(net, "dist_metric", cfg.LOSS.DIST_METRIC) == 'euclidean'
                K.val_batch(embedded_x, embedded_y, embedded_z, euclid, criterion.margin, row)
            else:
                dista, distb, embedded_x, embedded_y, embedded_z = tripletnet(anchor, positive, negative)
                embedded_x, embedded_y = embedded_x.flatten(1), embedded_y.flatten(1)
                target = torch.full_like(dista, -1)
                row[REC_LOSS] = criterion(dista, distb, target)
                row[REC_ACC] = ((distb - dista) > 0).sum() * 1.0 / dista.size()[0]       # accuracy(), models/model_utils.py:232-235
                row[REC_B] = anchor.size(0)

            if metric == 'global':
                if cfg.NUM_GPUS > 1:
                    embedded_x, anchor_target = du_helper.all_gather([embedded_x, anchor_target])
                embeddings.append(embedded_x.detach())
                labels.append(anchor_target.detach())
            elif metric == 'local_batch':
                emb = torch.cat((embedded_x.detach(), embedded_y.detach()), dim=0)
                lab = torch.cat((anchor_target, positive_target.to(anchor_target.device)), dim=0)
                _check_rows(emb.shape[0])
                hits = K.label_hits(K.topk(emb, None, TOP_KS[-1], cfg.LOSS.DIST_METRIC), lab, lab, TOP_KS)
                row[REC_TOP1:REC_TOP5 + 1] = hits[:2].to(torch.float32) / emb.shape[0]
            else:
                print('Metric type:{} is not implemented'.format(metric))

            if ((batch_idx + 1) * world_size) % cfg.VAL.LOG_INTERVAL == 0:
                reduce_rows(batch_idx + 1)
                read_back(batch_idx + 1)
                if (is_master_proc):
                    msg = 'Val Epoch: {} [{}/{} | {:.1f}%]\t'\
                          'Loss: {:.4f} ({:.4f}) \t'\
                          'Triplet Acc: {:.2f}% ({:.2f}%)'.format(
                              epoch, losses.count,
                              len(val_loader.dataset), (losses.count*100./len(val_loader.dataset)),
                              losses.val, losses.avg,
                              accs.val*100., accs.avg*100.)

                    if metric == 'local_batch':
                        msg += '\t'
                        msg += 'Top1 Acc: {:.2f}% ({:.2f}%) \t'\
                               'Top5 Acc: {:.2f}% ({:.2f}%)'.format(
                                   top1_accs.val*100., top1_accs.avg*100.,
                                   top5_accs.val*100., top5_accs.avg*100.)
                    print(msg)

        reduce_rows(n_batches)
        if metric == 'global' and is_master_proc and embeddings:
            # Top 1/5 Acc over every anchor of the epoch: one search, its two fractions into the last row
            emb = torch.cat(embeddings, dim=0)
            lab = torch.cat(labels, dim=0)
            _check_rows(emb.shape[0])
            hits = K.label_hits(K.topk(emb, None, TOP_KS[-1], cfg.LOSS.DIST_METRIC), lab, lab, TOP_KS)
            rec[n_batches - 1, REC_TOP1:REC_TOP5 + 1] = hits[:2].to(torch.float32) / emb.shape[0]

    host = read_back(n_batches)
    if metric == 'global' and is_master_proc and embeddings:
        top1_accs.update(float(host[n_batches - 1, REC_TOP1]))
        top5_accs.update(float(host[n_batches - 1, REC_TOP5]))

    if (is_master_proc):
        # Log
        msg = '\nTest set: Average loss: {:.4f}, Triplet Accuracy: {:.2f}%'.format(losses.avg, accs.avg*100.)
        to_write = 'epoch:{} {:.4f} {:.2f}'.format(epoch, losses.avg, accs.avg*100.)
        if metric == 'global' or metric == 'local_batch':
            msg += ', '
            msg += 'Top1 Acc: {:.2f}% ({:.2f}%) \t'\
                   'Top5 Acc: {:.2f}% ({:.2f}%)'.format(100.*top1_accs.val, 100.*top1_accs.avg,
                                                        100.*top5_accs.val, 100.*top5_accs.avg)
            to_write += ' {:.2f} {:.2f}'.format(100.*top1_accs.avg, 100.*top5_accs.avg)

        to_write += '\n'
        print(msg)
        _append_log(cfg, 'val_loss_and_acc.txt', to_write)

    return accs.avg


def _check_rows(n):
    if n <= TOP_KS[-1]:
        raise ValueError("validate: the top-k accuracies need more than %d rows to search (get_topk_acc partitions every row of the "
                         "distance matrix at %d); got %d" % (TOP_KS[-1], TOP_KS[-1], n))

"""
Generates tests/golden/validation.npz by running the reference's own validation.validate (validation.py:12-151) on the CPU:
    python tests/golden/make_goldens_validation.py <directory of the reference checkout>
The packages the reference imports at module level and this environment lacks (fvcore, cv2, ...) and its dataset / config modules
are replaced by empty stand-ins BEFORE `import validation`; models.model_utils, models.triplet_net and evaluate's functions then
import for real, so AverageMeter, accuracy, Tripletnet, get_distance_matrix and get_topk_acc are the reference's.  joblib is not
touched (sklearn needs the real one).  Hard-coded .cuda() calls go through the oracle-only shim the other generators use.

Four cases, VAL.METRIC {global, local_batch} x LOSS.DIST_METRIC {cosine, euclidean}: a Flatten + Linear encoder, five batches of
12, 12, 11, 12, 12 triplets (the smaller one makes AverageMeter's n weighting visible), LOG_INTERVAL 2 (two log lines, the last batch
not on a log point).  Stored per case: the captured stdout lines, the file line, the return value, per batch dist_a, dist_b, loss,
acc.  Shared: encoder weights, all inputs and targets (numpy PCG64: the GPU machine regenerates nothing), the margin.
For k_nearest_embeddings (the reference function needs the dataset modules): get_distance_matrix + get_topk_acc on stored test /
train embeddings and labels, and the file line from the reference's format string.

The inputs must stay clear of near-ties, where float32 arithmetic could legitimately decide differently from the reference's;
asserted below in float64 — a violating seed is changed, rows are never dropped:
  * every top-k search has more than 20 gallery rows;
  * per query row the distance gaps between ranks 1|2, 5|6, 10|11, 20|21 exceed 1e-5;
  * per triplet |dist_b - dist_a| > 1e-5 and |dist_a - dist_b + margin| > 1e-5.
"""
import contextlib
import importlib.abc
import importlib.machinery
import io
import os
import sys
import tempfile
import types
sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn as nn

REFERENCE = os.path.abspath(sys.argv[1])
HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 2024
STUBS = ("fvcore", "cv2", "torchvision", "matplotlib", "seaborn", "PIL", "datasets", "spatial_transforms", "temporal_transforms",
         "config", "simplejson", "iopath", "psutil", "tensorboard", "kornia", "av", "pandas", "tqdm", "h5py", "skimage")


class _AnyMeta(type):
    def __getattr__(cls, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Any


class _Any(metaclass=_AnyMeta):
    """stands in for every name of a replaced module: a class (usable as a base), whose instances accept any call / attribute and
    work as pass-through decorators"""

    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Any()

    def __call__(self, *a, **k):
        if len(a) == 1 and not k and (isinstance(a[0], type) or callable(a[0])):
            return a[0]
        return _Any()


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Any


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, fullname, path, target=None):
        if fullname.split(".")[0] in STUBS:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        return _Stub(spec.name)

    def exec_module(self, module):
        pass


sys.meta_path.insert(0, _StubFinder())
sys.path.insert(0, REFERENCE)
torch.Tensor.cuda = lambda self, *a, **k: self              # oracle-only shim for hard-coded .cuda()
nn.Module.cuda = lambda self, *a, **k: self
import validation as ref_validation                                           # noqa: E402  (the reference)
from evaluate import get_distance_matrix, get_topk_acc                       # noqa: E402
from models.model_utils import accuracy                                      # noqa: E402
from models.triplet_net import Tripletnet                                    # noqa: E402

ns = types.SimpleNamespace
SIZES = [12, 12, 11, 12, 12]
CLIP = (3, 2, 4, 4)
FEAT, N_CLASSES, MARGIN, EPOCH, LOG_INTERVAL = 16, 6, 0.2, 3, 2
rng = np.random.default_rng(SEED)
W = (rng.standard_normal((FEAT, int(np.prod(CLIP)))) / np.sqrt(np.prod(CLIP))).astype(np.float32)
bias = (0.1 * rng.standard_normal(FEAT)).astype(np.float32)
N = sum(SIZES)
clips = rng.standard_normal((3, N) + CLIP).astype(np.float32)              # anchor, positive, negative
targets = rng.integers(0, N_CLASSES, (3, N)).astype(np.int64)
targets[1] = targets[0]                                                      # a positive shares its anchor's label
out = dict(enc_weight=W, enc_bias=bias, clips=clips, targets=targets, sizes=np.array(SIZES), margin=np.float32(MARGIN),
           epoch=np.int64(EPOCH), log_interval=np.int64(LOG_INTERVAL))


def encoder():
    m = nn.Sequential(nn.Flatten(), nn.Linear(W.shape[1], FEAT))
    with torch.no_grad():
        m[1].weight.copy_(torch.from_numpy(W))
        m[1].bias.copy_(torch.from_numpy(bias))
    return m


class Loader(list):
    dataset = range(N)


def loader():
    ld, s = Loader(), 0
    for b in SIZES:
        ld.append((tuple(torch.from_numpy(clips[i, s:s + b]) for i in range(3)),
                   tuple(torch.from_numpy(targets[i, s:s + b]) for i in range(3)), torch.arange(s, s + b)))
        s += b
    return ld


def dist64(x, y, metric):
    x, y = x.astype(np.float64), y.astype(np.float64)
    if metric == 'cosine':
        x = x / np.linalg.norm(x, axis=1, keepdims=True)
        y = y / np.linalg.norm(y, axis=1, keepdims=True)
        return 1.0 - x @ y.T
    return np.sqrt(((x[:, None, :] - y[None, :, :]) ** 2).sum(-1))


def assert_no_near_tie(d, what, self_search):
    d = d.copy()
    if self_search:
        np.fill_diagonal(d, np.inf)
    assert d.shape[1] - int(self_search) > 20, (what, d.shape)
    s = np.sort(d, axis=1)
    for r in (1, 5, 10, 20):
        gap = s[:, r] - s[:, r - 1]
        bad = np.flatnonzero(~(gap > 1e-5))
        assert not len(bad), "seed %d: %s row %d has a near-tie between ranks %d|%d" % (SEED, what, bad[0], r, r + 1)


class Recorder(nn.Module):
    """the criterion the reference calls, recording what it was called with"""

    def __init__(self):
        super().__init__()
        self.crit = nn.MarginRankingLoss(margin=MARGIN)
        self.rows = []

    def forward(self, dista, distb, target):
        loss = self.crit(dista, distb, target)
        self.rows.append((dista.numpy().copy(), distb.numpy().copy(), loss.item(), accuracy(dista, distb).item()))
        return loss


for metric in ("global", "local_batch"):
    for dm in ("cosine", "euclidean"):
        tag = "%s_%s" % (metric, dm)
        enc = encoder()
        with torch.no_grad():
            E = [enc(torch.from_numpy(clips[i])).numpy() for i in range(3)]
        da, db = (np.diag(dist64(E[0], E[i], dm)) for i in (1, 2))
        if dm == 'euclidean':
            da, db = (np.sqrt(((E[0].astype(np.float64) - E[i] + 1e-6) ** 2).sum(1)) for i in (1, 2))
        bad = np.flatnonzero((np.abs(db - da) <= 1e-5) | (np.abs(da - db + MARGIN) <= 1e-5))
        assert not len(bad), "seed %d: triplet %d sits on the accuracy's or the hinge's boundary" % (SEED, bad[0])
        if metric == "global":
            assert_no_near_tie(dist64(E[0], E[0], dm), tag, True)
        else:
            s = 0
            for b in SIZES:
                both = np.concatenate([E[0][s:s + b], E[1][s:s + b]])
                assert_no_near_tie(dist64(both, both, dm), "%s batch at %d" % (tag, s), True)
                s += b
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, "tnet_checkpoints"))
            cfg = ns(NUM_GPUS=1, OUTPUT_PATH=tmp, VAL=ns(METRIC=metric, LOG_INTERVAL=LOG_INTERVAL), LOSS=ns(DIST_METRIC=dm),
                     DATASET=ns(MODALITY=False), MODEL=ns(ARCH='3dresnet'))
            crit = Recorder()
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                ret = ref_validation.validate(loader(), Tripletnet(enc, dm), crit, EPOCH, cfg, False, "cpu", True)
            file_line = open(os.path.join(tmp, "tnet_checkpoints", "val_loss_and_acc.txt")).read()
        print(tag, repr(file_line))
        out[tag + "/stdout"] = np.array(buf.getvalue())
        out[tag + "/file"] = np.array(file_line)
        out[tag + "/return"] = np.float64(float(ret))
        out[tag + "/dist_a"] = np.concatenate([r[0] for r in crit.rows])
        out[tag + "/dist_b"] = np.concatenate([r[1] for r in crit.rows])
        out[tag + "/loss"] = np.array([r[2] for r in crit.rows], np.float64)
        out[tag + "/acc"] = np.array([r[3] for r in crit.rows], np.float64)

# ---- k_nearest_embeddings: test rows against train rows, clustered so that the accuracies are neither 0 nor 1
cen = rng.standard_normal((N_CLASSES, FEAT)).astype(np.float32)
knn_train_labels = rng.integers(0, N_CLASSES, 100).astype(np.int64)
knn_test_labels = rng.integers(0, N_CLASSES, 40).astype(np.int64)
knn_train = (cen[knn_train_labels] + 1.2 * rng.standard_normal((100, FEAT))).astype(np.float32)
knn_test = (cen[knn_test_labels] + 1.2 * rng.standard_normal((40, FEAT))).astype(np.float32)
out.update(knn_train=knn_train, knn_train_labels=knn_train_labels, knn_test=knn_test, knn_test_labels=knn_test_labels,
           knn_epoch=np.int64(7))
for dm in ("cosine", "euclidean"):
    assert_no_near_tie(dist64(knn_test, knn_train, dm), "knn " + dm, False)
    dmat = get_distance_matrix(torch.from_numpy(knn_test), torch.from_numpy(knn_train), dist_metric=dm)
    acc = get_topk_acc(dmat, knn_test_labels.tolist(), y_labels=knn_train_labels.tolist())
    out["knn_%s/acc" % dm] = np.asarray(acc, np.float64)
    # evaluate.py:372: two placeholders, four arguments
    out["knn_%s/file" % dm] = np.array('epoch:{} {:.2f} {:.2f}'.format(7, 100.*acc[0], 100.*acc[1], 100.*acc[2], 100.*acc[3]) + '\n')
    out["knn_%s/print" % dm] = np.array('Top1 Acc: {:.2f}%, Top5 Acc: {:.2f}%, Top10 Acc: {:.2f}%, Top20 Acc: {:.2f}%'.format(
        100.*acc[0], 100.*acc[1], 100.*acc[2], 100.*acc[3]))
    print("knn", dm, acc)

np.savez_compressed(os.path.join(HERE, "validation.npz"), **out)
print("wrote validation.npz", os.path.getsize(os.path.join(HERE, "validation.npz")), "bytes")

"""The parts of the reference's coclr_utils/utils.py that coclr_classify.py imports and that do arithmetic or printing:

    AverageMeter(name='null', fmt=':.4f')     running value / weighted average / average of the last `step` values / history
    ProgressMeter(num_batches, meters, prefix)
    neq_load_customized(model, pretrained_dict, verbose=True)
    calc_topk_accuracy, calc_mask_accuracy    re-exported from loss.classification and online_train, where they live

Written from their behaviour; the numbers and the printed text are the reference's.  The file helpers (save_checkpoint, write_log,
Logger) and the image de-normalisers are plain host code with nothing to port and are not repeated here.
"""
from collections import deque

import numpy as np

from ..loss.classification import calc_topk_accuracy          # noqa: F401
from ..online_train import calc_mask_accuracy                 # noqa: F401


class AverageMeter(object):
    """val: the last value; sum / count: weighted by n; avg = sum / count; local_avg: the mean of the last `step` values given with
    step > 0; history: the values given with history != 0.  An update with n == 0 moves val (and adds 0 to sum and count) and
    leaves everything else as it was."""

    def __init__(self, name='null', fmt=':.4f'):
        self.name, self.fmt = name, fmt
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0
        self.local_history = deque([])
        self.local_avg = 0
        self.history = []

    def update(self, val, n=1, history=0, step=5):
        self.val = val
        self.sum += val * n
        self.count += n
        if n == 0:
            return
        self.avg = self.sum / self.count
        if history:
            self.history.append(val)
        if step > 0:
            self.local_history.append(val)
            while len(self.local_history) > step:
                self.local_history.popleft()
            self.local_avg = np.average(self.local_history)

    def __len__(self):
        return self.count

    def __str__(self):
        return ('{name} {val' + self.fmt + '} ({avg' + self.fmt + '})').format(name=self.name, val=self.val, avg=self.avg)


class ProgressMeter(object):
    """display(i) prints prefix + '[  i/num_batches]' and every meter, tab-separated; i is padded to the digits of num_batches"""

    def __init__(self, num_batches, meters, prefix=""):
        digits = len(str(num_batches // 1))
        self.batch_fmtstr = '[{:' + str(digits) + 'd}/' + ('{:' + str(digits) + 'd}').format(num_batches) + ']'
        self.meters = meters
        self.prefix = prefix

    def display(self, batch):
        print('\t'.join([self.prefix + self.batch_fmtstr.format(batch)] + [str(m) for m in self.meters]))


def neq_load_customized(model, pretrained_dict, verbose=True):
    """load the entries of pretrained_dict whose names the model has and keep the model's own values for the rest; verbose lists both
    kinds of left-over names.  With verbose=False nothing is taken over, as in the reference (the selection sits inside its verbose
    branch)."""
    model_dict = model.state_dict()
    taken = {}
    if verbose:
        print('\n=======Check Weights Loading======')
        print('Weights not used from pretrained file:')
        for k, v in pretrained_dict.items():
            if k in model_dict:
                taken[k] = v
            else:
                print(k)
        print('---------------------------')
        print('Weights not loaded into new model:')
        for k in model_dict:
            if k not in pretrained_dict:
                print(k)
        print('===================================\n')
    model_dict.update(taken)
    model.load_state_dict(model_dict)
    return model

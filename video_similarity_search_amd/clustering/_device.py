"""
What every device provider of the cluster step opens with: the device check, resident rows and labels, a checked workspace.
Which form of the rows a caller takes:
    dense=False (a row-strided device view stays in place; the kernels take ld)   HipDbscanKernels, HipOpticsKernels, HipAggloKernels,
                                                                                  HipSilhouetteKernels
    dense=True  (always contiguous; the kernels take ld == D copies)              HipFinchKernels, HipKernels.to_device, fit_cluster
"""
import numpy as np
import torch

from .. import _lib


def require_device(who):
    _lib.load()
    if not torch.cuda.is_available():
        raise _lib.SlicError("{} needs a gfx950 device (no CPU fallback)".format(who))


def resident_rows(data, who, dense=False):
    """fp32 device rows [N, D] of an ndarray, a CPU tensor or a device tensor, with unit column stride (no copy when they already are)"""
    if torch.is_tensor(data):
        x = data.detach().to(device="cuda", dtype=torch.float32)
    else:
        x = torch.as_tensor(np.ascontiguousarray(data, dtype=np.float32)).cuda()
    if x.dim() != 2:
        raise ValueError("{} expects a 2-D array [n_samples, n_features], got shape {}".format(who, tuple(x.shape)))
    if dense or x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x


def resident_labels(labels):
    """int32 device labels with unit stride (no copy when they already are); `labels` is an int32 host array or a device tensor"""
    if torch.is_tensor(labels):
        x = labels.detach().to(device="cuda", dtype=torch.int32)
    else:
        x = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    return x.contiguous()


def workspace_bytes(size_fn_name, size_args, limits):
    """what the library's `*_workspace_bytes` entry point asks for; 0 means the sizes are outside what the call takes"""
    nbytes = getattr(_lib.load(), size_fn_name)(*size_args)
    if nbytes == 0:
        raise _lib.SlicError(limits)
    return nbytes


def sized_workspace(size_fn_name, size_args, device, tag, limits):
    return _lib.workspace(workspace_bytes(size_fn_name, size_args, limits), device, tag=tag)

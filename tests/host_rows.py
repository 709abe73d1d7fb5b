"""What the NumPy providers of the cluster step (tests/*_cpu_kernels.py) call "resident": host arrays.  Test infrastructure."""
import numpy as np


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else x


def host_rows(data, who):
    """contiguous float32 rows [N, D] of an ndarray or a tensor"""
    x = np.ascontiguousarray(np.asarray(_host(data), dtype=np.float32))
    if x.ndim != 2:
        raise ValueError("{} expects a 2-D array".format(who))
    return x


def host_labels(labels):
    """contiguous int32 labels of an ndarray or a tensor"""
    return np.ascontiguousarray(_host(labels), dtype=np.int32)

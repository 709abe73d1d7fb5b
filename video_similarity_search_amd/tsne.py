"""
The data path of the reference's embedding projection (tsne.py: the class subset, PCA(n_components=50), then
TSNE(n_components=2, perplexity=30)) on the MI355X.  No plotting: the caller gets the coordinates and the rows they belong to.
"""
import numpy as np
import torch

from .decomposition import PCA
from .manifold import TSNE


def tsne_projection(embeddings, labels, num_classes=101, n_class_subset=20, seed=42, perplexity=30, n_pca=50, pca_kernels=None,
                    tsne_kernels=None, **tsne_args):
    """-> (coords [M, 2] host fp32, row_mask [N] bool): the t-SNE coordinates of the rows whose label is in the class subset.
    The subset is the reference's: np.random.seed(seed); np.random.permutation(num_classes)[:n_class_subset] (drawn from a
    RandomState(seed) of its own: the same numbers, the global generator untouched).
    embeddings [N, D]: ndarray, CPU tensor, or device tensor; labels [N] integers.  The PCA keeps min(n_pca, D, M) components.
    pca_kernels / tsne_kernels: the providers of decomposition.PCA and manifold.TSNE; tsne_args go to TSNE."""
    lab = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if lab.ndim != 1 or lab.shape[0] != embeddings.shape[0]:
        raise ValueError("labels must be 1-D with one entry per embedding row: {} vs {}".format(lab.shape, tuple(embeddings.shape)))
    class_subset = np.random.RandomState(seed).permutation(num_classes)[:n_class_subset]
    row_mask = np.isin(lab, class_subset)
    M = int(row_mask.sum())
    if M < 2:
        raise ValueError("the class subset {} keeps {} rows; t-SNE needs at least 2".format(sorted(class_subset.tolist()), M))
    if torch.is_tensor(embeddings):
        rows = embeddings.detach()[torch.from_numpy(np.flatnonzero(row_mask)).to(embeddings.device)]
    else:
        rows = np.asarray(embeddings)[row_mask]
    pca = PCA(n_components=min(int(n_pca), rows.shape[1], M), kernels=pca_kernels)
    reduced = pca.fit_transform(rows, device=True)
    coords = TSNE(n_components=2, perplexity=perplexity, kernels=tsne_kernels, **tsne_args).fit_transform(reduced)
    return coords, row_mask

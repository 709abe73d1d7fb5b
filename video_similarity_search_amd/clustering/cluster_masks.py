"""
Drop-in for the reference's clustering/cluster_masks.py on the k-means path:
    preprocess_features_kmeans(data)                                   <- cluster_masks.py:30-34
    fit_cluster(embeddings, method, k, l2normalize, finch_partition)   <- cluster_masks.py:38-98
Same names, argument meaning, prints and return type (np.ndarray[N] labels).  method='kmeans'
(SURVEY.md §8 A5/A6), method='finch' (§8f row 1: the method the shipped configs select) and
method='DBSCAN' (cosine, clustering/dbscan.py) run on the GPU, and so does method='Agglomerative' (average linkage, cosine,
clustering/agglomerative.py) once the caller states its distance_threshold, and method='OPTICS' (cosine, cluster_method='dbscan',
clustering/optics.py) once the caller states its max_eps.  method='HDBSCAN' (cosine, clustering/hdbscan.py; not in the reference) is the
density method that needs no radius.
"""
import torch

from ._device import require_device, resident_rows
from .kmeans_hip import HipKernels, KMeans

_METHODS = ['DBSCAN', 'Agglomerative', 'OPTICS', 'kmeans', 'spherical_kmeans', 'finch', 'HDBSCAN']


def _to_device(embeddings):
    require_device("fit_cluster")
    return resident_rows(embeddings, "fit_cluster", dense=True)


def preprocess_features_kmeans(data, kernels=None):
    """row L2-normalise: data / torch.norm(data, dim=1, keepdim=True) (no epsilon), on the device.
    Returns a tensor on the device the data ended up on (CPU input is moved to the current GPU)."""
    if kernels is None:
        kernels = HipKernels()
        x = _to_device(data)
    else:                                   # explicit kernel provider (see KMeans(kernels=...)): tests of the host logic
        x = kernels.to_device(data)
    out = torch.empty_like(x)
    kernels.l2norm_rows(x, out)
    print('l2-normalized data')
    return out


def fit_cluster(embeddings, method='Agglomerative', k=1000, l2normalize=True, finch_partition=0,
                n_init=10, init='k-means++', process_group=None, random_state=None, kernels=None, exchange=None,
                *, eps=0.14, min_samples=None, distance_threshold=None, max_eps=None, precision=None, min_cluster_size=5):
    """Reference signature + keyword-only extras (n_init / init / process_group / random_state / kernels / exchange / eps /
    min_samples) that default to the reference's behaviour: KMeans(n_clusters=k, n_init=10).fit(embeddings).labels_, and for
    method='DBSCAN' DBSCAN(eps=0.14, min_samples=2, metric='cosine').fit(embeddings).labels_ (noise = -1; l2normalize does not
    apply, as in the reference; `kernels` is then a DBSCAN provider, see clustering/dbscan.py).
    method='Agglomerative' with distance_threshold=t runs AgglomerativeClustering(n_clusters=None, linkage='average',
    distance_threshold=t, metric='cosine').fit(embeddings).labels_ (clustering/agglomerative.py: sklearn's partition, clusters numbered
    by their smallest row; `kernels` is then an agglomerative provider).  The reference's t is the hand-tuned constant 0.24 ("0.24 for
    ucf train", cluster_masks.py:52): the caller states it; without it the method raises NotImplementedError.
    method='OPTICS' with max_eps=e runs OPTICS(min_samples=3, max_eps=e, cluster_method='dbscan', metric='cosine').fit(embeddings).labels_
    (clustering/optics.py; `kernels` is then an OPTICS provider).  The reference's e is the hand-tuned 0.20 (cluster_masks.py:88-89, "0.18
    for ucf val, 0.14 for ucf train, 0.12 for kin train"): the caller states it; without it the method raises NotImplementedError.
    min_samples=None is the reference's own value for the method: 2 for 'DBSCAN', 3 for 'OPTICS'.
    method='HDBSCAN' runs HDBSCAN(min_cluster_size=min_cluster_size, min_samples=min_samples, metric='cosine').fit(embeddings).labels_
    (clustering/hdbscan.py: sklearn's partition, clusters numbered by their smallest row, noise = -1; no radius to state;
    min_samples=None is min_cluster_size, as in sklearn; l2normalize does not apply; `kernels` is then an HDBSCAN provider).
    process_group: `embeddings` is this rank's row shard (rank order == row order), the returned labels are this rank's.
    exchange: the sharded Lloyd iteration's one collective — 'allreduce' (RCCL through torch.distributed; the default), 'allgather', or
    'oneshot' (the library's one-shot all-to-all over peer-mapped memory, csrc/oneshot.hip); None reads SLIC_KMEANS_EXCHANGE.
    precision ('kmeans' / 'spherical_kmeans'): 'fp32', 'bf16' (the certified bf16 E-step: the same labels) or None, see KMeans."""

    assert (method in _METHODS)
    if precision not in (None, "fp32", "bf16"):
        raise ValueError(f"precision={precision!r}: 'fp32' or 'bf16'")
    print("Clustering with {}...".format(method))
    if method == 'finch':
        # cluster_masks.py:79-86: FINCH(embeddings, distance='cosine'), take partition `finch_partition`
        from .finch import FINCH
        c, num_clust, req_c = FINCH(embeddings, distance='cosine')      # rows go to (or stay on) the device once
        PARTITION = finch_partition
        labels = c[:, PARTITION]
        n_clusters = num_clust[PARTITION]
        print('Taking partition {} from finch'.format(PARTITION))
        print("Fitted " + str(n_clusters) + " clusters with " + str(method))
        return labels
    if method == 'DBSCAN':
        # cluster_masks.py:55-61: DBSCAN(eps=0.14, min_samples=2, metric='cosine', n_jobs=-1).fit(embeddings)
        from .dbscan import DBSCAN
        km = DBSCAN(eps=eps, min_samples=2 if min_samples is None else min_samples, metric='cosine', kernels=kernels).fit(embeddings)
    elif method == 'HDBSCAN':
        from .hdbscan import HDBSCAN
        km = HDBSCAN(min_cluster_size=min_cluster_size, min_samples=min_samples, metric='cosine', kernels=kernels).fit(embeddings)
    elif method == 'OPTICS' and max_eps is not None:
        # cluster_masks.py:88-89: OPTICS(min_samples=3, max_eps=0.20, cluster_method='dbscan', metric='cosine', n_jobs=-1).fit(embeddings)
        from .optics import OPTICS
        km = OPTICS(min_samples=3 if min_samples is None else min_samples, max_eps=max_eps, cluster_method='dbscan', metric='cosine',
                    kernels=kernels).fit(embeddings)
    elif method == 'Agglomerative' and distance_threshold is not None:
        # cluster_masks.py:49-54: AgglomerativeClustering(n_clusters=None, linkage='average', distance_threshold=0.24, affinity='cosine')
        from .agglomerative import AgglomerativeClustering
        km = AgglomerativeClustering(n_clusters=None, linkage='average', distance_threshold=distance_threshold, metric='cosine',
                                     kernels=kernels).fit(embeddings)
    elif method not in ('kmeans', 'spherical_kmeans'):
        raise NotImplementedError(
            f"method={method!r}: 'kmeans', 'spherical_kmeans', 'finch' and 'DBSCAN' are on the MI355X hot path, and so is 'Agglomerative' "
            "when the keyword distance_threshold= is given (the reference's hand-tuned 0.24 is not assumed) and 'OPTICS' when the keyword "
            "max_eps= is given (the reference's hand-tuned 0.20 is not assumed)")
    elif method == 'spherical_kmeans':
        x = _to_device(embeddings) if kernels is None else kernels.to_device(embeddings)
        # cluster_masks.py:73-77: SphericalKMeans(n_clusters=k).fit(embeddings) (spherecluster: normalises the rows itself,
        # n_init=10, k-means++, centres renormalised every iteration).  spherecluster is not vendored: parity unpinned.
        print('clustering with spherical kmeans with k={}'.format(k))
        print(tuple(x.shape))
        km = KMeans(n_clusters=k, n_init=n_init, init=init, process_group=process_group, random_state=random_state,
                    spherical=True, kernels=kernels, exchange=exchange, precision=precision).fit(x)
    else:
        x = _to_device(embeddings) if kernels is None else kernels.to_device(embeddings)
        print("k:", k)
        if l2normalize:
            x = preprocess_features_kmeans(x, kernels)
        km = KMeans(n_clusters=k, n_init=n_init, init=init, process_group=process_group,
                    random_state=random_state, kernels=kernels, exchange=exchange, precision=precision).fit(x)
    labels = km.labels_
    print(labels.shape)
    n_clusters = len(set(labels.tolist())) - (1 if -1 in labels else 0)
    print("Fitted " + str(n_clusters) + " clusters with " + str(method))
    fit_cluster.last_model = km
    return labels

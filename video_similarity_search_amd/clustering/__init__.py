from .agglomerative import AgglomerativeClustering  # noqa: F401
from .cluster_masks import fit_cluster, preprocess_features_kmeans  # noqa: F401
from .hdbscan import HDBSCAN  # noqa: F401
from .kmeans_hip import KMeans  # noqa: F401
from .optics import OPTICS, cluster_optics_dbscan  # noqa: F401
from .metrics import adjusted_mutual_info_score, cluster_scores, normalized_mutual_info_score  # noqa: F401
from .metrics import silhouette_report, silhouette_samples, silhouette_score  # noqa: F401

"""
Generates tests/golden/silhouette.npz from scikit-learn (1.7.2) on FLOAT64 input: for every case of tests/silhouette_cases.py and
both metrics, sklearn.metrics.silhouette_samples, silhouette_score and the sample_size=200, random_state=3 score.
    python tests/golden/make_goldens_silhouette.py
The inputs are NOT stored: the tests redraw them from the seed (silhouette_cases.draw) and compare the stored checksum.
"""
import os
import sys
sys.dont_write_bytecode = True
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from silhouette_cases import GOLDEN_CASES, METRICS, checksum, draw          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    from sklearn.metrics import silhouette_samples, silhouette_score
    out = {}
    for name, (seed, N, D, K, spread) in GOLDEN_CASES.items():
        x, labels = draw(seed, N, D, K, spread)
        out[name + "__checksum"] = np.frombuffer(checksum(x, labels).encode(), dtype=np.uint8)
        x64 = x.astype(np.float64)
        for metric in METRICS:
            out["{}__{}__samples".format(name, metric)] = silhouette_samples(x64, labels, metric=metric)
            out["{}__{}__score".format(name, metric)] = np.float64(silhouette_score(x64, labels, metric=metric))
            out["{}__{}__score200".format(name, metric)] = np.float64(
                silhouette_score(x64, labels, metric=metric, sample_size=200, random_state=3))
            print(name, metric, out["{}__{}__score".format(name, metric)], out["{}__{}__score200".format(name, metric)])
    np.savez_compressed(os.path.join(HERE, "silhouette.npz"), **out)


if __name__ == "__main__":
    main()

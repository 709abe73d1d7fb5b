"""
Records tests/golden/pair_stats_cluster_step_parent.json: provider calls, stdout, log files, labels and NMI of one
iterative_cluster_step (DBSCAN, 60 x 8 rows, recorded NumPy providers; tests/pair_stats_cases.py) with NO cfg.ITERCLUSTER.PAIR_STATS
attribute.  It was run on the commit before the pair-statistics lines were added to the step, and the test holds the step with the flag
absent or 0 to it.
    python tests/golden/make_goldens_pair_stats_cluster_step.py
"""
import json
import os
import sys
import tempfile
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from pair_stats_cases import run_step_recorded          # noqa: E402

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        rec = run_step_recorded(os.path.join(d, "step"))
    with open(os.path.join(HERE, "pair_stats_cluster_step_parent.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(rec["calls"])
    print(rec["stdout"])

"""TEST-ONLY: the hand-made [Nq, k] tables the CPU and GPU tests of slic_knn_vote / slic_retrieval_ranked share.  Seeded, no files."""
import numpy as np

# (k, Nq, C, n_top): every k that takes another path (one lane, a part chunk, a whole chunk, a chunk and one, the searches' limit, two
# chunks and a bit), a single query, a part workgroup (5 = 4 + 1, 97 = 24 * 4 + 1), C below / at / one past a lane sweep and the
# limit, n_top above C
VOTE_CASES = [(1, 97, 65, 5), (5, 97, 65, 5), (64, 97, 65, 5), (65, 97, 65, 5), (88, 97, 65, 5), (130, 97, 65, 5),
              (88, 1, 64, 1), (88, 5, 64, 8), (5, 1, 1, 1),
              (20, 5, 1, 5), (20, 97, 2, 8), (65, 5, 64, 8), (130, 5, 4096, 8), (88, 97, 4096, 1), (1, 1, 2, 8)]
NG_VOTE = 300


def vote_case(k, Nq, C, seed=0):
    """-> idx [Nq, k] int32, dist [Nq, k] float32 ascending, g_labels [NG_VOTE] int64.  In it: padding (-1 and rows >= Ng) in the
    middle and at the end of rows, one row of nothing but padding, gallery labels < 0 and >= C, rows that open with several zero
    distances, and rows whose distances are powers of two so that inverse-distance scores of two classes tie exactly."""
    rng = np.random.default_rng(1000 * k + 10 * Nq + C + seed)
    g_labels = rng.integers(-2, C + 2, NG_VOTE).astype(np.int64)          # -2, -1 and C, C + 1 never vote
    g_labels[:8] = np.arange(8) % C                                      # some rows certainly vote
    idx = rng.integers(0, NG_VOTE, (Nq, k)).astype(np.int32)
    dist = np.sort(rng.uniform(0.05, 2.0, (Nq, k)).astype(np.float32), axis=1)
    for q in range(Nq):
        kind = q % 6
        if kind == 1:                                                     # padding in the middle
            idx[q, rng.integers(0, k, max(1, k // 4))] = -1
        elif kind == 2:                                                   # padding at the end, some of it past the gallery
            cut = int(rng.integers(0, k))
            idx[q, cut:] = -1
            idx[q, cut + (k - cut) // 2:] = NG_VOTE + 5
            dist[q, cut:] = np.inf
        elif kind == 3:                                                   # several zero distances open the row
            dist[q, :min(k, 3)] = 0.0
        elif kind == 4:                                                   # powers of two: exact sums, exact ties between classes
            dist[q] = np.sort(np.exp2(rng.integers(-2, 2, k)).astype(np.float32))
            idx[q] = rng.integers(0, 8, k)                                # rows 0 .. 7: classes 0 .. min(8, C) - 1
    if Nq > 1:
        idx[Nq - 1] = -1                                                  # nobody votes
        if Nq > 2:
            idx[Nq - 2] = np.where(np.arange(k) % 2 == 0, -1, 1)          # one voting row at every other rank
    return idx, dist, g_labels


# (k, Nq, cut-offs): one lane, a whole chunk, a chunk and one, two chunks and a bit; cut-offs on both sides of the 64-lane boundary
RANKED_CASES = [(1, 1, (1,)), (1, 97, (1,)), (64, 97, (1, 5, 63, 64)), (65, 97, (1, 64, 65)), (130, 97, (1, 5, 10, 20, 64, 65, 128, 130)),
                (130, 1, (64, 65)), (88, 97, (1, 5, 10, 20, 50, 88))]
NG_RANKED = 400


def ranked_case(k, Nq, ks, seed=0):
    """-> idx [Nq, k] int32, q_labels [Nq], g_labels [NG_RANKED] int64, n_rel [Nq] int32.  Queries cycle through: relevant rows
    scattered over the list, no hit at all with n_rel = 0, no hit with n_rel > 0, one relevant row, n_rel = K - 1 / K / more than K for
    the largest cut-off (every one of them in the list), and a row padded from its middle on."""
    rng = np.random.default_rng(77 * k + Nq + seed)
    K = ks[-1]
    g_labels = rng.integers(0, 6, NG_RANKED).astype(np.int64)
    g_labels[:150] = 9                                                    # 150 rows of class 9: enough for n_rel > 130
    q_labels = rng.integers(0, 6, Nq).astype(np.int64)
    idx = rng.integers(150, NG_RANKED, (Nq, k)).astype(np.int32)
    n_rel = np.zeros(Nq, np.int32)
    for q in range(Nq):
        kind = q % 8
        if kind == 0:
            n_rel[q] = (g_labels == q_labels[q]).sum()
        elif kind == 1:                                                   # a label the gallery does not hold
            q_labels[q] = 77
        elif kind == 2:                                                   # relevant rows exist, none was found
            q_labels[q] = 9
            n_rel[q] = 150
        elif kind in (3, 4, 5, 6):                                        # class 9 with exactly n hits in the list
            q_labels[q] = 9
            n = {3: 1, 4: max(K - 1, 0), 5: K, 6: K}[kind]
            n = min(n, k)
            pos = rng.choice(k, n, replace=False)
            idx[q, pos] = rng.choice(150, n, replace=False)
            n_rel[q] = {3: 1, 4: K - 1, 5: K, 6: K + 7}[kind]
        else:
            n_rel[q] = (g_labels == q_labels[q]).sum()
            idx[q, k // 2:] = -1
    return idx, q_labels, g_labels, n_rel

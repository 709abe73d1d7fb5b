"""CPU: the euclidean top-k entry points answer without a device — the workspace size, and a loud error instead of a host fallback."""
import pytest


def test_euclidean_topk_workspace_covers_padded_copies():
    from video_similarity_search_amd import _lib
    lib = _lib.load()
    for Nq, Ng, D, k in ((10000, 100000, 512, 50), (33, 257, 40, 7), (1, 50, 5, 50), (300, 40000, 200, 88)):
        Dp = (D + 7) // 8 * 8
        b = lib.slic_euclidean_topk_workspace_bytes(Nq, Ng, D, k)
        assert b > 0
        # centred, padded copies of both sets + the half norms, besides the search's own workspace
        assert b >= 4 * (Nq * Dp + Ng * Dp + Ng) + Nq * min(k, 88) * 4


def test_euclidean_topk_without_gpu_raises():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.evaluate import euclidean_topk
    with pytest.raises(_lib.SlicError):
        euclidean_topk(torch.randn(4, 8), torch.randn(40000, 8), k=20)
    with pytest.raises(_lib.SlicError):
        euclidean_topk(torch.randn(40, 8), None, k=5)

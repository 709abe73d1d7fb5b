"""CPU: the certified bf16 candidate search's ABI, its plan query and — on a host emulation of what the kernel computes (rows rounded
to bf16 with round-to-nearest-even, exact products, fp32 accumulation) — the error bound eps its certificate rests on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

NAMES = ["slic_cosine_topk_bf16_workspace_bytes", "slic_cosine_topk_bf16_plan", "slic_cosine_topk_bf16", "slic_cosine_topk_bf16_eps"]
U = 2.0 ** -8            # unit roundoff of bf16: 8 significant bits, spacing 2^-7 in [1, 2), round to nearest


def test_header_table_and_library_agree():
    from video_similarity_search_amd import _lib
    txt = open(os.path.join(ROOT, "include", "slic_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, txt), n
        assert n in _lib.SIGNATURES, n
        assert hasattr(lib, n), n
    assert len(_lib.SIGNATURES["slic_cosine_topk_bf16"][1]) == 12
    assert _lib.SIGNATURES["slic_cosine_topk_bf16_eps"] == (ctypes.c_float, [])


def test_plan_answers_without_a_device(monkeypatch):
    from video_similarity_search_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int * 6)()
    monkeypatch.setenv("SLIC_TOPK_BF16", "1")
    assert lib.slic_cosine_topk_bf16_plan(10000, 100000, 512, 50, out) == 0
    assert out[0] == 1 and out[1] == 2048 and out[2] == 512
    assert lib.slic_cosine_topk_bf16_plan(65, 32781, 104, 1, out) == 0        # the switch reaches k = 1; a row of 104 columns is padded to 112
    assert out[0] == 1 and out[2] == 112
    ws1 = lib.slic_cosine_topk_bf16_workspace_bytes(65, 32781, 104, 1)
    assert ws1 >= (65 + 32781) * 112 * 2                                       # room for both bf16 images
    for Nq, Ng, D, k in [(100, 20000, 128, 20), (100, 40000, 520, 20)]:        # outside the collect path's domain: off even when forced
        assert lib.slic_cosine_topk_bf16_plan(Nq, Ng, D, k, out) == 0 and out[0] == 0
        assert lib.slic_cosine_topk_bf16_workspace_bytes(Nq, Ng, D, k) == lib.slic_cosine_topk_workspace_bytes(Nq, Ng, k)
    monkeypatch.delenv("SLIC_TOPK_BF16")                                       # the library's own choice: where the bf16 pass measured faster
    for shape, on in [((10000, 100000, 512, 50), 1), ((10000, 100000, 128, 1), 1), ((10000, 100000, 512, 88), 0),
                      ((1000, 100000, 512, 50), 0), ((10000, 100000, 64, 16), 0)]:
        assert lib.slic_cosine_topk_bf16_plan(*shape, out) == 0 and out[0] == on, shape
    monkeypatch.setenv("SLIC_TOPK_BF16", "0")
    assert lib.slic_cosine_topk_bf16_plan(10000, 100000, 512, 50, out) == 0 and out[0] == 0
    assert lib.slic_cosine_topk_bf16_plan(0, 100000, 512, 50, out) != 0
    assert b"slic_cosine_topk_bf16_plan" in lib.slic_last_error()


def test_eps_is_the_library_value():
    from video_similarity_search_amd import _lib, evaluate
    assert evaluate.TOPK_BF16_EPS == float(_lib.load().slic_cosine_topk_bf16_eps())
    assert evaluate.TOPK_BF16_EPS == float(np.float32(0.008))
    # the derivation of DESIGN.md: (2u + u^2) S + gamma_D (1 + u)^2 S (the MFMA's fp32 accumulation) + gamma_D S (the fp32 rescore),
    # S <= (1 + 2^-20)^2, D = 512, gamma_D taken with a unit roundoff of 2^-23 per addition (covers a truncating adder)
    g = 512 * 2.0 ** -23 / (1 - 512 * 2.0 ** -23)
    assert ((2 * U + U * U) + g * (1 + U) ** 2 + g) * (1 + 2.0 ** -20) ** 2 < evaluate.TOPK_BF16_EPS


def _unit(x):
    x = x.double()
    return (x / x.norm(dim=1, keepdim=True)).float()


def _coarse_minus_exact(q, g):
    """max |c - s|: c from bf16 rows (exactly representable products, summed in fp32), s in float64 from the fp32 rows"""
    c = q.bfloat16().float() @ g.bfloat16().float().T
    s = q.double() @ g.double().T
    return (c.double() - s).abs().max().item()


def _midpoint_row(D):
    """a row of norm just below 1 whose every entry is a tie between two bf16 numbers, at the bottom of its binade: 2^e (1 + 2^-8).
    Rounding (to even: down) moves each by the relative 2^-8 / (1 + 2^-8), nearly the whole unit roundoff, and all in one direction.
    The exponents are the base-4 digits of the norm budget, largest first; entries left over are negligibly small ties."""
    T = (1.0 + 2.0 ** -8) ** -2                              # sum of 4^e_i that makes the norm exactly 1
    acc, ex = 0.0, []
    for _ in range(D):
        rem = T - acc
        e = int(np.floor(np.log2(rem) / 2)) if rem > 4.0 ** -40 else -40
        e = max(e, -40)
        ex.append(e)
        acc += 4.0 ** e
    x = torch.tensor([2.0 ** e * (1.0 + 2.0 ** -8) for e in ex], dtype=torch.float64)
    return x.float()[None, :]


@pytest.mark.parametrize("D", [8, 104, 512])
def test_host_emulation_stays_inside_eps(D):
    from video_similarity_search_amd import evaluate
    eps = evaluate.TOPK_BF16_EPS
    rng = np.random.default_rng(D)
    tg = torch.Generator().manual_seed(D)
    q = _unit(torch.randn(256, D, generator=tg))
    g = _unit(torch.randn(4096, D, generator=tg))
    e_flat = _coarse_minus_exact(q, g)
    cent = torch.randn(40, D, generator=tg)
    gc = _unit(cent[torch.from_numpy(rng.integers(0, 40, 4096))] + 0.05 * torch.randn(4096, D, generator=tg))
    qc = _unit(gc[:256] + 0.3 * torch.randn(256, D, generator=tg))
    e_clu = _coarse_minus_exact(qc, gc)
    m = _midpoint_row(D)
    assert torch.equal(m.double().float(), m)
    n2 = float((m.double() ** 2).sum())                     # |q| |g| of q = g = m
    assert 0.97 < n2 <= 1.0 + 2.0 ** -20
    e_mid = _coarse_minus_exact(m, m)
    print("D=%d  max|c-s|: gaussian %.3e  clustered %.3e  midpoint %.3e (|m|^2 = %.6f, 2u = %.3e)  eps %.3e"
          % (D, e_flat, e_clu, e_mid, n2, 2 * U, eps))
    assert e_flat <= eps and e_clu <= eps and e_mid <= eps
    assert e_mid > 0.9 * 2 * U                              # the bound is tight: the constant is not padded


def test_unknown_precision_raises():
    from video_similarity_search_amd.evaluate import cosine_topk, euclidean_topk, topk_retrieval, topk_acc_device
    x = torch.randn(4, 8)
    with pytest.raises(ValueError):
        cosine_topk(x, x, k=2, precision="int8")
    with pytest.raises(ValueError):
        topk_acc_device(x, [0, 1, 0, 1], precision="int8")
    with pytest.raises(ValueError):
        topk_retrieval(X_train=x.numpy(), y_train=np.arange(4), X_test=x.numpy(), y_test=np.arange(4), ks=[1], precision="int8")
    with pytest.raises(ValueError):
        euclidean_topk(x, x, k=2, precision="bf16")         # unit rows only: see its docstring

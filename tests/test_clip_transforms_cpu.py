"""CPU: the host side of coclr_utils.transforms — planner, random draws, errors — with the NumPy provider
(tests/clip_transforms_cpu_kernels.py) as `kernels=`, against the reference's goldens (tests/golden/clip_transforms.npz, cases in
tests/clip_transforms_cases.py).

Gates.  Crop, centre crop, flip, pad, both to-float forms, normalise, brightness, saturation, gray and any chain of them: bit
equality (the provider rounds every operation as the reference's separate torch ops do).  Contrast and resize, and chains containing
them: 4 x the stored deviation of the reference's fp32 result from the same chain in float64, floored at 2^-23 for unit-range data
(divided by min(std) after Normalize): the mean's summation order and the order of the bilinear products are not the reference's."""
import os
import random

import numpy as np
import pytest
import torch

import clip_transforms_cases as cases
from clip_transforms_cpu_kernels import NumpyClipKernels
from conftest import GOLDEN
from video_similarity_search_amd import _lib
from video_similarity_search_amd.coclr_utils import transforms as T

G = np.load(os.path.join(GOLDEN, "clip_transforms.npz"))


def seed(s):
    random.seed(s)
    np.random.seed(s)


def compose(kern):
    return lambda ts: T.Compose(ts, kernels=kern)


def check_case(case, out):
    name, key, s, kind, build = case
    ref = G[f"out_{name}"]
    out = out.cpu().numpy()
    assert out.dtype == np.float32 and out.shape == ref.shape
    if kind == "eq":
        assert np.array_equal(out, ref), f"{name}: max |diff| {np.abs(out - ref).max():.3e}"
    else:
        tol = cases.gate(kind, G[f"dev_{name}"])
        err = float(np.abs(out.astype(np.float64) - ref).max())
        print(f"{name}: max |diff| {err:.3e}, gate {tol:.3e}")
        assert err <= tol, f"{name}: {err:.3e} > {tol:.3e}"


@pytest.mark.parametrize("case", cases.CASES, ids=[c[0] for c in cases.CASES])
def test_goldens_through_the_numpy_provider(case):
    name, key, s, kind, build = case
    assert int(G[f"seed_{name}"]) == s
    seed(s)
    out = cases.run_case(build, T, compose(NumpyClipKernels()), T.Lambda, key, G[f"in_{key}"])
    nxt = (random.random(), np.random.uniform())
    assert nxt == tuple(G[f"next_{name}"]), "the generators are not in the reference's state after the call"
    check_case(case, out)


def test_all_six_jitter_orders_occur():
    x = torch.from_numpy(G["in_fs"])
    orders = set()
    for s in range(12):
        seed(s)
        prog = T.Compose([T.ColorJitter(0.4, 0.4, 0.4, consistent=True)], kernels=NumpyClipKernels()).plan(x)
        ops = [k for g in prog.groups() for k, _ in g.ops]
        assert sorted(ops) == [T.BRIGHTNESS, T.CONTRAST, T.SATURATION]
        orders.add(tuple(ops))
    assert len(orders) == 6, orders


def bench_chain(kern, contrast=True, size=(8, 10)):
    return T.Compose([T.ToFloatTensorInZeroOne(), T.RandomSizedCrop(size), T.RandomHorizontalFlip(),
                      T.ColorJitter(0.4, 0.4 if contrast else 0, 0.4, consistent=True), T.RandomGray(0.9), T.Normalize(cases.MEAN, cases.STD)],
                     kernels=kern)


def test_planner_groups_and_launches():
    x = torch.from_numpy(G["in_u5"])
    for contrast, want in ((True, ("stats", "apply")), (False, ("apply",))):
        kern = NumpyClipKernels()
        seed(3)
        chain = bench_chain(kern, contrast)
        groups = chain.plan(x).groups()
        assert len(groups) == 1 and groups[0].launches == want
        g = groups[0]
        assert g.kind == T.SRC_U8_255 and g.resample is not None and g.norm is not None and g.out_hw == (8, 10)
        assert [k for k, _ in g.ops][-1] == T.GRAY and len(g.ops) == (4 if contrast else 3)
        seed(3)
        chain(x)
        assert kern.launches == [want]
    kern = NumpyClipKernels()
    two = T.Compose([T.ToFloatTensorInZeroOne(), T.Resize((8, 10)), T.Resize((12, 9))], kernels=kern)
    assert [g.launches for g in two.plan(x).groups()] == [("apply",), ("apply",)]
    two(x)
    assert kern.launches == [("apply",), ("apply",)]
    # geometry after a colour op, two contrast ops, a fifth colour op, a pad with another fill over a visible one: a new group each
    f = torch.from_numpy(G["in_f13"])
    ones = torch.ones(3, dtype=torch.float64)
    split = T.Compose([T.Lambda(lambda v: T.adjust_brightness(v, ones)), T.RandomHorizontalFlip(p=1.0)], kernels=kern)
    assert len(split.plan(f).groups()) == 2
    split = T.Compose([T.Lambda(lambda v: T.adjust_contrast(v, ones))] * 2, kernels=kern)
    assert [g.launches for g in split.plan(f).groups()] == [("stats", "apply")] * 2
    split = T.Compose([T.Lambda(lambda v: T.adjust_saturation(v, ones))] * 5, kernels=kern)
    assert [len(g.ops) for g in split.plan(f).groups()] == [4, 1]
    assert len(T.Compose([T.Pad((1, 1, 1, 1), 0.5), T.Pad((1, 0, 0, 0), 0.25)], kernels=kern).plan(f).groups()) == 2
    assert len(T.Compose([T.Pad((1, 1, 1, 1), 0.5), T.Pad((1, 0, 0, 0), 0.5)], kernels=kern).plan(f).groups()) == 1
    # geometry folds on both sides of the resample
    fold = T.Compose([T.RandomHorizontalFlip(p=1.0), T.CenterCrop((9, 9)), T.Resize((6, 6)), T.Pad((1, 1, 1, 1)), T.RandomHorizontalFlip(p=1.0)],
                     kernels=kern)
    g, = fold.plan(f).groups()
    assert g.a.mx == -1 and g.b.mx == -1 and g.out_hw == (8, 8) and not g.b.full


def test_resize_int_follows_the_scale_factor():
    f = torch.from_numpy(G["in_f13"])
    g, = T.Compose([T.Resize(7)], kernels=NumpyClipKernels()).plan(f).groups()
    Ha, Wa, sc_y, sc_x = g.resample
    assert g.out_hw == (7, 10) and sc_y == sc_x == float(np.float32(13 / 7)) and sc_x != float(np.float32(19) / np.float32(10))


def test_errors():
    kern = NumpyClipKernels()
    f = torch.from_numpy(G["in_f13"])
    u = torch.from_numpy(G["in_u13"])
    f5 = torch.from_numpy(G["in_f5d"])
    st = random.getstate()
    with pytest.raises(ValueError, match=r"Compose\.batch"):
        T.Compose([T.ColorJitter(0.4, 0.4, 0.4)], kernels=kern)(f5)
    with pytest.raises(ValueError, match=r"Compose\.batch"):
        T.adjust_contrast(f5, torch.ones(4), kernels=kern)
    with pytest.raises(ValueError, match=r"Compose\.batch"):
        T.Compose([T.Resize((4, 4))], kernels=kern)(f5)
    assert random.getstate() == st                                   # refused before any draw
    for fn in (T.adjust_brightness, T.adjust_contrast, T.adjust_saturation):
        with pytest.raises(TypeError):
            fn(u, torch.ones(3), kernels=kern)
    with pytest.raises(TypeError):
        T.Compose([T.RandomGray(1.0)], kernels=kern)(u)
    with pytest.raises(ValueError, match="requires grad"):
        T.hflip(f.clone().requires_grad_(True), kernels=kern)
    with pytest.raises(ValueError, match="requires grad"):
        T.Compose([T.Normalize(cases.MEAN, cases.STD, channel=1)], kernels=kern)(f5.clone().requires_grad_(True))
    with pytest.raises(TypeError):
        T.hflip(f.double(), kernels=kern)
    with pytest.raises(ValueError):
        T.adjust_brightness(f, torch.ones(4), kernels=kern)          # four factors, three frames
    with pytest.raises(ValueError):
        T.normalize(f, cases.MEAN, cases.STD, channel=1, kernels=kern)


def test_batch_equals_stacked_calls_with_the_same_draws():
    clips = torch.from_numpy(G["in_u13_batch"])
    for contrast in (True, False):
        chain = bench_chain(NumpyClipKernels(), contrast)
        seed(9)
        one_by_one = torch.stack([chain(c) for c in clips])
        after = (random.random(), np.random.uniform())
        kern = NumpyClipKernels()
        chain = bench_chain(kern, contrast)
        seed(9)
        out = chain.batch(clips)
        assert (random.random(), np.random.uniform()) == after
        assert torch.equal(out, one_by_one) and out.is_contiguous() and out.shape == (3, 3, 3, 8, 10)
        assert kern.launches == [("stats", "apply") if contrast else ("apply",)]          # the whole batch: one group
        seed(9)
        assert torch.equal(chain.batch(list(clips)), out)                                 # a list of clips is the same
    # the three clips drew different parameters
    seed(9)
    progs = [bench_chain(NumpyClipKernels()).plan(c) for c in clips]
    assert len({(p.groups()[0].a.record(), p.groups()[0].b.mx) for p in progs}) == 3
    # clips whose chains come out in different shapes cannot be stacked
    with pytest.raises(ValueError, match="different shapes"):
        seed(9)
        T.Compose([T.ToFloatTensor(), T.RandomSizedCrop(8)], kernels=NumpyClipKernels()).batch(clips)


def test_untouched_input_is_returned_itself():
    f = torch.from_numpy(G["in_f13"])
    kern = NumpyClipKernels()
    assert T.Compose([T.RandomGray(0.0), T.RandomHorizontalFlip(p=0.0), T.ColorJitter(0.4, p=0.0)], kernels=kern)(f) is f
    assert T.random_grayscale(f, 0.0, kernels=kern) is f
    assert kern.launches == []


def test_without_a_provider_and_without_a_device_it_raises():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    f = torch.from_numpy(G["in_f13"])
    with pytest.raises(_lib.SlicError):
        T.hflip(f)
    with pytest.raises(_lib.SlicError):
        T.Compose([T.ToFloatTensorInZeroOne(), T.Normalize(cases.MEAN, cases.STD)])(torch.from_numpy(G["in_u13"]))
    with pytest.raises(_lib.SlicError):
        T.RandomSizedCrop((8, 8))(f)

"""CPU: the algorithm of csrc/stem_dgrad.hip (tests/stem_dgrad_cpu_kernels.py: coarse rows, parity columns, zero-padded weight
operand) against float64 torch.autograd.grad(F.conv3d) on the shapes of the GPU test; the tap-slot counts of the formulation;
the host surface of ConvPlan (input_grad exists, pack_dgrad on a W-run plan is still refused) without a device.

Gate 1e-12 absolute: both sides are float64 sums of at most 7 * 49 * 64 = 21952 products; the weights are drawn at the scale of
the layer's initialisation (1 / sqrt(reduction length)), so a gradient element is O(1) and the two summation orders differ by a
few hundred ulps of 2.2e-16 at the most."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stem_dgrad_cpu_kernels as sk

# (C, N, kernel, stride, B, (T, H, W)): the fast-path shapes of tests/test_input_grad_gpu.py
SHAPES = [
    (3, 8, (7, 7, 7), (1, 2, 2), 2, (8, 20, 20)),
    (2, 8, (3, 7, 7), (1, 2, 2), 2, (4, 13, 15)),
    (3, 64, (7, 7, 7), (1, 2, 2), 3, (3, 9, 11)),
    (3, 16, (7, 7, 7), (2, 2, 2), 1, (9, 12, 11)),
    (3, 64, (7, 7, 7), (1, 2, 2), 1, (4, 36, 44)),
]


def make_case(C, N, kernel, stride, B, dims, seed=0, dtype=torch.float64):
    """(w [N, C, kt, kh, kw], dz [B, N, To, Ho, Wo] NCDHW, gx = d<conv3d(x, w), dz>/dx in float64), seeded"""
    g = torch.Generator().manual_seed(1000 + seed)
    pad = tuple(k // 2 for k in kernel)
    red = N * int(np.prod(kernel)) / float(np.prod(stride))
    w = (torch.randn((N, C) + tuple(kernel), generator=g, dtype=torch.float64) / np.sqrt(red)).to(dtype)
    x = torch.zeros((B, C) + tuple(dims), dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x, w.double(), None, stride, pad)
    dz = torch.randn(y.shape, generator=g, dtype=torch.float64).to(dtype)
    gx, = torch.autograd.grad(y, x, dz.double())
    return w, dz, gx


@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_algorithm_vs_fp64_autograd(case):
    C, N, kernel, stride, B, dims = SHAPES[case]
    w, dz, gx = make_case(*SHAPES[case], seed=case)
    got = sk.stem_dgrad(dz.permute(0, 2, 3, 4, 1).numpy(), w.numpy(), dims, stride[0])
    assert got.shape == tuple(gx.shape)
    err = float(np.abs(got - gx.numpy()).max())
    print("case", case, "max |err|", err, "|g|max", float(gx.abs().max()))
    assert err <= 1e-12


def test_offset_table_and_taps():
    assert sk.offset_table(7, 2, 3) == [-1, 0, 1, 2]
    assert [sk.tap_of(0, o, 7, 2, 3) for o in (-1, 0, 1, 2)] == [5, 3, 1, None]
    assert [sk.tap_of(1, o, 7, 2, 3) for o in (-1, 0, 1, 2)] == [6, 4, 2, 0]
    assert sk.offset_table(7, 1, 3) == [-3, -2, -1, 0, 1, 2, 3]


def test_slot_counts():
    assert sk.slot_counts((7, 7, 7), (1, 2, 2), (3, 3, 3)) == (343, 448)
    assert sk.slot_counts((3, 7, 7), (1, 2, 2), (1, 3, 3)) == (147, 192)
    assert sk.slot_counts((7, 7, 7), (2, 2, 2), (3, 3, 3)) == (343, 512)
    # what the device kernel executes: t is a fine row index, so t-stride 2 pads nothing along t (two frames: 3 + 4 taps)
    assert sk.executed_slots(7, 1) == (343, 448)
    assert sk.executed_slots(3, 1) == (147, 192)
    assert sk.executed_slots(7, 2) == (343, 448)


def test_packed_operand_real_slots():
    w = torch.ones(8, 3, 7, 7, 7, dtype=torch.float64).numpy()
    wop = sk.pack_weight(w)
    assert wop.shape == (7, 16, 8, 16)
    assert int((wop[:, :, 0, :4] != 0).sum()) == 343            # one channel's 2 x 2 parity columns over 7 x 16 offsets
    assert not wop[..., 12:].any()                               # columns past 4 C
    flat = sk.device_pack_order(wop)
    assert flat.shape == (7 * 16 * 8 * 16,) and flat.sum() == wop.sum()


def test_conv_plan_host_surface():
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.models.conv_plan import ConvPlan
    from video_similarity_search_amd.models import resnet
    assert callable(getattr(ConvPlan, "input_grad", None))
    assert "stem_dgrad" in resnet.COUNTS and "wgrad" in resnet.COUNTS
    plan = ConvPlan.__new__(ConvPlan)                            # plan construction needs a device: read the rule off the class
    plan.wrun = True
    with pytest.raises(_lib.SlicError):
        plan.pack_dgrad(None)
    for name in ("slic_conv_stem_dgrad", "slic_pack_weight_stem_dgrad"):
        assert name in _lib.SIGNATURES


def test_entry_refuses_other_shapes_without_a_launch():
    """argument checks come before any device work: a shape outside the kernel's range returns non-zero with the message set"""
    import ctypes
    from video_similarity_search_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    for C, N, kt, st in ((5, 8, 7, 1), (3, 12, 7, 1), (3, 8, 4, 1), (3, 8, 9, 1), (3, 8, 7, 3)):
        assert lib.slic_conv_stem_dgrad(one, one, 1, C, 4, 8, 8, N, kt, st, one, None) != 0
        assert b"slic_conv_stem_dgrad" in lib.slic_last_error()
    assert lib.slic_pack_weight_stem_dgrad(one, 12, 3, 7, one, None) != 0
    assert b"slic_pack_weight_stem_dgrad" in lib.slic_last_error()

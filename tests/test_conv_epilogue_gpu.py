"""The fused epilogue of the gather-GEMM (csrc/conv_epilogue.h: conv_epilogue / conv_epilogue_rows) on each of its five direct launch
forms — conv_gemm_kernel (variant 0), conv_gemm_dma_kernel 64 x 64 and 128 x 64 (variants 20 / 22), conv_gemm_dma_multi_kernel (the parity
classes of a stride-2 data gradient) and conv_splitk_finish (slic_conv_gemm_tailsplit) — against the float64 reference of
tests/conv_epilogue_ref.py, which test_conv_epilogue_cpu.py proves against torch.

The cases hold data on which float32 is exact whatever the order of the additions (proved per case in the CPU file), so stored outputs,
statistic sums and backward sums are compared BIT FOR BIT, per block of the slabs; sum (v - mean_blk)^2 alone is held to the derived
bound conv_epilogue_ref.m2_bound.  dst, the addend and both slabs lie inside allocations filled with one NaN bit pattern: the rows in
front of and behind them, the columns N .. ldo - 1 of every row and the slab rows behind ceil(M / tile_m) must keep it.

The arguments are SlicConvArgs of a LinearPlan (accumulators = x W^T) with the epilogue fields set by hand and handed to
slic_conv_gemm / slic_conv_gemm_tailsplit / slic_conv_gemm_multi; the stride-2 data gradient goes through ConvPlan.dgrad."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import conv_epilogue_ref as R
from ws_guard import GuardedWorkspace

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_goldens_linear_sites", os.path.join(HERE, "golden", "make_goldens_linear_sites.py"))
_gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gen)
counting = _gen.counting

POISON = 0x7FC5A3E1            # a quiet NaN no computation produces
GUARD_ROWS = 3


class Rows:
    """a [rows, ld] float32 window with GUARD_ROWS rows in front of and behind it, the whole allocation filled with POISON"""

    def __init__(self, rows, ld):
        self.rows, self.ld = rows, ld
        self.whole = torch.empty((rows + 2 * GUARD_ROWS) * ld, dtype=torch.int32, device="cuda")
        self.whole.fill_(POISON)

    @property
    def window(self):
        return self.whole[GUARD_ROWS * self.ld:(GUARD_ROWS + self.rows) * self.ld].view(self.rows, self.ld)

    @property
    def address(self):
        return self.whole.data_ptr() + GUARD_ROWS * self.ld * 4

    def tensor(self, shape):
        """the window as a float32 tensor of `shape` (ld == the row length)"""
        return self.window.view(torch.float32).view(shape)

    def put(self, a, ncols=None):
        """poison everything, then columns 0 .. ncols - 1 of the window = the bits of a (float32 [rows, ncols])"""
        self.whole.fill_(POISON)
        if a is not None:
            a = np.ascontiguousarray(a, np.float32)
            self.window[:, :a.shape[1]] = torch.from_numpy(a.view(np.int32)).cuda()
        return self

    def read(self, what):
        """-> the window's bits [rows, ld]; asserts the guard rows"""
        bits = self.whole.cpu().numpy().view(np.uint32).reshape(-1, self.ld)
        assert (bits[:GUARD_ROWS] == POISON).all(), f"{what}: rows in front of it were written"
        assert (bits[GUARD_ROWS + self.rows:] == POISON).all(), f"{what}: rows behind it were written"
        return bits[GUARD_ROWS:GUARD_ROWS + self.rows]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).astype(np.float32).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _copy(a):
    from video_similarity_search_amd._lib import SlicConvArgs
    return SlicConvArgs.from_buffer_copy(a)


class Forward:
    """one forward-type case on the device: the plan's SlicConvArgs, its operands, poisoned destinations"""

    def __init__(self, lib, C, M, N, ldo, tile_m, variant):
        from video_similarity_search_amd.models.conv_plan import LinearPlan
        self.lib, self.M, self.N, self.ldo, self.tile_m, self.variant = lib, M, N, ldo, tile_m, variant
        self.case = c = R.make_case(C, M, N)
        self.plan = LinearPlan(C, N, "cuda")
        self.x, self.w = _dev(c["x"]), _dev(c["W"])
        self.wp = self.plan.pack_fwd(self.w)
        a = self.plan._fwd_args(self.x.view(M, 1, 1, 1, C), M)
        a.wgt, a.wgt_bytes = self.wp.data_ptr(), self.wp.numel() * 4
        a.ldo = ldo
        self.base = a
        assert lib.slic_conv_tile_m(ctypes.byref(a), variant) == tile_m
        self.R = -(-M // tile_m)
        self.vec = {k: _dev(c[k]) for k in ("bias", "scale", "shift", "mean", "invstd")}
        self.dst = Rows(M, ldo)
        self.addend = Rows(M, ldo).put(c["addend"])
        self.mask = {k: Rows(M, ldo).put(c[k]) for k in ("mask", "mask_bwd")}
        self.z = Rows(M, ldo).put(c["z"])
        self.stat, self.bwd = Rows(self.R, 2 * N), Rows(self.R, 2 * N)

    def args(self, ops):
        a = _copy(self.base)
        self.dst.put(self.case["addend"] if "alias" in ops else None)
        self.stat.put(None)
        self.bwd.put(None)
        a.dst = self.dst.address
        for k in ("bias", "scale", "shift"):
            if k in ops:
                setattr(a, k, self.vec[k].data_ptr())
        if "addend" in ops:
            a.addend = self.dst.address if "alias" in ops else self.addend.address
        a.relu = int("relu" in ops)
        if "mask" in ops:
            a.mask_src = self.mask["mask_bwd" if "bwd" in ops else "mask"].address
        if "stat" in ops:
            a.stat_partial = self.stat.address
        if "bwd" in ops:
            a.bwd_z, a.bwd_mean, a.bwd_invstd = self.z.address, self.vec["mean"].data_ptr(), self.vec["invstd"].data_ptr()
            a.bwd_partial = self.bwd.address
        return a

    def check(self, name, ops):
        """dst, both slabs and their surroundings after a launch of operand set (name, ops)"""
        M, N, tile_m = self.M, self.N, self.tile_m
        out, stat, bsum = R.case_ref(self.case, ops, tile_m)
        got = self.dst.read(f"{name}: dst")
        assert (got[:, N:] == POISON).all(), f"{name}: columns N .. ldo - 1 of dst were written"
        bad = got[:, :N] != _bits(out)
        assert not bad.any(), f"{name}: {bad.sum()} outputs differ, the first at (row, column) {np.argwhere(bad)[0]}"
        s = self.stat.read(f"{name}: stat_partial").reshape(self.R, 2, N)
        b = self.bwd.read(f"{name}: bwd_partial").reshape(self.R, 2, N)
        if "stat" in ops:
            bad = s[:, 0] != _bits(stat[:, 0])
            assert not bad.any(), f"{name}: sum v differs in (block, column) {np.argwhere(bad)[0]}"
            _, cnt = R.block_starts(M, tile_m)
            m2 = s[:, 1].view(np.float32).astype(np.float64)
            err, bound = np.abs(m2 - stat[:, 1]), R.m2_bound(cnt[:, None], stat[:, 1])
            assert (err <= bound).all(), (f"{name}: sum (v - mean)^2 off by {err.max():.3e} in (block, column) "
                                          f"{np.argwhere(~(err <= bound))[0]}, allowed {bound[~(err <= bound)][0]:.3e}")
        else:
            assert (s == POISON).all(), f"{name}: stat_partial is not an operand, yet was written"
        if "bwd" in ops:
            bad = b != _bits(bsum)
            assert not bad.any(), f"{name}: backward sums differ in (block, which, column) {np.argwhere(bad)[0]}"
        else:
            assert (b == POISON).all(), f"{name}: bwd_partial is not an operand, yet was written"
        return s

    def check_inputs(self):
        c = self.case
        for what, rows, a in (("addend", self.addend, c["addend"]), ("mask", self.mask["mask"], c["mask"]),
                              ("mask", self.mask["mask_bwd"], c["mask_bwd"]), ("z", self.z, c["z"])):
            got = rows.read(what)
            assert np.array_equal(got[:, :self.N], np.ascontiguousarray(a, np.float32).view(np.uint32)), f"{what} was changed"
            assert (got[:, self.N:] == POISON).all()


def _run_sets(f, launch):
    stats = {}
    for name, ops in R.OPERAND_SETS:
        launch(f.args(ops))
        torch.cuda.synchronize()
        stats[name] = f.check(name, ops)
    # the statistics are those of acc + bias: scale, shift, addend and ReLU must not move a bit of them
    assert np.array_equal(stats["stat+all5"], stats["stat+bias"])
    f.check_inputs()


@pytest.mark.parametrize("M,N,ldo", R.SHAPES)
@pytest.mark.parametrize("variant", sorted(R.KERNEL_C))
def test_epilogue_direct_kernels(gpu, variant, M, N, ldo):
    """slic_conv_gemm on variants 0, 20 and 22: every operand set at one (M, N, ldo)"""
    from video_similarity_search_amd import _lib
    f = Forward(gpu, R.KERNEL_C[variant], M, N, ldo, R.TILE_M[variant], variant)
    assert (f.base.tap_tab is None) == (variant == 0)
    _run_sets(f, lambda a: _lib.call("slic_conv_gemm", ctypes.byref(a), variant, _lib.stream()))


@pytest.mark.parametrize("M,N,ldo", R.TAIL_SHAPES)
@pytest.mark.parametrize("split", R.TAIL_PLANS)
@pytest.mark.parametrize("variant", [20, 22])
def test_epilogue_tailsplit_finish(gpu, variant, split, M, N, ldo):
    """slic_conv_gemm_tailsplit: the whole row blocks leave through the DMA kernel's epilogue, the cut ones through conv_splitk_finish;
    the workspace has the size its own query names, between guard bands"""
    from video_similarity_search_amd import _lib
    tile_m = R.TILE_M[variant]
    f = Forward(gpu, R.TAIL_C, M, N, ldo, tile_m, variant)
    assert f.base.nchunks == 32, "four k-tiles"
    nfull_rb, splits = {"(0, 2)": (0, 2), "(1, 3)": (1, 3), "last": (f.R - 1, 2)}[split]
    assert nfull_rb < f.R
    guard = GuardedWorkspace(0xFF)

    def launch(a):
        nbytes = gpu.slic_conv_gemm_tailsplit_workspace_bytes(ctypes.byref(a), variant, nfull_rb, splits)
        assert nbytes >= splits * (f.R - nfull_rb) * tile_m * N * 4
        ws = guard(nbytes, "cuda", "tail")
        _lib.call("slic_conv_gemm_tailsplit", ctypes.byref(a), variant, nfull_rb, splits, ctypes.c_void_p(ws.data_ptr()), _lib.stream())

    _run_sets(f, launch)
    guard.check()


# ---- the stride-2 data gradient: slic_conv_gemm_multi (32 channels) and kernel 0 with a strided dst (16 channels) ------------------------
class Dgrad:
    def __init__(self, kind, nout):
        from video_similarity_search_amd.models.conv_plan import ConvPlan
        self.case = c = R.dgrad_case(kind, nout)
        self.plan = ConvPlan(c["cin"], nout, c["kernel"], (2, 2, 2), c["pad"], c["dims"], "cuda")
        assert self.plan.out_dims == c["odims"]
        # the launch order and geometry the reference rebuilt are the plan's
        order = sorted(self.plan.dgrad_classes, key=lambda d: -d["nchunks"])
        assert [(d["cls"], d["grid"], d["nchunks"]) for d in order] == [(d["cls"], d["grid"], d["nchunks"]) for d in c["classes"]]
        self.order = order
        self.w, self.dz = _dev(c["W"]), _dev(c["dz"])
        self.wd = self.plan.pack_dgrad(self.w)
        self.P = c["full"].shape[0]
        self.shape = (c["B"],) + c["dims"] + (c["cin"],)
        self.dx = Rows(self.P, c["cin"])
        self.addend, self.mask, self.z = (Rows(self.P, c["cin"]).put(c[k]) for k in ("addend", "mask", "z"))
        self.mean, self.invstd = _dev(c["mean"]), _dev(c["invstd"])

    def run(self, fused, skip_empty=False):
        """-> (call counts, bwd slab bits or None); dx is poisoned first and handed over as `out`"""
        self.dx.put(None)
        kw = {}
        if fused:
            kw = dict(addend=self.addend.tensor(self.shape), mask=self.mask.tensor(self.shape),
                      bwd=(self.z.tensor(self.shape), self.mean, self.invstd))
        torch.cuda.synchronize()
        with counting() as calls:
            r = self.plan.dgrad(self.dz, self.wd, self.case["B"], out=self.dx.tensor(self.shape), skip_empty=skip_empty, **kw)
            torch.cuda.synchronize()
        return calls, (r[1].cpu().numpy().view(np.uint32) if fused else None)

    def check(self, what, fused, slab, written=None):
        c = self.case
        dx, ref_slab = R.dgrad_ref(c, fused)
        want = _bits(dx)
        if written is not None:
            want[~written] = POISON
        got = self.dx.read(f"{what}: dx")
        bad = got != want
        assert not bad.any(), f"{what}: {bad.sum()} elements of dx differ, the first at (position, channel) {np.argwhere(bad)[0]}"
        if fused:
            assert slab.shape == ref_slab.shape, "one slab row per 64-row block of every class, in launch order"
            bad = slab != _bits(ref_slab)
            assert not bad.any(), f"{what}: backward sums differ in (slab row, which, channel) {np.argwhere(bad)[0]}"
        for name, rows in (("addend", self.addend), ("mask", self.mask), ("z", self.z)):
            assert np.array_equal(rows.read(name), np.ascontiguousarray(c[name], np.float32).view(np.uint32)), f"{name} was changed"


def _launches(calls):
    return {k: v for k, v in calls.items() if k in ("slic_conv_gemm", "slic_conv_gemm_multi", "slic_conv_gemm_tailsplit")}


@pytest.mark.parametrize("nout", [32, 16])
@pytest.mark.parametrize("kind", sorted(R.DGRAD_KINDS))
def test_epilogue_stride2_data_gradient(gpu, kind, nout):
    """3 x 3 x 3 / stride 2 / pad 1 at (3, 5, 7) (eight classes of unequal grids, each one ragged block) and 1 x 1 x 1 / stride 2 (seven
    classes without a tap: their rows are the epilogue of a zero accumulator), through ConvPlan.dgrad with addend + mask + backward sums
    and plain; then with skip_empty=True onto a poisoned dx.

    Which launches carry the classes: with 32 channels every class that has a tap table takes the LDS-DMA kernel, and the 3 x 3 x 3
    plan's eight go out as ONE slic_conv_gemm_multi launch.  A class without a tap has no tap table (ConvPlan builds none), so the plan
    sends the 1 x 1 x 1 layer's classes out one by one — test_epilogue_multi_classes_without_a_tap hands those to the multi kernel itself.
    With 16 channels every class is a launch of kernel 0 with a strided dst."""
    d = Dgrad(kind, nout)
    want = {"slic_conv_gemm_multi": 1} if (nout, kind) == (32, "3x3x3") else {"slic_conv_gemm": 8}
    for fused in (True, False):
        calls, slab = d.run(fused)
        assert _launches(calls) == want, (fused, calls)
        d.check(f"fused={fused}", fused, slab)
    calls, _ = d.run(False, skip_empty=True)
    written = np.zeros(d.P, bool)
    for dc in d.case["classes"]:
        if dc["nchunks"]:
            written[R.class_rows(d.case, dc)] = True
    assert written.all() == (kind == "3x3x3") and (kind == "3x3x3" or written.sum() * 8 < d.P * 2)
    assert sum(_launches(calls).values()) == (1 if want == {"slic_conv_gemm_multi": 1} else sum(dc["nchunks"] > 0 for dc in d.case["classes"]))
    d.check("skip_empty", False, None, written)


def _class_args(d, dc, variant_tap=None):
    """the SlicConvArgs ConvPlan.dgrad builds for one parity class, with addend + mask + backward operands; variant_tap: the tap table
    a class without taps is given so that the LDS-DMA kernels take it (nchunks = 0: no record of it is used)"""
    from video_similarity_search_amd._lib import SlicConvArgs
    p, c = d.plan, d.case
    a = SlicConvArgs()
    a.src, a.src_bytes = d.dz.data_ptr(), d.dz.numel() * 4
    a.wgt, a.wgt_bytes = d.wd.data_ptr(), d.wd.numel() * 4
    a.dst = d.dx.address
    a.tab = dc["tab"].data_ptr()
    a.tap_tab = dc["tap"].data_ptr() if dc["tap"] is not None else variant_tap
    a.addend, a.mask_src, a.bwd_z = d.addend.address, d.mask.address, d.z.address
    a.bwd_mean, a.bwd_invstd = d.mean.data_ptr(), d.invstd.data_ptr()
    ga, gb, gc = dc["grid"]
    a.M, a.N, a.nchunks = c["B"] * ga * gb * gc, p.Cs, dc["nchunks"]
    a.Cs, (a.Ts, a.Hs, a.Ws) = p.N, p.out_dims
    a.Ga, a.Gb, a.Gc = ga, gb, gc
    a.sa = a.sb = a.sc = 1
    a.ldw, a.ldo = p.Kd, p.Cs
    a.dst_strided = 1
    a.Da, a.Db, a.Dc = p.in_dims
    a.da, a.db, a.dc = p.stride
    a.ea, a.eb, a.ec = dc["cls"]
    return a


@pytest.mark.parametrize("variant", [20, 22])
def test_epilogue_multi_classes_without_a_tap(gpu, variant):
    """slic_conv_gemm_multi on the eight classes of the 1 x 1 x 1 / stride 2 data gradient, seven of them with nchunks = 0: their
    workgroups run no k-tile and store epilogue(0).  The C ABI takes nchunks = 0 with any valid tap table; the classes borrow the table
    of the one class that has a tap.  Backward slab: poisoned, one row per class (each class is one ragged block)"""
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd._lib import SlicConvArgs
    d = Dgrad("1x1x1", 32)
    tap = next(dc["tap"] for dc in d.order if dc["tap"] is not None).data_ptr()
    tile_m = R.TILE_M[variant]
    blocks = [-(-d.case["B"] * int(np.prod(dc["grid"])) // tile_m) for dc in d.order]
    assert blocks == [1] * 8
    slab = Rows(sum(blocks), 2 * d.case["cin"])
    launches, r0 = [], 0
    for dc, r in zip(d.order, blocks):
        a = _class_args(d, dc, tap)
        a.bwd_partial = slab.address + r0 * 2 * d.case["cin"] * 4
        r0 += r
        launches.append(a)
    assert sorted(a.nchunks for a in launches) == [0] * 7 + [8]
    d.dx.put(None)
    _lib.call("slic_conv_gemm_multi", (SlicConvArgs * 8)(*launches), 8, variant, _lib.stream())
    torch.cuda.synchronize()
    d.check(f"multi, variant {variant}", True, slab.read("bwd_partial").reshape(-1, 2, d.case["cin"]))


def test_stat_and_bwd_partial_together_are_refused(gpu):
    """stat_partial excludes bwd_partial: slic_conv_gemm, slic_conv_gemm_multi and slic_conv_gemm_tailsplit refuse the pair on the host,
    before any launch — dst keeps its poison — and a valid call right after gives the right result"""
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd._lib import SlicConvArgs
    f = Forward(gpu, R.TAIL_C, 129, 36, 36, 64, 20)
    both = f.args(("stat", "bwd"))
    st = _lib.stream()
    ws = torch.empty(gpu.slic_conv_gemm_tailsplit_workspace_bytes(ctypes.byref(both), 20, 0, 2), dtype=torch.uint8, device="cuda")
    calls = [
        ("slic_conv_gemm", lambda: gpu.slic_conv_gemm(ctypes.byref(both), 20, st)),
        ("slic_conv_gemm", lambda: gpu.slic_conv_gemm(ctypes.byref(both), 0, st)),
        ("slic_conv_gemm_multi", lambda: gpu.slic_conv_gemm_multi((SlicConvArgs * 2)(f.args(("bwd",)), both), 2, 20, st)),
        ("slic_conv_gemm_tailsplit", lambda: gpu.slic_conv_gemm_tailsplit(ctypes.byref(both), 20, 0, 2, ctypes.c_void_p(ws.data_ptr()), st)),
    ]
    for name, go in calls:
        rc = go()
        msg = gpu.slic_last_error().decode()
        assert rc != 0, f"{name} accepted stat_partial with bwd_partial"
        assert name + ":" in msg and "excludes stat_partial" in msg, (name, msg)
    torch.cuda.synchronize()
    for rows, what in ((f.dst, "dst"), (f.stat, "stat_partial"), (f.bwd, "bwd_partial")):
        assert (rows.read(what) == POISON).all(), f"a refused call wrote to {what}"
    for name, ops in (("stat+all5", ("stat",) + R.ALL5), ("bwd+mask+addend", ("bwd", "mask", "addend"))):
        _lib.call("slic_conv_gemm", ctypes.byref(f.args(ops)), 20, st)
        torch.cuda.synchronize()
        f.check(name, ops)

"""The optimizer step on the device: torch.optim.SGD and torch.optim.Adam as one multi-tensor launch (csrc/optim.hip), the MoCo
key-encoder momentum update (models/infoNCE.py:87-90 of the reference) as one more, and what needs a norm: a LARS step,
torch.nn.utils.clip_grad_norm_ and the logged gradient norm, three launches each at the most.

`SGD` and `Adam` subclass torch.optim.Optimizer and override step() only, so param_groups, add_param_group, zero_grad, hooks,
lr schedulers and state_dict / load_state_dict are torch's, and the state keys and types are those of the installed torch
(`momentum_buffer`; `step` as a CPU scalar tensor, `exp_avg`, `exp_avg_sq`): a state dict written by either implementation loads into
the other and continues the same trajectory.  Adam is torch's Adam with L2 weight decay, not AdamW; amsgrad and maximize raise
NotImplementedError.

One step is at most one launch and at most one host-to-device copy of 128 bytes per tensor:
  chunk map     (tensor, chunk) per work item, a pure function of the tensor lengths: uploaded once per parameter set
  descriptors   pointers, length, flags and hyper-parameters (as doubles) per tensor: uploaded when a byte of it changed.  SGD with
                stable pointers (DDP bucket views, zero_grad(set_to_none=False)) and unchanged hyper-parameters uploads nothing;
                Adam's bias corrections change every step, so Adam uploads every step.
Staging: the descriptors of a step are written into a pinned slot of a ring and copied asynchronously.  A slot is written again only
after the event recorded behind its last launch has completed (an event QUERY; the host never waits): while the device is behind,
the ring grows instead, up to MAX_SLOTS, where the host waits for the oldest slot (the launch queue fills long before that).

Gradients: a parameter whose .grad is None is skipped (its state and its Adam `step` do not move).  A non-contiguous gradient is
copied contiguous for that step (rare; one extra torch copy, correctness kept).  Sparse gradients, parameters that are not
contiguous fp32 on one device raise before anything is launched.

Norms (`LARS`, `clip_grad_norm_`, `grad_norm`): two more launches over the same two tables leave per-tensor norms, LARS's trust ratios,
the total norm and the clip coefficient on the device, where the update or the scale launch reads them; no host read-back.  The
reduction is in double, in a fixed order, without atomics: the same inputs give the same bits.

`kernels=` takes another provider with HipOptimKernels' methods; the tests run the host logic on the CPU that way.  The product
path has no CPU fallback: HipOptimKernels raises SlicError without a gfx950 device.
"""
import contextlib
import math

import numpy as np
import torch

from . import _lib

# struct MtDesc of csrc/optim.hip (SLIC_MT_DESC_BYTES); s1, s2: momentum_buffer, - | exp_avg, exp_avg_sq | -, -
DESC = np.dtype([("p", "<u8"), ("g", "<u8"), ("s1", "<u8"), ("s2", "<u8"), ("n", "<i8"), ("flags", "<i4"), ("pad", "<i4"),
                 ("h", "<f8", (10,))])
assert DESC.itemsize == 128
VEC, NESTEROV, FIRST, ADAPT = 1, 2, 4, 8                    # SLIC_MT_* of include/slic_hip.h
OPS = ("sgd", "adam", "ema", "lars", "grad")                # grad: the gradient-only table of clip_grad_norm_ / grad_norm
NORM_MODES = {"lars": 0, "l2": 1, "inf": 2}                 # SLIC_MT_NORM_*


def build_chunk_map(lengths, chunk):
    """int32 [n_items, 2]: (tensor, chunk within the tensor) for every chunk of every tensor, tensors in order.  Chunk c of a tensor of
    n elements is [c * chunk, min((c + 1) * chunk, n)): every element is in exactly one item and no item spans two tensors."""
    lens = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lens.size == 0 or (lens <= 0).any():
        raise ValueError("build_chunk_map: every tensor needs at least one element")
    nch = (lens + (chunk - 1)) // chunk
    total = int(nch.sum())
    if total >= 2 ** 31 or int(nch.max()) >= 2 ** 31:
        raise ValueError("build_chunk_map: more than 2^31 work items")
    first = np.cumsum(nch) - nch
    out = np.empty((total, 2), dtype=np.int32)
    out[:, 0] = np.repeat(np.arange(lens.size, dtype=np.int64), nch)
    out[:, 1] = np.arange(total, dtype=np.int64) - np.repeat(first, nch)
    return out


def build_descriptors(p, g, s1, s2, n, hyper, flags=0):
    """the descriptor table from addresses (0: no such tensor), element counts, hyper-parameter rows [T, <= 10] and flag words.
    SLIC_MT_VEC is set here, on the tensors whose every address is 16-byte aligned."""
    T = len(p)
    d = np.zeros(T, dtype=DESC)
    d["p"], d["g"], d["s1"], d["s2"], d["n"] = p, g, s1, s2, n
    hyper = np.asarray(hyper, dtype=np.float64).reshape(T, -1)
    d["h"][:, :hyper.shape[1]] = hyper
    misaligned = (d["p"] | d["g"] | d["s1"] | d["s2"]) & np.uint64(15)
    d["flags"] = (np.asarray(flags, dtype=np.int32) & ~VEC) | np.where(misaligned == 0, VEC, 0).astype(np.int32)
    return d


class HipOptimKernels:
    """the device side (csrc/optim.hip): tables in pinned and device memory, launches on _lib.stream()"""
    dtype = torch.float32

    class Slot:
        def __init__(self, nbytes, device):
            self.nbytes = nbytes
            self.host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            self.dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self.event = torch.cuda.Event()
            self.views = {}

    def check(self, tensors):
        _lib.require_device(*tensors)

    def on(self, device):
        """the context in which tables are made and launches issued for tensors on `device`"""
        if device.index is None or device.index == torch.cuda.current_device():
            return contextlib.nullcontext()
        return torch.cuda.device(device)

    def chunk(self):
        return int(_lib.load().slic_multi_tensor_chunk())

    def stream_key(self):
        return _lib.stream().value

    def put_map(self, cmap, device):
        """the chunk map on the device; the pinned source lives (unchanged) as long as the handle"""
        host = torch.empty(cmap.shape, dtype=torch.int32, pin_memory=True)
        host.numpy()[:] = cmap
        return host, host.to(device, non_blocking=True)

    def new_slot(self, nbytes, device):
        return self.Slot(nbytes, device)

    def slot_free(self, slot):
        return slot.event.query()

    def slot_wait(self, slot):
        slot.event.synchronize()

    def write(self, slot, desc):
        slot.host.numpy()[:desc.nbytes] = desc.view(np.uint8).reshape(-1)

    def _tables(self, cmap, n_items, slot, n_tensors, upload):
        nbytes = n_tensors * DESC.itemsize
        if upload:
            v = slot.views.get(nbytes)
            if v is None:
                v = slot.views[nbytes] = (slot.dev[:nbytes], slot.host[:nbytes])
            v[0].copy_(v[1], non_blocking=True)
        return (_lib.ptr(cmap[1]), n_items, _lib.ptr(slot.dev), _lib.c_void_p(slot.host.data_ptr()), n_tensors)

    def launch(self, op, cmap, n_items, slot, n_tensors, upload, all_first):
        args = self._tables(cmap, n_items, slot, n_tensors, upload)
        if op == "sgd":
            _lib.call("slic_multi_sgd", *args, int(all_first), _lib.stream())
        else:
            _lib.call("slic_multi_adam" if op == "adam" else "slic_multi_ema", *args, _lib.stream())
        slot.event.record()

    # --- norms: per-item partial sums (cached beside the chunk map), the folded norms (a fresh allocation per operation, so a
    # returned norm is never overwritten by the next call), and the launches that read them
    def new_partials(self, n_items, device):
        return torch.empty((n_items, 2), dtype=torch.float64, device=device)

    def new_norms(self, n_tensors, device):
        """[2 + 3 T]: total norm, clip coefficient, then the rows wnorm, unorm, q"""
        return torch.empty(2 + 3 * n_tensors, dtype=torch.float32, device=device)

    def launch_norm(self, mode, cmap, n_items, slot, n_tensors, upload, partials):
        args = self._tables(cmap, n_items, slot, n_tensors, upload)
        _lib.call("slic_multi_sqnorm", *args, NORM_MODES[mode], _lib.ptr(partials), _lib.stream())
        slot.event.record()

    def launch_fold(self, mode, slot, n_tensors, n_items, partials, max_norm, norms):
        _lib.call("slic_multi_norm_fold", _lib.ptr(slot.dev), _lib.c_void_p(slot.host.data_ptr()), n_tensors, n_items, _lib.ptr(partials),
                  NORM_MODES[mode], float(max_norm), _lib.c_void_p(norms.data_ptr() + 8), _lib.ptr(norms), _lib.stream())
        slot.event.record()

    def launch_lars(self, cmap, n_items, slot, n_tensors, upload, all_first, norms):
        args = self._tables(cmap, n_items, slot, n_tensors, upload)
        ratios = None if norms is None else _lib.c_void_p(norms.data_ptr() + 8 + 8 * n_tensors)
        _lib.call("slic_multi_lars", *args, int(all_first), ratios, _lib.stream())
        slot.event.record()

    def launch_scale(self, cmap, n_items, slot, n_tensors, upload, norms):
        args = self._tables(cmap, n_items, slot, n_tensors, upload)
        _lib.call("slic_multi_scale", *args, _lib.ptr(norms), _lib.stream())
        slot.event.record()


_default_kernels = None


def _kern(kernels):
    global _default_kernels
    if kernels is not None:
        return kernels
    if _default_kernels is None:
        _default_kernels = HipOptimKernels()
    return _default_kernels


class MultiTensorLaunch:
    """the host side of one multi-tensor operation: the cached chunk maps, the staging ring, the decision whether to upload"""
    MAX_SLOTS = 64
    MAX_MAPS = 4

    def __init__(self, op, kernels):
        assert op in OPS
        self.op, self.kern = op, kernels
        self.maps = {}                    # (device, stream, lengths) -> [handle, n_items, partial sums of the norm pass or None]
        self.slots = []
        self.cur = None                   # the slot that holds `cur_bytes` on the device
        self.cur_bytes, self.cur_key = None, None

    def _map(self, desc, device, skey):
        key = (str(device), skey, desc["n"].tobytes())
        hit = self.maps.get(key)
        if hit is None:
            cmap = build_chunk_map(desc["n"], self.kern.chunk())
            if len(self.maps) >= self.MAX_MAPS:
                self.maps.pop(next(iter(self.maps)))
            hit = self.maps[key] = [self.kern.put_map(cmap, device), cmap.shape[0], None]
        return hit

    def _acquire(self, nbytes, device):
        """a slot nothing on the device still reads: a free one, else a new one, else (ring full) the oldest once it is done"""
        for i, s in enumerate(self.slots):
            if s.nbytes >= nbytes and self.kern.slot_free(s):
                self.slots.append(self.slots.pop(i))            # most recently used last
                return s
        if len(self.slots) >= self.MAX_SLOTS:
            s = self.slots.pop(0)
            self.kern.slot_wait(s)
            if s.nbytes >= nbytes:
                self.slots.append(s)
                return s
        s = self.kern.new_slot(max(4096, 2 * nbytes), device)
        self.slots.append(s)
        return s

    def _stage(self, desc, device):
        """-> (the map's cache entry, whether the next launch must upload): the table is staged only if it differs from what the
        device holds, so the launches of one operation over one table share one upload"""
        skey = (str(device), self.kern.stream_key())
        entry = self._map(desc, device, skey[1])
        raw = desc.tobytes()
        upload = self.cur is None or raw != self.cur_bytes or skey != self.cur_key
        if upload:
            self.cur = self._acquire(desc.nbytes, device)
            self.kern.write(self.cur, desc)
            self.cur_bytes, self.cur_key = raw, skey
        return entry, upload

    def run(self, desc, device, all_first=False):
        """one launch over the tensors of `desc`; uploads the table only if it differs from what the device holds"""
        with self.kern.on(device):
            entry, upload = self._stage(desc, device)
            self.kern.launch(self.op, entry[0], entry[1], self.cur, desc.shape[0], upload, bool(all_first))

    def norms(self, desc, device, mode, max_norm=1.0):
        """two launches, the norm pass and the fold -> [2 + 3 T] on the device: total norm, clip coefficient for `max_norm` (both:
        gradient modes only), then per tensor wnorm, unorm, q"""
        T = desc.shape[0]
        with self.kern.on(device):
            entry, upload = self._stage(desc, device)
            if entry[2] is None:
                entry[2] = self.kern.new_partials(entry[1], device)
            out = self.kern.new_norms(T, device)
            self.kern.launch_norm(mode, entry[0], entry[1], self.cur, T, upload, entry[2])
            self.kern.launch_fold(mode, self.cur, T, entry[1], entry[2], max_norm, out)
        return out

    def lars(self, desc, device, all_first, norms):
        """the LARS update; norms: what norms(desc, device, "lars") returned, None when no tensor is adaptive"""
        with self.kern.on(device):
            entry, upload = self._stage(desc, device)
            self.kern.launch_lars(entry[0], entry[1], self.cur, desc.shape[0], upload, bool(all_first), norms)

    def scale(self, desc, device, norms):
        """gradients *= the clip coefficient norms(desc, device, "l2" | "inf", max_norm) left on the device"""
        with self.kern.on(device):
            entry, upload = self._stage(desc, device)
            self.kern.launch_scale(entry[0], entry[1], self.cur, desc.shape[0], upload, norms)


def _check_param(p, kern, device, what):
    if not isinstance(p, torch.Tensor):
        raise TypeError(f"{what}: expected a tensor, got {type(p).__name__}")
    if p.layout != torch.strided:
        raise ValueError(f"{what}: sparse parameters are not supported")
    if p.dtype != kern.dtype:
        raise TypeError(f"{what}: {p.dtype} parameter; the device step is {kern.dtype} only")
    if not p.is_contiguous():
        raise ValueError(f"{what}: non-contiguous parameter of shape {tuple(p.shape)}")
    if device is not None and p.device != device:
        raise ValueError(f"{what}: parameters on more than one device ({device} and {p.device})")


def _grad_of(p, kern, what, keep):
    g = p.grad
    if g.is_sparse or g.layout != torch.strided:
        raise RuntimeError(f"{what} does not support sparse gradients")
    if g.dtype != kern.dtype or g.device != p.device or g.shape != p.shape:
        raise ValueError(f"{what}: gradient {g.dtype} {tuple(g.shape)} on {g.device} for a {p.dtype} {tuple(p.shape)} parameter on {p.device}")
    if not g.is_contiguous():
        g = g.contiguous()                 # documented: copied for this step
        keep.append(g)
    return g


def _state_tensor(state, key, p, make):
    """state[key] as a contiguous tensor like p (a loaded state may be neither); None -> make(p)"""
    t = state.get(key)
    if t is None:
        t = state[key] = make(p, memory_format=torch.contiguous_format)
        return t, True
    if t.dtype != p.dtype or t.device != p.device or not t.is_contiguous():
        t = state[key] = t.to(device=p.device, dtype=p.dtype).contiguous()
    if t.shape != p.shape:
        raise ValueError(f"state '{key}' of shape {tuple(t.shape)} for a parameter of shape {tuple(p.shape)}")
    return t, False


def _scalar(v):
    return float(v.item()) if isinstance(v, torch.Tensor) else float(v)


def _unsupported(group, *names):
    for name in names:
        if group.get(name):
            raise NotImplementedError(f"{name}=True is not supported by the device optimizer step")


class _Rec:
    """what a step remembers of one parameter so that the next step re-validates only what changed: the parameter and the address
    it was checked at (dtype and device cannot change under an unchanged address), its state dict, the state tensors already
    checked (by identity), Adam's `step` and a NumPy view of it"""
    __slots__ = ("p", "ptr", "state", "s1", "s2", "step", "step_np")

    def __init__(self, p, state):
        self.p, self.ptr, self.state, self.s1, self.s2, self.step, self.step_np = p, p.data_ptr(), state, None, None, None, None


class _Optimizer(torch.optim.Optimizer):
    _op = None

    def __init__(self, params, defaults, kernels):
        self._kernels = kernels
        super().__init__(params, defaults)
        kern, dev = _kern(kernels), None
        for group in self.param_groups:
            self._check_group(group)
            for p in group["params"]:
                _check_param(p, kern, dev, type(self).__name__)
                dev = p.device

    def _launcher(self):
        mt = self.__dict__.get("_mt")
        if mt is None:
            mt = self.__dict__["_mt"] = MultiTensorLaunch(self._op, _kern(self.__dict__.get("_kernels")))
        return mt

    def _records(self):
        """id(parameter) -> _Rec; dropped when load_state_dict replaced self.state (the records point into the old one)"""
        d = self.__dict__
        if d.get("_recs_of") is not self.state:
            d["_recs"], d["_recs_of"] = {}, self.state
        return d["_recs"]

    def _admit(self, recs, p, g, kern, dev, keep):
        """the full checks of one (parameter, gradient) the quick test of _update did not wave through -> (record, gradient to
        use); raises with the reason"""
        name = type(self).__name__
        _check_param(p, kern, dev, name)
        g = _grad_of(p, kern, name, keep)
        rec = recs.get(id(p))
        if rec is None or rec.p is not p:
            rec = recs[id(p)] = _Rec(p, self.state[p])
        rec.ptr = p.data_ptr()
        return rec, g

    def _gather(self, kern):
        """the table of a step with an optional momentum buffer (SGD, LARS) -> (descriptors, device, all_first, live parameters,
        gradient copies to keep alive until the launches are issued), None when no parameter has a gradient.
        _group_row(group) -> (hyper-parameter row with the momentum at [1], flag word of the group's tensors)"""
        recs, strided = self._records(), torch.strided
        ent, rows, flags, first, keep, live = [], [], [], [], [], []     # ent: (p, g, buf address, elements) per tensor
        dev, p0 = None, None
        for group in self.param_groups:
            self._check_group(group)
            row, flag = self._group_row(group)
            mom = row[1]
            before = len(ent)
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                rec = recs.get(id(p))
                ptr = p.data_ptr()
                # the per-step test: what an assignment to .data / .grad since the last step could have changed
                if rec is None or rec.p is not p or rec.ptr != ptr or dev is None or not p.is_contiguous() \
                        or g.layout is not strided or not g.is_contiguous():
                    rec, g = self._admit(recs, p, g, kern, dev, keep)
                    dev = p.device
                n = p.numel()
                if n == 0:
                    continue
                bptr = 0
                if mom != 0:
                    buf = rec.state.get("momentum_buffer")
                    if buf is None or buf is not rec.s1:
                        buf, new = _state_tensor(rec.state, "momentum_buffer", p, torch.empty_like)
                        rec.s1 = buf
                        if new:
                            first.append(len(ent))
                    bptr = buf.data_ptr()
                p0 = p
                ent.append((ptr, g.data_ptr(), bptr, n))
                live.append(p)
            cnt = len(ent) - before
            rows.extend([row] * cnt)
            flags.extend([flag] * cnt)
        if not ent:
            return None
        kern.check([p0])                   # one device for all, gradients on their parameter's device: .grad's setter sees to that
        # every tensor with a buffer on its first step (step 1 of a run): said by the launch argument, so the table of step 1
        # serves step 2
        all_first = bool(first) and len(first) == sum(1 for e in ent if e[2])
        if first and not all_first:
            for i in first:
                flags[i] |= FIRST
        cols = np.array(ent, dtype=np.uint64)
        return build_descriptors(cols[:, 0], cols[:, 1], cols[:, 2], 0, cols[:, 3], rows, flags), dev, all_first, live, keep

    def step(self, closure=None):
        """one optimization step: at most one launch (LARS with an adaptive tensor: three).  closure: as torch's, re-evaluates the model and returns the loss"""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        with torch.no_grad():
            self._update(self._launcher())
        return loss


class SGD(_Optimizer):
    """torch.optim.SGD (momentum, dampening, weight_decay, nesterov) with the update of all groups as one launch"""
    _op = "sgd"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, kernels=None):
        if maximize:
            raise NotImplementedError("maximize=True is not supported by the device optimizer step")
        if _scalar(lr) < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=False,
                        foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults, kernels)

    @staticmethod
    def _check_group(group):
        _unsupported(group, "maximize", "differentiable")
        if group["nesterov"] and (group["momentum"] <= 0 or group["dampening"] != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")

    @staticmethod
    def _group_row(group):
        return (_scalar(group["lr"]), float(group["momentum"]), 1.0 - float(group["dampening"]), _scalar(group["weight_decay"])), \
            (NESTEROV if group["nesterov"] else 0)

    def _update(self, mt):
        got = self._gather(mt.kern)
        if got is not None:
            desc, dev, all_first, _, _ = got
            mt.run(desc, dev, all_first)


class LARS(_Optimizer):
    """Layer-wise adaptive rate scaling (You, Gitman, Ginsburg 2017) as SimCLR / BYOL use it: momentum SGD whose update is scaled,
    per tensor, by the trust ratio q = trust_coefficient * |w| / |g + weight_decay * w| (1 where either norm is 0):

        u = g + weight_decay * w;   v = q * u  (adapt)  or  u;   buf = momentum * buf + v  (buf = v on the first step);   w -= lr * buf

    `adapt` is a per-group option.  The usual recipe keeps BatchNorm weights and all biases out of the adaptation and the decay:

        LARS([dict(params=weights), dict(params=norms_and_biases, adapt=False, weight_decay=0)], lr=..., weight_decay=1e-6)

    A step is three launches (per-item sums of squares in double, the per-tensor fold that leaves q on the device, the update that
    reads it) and no host read-back; with no adaptive tensor it is one launch, bit-identical to SGD(momentum, weight_decay).  The
    three launches share one descriptor upload.  The state key is `momentum_buffer`, as SGD's.  nesterov, dampening and maximize are
    not offered."""
    _op = "lars"

    def __init__(self, params, lr, momentum=0.9, weight_decay=0, trust_coefficient=0.001, *, adapt=True, kernels=None):
        if _scalar(lr) < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, trust_coefficient=trust_coefficient, adapt=bool(adapt))
        self._check_group(defaults)
        super().__init__(params, defaults, kernels)

    @staticmethod
    def _check_group(group):
        _unsupported(group, "maximize", "nesterov", "dampening", "differentiable")
        tc = float(group["trust_coefficient"])
        if not (tc > 0.0 and math.isfinite(tc)):
            raise ValueError(f"Invalid trust_coefficient value: {group['trust_coefficient']}")

    @staticmethod
    def _group_row(group):
        return (_scalar(group["lr"]), float(group["momentum"]), float(group["trust_coefficient"]), _scalar(group["weight_decay"])), \
            (ADAPT if group["adapt"] else 0)

    def _update(self, mt):
        got = self._gather(mt.kern)
        if got is None:
            return
        desc, dev, all_first, live, _ = got
        norms = mt.norms(desc, dev, "lars") if (desc["flags"] & ADAPT).any() else None
        mt.lars(desc, dev, all_first, norms)
        self.__dict__["_last"] = (live, norms)

    def trust_ratios(self):
        """(the parameters the last step updated, trust_coefficient * |w| / |u| of each as a [T] device tensor): what that step's
        update read for its adaptive tensors (the others have a ratio here too, and ignored it), with no synchronisation.  None
        before the first step."""
        last = self.__dict__.get("_last")
        if last is None:
            return None
        live, norms = last
        T = len(live)
        if norms is None:
            return live, torch.ones(T, dtype=live[0].dtype, device=live[0].device)
        return live, norms[2 + 2 * T:2 + 3 * T]


def _adam_scalar_dtype():
    return torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32


class Adam(_Optimizer):
    """torch.optim.Adam (L2 weight decay; not AdamW, no amsgrad) with the update of all groups as one launch.  The bias corrections
    1 - beta^step are computed here in double, per tensor, from the `step` state torch keeps."""
    _op = "adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False, kernels=None):
        if amsgrad:
            raise NotImplementedError("amsgrad=True is not supported by the device optimizer step")
        if maximize:
            raise NotImplementedError("maximize=True is not supported by the device optimizer step")
        if _scalar(lr) < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults, kernels)

    @staticmethod
    def _check_group(group):
        _unsupported(group, "amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")

    @staticmethod
    def _state(rec, p):
        """create (torch's lazy initialisation) or re-validate the three state entries of one parameter"""
        state = rec.state
        st = state.get("step")
        if st is None:
            st = state["step"] = torch.tensor(0.0, dtype=_adam_scalar_dtype())
        elif not isinstance(st, torch.Tensor) or st.device.type != "cpu" or st.dim() != 0:
            # a state saved by a fused / capturable torch.optim.Adam keeps `step` on the device: host it, as the default does
            st = state["step"] = torch.as_tensor(st, dtype=_adam_scalar_dtype()).detach().cpu().reshape(())
        rec.s1, _ = _state_tensor(state, "exp_avg", p, torch.zeros_like)
        rec.s2, _ = _state_tensor(state, "exp_avg_sq", p, torch.zeros_like)
        rec.step, rec.step_np = st, st.numpy()           # a view: the step is read and advanced without a torch call

    def _update(self, mt):
        kern, recs, strided = mt.kern, self._records(), torch.strided
        ent, hyp, live, keep = [], [], [], []                       # ent: (p, g, exp_avg, exp_avg_sq address, elements) per tensor
        dev, p0 = None, None
        for group in self.param_groups:
            self._check_group(group)
            b1, b2 = (_scalar(b) for b in group["betas"])
            h = (_scalar(group["lr"]), b1, b2, float(group["eps"]), _scalar(group["weight_decay"]))
            before = len(ent)
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                rec = recs.get(id(p))
                ptr = p.data_ptr()
                if rec is None or rec.p is not p or rec.ptr != ptr or dev is None or not p.is_contiguous() \
                        or g.layout is not strided or not g.is_contiguous():
                    rec, g = self._admit(recs, p, g, kern, dev, keep)
                    dev = p.device
                n = p.numel()
                if n == 0:
                    continue
                state = rec.state
                m = state.get("exp_avg")
                if m is None or m is not rec.s1 or state.get("exp_avg_sq") is not rec.s2 or state.get("step") is not rec.step:
                    self._state(rec, p)
                p0 = p
                ent.append((ptr, g.data_ptr(), rec.s1.data_ptr(), rec.s2.data_ptr(), n))
                live.append(rec)
            hyp.extend([h] * (len(ent) - before))
        if not ent:
            return
        kern.check([p0])
        rows, memo, last = [], {}, None
        for h, rec in zip(hyp, live):                        # every check has passed: the steps may move
            a = rec.step_np
            t = float(a) + 1.0
            a[()] = t
            if h is not last:
                memo, last = {}, h
            row = memo.get(t)
            if row is None:
                lr, b1, b2, eps, wd = h
                bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
                row = memo[t] = (lr / bc1, 1.0 - b1, b2, 1.0 - b2, eps, wd, math.sqrt(bc2))
            rows.append(row)
        cols = np.array(ent, dtype=np.uint64)
        mt.run(build_descriptors(cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 3], cols[:, 4], rows), dev)


def _params_of(x, what):
    if isinstance(x, torch.nn.Module):
        return list(x.parameters())
    if isinstance(x, torch.Tensor):
        raise TypeError(f"momentum_update: {what} is a module or an iterable of parameters, not one tensor")
    return list(x)


@torch.no_grad()
def momentum_update(key, query, m, *, kernels=None):
    """param_k = param_k * m + param_q * (1 - m) over every parameter pair of two modules (or two parameter iterables) of equal
    structure, as one launch (the reference's _momentum_update_key_encoder).  Parameters only, not buffers.  m and 1 - m are taken
    in double."""
    kern = _kern(kernels)
    K, Q = _params_of(key, "key"), _params_of(query, "query")
    if len(K) != len(Q):
        raise ValueError(f"momentum_update: {len(K)} key parameters against {len(Q)} query parameters")
    m = float(m)
    if not 0.0 <= m <= 1.0:
        raise ValueError(f"momentum_update: m = {m} outside [0, 1]")
    dev = None
    for i, (k, q) in enumerate(zip(K, Q)):
        if k.shape != q.shape:
            raise ValueError(f"momentum_update: parameter {i}: key {tuple(k.shape)} against query {tuple(q.shape)}")
        _check_param(k, kern, dev, "momentum_update")
        dev = k.device
        _check_param(q, kern, dev, "momentum_update")
    live = [i for i, k in enumerate(K) if k.numel() > 0]
    if not live:
        return
    kern.check([K[live[0]], Q[live[0]]])
    mt = kern.__dict__.get("_ema_launch")
    if mt is None:
        mt = kern.__dict__["_ema_launch"] = MultiTensorLaunch("ema", kern)
    desc = build_descriptors([K[i].data_ptr() for i in live], [Q[i].data_ptr() for i in live], 0, 0, [K[i].numel() for i in live],
                             [(m, 1.0 - m)] * len(live))
    mt.run(desc, dev)


def _live_grads(parameters, kern, what, in_place):
    """the gradients of `parameters` that exist and have elements -> (gradients, indices among the existing ones, how many exist,
    device); raises with the reason before anything is launched"""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    live, idx, dev = [], [], None
    for i, g in enumerate(grads):
        if g.is_sparse or g.layout != torch.strided:
            raise RuntimeError(f"{what} does not support sparse gradients")
        if g.dtype != kern.dtype:
            raise TypeError(f"{what}: {g.dtype} gradient; the device norm is {kern.dtype} only")
        if dev is not None and g.device != dev:
            raise ValueError(f"{what}: gradients on more than one device ({dev} and {g.device})")
        dev = g.device
        if not g.is_contiguous():
            if in_place:
                raise ValueError(f"{what}: non-contiguous gradient of shape {tuple(g.shape)}; clipping is in place")
            g = g.contiguous()
        if g.numel() > 0:
            live.append(g)
            idx.append(i)
    return live, idx, len(grads), dev


def _norm_mode(norm_type, what):
    t = float(norm_type)
    if t == 2.0:
        return "l2"
    if t == math.inf:
        return "inf"
    raise NotImplementedError(f"{what}: norm_type={norm_type}: the device norm pass computes sums of squares and maxima only (norm_type 2 and inf)")


def _grad_table(live, kern):
    mt = kern.__dict__.get("_grad_launch")
    if mt is None:
        mt = kern.__dict__["_grad_launch"] = MultiTensorLaunch("grad", kern)
    return mt, build_descriptors([0] * len(live), [g.data_ptr() for g in live], 0, 0, [g.numel() for g in live], [(0.0,)] * len(live))


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None, *, kernels=None):
    """torch.nn.utils.clip_grad_norm_ in at most three launches: the norm of all gradients taken together (per-item sums of squares
    or maxima in double, folded per tensor and over the tensors in a fixed order), then gradients *= min(max_norm / (total + 1e-6), 1)
    in place, the coefficient read on the device and rounded as torch rounds it.  Returns the total norm as a 0-dim tensor on the
    device; nothing is read back, and when nothing clips no gradient is written.

    norm_type: 2 or inf; anything else raises NotImplementedError.  error_if_nonfinite=True raises RuntimeError on a nan / inf total
    before anything is scaled, and costs the one read-back that decision needs.  foreach is accepted and ignored: every gradient is
    in the one launch.  Parameters without a gradient are skipped; with none left the result is a zero tensor, as torch's.  A
    non-contiguous gradient raises: clipping is in place.  max_norm=inf only measures (two launches)."""
    kern = _kern(kernels)
    what = "clip_grad_norm_"
    mode = _norm_mode(norm_type, what)
    max_norm = float(max_norm)
    if math.isnan(max_norm):
        raise ValueError(f"{what}: max_norm is nan")
    live, _, _, dev = _live_grads(parameters, kern, what, True)
    if not live:
        return torch.tensor(0.0)
    kern.check(live[:1])
    mt, desc = _grad_table(live, kern)
    norms = mt.norms(desc, dev, mode, max_norm if math.isfinite(max_norm) else 1.0)
    total = norms[0]
    if error_if_nonfinite and not bool(torch.isfinite(total)):
        raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, so it cannot be "
                           "clipped. To disable this error and scale the gradients by the non-finite norm anyway, set "
                           "`error_if_nonfinite=False`")
    if math.isfinite(max_norm):
        mt.scale(desc, dev, norms)
    return total


@torch.no_grad()
def grad_norm(parameters, norm_type=2.0, per_tensor=False, *, kernels=None):
    """the norm of the gradients of `parameters`, for logging: clip_grad_norm_'s two read-only launches, nothing read back.  Returns
    the 0-dim total on the device, or with per_tensor=True a [T] tensor of the norms of the T parameters that have a gradient, in
    parameter order.  A non-contiguous gradient is copied for the call."""
    kern = _kern(kernels)
    mode = _norm_mode(norm_type, "grad_norm")
    live, idx, n_grads, dev = _live_grads(parameters, kern, "grad_norm", False)
    if not live:
        return torch.zeros(n_grads) if per_tensor else torch.tensor(0.0)
    kern.check(live[:1])
    mt, desc = _grad_table(live, kern)
    T = len(live)
    norms = mt.norms(desc, dev, mode)
    if not per_tensor:
        return norms[0]
    row = norms[2 + T:2 + 2 * T]
    if T == n_grads:
        return row
    out = torch.zeros(n_grads, dtype=row.dtype, device=row.device)          # gradients without elements: norm 0
    out[torch.tensor(idx, device=row.device)] = row
    return out

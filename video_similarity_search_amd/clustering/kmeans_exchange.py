"""
The sharded k-means' side of the process group (driver: clustering/kmeans_hip.py): the library's own communicators and their life-cycle,
and `Exchange` — everything a sharded fit asks of its group, resolved ONCE per fit: the route of the iteration's one collective
(SLIC_KMEANS_EXCHANGE / exchange=, SLIC_KMEANS_COMM, the group's backend), the payload's dtype and number of parts, the bounded wait of
the status read, and the small set-up / wrap-up exchanges (all-gather, broadcast of rank 0's draws).
"""
import atexit
import ctypes
import os
import socket
import weakref

import torch

from .. import _lib
from .._lib import call, ptr, stream


# process group -> slic_comm* (an RCCL communicator of the library's own, created once per group).  Keyed on the group OBJECT through
# weak references: a destroyed group's id() may be re-used by a new group with other members, and a stale communicator would hang or
# reduce over the wrong ranks; when the group goes away its communicator is destroyed with it.
_COMMS = weakref.WeakKeyDictionary()
_ONESHOTS = weakref.WeakKeyDictionary()

_EXITING = []


def _mark_exiting():
    _EXITING.append(True)


class _CommHandle:
    """owns one slic_comm*: slic_comm_destroy (finalize, bounded settle, destroy) when the handle dies because its group was collected;
    slic_comm_abort at interpreter exit — torch may have torn its process group down by then and a peer may be gone: the exit path
    must not wait for anybody"""

    _hooked = False

    def __init__(self, ptr_):
        self.ptr = ptr_
        self._fin = weakref.finalize(self, _CommHandle._close, ptr_)
        if not _CommHandle._hooked:
            # registered AFTER weakref's own exit hook (created with the first finalize object), so it runs BEFORE it (LIFO)
            atexit.register(_mark_exiting)
            _CommHandle._hooked = True

    @staticmethod
    def _close(ptr_):
        try:
            lib = _lib.load()
            (lib.slic_comm_abort if _EXITING else lib.slic_comm_destroy)(ptr_)
        except Exception:
            pass


def comm_timeout_ms():
    """deadline of the library communicator's waits (SLIC_COMM_TIMEOUT_MS, default five minutes — torch.distributed's own collectives
    default to ten): a peer that never joins makes every rank raise instead of hang"""
    return int(os.environ.get("SLIC_COMM_TIMEOUT_MS", "300000"))


def _slic_comm(pg, dev):
    """the C-ABI communicator for the sharded iteration's all-reduce (include/slic_hip.h: slic_comm_create_timeout): rank 0 of the
    group draws the unique id, torch.distributed carries it to the others, every rank joins on its device — under a deadline"""
    h = _COMMS.get(pg)
    if h is not None:
        return h.ptr
    lib = _lib.load()
    W, rank = torch.distributed.get_world_size(pg), torch.distributed.get_rank(pg)
    idt = torch.zeros(128, dtype=torch.uint8, device=dev)
    if rank == 0:
        buf = (ctypes.c_ubyte * 128)()
        _lib.check(lib.slic_comm_unique_id(buf), "slic_comm_unique_id")
        idt.copy_(torch.tensor(list(buf), dtype=torch.uint8))
    torch.distributed.broadcast(idt, src=torch.distributed.get_global_rank(pg, 0), group=pg)
    raw = bytes(idt.cpu().numpy().tobytes())
    comm = ctypes.c_void_p()
    _lib.check(lib.slic_comm_create_timeout(raw, W, rank, comm_timeout_ms(), ctypes.byref(comm)), "slic_comm_create_timeout")
    _COMMS[pg] = _CommHandle(comm)
    return comm


class _OneshotHandle:
    """owns one slic_oneshot*; destroyed with its process group or at interpreter exit (slic_oneshot_destroy never waits for a peer)"""

    def __init__(self, ptr_, max_n):
        self.ptr, self.max_n = ptr_, max_n
        self._fin = weakref.finalize(self, _OneshotHandle._close, ptr_)

    @staticmethod
    def _close(ptr_):
        try:
            _lib.load().slic_oneshot_destroy(ptr_)
        except Exception:
            pass


def _pg_all_gather_bytes(pg, raw, dev):
    """all-gather one small byte string per rank over the process group (RCCL: device tensors; gloo: host tensors) -> bytes, rank order"""
    W = torch.distributed.get_world_size(pg)
    on_dev = torch.distributed.get_backend(pg) == "nccl"
    t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).clone()
    t = t.to(dev) if on_dev else t
    out = torch.empty(W * t.numel(), dtype=torch.uint8, device=t.device)
    torch.distributed.all_gather_into_tensor(out, t, group=pg)
    return bytes(out.cpu().numpy().tobytes())


def _slic_oneshot(pg, dev, n):
    """the one-shot exchange of the sharded iteration (include/slic_hip.h: slic_oneshot_*): every rank allocates its inbox, the IPC handles
    travel over the process group, every rank maps its peers.  One communicator per group, re-made when a larger payload comes along."""
    h = _ONESHOTS.get(pg)
    if h is not None and h.max_n >= n:
        return h.ptr
    lib = _lib.load()
    W, rank = torch.distributed.get_world_size(pg), torch.distributed.get_rank(pg)
    if W > 1 and os.environ.get("SLIC_ONESHOT_MULTI_GPU", "0") != "1":
        # EXPERIMENTAL between GPUs: every test of this exchange ran its ranks as processes on ONE device (one-GPU boxes); a run over xGMI has
        # never been compared with the all-reduce route.  Ranks on different devices must opt in.  Every rank sees the same
        # gathered identities, so every rank raises (or none does).
        pr = torch.cuda.get_device_properties(dev)
        ident = "%s/%s/%s/%s/%s" % (socket.gethostname(), getattr(pr, "uuid", ""), getattr(pr, "pci_domain_id", ""), getattr(pr, "pci_bus_id", ""),
                                    getattr(pr, "pci_device_id", ""))
        ids = _pg_all_gather_bytes(pg, ident.encode()[:96].ljust(96, b"\0"), dev)
        if len({ids[i * 96:(i + 1) * 96] for i in range(W)}) > 1:
            raise _lib.SlicError("exchange='oneshot' between different GPUs is experimental (never verified against the RCCL all-reduce on a multi-GPU "
                                 "node): set SLIC_ONESHOT_MULTI_GPU=1 to opt in, or use exchange='allreduce'")
    hb = 64
    mine = (ctypes.c_ubyte * hb)()
    comm = ctypes.c_void_p()
    with torch.cuda.device(dev):
        _lib.check(lib.slic_oneshot_create(W, rank, n, comm_timeout_ms(), ctypes.byref(comm), mine), "slic_oneshot_create")
        allh = _pg_all_gather_bytes(pg, bytes(mine), dev)
        _lib.check(lib.slic_oneshot_connect(comm, allh), "slic_oneshot_connect")
    # nobody may push into an inbox before its owner has mapped... (a push only needs the PUSHER's mapping; the barrier keeps a fast rank's
    # first exchange from racing a slow rank's connect bookkeeping and gives create / connect failures a common point to surface)
    torch.distributed.barrier(group=pg)
    _ONESHOTS[pg] = _OneshotHandle(comm, n)
    return comm


def _gather(pg, staged, t):
    """all-gather a per-rank tensor [*] -> [W, *] (same shape on every rank); staged: through host copies"""
    W = torch.distributed.get_world_size(pg)
    src = t.contiguous().reshape(-1)
    if staged:
        src = src.cpu()
    flat = torch.empty(W * t.numel(), dtype=t.dtype, device=src.device)    # concatenated form (gloo and RCCL)
    torch.distributed.all_gather_into_tensor(flat, src, group=pg)
    return flat.to(t.device).view((W,) + tuple(t.shape))


class Exchange:
    """What one sharded fit asks of its process group.  Built once, in KMeans.fit(); `kind` is 'allreduce', 'allgather' or 'oneshot',
    `n` the payload's length K*D + K + 2.  The Lloyd loop uses
        dtype, n_parts          the payload's element type, and how many payloads the global half combines (1: reduced in place; W: gathered)
        reduce(payload, parts)  the iteration's ONE collective, enqueued / run on the chosen route (parts is payload itself where n_parts == 1)
        sync(event)             host wait for an iteration's status read-back — bounded where the route is the library's own
        communicator_kind_, payload_bytes_   what a benchmark line reports about the exchange (bench.py: secondary.exchange)"""

    def __init__(self, pg, kind, dev, n):
        self.pg = pg
        self.world = torch.distributed.get_world_size(pg)
        self.rank = torch.distributed.get_rank(pg)
        backend = torch.distributed.get_backend(pg)
        on_gpu = dev.type == "cuda"
        # device tensors over a gloo group (two ranks sharing ONE GPU — how a one-GPU box runs exchange='oneshot' with two processes; RCCL
        # cannot put two ranks on a device) go through host copies; RCCL groups and host tensors are used as they are
        self._gloo = backend == "gloo"
        self._staged = on_gpu and self._gloo
        reduced = kind in ("allreduce", "oneshot")
        self.dtype = torch.float64 if reduced else torch.float32
        self.n_parts = 1 if reduced else self.world
        self.payload_bytes_ = int(n * (8 if reduced else 4))
        self.sync = torch.cuda.Event.synchronize
        if kind == "oneshot":
            # the library's one-shot all-to-all over peer-mapped memory (slic_allreduce_oneshot_f64: one kernel per iteration instead of a
            # ring all-reduce; csrc/oneshot.hip).  The process group only carries the IPC handles at set-up.
            assert on_gpu, "exchange='oneshot' moves device memory between GPUs"
            oneshot = _slic_oneshot(pg, dev, n)
            self.communicator_kind_ = "slic_oneshot (peer-mapped inboxes, one kernel per exchange; no RCCL in the loop)"
            self.reduce = lambda payload, parts: call("slic_allreduce_oneshot_f64", oneshot, ptr(payload), payload.numel(), stream())

            def sync(event):
                event.synchronize()
                call("slic_oneshot_check", oneshot)      # the exchange kernel never hangs: a wait that ran out (a lost peer) surfaces here
            self.sync = sync
        elif kind == "allreduce" and on_gpu and backend == "nccl" and os.environ.get("SLIC_KMEANS_COMM", "torch") == "slic":
            # the all-reduce goes through torch.distributed's process group by default (below: RCCL on the GPU, gloo in the CPU tests): its
            # collectives carry the group's timeout and it is the path every multi-rank test runs.  SLIC_KMEANS_COMM=slic opts into the
            # library's own RCCL communicator (slic_allreduce_f64 on the compute stream, the C ABI's collective for callers without
            # torch.distributed); its waits are bounded too (slic_comm_create_timeout / slic_comm_wait)
            comm = _slic_comm(pg, dev)
            self.communicator_kind_ = "slic_comm (the library's own RCCL communicator, slic_allreduce_f64)"
            self.reduce = lambda payload, parts: call("slic_allreduce_f64", comm, ptr(payload), payload.numel(), stream())

            def sync(event):
                # bounded: a peer that never joined the iteration's all-reduce aborts the communicator and raises here.  The wait is on
                # THIS iteration's event (recorded behind its collective and status read-back): the next iteration, already enqueued,
                # keeps running ahead, and the deadline covers one iteration
                call("slic_comm_wait_event", comm, ctypes.c_void_p(event.cuda_event), comm_timeout_ms())
                event.synchronize()
            self.sync = sync
        else:
            # (the callables below close over the group, not over this object: an Exchange that referred to itself would be freed by the
            # cycle collector only, and would keep the group alive past torch.distributed.destroy_process_group())
            self.communicator_kind_ = f"torch.distributed process group ({backend})"
            staged = self._staged
            if kind == "allgather":
                if staged:
                    self.reduce = lambda payload, parts: parts.copy_(_gather(pg, True, payload.view(-1)).view_as(parts))
                else:
                    self.reduce = lambda payload, parts: torch.distributed.all_gather_into_tensor(parts.view(-1), payload.view(-1), group=pg)
            elif staged:
                def reduce(payload, parts):
                    h = payload.cpu()
                    torch.distributed.all_reduce(h, group=pg)
                    payload.copy_(h)
                self.reduce = reduce
            else:
                self.reduce = lambda payload, parts: torch.distributed.all_reduce(payload, group=pg)

    # ---- the fit's small set-up / wrap-up exchanges (shard sizes, column statistics, relocation candidates, inertia, k-means++)
    def gather(self, t):
        """all-gather a per-rank tensor [*] -> [W, *] (same shape on every rank)"""
        return _gather(self.pg, self._staged, t)

    def bcast(self, a, dev):
        """rank 0's numpy array on every rank"""
        t = torch.from_numpy(a)
        t = t if self._gloo else t.to(dev)
        torch.distributed.broadcast(t, torch.distributed.get_global_rank(self.pg, 0), group=self.pg)
        return t.cpu().numpy()

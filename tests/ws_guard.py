"""A guarded, exact-size, poisoned stand-in for `_lib.workspace`, for the workspace-contract tests (test_workspace_contract_gpu.py).

The production `_lib.workspace` is a grow-only cache per (device, tag, stream): inside one pytest process a small shape nearly always
runs on a buffer an earlier, larger case grew, so a size query that is short at exactly the small shapes, or a kernel that reads a
workspace slot nothing in the same call wrote, cannot be seen.  Under `guarded(monkeypatch, poison)` every request gets

  * a uint8 view of EXACTLY `nbytes` bytes (no `max(nbytes, 256)`),
  * inside a larger allocation with a GUARD-byte region on both sides, each filled with the `i % 251` pattern of test_hdbscan_gpu.py
    (GUARD = 64 KiB is a multiple of 4096, so the view keeps the alignment of a fresh torch allocation): an overrun lands in memory the
    test owns and is a failed assertion, never a fault,
  * an interior filled ONCE, at creation, with the poison byte the test chose: 0x00, or 0xFF (NaN as float and double, -1 as int32).

Buffers are keyed by (device, tag, stream, nbytes): the same key returns the same buffer, not poisoned again, so state a driver keeps
in its workspace across the calls of one fit survives; another size under the same tag gets a fresh exact buffer.  `log` lists the
(tag, nbytes) requests in order; `check()` synchronises and asserts every guard byte of every buffer.

Not a conftest.py and not a plugin: a plain module the tests import.  `_lib.workspace` itself is left as it is; the drivers call it as
`_lib.workspace(...)`, so one monkeypatch.setattr reaches them all."""
import contextlib

import torch

GUARD = 64 * 1024
POISONS = (0x00, 0xFF)


class GuardedWorkspace:
    def __init__(self, poison):
        assert poison in POISONS, "poison byte must be 0x00 or 0xFF"
        self.poison = poison
        self.log = []                    # (tag, nbytes) of every request, in order
        self._bufs = {}                  # (device, tag, stream, nbytes) -> (whole allocation, view)
        self._pattern = {}               # device -> the guard pattern there

    def _guard(self, device):
        key = str(device)
        if key not in self._pattern:
            self._pattern[key] = (torch.arange(GUARD, device=device) % 251).to(torch.uint8)
        return self._pattern[key]

    def __call__(self, nbytes, device, tag="default"):
        nbytes = int(nbytes)
        assert nbytes >= 0, f"workspace request of {nbytes} bytes under tag {tag!r}"
        self.log.append((tag, nbytes))
        key = (str(device), tag, torch.cuda.current_stream().cuda_stream, nbytes)
        hit = self._bufs.get(key)
        if hit is None:
            whole = torch.empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device=device)
            whole[:GUARD] = self._guard(device)
            whole[GUARD + nbytes:] = self._guard(device)
            whole[GUARD:GUARD + nbytes] = self.poison
            hit = self._bufs[key] = (whole, whole[GUARD:GUARD + nbytes])
        return hit[1]

    def allocation(self, view):
        """the whole allocation (guard | view | guard) a view handed out earlier lies in"""
        for whole, v in self._bufs.values():
            if v.data_ptr() == view.data_ptr() and v.numel() == view.numel():
                return whole
        raise KeyError("not a view of this allocator")

    def lookup(self, address):
        """(tag, nbytes) of the view that starts at a device address (what a driver passed to the library), or None"""
        for (_, tag, _, nbytes), (_, v) in self._bufs.items():
            if v.data_ptr() == address:
                return tag, nbytes
        return None

    def sizes(self, tag):
        """the sizes requested under `tag`, in order of first request, each once"""
        return list(dict.fromkeys(n for t, n in self.log if t == tag))

    def tags(self):
        return set(t for t, _ in self.log)

    def check(self):
        torch.cuda.synchronize()
        for (device, tag, _, nbytes), (whole, _) in self._bufs.items():
            pat = self._guard(whole.device)
            lo, hi = whole[:GUARD], whole[GUARD + nbytes:]
            if not torch.equal(lo, pat):
                bad = torch.nonzero(lo != pat).flatten()
                raise AssertionError(f"workspace {tag!r} of {nbytes} bytes on {device}: {bad.numel()} bytes written BEFORE it, "
                                     f"the farthest {GUARD - int(bad[0])} bytes before its start")
            if not torch.equal(hi, pat):
                bad = torch.nonzero(hi != pat).flatten()
                raise AssertionError(f"workspace {tag!r} of {nbytes} bytes on {device}: {bad.numel()} bytes written PAST it, "
                                     f"the farthest at offset {nbytes + int(bad[-1])}")


@contextlib.contextmanager
def guarded(monkeypatch, poison):
    """with guarded(monkeypatch, 0xFF) as ws: run a driver; ws.check(); ws.log ...  The patch ends with the block."""
    from video_similarity_search_amd import _lib
    ws = GuardedWorkspace(poison)
    with monkeypatch.context() as m:
        m.setattr(_lib, "workspace", ws)
        yield ws


@contextlib.contextmanager
def spy_calls(monkeypatch, modules, size_rules):
    """Record what the drivers of `modules` hand to the library.  Those modules reach it as `call(name, *args)` (imported from _lib),
    so the name `call` is replaced in each of them for the block.  size_rules: entry point -> f(lib, args) = the bytes its
    `*_workspace_bytes` query returns for the arguments of THIS call, worked out before the call is forwarded (the argument struct
    is the driver's own and may change afterwards).  The workspace pointer is the argument before the stream.
    -> a list of (entry point, workspace address, bytes the query asks for)."""
    from video_similarity_search_amd import _lib
    lib, real, seen = _lib.load(), _lib.call, []

    def call(name, *args):
        rule = size_rules.get(name)
        if rule is not None:
            seen.append((name, getattr(args[-2], "value", args[-2]), int(rule(lib, args))))
        return real(name, *args)

    with monkeypatch.context() as m:
        for mod in modules:
            m.setattr(mod, "call", call)
        yield seen


def run_both(monkeypatch, fn):
    """fn() under poison 0x00, then under 0xFF in a fresh allocator; guards checked after each -> [(outputs, ws), (outputs, ws)]"""
    runs = []
    for poison in POISONS:
        with guarded(monkeypatch, poison) as ws:
            out = fn()
            ws.check()
        runs.append((out, ws))
    return runs

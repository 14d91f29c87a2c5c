"""Poisoned and guarded device outputs: no test passes on stale bytes, no store past an output goes unseen.

Every output the library writes is a torch.empty (or torch.zeros) of retargetvid_amd/ops.py and transnetv1_handler.py.  PyTorch's
caching allocator hands a freed block to the next request of its size, so the second of two twin calls that a test compares
receives the block that already holds the expected bytes: a kernel that leaves a row tail unwritten passes.  Poison stands in
for the `torch` module of those two files: everything passes through, but empty() / zeros() carve the tensor out of a uint8 base of
G + nbytes + G bytes that is filled with one byte value first.  What a kernel does not write then reads as the fill, and check()
finds every store that landed in a guard band.

The fill 0xA5 reads as a finite float32 / float64 (-2.9e-16 / -2.5e-127) that no correct result takes -- NaN is a legitimate centre,
so the fill must not read as one; 0x5A is the second fill of the directed tests (tests/test_gpu_write_extent.py): a byte that
equals its reference under both fills was written.  G = 256 keeps the 16-byte phase of a plain allocation (the allocator's blocks are
512-aligned), so every test takes the vector kernels it took before; phase= moves the data to G + phase for the directed tests.

The fixture `poisoned_outputs` puts one Poison in place for one test and checks the guards at teardown; a module opts in with
pytest.mark.usefixtures('poisoned_outputs') after importing the fixture from here.

The same hole inside the library: a handle keeps its workspaces from call to call (DevBuf::ensure only grows), so a kernel that reads a
value its pass should have computed reads the previous call's -- often the right one.  The fixture `poisoned_workspaces` turns the
library's test switch on (svc_debug_scratch_fill, 0xFF) for one test; tests/test_gpu_scratch.py has the directed cases."""
import sys
import threading

import pytest
import torch

G = 256                     # bytes of guard band on either side of the data
FILL, FILL2 = 0xA5, 0x5A
FILLS = (FILL, FILL2)
LIMIT = 1 << 30             # bytes the registry may pin before check() runs early


class Poison:
    """A proxy for the torch module whose empty() and zeros() return poisoned (zeroed) and guarded tensors."""

    def __init__(self, fill=FILL, limit=LIMIT):
        assert 0 <= int(fill) <= 255
        self.fill, self.limit = int(fill), int(limit)
        self._lock = threading.Lock()
        self._held = []                 # (base, offset of the data, nbytes, description)
        self._bytes = 0
        self.allocations = 0            # over the proxy's life (check() does not reset it)

    def __getattr__(self, name):        # (only what the instance does not have: everything but empty / zeros and the above)
        return getattr(torch, name)

    # -- the two allocators -----------------------------------------------------------------------------------------------
    def empty(self, *size, dtype=None, device=None, phase=0):
        return self._alloc(size, dtype, device, phase, zero=False)

    def zeros(self, *size, dtype=None, device=None, phase=0):
        return self._alloc(size, dtype, device, phase, zero=True)

    def _alloc(self, size, dtype, device, phase, zero):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = size[0]
        shape = tuple(int(v) for v in size)
        dtype = torch.get_default_dtype() if dtype is None else dtype
        item = torch.empty((), dtype=dtype).element_size()
        phase = int(phase)
        if not 0 <= phase < 16 or phase % item:
            raise ValueError('phase %d: 0..15 and a multiple of the %d-byte element' % (phase, item))
        count = 1
        for v in shape:
            count *= v
        nbytes, off = count * item, G + phase
        base = torch.full((off + nbytes + G,), self.fill, dtype=torch.uint8, device=device)      # on the current stream
        data = base[off:off + nbytes]
        if zero:
            data.zero_()
        f = sys._getframe(2)
        what = '%s%s %s at %s:%d (%s)' % ('zeros' if zero else 'empty', shape, str(dtype).replace('torch.', ''),
                                         f.f_code.co_filename, f.f_lineno, f.f_code.co_name)
        with self._lock:
            self._held.append((base, off, nbytes, what))
            self._bytes += int(base.numel())
            self.allocations += 1
            early = self._bytes > self.limit
        if early:                       # a long test does not pin memory: what is held so far is checked and let go
            self.check(keep=base)
        return data.view(dtype).view(shape)

    # -- the guards -------------------------------------------------------------------------------------------------------
    def held(self):
        with self._lock:
            return len(self._held)

    def check(self, keep=None):
        """Synchronise, assert that both guard bands of every buffer handed out since the last check still hold the fill (the
        AssertionError names every buffer that does not: shape, dtype, call site, where the strays lie), forget the buffers.
        One comparison and one read per device, however many buffers.  keep: a base that stays registered."""
        with self._lock:
            held, self._held, self._bytes = self._held, [], 0
            if keep is not None:
                mine = [e for e in held if e[0] is keep]
                held = [e for e in held if e[0] is not keep]
                self._held, self._bytes = mine, sum(int(e[0].numel()) for e in mine)
        by_dev = {}
        for e in held:
            by_dev.setdefault(e[0].device, []).append(e)
        bad = []
        for dev, group in by_dev.items():
            if dev.type == 'cuda':
                torch.cuda.synchronize(dev)
            bands = torch.cat([b for base, off, nbytes, _ in group for b in (base[:off], base[off + nbytes:])])
            if bool((bands != self.fill).any()):
                for base, off, nbytes, what in group:
                    front = torch.nonzero(base[:off] != self.fill).flatten().cpu().tolist()
                    back = torch.nonzero(base[off + nbytes:] != self.fill).flatten().cpu().tolist()
                    if front or back:
                        bad.append('%s: %d byte(s) written below the data (nearest %d before its start), %d behind it (first at end + %d)'
                                   % (what, len(front), off - front[-1] if front else 0, len(back), back[0] if back else 0))
        assert not bad, 'stores outside an output:\n  ' + '\n  '.join(bad)


WS_FILL, WS_FILL2 = 0xFF, 0x7F     # the library's scratch: NaN in fp32 and in every bf16 plane; 3.39e38, which a clamp and a maximum keep
WS_SETTINGS = (None, WS_FILL, WS_FILL2)


@pytest.fixture
def poisoned_workspaces():
    """The library's own scratch -- the workspaces a handle keeps from call to call at the same addresses -- is filled with 0xFF before
    every pass of this test (ops.scratch_fill, process-wide: the session's engine, module-scoped nets, cloned nets and scheduler lanes
    all obey it), so no pass rides what the previous call left there; switched off at teardown, also when the test raised."""
    from retargetvid_amd import ops
    ops.scratch_fill(WS_FILL)
    try:
        yield WS_FILL
    finally:
        ops.scratch_fill(None)


@pytest.fixture
def poisoned_outputs(monkeypatch):
    """The outputs of retargetvid_amd.ops and .transnetv1_handler are poisoned and guarded for this test; guards checked at teardown."""
    from retargetvid_amd import ops, transnetv1_handler
    p = Poison()
    monkeypatch.setattr(ops, 'torch', p)
    monkeypatch.setattr(transnetv1_handler, 'torch', p)
    yield p
    p.check()

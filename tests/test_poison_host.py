"""The detector detects (tests/poison.py on CPU tensors, no GPU): a stray byte on either side of an output fails check(), an
untouched buffer passes, unwritten bytes differ from what was expected under both fills, and the view is what ops._need_cuda asks for."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import poison
from poison import poisoned_outputs  # noqa: F401  (a fixture)


def _write(addr, value, count=1):
    ctypes.memset(ctypes.c_void_p(addr), value, count)


@pytest.mark.parametrize('fill', poison.FILLS)
def test_a_stray_byte_behind_the_data_fails_the_check(fill):
    p = poison.Poison(fill)
    t = p.empty((3, 5, 7), dtype=torch.uint8)
    _write(t.data_ptr() + t.numel(), fill ^ 0xFF)
    with pytest.raises(AssertionError) as e:
        p.check()
    msg = str(e.value)
    assert 'empty(3, 5, 7) uint8' in msg and 'test_poison_host.py' in msg and '1 behind it (first at end + 0)' in msg
    assert p.held() == 0
    p.check()                                                   # the registry was cleared


@pytest.mark.parametrize('fill', poison.FILLS)
def test_a_stray_byte_below_the_data_fails_the_check(fill):
    p = poison.Poison(fill)
    ok = p.empty(9, dtype=torch.float64)
    t = p.zeros((4, 2), dtype=torch.int32)
    _write(t.data_ptr() - 1, 0)
    with pytest.raises(AssertionError) as e:
        p.check()
    msg = str(e.value)
    assert 'zeros(4, 2) int32' in msg and '1 byte(s) written below the data (nearest 1 before its start)' in msg
    assert 'float64' not in msg and ok.numel() == 9             # only the buffer that was hit is named


def test_the_far_ends_of_both_bands_are_watched():
    for at in (-poison.G, poison.G - 1):
        p = poison.Poison()
        t = p.empty((16,), dtype=torch.uint8)
        _write(t.data_ptr() + (at if at < 0 else t.numel() + at), 0)
        with pytest.raises(AssertionError):
            p.check()


@pytest.mark.parametrize('fill', poison.FILLS)
def test_an_untouched_and_a_fully_written_buffer_pass(fill):
    p = poison.Poison(fill)
    a = p.empty((2, 33), dtype=torch.uint8)
    b = p.empty((2, 33), dtype=torch.uint8, phase=9)
    z = p.zeros(5, dtype=torch.float32)
    e = p.empty((0, 4), dtype=torch.int32)
    b.copy_(torch.arange(66, dtype=torch.uint8).reshape(2, 33))
    _write(a.data_ptr(), 1, a.numel())                          # every byte of the data, none of the guards
    assert p.held() == 4
    p.check()
    assert p.held() == 0 and (a == 1).all() and (z == 0).all() and e.numel() == 0
    assert b.flatten().tolist() == list(range(66))


def test_unwritten_bytes_differ_from_the_expected_under_both_fills():
    """A 'kernel' that skips the last 5 bytes of every 37-byte row: each skipped byte differs from the expected under at least
    one fill (it can equal one fill, never both), so a byte equal to its reference under both fills was written."""
    want = np.random.RandomState(0).randint(0, 256, (6, 37)).astype(np.uint8)
    want[0, 33], want[1, 34] = poison.FILL, poison.FILL2        # the worst case: expected values that ARE a fill
    wrong = np.zeros(want.shape, bool)
    for fill in poison.FILLS:
        p = poison.Poison(fill)
        out = p.empty(want.shape, dtype=torch.uint8)
        out[:, :32] = torch.from_numpy(want[:, :32])
        got = out.numpy()
        assert (got[:, 32:] == fill).all()
        assert not np.array_equal(got, want)
        wrong |= got != want
        p.check()                                               # nothing outside the buffer: only the comparison can tell
    assert wrong[:, 32:].all() and not wrong[:, :32].any()
    z = poison.Poison().zeros((6, 37), dtype=torch.uint8)
    assert not z.numpy().any()


@pytest.mark.parametrize('dtype,shape', [(torch.uint8, (3, 14, 25, 3)), (torch.float64, (5, 2)), (torch.int32, (7, 4)), (torch.float32, (3, 17))])
def test_the_view_is_what_the_launchers_ask_for(dtype, shape):
    p = poison.Poison()
    item = torch.empty((), dtype=dtype).element_size()
    for phase in range(0, 16, item):
        for make in (lambda: p.empty(shape, dtype=dtype, phase=phase), lambda: p.zeros(*shape, dtype=dtype, phase=phase)):
            t = make()
            assert torch.is_tensor(t) and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape and not t.is_cuda
            base = p._held[-1][0]
            assert base.dtype == torch.uint8 and base.numel() == 2 * poison.G + phase + t.numel() * item
            assert t.data_ptr() - base.data_ptr() == poison.G + phase
    m = p.empty(6, dtype=torch.float64)                         # the other call form in use: empty(m, ...)
    assert tuple(m.shape) == (6,) and m.is_contiguous()
    raw = p.empty(shape, dtype=dtype).view(-1).view(torch.uint8)
    assert (raw == poison.FILL).all()
    if dtype.is_floating_point:                                 # the default fill reads as a finite number
        assert torch.isfinite(p.empty(shape, dtype=dtype)).all()
    for bad in (-1, 16, 1 if item > 1 else 17):
        with pytest.raises(ValueError):
            p.empty(shape, dtype=dtype, phase=bad)
    p.check()


def test_the_proxy_forwards_the_module():
    p = poison.Poison()
    assert p.is_tensor is torch.is_tensor and p.uint8 is torch.uint8 and p.cuda is torch.cuda
    assert p.from_numpy is torch.from_numpy and p.device is torch.device
    assert p.empty.__func__ is poison.Poison.empty and p.zeros.__func__ is poison.Poison.zeros
    with pytest.raises(AttributeError):
        p.no_such_name


def test_the_fixture_replaces_torch_in_both_modules_and_puts_it_back(poisoned_outputs):
    from retargetvid_amd import ops, transnetv1_handler
    assert ops.torch is poisoned_outputs and transnetv1_handler.torch is poisoned_outputs
    assert isinstance(poisoned_outputs, poison.Poison) and poisoned_outputs.fill == poison.FILL
    t = ops.torch.empty((2, 3), dtype=ops.torch.uint8)          # what an ops call does
    assert poisoned_outputs.held() == 1 and (t == poison.FILL).all()


def test_the_modules_have_their_torch_again():
    from retargetvid_amd import ops, transnetv1_handler
    assert ops.torch is torch and transnetv1_handler.torch is torch


def test_two_threads_allocating_at_once_lose_no_entry():
    p = poison.Poison()
    per, start, out = 400, threading.Barrier(2), [[], []]

    def work(k):
        start.wait()
        for i in range(per):
            out[k].append(p.empty((k + 1, i % 7 + 1), dtype=torch.uint8))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert p.held() == 2 * per and p.allocations == 2 * per
    assert p._bytes == sum(2 * poison.G + t.numel() for ts in out for t in ts)
    assert len({t.data_ptr() for ts in out for t in ts}) == 2 * per
    p.check()


def test_the_registry_is_checked_early_when_it_pins_too_much():
    p = poison.Poison(limit=3 * (2 * poison.G + 100))
    ts = [p.empty(100, dtype=torch.uint8) for _ in range(3)]
    assert p.held() == 3
    last = p.empty(100, dtype=torch.uint8)                      # over the limit: the first three are checked and let go
    assert p.held() == 1 and p.allocations == 4
    _write(last.data_ptr() + 100, 0)                            # the newest stays watched
    with pytest.raises(AssertionError):
        p.check()
    q = poison.Poison(limit=3 * (2 * poison.G + 100))
    ts = [q.empty(100, dtype=torch.uint8) for _ in range(3)]
    _write(ts[1].data_ptr() - 2, 0)
    with pytest.raises(AssertionError):                         # the early check itself reports
        q.empty(100, dtype=torch.uint8)

"""Poisoned scratch: for the duration of a context, every block the package allocates without initialising it is filled with a value that
a kernel must not have read.

The package owns no device memory.  Every output, partial-sum table and byte workspace that a kernel writes through a raw pointer comes from
`torch.empty`, `torch.empty_like` or `Tensor.new_empty`, and whether a kernel may read it before writing it rests on hand-sized clears and on
"every slot is written" arguments.  In a pytest process almost every block is fresh from the driver, which hands out zeros: exactly the
value that hides a forgotten clear, a fold that reads one partial slot too many, padding that is "already" zero.  `poisoned()` replaces the
three allocation calls (looked up at call time by the package and by its custom-op bodies) by versions that return the SAME tensor -- shape,
dtype, device and strides untouched -- filled with

    floating, complex   NaN (both parts)   an unwritten accumulator or a masked-by-multiply read becomes a NaN result, and every comparison
                                           of the suite is `assert err <= tol`, which NaN fails (tests/test_poison_cpu.py checks each one)
    int16 / 32 / 64     1                  differs from the driver's 0; a valid index and a harmless count (the rule of
                                           tests/test_arg_layouts_gpu.py for index padding)
    bool                True
    uint8 / int8        0xFF per byte      byte workspaces of mixed words: an int32 view reads -1, a float view reads NaN

No pattern is a large positive number when read as an integer: a latent bug must stay a wrong number and not become an out-of-bounds
access.  `meta` tensors (fake implementations) and tensors without elements pass through.  Allocations are counted per device type, so that
a test can show that it was not vacuous.

A device error ends the session (the rule of tests/test_arg_layouts_gpu.py): `device_guard()` synchronises after the test, and a
RuntimeError whose text names hip / illegal / fault / abort is answered with `pytest.exit` -- nothing more is started on the device."""
import collections
import contextlib
import re

import pytest
import torch

NAN = float("nan")
INT_POISON = 1
BYTE_POISON = 0xFF
_INTS = (torch.int16, torch.int32, torch.int64)
_FAULT_RE = re.compile(r"(?i)hip|illegal|fault|abort|device-side")
_FAULT = []  # a device error was seen: nothing more is started on the device in this session
TOTALS = collections.Counter()  # poisoned allocations of all `poisoned_case`s so far, per family (the test name up to its first "__")


def poison_(t):
    """Fill `t` in place with the poison of its dtype (see the module docstring) and return it."""
    with torch.no_grad():
        if t.dtype.is_complex:
            t.fill_(complex(NAN, NAN))
        elif t.dtype.is_floating_point:
            t.fill_(NAN)
        elif t.dtype in _INTS:
            t.fill_(INT_POISON)
        elif t.dtype == torch.bool:
            t.fill_(True)
        elif t.dtype == torch.uint8:
            t.fill_(BYTE_POISON)
        elif t.dtype == torch.int8:
            t.fill_(-1)
        else:  # a dtype the package does not allocate today: say so, do not let it through unpoisoned
            raise TypeError(f"tests/poison.py has no poison value for {t.dtype}")
    return t


class Poison:
    """What a `poisoned()` context hands out: `counts[device_type]` = number of allocations poisoned so far."""

    def __init__(self):
        self.counts = collections.Counter()

    def _wrap(self, original):
        def allocate(*args, **kwargs):
            t = original(*args, **kwargs)
            if not isinstance(t, torch.Tensor) or t.is_meta or t.numel() == 0:
                return t
            poison_(t)
            self.counts[t.device.type] += 1
            return t

        allocate.__name__ = getattr(original, "__name__", "allocate")
        allocate.__wrapped__ = original
        return allocate


@contextlib.contextmanager
def poisoned():
    """`torch.empty`, `torch.empty_like` and `torch.Tensor.new_empty` return poisoned memory inside the context; the originals are back on
    exit, also after an exception.  Yields the `Poison` with the allocation counts."""
    state = Poison()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch, "empty", state._wrap(torch.empty))
        mp.setattr(torch, "empty_like", state._wrap(torch.empty_like))
        mp.setattr(torch.Tensor, "new_empty", state._wrap(torch.Tensor.new_empty))
        yield state


def is_device_fault(exc):
    return isinstance(exc, RuntimeError) and _FAULT_RE.search(str(exc)) is not None


@contextlib.contextmanager
def device_guard(what=""):
    """Body of an autouse fixture: refuse to start after a device error, and look for one when the test is over (a kernel's fault is reported
    by the next call that synchronises, which may be nobody's)."""
    if _FAULT:
        pytest.exit(f"a device error was reported earlier ({_FAULT[0]}): no further GPU work in this session", returncode=3)
    yield
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            if not is_device_fault(e):
                raise
            _FAULT.append(f"{what}: {str(e)[:200]}")
            pytest.exit(f"device error after {what}: {str(e)[:200]}: no further GPU work in this session", returncode=3)


@contextlib.contextmanager
def poisoned_case(what="", device_type="cuda"):
    """The fixture body of tests/test_poisoned_scratch_gpu.py: device guard + poison + the check that the case was not vacuous."""
    with device_guard(what):
        with poisoned() as state:
            yield state
    TOTALS[what.split("::")[-1].split("__")[0]] += state.counts[device_type]
    assert state.counts[device_type] > 0, f"{what}: no poisoned allocation on {device_type}: the case proves nothing here and must leave the list"

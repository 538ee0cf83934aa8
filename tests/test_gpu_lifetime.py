"""What a call leaves behind on the device.

Every device allocation, pinned host allocation, stream and event of the library goes
through one counted front (csrc/ek_track.h); ``_lib.live_resources()`` reads the counts.
hipMemGetInfo would not do: the card is shared and other processes move its figures.

Three properties per entry point (tests/_lifetime_cases.py), all integers compared
with ``==``:

balance    after a warm-up call (which puts in place what the library keeps for the
           life of the process: DESIGN.md, "What stays for the life of the process"),
           three more calls leave the six live numbers -- device allocations and
           bytes, pinned allocations and bytes, streams, events -- where they were.
           For a handle: the numbers before ``open`` and after ``close``, also with an
           exception raised inside the ``with`` block.  (The seventh number, the
           monotonic count of device allocations, is what the injection below counts
           with; it cannot stand still over a call that allocates.)
raise      the same equality around every device-side raise the suite knows.
injection  A = device allocations of a clean call, read from the monotonic count; for
           each k < A the k-th allocation is made to fail (ek_fail_alloc_at: no real
           exhaustion of the shared card) and the call must raise the library's
           exception for a failed HIP call, leave the live numbers at the baseline and
           the arm clear; a clean call on a fresh handle then returns the bytes of the
           first clean call.  For a handle the failure is injected into its methods; the
           failed handle is only closed, never used again.  A case with
           ``recover = r`` has exactly r allocations whose failure the library
           survives by design (the quad copy, the active view's buffers: the case
           table says which); there the call returns the clean call's bytes, and
           exactly r of the k may do so.

No snapshot is preceded by a garbage collection except the baseline: a handle that a
call leaves to its finaliser is a handle left behind.
"""
import contextlib
import gc

import pytest

from _lifetime_cases import CASES, RAISES, bits
from enspara_amd import _lib
from enspara_amd.exception import InsufficientResourceError

pytestmark = pytest.mark.gpu

# a failed HIP call: EK_EHIP -> HipError, EK_ENOMEM -> InsufficientResourceError where
# a module tells them apart, HipError where it does not
FAILED = (_lib.HipError, InsufficientResourceError)
MAX_ALLOCS = 40


def live():
    """the six live numbers, as they stand: nothing is collected first, so a handle
    that a call under test leaves to its finaliser counts as left behind"""
    return tuple(_lib.live_resources())[:6]


def baseline():
    """the six live numbers to return to; collected once before, so that handles
    EARLIER tests left to their finalisers go now and not in the middle of this one"""
    gc.collect()
    return live()


def total():
    return _lib.live_resources().dev_allocs_total


class _Boom(Exception):
    pass


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_balance(case):
    first = bits(case.run())                        # warm-up
    before = baseline()
    for _ in range(3):
        assert bits(case.run()) == first
    assert live() == before
    if case.open is not None:
        with pytest.raises(_Boom):
            with case.open() as h:
                case.use(h)
                raise _Boom()
        assert live() == before


@pytest.mark.parametrize("name,call,exc", RAISES, ids=[r[0] for r in RAISES])
def test_raise_paths_balance(name, call, exc):
    with pytest.raises(exc):                        # warm-up
        call()
    before = baseline()
    for _ in range(3):
        with pytest.raises(exc):
            call()
    assert live() == before


INJECTED = [c for c in CASES if c.inject]


@pytest.mark.parametrize("case", INJECTED, ids=[c.name for c in INJECTED])
def test_injected_allocation_failure(case):
    want = bits(case.run())                         # warm-up, and the bytes to return
    base = baseline()
    with (case.open() if case.open else contextlib.nullcontext()) as h:
        call = (lambda: case.use(h)) if case.open else case.fn
        t0 = total()
        assert bits(call()) == want
        n_allocs = total() - t0
    assert live() == base
    print("%s: %d device allocations" % (case.name, n_allocs))
    assert n_allocs <= MAX_ALLOCS
    recovered = []
    for k in range(n_allocs):
        raised, got = False, None
        with (case.open() if case.open else contextlib.nullcontext()) as h:
            assert _lib.fail_alloc_at(k) == -1
            try:
                got = bits(case.use(h) if case.open else case.fn())
            except FAILED:
                raised = True
            finally:
                pending = _lib.fail_alloc_at(-1)
            # (the handle a failed call touched is closed here and never used again)
        assert pending == -1, "allocation %d: the arm is still set" % k
        if case.recover and not raised:
            assert got == want, "allocation %d: survived with other bytes" % k
            recovered.append(k)
        else:
            assert raised, "allocation %d failed and nothing was raised" % k
        assert live() == base, "allocation %d" % k
        assert bits(case.run()) == want, "the clean call after allocation %d" % k
    # what the library is built to survive the failure of, and nothing else
    assert len(recovered) == case.recover, recovered

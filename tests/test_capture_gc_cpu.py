"""trainer.no_gc, the guard around every stream capture: it collects the garbage that exists on entry (a dead cycle may hold a
torch.cuda.CUDAGraph, whose destructor must not run inside another capture), holds the cyclic collector off for the block and
puts it back as it was - also when the block raises, also when the collector was off before."""
import gc
import weakref

import pytest

from depthinspace_amd.trainer import no_gc


class _Node(object):
    pass


def _dead_cycle():
    a, b = _Node(), _Node()
    a.other, b.other = b, a
    return weakref.ref(a)


def test_no_gc_collects_on_entry_and_holds_the_collector_off():
    assert gc.isenabled()
    gc.disable()                 # (so that the cycle below is certainly still there on entry)
    try:
        ref = _dead_cycle()
        assert ref() is not None
    finally:
        gc.enable()
    with no_gc():
        assert ref() is None
        assert not gc.isenabled()
        inner = _dead_cycle()
        for _ in range(5000):    # far more container allocations than generation 0's threshold
            _dead_cycle()
        assert inner() is not None
    assert gc.isenabled()
    gc.collect()
    assert inner() is None


def test_no_gc_restores_the_collector_as_it_was():
    with pytest.raises(RuntimeError):
        with no_gc():
            raise RuntimeError('capture failed')
    assert gc.isenabled()
    gc.disable()
    try:
        with no_gc():
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()

"""wxengine.engine.NativeHandle, the one owner of a C-ABI handle on the Python side, against a fake destroy callable (no library, no GPU)."""
import ctypes as C
import gc

import pytest

from wxengine.engine import NativeHandle


class FakeLib:
    def __init__(self, fail=False):
        self.destroyed, self.fail = [], fail

    def create(self, out, value=0x1234):
        out._obj.value = value            # what a wx_*_create does through its out argument

    def destroy(self, h):
        self.destroyed.append(h.value)
        if self.fail:
            raise RuntimeError("destroy failed")


def made(lib, value=0x1234):
    h = NativeHandle(lib.destroy)
    lib.create(h.out, value)
    return h


def test_close_twice_destroys_once():
    lib = FakeLib()
    h = made(lib)
    assert C.c_void_p.from_param(h).value == 0x1234      # ctypes takes the object where a handle is expected
    h.close()
    h.close()
    assert lib.destroyed == [0x1234]
    assert not C.c_void_p.from_param(h).value            # a closed handle reads as null


def test_dropping_the_last_reference_destroys_once():
    lib = FakeLib()
    h = made(lib)
    del h
    gc.collect()
    assert lib.destroyed == [0x1234]


def test_dropping_after_close_destroys_nothing_more():
    lib = FakeLib()
    h = made(lib)
    h.close()
    del h
    gc.collect()
    assert lib.destroyed == [0x1234]


def test_a_destroy_that_raises_does_not_leave_del():
    lib = FakeLib(fail=True)
    h = made(lib)
    with pytest.raises(RuntimeError, match="destroy failed"):
        h.close()                                        # close() itself reports the failure ...
    h = made(lib, 0x5678)
    h.__del__()                                          # ... __del__ swallows it
    del h
    gc.collect()
    assert lib.destroyed == [0x1234, 0x5678]             # and the handle was given up either way: no second attempt


def test_a_null_handle_is_never_destroyed():
    lib = FakeLib()
    h = NativeHandle(lib.destroy)                        # the create call failed or never ran
    h.close()
    del h
    made(lib, 0).close()                                 # a create that returned null
    gc.collect()
    assert lib.destroyed == []

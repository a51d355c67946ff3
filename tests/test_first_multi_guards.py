"""CPU: mh_search_first_multi refuses bad arguments before any device is touched (these run on a
machine without a GPU), and search_first_multi passes its arguments through."""
import ctypes

import pytest

import minehip
from minehip import _lib

U64 = (1 << 64) - 1


def call(devs, msg, lower, upper, target, chunk, flags, out=True, ndev=None):
    arr = (ctypes.c_int * max(1, len(devs)))(*devs)
    f = _lib.mh_first()
    rc = minehip.lib.mh_search_first_multi(arr, len(devs) if ndev is None else ndev, msg, len(msg or b""), lower, upper,
                                           target, chunk, flags, ctypes.byref(f) if out else None)
    return rc, minehip.lib.mh_last_error().decode()


def test_guards_come_before_any_device():
    assert call([0], b"x", 0, 9, 5, 0, 2) == (minehip.MH_EINVAL, "unknown flag bit")
    assert call([0], b"x", 0, 9, 5, 0, 0x80000001)[0] == minehip.MH_EINVAL
    assert call([], b"x", 0, 9, 5, 0, 0)[0] == minehip.MH_EINVAL
    assert call([0], b"x", 0, 9, 5, 0, 0, ndev=-1)[0] == minehip.MH_EINVAL
    rc, what = call([0] * (_lib.MH_MAX_WORKERS + 1), b"x", 0, 9, 5, 0, 0)
    assert rc == minehip.MH_EINVAL and "MH_MAX_WORKERS" in what
    assert call([0], b"x", 0, 9, 5, 0, 0, out=False)[0] == minehip.MH_EINVAL
    assert call([0], b"x", 9, 8, 5, 0, 1) == (minehip.MH_ERANGE, "lower > upper")
    assert call([0] * _lib.MH_MAX_WORKERS, b"x", U64, 0, 5, 1, 0)[0] == minehip.MH_ERANGE
    # the flag is checked first, the range last
    assert call([], b"x", 9, 8, 5, 0, 4, out=False) == (minehip.MH_EINVAL, "unknown flag bit")


def test_python_wrapper_raises_the_code():
    with pytest.raises(minehip.MinehipError) as e:
        minehip.search_first_multi("x", 9, 8, 5, devs=[0])
    assert e.value.code == minehip.MH_ERANGE
    with pytest.raises(minehip.MinehipError) as e:
        minehip.search_first_multi("x", 0, 8, 5, devs=[])
    assert e.value.code == minehip.MH_EINVAL
    if minehip.device_count() == 0:
        with pytest.raises(minehip.MinehipError) as e:
            minehip.search_first_multi("x", 0, 8, 5, devs=[0], stop_running=True)
        assert e.value.code == minehip.MH_ENODEV

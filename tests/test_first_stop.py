"""mh_search_first_ex on the CPU: the symbol, its flag and argument handling, and the binding's
keyword.  No GPU compute is called here: every refusal below returns before a device is touched
(the checks run on a machine without one, and mh_last_error names the argument, never a device)."""
import ctypes

import minehip
from minehip import _lib

U64 = (1 << 64) - 1


def test_symbol_exported_and_bound():
    assert "mh_search_first_ex" in _lib.EXPORTS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "mh_search_first_ex")
    for name in ("mh_first_stop_co_begin", "mh_first_stop_co_end"):
        assert hasattr(raw, name), name
    fn = minehip.lib.mh_search_first_ex
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 8
    assert fn.argtypes[5] is ctypes.c_uint64 and fn.argtypes[6] is ctypes.c_uint32
    assert fn.argtypes[7]._type_ is _lib.mh_first
    assert minehip.MH_FIRST_STOP_RUNNING == _lib.MH_FIRST_STOP_RUNNING == 1
    assert ctypes.sizeof(_lib.mh_first) == 32 and minehip.lib.mh_abi_version() == 5   # additive
    header = open(_header()).read()
    assert "#define MH_FIRST_STOP_RUNNING 1u" in header and "int mh_search_first_ex(int dev," in header


def _header():
    import os
    from conftest import ROOT
    return os.path.join(ROOT, "include", "minehip.h")


def test_argument_errors_come_before_any_device():
    out = _lib.mh_first()
    f = minehip.lib.mh_search_first_ex
    err = minehip.lib.mh_last_error
    for flags in (0, minehip.MH_FIRST_STOP_RUNNING):
        assert f(0, b"x", 1, 5, 4, 7, flags, ctypes.byref(out)) == minehip.MH_ERANGE
        assert b"lower > upper" in err()
        assert f(0, b"x", 1, 0, 4, 7, flags, None) == minehip.MH_EINVAL
        assert b"NULL" in err()
        assert f(0, b"x", 1, 5, 4, 7, flags, None) == minehip.MH_EINVAL      # out == NULL first, as mh_search_first
        assert f(0, None, 3, 0, 4, 7, flags, ctypes.byref(out)) == minehip.MH_EINVAL
        big = b"y" * ((1 << 20) + 1)
        assert f(0, big, len(big), 0, 4, 7, flags, ctypes.byref(out)) == minehip.MH_ETOOLONG
    # an unknown flag bit, alone or beside the known one, on an otherwise valid call and on a device
    # index no machine has: refused for the flag, so before the device was looked at
    for flags in (2, 3, 1 << 31, 0xFFFFFFFF):
        for dev in (0, 10 ** 6):
            assert f(dev, b"x", 1, 0, 4, 7, flags, ctypes.byref(out)) == minehip.MH_EINVAL, flags
            assert b"flag" in err(), err()
    # ... and it wins over every other refusal
    assert f(0, b"x", 1, 5, 4, 7, 2, None) == minehip.MH_EINVAL and b"flag" in err()


def test_python_keyword_reaches_the_flag(monkeypatch):
    calls = []

    class Lib:
        def mh_search_first(self, *a):
            calls.append(("first", a))
            return minehip.MH_OK

        def mh_search_first_ex(self, *a):
            calls.append(("ex", a))
            return minehip.MH_OK

    monkeypatch.setattr(minehip, "lib", Lib())
    assert minehip.search_first("m", 1, 2, 3) == (False, 0, 0, 0)
    assert minehip.search_first("m", 1, 2, 3, stop_running=False) == (False, 0, 0, 0)
    assert minehip.search_first("m", 1, 2, 3, dev=4, stop_running=True) == (False, 0, 0, 0)
    assert [c[0] for c in calls] == ["first", "first", "ex"]
    assert all(len(c[1]) == 7 for c in calls[:2])                     # flags 0 stays mh_search_first itself
    dev, m, n, lo, hi, T, flags, _ = calls[2][1]
    assert (dev, m, n, lo, hi, T, flags) == (4, b"m", 1, 1, 2, 3, minehip.MH_FIRST_STOP_RUNNING)


def test_dev_build_refuses_the_hash_and_code_object_hooks():
    """As mh_search_first: stop_scan has no variants of the dev build's hash and code-object hooks,
    so with one set the call fails with MH_EINVAL before it touches a device."""
    from conftest import run_dev
    r = run_dev("""
import os, minehip
assert minehip.LIB_PATH.endswith("build/dev/libminehip.so"), minehip.LIB_PATH
for k, v in (("MINEHIP_DEV_HASH_KEEP", "2,0"), ("MINEHIP_DEV_HASH_XOR", "1f"),
             ("MINEHIP_DEV_CODE_OBJECT", "build/fast_search_keep.hsaco")):
    os.environ[k] = v
    try:
        minehip.search_first(b"cmu440", 0, 1000, 5, stop_running=True)
        raise SystemExit("searched with " + k)
    except minehip.MinehipError as e:
        assert e.code == minehip.MH_EINVAL and k in str(e), e
    del os.environ[k]
print("refused")
""", timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "refused", r.stderr[-2000:] + r.stdout[-500:]


def test_keyword_errors_are_search_firsts():
    for kw in (False, True):
        try:
            minehip.search_first("x", 9, 3, 1, stop_running=kw)
            raise AssertionError("searched lower > upper")
        except minehip.MinehipError as e:
            assert e.code == minehip.MH_ERANGE
    if minehip.device_count() == 0:               # no CPU fallback here either
        try:
            minehip.search_first("cmu440", 0, 10, U64, stop_running=True)
            raise AssertionError("searched without a device")
        except minehip.MinehipError as e:
            assert e.code == minehip.MH_ENODEV

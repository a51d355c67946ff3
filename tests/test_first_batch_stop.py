"""mh_search_first_batch_stop on the CPU: the ABI surface, the argument handling up to the device
call and the binding.  No GPU compute is called here.

The call is mh_search_first_batch_ex(MH_BATCH_FUSE_FAST) whose fast launches are batch_stop<J, MODE>'s
(include/minehip.h): an entry point of its own, since the flag bits of
mh_search_first_batch_ex other than MH_BATCH_FUSE_FAST stay MH_EINVAL (tests/test_first_batch_fast.py)."""
import ctypes

import pytest

import minehip
from minehip import _lib

U64 = (1 << 64) - 1


def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert "mh_search_first_batch_stop" in _lib.EXPORTS and hasattr(raw, "mh_search_first_batch_stop")
    for name in ("mh_batch_first_stop_co_begin", "mh_batch_first_stop_co_end"):
        assert hasattr(raw, name), name
    fn = minehip.lib.mh_search_first_batch_stop
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 4 and fn.argtypes[0] is ctypes.c_int
    assert fn.argtypes[1]._type_ is _lib.mh_first_request and fn.argtypes[3]._type_ is _lib.mh_first_result
    assert ctypes.sizeof(_lib.mh_first_request) == 40 and ctypes.sizeof(_lib.mh_first_result) == 32
    assert minehip.lib.mh_abi_version() == 5      # additive: no existing struct changed
    from minehip import codeobj
    assert callable(codeobj.batch_first_stop_code_object) and callable(codeobj.batch_first_stop_kernel_resources)
    assert codeobj.batch_first_stop_code_object()[:4] == b"\x7fELF"


def _reqs(*quads):
    arr = (_lib.mh_first_request * len(quads))()
    keep = []
    for i, (m, lo, hi, T) in enumerate(quads):
        keep.append(m)
        arr[i].msg, arr[i].len, arr[i].lower, arr[i].upper, arr[i].target = m, (len(m) if m is not None else 3), lo, hi, T
    return arr, keep


def test_arguments_without_a_device():
    L = minehip.lib
    arr, _ = _reqs((b"cmu440", 0, 99, 7))
    out = (_lib.mh_first_result * 1)()
    assert L.mh_search_first_batch_stop(0, None, 0, None) == minehip.MH_OK       # n = 0: no device touched
    assert L.mh_search_first_batch_stop(0, arr, 0, out) == minehip.MH_OK
    assert L.mh_search_first_batch_stop(0, None, 1, out) == minehip.MH_EINVAL
    assert b"NULL" in L.mh_last_error()
    assert L.mh_search_first_batch_stop(0, arr, 1, None) == minehip.MH_EINVAL
    # every request refused on its own: each has its status, the call is MH_OK, no device needed
    big = b"y" * ((1 << 20) + 1)
    bad, _ = _reqs((b"x", 9, 3, 5), (None, 0, 9, 5), (big, 0, 4, 5), (b"y", U64, 0, U64))
    res = (_lib.mh_first_result * 4)()
    assert L.mh_search_first_batch_stop(0, bad, 4, res) == minehip.MH_OK
    assert [o.status for o in res] == [minehip.MH_ERANGE, minehip.MH_EINVAL, minehip.MH_ETOOLONG, minehip.MH_ERANGE]


def test_python_call():
    with pytest.raises(ValueError, match="fuse_fast"):
        minehip.search_first_batch([("cmu440", 0, 99, 7)], stop_running=True)
    with pytest.raises(ValueError, match="fuse_fast"):
        minehip.search_first_batch([], stop_running=True)                        # before anything else
    assert minehip.search_first_batch([], fuse_fast=True, stop_running=True) == []
    res = minehip.search_first_batch([("x", 9, 3, 1), ("y", 2, 1, 1)], errors="return", fuse_fast=True, stop_running=True)
    assert [(r.code, r.index) for r in res] == [(minehip.MH_ERANGE, 0), (minehip.MH_ERANGE, 1)]
    with pytest.raises(minehip.MinehipError) as e:
        minehip.search_first_batch([("x", 9, 3, 1)], fuse_fast=True, stop_running=True)
    assert e.value.code == minehip.MH_ERANGE and e.value.index == 0
    if minehip.device_count() == 0:                # no CPU fallback: fused and fallback requests alike
        for r in (("cmu440", 0, 99, U64), ("cmu440", 0, 3 * 10 ** 6, U64), ("cmu440", 0, 2 * 10 ** 9, U64)):
            with pytest.raises(minehip.MinehipError) as e:
                minehip.search_first_batch([r], errors="return", fuse_fast=True, stop_running=True)
            assert e.value.code == minehip.MH_ENODEV


def test_dev_build_refuses_the_hash_hooks():
    """As the other first-hit calls: with a hash or code-object hook set the dev build fails with
    MH_EINVAL before it touches a device, instead of silently ignoring the hook."""
    from conftest import run_dev
    r = run_dev("""
import os, minehip
assert minehip.LIB_PATH.endswith("build/dev/libminehip.so"), minehip.LIB_PATH
for k, v in (("MINEHIP_DEV_HASH_KEEP", "2,0"), ("MINEHIP_DEV_HASH_XOR", "1f"),
             ("MINEHIP_DEV_CODE_OBJECT", "build/fast_search_keep.hsaco")):
    os.environ[k] = v
    for req in ((b"cmu440", 0, 1000, 5), (b"cmu440", 0, 3 * 10 ** 6, 5)):
        try:
            minehip.search_first_batch([req], fuse_fast=True, stop_running=True)
            raise SystemExit("searched with " + k)
        except minehip.MinehipError as e:
            assert e.code == minehip.MH_EINVAL and k in str(e) and "mh_search_first_batch_stop" in str(e), e
    del os.environ[k]
print("ok")
""")
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr[-2000:])

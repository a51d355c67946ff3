"""minehip -- MI355X (gfx950) SHA-256 nonce search for the CMU 15-440 miner.

Python face of libminehip.so, named after the reference's own API so parity
tests read like the reference (line numbers into the reference repo):

  Hash(msg, nonce)           bitcoin/hash.go:13-17, computed on the GPU
  hash_batch(msg, nonces)    the same for many nonces
  search(msg, lower, upper)  the miner scan (stub miner.go:33)
  search_multi(...)          the scan sharded over several devices
  search_batch(requests)     many small scans fused into one GPU pass (fuse_fast=True: the
                             fast pieces of larger ones too)
  search_first(msg, lower, upper, target)
                             the smallest nonce whose hash is <= target
  search_first_multi(msg, lower, upper, target, devs)
                             the same over several devices, chunk by chunk in ascending order
  search_hits(msg, lower, upper, target, cap=4096)
                             every nonce whose hash is <= target, and how many there are
  search_first_hits(msg, lower, upper, target, k)
                             the k smallest nonces whose hash is <= target, without the full scan
  search_first_batch(requests)
                             many small first-hit searches fused into one GPU pass
                             (fuse_fast=True: the fast pieces of larger ones too)
  search_hits_batch(requests, cap=4096)
                             every hit of many small requests in one GPU pass
                             (fuse_fast=True: the fast pieces of larger ones too)
  search_first_hits_batch(requests)
                             the k smallest hits of many requests in one GPU pass
                             (fuse_fast=True: the fast pieces of larger ones too)
  miner_handle_batch(...)    miner_handle for the payloads a miner holds at once (fuse_fast=True:
                             the fast pieces of the larger Requests fuse too)
  Scheduler / Server         the server's chunk scheduler and message loop (depth=: how many
                             chunks a miner may hold at once, so small Requests reach it as a batch)
  Message / NewRequest / NewResult / NewJoin / marshal / unmarshal
                             bitcoin/message.go:7-62 with Go encoding/json bytes
  NewTargetRequest(data, lower, upper, target)
                             a Request with the optional Target key: the first-hit question through the
                             server, its miners and the client (Scheduler.submit_first)
  miner_handle(request)      one miner step: Request payload -> Result payload

All compute goes through the C-ABI; there is no host fallback.
"""
import ctypes

import numpy as np

from ._lib import lib, mh_piece, mh_message, mh_kernel_stat, mh_span, OPS_PER_BLOCK, EXPORTS, LIB_PATH  # noqa: F401
from ._lib import MH_OK, MH_EINVAL, MH_ERANGE, MH_ETOOLONG, MH_ENODEV, MH_EHIP  # noqa: F401
from ._lib import MH_ENOTREQ, MH_EINTERNAL, MH_EREJECTED  # noqa: F401
from ._lib import mh_request, mh_result, mh_batch_item, mh_first  # noqa: F401
from ._lib import mh_batch_piece, MH_BATCH_FUSE_FAST, MH_BATCH_FAST_MAX_NONCES  # noqa: F401
from ._lib import mh_first_request, mh_first_result, MH_FIRST_STOP_RUNNING  # noqa: F401
from ._lib import mh_hit, mh_hits, MH_HITS_MAX_CAP, mh_first_hits  # noqa: F401
from ._lib import mh_hits_request, mh_hits_result, mh_hits_region  # noqa: F401
from ._lib import mh_first_hits_request, mh_first_hits_result  # noqa: F401
from ._lib import mh_message_ex, mh_sched_first_stats  # noqa: F401

U64_MAX = (1 << 64) - 1


class MinehipError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"minehip error {code}: {what}")
        self.code = code


def _check(rc):
    if rc != MH_OK:
        raise MinehipError(rc, lib.mh_last_error().decode("utf-8", "replace"))


def _b(msg):
    return msg.encode("utf-8") if isinstance(msg, str) else bytes(msg)


def device_count():
    return lib.mh_device_count()


def search(msg, lower, upper, dev=0):
    """(hash, nonce) = lexicographic min of (Hash(msg, n), n), n in [lower, upper]."""
    m = _b(msg)
    h = ctypes.c_uint64()
    n = ctypes.c_uint64()
    _check(lib.mh_search(dev, m, len(m), lower, upper, ctypes.byref(h), ctypes.byref(n)))
    return h.value, n.value


def search_first(msg, lower, upper, target, dev=0, stop_running=False):
    """(found, hash, nonce, scanned): the smallest nonce n of [lower, upper] with Hash(msg, n) <=
    target and its hash (found True), or search()'s (hash, nonce) when none qualifies (found
    False); scanned is how many nonces of the range were hashed (mh_search_first).
    stop_running: mh_search_first_ex with MH_FIRST_STOP_RUNNING -- the same answer, from kernels that
    also leave a chunk already running once it lies wholly above a published hit."""
    m = _b(msg)
    out = mh_first()
    if stop_running:
        _check(lib.mh_search_first_ex(dev, m, len(m), lower, upper, target, MH_FIRST_STOP_RUNNING, ctypes.byref(out)))
        return bool(out.found), out.hash, out.nonce, out.scanned
    _check(lib.mh_search_first(dev, m, len(m), lower, upper, target, ctypes.byref(out)))
    return bool(out.found), out.hash, out.nonce, out.scanned


def search_hits(msg, lower, upper, target, cap=4096, dev=0):
    """(count, [(nonce, hash), ...], (min_hash, min_nonce)): how many nonces n of [lower, upper] have
    Hash(msg, n) <= target, the min(count, cap) smallest of them in increasing order with their
    hashes, and search()'s result for the range (mh_search_hits).  cap = 0 only counts."""
    m = _b(msg)
    if cap < 0 or cap > MH_HITS_MAX_CAP:
        raise MinehipError(MH_EINVAL, f"cap must be 0..{MH_HITS_MAX_CAP}")
    buf = (mh_hit * cap)() if cap else None
    out = mh_hits()
    _check(lib.mh_search_hits(dev, m, len(m), lower, upper, target, buf, cap, ctypes.byref(out)))
    return out.count, [(buf[i].nonce, buf[i].hash) for i in range(out.stored)], (out.hash, out.nonce)


def search_first_hits(msg, lower, upper, target, k, dev=0):
    """([(nonce, hash), ...], (hash, nonce), scanned): the min(k, count) smallest nonces n of [lower,
    upper] with Hash(msg, n) <= target in increasing order with their hashes -- search_hits' first
    entries -- from kernels that stop once k of them are known (mh_search_first_hits); (hash, nonce)
    is search()'s result for the range when fewer than k qualify, else the minimum of the k entries;
    scanned is how many nonces of the range were hashed."""
    m = _b(msg)
    if k < 1 or k > MH_HITS_MAX_CAP:
        raise MinehipError(MH_EINVAL, f"k must be 1..{MH_HITS_MAX_CAP}")
    buf = (mh_hit * k)()
    out = mh_first_hits()
    _check(lib.mh_search_first_hits(dev, m, len(m), lower, upper, target, buf, k, ctypes.byref(out)))
    return [(buf[i].nonce, buf[i].hash) for i in range(out.stored)], (out.hash, out.nonce), out.scanned


def search_multi(msg, lower, upper, devs=None, chunk=0):
    m = _b(msg)
    if devs is None:
        devs = list(range(device_count()))
    arr = (ctypes.c_int * len(devs))(*devs)
    h = ctypes.c_uint64()
    n = ctypes.c_uint64()
    _check(lib.mh_search_multi(arr, len(devs), m, len(m), lower, upper, chunk, ctypes.byref(h),
                               ctypes.byref(n)))
    return h.value, n.value


def search_first_multi(msg, lower, upper, target, devs=None, chunk=0, stop_running=False):
    """search_first over the listed devices (default: every device), chunk by chunk through a target
    job of the scheduler: (found, hash, nonce, scanned) with found, hash and nonce exactly
    search_first's; scanned sums the chunks that completed, those above the hit included
    (mh_search_first_multi).  chunk = 0: 2^30 nonces, the scheduler's default, not tuned."""
    m = _b(msg)
    if devs is None:
        devs = list(range(device_count()))
    arr = (ctypes.c_int * max(1, len(devs)))(*devs)
    out = mh_first()
    _check(lib.mh_search_first_multi(arr, len(devs), m, len(m), lower, upper, target, chunk,
                                     MH_FIRST_STOP_RUNNING if stop_running else 0, ctypes.byref(out)))
    return bool(out.found), out.hash, out.nonce, out.scanned


def _requests(requests):
    """(msg, lower, upper) triples -> (mh_request array, the message bytes it points into)."""
    keep = []
    arr = (mh_request * max(1, len(requests)))()
    for i, r in enumerate(requests):
        try:
            msg, lower, upper = r
        except (TypeError, ValueError):
            raise ValueError(f"request {i}: expected (msg, lower, upper), got {r!r}") from None
        for name, v in (("lower", lower), ("upper", upper)):
            if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= U64_MAX:
                raise ValueError(f"request {i}: {name} = {v!r} is not a uint64")
        m = _b(msg)
        keep.append(m)
        arr[i].msg, arr[i].len, arr[i].lower, arr[i].upper = m, len(m), lower, upper
    return arr, keep


_REQUEST_ERRORS = {MH_EINVAL: "msg is NULL", MH_ERANGE: "lower > upper",
                   MH_ETOOLONG: "message longer than MH_MAX_MSG_LEN"}


def search_batch(requests, dev=0, errors="raise", fuse_fast=False):
    """[(hash, nonce), ...] of many (msg, lower, upper) requests, each exactly what search() gives,
    with the small ones fused into one GPU pass (mh_search_batch).  fuse_fast=True also fuses the
    fast pieces of the larger requests, up to MH_BATCH_FAST_MAX_NONCES nonces each
    (mh_search_batch_ex with MH_BATCH_FUSE_FAST).  A request that fails alone
    (lower > upper, message too long) raises MinehipError naming its index, or with
    errors="return" leaves that MinehipError in its place in the list."""
    if errors not in ("raise", "return"):
        raise ValueError(f"errors = {errors!r}: expected 'raise' or 'return'")
    requests = list(requests)
    arr, keep = _requests(requests)
    out = (mh_result * max(1, len(requests)))()
    if fuse_fast:
        _check(lib.mh_search_batch_ex(dev, arr, len(requests), MH_BATCH_FUSE_FAST, out))
    else:
        _check(lib.mh_search_batch(dev, arr, len(requests), out))
    res = []
    for i in range(len(requests)):
        if out[i].status == MH_OK:
            res.append((out[i].hash, out[i].nonce))
            continue
        e = MinehipError(out[i].status, f"request {i}: {_REQUEST_ERRORS.get(out[i].status, 'failed')}")
        e.index = i
        if errors == "raise":
            raise e
        res.append(e)
    return res


def batch_plan(requests, cap=1 << 16):
    """Host-only: how search_batch would run the requests -- one dict per entry of a fused request
    (kind 0: its pass, first partial slot and tiles) and one per fallback request (kind 1)."""
    requests = list(requests)
    arr, keep = _requests(requests)
    buf = (mh_batch_item * cap)()
    k = lib.mh_batch_plan(arr, len(requests), buf, cap)
    if k < 0:
        _check(k)
    if k > cap:
        raise ValueError("batch plan longer than cap")
    return [{f: getattr(buf[i], f) for f, _ in mh_batch_item._fields_} for i in range(k)]


def batch_plan_ex(requests, fuse_fast=True, cap=1 << 16, flags=None):
    """Host-only: how search_batch(fuse_fast=...) would run the requests -- one dict per piece of a
    fused request (kind 0: a generic entry, its pass, first partial slot and tiles; kind 2: a fast
    piece, its pass, first slot, chunks, layout word / mode / lo_digits and launch) and one per
    fallback request (kind 1) (mh_batch_plan_ex; `flags` overrides the flag word)."""
    requests = list(requests)
    arr, keep = _requests(requests)
    buf = (mh_batch_piece * cap)()
    k = lib.mh_batch_plan_ex(arr, len(requests), (MH_BATCH_FUSE_FAST if fuse_fast else 0) if flags is None else flags,
                             buf, cap)
    if k < 0:
        _check(k)
    if k > cap:
        raise ValueError("batch plan longer than cap")
    return [{f: getattr(buf[i], f) for f, _ in mh_batch_piece._fields_} for i in range(k)]


def search_first_batch(requests, dev=0, errors="raise", fuse_fast=False, stop_running=False):
    """[(found, hash, nonce, scanned), ...] of many (msg, lower, upper, target) requests: found,
    hash and nonce exactly what search_first() gives for each, with the small ones fused into one
    GPU pass (mh_search_first_batch).  fuse_fast=True also fuses the fast pieces of the larger
    requests, up to MH_BATCH_FAST_MAX_NONCES nonces each (mh_search_first_batch_ex with
    MH_BATCH_FUSE_FAST).  stop_running=True (with fuse_fast=True: its plan is the fused one) gives
    the same answers from kernels that also leave a running chunk once it lies wholly above a hit
    of its request (mh_search_first_batch_stop).  Per-request failures as search_batch: raised with the
    request's index, or with errors="return" left in place in the list."""
    if errors not in ("raise", "return"):
        raise ValueError(f"errors = {errors!r}: expected 'raise' or 'return'")
    if stop_running and not fuse_fast:
        raise ValueError("stop_running=True requires fuse_fast=True: its plan is the fused one")
    requests = list(requests)
    keep = []
    arr = (mh_first_request * max(1, len(requests)))()
    for i, r in enumerate(requests):
        try:
            msg, lower, upper, target = r
        except (TypeError, ValueError):
            raise ValueError(f"request {i}: expected (msg, lower, upper, target), got {r!r}") from None
        for name, v in (("lower", lower), ("upper", upper), ("target", target)):
            if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= U64_MAX:
                raise ValueError(f"request {i}: {name} = {v!r} is not a uint64")
        m = _b(msg)
        keep.append(m)
        arr[i].msg, arr[i].len, arr[i].lower, arr[i].upper, arr[i].target = m, len(m), lower, upper, target
    out = (mh_first_result * max(1, len(requests)))()
    if stop_running:
        _check(lib.mh_search_first_batch_stop(dev, arr, len(requests), out))
    elif fuse_fast:
        _check(lib.mh_search_first_batch_ex(dev, arr, len(requests), MH_BATCH_FUSE_FAST, out))
    else:
        _check(lib.mh_search_first_batch(dev, arr, len(requests), out))
    res = []
    for i in range(len(requests)):
        if out[i].status == MH_OK:
            res.append((bool(out[i].found), out[i].hash, out[i].nonce, out[i].scanned))
            continue
        e = MinehipError(out[i].status, f"request {i}: {_REQUEST_ERRORS.get(out[i].status, 'failed')}")
        e.index = i
        if errors == "raise":
            raise e
        res.append(e)
    return res


def first_batch_order(requests, pass_=0, cap=1 << 18, fuse_fast=False, launch=-1, flags=None):
    """Host-only: the dispatch order of pass `pass_` of search_first_batch over (msg, lower, upper)
    requests (a target, if given, is ignored): entry b is the partial slot of the tile that
    workgroup b runs (mh_first_batch_order).  With fuse_fast=True the pass is one of
    search_first_batch(fuse_fast=True): launch=-1 is its generic launch, launch >= 0 that
    batch_first launch, entry b the partial slot of the chunk that workgroup b runs
    (mh_first_batch_order_ex; `flags` overrides the flag word)."""
    requests = [tuple(r)[:3] for r in requests]
    arr, keep = _requests(requests)
    buf = (ctypes.c_uint32 * cap)()
    if fuse_fast or launch != -1 or flags is not None:
        k = lib.mh_first_batch_order_ex(arr, len(requests), (MH_BATCH_FUSE_FAST if fuse_fast else 0) if flags is None
                                        else flags, pass_, launch, buf, cap)
    else:
        k = lib.mh_first_batch_order(arr, len(requests), pass_, buf, cap)
    if k < 0:
        _check(k)
    if k > cap:
        raise ValueError("order longer than cap")
    return list(buf[:k])


def _hits_requests(requests, cap):
    """(msg, lower, upper, target[, cap]) tuples -> (mh_hits_request array, the message bytes it
    points into, the offsets of the requests' entries, their sum)."""
    if not isinstance(cap, int) or isinstance(cap, bool) or not 0 <= cap <= U64_MAX:
        raise ValueError(f"cap = {cap!r} is not a uint64")
    keep, offsets, total = [], [], 0
    arr = (mh_hits_request * max(1, len(requests)))()
    for i, r in enumerate(requests):
        try:
            msg, lower, upper, target, c = r if len(r) == 5 else tuple(r) + (cap,)
        except (TypeError, ValueError):
            raise ValueError(f"request {i}: expected (msg, lower, upper, target[, cap]), got {r!r}") from None
        for name, v in (("lower", lower), ("upper", upper), ("target", target), ("cap", c)):
            if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= U64_MAX:
                raise ValueError(f"request {i}: {name} = {v!r} is not a uint64")
        m = _b(msg)
        keep.append(m)
        arr[i].msg, arr[i].len, arr[i].lower, arr[i].upper, arr[i].target, arr[i].cap = m, len(m), lower, upper, target, c
        offsets.append(total)
        total += c if c <= MH_HITS_MAX_CAP else 0       # as the library counts them
    return arr, keep, offsets, total


def search_hits_batch(requests, cap=4096, dev=0, errors="raise", fuse_fast=False, flags=None):
    """[(count, [(nonce, hash), ...], (min_hash, min_nonce)), ...] of many (msg, lower, upper,
    target) or (msg, lower, upper, target, cap) requests, each exactly what search_hits() gives,
    with the small ones fused into one GPU pass (mh_search_hits_batch); `cap` is the cap of the
    requests that carry none.  fuse_fast=True also fuses the fast pieces of the larger requests,
    up to MH_BATCH_FAST_MAX_NONCES nonces each (mh_search_hits_batch_ex with MH_BATCH_FUSE_FAST;
    `flags` overrides the flag word).  Per-request failures as search_batch: raised with the
    request's index, or with errors="return" left in place in the list."""
    if errors not in ("raise", "return"):
        raise ValueError(f"errors = {errors!r}: expected 'raise' or 'return'")
    requests = list(requests)
    arr, keep, offsets, total = _hits_requests(requests, cap)
    # not a ctypes array: that would be zero-filled, all sum-of-caps entries of it, on every call
    buf = np.empty((max(1, total), 2), dtype=np.uint64)
    out = (mh_hits_result * max(1, len(requests)))()
    hits = buf.ctypes.data_as(ctypes.POINTER(mh_hit)) if total else None
    if fuse_fast or flags is not None:
        _check(lib.mh_search_hits_batch_ex(dev, arr, len(requests), MH_BATCH_FUSE_FAST if flags is None else flags,
                                           hits, total, out))
    else:
        _check(lib.mh_search_hits_batch(dev, arr, len(requests), hits, total, out))
    res = []
    for i in range(len(requests)):
        o = out[i]
        if o.status == MH_OK:
            assert o.offset == offsets[i]
            entries = [(n, h) for h, n in buf[o.offset:o.offset + o.stored].tolist()] if o.stored else []
            res.append((o.count, entries, (o.hash, o.nonce)))
            continue
        what = ("cap is larger than MH_HITS_MAX_CAP" if o.status == MH_EINVAL and arr[i].cap > MH_HITS_MAX_CAP
                else _REQUEST_ERRORS.get(o.status, "failed"))
        e = MinehipError(o.status, f"request {i}: {what}")
        e.index = i
        if errors == "raise":
            raise e
        res.append(e)
    return res


def hits_batch_regions(requests, cap=4096, fuse_fast=False, flags=None):
    """Host-only: how search_hits_batch would run the requests -- one dict per request: kind (0
    fused, 1 fallback), its pass, its window (how many drains precede it) and its region (offset,
    slots) of the device hit buffer (mh_hits_batch_regions).  fuse_fast=True: how
    search_hits_batch(fuse_fast=True) would, kind and pass following batch_plan_ex
    (mh_hits_batch_regions_ex; `flags` overrides the flag word)."""
    requests = list(requests)
    arr, keep, _, _ = _hits_requests(requests, cap)
    buf = (mh_hits_region * max(1, len(requests)))()
    if fuse_fast or flags is not None:
        k = lib.mh_hits_batch_regions_ex(arr, len(requests), MH_BATCH_FUSE_FAST if flags is None else flags, buf,
                                         len(requests))
    else:
        k = lib.mh_hits_batch_regions(arr, len(requests), buf, len(requests))
    if k < 0:
        _check(k)
    return [{f: getattr(buf[i], f) for f, _ in mh_hits_region._fields_ if f != "reserved"} for i in range(k)]


def _first_hits_requests(requests):
    """(msg, lower, upper, target, k) tuples -> (mh_first_hits_request array, the message bytes it
    points into, the offsets of the requests' entries, their sum)."""
    keep, offsets, total = [], [], 0
    arr = (mh_first_hits_request * max(1, len(requests)))()
    for i, r in enumerate(requests):
        try:
            msg, lower, upper, target, k = r
        except (TypeError, ValueError):
            raise ValueError(f"request {i}: expected (msg, lower, upper, target, k), got {r!r}") from None
        for name, v in (("lower", lower), ("upper", upper), ("target", target), ("k", k)):
            if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= U64_MAX:
                raise ValueError(f"request {i}: {name} = {v!r} is not a uint64")
        m = _b(msg)
        keep.append(m)
        arr[i].msg, arr[i].len, arr[i].lower, arr[i].upper, arr[i].target, arr[i].k = m, len(m), lower, upper, target, k
        offsets.append(total)
        total += k if k <= MH_HITS_MAX_CAP else 0       # as the library counts them
    return arr, keep, offsets, total


def search_first_hits_batch(requests, dev=0, errors="raise", fuse_fast=False, flags=None):
    """[([(nonce, hash), ...], (hash, nonce), scanned, path), ...] of many (msg, lower, upper, target,
    k) requests: entries and (hash, nonce) exactly what search_first_hits() gives for each, with the
    small ones fused into one GPU pass whose tiles stop at their request's own bound
    (mh_search_first_hits_batch).  fuse_fast=True also fuses the fast pieces of the larger requests,
    up to MH_BATCH_FAST_MAX_NONCES nonces each (MH_BATCH_FUSE_FAST; `flags` overrides the flag word).
    path: 0 answered from the fused pass, 1 fallback, 2 fused and then rebuilt through the
    search_first_hits path.  Per-request failures as search_batch: raised with the request's index,
    or with errors="return" left in place in the list."""
    if errors not in ("raise", "return"):
        raise ValueError(f"errors = {errors!r}: expected 'raise' or 'return'")
    requests = list(requests)
    arr, keep, offsets, total = _first_hits_requests(requests)
    buf = np.empty((max(1, total), 2), dtype=np.uint64)
    out = (mh_first_hits_result * max(1, len(requests)))()
    hits = buf.ctypes.data_as(ctypes.POINTER(mh_hit)) if total else None
    word = (MH_BATCH_FUSE_FAST if fuse_fast else 0) if flags is None else flags
    _check(lib.mh_search_first_hits_batch(dev, arr, len(requests), word, hits, total, out))
    res = []
    for i in range(len(requests)):
        o = out[i]
        if o.status == MH_OK:
            assert o.offset == offsets[i]
            entries = [(n, h) for h, n in buf[o.offset:o.offset + o.stored].tolist()] if o.stored else []
            res.append((entries, (o.hash, o.nonce), o.scanned, o.path))
            continue
        what = ("k is 0" if o.status == MH_EINVAL and arr[i].k == 0
                else "k is larger than MH_HITS_MAX_CAP" if o.status == MH_EINVAL and arr[i].k > MH_HITS_MAX_CAP
                else _REQUEST_ERRORS.get(o.status, "failed"))
        e = MinehipError(o.status, f"request {i}: {what}")
        e.index = i
        if errors == "raise":
            raise e
        res.append(e)
    return res


def first_hits_batch_regions(requests, fuse_fast=False, flags=None):
    """Host-only: how search_first_hits_batch would run the requests -- hits_batch_regions' dicts
    with the regions of that call: a request of k wants min(its nonce count, max(4 k, 256)) entries
    (mh_first_hits_batch_regions; kind and pass follow batch_plan_ex with the same flags)."""
    requests = list(requests)
    arr, keep, _, _ = _first_hits_requests(requests)
    buf = (mh_hits_region * max(1, len(requests)))()
    word = (MH_BATCH_FUSE_FAST if fuse_fast else 0) if flags is None else flags
    k = lib.mh_first_hits_batch_regions(arr, len(requests), word, buf, len(requests))
    if k < 0:
        _check(k)
    return [{f: getattr(buf[i], f) for f, _ in mh_hits_region._fields_ if f != "reserved"} for i in range(k)]


def hash_batch(msg, nonces, dev=0):
    m = _b(msg)
    a = np.ascontiguousarray(nonces, dtype=np.uint64)
    out = np.empty_like(a)
    p = ctypes.POINTER(ctypes.c_uint64)
    _check(lib.mh_hash_batch(dev, m, len(m), a.ctypes.data_as(p), a.size, out.ctypes.data_as(p)))
    return out


def Hash(msg, nonce, dev=0):  # noqa: N802  (reference name, bitcoin/hash.go:13)
    return int(hash_batch(msg, [nonce], dev)[0])


def plan(msg, lower, upper, cap=1 << 16):
    """Host-only: the launch plan of a search (list of dicts)."""
    m = _b(msg)
    buf = (mh_piece * cap)()
    k = lib.mh_plan(m, len(m), lower, upper, buf, cap)
    if k < 0:
        _check(k)
    if k > cap:
        raise ValueError("plan longer than cap")
    return [{f: getattr(buf[i], f) for f, _ in mh_piece._fields_} for i in range(k)]


def multi_plan(msg, lower, upper, ndev, weights=None, cap=1 << 12):
    """Host-only: how search_multi (chunk = 0) splits [lower, upper] over ndev workers with rates in
    proportion to `weights` (None = equal): head shards, then tail chunks (list of dicts)."""
    if weights is not None and len(weights) != ndev:
        raise ValueError(f"multi_plan: {len(weights)} weights for {ndev} workers")
    m = _b(msg)
    buf = (mh_span * cap)()
    w = None if weights is None else (ctypes.c_double * ndev)(*weights)
    k = lib.mh_multi_plan(m, len(m), lower, upper, w, ndev, buf, cap)
    if k < 0:
        _check(k)
    if k > cap:
        raise ValueError("split longer than cap")
    return [{f: getattr(buf[i], f) for f, _ in mh_span._fields_} for i in range(k)]


def multi_rates(devs):
    """The per-process device rates search_multi sizes its shards by (cost units per ns, 0 = none)."""
    arr = (ctypes.c_int * len(devs))(*devs)
    out = (ctypes.c_double * len(devs))()
    _check(lib.mh_multi_rates(arr, len(devs), out))
    return list(out)


def profile_enable(dev=0, on=True):
    _check(lib.mh_profile_enable(dev, 1 if on else 0))


def profile_read(dev=0):
    out = (ctypes.c_uint64 * 8)()
    _check(lib.mh_profile_read(dev, out, 8))
    keys = ("fast_launches", "fast_nonces", "fast_ns", "fast_ops", "generic_nonces", "generic_ns", "fast_slots")
    return {k: int(out[i]) for i, k in enumerate(keys)}


def profile_kernels(dev=0):
    """Per fast_search<J, MODE> variant and lane length L (lo_digits): launches, nonces, ns, ops
    (largest ns first).  `name` is the kernel's name in a rocprofv3 trace (the same for every L)."""
    cap = 256
    buf = (mh_kernel_stat * cap)()
    n = lib.mh_profile_kernels(dev, buf, cap)
    if n < 0:
        _check(n)
    out = [{f: int(getattr(buf[i], f)) for f, _ in mh_kernel_stat._fields_ if f != "reserved"}
           for i in range(min(n, cap))]
    for k in out:
        k["name"] = f"mh::fast_search<{k['word']}, {k['mode']}>"
    return sorted(out, key=lambda k: -k["ns"])


# ---- bitcoin/message.go mirror --------------------------------------------
Join, Request, Result = 0, 1, 2  # MsgType iota, message.go:9-13


class Message:
    """bitcoin.Message (message.go:18-23), plus the optional Target of a Request (None: absent;
    include/minehip.h mh_message_ex)."""

    __slots__ = ("Type", "Data", "Lower", "Upper", "Hash", "Nonce", "Target")

    def __init__(self, Type=0, Data=b"", Lower=0, Upper=0, Hash=0, Nonce=0, Target=None):  # noqa: N803
        self.Type, self.Data = Type, _b(Data)
        self.Lower, self.Upper, self.Hash, self.Nonce = Lower, Upper, Hash, Nonce
        self.Target = Target

    def __eq__(self, o):
        return isinstance(o, Message) and all(getattr(self, k) == getattr(o, k) for k in self.__slots__)

    def __repr__(self):
        return self.String()

    def String(self):  # noqa: N802  (message.go:51-62)
        if self.Type == Request:
            return "[Request %s %d %d]" % (self.Data.decode("utf-8", "replace"), self.Lower, self.Upper)
        if self.Type == Result:
            return "[Result %d %d]" % (self.Hash, self.Nonce)
        if self.Type == Join:
            return "[Join]"
        return ""


def NewRequest(data, lower, upper):  # noqa: N802  (message.go:27-34)
    return Message(Request, data, lower, upper)


def NewTargetRequest(data, lower, upper, target):  # noqa: N802
    """A Request asking for the smallest nonce of [lower, upper] whose hash is <= target."""
    return Message(Request, data, lower, upper, Target=target)


def NewResult(hash_, nonce):  # noqa: N802  (message.go:38-44)
    return Message(Result, b"", 0, 0, hash_, nonce)


def NewJoin():  # noqa: N802  (message.go:47-49)
    return Message(Join)


def marshal(m):
    """json.Marshal(m) as Go produces it."""
    need = ctypes.c_size_t()
    if m.Target is not None:  # the six reference keys, then "Target" (mh_msg_encode_ex)
        args = (m.Type, m.Data, len(m.Data), m.Lower, m.Upper, m.Hash, m.Nonce, 1, m.Target)
        lib.mh_msg_encode_ex(*args, None, 0, ctypes.byref(need))
        buf = ctypes.create_string_buffer(need.value)
        _check(lib.mh_msg_encode_ex(*args, buf, need.value, ctypes.byref(need)))
        return buf.raw[:need.value]
    lib.mh_msg_encode(m.Type, m.Data, len(m.Data), m.Lower, m.Upper, m.Hash, m.Nonce, None, 0,
                      ctypes.byref(need))
    buf = ctypes.create_string_buffer(need.value)
    _check(lib.mh_msg_encode(m.Type, m.Data, len(m.Data), m.Lower, m.Upper, m.Hash, m.Nonce, buf,
                             need.value, ctypes.byref(need)))
    return buf.raw[:need.value]


def unmarshal(payload):
    """json.Unmarshal(payload, &m) with Go's decoding rules."""
    p = _b(payload)
    mm = mh_message_ex()
    cap = len(p) + 16
    data = ctypes.create_string_buffer(cap)
    _check(lib.mh_msg_decode_ex(p, len(p), ctypes.byref(mm), data, cap))
    return Message(mm.type, data.raw[:mm.data_len], mm.lower, mm.upper, mm.hash, mm.nonce,
                   mm.target if mm.has_target else None)


def miner_handle(request_payload, devs=(0,)):
    """One GPU-miner step: Request payload -> Result payload (both Go JSON)."""
    p = _b(request_payload)
    arr = (ctypes.c_int * len(devs))(*devs)
    need = ctypes.c_size_t()
    buf = ctypes.create_string_buffer(256)
    _check(lib.mh_miner_handle(arr, len(devs), p, len(p), buf, 256, ctypes.byref(need)))
    return buf.raw[:need.value]


def miner_handle_batch(payloads, devs=(0,), errors="return", fuse_fast=False):
    """miner_handle for the payloads a miner holds at once (mh_miner_handle_batch): the valid
    small Requests run as one fused batch on devs[0]; fuse_fast=True also fuses the fast pieces
    of the larger ones, up to MH_BATCH_FAST_MAX_NONCES nonces each (mh_miner_handle_batch_ex with
    MH_BATCH_FUSE_FAST).  A list with, per payload, the Result payload or the MinehipError
    miner_handle would raise (MH_ENOTREQ, MH_ERANGE: a miner skips those); errors="raise" raises
    the first one instead."""
    if errors not in ("raise", "return"):
        raise ValueError(f"errors = {errors!r}: expected 'raise' or 'return'")
    ps = [_b(p) for p in payloads]
    n, cap = len(ps), 256
    arr = (ctypes.c_int * len(devs))(*devs)
    reqs = (ctypes.c_char_p * max(1, n))(*ps)
    lens = (ctypes.c_size_t * max(1, n))(*[len(p) for p in ps])
    out = ctypes.create_string_buffer(max(1, n) * cap)
    out_lens = (ctypes.c_size_t * max(1, n))()
    status = (ctypes.c_int * max(1, n))()
    if fuse_fast:
        _check(lib.mh_miner_handle_batch_ex(arr, len(devs), reqs, lens, n, MH_BATCH_FUSE_FAST, out, cap, out_lens,
                                            status))
    else:
        _check(lib.mh_miner_handle_batch(arr, len(devs), reqs, lens, n, out, cap, out_lens, status))
    what = {MH_ENOTREQ: "not a Request", MH_ERANGE: "lower > upper"}
    res = []
    for i in range(n):
        if status[i] == MH_OK:
            res.append(out.raw[i * cap:i * cap + out_lens[i]])
            continue
        e = MinehipError(status[i], f"payload {i}: {what.get(status[i], 'failed')}")
        e.index = i
        if errors == "raise":
            raise e
        res.append(e)
    return res


# ---- bitcoin/server/server.go (stub :62) mirror: include/minehip_server.h ----
from ._lib import mh_sched_opts, mh_assignment, mh_completion, mh_sched_stats  # noqa: E402
from ._lib import mh_sched_queue_opts, MH_SCHED_MAX_DEPTH  # noqa: E402,F401


def _opts(init_chunk=None, min_chunk=None, max_chunk=None, target_ns=None):
    o = mh_sched_opts()
    lib.mh_sched_default_opts(ctypes.byref(o))
    for k, v in (("init_chunk", init_chunk), ("min_chunk", min_chunk), ("max_chunk", max_chunk),
                 ("target_ns", target_ns)):
        if v is not None:
            setattr(o, k, v)
    return o


def _queue_opts(depth=None, queue_ns=None):
    """mh_sched_queue_opts for depth / queue_ns, or None (mh_sched_create's own path) when neither
    is given.  Values that do not fit the struct's fields raise like the library's MH_EINVAL."""
    if depth is None and queue_ns is None:
        return None
    q = mh_sched_queue_opts()
    lib.mh_sched_default_queue_opts(ctypes.byref(q))
    for k, v, top in (("depth", depth, 0xFFFFFFFF), ("queue_ns", queue_ns, U64_MAX)):
        if v is None:
            continue
        if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= top:
            raise MinehipError(MH_EINVAL, f"{k} = {v!r} is out of range")
        setattr(q, k, v)
    return q


def _stats(fn, h):
    st = mh_sched_stats()
    _check(fn(h, ctypes.byref(st)))
    return {f: int(getattr(st, f)) for f, _ in mh_sched_stats._fields_}


def _first_stats(fn, h):
    st = mh_sched_first_stats()
    _check(fn(h, ctypes.byref(st)))
    return {f: int(getattr(st, f)) for f, _ in mh_sched_first_stats._fields_}


def _chk_neg(rc):
    if rc < 0:
        _check(rc)
    return rc


class Scheduler:
    """The server's chunk scheduler (mh_sched_*): jobs are client Requests,
    chunks go to miners, Results merge by the lexicographic min.  Times are
    caller-supplied nanoseconds.  depth (1..MH_SCHED_MAX_DEPTH, default 1) is how
    many chunks one miner may hold at once and queue_ns the work it may hold, as
    time at its measured rate (0: target_ns) (mh_sched_create_ex)."""

    def __init__(self, depth=None, queue_ns=None, **opts):
        self._h = None
        q = _queue_opts(depth, queue_ns)
        if q is None:
            self._h = lib.mh_sched_create(ctypes.byref(_opts(**opts)))
        else:
            self._h = lib.mh_sched_create_ex(ctypes.byref(_opts(**opts)), ctypes.byref(q))
        if not self._h:
            _check(MH_EINVAL)

    def close(self):
        if self._h:
            lib.mh_sched_destroy(self._h)
            self._h = None

    __del__ = close

    def add_miner(self, miner):
        _check(lib.mh_sched_add_miner(self._h, miner))

    def remove_miner(self, miner):
        _check(lib.mh_sched_remove_miner(self._h, miner))

    def submit(self, client, msg, lower, upper):
        m = _b(msg)
        return _chk_neg(lib.mh_sched_submit(self._h, client, m, len(m), lower, upper))

    def submit_first(self, client, msg, lower, upper, target):
        """A target job: the smallest nonce of [lower, upper] whose hash is <= target
        (mh_sched_submit_first); its completion is that hit, or the minimum when none qualifies."""
        m = _b(msg)
        return _chk_neg(lib.mh_sched_submit_first(self._h, client, m, len(m), lower, upper, target))

    def job_target(self, job):
        """The job's target, or None for a plain job (mh_sched_job_target)."""
        has = ctypes.c_int()
        t = ctypes.c_uint64()
        _check(lib.mh_sched_job_target(self._h, job, ctypes.byref(has), ctypes.byref(t)))
        return t.value if has.value else None

    def first_stats(self):
        return _first_stats(lib.mh_sched_first_stats_read, self._h)

    def drop_client(self, client):
        return _chk_neg(lib.mh_sched_drop_client(self._h, client))

    def next(self, miner=-1, now=0):
        """(miner, job, lower, upper) or None."""
        a = mh_assignment()
        if _chk_neg(lib.mh_sched_next(self._h, miner, now, ctypes.byref(a))) == 0:
            return None
        return a.miner, a.job, a.lower, a.upper

    def queue(self, miner, cap=MH_SCHED_MAX_DEPTH):
        """[(job, lower, upper), ...]: the chunks `miner` holds, oldest first (mh_sched_miner_queue)."""
        buf = (mh_assignment * max(1, cap))()
        k = _chk_neg(lib.mh_sched_miner_queue(self._h, miner, buf, cap))
        if k > cap:
            raise ValueError("queue longer than cap")
        return [(buf[i].job, buf[i].lower, buf[i].upper) for i in range(k)]

    def job_msg(self, job):
        n = ctypes.c_size_t()
        buf = ctypes.create_string_buffer(MAX_MSG)
        _check(lib.mh_sched_job_msg(self._h, job, buf, MAX_MSG, ctypes.byref(n)))
        return buf.raw[:n.value]

    def result(self, miner, hash_, nonce, now=0):
        """(job, client, hash, nonce) when this Result finished its job, else None."""
        c = mh_completion()
        if _chk_neg(lib.mh_sched_result(self._h, miner, hash_, nonce, now, ctypes.byref(c))) == 0:
            return None
        return c.job, c.client, c.hash, c.nonce

    def stats(self):
        return _stats(lib.mh_sched_stats_read, self._h)


MAX_MSG = 1 << 20  # MH_MAX_MSG_LEN


class Server:
    """The server's message loop (mh_server_*): feed it what lsp.Server.Read
    returns, send what writes() yields with lsp.Server.Write.  depth and
    queue_ns as Scheduler's (mh_server_create_ex)."""

    def __init__(self, depth=None, queue_ns=None, **opts):
        self._h = None
        q = _queue_opts(depth, queue_ns)
        if q is None:
            self._h = lib.mh_server_create(ctypes.byref(_opts(**opts)))
        else:
            self._h = lib.mh_server_create_ex(ctypes.byref(_opts(**opts)), ctypes.byref(q))
        if not self._h:
            _check(MH_EINVAL)
        self._buf = ctypes.create_string_buffer(4096)  # grown on demand (writes())

    def close(self):
        if self._h:
            lib.mh_server_destroy(self._h)
            self._h = None

    __del__ = close

    def read(self, conn, payload, now=0):
        p = _b(payload)
        _check(lib.mh_server_read(self._h, conn, p, len(p), now))

    def lost(self, conn, now=0):
        _check(lib.mh_server_lost(self._h, conn, now))

    def writes(self):
        """Drain the queued writes: list of (conn, payload bytes)."""
        out = []
        conn = ctypes.c_int64()
        n = ctypes.c_size_t()
        while True:
            rc = lib.mh_server_pop_write(self._h, ctypes.byref(conn), self._buf, len(self._buf), ctypes.byref(n))
            if rc == MH_EINVAL and n.value > len(self._buf):
                # an encoded Request can be ~6x its Data (JSON escapes): grow to the reported size
                self._buf = ctypes.create_string_buffer(n.value)
                continue
            if _chk_neg(rc) != 1:
                return out
            out.append((conn.value, self._buf.raw[:n.value]))

    def stats(self):
        return _stats(lib.mh_server_stats, self._h)

    def first_stats(self):
        return _first_stats(lib.mh_server_first_stats, self._h)

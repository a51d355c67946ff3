"""ctypes binding of libminehip.so (C-ABI: include/minehip.h, include/minehip_server.h).

The library is built in-tree (``make`` at the repo root, or
``__graft_entry__.build()``) next to this file.  There is no fallback: if the
shared object is missing, importing this module raises.

MINEHIP_LIB names another build of the same ABI to load instead -- the dev
build (``make dev``: build/dev/libminehip.so, with the experiment and test
hooks) for tools/kbench.py A/Bs and the GPU tests that inject failures.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB_PATH = os.path.join(_HERE, "libminehip.so")
LIB_PATH = os.environ.get("MINEHIP_LIB") or PRODUCT_LIB_PATH

MH_OK = 0
MH_EINVAL = -1
MH_ERANGE = -2
MH_ETOOLONG = -3
MH_ENODEV = -4
MH_EHIP = -5
MH_ENOTREQ = -6
MH_EINTERNAL = -7
MH_EREJECTED = -8
OPS_PER_BLOCK = 1376  # MH_OPS_PER_BLOCK
MH_ABI_VERSION = 5    # include/minehip.h: the struct layouts below are this version's
MH_MAX_WORKERS = 256  # most devices one mh_search_multi / mh_multi_plan call may list
MH_HITS_MAX_CAP = 1 << 20  # most entries one mh_search_hits call returns
MH_BATCH_FUSE_FAST = 1     # mh_search_batch_ex / mh_batch_plan_ex flag
MH_BATCH_FAST_MAX_NONCES = 10 ** 9  # most nonces of a request MH_BATCH_FUSE_FAST fuses
MH_FIRST_STOP_RUNNING = 1  # mh_search_first_ex flag
MH_SCHED_MAX_DEPTH = 64    # include/minehip_server.h: most chunks one miner may hold at once

#: every symbol include/*.h declares
EXPORTS = (
    "mh_abi_version", "mh_device_count", "mh_search", "mh_search_multi", "mh_hash_batch",
    "mh_last_error", "mh_msg_encode", "mh_msg_decode", "mh_miner_handle",
    "mh_profile_enable", "mh_profile_read", "mh_profile_kernels", "mh_plan", "mh_multi_plan",
    "mh_multi_rates", "mh_search_batch", "mh_batch_plan", "mh_miner_handle_batch",
    "mh_search_first", "mh_search_first_batch", "mh_first_batch_order", "mh_search_hits",
    "mh_search_hits_batch", "mh_hits_batch_regions", "mh_search_batch_ex", "mh_batch_plan_ex",
    "mh_search_first_batch_ex", "mh_first_batch_order_ex", "mh_search_hits_batch_ex", "mh_hits_batch_regions_ex",
    "mh_miner_handle_batch_ex", "mh_search_first_ex", "mh_search_first_batch_stop",
    "mh_search_first_hits", "mh_first_hits_slices", "mh_first_hits_bound",
    "mh_search_first_hits_batch", "mh_first_hits_batch_regions",
    "mh_msg_encode_ex", "mh_msg_decode_ex", "mh_search_first_multi",
    # minehip_server.h
    "mh_sched_default_opts", "mh_sched_create", "mh_sched_destroy", "mh_sched_add_miner",
    "mh_sched_remove_miner", "mh_sched_submit", "mh_sched_drop_client", "mh_sched_next",
    "mh_sched_job_msg", "mh_sched_result", "mh_sched_stats_read",
    "mh_server_create", "mh_server_destroy", "mh_server_read", "mh_server_lost",
    "mh_server_pop_write", "mh_server_stats",
    "mh_sched_default_queue_opts", "mh_sched_create_ex", "mh_server_create_ex", "mh_sched_miner_queue",
    "mh_sched_submit_first", "mh_sched_job_target", "mh_sched_first_stats_read", "mh_server_first_stats",
)


class mh_piece(ctypes.Structure):
    _fields_ = [("first", ctypes.c_uint64), ("count", ctypes.c_uint64), ("kind", ctypes.c_int32),
                ("digits", ctypes.c_int32), ("lo_digits", ctypes.c_int32), ("word", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("blocks", ctypes.c_int32), ("nonce_ops", ctypes.c_uint32),
                ("nonce_slots", ctypes.c_uint32)]


class mh_kernel_stat(ctypes.Structure):
    _fields_ = [("word", ctypes.c_int32), ("mode", ctypes.c_int32), ("launches", ctypes.c_uint64),
                ("nonces", ctypes.c_uint64), ("ns", ctypes.c_uint64), ("ops", ctypes.c_uint64),
                ("slots", ctypes.c_uint64), ("lo_digits", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class mh_span(ctypes.Structure):
    _fields_ = [("lower", ctypes.c_uint64), ("upper", ctypes.c_uint64), ("worker", ctypes.c_int32),
                ("kind", ctypes.c_int32), ("cost", ctypes.c_double)]


class mh_request(ctypes.Structure):
    _fields_ = [("msg", ctypes.c_char_p), ("len", ctypes.c_size_t), ("lower", ctypes.c_uint64),
                ("upper", ctypes.c_uint64)]


class mh_result(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("reserved", ctypes.c_int32), ("hash", ctypes.c_uint64),
                ("nonce", ctypes.c_uint64)]


class mh_first(ctypes.Structure):
    _fields_ = [("found", ctypes.c_int32), ("reserved", ctypes.c_int32), ("hash", ctypes.c_uint64),
                ("nonce", ctypes.c_uint64), ("scanned", ctypes.c_uint64)]


class mh_hit(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint64), ("nonce", ctypes.c_uint64)]


class mh_hits(ctypes.Structure):
    _fields_ = [("count", ctypes.c_uint64), ("stored", ctypes.c_uint64), ("hash", ctypes.c_uint64),
                ("nonce", ctypes.c_uint64)]


class mh_first_hits(ctypes.Structure):
    _fields_ = [("stored", ctypes.c_uint64), ("scanned", ctypes.c_uint64), ("hash", ctypes.c_uint64),
                ("nonce", ctypes.c_uint64)]


class mh_first_request(ctypes.Structure):
    _fields_ = [("msg", ctypes.c_char_p), ("len", ctypes.c_size_t), ("lower", ctypes.c_uint64),
                ("upper", ctypes.c_uint64), ("target", ctypes.c_uint64)]


class mh_first_result(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("found", ctypes.c_int32), ("hash", ctypes.c_uint64),
                ("nonce", ctypes.c_uint64), ("scanned", ctypes.c_uint64)]


class mh_hits_request(ctypes.Structure):
    _fields_ = [("msg", ctypes.c_char_p), ("len", ctypes.c_size_t), ("lower", ctypes.c_uint64),
                ("upper", ctypes.c_uint64), ("target", ctypes.c_uint64), ("cap", ctypes.c_uint64)]


class mh_hits_result(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("reserved", ctypes.c_int32), ("count", ctypes.c_uint64),
                ("stored", ctypes.c_uint64), ("hash", ctypes.c_uint64), ("nonce", ctypes.c_uint64),
                ("offset", ctypes.c_uint64)]


class mh_first_hits_request(ctypes.Structure):
    _fields_ = [("msg", ctypes.c_char_p), ("len", ctypes.c_size_t), ("lower", ctypes.c_uint64),
                ("upper", ctypes.c_uint64), ("target", ctypes.c_uint64), ("k", ctypes.c_uint64)]


class mh_first_hits_result(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("path", ctypes.c_int32), ("stored", ctypes.c_uint64),
                ("scanned", ctypes.c_uint64), ("hash", ctypes.c_uint64), ("nonce", ctypes.c_uint64),
                ("offset", ctypes.c_uint64)]


class mh_hits_region(ctypes.Structure):
    _fields_ = [("req", ctypes.c_uint64), ("kind", ctypes.c_int32), ("pass", ctypes.c_int32),
                ("window", ctypes.c_int32), ("reserved", ctypes.c_int32), ("offset", ctypes.c_uint64),
                ("slots", ctypes.c_uint64)]


class mh_batch_item(ctypes.Structure):
    _fields_ = [("req", ctypes.c_uint64), ("first", ctypes.c_uint64), ("count", ctypes.c_uint64),
                ("kind", ctypes.c_int32), ("pass", ctypes.c_int32), ("slot", ctypes.c_uint32),
                ("slots", ctypes.c_uint32)]


class mh_batch_piece(ctypes.Structure):
    _fields_ = [("req", ctypes.c_uint64), ("first", ctypes.c_uint64), ("count", ctypes.c_uint64),
                ("kind", ctypes.c_int32), ("pass", ctypes.c_int32), ("slot", ctypes.c_uint32),
                ("slots", ctypes.c_uint32), ("word", ctypes.c_int32), ("mode", ctypes.c_int32),
                ("lo_digits", ctypes.c_int32), ("launch", ctypes.c_int32)]


class mh_message(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int64), ("lower", ctypes.c_uint64), ("upper", ctypes.c_uint64),
                ("hash", ctypes.c_uint64), ("nonce", ctypes.c_uint64), ("data_len", ctypes.c_size_t)]


class mh_message_ex(ctypes.Structure):
    _fields_ = mh_message._fields_ + [("has_target", ctypes.c_int32), ("reserved", ctypes.c_int32),
                                      ("target", ctypes.c_uint64)]


class mh_sched_opts(ctypes.Structure):
    _fields_ = [("init_chunk", ctypes.c_uint64), ("min_chunk", ctypes.c_uint64),
                ("max_chunk", ctypes.c_uint64), ("target_ns", ctypes.c_uint64)]


class mh_sched_queue_opts(ctypes.Structure):
    _fields_ = [("depth", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("queue_ns", ctypes.c_uint64)]


class mh_assignment(ctypes.Structure):
    _fields_ = [("miner", ctypes.c_int64), ("job", ctypes.c_int64), ("lower", ctypes.c_uint64),
                ("upper", ctypes.c_uint64), ("msg_len", ctypes.c_size_t)]


class mh_completion(ctypes.Structure):
    _fields_ = [("job", ctypes.c_int64), ("client", ctypes.c_int64), ("hash", ctypes.c_uint64),
                ("nonce", ctypes.c_uint64)]


class mh_sched_stats(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in (
        "miners", "idle_miners", "jobs", "chunks_assigned", "chunks_done", "chunks_requeued",
        "nonces_done", "jobs_done", "jobs_cancelled")]


class mh_sched_first_stats(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in ("jobs_first", "jobs_found", "nonces_dropped", "results_ignored")]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libminehip.so not found at {LIB_PATH}; build it with `make` at the repo root "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    L.mh_abi_version.restype = ctypes.c_int
    got = L.mh_abi_version()
    if got != MH_ABI_VERSION:
        # a library of another ABI would read and write these structs at other strides
        raise ImportError(f"{LIB_PATH} has ABI {got}, this binding needs {MH_ABI_VERSION}: rebuild (make)")
    u8p = ctypes.c_char_p
    sz = ctypes.c_size_t
    u64 = ctypes.c_uint64
    u64p = ctypes.POINTER(ctypes.c_uint64)
    intp = ctypes.POINTER(ctypes.c_int)
    L.mh_abi_version.restype = ctypes.c_int
    L.mh_device_count.restype = ctypes.c_int
    L.mh_last_error.restype = ctypes.c_char_p
    L.mh_search.argtypes = [ctypes.c_int, u8p, sz, u64, u64, u64p, u64p]
    L.mh_search_multi.argtypes = [intp, ctypes.c_int, u8p, sz, u64, u64, u64, u64p, u64p]
    L.mh_hash_batch.argtypes = [ctypes.c_int, u8p, sz, u64p, sz, u64p]
    L.mh_msg_encode.argtypes = [ctypes.c_int64, u8p, sz, u64, u64, u64, u64, ctypes.c_char_p, sz,
                                ctypes.POINTER(sz)]
    L.mh_msg_decode.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(mh_message), ctypes.c_char_p, sz]
    L.mh_msg_encode_ex.argtypes = [ctypes.c_int64, u8p, sz, u64, u64, u64, u64, ctypes.c_int, u64, ctypes.c_char_p, sz,
                                   ctypes.POINTER(sz)]
    L.mh_msg_decode_ex.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(mh_message_ex), ctypes.c_char_p, sz]
    L.mh_search_first_multi.argtypes = [intp, ctypes.c_int, u8p, sz, u64, u64, u64, u64, ctypes.c_uint32,
                                        ctypes.POINTER(mh_first)]
    L.mh_miner_handle.argtypes = [intp, ctypes.c_int, ctypes.c_char_p, sz, ctypes.c_char_p, sz,
                                  ctypes.POINTER(sz)]
    L.mh_profile_enable.argtypes = [ctypes.c_int, ctypes.c_int]
    L.mh_profile_read.argtypes = [ctypes.c_int, u64p, ctypes.c_int]
    L.mh_profile_kernels.argtypes = [ctypes.c_int, ctypes.POINTER(mh_kernel_stat), ctypes.c_int]
    L.mh_plan.argtypes = [u8p, sz, u64, u64, ctypes.POINTER(mh_piece), ctypes.c_int64]
    L.mh_plan.restype = ctypes.c_int64
    L.mh_multi_plan.argtypes = [u8p, sz, u64, u64, ctypes.POINTER(ctypes.c_double), ctypes.c_int,
                                ctypes.POINTER(mh_span), ctypes.c_int64]
    L.mh_multi_rates.argtypes = [intp, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    L.mh_search_batch.argtypes = [ctypes.c_int, ctypes.POINTER(mh_request), sz, ctypes.POINTER(mh_result)]
    L.mh_search_first.argtypes = [ctypes.c_int, u8p, sz, u64, u64, u64, ctypes.POINTER(mh_first)]
    L.mh_search_first_ex.argtypes = [ctypes.c_int, u8p, sz, u64, u64, u64, ctypes.c_uint32, ctypes.POINTER(mh_first)]
    L.mh_search_hits.argtypes = [ctypes.c_int, u8p, sz, u64, u64, u64, ctypes.POINTER(mh_hit), sz,
                                 ctypes.POINTER(mh_hits)]
    L.mh_search_first_batch.argtypes = [ctypes.c_int, ctypes.POINTER(mh_first_request), sz,
                                        ctypes.POINTER(mh_first_result)]
    L.mh_first_batch_order.argtypes = [ctypes.POINTER(mh_request), sz, ctypes.c_int32,
                                       ctypes.POINTER(ctypes.c_uint32), ctypes.c_int64]
    L.mh_search_first_batch_ex.argtypes = [ctypes.c_int, ctypes.POINTER(mh_first_request), sz, ctypes.c_uint32,
                                           ctypes.POINTER(mh_first_result)]
    L.mh_search_first_batch_stop.argtypes = [ctypes.c_int, ctypes.POINTER(mh_first_request), sz,
                                             ctypes.POINTER(mh_first_result)]
    L.mh_first_batch_order_ex.argtypes = [ctypes.POINTER(mh_request), sz, ctypes.c_uint32, ctypes.c_int32,
                                          ctypes.c_int32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int64]
    L.mh_search_first_hits.argtypes = [ctypes.c_int, u8p, sz, u64, u64, u64, ctypes.POINTER(mh_hit), sz,
                                       ctypes.POINTER(mh_first_hits)]
    L.mh_first_hits_slices.argtypes = [u64, u64, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.mh_first_hits_bound.argtypes = [u64, u64, u64, ctypes.POINTER(ctypes.c_uint32)]
    L.mh_search_hits_batch.argtypes = [ctypes.c_int, ctypes.POINTER(mh_hits_request), sz, ctypes.POINTER(mh_hit), sz,
                                       ctypes.POINTER(mh_hits_result)]
    L.mh_search_hits_batch_ex.argtypes = [ctypes.c_int, ctypes.POINTER(mh_hits_request), sz, ctypes.c_uint32,
                                          ctypes.POINTER(mh_hit), sz, ctypes.POINTER(mh_hits_result)]
    L.mh_hits_batch_regions_ex.argtypes = [ctypes.POINTER(mh_hits_request), sz, ctypes.c_uint32,
                                           ctypes.POINTER(mh_hits_region), ctypes.c_int64]
    L.mh_hits_batch_regions.argtypes = [ctypes.POINTER(mh_hits_request), sz, ctypes.POINTER(mh_hits_region),
                                        ctypes.c_int64]
    L.mh_search_first_hits_batch.argtypes = [ctypes.c_int, ctypes.POINTER(mh_first_hits_request), sz, ctypes.c_uint32,
                                             ctypes.POINTER(mh_hit), sz, ctypes.POINTER(mh_first_hits_result)]
    L.mh_first_hits_batch_regions.argtypes = [ctypes.POINTER(mh_first_hits_request), sz, ctypes.c_uint32,
                                              ctypes.POINTER(mh_hits_region), ctypes.c_int64]
    L.mh_batch_plan.argtypes = [ctypes.POINTER(mh_request), sz, ctypes.POINTER(mh_batch_item), ctypes.c_int64]
    L.mh_search_batch_ex.argtypes = [ctypes.c_int, ctypes.POINTER(mh_request), sz, ctypes.c_uint32,
                                     ctypes.POINTER(mh_result)]
    L.mh_batch_plan_ex.argtypes = [ctypes.POINTER(mh_request), sz, ctypes.c_uint32, ctypes.POINTER(mh_batch_piece),
                                   ctypes.c_int64]
    L.mh_miner_handle_batch.argtypes = [intp, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), sz,
                                        ctypes.c_char_p, sz, ctypes.POINTER(sz), intp]
    L.mh_miner_handle_batch_ex.argtypes = [intp, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), sz,
                                           ctypes.c_uint32, ctypes.c_char_p, sz, ctypes.POINTER(sz), intp]
    vp = ctypes.c_void_p
    i64 = ctypes.c_int64
    L.mh_sched_default_queue_opts.argtypes = [ctypes.POINTER(mh_sched_queue_opts)]
    L.mh_sched_create_ex.argtypes = [ctypes.POINTER(mh_sched_opts), ctypes.POINTER(mh_sched_queue_opts)]
    L.mh_server_create_ex.argtypes = [ctypes.POINTER(mh_sched_opts), ctypes.POINTER(mh_sched_queue_opts)]
    L.mh_sched_miner_queue.argtypes = [vp, i64, ctypes.POINTER(mh_assignment), i64]
    L.mh_sched_default_opts.argtypes = [ctypes.POINTER(mh_sched_opts)]
    L.mh_sched_create.argtypes = [ctypes.POINTER(mh_sched_opts)]
    L.mh_sched_destroy.argtypes = [vp]
    L.mh_sched_add_miner.argtypes = [vp, i64]
    L.mh_sched_remove_miner.argtypes = [vp, i64]
    L.mh_sched_submit.argtypes = [vp, i64, u8p, sz, u64, u64]
    L.mh_sched_submit_first.argtypes = [vp, i64, u8p, sz, u64, u64, u64]
    L.mh_sched_job_target.argtypes = [vp, i64, intp, u64p]
    L.mh_sched_first_stats_read.argtypes = [vp, ctypes.POINTER(mh_sched_first_stats)]
    L.mh_server_first_stats.argtypes = [vp, ctypes.POINTER(mh_sched_first_stats)]
    L.mh_sched_drop_client.argtypes = [vp, i64]
    L.mh_sched_next.argtypes = [vp, i64, u64, ctypes.POINTER(mh_assignment)]
    L.mh_sched_job_msg.argtypes = [vp, i64, ctypes.c_char_p, sz, ctypes.POINTER(sz)]
    L.mh_sched_result.argtypes = [vp, i64, u64, u64, u64, ctypes.POINTER(mh_completion)]
    L.mh_sched_stats_read.argtypes = [vp, ctypes.POINTER(mh_sched_stats)]
    L.mh_server_create.argtypes = [ctypes.POINTER(mh_sched_opts)]
    L.mh_server_destroy.argtypes = [vp]
    L.mh_server_read.argtypes = [vp, i64, ctypes.c_char_p, sz, u64]
    L.mh_server_lost.argtypes = [vp, i64, u64]
    L.mh_server_pop_write.argtypes = [vp, ctypes.POINTER(i64), ctypes.c_char_p, sz, ctypes.POINTER(sz)]
    L.mh_server_stats.argtypes = [vp, ctypes.POINTER(mh_sched_stats)]
    restype = {"mh_plan": ctypes.c_int64, "mh_multi_plan": ctypes.c_int64, "mh_batch_plan": ctypes.c_int64,
               "mh_batch_plan_ex": ctypes.c_int64,
               "mh_first_batch_order": ctypes.c_int64, "mh_hits_batch_regions": ctypes.c_int64,
               "mh_first_batch_order_ex": ctypes.c_int64, "mh_hits_batch_regions_ex": ctypes.c_int64,
               "mh_first_hits_batch_regions": ctypes.c_int64,
               "mh_last_error": ctypes.c_char_p, "mh_sched_submit": i64, "mh_sched_submit_first": i64,
               "mh_sched_create": vp, "mh_server_create": vp, "mh_sched_default_opts": None,
               "mh_sched_create_ex": vp, "mh_server_create_ex": vp, "mh_sched_default_queue_opts": None,
               "mh_sched_miner_queue": i64, "mh_first_hits_bound": u64,
               "mh_sched_destroy": None, "mh_server_destroy": None}
    for name in EXPORTS:
        getattr(L, name).restype = restype.get(name, ctypes.c_int)
    return L


lib = _load()

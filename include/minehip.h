/*
 * minehip.h -- C-ABI of libminehip.so, the MI355X (gfx950) SHA-256 nonce-search
 * backend for the CMU 15-440 bitcoin miner (jack-nie/bitcoin-miner).
 *
 * The reference hot path this library replaces (line numbers into the
 * reference repository):
 *   - bitcoin/hash.go:13-17   func Hash(msg string, nonce uint64) uint64
 *       = BigEndian.Uint64(sha256(fmt.Sprintf("%s %d", msg, nonce))[:8])
 *   - bitcoin/miner/miner.go:33  the miner's scan loop (a TODO stub in the
 *       reference; specification in SURVEY.md §8(a) row A2): over the
 *       inclusive range [Lower, Upper] of a Request (bitcoin/message.go:18-34)
 *       return the first strict-< minimum, i.e. the lexicographic minimum of
 *       (hash, nonce), which becomes a Result (bitcoin/message.go:38-44).
 *
 * A Go miner binds these through cgo; the Python
 * package bitcoin-miner_amd/minehip binds them through ctypes.
 *
 * Conventions for every entry point:
 *   - Plain pointers and sizes; no torch / HIP types cross the ABI.
 *   - The caller owns every buffer.  `msg` is read (and copied) during the
 *     call only; the library never keeps a caller pointer nor hands out
 *     memory the caller must free.
 *   - Return 0 on success or a negative MH_E* code; mh_last_error() then
 *     describes the failure of the calling thread's last call.
 *   - Blocking.  Each call selects its device itself, so one OS thread per
 *     device may call concurrently (the cgo wrapper pins one goroutine per
 *     device with runtime.LockOSThread).
 *   - No CPU fallback: when no usable gfx950 device is present the search
 *     functions fail with MH_ENODEV instead of computing on the host.
 */
#ifndef MINEHIP_H
#define MINEHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Error codes (negative returns). */
#define MH_OK 0
#define MH_EINVAL (-1)   /* NULL output pointer, bad device index, ...      */
#define MH_ERANGE (-2)   /* lower > upper                                   */
#define MH_ETOOLONG (-3) /* len(msg) > MH_MAX_MSG_LEN                       */
#define MH_ENODEV (-4)   /* no HIP device / not gfx950                      */
#define MH_EHIP (-5)     /* a HIP runtime call failed (see mh_last_error)   */
#define MH_ENOTREQ (-6)  /* mh_miner_handle: the payload is not a JSON Request */
#define MH_EINTERNAL (-7) /* a launch-plan invariant failed (a library bug)  */
#define MH_EREJECTED (-8) /* mh_server_read: a client's Request was refused  */

/* Longest accepted message.  The LSP transport caps a datagram at 1000 bytes
 * (lsp/util.go:16, lsp/client_impl.go:203), i.e. ~600 bytes of Data after
 * JSON framing; the kernels themselves accept any length (the full 64-byte
 * blocks of "msg " are absorbed into a host midstate). */
#define MH_MAX_MSG_LEN (1u << 20)

/* ABI version of this header, returned by mh_abi_version(). */
#define MH_ABI_VERSION 5

int mh_abi_version(void);

/* Number of HIP devices this process can see (0 when none).  Replaces nothing
 * in the reference; lets the caller size its per-device goroutines. */
int mh_device_count(void);

/* Lexicographic min of (Hash(msg, n), n) over n in [lower, upper] (inclusive,
 * upper may be 2^64-1) on device `dev`.
 * Replaces the miner scan loop over bitcoin.Hash (miner.go:33 spec over
 * hash.go:13-17); *out_hash / *out_nonce are Result.Hash / Result.Nonce
 * (message.go:38-44). */
int mh_search(int dev, const uint8_t *msg, size_t len, uint64_t lower, uint64_t upper,
              uint64_t *out_hash, uint64_t *out_nonce);

/* Same result, the range split over the listed devices, one host thread + HIP
 * stream per listed device, merged on the host by the same lexicographic min
 * (associative, so bit-exact with mh_search).  No device-to-device traffic:
 * each span returns one 16-byte (hash, nonce).
 *   chunk == 0 (adaptive): one contiguous shard per device, sized in
 *     proportion to the device's measured rate (kept per process across
 *     calls; equal shards until measured), so each device runs one search.
 *     A range of >= 2^35 nonces per device keeps its last 1/16 back as 2
 *     chunks per device, handed out as the shards finish (mh_multi_plan
 *     shows the split).
 *   chunk > 0: fixed chunks of that many nonces from the server's scheduler
 *     (include/minehip_server.h).
 * A device that fails hands its shard or chunk back to the others; the call
 * fails only if every device fails (with the first failure's code).  A list
 * may repeat a device (its searches then run one after the other). */
int mh_search_multi(const int *devs, int ndev, const uint8_t *msg, size_t len, uint64_t lower,
                    uint64_t upper, uint64_t chunk, uint64_t *out_hash, uint64_t *out_nonce);

/* Most entries a device list of mh_search_multi / mh_multi_plan may have (one host thread each;
 * a device may be listed more than once). */
#define MH_MAX_WORKERS 256

/* out_hashes[i] = Hash(msg, nonces[i]) computed on device `dev` -- the batched
 * GPU form of bitcoin.Hash (hash.go:13-17).  n may be 0. */
int mh_hash_batch(int dev, const uint8_t *msg, size_t len, const uint64_t *nonces, size_t n,
                  uint64_t *out_hashes);

/* ---- batched search: many small Requests in one fused GPU pass ---------- */

/* One Request (message.go:27-34) and its Result.  msg is read during the call only. */
typedef struct mh_request {
    const uint8_t *msg;
    size_t len;
    uint64_t lower, upper;
} mh_request;

typedef struct mh_result {
    int32_t status, reserved; /* MH_OK, or the MH_E* of this request alone */
    uint64_t hash, nonce;     /* valid when status == MH_OK */
} mh_result;

/* out[i] = what mh_search(dev, reqs[i].msg, reqs[i].len, reqs[i].lower, reqs[i].upper) returns,
 * for n Requests at once.  A single small search is almost all fixed cost (reset, launch, merge,
 * 16-byte copy-back, host synchronise); here every request whose plan holds only generic pieces
 * (for "cmu440", ranges up to [0, 2 * 10^6]) is fused: its nonces become 2,560-nonce tiles of
 * one launch of the batch_scan kernel per pass, one segmented merge and one copy-back per pass,
 * and one host synchronise for the whole call while the passes' results fit the results buffer
 * (65,536 requests).  A pass holds up to 4,096 requests and 2^18 tiles (MINEHIP_BATCH_SLOTS
 * lowers the tiles, for tests); a request never spans passes.  A request with a fast piece, or
 * with more tiles than a pass holds, runs through the mh_search path after the fused passes
 * (fallback).  Results are in request order either way.
 * Per-request failures go to out[i].status and do not stop the others: MH_ERANGE (lower > upper),
 * MH_ETOOLONG, MH_EINVAL (msg NULL with len > 0).  The call returns MH_OK when every request
 * has a status; n == 0 returns MH_OK without touching a device; NULL arrays with n > 0 return
 * MH_EINVAL; a device-level failure (MH_ENODEV, MH_EHIP, MH_EINTERNAL) is the call's return
 * code and leaves out undefined.  One device only. */
int mh_search_batch(int dev, const mh_request *reqs, size_t n, mh_result *out);

/* mh_search_batch with flags.  flags == 0 is exactly mh_search_batch; an unknown flag bit returns
 * MH_EINVAL.  MH_BATCH_FUSE_FAST also fuses the requests whose plan holds fast pieces: the pieces
 * of one layout <J, MODE> of a pass run as one launch of the batch_fast<J, MODE> kernel (the
 * product's per-nonce loop, one workgroup per 256-run chunk of a table of pieces) beside the pass's
 * batch_scan launch, into the same per-request slot segments, so a pass is still one copy of
 * tables, its launches, one segmented merge and one copy-back, and the call one host synchronise.
 * A request is fused when its tiles and chunks fit one pass (2^18 slots; MINEHIP_BATCH_SLOTS), its
 * entries and its fast pieces (at most 1,024) one pass's tables, and it has at most
 * MH_BATCH_FAST_MAX_NONCES nonces; anything else is a fallback as in mh_search_batch.  Every
 * request keeps the pieces and lanes of its own mh_search plan (mh_batch_plan_ex shows the plan;
 * DESIGN.md section 3 has the measurements behind the cap and the lane rule).
 * out[i] is what mh_search returns for request i, bit for bit, whatever the batch holds, the lanes
 * chosen, the passes, the launch order or the fused / fallback split.  Errors are
 * mh_search_batch's.  Additive in ABI 5 (no existing struct or function changes). */
#define MH_BATCH_FUSE_FAST 1u
#define MH_BATCH_FAST_MAX_NONCES 1000000000ull
int mh_search_batch_ex(int dev, const mh_request *reqs, size_t n, uint32_t flags, mh_result *out);

/* ---- first-hit search: the smallest nonce whose hash meets a target ------ */

typedef struct mh_first {
    int32_t found, reserved;  /* 1: some nonce of the range has Hash <= target */
    uint64_t hash, nonce;     /* found: the SMALLEST such nonce and its hash;
                                 not found: exactly what mh_search returns   */
    uint64_t scanned;         /* nonces of [lower, upper] actually hashed    */
} mh_first;

/* The proof-of-work question over [lower, upper] on device `dev`: the smallest nonce n with
 * Hash(msg, n) <= target -- usually not the nonce of the range's minimum -- found without hashing
 * the whole range: once some part of the search has found a qualifying nonce, the work that lies
 * wholly above it is skipped.  The result is deterministic and bit-exact, whatever the launch
 * plan, the streams, the queue mode or the timing; only `scanned` depends on them.  It is counted
 * on the device: upper - lower + 1 when nothing qualifies (the result is then mh_search's), and
 * always >= nonce - lower + 1 otherwise, since nothing below the answer is ever skipped.
 * target == 2^64-1 makes every nonce qualify (the answer is lower); target == 0 only a zero hash.
 * Errors and calling conventions as mh_search: MH_ERANGE, MH_ETOOLONG, MH_EINVAL (out == NULL
 * too), MH_ENODEV.  Additive in ABI 5 (no existing struct changes).
 * The multi-device form is mh_search_first_multi, the batched form mh_search_first_batch, both
 * below; through the LSP protocol the question is a Request with a Target (mh_message_ex). */
int mh_search_first(int dev, const uint8_t *msg, size_t len, uint64_t lower, uint64_t upper,
                    uint64_t target, mh_first *out);

/* mh_search_first with flags.  flags == 0 is exactly mh_search_first; an unknown flag bit returns
 * MH_EINVAL before any device is touched.  mh_search_first skips work that has not begun: a
 * 256-run chunk that is already running when a hit becomes known runs to its end, and reports its
 * own hit only there.  With MH_FIRST_STOP_RUNNING (the only flag) the fast kernels are
 * stop_scan<J, MODE> (a code object of its own, loaded by the first call that asks for it): a wave
 * publishes a hit when it finds it, and once per group of ten nonces -- outside the per-nonce loop,
 * which stays the product's -- polls the published value and leaves its chunk when every nonce of
 * the chunk lies above it.  Nothing waits on the value.
 * found, hash and nonce are bit for bit mh_search_first's, whatever the plan, streams, queue mode
 * or timing (the published value is always a qualifying nonce of the range, so an abandoned chunk
 * holds only nonces above the answer; DESIGN.md section 3 has the argument).  scanned is still the
 * nonces of the range actually hashed, counted on the device by the waves themselves:
 * upper - lower + 1 when nothing qualifies, else within [nonce - lower + 1, upper - lower + 1].
 * Errors and conventions are mh_search_first's.  Opt-in: DESIGN.md section 3 has what the poll
 * costs a search without an early hit.  The batched forms do not take the flag (the stopping
 * batch is a call of its own, mh_search_first_batch_stop below).
 * Additive in ABI 5 (no existing struct or function changes). */
#define MH_FIRST_STOP_RUNNING 1u
int mh_search_first_ex(int dev, const uint8_t *msg, size_t len, uint64_t lower, uint64_t upper,
                       uint64_t target, uint32_t flags, mh_first *out);

/* mh_search_first over the listed devices: one host thread per entry of devs, each taking the
 * next chunk of `chunk` nonces from a target job of the server's scheduler (minehip_server.h:
 * chunks in ascending order, nothing handed out above a known hit, done once everything below
 * the hit is answered) and running mh_search_first_ex(devs[i], ..., flags) on it.
 * flags: 0 or MH_FIRST_STOP_RUNNING; any other bit is MH_EINVAL before a device is touched.
 * chunk == 0 means 2^30, the scheduler's own init_chunk default; it is not tuned for this call.
 * found, hash and nonce are bit for bit mh_search_first's, whatever the chunk, the number of
 * workers or the timing.  scanned is the sum of scanned over the chunks that completed, those
 * above the hit included: nonce - lower + 1 <= scanned <= upper - lower + 1 when found, and
 * upper - lower + 1 when not.
 * A device that fails hands its chunk back to the others, as in mh_search_multi's fixed-chunk
 * mode; the call fails only if every worker fails (with the first failure's code).  A list may
 * repeat a device and holds at most MH_MAX_WORKERS entries.  Errors as mh_search_first, plus
 * MH_EINVAL for a bad device list.  Additive in ABI 5. */
int mh_search_first_multi(const int *devs, int ndev, const uint8_t *msg, size_t len, uint64_t lower,
                          uint64_t upper, uint64_t target, uint64_t chunk, uint32_t flags, mh_first *out);

/* ---- batched first-hit search: many small proof-of-work questions at once ---- */

typedef struct mh_first_request {
    const uint8_t *msg;
    size_t len;
    uint64_t lower, upper, target;
} mh_first_request; /* 40 bytes */

typedef struct mh_first_result {
    int32_t status, found;        /* status: MH_OK, or the MH_E* of this request alone */
    uint64_t hash, nonce, scanned; /* valid when status == MH_OK */
} mh_first_result; /* 32 bytes */

/* out[i] = what mh_search_first(dev, reqs[i].msg, ..., reqs[i].target) gives, for n requests at
 * once.  For a request whose status is MH_OK, found, hash and nonce are exactly mh_search_first's:
 * the smallest nonce of the range with Hash <= target and its hash (found = 1), or, when nothing
 * qualifies, mh_search's result with found = 0 and scanned = upper - lower + 1.  When something
 * qualifies, nonce - lower + 1 <= scanned <= upper - lower + 1.  found, hash and nonce never
 * depend on timing, pass packing, dispatch order or the fused / fallback split; only scanned does.
 * Fused or fallback is decided as in mh_search_batch (the plan does not depend on the targets:
 * mh_batch_plan shows it): the fused requests run as 2,560-nonce tiles of one launch of the
 * batch_scan_first kernel per pass, one segmented merge and one copy-back per pass, one host
 * synchronise for the call; a fallback request runs through the mh_search_first path after the
 * fused passes.  Inside a pass the tiles are dispatched rank-major -- tile 0 of every request,
 * then tile 1 of every request that has one, and so on (mh_first_batch_order) -- so that each
 * request's lowest nonces are hashed first and a tile that starts after a smaller hit of its
 * request was reported is skipped.  A tile that has started runs to its end: there is no check
 * inside a tile, and no lane stops at its first hit.  MINEHIP_FIRST_BATCH_ORDER=request (read per
 * call) keeps the request-major order instead.
 * Per-request failures (MH_ERANGE, MH_ETOOLONG, MH_EINVAL for msg NULL with len > 0) go to
 * out[i].status and do not stop the others; n == 0 returns MH_OK without touching a device; NULL
 * arrays with n > 0 return MH_EINVAL; a device-level failure is the call's return code and leaves
 * out undefined.  Results are in request order.  One device only; no multi-device form, no fused
 * fast pieces, nothing in the LSP protocol or the miner.  Additive in ABI 5. */
int mh_search_first_batch(int dev, const mh_first_request *reqs, size_t n, mh_first_result *out);

/* mh_search_first_batch with flags.  flags == 0 is exactly mh_search_first_batch; an unknown flag
 * bit returns MH_EINVAL.  MH_BATCH_FUSE_FAST (the only flag) also fuses the requests whose plan holds
 * fast pieces, exactly as mh_search_batch_ex decides it (the plan is mh_batch_plan_ex's: the same
 * fused / fallback split, passes, slots, launches and cap, MH_BATCH_FAST_MAX_NONCES; the targets
 * play no part, and every request keeps the lanes of its own mh_search plan).  The fast pieces of
 * one layout <J, MODE> of a pass run as one launch of the batch_first<J, MODE> kernel -- the
 * first-hit per-nonce loop of mh_search_first, one workgroup per 256-run chunk of a table of
 * pieces -- behind the pass's batch_scan_first launch on the same stream and into the same
 * per-request slot segments and device words.  Before any hashing a chunk reads its request's
 * smallest reported hit once and is skipped when all its nonces are larger; a chunk that has
 * started runs to its end.  No workgroup waits for another.  Inside a launch the chunks are
 * dispatched rank-major -- chunk 0 of every piece, then chunk 1 of every piece that has one, and
 * so on (mh_first_batch_order_ex) -- unless MINEHIP_FIRST_BATCH_ORDER=request.  A pass is one copy
 * of tables, its launches, one segmented merge and one copy-back; the call has one host
 * synchronise; fallbacks run through the mh_search_first path after the fused passes.
 * Per request, found, hash and nonce are bit for bit mh_search_first's, whatever the batch holds,
 * the lanes, the passes, the order, the timing or the fused / fallback split; scanned is
 * upper - lower + 1 when nothing qualifies and nonce - lower + 1 <= scanned <= upper - lower + 1
 * otherwise.  Errors and per-request statuses are mh_search_first_batch's.  Additive in ABI 5. */
int mh_search_first_batch_ex(int dev, const mh_first_request *reqs, size_t n, uint32_t flags,
                             mh_first_result *out);

/* mh_search_first_batch_ex(MH_BATCH_FUSE_FAST) whose running chunks stop, as
 * mh_search_first_ex(MH_FIRST_STOP_RUNNING)'s do.  An entry point of its own and not a flag: the
 * flag bits of mh_search_first_batch_ex other than MH_BATCH_FUSE_FAST stay MH_EINVAL.  The plan is
 * mh_batch_plan_ex(MH_BATCH_FUSE_FAST)'s and the dispatch order
 * mh_first_batch_order_ex(MH_BATCH_FUSE_FAST)'s (MINEHIP_FIRST_BATCH_ORDER included); the generic
 * tiles, the merge, the one copy each way per pass and the one host synchronise per call are
 * mh_search_first_batch_ex's.  The fast pieces of one layout of a pass run as one launch of
 * batch_stop<J, MODE> (a code object of its own, loaded by the first call that asks for it):
 * batch_first's tables, order and skip of an unbegun chunk, around stop_scan's chunk body -- a wave
 * lowers its request's word when it finds a hit, and once per group of ten nonces, outside the
 * per-nonce loop, polls that word and leaves its chunk when every nonce of the chunk lies above
 * it.  The word is the request's own, the one its generic tiles lower too, so a hit of any piece
 * or tile of a request stops that request's running chunks and no other's.  Nothing waits on the
 * word.  A fallback request runs through the mh_search_first_ex(MH_FIRST_STOP_RUNNING) path after
 * the fused passes.
 * Per request, found, hash and nonce are bit for bit mh_search_first's, whatever the batch holds,
 * the passes, the order or the timing (DESIGN.md section 3 has the argument); scanned is counted
 * by the waves themselves: upper - lower + 1 when nothing qualifies, else within
 * [nonce - lower + 1, upper - lower + 1].  Errors, per-request statuses, n == 0 and NULL arrays are
 * mh_search_first_batch_ex's.  Opt-in: DESIGN.md section 3 has what was measured, the poll's cost
 * for a batch without a hit included.  Additive in ABI 5 (no existing struct or function changes). */
int mh_search_first_batch_stop(int dev, const mh_first_request *reqs, size_t n, mh_first_result *out);

/* ---- every hit: all nonces of a range whose hash meets a target ---------- */

#define MH_HITS_MAX_CAP (1u << 20) /* most entries one call returns */

typedef struct mh_hit {
    uint64_t hash, nonce;
} mh_hit; /* 16 bytes */

typedef struct mh_hits {
    uint64_t count;       /* nonces of [lower, upper] with Hash <= target (mod 2^64) */
    uint64_t stored;      /* entries written to hits: min(count, cap) */
    uint64_t hash, nonce; /* exactly what mh_search returns for the range */
} mh_hits; /* 32 bytes */

/* Which nonces of [lower, upper] have Hash(msg, n) <= target, and how many -- the shares a pool
 * collects, the sample a difficulty estimate needs.  out->count is the exact number of them,
 * hits[0 .. out->stored) the stored = min(count, cap) SMALLEST of them in strictly increasing
 * nonce order, each with its hash, and out->hash / out->nonce the range's minimum, whether or not
 * anything qualifies.  cap == 0 with hits == NULL asks for the count (and the minimum) alone.
 * The call hashes the whole range once, like mh_search: the scan kernels are mh_search's with an
 * append of every hit to a device buffer, so there is no early end.  It is built for sparse
 * targets; a loose one, where most wave steps hold a hit, is correct but slow (the hits of a wave
 * step are appended one after the other).  The buffer holds MH_HITS_MAX_CAP entries
 * (MINEHIP_HITS_SLOTS, read per call, lowers that for tests); with more hits than that and
 * cap > 0, the list is rebuilt from `lower` upward by re-scanning windows of the range until
 * `stored` entries are collected.  Nothing returned depends on the launch plan, the streams, the
 * queue mode, the timing or the size of that buffer.
 * Errors: MH_EINVAL for out == NULL, cap > MH_HITS_MAX_CAP, or hits == NULL with cap > 0;
 * MH_ERANGE, MH_ETOOLONG, MH_ENODEV as mh_search.  One device only; nothing in the LSP protocol;
 * the batched form is mh_search_hits_batch below.  Additive in ABI 5 (no existing struct changes). */
int mh_search_hits(int dev, const uint8_t *msg, size_t len, uint64_t lower, uint64_t upper,
                   uint64_t target, mh_hit *hits, size_t cap, mh_hits *out);

/* ---- the first k hits: the k smallest qualifying nonces, without the full scan ---- */

typedef struct mh_first_hits {
    uint64_t stored;      /* entries written to hits: min(k, qualifying nonces of the range) */
    uint64_t scanned;     /* nonces of [lower, upper] actually hashed */
    uint64_t hash, nonce; /* stored < k: exactly what mh_search returns for the range;
                             stored == k: the lexicographic minimum (hash, nonce) of the k entries */
} mh_first_hits; /* 32 bytes */

/* The first k nonces of [lower, upper] with Hash(msg, n) <= target -- what a share collector asks --
 * between mh_search_first (k = 1, stops early) and mh_search_hits (every hit, never stops early).
 * hits[0 .. out->stored) are the `stored` smallest such nonces in strictly increasing nonce order,
 * each with its hash: bit for bit the first `stored` entries mh_search_hits(..., cap = k) returns.
 * stored, the entries, hash and nonce never depend on the launch plan, the streams, the queue mode,
 * the timing or MINEHIP_HITS_SLOTS; only `scanned` does.  With stored < k the whole range was
 * hashed: scanned == upper - lower + 1 and hash / nonce are mh_search's.  With stored == k,
 * hits[k-1].nonce - lower + 1 <= scanned <= upper - lower + 1.  Hence with k == 1, stored, hash and
 * nonce equal mh_search_first's found, hash and nonce; with k >= count, stored, the entries, hash
 * and nonce equal mh_search_hits' count, entries and minimum.
 * The scan kernels are mh_search_hits' with one device word per search, the bound: every hit that is
 * appended also counts in one of at most 1,024 slices of the range (mh_first_hits_slices), and once
 * the slices hold k hits the end of the slice where the prefix sum reaches k is published
 * (mh_first_hits_bound), only ever lowered: at least k qualifying nonces are <= it, so a chunk or
 * tile wholly above it is skipped and a running chunk is left at its next group of ten nonces.
 * Nothing waits on the word; a stale read only stops later.  If the device hit buffer
 * (MH_HITS_MAX_CAP entries, MINEHIP_HITS_SLOTS) overflowed, the list is rebuilt from `lower` upward
 * by mh_search_hits' window walk until k entries are collected.
 * Errors, before any device is touched: MH_EINVAL for out == NULL, hits == NULL, k == 0 or
 * k > MH_HITS_MAX_CAP; MH_ERANGE, MH_ETOOLONG and MH_EINVAL for a NULL msg with len > 0, as
 * mh_search; then MH_ENODEV.  The dev build refuses the hash and code-object hooks as
 * mh_search_hits does.  One device only; the batched form is mh_search_first_hits_batch below;
 * nothing in the LSP protocol or the miner.
 * Additive in ABI 5 (no existing struct or function changes). */
int mh_search_first_hits(int dev, const uint8_t *msg, size_t len, uint64_t lower, uint64_t upper,
                         uint64_t target, mh_hit *hits, size_t k, mh_first_hits *out);

/* Host only: shift and slice count (<= 1024) mh_search_first_hits uses for [lower, upper]: slices of
 * 2^shift nonces, shift the smallest value with 1024 << shift >= upper - lower + 1.  MH_EINVAL for a
 * NULL pointer, MH_ERANGE for lower > upper. */
int mh_first_hits_slices(uint64_t lower, uint64_t upper, uint32_t *shift, uint32_t *slices);
/* Host only: the value the kernels publish from these slice counts (counts[s]: hits counted in
 * slice s, nonces lower + (s << shift) ..): lower + min(upper - lower, ((s + 1) << shift) - 1) for
 * the first slice s whose prefix sum is >= k; 2^64-1 while the counts sum to < k (or for a NULL
 * pointer, k == 0 or lower > upper). */
uint64_t mh_first_hits_bound(uint64_t lower, uint64_t upper, uint64_t k, const uint32_t *counts);

/* ---- batched hits: every hit of many small Requests in one pass ----------- */

typedef struct mh_hits_request {
    const uint8_t *msg;
    size_t len;
    uint64_t lower, upper, target;
    uint64_t cap; /* most entries wanted for this request, <= MH_HITS_MAX_CAP; 0: count only */
} mh_hits_request; /* 48 bytes */

typedef struct mh_hits_result {
    int32_t status, reserved; /* MH_OK, or the MH_E* of this request alone */
    uint64_t count, stored;   /* as mh_hits: exact count; stored = min(count, cap) */
    uint64_t hash, nonce;     /* exactly what mh_search returns for the range */
    uint64_t offset;          /* this request's entries are hits[offset .. offset + stored) */
} mh_hits_result; /* 48 bytes */

/* For every request whose status is MH_OK: count, stored, hash, nonce and the `stored` entries at
 * hits + offset are exactly what mh_search_hits(dev, msg, len, lower, upper, target, hits + offset,
 * cap, ...) gives -- the min(count, cap) smallest qualifying nonces in strictly increasing nonce
 * order, each with its hash, and the range's minimum whether or not anything qualifies.  Nothing
 * returned depends on pass packing, the fused / fallback split, the size of the device hit buffer
 * or timing.
 * offset of request i is the sum of cap over requests 0 .. i-1 whatever their status, a cap above
 * MH_HITS_MAX_CAP counting as 0: the caller can compute the offsets beforehand, and the regions
 * never overlap.  hits holds hits_cap entries.
 * Fused or fallback is decided as in mh_search_batch (the plan depends neither on the targets nor
 * on the caps: mh_batch_plan shows it).  The fused requests run as 2,560-nonce tiles of one launch
 * of the batch_scan_hits kernel per pass -- batch_scan with an append of every hit through a
 * per-request cursor into the request's region of the device hit buffer -- one segmented merge and
 * one copy-back of {hash, nonce, count} per pass; the whole range is hashed, there is no early
 * end, since the count needs it.  The device hit buffer holds MH_HITS_MAX_CAP entries
 * (MINEHIP_HITS_SLOTS, read per call, lowers that for tests) and is handed out in windows: a
 * request gets min(cap, its nonce count, what the window has left) entries, and a pass whose
 * requests want more than the window has left starts a new window after a drain (one host
 * synchronise and one copy of the entries stored; mh_hits_batch_regions shows the schedule).  A
 * batch whose wants fit one window has one synchronise.  A fallback request runs through the
 * mh_search_hits path after the fused passes.
 * Asking for fewer entries than qualify (0 < cap < count, or a region cut short by the window)
 * costs that request a second scan: which entries its region kept depends on timing, so its list
 * is rebuilt through the mh_search_hits path; cap == 0 never needs that.  Built for sparse
 * targets, as mh_search_hits: a loose one is correct but slow.
 * Per-request failures go to out[i].status and do not stop the others: MH_ERANGE, MH_ETOOLONG,
 * MH_EINVAL (msg NULL with len > 0, or cap > MH_HITS_MAX_CAP).  For the call: MH_EINVAL for NULL
 * reqs or out with n > 0, for the sum of the caps (as counted for offset) above hits_cap, and for
 * hits == NULL with that sum above 0; n == 0 returns MH_OK without touching a device; a
 * device-level failure (MH_ENODEV, MH_EHIP, MH_EINTERNAL) is the call's return code and leaves
 * out undefined.  One device only; nothing in the LSP protocol or the miner.  Additive in ABI 5. */
int mh_search_hits_batch(int dev, const mh_hits_request *reqs, size_t n, mh_hit *hits, size_t hits_cap,
                         mh_hits_result *out);

/* mh_search_hits_batch with flags.  flags == 0 is exactly mh_search_hits_batch; an unknown flag bit
 * returns MH_EINVAL.  MH_BATCH_FUSE_FAST (the only flag) also fuses the requests whose plan holds
 * fast pieces, exactly as mh_search_batch_ex decides it (the plan is mh_batch_plan_ex's: the same
 * fused / fallback split, passes, slots, launches, lane rule and cap, MH_BATCH_FAST_MAX_NONCES;
 * targets and caps play no part).  The fast pieces of one layout <J, MODE> of a pass run as one
 * launch of the batch_hits<J, MODE> kernel -- the per-nonce loop and the append of mh_search_hits,
 * one workgroup per 256-run chunk of a table of pieces -- behind the pass's batch_scan_hits launch
 * on the same stream: the fast pieces and the generic tiles of one request append through one
 * cursor into one region of the device hit buffer and write the request's one slot segment.  Every
 * chunk runs (the count needs every nonce); no workgroup waits for another.  A pass is one copy of
 * tables, its launches, one segmented merge and one copy-back; windows, drains, region sizes and
 * rebuilds are mh_search_hits_batch's (mh_hits_batch_regions_ex shows the schedule), the items and
 * per-chunk tables counting against the table buffer a window's passes share; rebuilds and
 * fallbacks run through the mh_search_hits path after the fused passes, a list cut by its cap
 * (0 < cap < count) from a prefix of the range sized by the fused scan's count for cap hits.
 * For every request whose status is MH_OK: count, stored, hash, nonce and the `stored` entries at
 * hits + offset are bit for bit mh_search_hits', whatever the batch holds, the lanes, the passes,
 * the fused / fallback split, the size of the device hit buffer or the timing.  offset, the
 * per-request statuses and the call's errors are mh_search_hits_batch's.  Measured
 * (profiles/hits_batch_fast_latency.json): no size up to 8 x 10^9 nonces is slower
 * fused than the fallback loop by more than that loop's own spread, so the cap stays
 * MH_BATCH_FAST_MAX_NONCES.  Additive in ABI 5. */
int mh_search_hits_batch_ex(int dev, const mh_hits_request *reqs, size_t n, uint32_t flags, mh_hit *hits,
                            size_t hits_cap, mh_hits_result *out);

/* ---- batched first k hits: the k smallest hits of many Requests ---------- */

typedef struct mh_first_hits_request {
    const uint8_t *msg;
    size_t len;
    uint64_t lower, upper, target;
    uint64_t k; /* entries wanted for this request, 1 .. MH_HITS_MAX_CAP */
} mh_first_hits_request; /* 48 bytes */

typedef struct mh_first_hits_result {
    int32_t status; /* MH_OK, or the MH_E* of this request alone (the other fields are then 0, but offset) */
    int32_t path;   /* 0 answered from the fused pass; 1 fallback (never fused); 2 fused, then rebuilt
                       through the mh_search_first_hits path */
    uint64_t stored, scanned, hash, nonce; /* exactly mh_first_hits' fields */
    uint64_t offset; /* this request's entries are hits[offset .. offset + stored) */
} mh_first_hits_result; /* 48 bytes */

/* mh_search_first_hits for n requests on one device.  For every request whose status is MH_OK,
 * stored, hash, nonce and the `stored` entries at hits + offset are bit for bit what
 * mh_search_first_hits(dev, msg, len, lower, upper, target, hits + offset, k, ...) returns; they do
 * not depend on the batch's contents, the packing into passes, the dispatch order
 * (MINEHIP_FIRST_BATCH_ORDER), the fused / fallback / rebuilt split, MINEHIP_HITS_SLOTS,
 * MINEHIP_BATCH_SLOTS or timing.  Only scanned and path may: with stored < k, scanned ==
 * upper - lower + 1; with stored == k, hits[k-1].nonce - lower + 1 <= scanned <= upper - lower + 1.
 * offset of request i is the sum of k over requests 0 .. i-1 whatever their status, a k of 0 or
 * above MH_HITS_MAX_CAP counting as 0 (mh_search_hits_batch's rule for cap).  hits holds hits_cap
 * entries.
 * flags == 0 fuses the requests whose plan holds only generic pieces (mh_batch_plan's split);
 * MH_BATCH_FUSE_FAST (the only flag; any other bit: MH_EINVAL before a device is touched) also
 * fuses requests with fast pieces exactly as mh_batch_plan_ex decides it (the same cap,
 * MH_BATCH_FAST_MAX_NONCES, and lane rule).  The plan depends on neither targets nor k.
 * A fused request has one set of device words in its pass's tables -- target, cursor, region, k,
 * bound, the slicing of its own range (mh_first_hits_slices, mh_first_hits_bound) and the scanned
 * count -- and 1,024 slice counters of its own.  Its generic tiles (batch_scan_bound, taken in
 * mh_first_batch_order_ex's rank-major order) and the chunks of its fast pieces (batch_bound<J, MODE>)
 * append through its cursor into its region of the device hit buffer, count every hit in its slices
 * before the cursor advances, publish its bound once the slices hold k hits, and skip a tile or chunk
 * -- or leave a running chunk at its next group of ten nonces -- that lies wholly above its bound.  A
 * request's bound stops that request's work and no other's.  Nothing waits on a word.
 * A request gets min(its nonce count, max(4 k, 256), what the window has left) entries of the device
 * hit buffer (mh_first_hits_batch_regions shows the schedule); windows and drains are
 * mh_search_hits_batch's, and a batch whose wants fit one window has one host synchronise.  A fused
 * request that appended more hits than its region holds (path 2) and a fallback (path 1) run through
 * the mh_search_first_hits path after the fused passes.
 * Per-request failures go to out[i].status and do not stop the others: MH_ERANGE, MH_ETOOLONG,
 * MH_EINVAL (msg NULL with len > 0, k == 0 or k > MH_HITS_MAX_CAP).  For the call: MH_EINVAL for
 * NULL reqs or out with n > 0, for the sum of k (as counted for offset) above hits_cap, and for
 * hits == NULL with that sum above 0; n == 0 returns MH_OK without touching a device; a
 * device-level failure (MH_ENODEV, MH_EHIP, MH_EINTERNAL) is the call's return code and leaves out
 * undefined.  The dev build refuses the hash and code-object hooks as mh_search_first_hits does.
 * One device only; nothing in the LSP protocol or the miner.  Additive in ABI 5. */
int mh_search_first_hits_batch(int dev, const mh_first_hits_request *reqs, size_t n, uint32_t flags,
                               mh_hit *hits, size_t hits_cap, mh_first_hits_result *out);

/* Thread-local description of the calling thread's last failure ("" if none). */
const char *mh_last_error(void);

/* ---- miner process (bitcoin/miner/miner.go, bitcoin/message.go) -------- */

/* bitcoin.Message (message.go:18-23).  type: 0 Join, 1 Request, 2 Result
 * (message.go:7-13). */
typedef struct mh_message {
    int64_t type;
    uint64_t lower, upper;
    uint64_t hash, nonce;
    size_t data_len; /* bytes of Data (UTF-8) */
} mh_message;

/* Go json.Marshal of bitcoin.Message{type, data, lower, upper, hash, nonce},
 * byte for byte: {"Type":..,"Data":"..","Lower":..,"Upper":..,"Hash":..,
 * "Nonce":..} with Go's string escaping (HTML-safe, invalid UTF-8 ->
 * \ufffd).  *out_len receives the needed size; MH_EINVAL if cap is short. */
int mh_msg_encode(int64_t type, const uint8_t *data, size_t dlen, uint64_t lower, uint64_t upper,
                  uint64_t hash, uint64_t nonce, char *out, size_t cap, size_t *out_len);

/* Go json.Unmarshal into bitcoin.Message: case-insensitive keys, unknown
 * keys ignored.  Data (UTF-8) is copied to data[0..data_len); MH_ETOOLONG
 * if data_cap is short (out->data_len still set), MH_EINVAL on bad JSON. */
int mh_msg_decode(const char *json, size_t len, mh_message *out, uint8_t *data, size_t data_cap);

/* A Message with the optional Target of a Request: the proof-of-work question (mh_search_first)
 * through the protocol.  The reference's Message has no such field, and needs none to stay
 * compatible: Go's json.Unmarshal ignores unknown keys, so every reference endpoint reads a
 * Request that carries "Target" as a plain Request.  (In Go the field is
 *     Target *uint64 `json:",omitempty"`
 * as the last field of bitcoin.Message; INTEGRATION.md.)  A Result has no new field: a chunk
 * with a hit answers with that hit, one without with its minimum, and whoever merges tells them
 * apart by hash <= target. */
typedef struct mh_message_ex {
    int64_t type;
    uint64_t lower, upper;
    uint64_t hash, nonce;
    size_t data_len;
    int32_t has_target, reserved; /* 1: the payload has a "Target" key that is not null */
    uint64_t target;              /* its value; 0 without one */
} mh_message_ex;

/* mh_msg_encode, and when has_target != 0 `,"Target":<target>` as a seventh and last key.  With
 * has_target == 0 the bytes are mh_msg_encode's.  Additive in ABI 5. */
int mh_msg_encode_ex(int64_t type, const uint8_t *data, size_t dlen, uint64_t lower, uint64_t upper,
                     uint64_t hash, uint64_t nonce, int has_target, uint64_t target, char *out, size_t cap,
                     size_t *out_len);

/* mh_msg_decode that also reads the key "Target" (case-insensitive, as every key): a uint64,
 * refused (MH_EINVAL) when malformed, negative, fractional or above 2^64-1, exactly as Lower is;
 * null counts as absent.  mh_msg_decode itself ignores the key.  Additive in ABI 5. */
int mh_msg_decode_ex(const char *json, size_t len, mh_message_ex *out, uint8_t *data, size_t data_cap);

/* One step of the GPU miner (miner.go:33 TODO, spec SURVEY.md §8(a) A2):
 * decode a Request payload, search [Lower, Upper] on the listed devices,
 * encode NewResult(hash, nonce) (message.go:38-44) into out.  The Go miner
 * wraps this between lsp.Client.Read and lsp.Client.Write.  MH_ENOTREQ when
 * the payload is not a JSON bitcoin.Message of type Request, MH_ERANGE when
 * its Lower > Upper: a miner skips those.  Any other error comes from the
 * search itself (MH_EHIP, MH_EINTERNAL, ...): the miner should exit, so the
 * server's lost-miner path hands the chunk to another miner.
 * A Request with a Target (mh_message_ex) is answered by NewResult(hash, nonce) of the first-hit
 * search of [Lower, Upper]: mh_search_first_ex on one listed device, mh_search_first_multi
 * (chunk 0) on several -- the chunk's smallest qualifying nonce, or its minimum when none
 * qualifies, which is what the server's target jobs rely on (minehip_server.h). */
int mh_miner_handle(const int *devs, int ndev, const char *request, size_t len, char *out, size_t cap,
                    size_t *out_len);

/* The same step for n payloads a miner holds at once (its connection's queue): status[i], the
 * bytes at out + i * cap_each and out_lens[i] are what mh_miner_handle would give for
 * requests[i] (lens[i] bytes) with a buffer of cap_each bytes, MH_ENOTREQ and MH_ERANGE
 * included.  The valid Requests that mh_search_batch fuses go through one mh_search_batch on
 * devs[0]; the others (fallbacks) through mh_miner_handle's own path, over all listed devices.
 * Returns MH_OK when every payload has a status (MH_OK: answer with the Result; MH_ENOTREQ,
 * MH_ERANGE: skip; MH_EINVAL: cap_each is short, out_lens[i] is the size needed); a device-level
 * failure of a search (MH_ENODEV, MH_EHIP, MH_EINTERNAL) is the call's return code: the miner
 * should exit.  out_lens may be NULL.
 * When some payload carries a Target (mh_message_ex), the plain Requests go where they go
 * otherwise and the Target Requests through one mh_search_first_batch_ex on devs[0] (with
 * MH_BATCH_FUSE_FAST when mh_miner_handle_batch_ex was given it; the requests that call runs as
 * fallbacks take its own fallback path).  Statuses and Results stay in payload order, each bit
 * for bit mh_miner_handle's for that payload.  A list without a Target runs as it always did. */
int mh_miner_handle_batch(const int *devs, int ndev, const char *const *requests, const size_t *lens, size_t n,
                          char *out, size_t cap_each, size_t *out_lens, int *status);

/* mh_miner_handle_batch with the flags of mh_search_batch_ex: flags == 0 is mh_miner_handle_batch;
 * MH_BATCH_FUSE_FAST runs the fused part through mh_search_batch_ex's plan, so queued Requests
 * of up to MH_BATCH_FAST_MAX_NONCES nonces fuse too (the others still go through
 * mh_miner_handle's own path, over all listed devices).  Statuses, Results and return code as
 * mh_miner_handle_batch, bit for bit; an unknown flag bit returns MH_EINVAL. */
int mh_miner_handle_batch_ex(const int *devs, int ndev, const char *const *requests, const size_t *lens, size_t n,
                             uint32_t flags, char *out, size_t cap_each, size_t *out_lens, int *status);

/* ---- measurement (no reference counterpart; used by bench.py) ---------- */

/* Enable (on != 0: counters reset) or disable (counters kept, readable) the
 * HIP-event timing of every search-kernel launch on `dev`'s stream. */
int mh_profile_enable(int dev, int on);

/* Counters since the last mh_profile_enable(dev, 1):
 *   out[0] launches of the dominant (fast search) kernel
 *   out[1] nonces those launches processed
 *   out[2] summed kernel duration, nanoseconds (HIP events on the lib's stream)
 *   out[3] algorithmic VALU instructions of those launches: per piece,
 *          nonces x mh_piece.nonce_ops (the nonce-dependent SHA-256 work,
 *          DESIGN.md §4); x64 lanes = int32 lane-ops
 *   out[4] nonces processed by the generic (edge) kernel
 *   out[5] generic kernel duration, nanoseconds
 *   out[6] the same fast-kernel work in SIMD-32 issue slots: per piece,
 *          nonces x mh_piece.nonce_slots (the roofline unit)
 * n = number of slots the caller provides (<= 8). */
int mh_profile_read(int dev, uint64_t *out, int n);

/* Per fast_search<J, MODE> variant and lane length L (lo_digits: 10^L
 * nonces per lane) counters since mh_profile_enable(dev, 1); the roofline's
 * "dominant kernel" is the entry with the largest ns.  The kernel name in a
 * rocprofv3 trace is `mh::fast_search<word, mode>` for every L (the trace
 * tells the launches apart by grid size).  ABI 3 appended lo_digits. */
typedef struct mh_kernel_stat {
    int32_t word, mode;
    uint64_t launches, nonces, ns, ops, slots;
    int32_t lo_digits, reserved;
} mh_kernel_stat;

/* Writes up to cap variants that ran; returns how many ran (or MH_E*). */
int mh_profile_kernels(int dev, mh_kernel_stat *out, int cap);

/* gfx950 VALU instructions of one full SHA-256 compression with no work
 * hoisted (64 rounds x 14 + 48 schedule words x 10). */
#define MH_OPS_PER_BLOCK 1376u

/* ---- introspection (host only, no GPU needed; used by CPU tests) -------- */

/* One piece of a search plan: [first, first+count-1] covered by one kernel. */
typedef struct mh_piece {
    uint64_t first;
    uint64_t count;
    int32_t kind;       /* 0 = fast run kernel, 1 = generic per-nonce kernel */
    int32_t digits;     /* decimal digits of every nonce in the piece */
    int32_t lo_digits;  /* fast: digits enumerated inside a run (L)        */
    int32_t word;       /* fast: message word of the per-nonce digit (J): the last digit's, or
                           (modes 3..5) the word before it, whose last byte is then the digit
                           enumerated innermost (ABI 5) */
    int32_t mode;       /* fast: 0 one block, 1 prefix block per run, 2 two blocks per nonce;
                           3, 4, 5 the same with the innermost digit in word J (ABI 5) */
    int32_t blocks;     /* tail blocks hashed per nonce in the final message */
    uint32_t nonce_ops; /* fast: algorithmic VALU instructions per nonce */
    uint32_t nonce_slots; /* fast: the same work in SIMD-32 issue slots */
} mh_piece;

/* Plan the search of [lower, upper] for `msg`: writes the pieces in
 * increasing nonce order to out (may be NULL) and returns how many there are,
 * or cap + 1 when the plan has more than cap pieces (the first cap written),
 * or a negative MH_E* code. */
int64_t mh_plan(const uint8_t *msg, size_t len, uint64_t lower, uint64_t upper, mh_piece *out, int64_t cap);

/* One item of a batch plan: an entry (one generic piece) of a fused request, or a fallback
 * request. */
typedef struct mh_batch_item {
    uint64_t req;          /* index into reqs */
    uint64_t first, count; /* fused: the entry's nonces; fallback: the request's (count mod 2^64) */
    int32_t kind;          /* 0 fused, 1 fallback */
    int32_t pass;          /* fused: its pass, from 0; fallback: -1 */
    uint32_t slot, slots;  /* fused: first partial slot within the pass, and tiles: the aligned
                              decades first/10 .. (first+count-1)/10 in tiles of 256 decades
                              (2,560 nonces); fallback: 0, 0 */
} mh_batch_item;

/* Host only: how mh_search_batch would run reqs[0..n): one item per entry of a fused request and
 * one item (slots = 0) per fallback request, in request order.  Within a pass the fused requests'
 * slot segments are contiguous, disjoint and in order.  Returns the item count, cap + 1 when there
 * are more than cap (the first cap written, as mh_plan), or the MH_E* of the first request
 * mh_search would refuse.  n == 0 returns 0. */
int64_t mh_batch_plan(const mh_request *reqs, size_t n, mh_batch_item *out, int64_t cap);

/* One piece of a fused request of mh_search_batch_ex's plan, or one fallback request. */
typedef struct mh_batch_piece {
    uint64_t req;          /* index into reqs */
    uint64_t first, count; /* the piece's nonces; fallback: the request's (count mod 2^64) */
    int32_t kind;          /* 0 fused generic entry, 1 fallback, 2 fused fast piece */
    int32_t pass;          /* fused: its pass, from 0; fallback: -1 */
    uint32_t slot, slots;  /* fused: first partial slot within the pass, and its tiles (kind 0, as
                              mh_batch_item) or 256-run chunks (kind 2); fallback: 0, 0 */
    int32_t word, mode, lo_digits; /* kind 2: J, MODE and L, as mh_piece; else 0 */
    int32_t launch;        /* kind 2: index of its batch_fast launch within the pass (one launch per
                              layout, pieces ordered by L descending, then request order); else -1 */
} mh_batch_piece;

/* Host only: how mh_search_batch_ex(flags) would run reqs[0..n): one piece per entry and per fast
 * piece of a fused request, in nonce order, and one (slots = 0) per fallback request, in request
 * order.  Within a pass the fused requests' slot segments are contiguous, disjoint and in order,
 * and a request's pieces fill its segment in nonce order.  flags == 0: mh_batch_plan's plan.
 * Honours every MINEHIP_* planning variable the call honours.  Returns as mh_batch_plan does;
 * MH_EINVAL for an unknown flag bit. */
int64_t mh_batch_plan_ex(const mh_request *reqs, size_t n, uint32_t flags, mh_batch_piece *out, int64_t cap);

/* Host only: the dispatch order of pass `pass` of mh_search_first_batch over reqs[0..n) (the plan
 * is mh_batch_plan's; the targets play no part): out[b] is the partial slot of the tile that
 * workgroup b of batch_scan_first runs, a permutation of the pass's slots.  Rank-major unless
 * MINEHIP_FIRST_BATCH_ORDER=request; honours MINEHIP_BATCH_SLOTS.  Returns the pass's tile count,
 * cap + 1 when there are more than cap (the first cap written, as mh_plan), the MH_E* of the
 * first request mh_search would refuse, or MH_EINVAL when the plan has no such pass. */
int64_t mh_first_batch_order(const mh_request *reqs, size_t n, int32_t pass, uint32_t *out, int64_t cap);

/* Host only: the dispatch order of one launch of pass `pass` of mh_search_first_batch_ex(flags)
 * over reqs[0..n) (the plan is mh_batch_plan_ex's).  launch == -1: the pass's generic launch
 * (batch_scan_first), out[b] the partial slot of the tile workgroup b runs, a permutation of the
 * slots of the pass's generic entries; with flags == 0 that is mh_first_batch_order.  launch >= 0:
 * that batch_first launch of the pass (mh_batch_piece::launch), out[b] the partial slot of the chunk
 * workgroup b runs, a permutation of the slots of that launch's pieces.  Rank-major unless
 * MINEHIP_FIRST_BATCH_ORDER=request.  Returns the launch's workgroup count (0 for the generic launch
 * of a pass without a generic entry), cap + 1 when there are more than cap (the first cap written),
 * the MH_E* of the first request mh_search would refuse, or MH_EINVAL for an unknown flag bit or a
 * pass or launch the plan lacks. */
int64_t mh_first_batch_order_ex(const mh_request *reqs, size_t n, uint32_t flags, int32_t pass, int32_t launch,
                                uint32_t *out, int64_t cap);

/* One request of mh_search_hits_batch's schedule. */
typedef struct mh_hits_region {
    uint64_t req;          /* index into reqs */
    int32_t kind, pass;    /* 0 fused, 1 fallback; its pass, exactly mh_batch_plan's (fallback: -1) */
    int32_t window, reserved; /* fused: how many drains precede its pass; fallback: -1 */
    uint64_t offset, slots;   /* fused: its region of the device hit buffer; fallback: 0, 0 */
} mh_hits_region; /* 40 bytes */

/* Host only: how mh_search_hits_batch would run reqs[0..n): one item per request, in request
 * order.  The regions of one window are disjoint, in order and inside the device hit buffer
 * (honours MINEHIP_HITS_SLOTS and MINEHIP_BATCH_SLOTS).  Returns the item count, cap + 1 when
 * there are more than cap (the first cap written, as mh_plan), or the MH_E* of the first request
 * mh_search_hits_batch would refuse.  n == 0 returns 0. */
int64_t mh_hits_batch_regions(const mh_hits_request *reqs, size_t n, mh_hits_region *out, int64_t cap);

/* mh_hits_batch_regions for mh_search_hits_batch_ex(flags): flags == 0 is mh_hits_batch_regions; an
 * unknown flag bit returns MH_EINVAL.  With MH_BATCH_FUSE_FAST kind and pass follow
 * mh_batch_plan_ex: kind 0 for a fused request (its pieces there have kind 0 or 2) with the pass
 * of its pieces, kind 1 for a fallback. */
int64_t mh_hits_batch_regions_ex(const mh_hits_request *reqs, size_t n, uint32_t flags, mh_hits_region *out,
                                 int64_t cap);

/* Host only: how mh_search_first_hits_batch(flags) would run reqs[0..n): mh_hits_batch_regions_ex's
 * items with the regions of that call -- a request of k wants min(its nonce count, max(4 k, 256))
 * entries and gets min(that, what the window has left).  kind and pass follow mh_batch_plan_ex(flags).
 * Honours MINEHIP_HITS_SLOTS and MINEHIP_BATCH_SLOTS.  The return values are mh_hits_batch_regions';
 * the first request the call would refuse (k == 0 included) gives its MH_E*. */
int64_t mh_first_hits_batch_regions(const mh_first_hits_request *reqs, size_t n, uint32_t flags,
                                    mh_hits_region *out, int64_t cap);

/* One span of mh_search_multi's adaptive split (chunk == 0), ABI 4. */
typedef struct mh_span {
    uint64_t lower, upper; /* inclusive */
    int32_t worker;        /* head shard: index into devs; tail chunk: -1 */
    int32_t kind;          /* 0 head shard, 1 tail chunk (handed to the first free worker) */
    double cost;           /* relative cost (issue slots): shards ~ weights */
} mh_span;

/* Host only: how mh_search_multi(chunk = 0) would split [lower, upper] over
 * ndev workers whose rates are in proportion to weights[0..ndev) (> 0; NULL =
 * equal).  Head shards (worker order, empty ones omitted), then tail chunks
 * (nonce order); together they tile [lower, upper] exactly once.  Returns the
 * span count (cap + 1 style truncation as mh_plan) or MH_E*. */
int64_t mh_multi_plan(const uint8_t *msg, size_t len, uint64_t lower, uint64_t upper, const double *weights,
                      int ndev, mh_span *out, int64_t cap);

/* The per-process rate table mh_search_multi sizes its shards by: out[i] =
 * devs[i]'s measured rate in cost units per ns (0 = not measured yet). */
int mh_multi_rates(const int *devs, int ndev, double *out);

#ifdef __cplusplus
}
#endif

#endif /* MINEHIP_H */

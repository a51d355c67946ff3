// batch.cpp -- the batched entry points of libminehip.so's C-ABI (declared in include/minehip.h):
// mh_search_batch[_ex], mh_search_first_batch[_ex], mh_search_first_batch_stop,
// mh_search_hits_batch[_ex], mh_search_first_hits_batch, their host-only plan probes,
// mh_miner_handle, mh_miner_handle_batch[_ex] and mh_hash_batch.
//
// A batch fuses its small requests into passes on the device's one stream: per pass one H2D copy
// of its tables, the scan of the generic entries, one fast launch per layout present, a merge and
// one D2H copy of its results, with no synchronise until a buffer is full (a drain).  The passes
// of the entry points differ in their tables, kernels and results; what they share -- the fused
// call's start and end, the profile's bookkeeping of a launch, the checks -- is here once.
#include <functional>

#include "host_ctx.hpp"
#include "msgcodec.hpp"

using namespace mh::host;

namespace {

using mh::Partial;

// ---- batched search ----

//   MINEHIP_BATCH_SLOTS    partial slots (tiles) one pass of mh_search_batch may use
//                          (1..kMaxBlocksPerLaunch, the default): a lower value makes small
//                          batches run several passes and send their larger requests to the
//                          fallback path (tests; the results never depend on it)
uint32_t batch_slots() {
    if (const char* e = getenv("MINEHIP_BATCH_SLOTS")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v >= 1 && v <= mh::kMaxBlocksPerLaunch) return (uint32_t)v;
    }
    return mh::kMaxBlocksPerLaunch;
}

inline size_t align16(size_t x) { return (x + 15u) & ~(size_t)15u; }

// ---- what the batched entry points share ----

// The start of every fused call: the device's context, its lock held until the session ends, the
// context initialised, the device current, then the call's own buffers (`inits`, in their order).
struct BatchSession {
    DevCtx* c = nullptr;
    std::unique_lock<std::mutex> lk;
    int open(int dev, std::initializer_list<int (*)(DevCtx*)> inits) {
        MH_TRY(get_ctx(dev, &c));
        lk = std::unique_lock<std::mutex>(c->mu);
        MH_TRY(init_locked(c, dev));
        MH_HIP(hipSetDevice(dev));
        for (const auto init : inits) MH_TRY(init(c));
        return MH_OK;
    }
};

// The end of every fused call: the last drain, and after a failure nothing of the call stays in flight.
template <class Drain>
int finish_fused(DevCtx* c, int rc, Drain drain) {
    if (!rc) rc = drain();
    if (rc) (void)hipStreamSynchronize(c->stream);
    return rc;
}

// What every drain starts with: the one synchronise, and the timings of the launches it waited for.
int sync_and_harvest(DevCtx* c) {
    MH_HIP(hipStreamSynchronize(c->stream));
    return c->prof ? harvest_locked(c) : MH_OK;
}

// The event pool cannot take `pairs` more launches: the pass drains first (a drain harvests the pool).
bool prof_needs_drain(const DevCtx* c, int pairs) { return c->prof && c->used + pairs > kEventPairs; }

// A launch on c->stream as the profile sees it: between prof_begin and prof_end_generic (a
// batch_scan* launch: the generic class, mh_profile_read out[4], out[5], with the pass's planned
// nonces) or prof_end_fast (a fused fast launch, below).  *tm stays null while the profile is off.
int prof_begin(DevCtx* c, int kind, int var, Timed** tm) {
    if (!c->prof) return MH_OK;
    *tm = &c->pool[(size_t)c->used++];
    (*tm)->kind = kind;
    (*tm)->var = var;
    MH_HIP(hipEventRecord((*tm)->start, c->stream));
    return MH_OK;
}

int prof_end_generic(DevCtx* c, Timed* tm, uint64_t nonces) {
    if (!tm) return MH_OK;
    MH_HIP(hipEventRecord(tm->stop, c->stream));
    c->cnt[4] += nonces;
    return MH_OK;
}

// The fast class: per piece of the launch its nonces, ops and slots under its (J, MODE, L); the
// launch and its time under the (J, MODE, L) of its first, longest-lane piece (prof_begin's var).
int prof_end_fast(DevCtx* c, Timed* tm, const mh::BatchFastLaunch& l, const mh::BatchFastTables& f,
                  const std::vector<mh::BatchPiece>& pieces) {
    if (!tm) return MH_OK;
    MH_HIP(hipEventRecord(tm->stop, c->stream));
    c->cnt[0] += 1;
    c->var[tm->var].launches += 1;
    for (uint32_t k = l.item0; k < l.item0 + l.items; ++k) {
        const mh::BatchPiece& p = pieces[f.piece[k]];
        c->cnt[1] += p.count;
        c->cnt[3] += p.count * (uint64_t)p.ops;
        c->cnt[6] += p.count * (uint64_t)p.nslots;
        VarStat& v = c->var[var_index(p.J, p.mode, p.L)];
        v.nonces += p.count;
        v.ops += p.count * (uint64_t)p.ops;
        v.slots += p.count * (uint64_t)p.nslots;
    }
    return MH_OK;
}

// The fast launches of a pass, one per layout in the plan's order: launch(l) enqueues launch l's
// kernel on c->stream and returns an MH_* code.
template <class Launch>
int run_fast_launches(DevCtx* c, const mh::BatchFastTables& f, const std::vector<mh::BatchPiece>& pieces,
                      Launch launch) {
    for (const mh::BatchFastLaunch& l : f.launches) {
        Timed* tm = nullptr;
        MH_TRY(prof_begin(c, 0, var_index(l.J, l.mode, (int)f.items[l.item0].args.L), &tm));
        MH_TRY(launch(l));
        MH_TRY(prof_end_fast(c, tm, l, f, pieces));
    }
    return MH_OK;
}

// The Early pieces among a pass's fast items, re-checked where they reach the kernel (early_piece_ok).
int check_early_items(const mh::BatchFastTables& f, const std::vector<mh::BatchPiece>& pieces) {
    for (size_t k = 0; k < f.items.size(); ++k) {
        const mh::BatchPiece& p = pieces[f.piece[k]];
        if (f.items[k].args.mode >= mh::kModeOneEarly && !early_piece_ok(f.items[k].args, p.J))
            return fail(MH_EINTERNAL, "internal: bad Early piece (an enumerated digit outside word J)");
    }
    return MH_OK;
}

// The fused passes of a plan: one more than the last pass of an item or piece that is no fallback.
int batch_passes(const std::vector<mh::BatchItem>& items) {
    int passes = 0;
    for (const mh::BatchItem& it : items)
        if (it.kind == 0) passes = std::max(passes, it.pass + 1);
    return passes;
}
int batch_passes(const std::vector<mh::BatchPiece>& pieces) {
    int passes = 0;
    for (const mh::BatchPiece& p : pieces)
        if (p.kind != 1) passes = std::max(passes, p.pass + 1);
    return passes;
}

// The per-request checks of a batch: a status for every request, and the valid ones as
// BatchRequests.  extra(request): the entry point's own check, made between the message's and the
// range's; the first check that fails decides the request's status and the message.
template <class Req, class Extra>
void batch_requests(const Req* reqs, size_t n, std::vector<int>* status, std::vector<mh::BatchRequest>* valid,
                    Extra extra) {
    status->assign(n, MH_OK);
    valid->clear();
    valid->reserve(n);
    for (size_t i = 0; i < n; ++i) {
        int st = check_common(reqs[i].msg, reqs[i].len);
        if (!st) st = extra(reqs[i]);
        if (!st && reqs[i].lower > reqs[i].upper) st = fail(MH_ERANGE, "lower > upper");
        (*status)[i] = st;
        if (st) continue;
        valid->emplace_back();
        mh::BatchRequest& r = valid->back();
        mh::absorb_prefix(reqs[i].msg, reqs[i].len, &r.pre);
        r.lower = reqs[i].lower;
        r.upper = reqs[i].upper;
        r.id = i;
    }
}
template <class Req>
void batch_requests(const Req* reqs, size_t n, std::vector<int>* status, std::vector<mh::BatchRequest>* valid) {
    batch_requests(reqs, n, status, valid, [](const Req&) { return MH_OK; });
}

// The plan probes refuse a whole call by the first request a search would refuse: its status, and
// the message of the check that set it.
const char* first_refusal(int status) {
    return status == MH_ERANGE ? "lower > upper" : status == MH_ETOOLONG ? "message longer than MH_MAX_MSG_LEN" : "msg is NULL";
}
int refuse_first(const std::vector<int>& status) {
    for (const int st : status)
        if (st) return fail(st, first_refusal(st));
    return MH_OK;
}

int batch_init_locked(DevCtx* c) {
    if (!c->d_btab) MH_HIP(hipMalloc(&c->d_btab, kBatchTableBytes));
    if (!c->h_btab) MH_HIP(hipHostMalloc(&c->h_btab, kBatchTableBytes, hipHostMallocDefault));
    if (!c->d_bres) MH_HIP(hipMalloc(&c->d_bres, sizeof(Partial) * kBatchResults));
    if (!c->h_bres) MH_HIP(hipHostMalloc(&c->h_bres, sizeof(Partial) * kBatchResults, hipHostMallocDefault));
    return MH_OK;
}

// The results of the passes enqueued since the last drain, waiting in h_bres for the synchronise.
struct BatchPending {
    std::vector<size_t> req_idx;  // in h_bres order
    size_t toff = 0;              // table bytes in use
};

int batch_drain(DevCtx* c, const mh::BatchRequest* reqs, BatchPending* pend, mh_result* out) {
    MH_TRY(sync_and_harvest(c));
    for (size_t k = 0; k < pend->req_idx.size(); ++k) {
        mh_result& r = out[reqs[pend->req_idx[k]].id];
        r.hash = c->h_bres[k].hash;
        r.nonce = c->h_bres[k].nonce;
    }
    pend->req_idx.clear();
    pend->toff = 0;
    return MH_OK;
}

// One pass on c->stream, of mh_search_batch and of mh_search_batch_ex: one H2D copy of all its tables
// from the pinned staging (entries, segments, per-tile entry, fast items, per-chunk item), the scan
// of the generic entries, one batch_fast<J, MODE> launch per layout present, merge_segments, one D2H
// copy of its results.  No synchronise: the tables and results of successive passes sit behind one
// another until a buffer is full.  A pass without a fast piece (f.items empty: every pass of
// mh_search_batch, where slot0 == tile0 throughout) is checked by batch_tables_ok, scans with
// batch_scan and has the image of its three tables alone (align16(0) == 0); one with fast pieces
// is checked by batch_tables_ex_ok and scans with batch_scan_slots.  The scan counts in the generic
// class of the profile (prof_end_generic), the fast launches in the fast class (prof_end_fast).
int batch_run_pass(DevCtx* c, const mh::BatchRequest* reqs, const std::vector<mh::BatchPiece>& pieces,
                   const mh::BatchTables& t, const mh::BatchFastTables& f, uint32_t slot_cap, BatchPending* pend,
                   mh_result* out) {
    const bool fast = !f.items.empty();
    if (!(fast ? mh::batch_tables_ex_ok(t, f, slot_cap) : mh::batch_tables_ok(t, slot_cap)))
        return fail(MH_EINTERNAL, "internal: bad batch tables");
    MH_TRY(check_early_items(f, pieces));
    const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
    const size_t ni = f.items.size(), chunks = f.chunk_item.size();
    const size_t o_seg = align16(ne * sizeof(mh::BatchEntry)), o_tile = o_seg + align16((nreq + 1u) * sizeof(uint32_t));
    const size_t o_item = o_tile + align16(tiles * sizeof(uint32_t)), o_chunk = o_item + ni * sizeof(mh::BatchFastItem);
    const size_t bytes = o_chunk + align16(chunks * sizeof(uint32_t));
    if (bytes > kBatchTableBytes || nreq > kBatchResults) return fail(MH_EINTERNAL, "internal: batch pass too large");
    if (pend->toff + bytes > kBatchTableBytes || pend->req_idx.size() + nreq > kBatchResults ||
        prof_needs_drain(c, 1 + (int)f.launches.size()))
        MH_TRY(batch_drain(c, reqs, pend, out));
    uint8_t* h = c->h_btab + pend->toff;
    uint8_t* d = c->d_btab + pend->toff;
    memcpy(h, t.entries.data(), ne * sizeof(mh::BatchEntry));
    memcpy(h + o_seg, t.seg.data(), (nreq + 1u) * sizeof(uint32_t));
    memcpy(h + o_tile, t.tile_entry.data(), tiles * sizeof(uint32_t));
    memcpy(h + o_item, f.items.data(), ni * sizeof(mh::BatchFastItem));
    memcpy(h + o_chunk, f.chunk_item.data(), chunks * sizeof(uint32_t));
#ifdef MH_DEV_HOOKS
    for (size_t i = 0; i < ne; ++i) ((mh::BatchEntry*)h)[i].g.pad = c->keep;
    for (size_t i = 0; i < ni; ++i) ((mh::BatchFastItem*)(h + o_item))[i].args.pad_ = c->keep;
#endif
    MH_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    if (tiles) {  // always, without a fast piece (batch_tables_ok)
        Timed* tm = nullptr;
        MH_TRY(prof_begin(c, 1, 0, &tm));
        MH_HIP((fast ? mh::launch_batch_scan_slots : mh::launch_batch_scan)(
            (const mh::BatchEntry*)d, (const uint32_t*)(d + o_tile), c->d_partials, (uint32_t)tiles, c->stream));
        MH_TRY(prof_end_generic(c, tm, t.nonces));
    }
    MH_TRY(run_fast_launches(c, f, pieces, [&](const mh::BatchFastLaunch& l) {
        MH_HIP(mh::launch_batch_fast(c->dev, l.J, l.mode, (const mh::BatchFastItem*)(d + o_item),
                                     (const uint32_t*)(d + o_chunk) + l.chunk0, c->d_partials, l.chunks, c->stream));
        return MH_OK;
    }));
    const size_t roff = pend->req_idx.size();
    MH_HIP(mh::launch_merge_segments(c->d_partials, (const uint32_t*)(d + o_seg), c->d_bres + roff, (uint32_t)nreq,
                                     c->stream));
    MH_HIP(hipMemcpyAsync(c->h_bres + roff, c->d_bres + roff, nreq * sizeof(Partial), hipMemcpyDeviceToHost, c->stream));
    pend->req_idx.insert(pend->req_idx.end(), t.req_idx.begin(), t.req_idx.end());
    pend->toff += bytes;
    return MH_OK;
}

// The fused passes of a batch, under the device's lock.
int batch_run_fused(int dev, const mh::BatchRequest* reqs, const std::vector<mh::BatchItem>& items, int passes,
                    uint32_t slot_cap, mh_result* out) {
    BatchSession s;
    MH_TRY(s.open(dev, {batch_init_locked}));
    DevCtx* c = s.c;
#ifdef MH_DEV_HOOKS
    MH_TRY(read_hash_keep(c));
    MH_TRY(read_hash_xor(c));
#endif
    BatchPending pend;
    mh::BatchTables t;
    const mh::BatchFastTables no_fast;  // mh_search_batch fuses no fast piece
    const std::vector<mh::BatchPiece> no_pieces;
    int rc = MH_OK;
    for (int p = 0; p < passes && !rc; ++p) {
        mh::build_batch_tables(reqs, items, p, &t);
        rc = batch_run_pass(c, reqs, no_pieces, t, no_fast, slot_cap, &pend, out);
    }
    return finish_fused(c, rc, [&] { return batch_drain(c, reqs, &pend, out); });
}

// ---- batched search with fused fast pieces (mh_search_batch_ex) ----

//   MINEHIP_BATCH_FAST_MAX    most nonces of a request mh_search_batch_ex(MH_BATCH_FUSE_FAST) fuses
//                             (default kBatchFastMaxNonces; 0: no request with a fast piece is fused)
//   MINEHIP_BATCH_FAST_LANES  "shared": the batch-aware lane rule (plan.hpp batch_min_lanes), which the
//                             measurement did not favour; otherwise every request
//                             keeps the lanes of its own mh_search plan (default)
// (tests and tools/batch_fast_latency.py; the results never depend on them)
uint64_t batch_fast_max() {
    if (const char* e = getenv("MINEHIP_BATCH_FAST_MAX"))
        if (*e) return strtoull(e, nullptr, 10);
    return mh::kBatchFastMaxNonces;
}
bool batch_fast_shared_lanes() {
    const char* e = getenv("MINEHIP_BATCH_FAST_LANES");
    return e && strcmp(e, "shared") == 0;
}

// The fused passes of mh_search_batch_ex(MH_BATCH_FUSE_FAST), under the device's lock.
int batch_run_fused_ex(int dev, const mh::BatchRequest* reqs, const std::vector<mh::BatchPiece>& pieces,
                       const std::vector<mh::FastArgs>& args, int passes, uint32_t slot_cap, mh_result* out) {
    BatchSession s;
    MH_TRY(s.open(dev, {batch_init_locked}));
    DevCtx* c = s.c;
#ifdef MH_DEV_HOOKS
    MH_TRY(read_hash_keep(c));
    MH_TRY(read_hash_xor(c));
    const bool any_fast = std::any_of(pieces.begin(), pieces.end(), [](const mh::BatchPiece& p) { return p.kind == 2; });
    if (any_fast && (c->keep || c->xor_on)) {  // the hooks of the batch code object, as enqueue_piece's of the product's
        uint64_t x = 0;
        if (const char* e = getenv("MINEHIP_DEV_HASH_XOR")) x = strtoull(e, nullptr, 16);  // read_hash_xor accepted it
        bool keep_ok = false, xor_ok = false;
        MH_HIP(mh::batch_fast_hooks(c->dev, x, c->stream, &keep_ok, &xor_ok));
        if (c->keep && !keep_ok)
            return fail(MH_EINVAL, "MINEHIP_DEV_HASH_KEEP is set but the batch code object is not the coarse-hash "
                                   "variant (MINEHIP_DEV_BATCH_CODE_OBJECT=build/fast_batch_keep.hsaco)");
        if (c->xor_on && !xor_ok)
            return fail(MH_EINVAL, "MINEHIP_DEV_HASH_XOR is set but the batch code object has no mh_dev_hash_xor "
                                   "(MINEHIP_DEV_BATCH_CODE_OBJECT=build/fast_batch_keep.hsaco)");
    } else if (any_fast) {  // off: a variant code object's word may still hold an earlier call's constant
        bool keep_ok = false, xor_ok = false;
        if (getenv("MINEHIP_DEV_BATCH_CODE_OBJECT")) MH_HIP(mh::batch_fast_hooks(c->dev, 0, c->stream, &keep_ok, &xor_ok));
    }
#endif
    BatchPending pend;
    mh::BatchTables t;
    mh::BatchFastTables f;
    int rc = MH_OK;
    for (int p = 0; p < passes && !rc; ++p) {
        mh::build_batch_tables_ex(reqs, pieces, args, p, &t, &f);
        rc = batch_run_pass(c, reqs, pieces, t, f, slot_cap, &pend, out);
    }
    return finish_fused(c, rc, [&] { return batch_drain(c, reqs, &pend, out); });
}

// A fallback request's search: (request, hash, nonce) -> MH_*.
using BatchFallback = std::function<int(const mh::BatchRequest&, uint64_t*, uint64_t*)>;

int search_batch_impl(int dev, const mh_request* reqs, size_t n, mh_result* out, const BatchFallback& fallback) {
    std::vector<int> status;
    std::vector<mh::BatchRequest> valid;
    batch_requests(reqs, n, &status, &valid);
    for (size_t i = 0; i < n; ++i) out[i] = mh_result{status[i], 0, 0, 0};
    if (valid.empty()) return MH_OK;
    g_err.clear();
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchItem> items;
    mh::plan_batch(valid.data(), valid.size(), plan_opts(), slot_cap, &items);
    const int passes = batch_passes(items);
    if (passes) MH_TRY(batch_run_fused(dev, valid.data(), items, passes, slot_cap, out));
    for (const mh::BatchItem& it : items) {
        if (it.kind != 1) continue;
        const mh::BatchRequest& r = valid[it.idx];
        const int rc = fallback(r, &out[r.id].hash, &out[r.id].nonce);
        if (rc) return rc;
    }
    return MH_OK;
}

// ---- batched first-hit search ----

//   MINEHIP_FIRST_BATCH_ORDER  "request": workgroup b of batch_scan_first runs tile b (the identity,
//                              request-major order) instead of the rank-major order; read per
//                              call (measurement and tests; found, hash and nonce never depend on it)
bool first_batch_rank_major() {
    const char* e = getenv("MINEHIP_FIRST_BATCH_ORDER");
    return !(e && strcmp(e, "request") == 0);
}

int first_batch_init_locked(DevCtx* c) {
    if (!c->d_fres) MH_HIP(hipMalloc(&c->d_fres, sizeof(mh::BatchFirstResult) * kBatchResults));
    if (!c->h_fres)
        MH_HIP(hipHostMalloc(&c->h_fres, sizeof(mh::BatchFirstResult) * kBatchResults, hipHostMallocDefault));
    return MH_OK;
}

void put_first_result(mh_first_result* r, uint64_t hash, uint64_t nonce, uint64_t scanned, uint64_t target) {
    r->hash = hash;
    r->nonce = nonce;
    r->scanned = scanned;
    r->found = hash <= target ? 1 : 0;  // without a qualifying nonce the minimum itself is > target
}

int first_batch_drain(DevCtx* c, const mh::BatchRequest* reqs, const mh_first_request* src, BatchPending* pend,
                      mh_first_result* out) {
    MH_TRY(sync_and_harvest(c));
    for (size_t k = 0; k < pend->req_idx.size(); ++k) {
        const size_t id = reqs[pend->req_idx[k]].id;
        put_first_result(&out[id], c->h_fres[k].hash, c->h_fres[k].nonce, c->h_fres[k].scanned, src[id].target);
    }
    pend->req_idx.clear();
    pend->toff = 0;
    return MH_OK;
}

// batch_run_pass over the first-hit kernels: the pass's one H2D copy also carries the per-entry
// request index, the dispatch order and the requests' device words with their initial values
// (target; first = all ones; scanned = 0), so there is no memset and no fill kernel; then
// batch_scan_first, merge_segments_first and one D2H copy of {hash, nonce, scanned} per request.
int first_batch_run_pass(DevCtx* c, const mh::BatchRequest* reqs, const mh_first_request* src, const mh::BatchTables& t,
                         uint32_t slot_cap, bool rank_major, BatchPending* pend, mh_first_result* out) {
    if (!mh::batch_tables_ok(t, slot_cap)) return fail(MH_EINTERNAL, "internal: bad batch tables");
    mh::FirstBatchTables ft;
    mh::build_first_batch_tables(t, rank_major, &ft);
    if (!mh::first_batch_tables_ok(t, ft)) return fail(MH_EINTERNAL, "internal: bad first-hit batch tables");
    const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
    const size_t o_seg = align16(ne * sizeof(mh::BatchEntry)), o_tile = o_seg + align16((nreq + 1u) * sizeof(uint32_t));
    const size_t o_ereq = o_tile + align16(tiles * sizeof(uint32_t)), o_order = o_ereq + align16(ne * sizeof(uint32_t));
    const size_t o_words = o_order + align16(tiles * sizeof(uint32_t));
    const size_t bytes = o_words + align16(nreq * sizeof(mh::BatchFirstWords));
    if (bytes > kBatchTableBytes || nreq > kBatchResults) return fail(MH_EINTERNAL, "internal: batch pass too large");
    if (pend->toff + bytes > kBatchTableBytes || pend->req_idx.size() + nreq > kBatchResults || prof_needs_drain(c, 1))
        MH_TRY(first_batch_drain(c, reqs, src, pend, out));
    uint8_t* h = c->h_btab + pend->toff;
    uint8_t* d = c->d_btab + pend->toff;
    memcpy(h, t.entries.data(), ne * sizeof(mh::BatchEntry));
    memcpy(h + o_seg, t.seg.data(), (nreq + 1u) * sizeof(uint32_t));
    memcpy(h + o_tile, t.tile_entry.data(), tiles * sizeof(uint32_t));
    memcpy(h + o_ereq, ft.entry_req.data(), ne * sizeof(uint32_t));
    memcpy(h + o_order, ft.order.data(), tiles * sizeof(uint32_t));
    mh::BatchFirstWords* hw = (mh::BatchFirstWords*)(h + o_words);
    for (size_t r = 0; r < nreq; ++r) hw[r] = mh::BatchFirstWords{src[reqs[t.req_idx[r]].id].target, ~0ull, 0ull};
    MH_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    Timed* tm = nullptr;
    MH_TRY(prof_begin(c, 1, 0, &tm));
    MH_HIP(mh::launch_batch_scan_first((const mh::BatchEntry*)d, (const uint32_t*)(d + o_tile),
                                       (const uint32_t*)(d + o_ereq), (const uint32_t*)(d + o_order),
                                       (mh::BatchFirstWords*)(d + o_words), c->d_partials, (uint32_t)tiles, c->stream));
    MH_TRY(prof_end_generic(c, tm, t.nonces));
    const size_t roff = pend->req_idx.size();
    MH_HIP(mh::launch_merge_segments_first(c->d_partials, (const uint32_t*)(d + o_seg), (const mh::BatchEntry*)d,
                                           (const uint32_t*)(d + o_tile), (const mh::BatchFirstWords*)(d + o_words),
                                           c->d_fres + roff, (uint32_t)nreq, c->stream));
    MH_HIP(hipMemcpyAsync(c->h_fres + roff, c->d_fres + roff, nreq * sizeof(mh::BatchFirstResult), hipMemcpyDeviceToHost,
                          c->stream));
    pend->req_idx.insert(pend->req_idx.end(), t.req_idx.begin(), t.req_idx.end());
    pend->toff += bytes;
    return MH_OK;
}

// The fused passes of a first-hit batch, under the device's lock.
int first_batch_run_fused(int dev, const mh::BatchRequest* reqs, const mh_first_request* src,
                          const std::vector<mh::BatchItem>& items, int passes, uint32_t slot_cap, mh_first_result* out) {
    BatchSession s;
    MH_TRY(s.open(dev, {batch_init_locked, first_batch_init_locked}));
    DevCtx* c = s.c;
    const bool rank_major = first_batch_rank_major();
    BatchPending pend;
    mh::BatchTables t;
    int rc = MH_OK;
    for (int p = 0; p < passes && !rc; ++p) {
        mh::build_batch_tables(reqs, items, p, &t);
        rc = first_batch_run_pass(c, reqs, src, t, slot_cap, rank_major, &pend, out);
    }
    return finish_fused(c, rc, [&] { return first_batch_drain(c, reqs, src, &pend, out); });
}

// ---- batched first-hit search with fused fast pieces (mh_search_first_batch_ex) ----

int first_batch_fast_init_locked(DevCtx* c) {
    if (!c->d_ftab) MH_HIP(hipMalloc(&c->d_ftab, kFirstBatchFastTableBytes));
    if (!c->h_ftab) MH_HIP(hipHostMalloc(&c->h_ftab, kFirstBatchFastTableBytes, hipHostMallocDefault));
    return MH_OK;
}

// first_batch_run_pass for a pass that holds fast pieces: one H2D copy of all its tables -- entries,
// segments, per-tile entry, per-entry request, tile order, the requests' words with their initial
// values, a GenArgs per request, the fast items (each with its request's target and the device
// addresses of its request's words), per-chunk item and chunk order -- then, on the one stream,
// batch_scan_first_slots for the generic entries, one batch_first<J, MODE> launch per layout in the
// plan's order, merge_segments_first_ex and one D2H copy of {hash, nonce, scanned} per request.
// *toff: bytes of the d_ftab / h_ftab buffer in use by the passes in flight.  The fast launches
// count in the fast class of the profile as batch_run_pass_ex counts them, each piece with its
// planned nonces, skipped chunks included (mh_search_first's rule for its first_scan launches).
// stop (mh_search_first_batch_stop): the fast launches are batch_stop<J, MODE>'s, over the same tables
// in the same order; nothing else of the pass differs.
int first_batch_run_pass_ex(DevCtx* c, const mh::BatchRequest* reqs, const mh_first_request* src,
                            const std::vector<mh::BatchPiece>& pieces, const mh::BatchTables& t,
                            const mh::BatchFastTables& f, uint32_t slot_cap, bool rank_major, bool stop,
                            BatchPending* pend, size_t* toff, mh_first_result* out) {
    mh::FirstBatchFastTables x;
    mh::build_first_batch_tables_ex(t, f, rank_major, &x);
    if (!mh::first_batch_tables_ex_ok(t, f, x, slot_cap)) return fail(MH_EINTERNAL, "internal: bad first-hit batch tables");
    MH_TRY(check_early_items(f, pieces));
    const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
    const size_t ni = f.items.size(), chunks = f.chunk_item.size();
    const size_t o_seg = align16(ne * sizeof(mh::BatchEntry)), o_tile = o_seg + align16((nreq + 1u) * sizeof(uint32_t));
    const size_t o_ereq = o_tile + align16(tiles * sizeof(uint32_t)), o_order = o_ereq + align16(ne * sizeof(uint32_t));
    const size_t o_words = o_order + align16(tiles * sizeof(uint32_t));
    const size_t o_gen = o_words + align16(nreq * sizeof(mh::BatchFirstWords));
    const size_t o_item = o_gen + nreq * sizeof(mh::GenArgs), o_chunk = o_item + ni * sizeof(mh::BatchFirstItem);
    const size_t o_corder = o_chunk + align16(chunks * sizeof(uint32_t));
    const size_t bytes = o_corder + align16(chunks * sizeof(uint32_t));
    static_assert(sizeof(mh::GenArgs) % 16 == 0 && sizeof(mh::BatchFirstItem) % 16 == 0, "tables stay 16-byte aligned");
    if (bytes > kFirstBatchFastTableBytes || nreq > kBatchResults)
        return fail(MH_EINTERNAL, "internal: batch pass too large");
    if (*toff + bytes > kFirstBatchFastTableBytes || pend->req_idx.size() + nreq > kBatchResults ||
        prof_needs_drain(c, 1 + (int)f.launches.size())) {
        MH_TRY(first_batch_drain(c, reqs, src, pend, out));
        *toff = 0;
    }
    uint8_t* h = c->h_ftab + *toff;
    uint8_t* d = c->d_ftab + *toff;
    memcpy(h, t.entries.data(), ne * sizeof(mh::BatchEntry));
    memcpy(h + o_seg, t.seg.data(), (nreq + 1u) * sizeof(uint32_t));
    memcpy(h + o_tile, t.tile_entry.data(), tiles * sizeof(uint32_t));
    memcpy(h + o_ereq, x.entry_req.data(), ne * sizeof(uint32_t));
    memcpy(h + o_order, x.tile_order.data(), tiles * sizeof(uint32_t));
    mh::BatchFirstWords* hw = (mh::BatchFirstWords*)(h + o_words);
    mh::BatchFirstWords* dw = (mh::BatchFirstWords*)(d + o_words);
    mh::GenArgs* hg = (mh::GenArgs*)(h + o_gen);
    for (size_t r = 0; r < nreq; ++r) {
        hw[r] = mh::BatchFirstWords{src[reqs[t.req_idx[r]].id].target, ~0ull, 0ull};
        mh::make_gen_args(reqs[t.req_idx[r]].pre, &hg[r]);
    }
    mh::BatchFirstItem* hi = (mh::BatchFirstItem*)(h + o_item);
    for (size_t k = 0; k < ni; ++k) {
        const uint32_t r = x.item_req[k];  // < nreq, and the request owns the item's slots (checked above)
        mh::BatchFirstItem it;
        memset(&it, 0, sizeof it);
        it.args = f.items[k].args;
        it.unused = nullptr;
        it.f = mh::FirstArgs{hw[r].target, &dw[r].first, &dw[r].scanned};
        it.chunk0 = f.items[k].chunk0;
        it.slot0 = f.items[k].slot0;
        hi[k] = it;
    }
    memcpy(h + o_chunk, f.chunk_item.data(), chunks * sizeof(uint32_t));
    memcpy(h + o_corder, x.chunk_order.data(), chunks * sizeof(uint32_t));
    MH_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    if (tiles) {
        Timed* tm = nullptr;
        MH_TRY(prof_begin(c, 1, 0, &tm));
        MH_HIP(mh::launch_batch_scan_first_slots((const mh::BatchEntry*)d, (const uint32_t*)(d + o_tile),
                                                 (const uint32_t*)(d + o_ereq), (const uint32_t*)(d + o_order), dw,
                                                 c->d_partials, (uint32_t)tiles, c->stream));
        MH_TRY(prof_end_generic(c, tm, t.nonces));
    }
    MH_TRY(run_fast_launches(c, f, pieces, [&](const mh::BatchFastLaunch& l) {
        MH_HIP((stop ? mh::launch_batch_stop : mh::launch_batch_first)(
            c->dev, l.J, l.mode, (const mh::BatchFirstItem*)(d + o_item), (const uint32_t*)(d + o_chunk) + l.chunk0,
            (const uint32_t*)(d + o_corder) + l.chunk0, c->d_partials, l.chunks, c->stream));
        return MH_OK;
    }));
    const size_t roff = pend->req_idx.size();
    MH_HIP(mh::launch_merge_segments_first_ex(c->d_partials, (const uint32_t*)(d + o_seg), (const mh::GenArgs*)(d + o_gen),
                                              dw, c->d_fres + roff, (uint32_t)nreq, c->stream));
    MH_HIP(hipMemcpyAsync(c->h_fres + roff, c->d_fres + roff, nreq * sizeof(mh::BatchFirstResult), hipMemcpyDeviceToHost,
                          c->stream));
    pend->req_idx.insert(pend->req_idx.end(), t.req_idx.begin(), t.req_idx.end());
    *toff += bytes;
    return MH_OK;
}

// The fused passes of mh_search_first_batch_ex(MH_BATCH_FUSE_FAST), under the device's lock (stop: of
// mh_search_first_batch_stop, first_batch_run_pass_ex).
int first_batch_run_fused_ex(int dev, const mh::BatchRequest* reqs, const mh_first_request* src,
                             const std::vector<mh::BatchPiece>& pieces, const std::vector<mh::FastArgs>& args, int passes,
                             uint32_t slot_cap, bool stop, mh_first_result* out) {
    BatchSession s;
    MH_TRY(s.open(dev, {batch_init_locked, first_batch_init_locked}));
    DevCtx* c = s.c;
    const bool rank_major = first_batch_rank_major();
    BatchPending pend;
    size_t toff_fast = 0;
    mh::BatchTables t;
    mh::BatchFastTables f;
    int rc = MH_OK;
    for (int p = 0; p < passes && !rc; ++p) {
        mh::build_batch_tables_ex(reqs, pieces, args, p, &t, &f);
        if (f.items.empty()) {  // mh_search_first_batch's own pass (slot0 == tile0 throughout)
            rc = first_batch_run_pass(c, reqs, src, t, slot_cap, rank_major, &pend, out);
        } else {
            rc = first_batch_fast_init_locked(c);
            if (!rc) rc = first_batch_run_pass_ex(c, reqs, src, pieces, t, f, slot_cap, rank_major, stop, &pend, &toff_fast, out);
        }
    }
    return finish_fused(c, rc, [&] { return first_batch_drain(c, reqs, src, &pend, out); });
}

// ---- batched hits ----

// The per-request checks of mh_search_hits_batch: batch_requests' and the cap.
void hits_batch_requests(const mh_hits_request* reqs, size_t n, std::vector<int>* status,
                         std::vector<mh::BatchRequest>* valid, std::vector<uint64_t>* caps) {
    batch_requests(reqs, n, status, valid, [](const mh_hits_request& q) {
        return q.cap > MH_HITS_MAX_CAP ? fail(MH_EINVAL, "cap is larger than MH_HITS_MAX_CAP") : MH_OK;
    });
    caps->clear();
    for (const mh::BatchRequest& r : *valid) caps->push_back(reqs[r.id].cap);
}

// first_refusal for the region probes of the hits batches: a refused request's message, the cap's among them.
const char* hits_batch_refusal(int status, const mh_hits_request& q) {
    return status == MH_EINVAL && q.cap > MH_HITS_MAX_CAP ? "cap is larger than MH_HITS_MAX_CAP" : first_refusal(status);
}

mh::HitsBatchLimits hits_batch_limits() { return mh::HitsBatchLimits{kBatchTableBytes, kBatchResults, hits_slots()}; }

int hits_batch_init_locked(DevCtx* c) {
    if (!c->d_hits) MH_HIP(hipMalloc(&c->d_hits, sizeof(mh::Hit) * MH_HITS_MAX_CAP));
    if (!c->d_hres) MH_HIP(hipMalloc(&c->d_hres, sizeof(mh::BatchHitsResult) * kBatchResults));
    if (!c->h_hres)
        MH_HIP(hipHostMalloc(&c->h_hres, sizeof(mh::BatchHitsResult) * kBatchResults, hipHostMallocDefault));
    if (!c->d_hpacked) MH_HIP(hipMalloc(&c->d_hpacked, sizeof(mh::Hit) * MH_HITS_MAX_CAP));
    if (!c->d_hbase) MH_HIP(hipMalloc(&c->d_hbase, 2 * sizeof(uint64_t)));
    return MH_OK;
}

// The requests of the passes enqueued since the last drain (one window), in h_hres order.
struct HitsBatchPending {
    std::vector<size_t> req_idx;
    std::vector<mh::HitsRegion> region;
    mh::HitsBatchState st;
    uint32_t passes = 0;  // of this window
};

// The base words of a window's next merge: the entries the window's passes packed so far are read
// from one word of d_hbase (none before the window's first pass) and written to the other, in turn.
void hit_window_bases(const DevCtx* c, const HitsBatchPending* pend, const unsigned long long** base_in,
                      unsigned long long** base_out) {
    *base_in = pend->passes ? (const unsigned long long*)c->d_hbase + (pend->passes & 1u) : nullptr;
    *base_out = (unsigned long long*)c->d_hbase + ((pend->passes + 1u) & 1u);
}

// The end of a window: one synchronise, one copy of the entries the window's regions kept (the
// merges packed them, in request order: min(count, slots) per request), then per request its
// minimum and count, and -- where its region held every hit -- its entries sorted by nonce into
// the caller's buffer.  A request that wanted entries and has more hits than its region had slots
// goes to *rebuild.  pend->st is left to the caller.
int hits_batch_drain(DevCtx* c, const mh::BatchRequest* reqs, const mh_hits_request* src, HitsBatchPending* pend,
                     mh_hit* hits, mh_hits_result* out, std::vector<size_t>* rebuild, std::vector<mh::Hit>* stage) {
    MH_TRY(sync_and_harvest(c));
    uint64_t kept = 0;
    for (size_t k = 0; k < pend->req_idx.size(); ++k) kept += std::min(c->h_hres[k].count, pend->region[k].slots);
    if (kept > pend->st.used || kept > MH_HITS_MAX_CAP) return fail(MH_EINTERNAL, "internal: hit window larger than the buffer");
    if (stage->size() < kept) stage->resize((size_t)kept);
    if (kept) MH_HIP(hipMemcpy(stage->data(), c->d_hpacked, (size_t)kept * sizeof(mh::Hit), hipMemcpyDeviceToHost));
    uint64_t pos = 0;  // of the request's entries in the packed order
    for (size_t k = 0; k < pend->req_idx.size(); ++k) {
        const size_t id = reqs[pend->req_idx[k]].id;
        const mh::HitsRegion& g = pend->region[k];
        const mh::BatchHitsResult& res = c->h_hres[k];
        mh_hits_result& r = out[id];
        r.hash = res.hash;
        r.nonce = res.nonce;
        r.count = res.count;
        r.stored = std::min<uint64_t>(res.count, src[id].cap);
        mh::Hit* first = stage->data() + pos;
        pos += std::min(res.count, g.slots);
        if (!src[id].cap) continue;
        if (res.count > g.slots) {  // the region dropped entries; which ones depends on timing
            rebuild->push_back(pend->req_idx[k]);
            continue;
        }
        // count <= slots <= cap: all of them, stored == count
        std::sort(first, first + res.count, [](const mh::Hit& x, const mh::Hit& y) { return x.nonce < y.nonce; });
        for (uint64_t i = 0; i < res.count; ++i) hits[r.offset + i] = mh_hit{first[i].hash, first[i].nonce};
    }
    pend->req_idx.clear();
    pend->region.clear();
    pend->passes = 0;
    return MH_OK;
}

// batch_run_pass over the hits kernels, of mh_search_hits_batch and of mh_search_hits_batch_ex: one
// H2D copy of all its tables -- entries, segments, per-tile entry, per-entry request, the requests'
// words with their initial values (target; cursor = 0; the region), so there is no memset and no
// fill kernel, the fast items (each with its request's target, the device address of its request's
// cursor and its request's region of the device hit buffer) and per-chunk item -- then, on the one
// stream, the scan of the generic entries, one batch_hits<J, MODE> launch per layout in the plan's
// order, merge_segments_hits (it reads segments and words, so it serves slot segments unchanged)
// and one D2H copy of {hash, nonce, count} per request.  The passes of one window queue without a
// synchronise; the items and the per-chunk table count against the window's table buffer.
// A pass without a fast piece (f.items empty: every pass of mh_search_hits_batch, where slot0 ==
// tile0 throughout) is checked by batch_tables_ok and hits_batch_tables_ok, scans with
// batch_scan_hits, has the image of its five tables alone (hits_batch_table_bytes_ex(.., 0, 0) ==
// hits_batch_table_bytes(..)) and leaves a full event pool alone while nothing is in flight; one
// with fast pieces is checked by the _ex checks and scans with batch_scan_hits_slots.  The profile
// counts the launches as batch_run_pass does.
int hits_batch_run_pass(DevCtx* c, const mh::BatchRequest* reqs, const mh_hits_request* src, const uint64_t* caps,
                        const std::vector<mh::BatchPiece>& pieces, const mh::BatchTables& t,
                        const mh::BatchFastTables& f, uint32_t slot_cap, const mh::HitsBatchLimits& lim,
                        HitsBatchPending* pend, mh_hit* hits, mh_hits_result* out, std::vector<size_t>* rebuild,
                        std::vector<mh::Hit>* stage) {
    const bool fast = !f.items.empty();
    if (!(fast ? mh::batch_tables_ex_ok(t, f, slot_cap) : mh::batch_tables_ok(t, slot_cap)))
        return fail(MH_EINTERNAL, "internal: bad batch tables");
    MH_TRY(check_early_items(f, pieces));
    const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
    const size_t ni = f.items.size(), chunks = f.chunk_item.size();
    const size_t o_seg = align16(ne * sizeof(mh::BatchEntry)), o_tile = o_seg + align16((nreq + 1u) * sizeof(uint32_t));
    const size_t o_ereq = o_tile + align16(tiles * sizeof(uint32_t)), o_words = o_ereq + align16(ne * sizeof(uint32_t));
    const size_t o_item = o_words + align16(nreq * sizeof(mh::BatchHitsWords));
    const size_t o_chunk = o_item + ni * sizeof(mh::BatchHitsItem);
    const size_t bytes = o_chunk + align16(chunks * sizeof(uint32_t));
    static_assert(sizeof(mh::BatchHitsItem) % 16 == 0 && sizeof(mh::BatchHitsWords) % 16 == 0, "tables stay 16-byte aligned");
    if (bytes != mh::hits_batch_table_bytes_ex(ne, nreq, tiles, ni, chunks) || bytes > kBatchTableBytes ||
        nreq > kBatchResults)
        return fail(MH_EINTERNAL, "internal: batch pass too large");
    // the event pool cannot take the pass's launches: a drain of its own
    if (prof_needs_drain(c, 1 + (int)f.launches.size()) && (fast || !pend->req_idx.empty())) {
        MH_TRY(hits_batch_drain(c, reqs, src, pend, hits, out, rebuild, stage));
        mh::hits_batch_drained(&pend->st);
    }
    mh::HitsBatchFastTables x;
    mh::HitsBatchState next = pend->st;
    const bool drain = mh::plan_hits_batch_pass_ex(t, f, reqs, caps, lim, &next, &x);  // without items: plan_hits_batch_pass
    if (drain) MH_TRY(hits_batch_drain(c, reqs, src, pend, hits, out, rebuild, stage));
    const uint64_t used_before = drain ? 0u : pend->st.used;
    const size_t toff = drain ? 0u : pend->st.toff;
    pend->st = next;
    const uint64_t window = std::min<uint64_t>(lim.window_slots, MH_HITS_MAX_CAP);
    if (!(fast ? mh::hits_batch_tables_ex_ok(t, f, reqs, x, slot_cap, used_before, window)
               : mh::hits_batch_tables_ok(t, reqs, x.h, used_before, window)) ||
        toff + bytes > kBatchTableBytes || pend->req_idx.size() + nreq > kBatchResults)
        return fail(MH_EINTERNAL, "internal: bad hits batch tables");
    uint8_t* h = c->h_btab + toff;
    uint8_t* d = c->d_btab + toff;
    memcpy(h, t.entries.data(), ne * sizeof(mh::BatchEntry));
    memcpy(h + o_seg, t.seg.data(), (nreq + 1u) * sizeof(uint32_t));
    memcpy(h + o_tile, t.tile_entry.data(), tiles * sizeof(uint32_t));
    memcpy(h + o_ereq, x.h.entry_req.data(), ne * sizeof(uint32_t));
    mh::BatchHitsWords* hw = (mh::BatchHitsWords*)(h + o_words);
    mh::BatchHitsWords* dw = (mh::BatchHitsWords*)(d + o_words);
    for (size_t r = 0; r < nreq; ++r)
        hw[r] = mh::BatchHitsWords{src[reqs[t.req_idx[r]].id].target, 0ull, x.h.region[r].offset, x.h.region[r].slots};
    mh::BatchHitsItem* hi = (mh::BatchHitsItem*)(h + o_item);
    for (size_t k = 0; k < ni; ++k) {
        const uint32_t r = x.item_req[k];  // < nreq, and the request owns the item's slots (checked above)
        mh::BatchHitsItem it;
        memset(&it, 0, sizeof it);
        it.args = f.items[k].args;
        it.unused = nullptr;
        // the region lies inside the window, the window inside the device hit buffer (checked above)
        it.h = mh::HitsArgs{hw[r].target, &dw[r].cursor, c->d_hits + hw[r].offset, hw[r].slots};
        it.chunk0 = f.items[k].chunk0;
        it.slot0 = f.items[k].slot0;
        hi[k] = it;
    }
    memcpy(h + o_chunk, f.chunk_item.data(), chunks * sizeof(uint32_t));
    MH_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    if (tiles) {  // always, without a fast piece (batch_tables_ok)
        Timed* tm = nullptr;
        MH_TRY(prof_begin(c, 1, 0, &tm));
        MH_HIP((fast ? mh::launch_batch_scan_hits_slots : mh::launch_batch_scan_hits)(
            (const mh::BatchEntry*)d, (const uint32_t*)(d + o_tile), (const uint32_t*)(d + o_ereq), dw, c->d_hits,
            c->d_partials, (uint32_t)tiles, c->stream));
        MH_TRY(prof_end_generic(c, tm, t.nonces));
    }
    MH_TRY(run_fast_launches(c, f, pieces, [&](const mh::BatchFastLaunch& l) {
        MH_HIP(mh::launch_batch_hits(c->dev, l.J, l.mode, (const mh::BatchHitsItem*)(d + o_item),
                                     (const uint32_t*)(d + o_chunk) + l.chunk0, c->d_partials, l.chunks, c->stream));
        return MH_OK;
    }));
    const size_t roff = pend->req_idx.size();
    const unsigned long long* base_in;
    unsigned long long* base_out;
    hit_window_bases(c, pend, &base_in, &base_out);
    MH_HIP(mh::launch_merge_segments_hits(c->d_partials, (const uint32_t*)(d + o_seg), dw, c->d_hits, c->d_hpacked,
                                          pend->st.used, base_in, base_out, c->d_hres + roff, (uint32_t)nreq, c->stream));
    ++pend->passes;
    MH_HIP(hipMemcpyAsync(c->h_hres + roff, c->d_hres + roff, nreq * sizeof(mh::BatchHitsResult), hipMemcpyDeviceToHost,
                          c->stream));
    pend->req_idx.insert(pend->req_idx.end(), t.req_idx.begin(), t.req_idx.end());
    pend->region.insert(pend->region.end(), x.h.region.begin(), x.h.region.end());
    return MH_OK;
}

// The fused passes of a hits batch, under the device's lock.
int hits_batch_run_fused(int dev, const mh::BatchRequest* reqs, const mh_hits_request* src, const uint64_t* caps,
                         const std::vector<mh::BatchItem>& items, int passes, uint32_t slot_cap, mh_hit* hits,
                         mh_hits_result* out, std::vector<size_t>* rebuild) {
    BatchSession s;
    MH_TRY(s.open(dev, {batch_init_locked, hits_batch_init_locked}));
    DevCtx* c = s.c;
    const mh::HitsBatchLimits lim = hits_batch_limits();
    HitsBatchPending pend;
    std::vector<mh::Hit> stage;
    mh::BatchTables t;
    const mh::BatchFastTables no_fast;  // mh_search_hits_batch fuses no fast piece
    const std::vector<mh::BatchPiece> no_pieces;
    int rc = MH_OK;
    for (int p = 0; p < passes && !rc; ++p) {
        mh::build_batch_tables(reqs, items, p, &t);
        rc = hits_batch_run_pass(c, reqs, src, caps, no_pieces, t, no_fast, slot_cap, lim, &pend, hits, out, rebuild,
                                 &stage);
    }
    return finish_fused(c, rc, [&] { return hits_batch_drain(c, reqs, src, &pend, hits, out, rebuild, &stage); });
}

// ---- batched hits with fused fast pieces (mh_search_hits_batch_ex) ----

// The fused passes of mh_search_hits_batch_ex(MH_BATCH_FUSE_FAST), under the device's lock.
int hits_batch_run_fused_ex(int dev, const mh::BatchRequest* reqs, const mh_hits_request* src, const uint64_t* caps,
                            const std::vector<mh::BatchPiece>& pieces, const std::vector<mh::FastArgs>& args, int passes,
                            uint32_t slot_cap, mh_hit* hits, mh_hits_result* out, std::vector<size_t>* rebuild) {
    BatchSession s;
    MH_TRY(s.open(dev, {batch_init_locked, hits_batch_init_locked}));
    DevCtx* c = s.c;
    const mh::HitsBatchLimits lim = hits_batch_limits();
    HitsBatchPending pend;
    std::vector<mh::Hit> stage;
    mh::BatchTables t;
    mh::BatchFastTables f;
    int rc = MH_OK;
    for (int p = 0; p < passes && !rc; ++p) {
        mh::build_batch_tables_ex(reqs, pieces, args, p, &t, &f);
        rc = hits_batch_run_pass(c, reqs, src, caps, pieces, t, f, slot_cap, lim, &pend, hits, out, rebuild, &stage);
    }
    return finish_fused(c, rc, [&] { return hits_batch_drain(c, reqs, src, &pend, hits, out, rebuild, &stage); });
}

// ---- batched first k hits (mh_search_first_hits_batch) ----

// The per-request checks of mh_search_first_hits_batch: batch_requests' and k; per valid request its
// target, k and want (plan.hpp first_hits_batch_want), indexed as `valid`.
void first_hits_batch_requests(const mh_first_hits_request* reqs, size_t n, std::vector<int>* status,
                               std::vector<mh::BatchRequest>* valid, std::vector<uint64_t>* targets,
                               std::vector<uint64_t>* ks, std::vector<uint64_t>* wants) {
    batch_requests(reqs, n, status, valid, [](const mh_first_hits_request& q) {
        if (q.k == 0) return fail(MH_EINVAL, "k is 0");
        if (q.k > MH_HITS_MAX_CAP) return fail(MH_EINVAL, "k is larger than MH_HITS_MAX_CAP");
        return MH_OK;
    });
    targets->clear();
    ks->clear();
    wants->clear();
    for (const mh::BatchRequest& r : *valid) {
        targets->push_back(reqs[r.id].target);
        ks->push_back(reqs[r.id].k);
        wants->push_back(mh::first_hits_batch_want(reqs[r.id].k));
    }
}

// first_refusal for the region probe of mh_search_first_hits_batch: a refused request's message, k's among them.
const char* first_hits_batch_refusal(int status, const mh_first_hits_request& q) {
    if (status != MH_EINVAL) return first_refusal(status);
    return q.k == 0 ? "k is 0" : q.k > MH_HITS_MAX_CAP ? "k is larger than MH_HITS_MAX_CAP" : first_refusal(status);
}

mh::HitsBatchLimits first_hits_batch_limits() {
    return mh::HitsBatchLimits{kFirstBatchFastTableBytes, kBatchResults, hits_slots()};
}

int first_hits_batch_init_locked(DevCtx* c) {
    if (!c->d_kres) MH_HIP(hipMalloc(&c->d_kres, sizeof(mh::BatchBoundResult) * kBatchResults));
    if (!c->h_kres)
        MH_HIP(hipHostMalloc(&c->h_kres, sizeof(mh::BatchBoundResult) * kBatchResults, hipHostMallocDefault));
    if (!c->d_bslices)
        MH_HIP(hipMalloc(&c->d_bslices, sizeof(uint32_t) * mh::kFirstHitsSlices * mh::kBatchMaxRequests));
    return MH_OK;
}

// What a call hands to its passes and drains.
struct FirstHitsBatchCall {
    const mh::BatchRequest* reqs;
    const mh_first_hits_request* src;
    const uint64_t *targets, *ks, *wants;  // indexed as reqs
    mh_hit* hits;
    mh_first_hits_result* out;
    std::vector<size_t>* rebuild;
    std::vector<mh::Hit> stage;
};

// The end of a window, as hits_batch_drain: one synchronise, one copy of the entries the window's
// regions kept, then the host's reading of every request (plan.hpp read_first_hits_batch): a request
// whose region dropped entries goes to *rebuild; any other has its entries sorted by nonce into the
// caller's buffer, stored = min(count, k), and with stored == k the minimum of those k, with fewer
// the merged minimum -- nothing of it was then skipped, so scanned must be its whole range.
int first_hits_batch_drain(DevCtx* c, FirstHitsBatchCall* call, HitsBatchPending* pend) {
    MH_TRY(sync_and_harvest(c));
    uint64_t kept = 0;
    for (size_t k = 0; k < pend->req_idx.size(); ++k) kept += std::min(c->h_kres[k].count, pend->region[k].slots);
    if (kept > pend->st.used || kept > MH_HITS_MAX_CAP) return fail(MH_EINTERNAL, "internal: hit window larger than the buffer");
    if (call->stage.size() < kept) call->stage.resize((size_t)kept);
    if (kept) MH_HIP(hipMemcpy(call->stage.data(), c->d_hpacked, (size_t)kept * sizeof(mh::Hit), hipMemcpyDeviceToHost));
    uint64_t pos = 0;  // of the request's entries in the packed order
    for (size_t k = 0; k < pend->req_idx.size(); ++k) {
        const size_t idx = pend->req_idx[k];
        const mh::BatchRequest& q = call->reqs[idx];
        const mh::HitsRegion& g = pend->region[k];
        const mh::BatchBoundResult& res = c->h_kres[k];
        mh_first_hits_result& r = call->out[q.id];
        mh::Hit* first = call->stage.data() + pos;
        pos += std::min(res.count, g.slots);
        r.scanned = res.scanned;
        r.path = 0;
        uint64_t stored = 0, hash = res.hash, nonce = res.nonce;
        if (!mh::read_first_hits_batch(first, res.count, g.slots, call->ks[idx], &stored, &hash, &nonce)) {
            call->rebuild->push_back(idx);
            continue;
        }
        if (stored < call->ks[idx] && res.scanned != q.upper - q.lower + 1u)
            return fail(MH_EINTERNAL, "internal: fewer than k hits, but the fused scan did not hash the whole range");
        r.stored = stored;
        r.hash = hash;
        r.nonce = nonce;
        for (uint64_t i = 0; i < stored; ++i) call->hits[r.offset + i] = mh_hit{first[i].hash, first[i].nonce};
    }
    pend->req_idx.clear();
    pend->region.clear();
    pend->passes = 0;
    return MH_OK;
}

// One pass: its image (plan.cpp build_first_hits_batch_image: every table, the requests' words with
// their initial values, the items with the addresses of their request's words, region and counters)
// checked and copied in one H2D copy, a memset of the pass's slice counters, then on the one stream
// batch_scan_bound[_slots] for the generic entries, one batch_bound<J, MODE> launch per layout in the
// plan's order, merge_segments_bound and one D2H copy of {hash, nonce, count, scanned} per request.
// Windows, regions and drains are hits_batch_run_pass_ex's with the wants in the caps' place; the
// profile counts the launches as that function does.
int first_hits_batch_run_pass(DevCtx* c, FirstHitsBatchCall* call, const std::vector<mh::BatchPiece>* pieces,
                              const mh::BatchTables& t, const mh::BatchFastTables& f, uint32_t slot_cap,
                              const mh::HitsBatchLimits& lim, bool rank_major, HitsBatchPending* pend) {
    MH_TRY(check_early_items(f, *pieces));
    const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
    const mh::FirstHitsBatchLayout l = mh::first_hits_batch_layout(ne, nreq, tiles, f.items.size(), f.chunk_item.size());
    if (l.bytes > kFirstBatchFastTableBytes || nreq > kBatchResults || nreq > mh::kBatchMaxRequests)
        return fail(MH_EINTERNAL, "internal: batch pass too large");
    // the event pool cannot take the pass's launches: a drain of its own
    if (prof_needs_drain(c, 1 + (int)f.launches.size())) {
        MH_TRY(first_hits_batch_drain(c, call, pend));
        mh::hits_batch_drained(&pend->st);
    }
    mh::FirstHitsBatchTables x;
    mh::HitsBatchState next = pend->st;
    const bool drain = mh::plan_first_hits_batch_pass(t, f, call->reqs, call->wants, lim, rank_major, &next, &x);
    if (drain) MH_TRY(first_hits_batch_drain(c, call, pend));
    const uint64_t used_before = drain ? 0u : pend->st.used;
    const size_t toff = drain ? 0u : pend->st.toff;
    pend->st = next;
    const uint64_t window = std::min<uint64_t>(lim.window_slots, MH_HITS_MAX_CAP);
    if (!mh::first_hits_batch_tables_ok(t, f, call->reqs, x, slot_cap, used_before, window) ||
        toff + l.bytes > kFirstBatchFastTableBytes || pend->req_idx.size() + nreq > kBatchResults)
        return fail(MH_EINTERNAL, "internal: bad first-hits batch tables");
    uint8_t* h = c->h_ftab + toff;
    uint8_t* d = c->d_ftab + toff;
    const mh::FirstHitsBatchAddrs at{(uint64_t)(uintptr_t)d, (uint64_t)(uintptr_t)c->d_hits, (uint64_t)(uintptr_t)c->d_bslices};
    mh::build_first_hits_batch_image(t, f, x, call->reqs, call->targets, call->ks, at, h);
    if (!mh::first_hits_batch_image_ok(t, f, x, call->reqs, at, window, h))
        return fail(MH_EINTERNAL, "internal: bad first-hits batch image");
    MH_HIP(hipMemcpyAsync(d, h, l.bytes, hipMemcpyHostToDevice, c->stream));
    MH_HIP(hipMemsetAsync(c->d_bslices, 0, nreq * sizeof(uint32_t) * mh::kFirstHitsSlices, c->stream));
    mh::BatchBoundWords* dw = (mh::BatchBoundWords*)(d + l.o_words);
    if (tiles) {
        Timed* tm = nullptr;
        MH_TRY(prof_begin(c, 1, 0, &tm));
        MH_HIP(mh::launch_batch_scan_bound(!f.items.empty(), (const mh::BatchEntry*)d, (const uint32_t*)(d + l.o_tile),
                                           (const uint32_t*)(d + l.o_ereq), (const uint32_t*)(d + l.o_order), dw,
                                           c->d_bslices, c->d_hits, c->d_partials, (uint32_t)tiles, c->stream));
        MH_TRY(prof_end_generic(c, tm, t.nonces));
    }
    MH_TRY(run_fast_launches(c, f, *pieces, [&](const mh::BatchFastLaunch& fl) {
        MH_HIP(mh::launch_batch_bound(c->dev, fl.J, fl.mode, (const mh::BatchBoundItem*)(d + l.o_item),
                                      (const uint32_t*)(d + l.o_chunk) + fl.chunk0,
                                      (const uint32_t*)(d + l.o_corder) + fl.chunk0, c->d_partials, fl.chunks, c->stream));
        return MH_OK;
    }));
    const size_t roff = pend->req_idx.size();
    const unsigned long long* base_in;
    unsigned long long* base_out;
    hit_window_bases(c, pend, &base_in, &base_out);
    MH_HIP(mh::launch_merge_segments_bound(c->d_partials, (const uint32_t*)(d + l.o_seg), dw, c->d_hits, c->d_hpacked,
                                           pend->st.used, base_in, base_out, c->d_kres + roff, (uint32_t)nreq, c->stream));
    ++pend->passes;
    MH_HIP(hipMemcpyAsync(c->h_kres + roff, c->d_kres + roff, nreq * sizeof(mh::BatchBoundResult), hipMemcpyDeviceToHost,
                          c->stream));
    pend->req_idx.insert(pend->req_idx.end(), t.req_idx.begin(), t.req_idx.end());
    pend->region.insert(pend->region.end(), x.region.begin(), x.region.end());
    return MH_OK;
}

// The fused passes of mh_search_first_hits_batch, under the device's lock.  items: the plan of
// flags == 0 (plan_batch); else pieces and args (plan_batch_ex).
int first_hits_batch_run_fused(int dev, FirstHitsBatchCall* call, const std::vector<mh::BatchItem>* items,
                               const std::vector<mh::BatchPiece>* pieces, const std::vector<mh::FastArgs>* args, int passes,
                               uint32_t slot_cap) {
    BatchSession s;
    MH_TRY(s.open(dev, {batch_init_locked, hits_batch_init_locked, first_batch_fast_init_locked,
                        first_hits_batch_init_locked}));
    DevCtx* c = s.c;
#ifdef MH_DEV_HOOKS
    c->keep = 0;  // mh_search_first_hits_batch refused the hash hooks; nothing of an earlier search's stays
    c->keep_fast = c->xor_on = c->xor_fast = false;
#endif
    const mh::HitsBatchLimits lim = first_hits_batch_limits();
    const bool rank_major = first_batch_rank_major();
    HitsBatchPending pend;
    mh::BatchTables t;
    mh::BatchFastTables f;
    int rc = MH_OK;
    for (int p = 0; p < passes && !rc; ++p) {
        if (items)
            mh::build_batch_tables(call->reqs, *items, p, &t);
        else
            mh::build_batch_tables_ex(call->reqs, *pieces, *args, p, &t, &f);
        rc = first_hits_batch_run_pass(c, call, pieces, t, f, slot_cap, lim, rank_major, &pend);
    }
    return finish_fused(c, rc, [&] { return first_hits_batch_drain(c, call, &pend); });
}

// mh_search_batch_ex(MH_BATCH_FUSE_FAST) over n >= 1 requests, the fallbacks through `fallback`.
int search_batch_ex_impl(int dev, const mh_request* reqs, size_t n, mh_result* out, const BatchFallback& fallback) {
    std::vector<int> status;
    std::vector<mh::BatchRequest> valid;
    batch_requests(reqs, n, &status, &valid);
    for (size_t i = 0; i < n; ++i) out[i] = mh_result{status[i], 0, 0, 0};
    if (valid.empty()) return MH_OK;
    g_err.clear();
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    mh::plan_batch_ex(valid.data(), valid.size(), plan_opts(), slot_cap, batch_fast_shared_lanes(), batch_fast_max(),
                      &pieces, &args);
    const int passes = batch_passes(pieces);
    if (passes) MH_TRY(batch_run_fused_ex(dev, valid.data(), pieces, args, passes, slot_cap, out));
    for (const mh::BatchPiece& p : pieces) {  // the fallbacks, after the fused passes
        if (p.kind != 1) continue;
        const mh::BatchRequest& r = valid[p.idx];
        const int rc = fallback(r, &out[r.id].hash, &out[r.id].nonce);
        if (rc) return rc;
    }
    return MH_OK;
}

}  // namespace

extern "C" {

int mh_search_batch(int dev, const mh_request* reqs, size_t n, mh_result* out) {
    g_err.clear();
    if (n == 0) return MH_OK;
    if (!reqs || !out) return fail(MH_EINVAL, "NULL array");
    return search_batch_impl(dev, reqs, n, out, [dev](const mh::BatchRequest& r, uint64_t* h, uint64_t* nn) {
        return search_impl(dev, r.pre, r.lower, r.upper, h, nn);
    });
}

int mh_search_batch_ex(int dev, const mh_request* reqs, size_t n, uint32_t flags, mh_result* out) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (!(flags & MH_BATCH_FUSE_FAST)) return mh_search_batch(dev, reqs, n, out);
    if (n == 0) return MH_OK;
    if (!reqs || !out) return fail(MH_EINVAL, "NULL array");
    return search_batch_ex_impl(dev, reqs, n, out, [dev](const mh::BatchRequest& r, uint64_t* h, uint64_t* nn) {
        return search_impl(dev, r.pre, r.lower, r.upper, h, nn);
    });
}

int64_t mh_batch_plan_ex(const mh_request* reqs, size_t n, uint32_t flags, mh_batch_piece* out, int64_t cap) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (n == 0) return 0;
    if (!reqs) return fail(MH_EINVAL, "NULL array");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    std::vector<int> status;
    std::vector<mh::BatchRequest> all;
    batch_requests(reqs, n, &status, &all);
    MH_TRY(refuse_first(status));  // the first request mh_search would refuse
    int64_t k = 0;
    if (!(flags & MH_BATCH_FUSE_FAST)) {  // mh_batch_plan's plan in the new struct
        std::vector<mh::BatchItem> items;
        mh::plan_batch(all.data(), n, plan_opts(), batch_slots(), &items);
        for (const mh::BatchItem& it : items) {
            if (k >= cap) return cap + 1;  // cap + 1 signals truncation
            if (out) out[k] = mh_batch_piece{it.req, it.first, it.count, it.kind, it.pass, it.slot, it.slots, 0, 0, 0, -1};
            ++k;
        }
        return k;
    }
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    mh::plan_batch_ex(all.data(), n, plan_opts(), batch_slots(), batch_fast_shared_lanes(), batch_fast_max(), &pieces,
                      &args);
    for (const mh::BatchPiece& p : pieces) {
        if (k >= cap) return cap + 1;
        if (out)
            out[k] = mh_batch_piece{p.req, p.first, p.count, p.kind, p.pass, p.slot, p.slots, p.J, p.mode, p.L, p.launch};
        ++k;
    }
    return k;
}

int64_t mh_batch_plan(const mh_request* reqs, size_t n, mh_batch_item* out, int64_t cap) {
    g_err.clear();
    if (n == 0) return 0;
    if (!reqs) return fail(MH_EINVAL, "NULL array");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    std::vector<int> status;
    std::vector<mh::BatchRequest> all;
    batch_requests(reqs, n, &status, &all);
    MH_TRY(refuse_first(status));  // the first request mh_search would refuse
    std::vector<mh::BatchItem> items;
    mh::plan_batch(all.data(), n, plan_opts(), batch_slots(), &items);
    int64_t k = 0;
    for (const mh::BatchItem& it : items) {
        if (k >= cap) return cap + 1;  // cap + 1 signals truncation
        if (out) out[k] = mh_batch_item{it.req, it.first, it.count, it.kind, it.pass, it.slot, it.slots};
        ++k;
    }
    return k;
}

int mh_search_first_batch(int dev, const mh_first_request* reqs, size_t n, mh_first_result* out) {
    g_err.clear();
    if (n == 0) return MH_OK;
    if (!reqs || !out) return fail(MH_EINVAL, "NULL array");
    MH_TRY(refuse_hash_hooks("mh_search_first_batch"));
    std::vector<int> status;
    std::vector<mh::BatchRequest> valid;
    batch_requests(reqs, n, &status, &valid);
    for (size_t i = 0; i < n; ++i) out[i] = mh_first_result{status[i], 0, 0, 0, 0};
    if (valid.empty()) return MH_OK;
    g_err.clear();
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchItem> items;
    mh::plan_batch(valid.data(), valid.size(), plan_opts(), slot_cap, &items);
    const int passes = batch_passes(items);
    if (passes) MH_TRY(first_batch_run_fused(dev, valid.data(), reqs, items, passes, slot_cap, out));
    for (const mh::BatchItem& it : items) {  // the fallbacks, after the fused passes
        if (it.kind != 1) continue;
        const mh::BatchRequest& r = valid[it.idx];
        mh_first f;
        const int rc = search_first_impl(dev, r.pre, r.lower, r.upper, reqs[r.id].target, 0u, &f);
        if (rc) return rc;
        put_first_result(&out[r.id], f.hash, f.nonce, f.scanned, reqs[r.id].target);
    }
    return MH_OK;
}

// mh_search_first_batch_ex(MH_BATCH_FUSE_FAST) and, with stop, mh_search_first_batch_stop (`name`: the
// caller's, for messages): the same plan, passes and order; stop selects batch_stop<J, MODE> for the
// fast launches and mh_search_first_ex(MH_FIRST_STOP_RUNNING)'s path for the fallbacks.
static int first_batch_fused_impl(int dev, const mh_first_request* reqs, size_t n, bool stop, const char* name,
                           mh_first_result* out) {
    if (n == 0) return MH_OK;
    if (!reqs || !out) return fail(MH_EINVAL, "NULL array");
    MH_TRY(refuse_hash_hooks(name));
    std::vector<int> status;
    std::vector<mh::BatchRequest> valid;
    batch_requests(reqs, n, &status, &valid);
    for (size_t i = 0; i < n; ++i) out[i] = mh_first_result{status[i], 0, 0, 0, 0};
    if (valid.empty()) return MH_OK;
    g_err.clear();
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    mh::plan_batch_ex(valid.data(), valid.size(), plan_opts(), slot_cap, batch_fast_shared_lanes(), batch_fast_max(),
                      &pieces, &args);
    const int passes = batch_passes(pieces);
    if (passes) MH_TRY(first_batch_run_fused_ex(dev, valid.data(), reqs, pieces, args, passes, slot_cap, stop, out));
    for (const mh::BatchPiece& p : pieces) {  // the fallbacks, after the fused passes
        if (p.kind != 1) continue;
        const mh::BatchRequest& r = valid[p.idx];
        mh_first f;
        const int rc = search_first_impl(dev, r.pre, r.lower, r.upper, reqs[r.id].target,
                                         stop ? (uint32_t)MH_FIRST_STOP_RUNNING : 0u, &f);
        if (rc) return rc;
        put_first_result(&out[r.id], f.hash, f.nonce, f.scanned, reqs[r.id].target);
    }
    return MH_OK;
}

int mh_search_first_batch_ex(int dev, const mh_first_request* reqs, size_t n, uint32_t flags, mh_first_result* out) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (!(flags & MH_BATCH_FUSE_FAST)) return mh_search_first_batch(dev, reqs, n, out);
    return first_batch_fused_impl(dev, reqs, n, false, "mh_search_first_batch_ex", out);
}

int mh_search_first_batch_stop(int dev, const mh_first_request* reqs, size_t n, mh_first_result* out) {
    g_err.clear();
    return first_batch_fused_impl(dev, reqs, n, true, "mh_search_first_batch_stop", out);
}

int64_t mh_first_batch_order(const mh_request* reqs, size_t n, int32_t pass, uint32_t* out, int64_t cap) {
    g_err.clear();
    if (!reqs && n > 0) return fail(MH_EINVAL, "NULL array");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    std::vector<int> status;
    std::vector<mh::BatchRequest> all;
    batch_requests(reqs, n, &status, &all);
    MH_TRY(refuse_first(status));  // the first request mh_search would refuse, as mh_batch_plan
    std::vector<mh::BatchItem> items;
    const uint32_t slot_cap = batch_slots();
    mh::plan_batch(all.data(), n, plan_opts(), slot_cap, &items);
    if (pass < 0 || pass >= batch_passes(items)) return fail(MH_EINVAL, "no such pass");
    mh::BatchTables t;
    mh::build_batch_tables(all.data(), items, pass, &t);
    if (!mh::batch_tables_ok(t, slot_cap)) return fail(MH_EINTERNAL, "internal: bad batch tables");
    mh::FirstBatchTables ft;
    mh::build_first_batch_tables(t, first_batch_rank_major(), &ft);
    if (!mh::first_batch_tables_ok(t, ft)) return fail(MH_EINTERNAL, "internal: bad first-hit batch tables");
    int64_t k = 0;
    for (const uint32_t s : ft.order) {
        if (k >= cap) return cap + 1;  // cap + 1 signals truncation
        if (out) out[k] = s;
        ++k;
    }
    return k;
}

int64_t mh_first_batch_order_ex(const mh_request* reqs, size_t n, uint32_t flags, int32_t pass, int32_t launch,
                                uint32_t* out, int64_t cap) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (!(flags & MH_BATCH_FUSE_FAST)) {
        if (launch != -1) return fail(MH_EINVAL, "no such launch");
        return mh_first_batch_order(reqs, n, pass, out, cap);
    }
    if (!reqs && n > 0) return fail(MH_EINVAL, "NULL array");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    std::vector<int> status;
    std::vector<mh::BatchRequest> all;
    batch_requests(reqs, n, &status, &all);
    MH_TRY(refuse_first(status));  // the first request mh_search would refuse, as mh_batch_plan
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    mh::plan_batch_ex(all.data(), n, plan_opts(), slot_cap, batch_fast_shared_lanes(), batch_fast_max(), &pieces, &args);
    if (pass < 0 || pass >= batch_passes(pieces)) return fail(MH_EINVAL, "no such pass");
    mh::BatchTables t;
    mh::BatchFastTables f;
    mh::build_batch_tables_ex(all.data(), pieces, args, pass, &t, &f);
    if (launch < -1 || launch >= (int32_t)f.launches.size()) return fail(MH_EINVAL, "no such launch");
    mh::FirstBatchFastTables x;
    mh::build_first_batch_tables_ex(t, f, first_batch_rank_major(), &x);
    if (!mh::first_batch_tables_ex_ok(t, f, x, slot_cap)) return fail(MH_EINTERNAL, "internal: bad first-hit batch tables");
    const uint32_t* ord = launch < 0 ? x.tile_order.data() : x.chunk_order.data() + f.launches[(size_t)launch].chunk0;
    const size_t cnt = launch < 0 ? x.tile_order.size() : f.launches[(size_t)launch].chunks;
    int64_t k = 0;
    for (size_t b = 0; b < cnt; ++b) {
        if (k >= cap) return cap + 1;  // cap + 1 signals truncation
        if (out) out[k] = mh::first_batch_order_slot(t, f, launch, ord[b]);
        ++k;
    }
    return k;
}

int mh_search_hits_batch(int dev, const mh_hits_request* reqs, size_t n, mh_hit* hits, size_t hits_cap,
                         mh_hits_result* out) {
    g_err.clear();
    if (n == 0) return MH_OK;
    if (!reqs || !out) return fail(MH_EINVAL, "NULL array");
    MH_TRY(refuse_hash_hooks("mh_search_hits_batch"));
    std::vector<int> status;
    std::vector<mh::BatchRequest> valid;
    std::vector<uint64_t> caps;
    hits_batch_requests(reqs, n, &status, &valid, &caps);
    uint64_t total = 0;  // the offsets: prefix sums of the caps, whatever the status; an out-of-range cap counts as 0
    for (size_t i = 0; i < n; ++i) {
        out[i] = mh_hits_result{status[i], 0, 0, 0, 0, 0, total};
        if (reqs[i].cap <= MH_HITS_MAX_CAP) total += reqs[i].cap;
        if (total > hits_cap) return fail(MH_EINVAL, "the caps add up to more than hits_cap");
    }
    if (!hits && total > 0) return fail(MH_EINVAL, "hits is NULL with a cap > 0");
    if (valid.empty()) return MH_OK;
    g_err.clear();
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchItem> items;
    mh::plan_batch(valid.data(), valid.size(), plan_opts(), slot_cap, &items);
    const int passes = batch_passes(items);
    std::vector<size_t> rebuild;  // fused requests whose region dropped entries
    if (passes)
        MH_TRY(hits_batch_run_fused(dev, valid.data(), reqs, caps.data(), items, passes, slot_cap, hits, out, &rebuild));
    for (const size_t idx : rebuild) {  // the list again through the mh_search_hits path: count and minimum must agree
        const mh::BatchRequest& r = valid[idx];
        mh_hits_result& o = out[r.id];
        mh_hits h;
        const int rc = search_hits_impl(dev, r.pre, r.lower, r.upper, reqs[r.id].target, hits + o.offset,
                                        (size_t)reqs[r.id].cap, &h);
        if (rc) return rc;
        if (h.count != o.count || h.hash != o.hash || h.nonce != o.nonce || h.stored != o.stored)
            return fail(MH_EINTERNAL, "internal: a rebuilt hit list disagrees with the fused scan");
    }
    for (const mh::BatchItem& it : items) {  // the fallbacks, after the fused passes
        if (it.kind != 1) continue;
        const mh::BatchRequest& r = valid[it.idx];
        mh_hits_result& o = out[r.id];
        mh_hits h;
        const int rc = search_hits_impl(dev, r.pre, r.lower, r.upper, reqs[r.id].target,
                                        reqs[r.id].cap ? hits + o.offset : nullptr, (size_t)reqs[r.id].cap, &h);
        if (rc) return rc;
        o.count = h.count;
        o.stored = h.stored;
        o.hash = h.hash;
        o.nonce = h.nonce;
    }
    return MH_OK;
}

int64_t mh_hits_batch_regions(const mh_hits_request* reqs, size_t n, mh_hits_region* out, int64_t cap) {
    g_err.clear();
    if (n == 0) return 0;
    if (!reqs) return fail(MH_EINVAL, "NULL array");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    std::vector<int> status;
    std::vector<mh::BatchRequest> all;
    std::vector<uint64_t> caps;
    hits_batch_requests(reqs, n, &status, &all, &caps);
    for (size_t i = 0; i < n; ++i)  // the first request mh_search_hits_batch would refuse
        if (status[i]) return fail(status[i], hits_batch_refusal(status[i], reqs[i]));
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchItem> items;
    mh::plan_batch(all.data(), n, plan_opts(), slot_cap, &items);
    const int passes = batch_passes(items);
    std::vector<mh_hits_region> regions(n);
    for (const mh::BatchItem& it : items)
        if (it.kind == 1) regions[it.idx] = mh_hits_region{it.req, 1, -1, -1, 0, 0, 0};
    const mh::HitsBatchLimits lim = hits_batch_limits();
    mh::HitsBatchState st;
    mh::BatchTables t;
    mh::HitsBatchTables ht;
    for (int p = 0; p < passes; ++p) {
        mh::build_batch_tables(all.data(), items, p, &t);
        if (!mh::batch_tables_ok(t, slot_cap)) return fail(MH_EINTERNAL, "internal: bad batch tables");
        const uint64_t before = st.used;
        const bool drain = mh::plan_hits_batch_pass(t, all.data(), caps.data(), lim, &st, &ht);
        if (!mh::hits_batch_tables_ok(t, all.data(), ht, drain ? 0u : before, lim.window_slots))
            return fail(MH_EINTERNAL, "internal: bad hits batch tables");
        for (size_t r = 0; r < t.req_idx.size(); ++r)
            regions[t.req_idx[r]] = mh_hits_region{all[t.req_idx[r]].id, 0, p, st.window, 0, ht.region[r].offset,
                                                   ht.region[r].slots};
    }
    int64_t k = 0;
    for (const mh_hits_region& g : regions) {
        if (k >= cap) return cap + 1;  // cap + 1 signals truncation
        if (out) out[k] = g;
        ++k;
    }
    return k;
}

int mh_search_hits_batch_ex(int dev, const mh_hits_request* reqs, size_t n, uint32_t flags, mh_hit* hits,
                            size_t hits_cap, mh_hits_result* out) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (!(flags & MH_BATCH_FUSE_FAST)) return mh_search_hits_batch(dev, reqs, n, hits, hits_cap, out);
    if (n == 0) return MH_OK;
    if (!reqs || !out) return fail(MH_EINVAL, "NULL array");
    MH_TRY(refuse_hash_hooks("mh_search_hits_batch_ex"));
    std::vector<int> status;
    std::vector<mh::BatchRequest> valid;
    std::vector<uint64_t> caps;
    hits_batch_requests(reqs, n, &status, &valid, &caps);
    uint64_t total = 0;  // the offsets, as mh_search_hits_batch
    for (size_t i = 0; i < n; ++i) {
        out[i] = mh_hits_result{status[i], 0, 0, 0, 0, 0, total};
        if (reqs[i].cap <= MH_HITS_MAX_CAP) total += reqs[i].cap;
        if (total > hits_cap) return fail(MH_EINVAL, "the caps add up to more than hits_cap");
    }
    if (!hits && total > 0) return fail(MH_EINVAL, "hits is NULL with a cap > 0");
    if (valid.empty()) return MH_OK;
    g_err.clear();
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    mh::plan_batch_ex(valid.data(), valid.size(), plan_opts(), slot_cap, batch_fast_shared_lanes(), batch_fast_max(),
                      &pieces, &args);
    const int passes = batch_passes(pieces);
    std::vector<size_t> rebuild;  // fused requests whose region dropped entries
    if (passes)
        MH_TRY(hits_batch_run_fused_ex(dev, valid.data(), reqs, caps.data(), pieces, args, passes, slot_cap, hits, out,
                                       &rebuild));
    // The lists again through the mh_search_hits path.  The fused scan has the exact count, so a
    // list cut by its cap (stored < count) is rebuilt from a prefix of the range: the `stored`
    // smallest qualifying nonces of [lower, hi] are those of the whole range once [lower, hi] holds
    // at least `stored` hits.  The prefix is sized from the observed density with a quarter to
    // spare and doubled while it holds too few; at hi == upper the count and minimum must agree.
    for (const size_t idx : rebuild) {
        const mh::BatchRequest& r = valid[idx];
        mh_hits_result& o = out[r.id];
        const double total = (double)(r.upper - r.lower) + 1.0;
        double want = o.stored < o.count ? 1.25 * total * (double)o.stored / (double)o.count + 1024.0 : total;
        for (;;) {
            const uint64_t span = want >= total ? r.upper - r.lower : (uint64_t)want;  // hi - lower
            const uint64_t hi = span >= r.upper - r.lower ? r.upper : r.lower + span;
            mh_hits h;
            const int rc = search_hits_impl(dev, r.pre, r.lower, hi, reqs[r.id].target, hits + o.offset,
                                            (size_t)reqs[r.id].cap, &h);
            if (rc) return rc;
            if (hi == r.upper) {
                if (h.count != o.count || h.hash != o.hash || h.nonce != o.nonce || h.stored != o.stored)
                    return fail(MH_EINTERNAL, "internal: a rebuilt hit list disagrees with the fused scan");
                break;
            }
            if (h.count > o.count) return fail(MH_EINTERNAL, "internal: a prefix holds more hits than the fused scan counted");
            if (h.stored == o.stored) break;  // stored == cap here: the prefix held at least cap hits
            want *= 2.0;
        }
    }
    for (const mh::BatchPiece& p : pieces) {  // the fallbacks, after the fused passes
        if (p.kind != 1) continue;
        const mh::BatchRequest& r = valid[p.idx];
        mh_hits_result& o = out[r.id];
        mh_hits h;
        const int rc = search_hits_impl(dev, r.pre, r.lower, r.upper, reqs[r.id].target,
                                        reqs[r.id].cap ? hits + o.offset : nullptr, (size_t)reqs[r.id].cap, &h);
        if (rc) return rc;
        o.count = h.count;
        o.stored = h.stored;
        o.hash = h.hash;
        o.nonce = h.nonce;
    }
    return MH_OK;
}

int64_t mh_hits_batch_regions_ex(const mh_hits_request* reqs, size_t n, uint32_t flags, mh_hits_region* out,
                                 int64_t cap) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (!(flags & MH_BATCH_FUSE_FAST)) return mh_hits_batch_regions(reqs, n, out, cap);
    if (n == 0) return 0;
    if (!reqs) return fail(MH_EINVAL, "NULL array");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    std::vector<int> status;
    std::vector<mh::BatchRequest> all;
    std::vector<uint64_t> caps;
    hits_batch_requests(reqs, n, &status, &all, &caps);
    for (size_t i = 0; i < n; ++i)  // the first request mh_search_hits_batch would refuse
        if (status[i]) return fail(status[i], hits_batch_refusal(status[i], reqs[i]));
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    mh::plan_batch_ex(all.data(), n, plan_opts(), slot_cap, batch_fast_shared_lanes(), batch_fast_max(), &pieces, &args);
    const int passes = batch_passes(pieces);
    std::vector<mh_hits_region> regions(n);
    for (const mh::BatchPiece& p : pieces)
        if (p.kind == 1) regions[p.idx] = mh_hits_region{p.req, 1, -1, -1, 0, 0, 0};
    const mh::HitsBatchLimits lim = hits_batch_limits();
    mh::HitsBatchState st;
    mh::BatchTables t;
    mh::BatchFastTables f;
    mh::HitsBatchFastTables x;
    for (int p = 0; p < passes; ++p) {
        mh::build_batch_tables_ex(all.data(), pieces, args, p, &t, &f);
        const uint64_t before = st.used;
        const bool fast = !f.items.empty();  // the plan and the checks of hits_batch_run_pass
        if (!fast && !mh::batch_tables_ok(t, slot_cap)) return fail(MH_EINTERNAL, "internal: bad batch tables");
        const bool drain = mh::plan_hits_batch_pass_ex(t, f, all.data(), caps.data(), lim, &st, &x);
        if (!(fast ? mh::hits_batch_tables_ex_ok(t, f, all.data(), x, slot_cap, drain ? 0u : before, lim.window_slots)
                   : mh::hits_batch_tables_ok(t, all.data(), x.h, drain ? 0u : before, lim.window_slots)))
            return fail(MH_EINTERNAL, "internal: bad hits batch tables");
        for (size_t r = 0; r < t.req_idx.size(); ++r)
            regions[t.req_idx[r]] = mh_hits_region{all[t.req_idx[r]].id, 0, p, st.window, 0, x.h.region[r].offset,
                                                   x.h.region[r].slots};
    }
    int64_t k = 0;
    for (const mh_hits_region& g : regions) {
        if (k >= cap) return cap + 1;  // cap + 1 signals truncation
        if (out) out[k] = g;
        ++k;
    }
    return k;
}

int mh_search_first_hits_batch(int dev, const mh_first_hits_request* reqs, size_t n, uint32_t flags, mh_hit* hits,
                               size_t hits_cap, mh_first_hits_result* out) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (n == 0) return MH_OK;
    if (!reqs || !out) return fail(MH_EINVAL, "NULL array");
    MH_TRY(refuse_hash_hooks("mh_search_first_hits_batch"));
    std::vector<int> status;
    std::vector<mh::BatchRequest> valid;
    std::vector<uint64_t> targets, ks, wants;
    first_hits_batch_requests(reqs, n, &status, &valid, &targets, &ks, &wants);
    uint64_t total = 0;  // the offsets: prefix sums of k, whatever the status; a k out of range counts as 0
    for (size_t i = 0; i < n; ++i) {
        out[i] = mh_first_hits_result{status[i], 0, 0, 0, 0, 0, total};
        if (reqs[i].k <= MH_HITS_MAX_CAP) total += reqs[i].k;
        if (total > hits_cap) return fail(MH_EINVAL, "the k add up to more than hits_cap");
    }
    if (!hits && total > 0) return fail(MH_EINVAL, "hits is NULL with a k > 0");
    if (valid.empty()) return MH_OK;
    g_err.clear();
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchItem> items;
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    std::vector<size_t> fallback;  // positions in `valid`
    int passes;
    if (flags & MH_BATCH_FUSE_FAST) {
        mh::plan_batch_ex(valid.data(), valid.size(), plan_opts(), slot_cap, batch_fast_shared_lanes(), batch_fast_max(),
                          &pieces, &args);
        passes = batch_passes(pieces);
        for (const mh::BatchPiece& p : pieces)
            if (p.kind == 1) fallback.push_back(p.idx);
    } else {
        mh::plan_batch(valid.data(), valid.size(), plan_opts(), slot_cap, &items);
        passes = batch_passes(items);
        for (const mh::BatchItem& it : items)
            if (it.kind != 0) fallback.push_back(it.idx);
    }
    std::vector<size_t> rebuild;  // fused requests whose region dropped entries
    if (passes) {
        FirstHitsBatchCall call{valid.data(), reqs, targets.data(), ks.data(), wants.data(), hits, out, &rebuild, {}};
        MH_TRY(first_hits_batch_run_fused(dev, &call, (flags & MH_BATCH_FUSE_FAST) ? nullptr : &items, &pieces, &args,
                                          passes, slot_cap));
    }
    // the rebuilt requests and the fallbacks through the mh_search_first_hits path, after the fused passes
    for (int which = 0; which < 2; ++which)
        for (const size_t idx : which ? fallback : rebuild) {
            const mh::BatchRequest& r = valid[idx];
            mh_first_hits_result& o = out[r.id];
            mh_first_hits h;
            const int rc = search_first_hits_impl(dev, r.pre, r.lower, r.upper, targets[idx], hits + o.offset, (size_t)ks[idx], &h,
                                                  true);
            if (rc) return rc;
            o.stored = h.stored;
            o.scanned = h.scanned;
            o.hash = h.hash;
            o.nonce = h.nonce;
            o.path = which ? 1 : 2;
        }
    return MH_OK;
}

int64_t mh_first_hits_batch_regions(const mh_first_hits_request* reqs, size_t n, uint32_t flags, mh_hits_region* out,
                                    int64_t cap) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (n == 0) return 0;
    if (!reqs) return fail(MH_EINVAL, "NULL array");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    std::vector<int> status;
    std::vector<mh::BatchRequest> all;
    std::vector<uint64_t> targets, ks, wants;
    first_hits_batch_requests(reqs, n, &status, &all, &targets, &ks, &wants);
    for (size_t i = 0; i < n; ++i)  // the first request mh_search_first_hits_batch would refuse
        if (status[i]) return fail(status[i], first_hits_batch_refusal(status[i], reqs[i]));
    const uint32_t slot_cap = batch_slots();
    const bool fast = (flags & MH_BATCH_FUSE_FAST) != 0;
    std::vector<mh::BatchItem> items;
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    std::vector<mh_hits_region> regions(n);
    int passes;
    if (fast) {
        mh::plan_batch_ex(all.data(), n, plan_opts(), slot_cap, batch_fast_shared_lanes(), batch_fast_max(), &pieces, &args);
        passes = batch_passes(pieces);
        for (const mh::BatchPiece& p : pieces)
            if (p.kind == 1) regions[p.idx] = mh_hits_region{p.req, 1, -1, -1, 0, 0, 0};
    } else {
        mh::plan_batch(all.data(), n, plan_opts(), slot_cap, &items);
        passes = batch_passes(items);
        for (const mh::BatchItem& it : items)
            if (it.kind != 0) regions[it.idx] = mh_hits_region{it.req, 1, -1, -1, 0, 0, 0};
    }
    const mh::HitsBatchLimits lim = first_hits_batch_limits();
    const bool rank_major = first_batch_rank_major();
    mh::HitsBatchState st;
    mh::BatchTables t;
    mh::BatchFastTables f;
    mh::FirstHitsBatchTables x;
    for (int p = 0; p < passes; ++p) {
        if (fast)
            mh::build_batch_tables_ex(all.data(), pieces, args, p, &t, &f);
        else
            mh::build_batch_tables(all.data(), items, p, &t);
        const uint64_t before = st.used;
        const bool drain = mh::plan_first_hits_batch_pass(t, f, all.data(), wants.data(), lim, rank_major, &st, &x);
        if (!mh::first_hits_batch_tables_ok(t, f, all.data(), x, slot_cap, drain ? 0u : before, lim.window_slots))
            return fail(MH_EINTERNAL, "internal: bad first-hits batch tables");
        for (size_t r = 0; r < t.req_idx.size(); ++r)
            regions[t.req_idx[r]] = mh_hits_region{all[t.req_idx[r]].id, 0, p, st.window, 0, x.region[r].offset,
                                                   x.region[r].slots};
    }
    int64_t k = 0;
    for (const mh_hits_region& g : regions) {
        if (k >= cap) return cap + 1;  // cap + 1 signals truncation
        if (out) out[k] = g;
        ++k;
    }
    return k;
}

int mh_miner_handle(const int* devs, int ndev, const char* request, size_t len, char* out, size_t cap,
                    size_t* out_len) {
    if (!request || !devs || ndev <= 0) return fail(MH_EINVAL, "bad arguments");
    mh::Msg m;
    if (!mh::decode(request, len, &m)) return fail(MH_ENOTREQ, "payload is not a JSON bitcoin.Message");
    if (m.type != 1) return fail(MH_ENOTREQ, "not a Request");  // message.go:10
    if (m.lower > m.upper) return fail(MH_ERANGE, "lower > upper");
    const uint8_t* d = (const uint8_t*)m.data.data();
    uint64_t h = 0, n = 0;
    if (m.has_target) {  // a chunk of a target job (minehip_server.h): the chunk's first hit, else its minimum
        mh_first f;
        const int rc = (ndev == 1)
                           ? mh_search_first_ex(devs[0], d, m.data.size(), m.lower, m.upper, m.target, 0u, &f)
                           : mh_search_first_multi(devs, ndev, d, m.data.size(), m.lower, m.upper, m.target, 0, 0u, &f);
        if (rc) return rc;
        h = f.hash;
        n = f.nonce;
    } else {
        const int rc = (ndev == 1) ? mh_search(devs[0], d, m.data.size(), m.lower, m.upper, &h, &n)
                                   : mh_search_multi(devs, ndev, d, m.data.size(), m.lower, m.upper, 0, &h, &n);
        if (rc) return rc;
    }
    const std::string s = mh::encode(2, nullptr, 0, 0, 0, h, n);  // NewResult (message.go:38-44)
    if (out_len) *out_len = s.size();
    if (!out || cap < s.size()) return fail(MH_EINVAL, "output buffer too small");
    memcpy(out, s.data(), s.size());
    return MH_OK;
}

int mh_miner_handle_batch(const int* devs, int ndev, const char* const* requests, const size_t* lens, size_t n,
                          char* out, size_t cap_each, size_t* out_lens, int* status) {
    return mh_miner_handle_batch_ex(devs, ndev, requests, lens, n, 0, out, cap_each, out_lens, status);
}

int mh_miner_handle_batch_ex(const int* devs, int ndev, const char* const* requests, const size_t* lens, size_t n,
                             uint32_t flags, char* out, size_t cap_each, size_t* out_lens, int* status) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (n == 0) return MH_OK;
    if (!devs || ndev <= 0 || !requests || !lens || !status) return fail(MH_EINVAL, "bad arguments");
    std::vector<mh::Msg> msgs(n);
    std::vector<mh_request> reqs;
    std::vector<size_t> where;  // reqs[k] is payload where[k]
    std::vector<mh_first_request> freqs;  // the Requests with a Target, and their payloads
    std::vector<size_t> fwhere;
    for (size_t i = 0; i < n; ++i) {
        if (out_lens) out_lens[i] = 0;
        mh::Msg& m = msgs[i];
        if (!requests[i]) {
            status[i] = fail(MH_EINVAL, "bad arguments");
        } else if (!mh::decode(requests[i], lens[i], &m)) {
            status[i] = fail(MH_ENOTREQ, "payload is not a JSON bitcoin.Message");
        } else if (m.type != 1) {
            status[i] = fail(MH_ENOTREQ, "not a Request");  // message.go:10
        } else if (m.lower > m.upper) {
            status[i] = fail(MH_ERANGE, "lower > upper");
        } else if (m.has_target) {
            status[i] = MH_OK;
            freqs.push_back(mh_first_request{(const uint8_t*)m.data.data(), m.data.size(), m.lower, m.upper, m.target});
            fwhere.push_back(i);
        } else {
            status[i] = MH_OK;
            reqs.push_back(mh_request{(const uint8_t*)m.data.data(), m.data.size(), m.lower, m.upper});
            where.push_back(i);
        }
    }
    // NewResult (message.go:38-44) of payload i
    auto put = [&](size_t i, uint64_t hash, uint64_t nonce) {
        const std::string s = mh::encode(2, nullptr, 0, 0, 0, hash, nonce);
        if (out_lens) out_lens[i] = s.size();
        if (!out || cap_each < s.size()) {
            status[i] = fail(MH_EINVAL, "output buffer too small");
            return;
        }
        memcpy(out + i * cap_each, s.data(), s.size());
    };
    if (!freqs.empty()) {
        // the Target Requests: one first-hit batch on devs[0], answered as mh_miner_handle answers each
        std::vector<mh_first_result> fres(freqs.size());
        const int rc = mh_search_first_batch_ex(devs[0], freqs.data(), freqs.size(), flags, fres.data());
        if (rc) return rc;
        for (size_t k = 0; k < freqs.size(); ++k) {
            status[fwhere[k]] = fres[k].status;
            if (fres[k].status == MH_OK) put(fwhere[k], fres[k].hash, fres[k].nonce);
        }
    }
    if (reqs.empty()) return MH_OK;
    std::vector<mh_result> res(reqs.size());
    // fallbacks as mh_miner_handle searches: one device through mh_search's path, several through
    // mh_search_multi's adaptive split
    const BatchFallback fallback = [&](const mh::BatchRequest& r, uint64_t* h, uint64_t* nn) {
        if (ndev == 1) return search_impl(devs[0], r.pre, r.lower, r.upper, h, nn);
        const mh_request& q = reqs[r.id];
        return mh_search_multi(devs, ndev, q.msg, q.len, q.lower, q.upper, 0, h, nn);
    };
    const int rc = (flags & MH_BATCH_FUSE_FAST)
                       ? search_batch_ex_impl(devs[0], reqs.data(), reqs.size(), res.data(), fallback)
                       : search_batch_impl(devs[0], reqs.data(), reqs.size(), res.data(), fallback);
    if (rc) return rc;
    for (size_t k = 0; k < reqs.size(); ++k) {
        const size_t i = where[k];
        status[i] = res[k].status;
        if (res[k].status) continue;
        put(i, res[k].hash, res[k].nonce);
    }
    return MH_OK;
}

int mh_hash_batch(int dev, const uint8_t* msg, size_t len, const uint64_t* nonces, size_t n, uint64_t* out_hashes) {
    g_err.clear();
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (n == 0) return MH_OK;
    if (!nonces || !out_hashes) return fail(MH_EINVAL, "NULL buffer");
    DevCtx* c;
    rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipSetDevice(dev));
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    mh::GenArgs ga;
    mh::make_gen_args(pre, &ga);
    for (size_t off = 0; off < n; off += kBatchChunk) {
        const size_t m = (n - off < kBatchChunk) ? n - off : kBatchChunk;
        MH_HIP(hipMemcpyAsync(c->d_nonces, nonces + off, m * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        MH_HIP(mh::launch_hash_batch(ga, c->d_nonces, c->d_hashes, m, c->stream));
        MH_HIP(hipMemcpyAsync(out_hashes + off, c->d_hashes, m * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        MH_HIP(hipStreamSynchronize(c->stream));
    }
    return MH_OK;
}

}  // extern "C"

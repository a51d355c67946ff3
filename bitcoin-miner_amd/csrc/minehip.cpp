// minehip.cpp -- C-ABI of libminehip.so (declared in include/minehip.h).
//
// Per device: one HIP stream, a partials buffer, a 16-byte running minimum
// and a pinned 16-byte host slot, created on first use and reused by every
// call.  A search enqueues all of its launches (fast runs, generic edges,
// merges) on that stream and synchronises once, when it copies the 16-byte
// result back.  No CPU fallback exists: without a gfx950 device the calls fail
// with MH_ENODEV.
//
// The batched entry points (mh_search_batch and its kin) are in batch.cpp; host_ctx.hpp holds what
// the two files share.
#include <stdio.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <memory>
#include <system_error>
#include <thread>

#include "../../include/minehip_server.h"
#include "host_ctx.hpp"
#include "msgcodec.hpp"
#include "multi.hpp"
#include "sched.hpp"

namespace mh {
namespace host {

thread_local std::string g_err;

int fail(int code, const std::string& what) {
    g_err = what;
    return code;
}

}  // namespace host

int set_error(int code, const char* what) { return host::fail(code, what); }

namespace host {

static std::mutex g_tab_mu;
static std::vector<std::unique_ptr<DevCtx>> g_tab;
static int g_ndev = -1;

static int device_count_impl() {
    std::lock_guard<std::mutex> lk(g_tab_mu);
    if (g_ndev < 0) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
        g_ndev = n;
        g_tab.resize((size_t)n);
        for (auto& p : g_tab) p.reset(new DevCtx());
    }
    return g_ndev;
}

// Returns the context for dev, initialised, with its mutex NOT held.
int get_ctx(int dev, DevCtx** out) {
    const int n = device_count_impl();
    if (n <= 0) return fail(MH_ENODEV, "no HIP device visible");
    if (dev < 0 || dev >= n) return fail(MH_EINVAL, "device index out of range");
    DevCtx* c = g_tab[(size_t)dev].get();
    *out = c;
    return MH_OK;
}

int init_locked(DevCtx* c, int dev) {
    if (c->ready) return MH_OK;
    MH_HIP(hipSetDevice(dev));
    hipDeviceProp_t prop;
    MH_HIP(hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MH_ENODEV, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    // each resource only once: a call after a failed init (e.g. the code object
    // did not load) resumes where that one stopped instead of allocating again
    if (!c->stream) MH_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    if (!c->ps[0] || !c->ps[1]) {
        int least = 0, greatest = 0;
        MH_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));  // gfx950: 1 .. -1
        if (!c->ps[0]) MH_HIP(hipStreamCreateWithPriority(&c->ps[0], hipStreamNonBlocking, greatest));
        if (!c->ps[1]) MH_HIP(hipStreamCreateWithPriority(&c->ps[1], hipStreamNonBlocking, least));
    }
    for (auto& e : c->ev_piece)
        if (!e) MH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (!c->ev_main) MH_HIP(hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming));
    if (!c->d_partials) MH_HIP(hipMalloc(&c->d_partials, sizeof(Partial) * mh::kMaxBlocksPerLaunch));
    if (!c->d_best) MH_HIP(hipMalloc(&c->d_best, sizeof(Partial)));
    if (!c->d_counters) MH_HIP(hipMalloc(&c->d_counters, sizeof(uint32_t) * kQueueSlots));
    if (!c->h_best) MH_HIP(hipHostMalloc(&c->h_best, sizeof(Partial), hipHostMallocDefault));
    if (!c->d_nonces) MH_HIP(hipMalloc(&c->d_nonces, sizeof(uint64_t) * kBatchChunk));
    if (!c->d_hashes) MH_HIP(hipMalloc(&c->d_hashes, sizeof(uint64_t) * kBatchChunk));
    if (c->pool.empty()) c->pool.resize(kEventPairs);
    for (auto& t : c->pool) {
        if (!t.start) MH_HIP(hipEventCreate(&t.start));
        if (!t.stop) MH_HIP(hipEventCreate(&t.stop));
    }
    MH_HIP(mh::fast_module_init(dev));  // the fast_search code object (issue-priority build)
    c->dev = dev;
    c->ready = true;
    return MH_OK;
}

#ifdef MH_DEV_HOOKS
// MINEHIP_DEV_HASH_KEEP=k0,k1 (dev build only, 0 <= k <= 32): every scan kernel keeps
// only the top k0 bits of H0 and the top k1 bits of H1 of each nonce's hash, so that many nonces
// tie and the (hash, nonce) tie-breaking of the kernels and merges decides the result; the search
// returns the masked hash.  Read by every search (one process can run many settings) into
// c->keep, the word the pieces carry (layout.hpp keep_word).  The fast kernels mask only in the
// variant code object (build/fast_search_keep.hsaco through MINEHIP_DEV_CODE_OBJECT): with any
// other, a fast piece fails the search (enqueue_piece) instead of mixing masked and full hashes.
int read_hash_keep(DevCtx* c) {
    c->keep = 0;
    c->keep_fast = false;
    const char* e = getenv("MINEHIP_DEV_HASH_KEEP");
    if (!e || !*e) return MH_OK;
    unsigned k0 = 0, k1 = 0;
    char rest = 0;
    if (sscanf(e, "%u,%u%c", &k0, &k1, &rest) != 2 || k0 > 32u || k1 > 32u)
        return fail(MH_EINVAL, "MINEHIP_DEV_HASH_KEEP: expected k0,k1 with 0 <= k <= 32");
    MH_HIP(mh::fast_keep_ok(c->dev, &c->keep_fast));
    c->keep = mh::keep_word(k0, k1);
    return MH_OK;
}

// MINEHIP_DEV_HASH_XOR=<1-16 hex digits> (dev build only): every scan kernel XORs each
// nonce's (H0, H1) with the high and low 32 bits of the constant before the keep mask and before any
// comparison, so a test decides which nonce of a range wins: with x = Hash(msg, n) the search returns
// (0, n) exactly if it hashes n correctly, considers it and rebuilds its value.  Unset or zero: off.
// Read by every search, after read_hash_keep and before anything of the search is enqueued; the
// constant reaches the kernels through a device word (search_kernels.hip set_hash_xor) rewritten only
// when the value changes.  The fast kernels XOR only in the variant code object: with any other,
// a fast piece fails the search (enqueue_piece).
int read_hash_xor(DevCtx* c) {
    c->xor_on = c->xor_fast = false;
    const char* e = getenv("MINEHIP_DEV_HASH_XOR");
    uint64_t x = 0;
    if (e && *e) {
        size_t n = 0;
        for (; e[n]; ++n) {
            const char ch = e[n];
            const int v = (ch >= '0' && ch <= '9') ? ch - '0' : (ch >= 'a' && ch <= 'f') ? ch - 'a' + 10
                        : (ch >= 'A' && ch <= 'F') ? ch - 'A' + 10 : -1;
            if (v < 0 || n >= 16) return fail(MH_EINVAL, "MINEHIP_DEV_HASH_XOR: expected 1 to 16 hex digits");
            x = (x << 4) | (uint64_t)v;
        }
    }
    MH_HIP(mh::set_hash_xor(c->dev, x, c->stream, &c->xor_fast));
    c->xor_on = x != 0;
    return MH_OK;
}
#endif

// Stream must be idle or synchronised by the caller.
int harvest_locked(DevCtx* c) {
    for (int i = 0; i < c->used; ++i) {
        float ms = 0.f;
        MH_HIP(hipEventElapsedTime(&ms, c->pool[(size_t)i].start, c->pool[(size_t)i].stop));
        const uint64_t ns = (uint64_t)((double)ms * 1.0e6);
        c->cnt[c->pool[(size_t)i].kind == 0 ? 2 : 5] += ns;
        if (c->pool[(size_t)i].kind == 0) c->var[c->pool[(size_t)i].var].ns += ns;
    }
    c->used = 0;
    return MH_OK;
}

// The piece streams start after the main stream's work so far (the reset, a merge).
static int piece_streams_wait_main(DevCtx* c) {
    MH_HIP(hipEventRecord(c->ev_main, c->stream));
    for (auto s : c->ps) MH_HIP(hipStreamWaitEvent(s, c->ev_main, 0));
    return MH_OK;
}

// Fold the pending partials into the running minimum.  With two piece
// streams the merge (on the main stream) first waits for both, and both wait
// for the merge before any later piece reuses the partials buffer.
static int flush_partials(DevCtx* c, bool split) {
    if (!c->poff) return MH_OK;
    if (split) {
        for (int k = 0; k < 2; ++k) {
            MH_HIP(hipEventRecord(c->ev_piece[k], c->ps[k]));
            MH_HIP(hipStreamWaitEvent(c->stream, c->ev_piece[k], 0));
        }
    }
    MH_HIP(mh::launch_merge(c->d_partials, c->poff, c->d_best, c->stream));
    c->poff = 0;
    if (split) return piece_streams_wait_main(c);
    return MH_OK;
}

// Coarse pieces (the full L: 1,000-nonce lanes) go to the high-priority stream, the others
// (shorter lanes, generic edges, the tail split) to the low-priority one.
static bool coarse_piece(const mh::Piece& p, const mh::PlanOpts& opt) { return p.kind == 0 && p.L == opt.lower_digits; }

// An Early piece (layout.hpp kMode*Early) enumerates its innermost digit and the L - 1 group digits
// before it inside word J: the kernel adds every group digit into word J, so a digit elsewhere
// would be hashed at the wrong place.  make_fast_args only builds such pieces; this re-checks it
// where a piece reaches the kernel, with the U digits' hole inside the d digits.
bool early_piece_ok(const mh::FastArgs& a, int word) {
    const uint32_t J = (uint32_t)word;
    if ((a.inner >> 2) != J || a.hole + a.hole_w > a.n_hi + a.L) return false;
    for (uint32_t j = 0; j + 1u < a.L; ++j) {
        const uint32_t pos = a.g_last - j - (j >= a.g_hole ? 1u : 0u);
        if (pos > a.g_last || (pos >> 2) != J) return false;
    }
    return true;
}

// Enqueue one piece on the context's stream.  Its workgroups write their
// partials after those of the previous pieces; one merge folds them all (or
// earlier, when the buffer would overflow), instead of one merge per piece.
static int enqueue_piece(DevCtx* c, const mh::Piece& p, const mh::PlanOpts& opt, bool split) {
    hipStream_t s = !split ? c->stream : c->ps[coarse_piece(p, opt) ? 0 : 1];
    uint32_t blocks;
    if (p.kind == 0) {
        // host-side shape checks: the grid covers exactly n_runs lanes and the
        // partials buffer holds one slot per block
        if (p.fa.n_runs == 0 || p.fa.L < 1 || p.fa.L > 5 || p.fa.n_hi + p.fa.L > 20)
            return fail(MH_EINTERNAL, "internal: bad fast piece");
        if (p.fa.mode >= mh::kModeOneEarly && !early_piece_ok(p.fa, p.J))
            return fail(MH_EINTERNAL, "internal: bad Early piece (an enumerated digit outside word J)");
        blocks = (p.fa.n_runs + mh::kBlockThreads - 1) / mh::kBlockThreads;
    } else {
        if (p.ga.count == 0 || p.ga.count > (uint64_t)mh::kMaxBlocksPerLaunch * mh::kBlockThreads)
            return fail(MH_EINTERNAL, "internal: bad generic piece");
        blocks = (uint32_t)((p.ga.count + mh::kBlockThreads - 1) / mh::kBlockThreads);
    }
    if (blocks > mh::kMaxBlocksPerLaunch) return fail(MH_EINTERNAL, "internal: grid too large");
    if (c->poff + blocks > mh::kMaxBlocksPerLaunch) {
        const int rc = flush_partials(c, split);
        if (rc) return rc;
    }
    Partial* out = c->d_partials + c->poff;
    Timed* tm = nullptr;
    mh::FastArgs fa = p.fa;
#ifdef MH_DEV_HOOKS
    mh::GenArgs ga = p.ga;
    ga.pad = c->keep;
    if (p.kind == 0) {
        if (c->keep && !c->keep_fast)
            return fail(MH_EINVAL, "MINEHIP_DEV_HASH_KEEP is set but the fast code object is not the coarse-hash "
                                   "variant (MINEHIP_DEV_CODE_OBJECT=build/fast_search_keep.hsaco)");
        if (c->xor_on && !c->xor_fast)
            return fail(MH_EINVAL, "MINEHIP_DEV_HASH_XOR is set but the fast code object has no mh_dev_hash_xor "
                                   "(MINEHIP_DEV_CODE_OBJECT=build/fast_search_keep.hsaco)");
        fa.pad_ = c->keep;
    }
#else
    const mh::GenArgs& ga = p.ga;
#endif
    if (p.kind == 0) {
        fa.n_chunks = blocks;
        // work queue while this search has counters left (a longer search runs the rest static)
        fa.counter = (opt.queue && c->qoff < kQueueSlots) ? c->d_counters + c->qoff++ : nullptr;
    }
    if (c->prof) {
        if (c->used == kEventPairs) {
            MH_HIP(hipStreamSynchronize(c->stream));
            for (auto ps : c->ps) MH_HIP(hipStreamSynchronize(ps));
            int rc = harvest_locked(c);
            if (rc) return rc;
        }
        tm = &c->pool[(size_t)c->used++];
        tm->kind = p.kind;
        tm->var = p.kind == 0 ? var_index(p.J, p.mode, p.L) : 0;
        MH_HIP(hipEventRecord(tm->start, s));
    }
    if (c->first) {  // mh_search_first: the first-hit kernels over the same pieces
        if (p.kind == 0)
            MH_HIP(mh::launch_fast_first(c->dev, p.J, p.mode, fa, out, *c->first, c->first_stop, s));
        else
            MH_HIP(mh::launch_generic_scan_first(ga, out, blocks, *c->first, s));
    } else if (c->hits_stop) {  // mh_search_first_hits: the stopping hits kernels over the same pieces
        if (p.kind == 0)
            MH_HIP(mh::launch_fast_hits_stop(c->dev, p.J, p.mode, fa, out, *c->hits_stop, s));
        else
            MH_HIP(mh::launch_generic_scan_hits_stop(ga, out, blocks, *c->hits_stop, s));
    } else if (c->hits) {  // mh_search_hits: the hits kernels over the same pieces
        if (p.kind == 0)
            MH_HIP(mh::launch_fast_hits(c->dev, p.J, p.mode, fa, out, *c->hits, s));
        else
            MH_HIP(mh::launch_generic_scan_hits(ga, out, blocks, *c->hits, s));
    } else if (p.kind == 0)
        MH_HIP(mh::launch_fast(c->dev, p.J, p.mode, fa, out, s));
    else
        MH_HIP(mh::launch_generic_scan(ga, out, blocks, s));
    if (tm) MH_HIP(hipEventRecord(tm->stop, s));
    c->poff += blocks;
    if (c->prof) {
        if (p.kind == 0) {
            const uint64_t n = p.count;
            c->cnt[0] += 1;
            c->cnt[1] += n;
            c->cnt[3] += n * (uint64_t)p.ops;
            c->cnt[6] += n * (uint64_t)p.slots;
            VarStat& v = c->var[var_index(p.J, p.mode, p.L)];
            v.launches += 1;
            v.nonces += n;
            v.ops += n * (uint64_t)p.ops;
            v.slots += n * (uint64_t)p.slots;
        } else {
            c->cnt[4] += p.count;
        }
    }
    return MH_OK;
}

// Planner knobs, overridable for tests and tuning (the result never depends
// on them -- tests/test_gpu_parity.py checks exactly that):
//   MINEHIP_LOWER_DIGITS   L, digits enumerated inside one lane (1..5, default 3)
//   MINEHIP_MIN_LANES      lower L per bucket until it has this many runs (2^19)
//   MINEHIP_LAUNCH_NONCES  nonces per fast launch (default 2^35)
//   MINEHIP_GENERIC_BELOW  buckets with fewer nonces go to the generic kernel (2^20)
//   MINEHIP_MAX_BLOCKS     workgroups per launch (1..kMaxBlocksPerLaunch)
//   MINEHIP_STREAMS        1: one stream; 2: coarse / fine pieces on high / low priority
//                          streams (default 2)
//   MINEHIP_FINE_TAIL      nonces at the end of each full-L bucket planned at L - 1 (default
//                          2^28; 0: none)
//   MINEHIP_QUEUE          1: fast launches as work queues (workgroups claim chunks, so faster
//                          XCDs take more; default); 0: one workgroup per chunk
//   MINEHIP_EARLY          1: the Early layouts where a nonce costs less with the digit ending the
//                          word before the last digit's innermost (default); 0: never
mh::PlanOpts plan_opts() {
    mh::PlanOpts o;
    if (const char* e = getenv("MINEHIP_LOWER_DIGITS")) {
        const int v = atoi(e);
        if (v >= 1 && v <= 5) o.lower_digits = v;
    }
    if (const char* e = getenv("MINEHIP_MIN_LANES")) o.min_lanes = strtoull(e, nullptr, 10);
    if (const char* e = getenv("MINEHIP_LAUNCH_NONCES")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v >= 1) o.max_nonces_per_launch = v;
    }
    if (const char* e = getenv("MINEHIP_GENERIC_BELOW")) o.generic_below = strtoull(e, nullptr, 10);
    if (const char* e = getenv("MINEHIP_MAX_BLOCKS")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v >= 1 && v <= mh::kMaxBlocksPerLaunch) o.max_blocks = (uint32_t)v;
    }
    if (const char* e = getenv("MINEHIP_STREAMS")) {
        const int v = atoi(e);
        if (v == 1 || v == 2) o.streams = v;
    }
    if (const char* e = getenv("MINEHIP_FINE_TAIL")) o.fine_tail = strtoull(e, nullptr, 10);
    if (const char* e = getenv("MINEHIP_QUEUE")) {
        const int v = atoi(e);
        if (v == 0 || v == 1) o.queue = v;
    }
    if (const char* e = getenv("MINEHIP_EARLY")) {
        const int v = atoi(e);
        if (v == 0 || v == 1) o.early = v;
    }
    return o;
}

static uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

// busy_ns (optional): the search's own wall time, from holding the initialised device to having
// its result -- without the wait for another thread's search on the same device.
int search_impl(int dev, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t* oh, uint64_t* on,
                uint64_t* busy_ns) {
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    const uint64_t t0 = now_ns();
    MH_HIP(hipSetDevice(dev));
#ifdef MH_DEV_HOOKS
    rc = read_hash_keep(c);
    if (rc) return rc;
    rc = read_hash_xor(c);
    if (rc) return rc;
#endif
    MH_HIP(hipMemsetAsync(c->d_best, 0xFF, sizeof(Partial), c->stream));
    const mh::PlanOpts opt = plan_opts();
    if (opt.queue) MH_HIP(hipMemsetAsync(c->d_counters, 0, sizeof(uint32_t) * kQueueSlots, c->stream));
    c->qoff = 0;
    // Two streams only when there is something to overlap: coarse pieces and others.  A small
    // search (generic edges, short-lane buckets) stays on one stream and skips the events.  The
    // plan is streamed, never stored (a range can hold ~2^30 pieces); this first pass stops as
    // soon as it has seen both kinds.
    bool any_coarse = false, any_fine = false;
    if (opt.streams == 2)
        mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
            (coarse_piece(p, opt) ? any_coarse : any_fine) = true;
            return !(any_coarse && any_fine);
        });
    const bool split = opt.streams == 2 && any_coarse && any_fine;
    if (split) {  // the piece streams start after the reset (and after the previous search)
        rc = piece_streams_wait_main(c);
        if (rc) return rc;
    }
    int err = MH_OK;
    c->poff = 0;
    mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
        err = enqueue_piece(c, p, opt, split);
        return err == MH_OK;
    });
    if (!err) err = flush_partials(c, split);
    if (err) {
        for (auto ps : c->ps)
            if (ps) (void)hipStreamSynchronize(ps);
        (void)hipStreamSynchronize(c->stream);
        return err;
    }
    MH_HIP(hipMemcpyAsync(c->h_best, c->d_best, sizeof(Partial), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    if (c->prof) {
        rc = harvest_locked(c);
        if (rc) return rc;
    }
    *oh = c->h_best->hash;
    *on = c->h_best->nonce;
    if (busy_ns) *busy_ns = now_ns() - t0;
    return MH_OK;
}

// mh_search_first: search_impl's plan, streams, partial flushes and work-queue counters over the
// first-hit kernels (first_scan<J, MODE>, generic_scan_first; layout.hpp FirstArgs), then
// finish_first on the main stream and one 24-byte copy-back with the one synchronise.  The word
// the kernels skip later chunks by and the scanned count are reset beside the running minimum.
// flags (mh_search_first_ex, checked by the caller): MH_FIRST_STOP_RUNNING launches stop_scan<J, MODE>
// in place of first_scan<J, MODE>; nothing else differs.
int search_first_impl(int dev, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t target, uint32_t flags,
                      mh_first* out) {
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipSetDevice(dev));
    if (!c->d_first) MH_HIP(hipMalloc(&c->d_first, 5 * sizeof(uint64_t)));
    if (!c->h_first) MH_HIP(hipHostMalloc(&c->h_first, 3 * sizeof(uint64_t), hipHostMallocDefault));
#ifdef MH_DEV_HOOKS
    c->keep = 0;  // mh_search_first refused the hash hooks; nothing of an earlier search's stays
    c->keep_fast = c->xor_on = c->xor_fast = false;
#endif
    MH_HIP(hipMemsetAsync(c->d_best, 0xFF, sizeof(Partial), c->stream));
    MH_HIP(hipMemsetAsync(c->d_first, 0xFF, sizeof(uint64_t), c->stream));
    MH_HIP(hipMemsetAsync(c->d_first + 1, 0, sizeof(uint64_t), c->stream));
    const mh::PlanOpts opt = plan_opts();
    if (opt.queue) MH_HIP(hipMemsetAsync(c->d_counters, 0, sizeof(uint32_t) * kQueueSlots, c->stream));
    c->qoff = 0;
    bool any_coarse = false, any_fine = false;
    if (opt.streams == 2)
        mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
            (coarse_piece(p, opt) ? any_coarse : any_fine) = true;
            return !(any_coarse && any_fine);
        });
    const bool split = opt.streams == 2 && any_coarse && any_fine;
    if (split) {
        rc = piece_streams_wait_main(c);
        if (rc) return rc;
    }
    const mh::FirstArgs fargs{target, (unsigned long long*)c->d_first, (unsigned long long*)(c->d_first + 1)};
    int err = MH_OK;
    c->poff = 0;
    c->first = &fargs;
    c->first_stop = (flags & MH_FIRST_STOP_RUNNING) != 0;
    mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
        err = enqueue_piece(c, p, opt, split);
        return err == MH_OK;
    });
    c->first = nullptr;
    c->first_stop = false;
    if (!err) err = flush_partials(c, split);
    if (err) {
        for (auto ps : c->ps)
            if (ps) (void)hipStreamSynchronize(ps);
        (void)hipStreamSynchronize(c->stream);
        return err;
    }
    mh::GenArgs ga;
    mh::make_gen_args(pre, &ga);
    MH_HIP(mh::launch_finish_first(ga, c->d_best, (const unsigned long long*)(c->d_first + 1), c->d_first + 2, c->stream));
    MH_HIP(hipMemcpyAsync(c->h_first, c->d_first + 2, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    if (c->prof) {
        rc = harvest_locked(c);
        if (rc) return rc;
    }
    out->hash = c->h_first[0];
    out->nonce = c->h_first[1];
    out->scanned = c->h_first[2];
    out->found = out->hash <= target ? 1 : 0;  // without a qualifying nonce the minimum itself is > target
    out->reserved = 0;
    return MH_OK;
}

//   MINEHIP_HITS_SLOTS     entries of the device hit buffer one scan of mh_search_hits may fill
//                          (1..MH_HITS_MAX_CAP, the default): a lower value makes a search with more
//                          hits rebuild its list window by window (tests; the results never depend
//                          on it)
uint64_t hits_slots() {
    if (const char* e = getenv("MINEHIP_HITS_SLOTS")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v >= 1 && v <= MH_HITS_MAX_CAP) return v;
    }
    return MH_HITS_MAX_CAP;
}

// One scan of [lower, upper] for mh_search_hits, under the device's lock: search_impl's plan,
// streams, partial flushes and work-queue counters over the hits kernels (hits_scan<J, MODE>,
// generic_scan_hits; layout.hpp HitsArgs), one synchronise, then the range's minimum in c->h_best,
// its hit count in *count and, if `got` is given, the min(count, slots) entries the device buffer
// holds in *got (in no particular order; all of the range's hits exactly if count <= slots).
static int hits_scan_range(DevCtx* c, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t target, uint64_t slots,
                    uint64_t* count, std::vector<mh::Hit>* got) {
    MH_HIP(hipMemsetAsync(c->d_best, 0xFF, sizeof(Partial), c->stream));
    MH_HIP(hipMemsetAsync(c->d_hcursor, 0, sizeof(uint64_t), c->stream));
    const mh::PlanOpts opt = plan_opts();
    if (opt.queue) MH_HIP(hipMemsetAsync(c->d_counters, 0, sizeof(uint32_t) * kQueueSlots, c->stream));
    c->qoff = 0;
    bool any_coarse = false, any_fine = false;
    if (opt.streams == 2)
        mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
            (coarse_piece(p, opt) ? any_coarse : any_fine) = true;
            return !(any_coarse && any_fine);
        });
    const bool split = opt.streams == 2 && any_coarse && any_fine;
    if (split) {
        const int rc = piece_streams_wait_main(c);
        if (rc) return rc;
    }
    const mh::HitsArgs hargs{target, (unsigned long long*)c->d_hcursor, c->d_hits, slots};
    int err = MH_OK;
    c->poff = 0;
    c->hits = &hargs;
    mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
        err = enqueue_piece(c, p, opt, split);
        return err == MH_OK;
    });
    c->hits = nullptr;
    if (!err) err = flush_partials(c, split);
    if (err) {
        for (auto ps : c->ps)
            if (ps) (void)hipStreamSynchronize(ps);
        (void)hipStreamSynchronize(c->stream);
        return err;
    }
    MH_HIP(hipMemcpyAsync(c->h_best, c->d_best, sizeof(Partial), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipMemcpyAsync(c->h_hcursor, c->d_hcursor, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    if (c->prof) {
        const int rc = harvest_locked(c);
        if (rc) return rc;
    }
    *count = *c->h_hcursor;
    if (got) {
        got->resize((size_t)std::min(*count, slots));
        if (!got->empty()) MH_HIP(hipMemcpy(got->data(), c->d_hits, got->size() * sizeof(mh::Hit), hipMemcpyDeviceToHost));
    }
    return MH_OK;
}

static bool hit_by_nonce(const mh::Hit& x, const mh::Hit& y) { return x.nonce < y.nonce; }

// The window walk of mh_search_hits and mh_search_first_hits, under the device's lock: the hits of
// [lower, upper] from `lower` upward, in nonce order, out of windows [cur, cur + w - 1] scanned by
// the non-stopping hits kernels (hits_scan_range), until `want` entries are collected or `upper` is
// reached.  w is sized from `spacing`, the nonces per hit the caller observed, for about a quarter
// of the buffer per window; a window that overflows the buffer all the same is halved and scanned
// again (one of at most `slots` nonces cannot overflow), one that fits is complete, so sorted and
// appended.  The last window's entries are all kept: *list may hold more than `want`.
// widen (the rebuilds of mh_search_first_hits_batch only; mh_search_hits and mh_search_first_hits walk
// as they always did): after a window that fit the next one is twice as wide again, up to the first
// size, so that two hits that lie close together narrow the windows around them only.  A walk that
// keeps its narrowest width takes range / smallest gap scans with a buffer of one entry, and a batch
// under a small MINEHIP_HITS_SLOTS rebuilds most of its requests.  The widths decide which windows
// are scanned, never what the list holds.
static int hits_window_walk(DevCtx* c, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t target, uint64_t slots,
                     uint64_t want, double spacing, std::vector<mh::Hit>* list, bool widen = false) {
    const double per_window = std::max(1.0, (double)slots / 4.0 * spacing);
    uint64_t w = per_window >= 9.0e18 ? (uint64_t)9.0e18 : (uint64_t)per_window;
    const uint64_t w0 = w;
    std::vector<mh::Hit> win;
    uint64_t cur = lower;
    list->clear();
    while (list->size() < want) {
        const uint64_t hi = (upper - cur < w - 1u) ? upper : cur + (w - 1u);
        uint64_t wc = 0;
        const int rc = hits_scan_range(c, pre, cur, hi, target, slots, &wc, &win);
        if (rc) return rc;
        if (wc > slots) {  // hi - cur + 1 > slots >= 1 here
            w = (hi - cur + 1u) / 2u;
            continue;
        }
        std::sort(win.begin(), win.end(), hit_by_nonce);
        list->insert(list->end(), win.begin(), win.end());
        if (hi == upper) break;
        cur = hi + 1u;
        if (widen && w < w0) w = w0 - w < w ? w0 : w * 2u;
    }
    return MH_OK;
}

// mh_search_hits: one scan of the whole range gives the minimum, the exact count (the cursor
// advances for every hit) and, while the count fits the device buffer, every hit; the host sorts
// them by nonce and returns the first `cap`.  When the buffer overflowed, which entries it kept
// depends on timing, so the list is rebuilt from `lower` upward out of windows [cur, cur + w - 1]
// scanned by the same kernels: w is sized from the observed density for about a quarter of the
// buffer per window, a window that overflows all the same is halved and scanned again (one of at
// most `slots` nonces cannot overflow), one that fits is complete, so sorted and appended, until
// min(count, cap) entries are collected (hits_window_walk).  The count and the minimum are the first scan's.
int search_hits_impl(int dev, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t target, mh_hit* hits,
                     size_t cap, mh_hits* out) {
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipSetDevice(dev));
    if (!c->d_hits) MH_HIP(hipMalloc(&c->d_hits, sizeof(mh::Hit) * MH_HITS_MAX_CAP));
    if (!c->d_hcursor) MH_HIP(hipMalloc(&c->d_hcursor, sizeof(uint64_t)));
    if (!c->h_hcursor) MH_HIP(hipHostMalloc(&c->h_hcursor, sizeof(uint64_t), hipHostMallocDefault));
#ifdef MH_DEV_HOOKS
    c->keep = 0;  // mh_search_hits refused the hash hooks; nothing of an earlier search's stays
    c->keep_fast = c->xor_on = c->xor_fast = false;
#endif
    const uint64_t slots = hits_slots();
    std::vector<mh::Hit> got;
    uint64_t count = 0;
    rc = hits_scan_range(c, pre, lower, upper, target, slots, &count, cap ? &got : nullptr);
    if (rc) return rc;
    out->count = count;
    out->stored = std::min<uint64_t>(count, cap);
    out->hash = c->h_best->hash;
    out->nonce = c->h_best->nonce;
    if (cap && count > slots) {  // the buffer dropped entries: rebuild the list window by window
        const double total = (double)(upper - lower) + 1.0;
        std::vector<mh::Hit> list;
        rc = hits_window_walk(c, pre, lower, upper, target, slots, out->stored, total / (double)count, &list);
        if (rc) return rc;
        if (list.size() < out->stored) return fail(MH_EINTERNAL, "internal: the hit windows hold fewer hits than the scan counted");
        got.swap(list);
    } else {
        std::sort(got.begin(), got.end(), hit_by_nonce);
    }
    for (uint64_t i = 0; i < out->stored; ++i) hits[i] = mh_hit{got[(size_t)i].hash, got[(size_t)i].nonce};
    return MH_OK;
}

// mh_search_first_hits: hits_scan_range's plan, streams, partial flushes and work-queue counters over
// the stopping hits kernels (hits_stop<J, MODE>, generic_scan_hits_stop; layout.hpp HitsStopArgs),
// one synchronise, then the k smallest of the appended hits.  Every nonce <= the bound word's final
// value was hashed (a chunk or tile is only skipped or left above a value the word held, and the
// word only decreases) and at least k hits are <= it, so the appended hits hold the k smallest of
// the range whenever they are k or more; with fewer the word was never lowered (it is lowered only
// from slice counts that hold k appended hits), nothing was skipped and the minimum is the range's.
// When the device buffer dropped entries, which ones depends on timing: the list is rebuilt from
// `lower` upward by the window walk of mh_search_hits, on the non-stopping kernels, until k entries
// are collected or `upper` is reached.
// widen_walk: hits_window_walk's `widen`, for the rebuilds and fallbacks of mh_search_first_hits_batch.
int search_first_hits_impl(int dev, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t target, mh_hit* hits,
                           size_t k, mh_first_hits* out, bool widen_walk) {
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipSetDevice(dev));
    if (!c->d_hits) MH_HIP(hipMalloc(&c->d_hits, sizeof(mh::Hit) * MH_HITS_MAX_CAP));
    if (!c->d_hcursor) MH_HIP(hipMalloc(&c->d_hcursor, sizeof(uint64_t)));
    if (!c->h_hcursor) MH_HIP(hipHostMalloc(&c->h_hcursor, sizeof(uint64_t), hipHostMallocDefault));
    if (!c->d_fhits) MH_HIP(hipMalloc(&c->d_fhits, 2 * sizeof(uint64_t)));
    if (!c->d_slices) MH_HIP(hipMalloc(&c->d_slices, sizeof(uint32_t) * mh::kFirstHitsSlices));
    if (!c->h_fhits) MH_HIP(hipHostMalloc(&c->h_fhits, sizeof(uint64_t), hipHostMallocDefault));
#ifdef MH_DEV_HOOKS
    c->keep = 0;  // mh_search_first_hits refused the hash hooks; nothing of an earlier search's stays
    c->keep_fast = c->xor_on = c->xor_fast = false;
#endif
    const uint64_t slots = hits_slots();
    const uint64_t total_m1 = upper - lower;  // the range's size minus 1 (its size may be 2^64)
    MH_HIP(hipMemsetAsync(c->d_best, 0xFF, sizeof(Partial), c->stream));
    MH_HIP(hipMemsetAsync(c->d_hcursor, 0, sizeof(uint64_t), c->stream));
    MH_HIP(hipMemsetAsync(c->d_fhits, 0xFF, sizeof(uint64_t), c->stream));
    MH_HIP(hipMemsetAsync(c->d_fhits + 1, 0, sizeof(uint64_t), c->stream));
    MH_HIP(hipMemsetAsync(c->d_slices, 0, sizeof(uint32_t) * mh::kFirstHitsSlices, c->stream));
    const mh::PlanOpts opt = plan_opts();
    if (opt.queue) MH_HIP(hipMemsetAsync(c->d_counters, 0, sizeof(uint32_t) * kQueueSlots, c->stream));
    c->qoff = 0;
    bool any_coarse = false, any_fine = false;
    if (opt.streams == 2)
        mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
            (coarse_piece(p, opt) ? any_coarse : any_fine) = true;
            return !(any_coarse && any_fine);
        });
    const bool split = opt.streams == 2 && any_coarse && any_fine;
    if (split) {
        rc = piece_streams_wait_main(c);
        if (rc) return rc;
    }
    const mh::HitsStopArgs hs{mh::HitsArgs{target, (unsigned long long*)c->d_hcursor, c->d_hits, slots},
                              (uint64_t)k,
                              (unsigned long long*)c->d_fhits,
                              c->d_slices,
                              lower,
                              total_m1,
                              mh::first_hits_shift(total_m1),
                              0u,
                              (unsigned long long*)(c->d_fhits + 1)};
    int err = MH_OK;
    c->poff = 0;
    c->hits_stop = &hs;
    mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
        err = enqueue_piece(c, p, opt, split);
        return err == MH_OK;
    });
    c->hits_stop = nullptr;
    if (!err) err = flush_partials(c, split);
    if (err) {
        for (auto ps : c->ps)
            if (ps) (void)hipStreamSynchronize(ps);
        (void)hipStreamSynchronize(c->stream);
        return err;
    }
    MH_HIP(hipMemcpyAsync(c->h_best, c->d_best, sizeof(Partial), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipMemcpyAsync(c->h_hcursor, c->d_hcursor, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipMemcpyAsync(c->h_fhits, c->d_fhits + 1, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    if (c->prof) {
        rc = harvest_locked(c);
        if (rc) return rc;
    }
    const uint64_t appended = *c->h_hcursor, scanned = *c->h_fhits;
    const Partial best = *c->h_best;  // the window walk below reuses the pinned words
    std::vector<mh::Hit> got;
    if (appended <= slots) {
        got.resize((size_t)appended);
        if (!got.empty()) MH_HIP(hipMemcpy(got.data(), c->d_hits, got.size() * sizeof(mh::Hit), hipMemcpyDeviceToHost));
        std::sort(got.begin(), got.end(), hit_by_nonce);
    } else {  // the buffer dropped entries: rebuild the list window by window, from the observed density
        rc = hits_window_walk(c, pre, lower, upper, target, slots, k, std::max(1.0, (double)scanned) / (double)appended, &got,
                              widen_walk);
        if (rc) return rc;
    }
    out->stored = std::min<uint64_t>(got.size(), k);
    out->scanned = scanned;
    if (out->stored < k) {
        // fewer than k hits: the bound was never lowered, so nothing was skipped
        if (scanned != total_m1 + 1u)
            return fail(MH_EINTERNAL, "internal: fewer than k hits, but the scan did not hash the whole range");
        out->hash = best.hash;
        out->nonce = best.nonce;
    } else {
        out->hash = got[0].hash;
        out->nonce = got[0].nonce;
        for (size_t i = 1; i < k; ++i)
            if (got[i].hash < out->hash || (got[i].hash == out->hash && got[i].nonce < out->nonce)) {
                out->hash = got[i].hash;
                out->nonce = got[i].nonce;
            }
    }
    for (uint64_t i = 0; i < out->stored; ++i) hits[i] = mh_hit{got[(size_t)i].hash, got[(size_t)i].nonce};
    return MH_OK;
}

int check_common(const uint8_t* msg, size_t len) {
    if (msg == nullptr && len != 0) return fail(MH_EINVAL, "msg is NULL");
    if (len > MH_MAX_MSG_LEN) return fail(MH_ETOOLONG, "message longer than MH_MAX_MSG_LEN");
    return MH_OK;
}

// The first-hit and hits kernels have no variants of the dev build's hash hooks: their entry points
// (`name`, for the message) refuse the hooks, never ignore them.
int refuse_hash_hooks(const char* name) {
#ifdef MH_DEV_HOOKS
    for (const char* hook : {"MINEHIP_DEV_HASH_KEEP", "MINEHIP_DEV_HASH_XOR", "MINEHIP_DEV_CODE_OBJECT"})
        if (const char* e = getenv(hook))
            if (*e) return fail(MH_EINVAL, std::string(name) + " does not support " + hook);
#else
    (void)name;
#endif
    return MH_OK;
}

}  // namespace host
}  // namespace mh

using namespace mh::host;

extern "C" {

int mh_abi_version(void) { return MH_ABI_VERSION; }

int mh_device_count(void) { return device_count_impl(); }

const char* mh_last_error(void) { return g_err.c_str(); }

int mh_search(int dev, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t* out_hash,
              uint64_t* out_nonce) {
    g_err.clear();
    if (!out_hash || !out_nonce) return fail(MH_EINVAL, "NULL output pointer");
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    return search_impl(dev, pre, lower, upper, out_hash, out_nonce);
}

int mh_search_first(int dev, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t target,
                    mh_first* out) {
    return mh_search_first_ex(dev, msg, len, lower, upper, target, 0u, out);
}

int mh_search_first_ex(int dev, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t target,
                       uint32_t flags, mh_first* out) {
    g_err.clear();
    if (flags & ~MH_FIRST_STOP_RUNNING) return fail(MH_EINVAL, "unknown flag bit");
    if (!out) return fail(MH_EINVAL, "NULL output pointer");
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
    rc = refuse_hash_hooks("mh_search_first");
    if (rc) return rc;
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    return search_first_impl(dev, pre, lower, upper, target, flags, out);
}

int mh_search_hits(int dev, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t target,
                   mh_hit* hits, size_t cap, mh_hits* out) {
    g_err.clear();
    if (!out) return fail(MH_EINVAL, "NULL output pointer");
    if (cap > MH_HITS_MAX_CAP) return fail(MH_EINVAL, "cap is larger than MH_HITS_MAX_CAP");
    if (!hits && cap > 0) return fail(MH_EINVAL, "hits is NULL with cap > 0");
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
    rc = refuse_hash_hooks("mh_search_hits");
    if (rc) return rc;
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    return search_hits_impl(dev, pre, lower, upper, target, hits, cap, out);
}

int mh_search_first_hits(int dev, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t target,
                         mh_hit* hits, size_t k, mh_first_hits* out) {
    g_err.clear();
    if (!out) return fail(MH_EINVAL, "NULL output pointer");
    if (!hits) return fail(MH_EINVAL, "hits is NULL");
    if (k == 0) return fail(MH_EINVAL, "k is 0");
    if (k > MH_HITS_MAX_CAP) return fail(MH_EINVAL, "k is larger than MH_HITS_MAX_CAP");
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
    rc = refuse_hash_hooks("mh_search_first_hits");
    if (rc) return rc;
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    return search_first_hits_impl(dev, pre, lower, upper, target, hits, k, out);
}

int mh_first_hits_slices(uint64_t lower, uint64_t upper, uint32_t* shift, uint32_t* slices) {
    g_err.clear();
    if (!shift || !slices) return fail(MH_EINVAL, "NULL output pointer");
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
    *shift = mh::first_hits_shift(upper - lower);
    *slices = mh::first_hits_slices(upper - lower, *shift);
    return MH_OK;
}

uint64_t mh_first_hits_bound(uint64_t lower, uint64_t upper, uint64_t k, const uint32_t* counts) {
    if (!counts || k == 0 || lower > upper) return ~0ull;
    return mh::first_hits_bound(lower, upper - lower, mh::first_hits_shift(upper - lower), k, counts);
}

// The test hooks of the multi-device coordinators, dev build only (`make dev`, -DMH_DEV_HOOKS):
// MINEHIP_TEST_FAIL_WORKER=i makes worker i's searches fail with MH_EHIP, to exercise the
// hand-back path on a one-GPU box; MINEHIP_TEST_SPAWN_LIMIT=k makes the host thread of every worker
// after the first k fail to start (std::system_error, as when the process is out of threads), so
// the start-failure path of the coordinators runs on any box.
static void multi_test_hooks(int* fail_worker, mh::ThreadStart* start) {
#ifdef MH_DEV_HOOKS
    if (const char* e = getenv("MINEHIP_TEST_FAIL_WORKER")) *fail_worker = atoi(e);
    if (const char* e = getenv("MINEHIP_TEST_SPAWN_LIMIT")) {
        auto started = std::make_shared<std::atomic<int>>(0);
        const int limit = atoi(e);
        *start = [started, limit](std::function<void()> fn) {
            if ((*started)++ >= limit)
                throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again));
            return std::thread(std::move(fn));
        };
    }
#else
    (void)fail_worker;
    (void)start;
#endif
}

int mh_search_multi(const int* devs, int ndev, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper,
                    uint64_t chunk, uint64_t* out_hash, uint64_t* out_nonce) {
    g_err.clear();
    if (!out_hash || !out_nonce || !devs || ndev <= 0) return fail(MH_EINVAL, "bad arguments");
    if (ndev > MH_MAX_WORKERS) return fail(MH_EINVAL, "more than MH_MAX_WORKERS devices listed");
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
    const int n = mh_device_count();
    for (int i = 0; i < ndev; ++i)
        if (devs[i] < 0 || devs[i] >= n) return fail(n <= 0 ? MH_ENODEV : MH_EINVAL, "device index out of range");
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    int fail_worker = -1;
    mh::ThreadStart start;
    multi_test_hooks(&fail_worker, &start);
    // One device and adaptive chunks: nothing to balance, so one search (one
    // plan, full-size launches) instead of a chain of shrinking chunks.
    if (ndev == 1 && chunk == 0 && fail_worker < 0 && !start)
        return search_impl(devs[0], pre, lower, upper, out_hash, out_nonce);
    // Adaptive: one rate-weighted shard per device (+ a short dynamic tail on long ranges), multi.hpp.
    if (chunk == 0) {
        const mh::SpanSearch search = [&](int worker, int dev, uint64_t lo, uint64_t hi, uint64_t* h, uint64_t* n,
                                          uint64_t* ns, std::string* err) {
            const int r = (worker == fail_worker) ? fail(MH_EHIP, "injected failure (dev build test hook)")
                                                  : search_impl(dev, pre, lo, hi, h, n, ns);
            if (r) *err = g_err;  // this worker thread's description
            return r;
        };
        std::string err;
        const int r = mh::search_shards(devs, ndev, pre, lower, upper, plan_opts(), search, out_hash, out_nonce, &err,
                                        start);
        return r ? fail(r, err) : MH_OK;
    }
    // Fixed chunks: one miner per listed device, fed by the server's scheduler (sched.hpp) with
    // chunks of exactly `chunk` nonces (multi.cpp search_chunks).  A device that fails hands its
    // chunk back to the others.
    const mh::ChunkSearch csearch = [&](int worker, uint64_t lo, uint64_t hi, uint64_t* h, uint64_t* nn,
                                        std::string* err) {
        const int r = (worker == fail_worker) ? fail(MH_EHIP, "injected failure (dev build test hook)")
                                              : search_impl(devs[worker], pre, lo, hi, h, nn);
        if (r) *err = g_err;
        return r;
    };
    std::string err;
    const int r = mh::search_chunks(ndev, msg, len, lower, upper, chunk, csearch, out_hash, out_nonce, &err, start);
    return r ? fail(r, err) : MH_OK;
}

int mh_search_first_multi(const int* devs, int ndev, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper,
                          uint64_t target, uint64_t chunk, uint32_t flags, mh_first* out) {
    g_err.clear();
    if (flags & ~MH_FIRST_STOP_RUNNING) return fail(MH_EINVAL, "unknown flag bit");
    if (!out || !devs || ndev <= 0) return fail(MH_EINVAL, "bad arguments");
    if (ndev > MH_MAX_WORKERS) return fail(MH_EINVAL, "more than MH_MAX_WORKERS devices listed");
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
    rc = refuse_hash_hooks("mh_search_first_multi");
    if (rc) return rc;
    const int n = mh_device_count();
    for (int i = 0; i < ndev; ++i)
        if (devs[i] < 0 || devs[i] >= n) return fail(n <= 0 ? MH_ENODEV : MH_EINVAL, "device index out of range");
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    int fail_worker = -1;
    mh::ThreadStart start;
    multi_test_hooks(&fail_worker, &start);
    if (chunk == 0) {  // the scheduler's own init_chunk default (2^30); not tuned for this call
        mh_sched_opts o;
        mh_sched_default_opts(&o);
        chunk = o.init_chunk;
    }
    // One miner per listed device over a target job of the server's scheduler (multi.cpp
    // search_first_chunks): each takes the next chunk, in ascending order, and answers it as
    // mh_miner_handle answers a Request with a Target.
    const mh::FirstChunkSearch csearch = [&](int worker, uint64_t lo, uint64_t hi, uint64_t* h, uint64_t* nn,
                                             uint64_t* scanned, std::string* err) {
        mh_first f{};
        const int r = (worker == fail_worker) ? fail(MH_EHIP, "injected failure (dev build test hook)")
                                              : search_first_impl(devs[worker], pre, lo, hi, target, flags, &f);
        if (r) *err = g_err;
        *h = f.hash;
        *nn = f.nonce;
        *scanned = f.scanned;
        return r;
    };
    std::string err;
    uint64_t h = 0, nn = 0, scanned = 0;
    const int r = mh::search_first_chunks(ndev, msg, len, lower, upper, target, chunk, csearch, &h, &nn, &scanned, &err,
                                          start);
    if (r) return fail(r, err);
    out->found = h <= target ? 1 : 0;
    out->reserved = 0;
    out->hash = h;
    out->nonce = nn;
    out->scanned = scanned;
    return MH_OK;
}

int mh_profile_enable(int dev, int on) {
    g_err.clear();
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipStreamSynchronize(c->stream));
    rc = harvest_locked(c);  // timings of launches already recorded stay counted
    if (rc) return rc;
    if (on) {  // enabling starts a fresh count; disabling keeps the counts readable
        memset(c->cnt, 0, sizeof c->cnt);
        for (auto& v : c->var) v = VarStat();
    }
    c->prof = on != 0;
    return MH_OK;
}

int mh_profile_read(int dev, uint64_t* out, int n) {
    g_err.clear();
    if (!out || n < 0) return fail(MH_EINVAL, "bad arguments");
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->ready) {
        MH_HIP(hipStreamSynchronize(c->stream));
        rc = harvest_locked(c);
        if (rc) return rc;
    }
    for (int i = 0; i < n && i < 8; ++i) out[i] = c->cnt[i];
    return MH_OK;
}

int mh_profile_kernels(int dev, mh_kernel_stat* out, int cap) {
    g_err.clear();
    if (cap < 0 || (!out && cap > 0)) return fail(MH_EINVAL, "bad arguments");
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->ready) {
        MH_HIP(hipStreamSynchronize(c->stream));
        rc = harvest_locked(c);
        if (rc) return rc;
    }
    int n = 0;
    for (int i = 0; i < kVariants; ++i) {
        const VarStat& v = c->var[i];
        // (a fused batch launch of mixed lane lengths counts under its first piece's L, the
        // other pieces' nonces under theirs, with no launch of their own)
        if (!v.launches && !v.nonces) continue;
        if (n < cap) {
            out[n].word = i % 16;
            out[n].mode = (i / 16) % mh::kModes;
            out[n].lo_digits = i / (16 * mh::kModes) + 1;
            out[n].reserved = 0;
            out[n].launches = v.launches;
            out[n].nonces = v.nonces;
            out[n].ns = v.ns;
            out[n].ops = v.ops;
            out[n].slots = v.slots;
        }
        ++n;
    }
    return n;
}

int64_t mh_plan(const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, mh_piece* out, int64_t cap) {
    g_err.clear();
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    int64_t k = 0;
    const mh::PlanOpts opt = plan_opts();
    mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
        if (k >= cap) {
            ++k;  // cap + 1 signals truncation
            return false;
        }
        if (out) {
            mh_piece& q = out[k];
            q.first = p.first;
            q.count = p.count;
            q.kind = p.kind;
            q.digits = p.digits;
            q.lo_digits = p.L;
            q.word = p.J;
            q.mode = p.mode;
            q.blocks = p.blocks;
            q.nonce_ops = p.ops;
            q.nonce_slots = p.slots;
        }
        ++k;
        return true;
    });
    return k;
}

int64_t mh_multi_plan(const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, const double* weights,
                      int ndev, mh_span* out, int64_t cap) {
    g_err.clear();
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
    if (ndev <= 0 || ndev > MH_MAX_WORKERS || cap < 0) return fail(MH_EINVAL, "bad arguments");
    std::vector<double> w((size_t)ndev, 1.0);
    if (weights)
        for (int i = 0; i < ndev; ++i) {
            if (!(weights[i] > 0.0) || !std::isfinite(weights[i])) return fail(MH_EINVAL, "weights must be finite and > 0");
            w[(size_t)i] = weights[i];
        }
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    mh::MultiPlan mp;
    mh::multi_plan(pre, lower, upper, plan_opts(), w, &mp);
    int64_t k = 0;
    auto put = [&](const mh::Span& s, int worker, int kind) {
        if (k < cap && out) {
            out[k].lower = s.lo;
            out[k].upper = s.hi;
            out[k].worker = worker;
            out[k].kind = kind;
            out[k].cost = mh::segments_cost(mp.segs, s.lo, s.hi);
        }
        ++k;
    };
    for (int i = 0; i < ndev; ++i)
        if (!mp.head[(size_t)i].empty) put(mp.head[(size_t)i], i, 0);
    for (const auto& s : mp.tail) put(s, -1, 1);
    return k;
}

int mh_multi_rates(const int* devs, int ndev, double* out) {
    g_err.clear();
    if (ndev < 0 || (ndev > 0 && (!devs || !out))) return fail(MH_EINVAL, "bad arguments");
    for (int i = 0; i < ndev; ++i) out[i] = mh::device_rate(devs[i]);
    return MH_OK;
}

}  // extern "C"

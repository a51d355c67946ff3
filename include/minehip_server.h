/*
 * minehip_server.h -- the caller side of the nonce search: the bitcoin
 * server's scheduler, exported by libminehip.so.
 *
 * Reference: bitcoin/server/server.go:12-20 (the server owns an lsp.Server)
 * and :62 ("TODO: implement this!") -- a stub.  Its job, per the CMU 15-440
 * P1 handout the stub belongs to:
 *   - miners connect and send Join (bitcoin/message.go:47-49);
 *   - a client sends Request{Data, Lower, Upper} (message.go:27-34);
 *   - the server splits [Lower, Upper] into chunks, hands each chunk to an
 *     idle miner as a Request, and merges the miners' Results
 *     (message.go:38-44) by the lexicographic min of (Hash, Nonce) -- the same
 *     associative merge as the miner's scan (miner.go:33 spec);
 *   - when every chunk is back it writes Result to the client;
 *   - a lost miner's chunk is handed to another miner, a lost client's job
 *     is dropped (lsp/server_api.go:7-17: Read returns the lost connID).
 *
 * Two layers, both transport-agnostic (no sockets: the LSP transport stays the
 * reference's, lsp/server_api.go):
 *   mh_sched_*   the scheduling state machine (jobs, chunks, miners);
 *   mh_server_*  the server's message loop on top of it: feed it every
 *                (connID, payload) that lsp.Server.Read returns, or the lost
 *                connID, and write out what mh_server_pop_write yields.
 * Every call is thread-safe (one internal mutex per object).  Times are
 * caller-supplied monotonic nanoseconds, so the schedule is deterministic
 * under test.  Return codes are those of minehip.h (mh_last_error explains).
 */
#ifndef MINEHIP_SERVER_H
#define MINEHIP_SERVER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Chunk sizing.  A miner's chunk is rate x target_ns, where rate is the
 * miner's measured nonces/ns (EWMA over its completed chunks; init_chunk
 * before the first one), capped at a fair share of the work left
 * (remaining / (2 x miners): guided self-scheduling, so the tail of a job is
 * spread over every miner) and clamped to [min_chunk, max_chunk]. */
typedef struct mh_sched_opts {
    uint64_t init_chunk; /* default 2^30: ~33 ms on one MI355X              */
    uint64_t min_chunk;  /* default 2^24                                     */
    uint64_t max_chunk;  /* default 2^38                                     */
    uint64_t target_ns;  /* default 250 ms per chunk                         */
} mh_sched_opts;

/* Defaults as documented above. */
void mh_sched_default_opts(mh_sched_opts *o);

typedef struct mh_sched mh_sched;

/* NULL opts = defaults.  Returns NULL on bad options (min > max, zero sizes). */
mh_sched *mh_sched_create(const mh_sched_opts *opts);
void mh_sched_destroy(mh_sched *s);

/* Queueing.  A miner holds a FIFO of up to `depth` outstanding chunks, so that the small Requests
 * of many clients reach it together and run as one fused batch (mh_miner_handle_batch).  A miner
 * with q chunks out may be handed another iff q == 0, or q < depth and the nonces it holds are
 * fewer than its budget: rate x queue_ns (init_chunk before the first rate sample).  The new
 * chunk is sized as above and is not cut to the budget, so a chunk of a large job (rate x
 * target_ns) fills the budget alone: large jobs are scheduled as at depth 1, small ones stack up.
 * (The last chunks of a large job are the exception: the fair-share cap cuts them smaller than the
 * budget, so several of them may queue on one miner, handed out fewest-first.)
 * A Result carries no id: it completes the miner's oldest chunk (LSP delivers in order and a
 * miner answers in arrival order).  With depth > 1 a Result is accepted only if its nonce lies in
 * that chunk and Hash(job's Data, nonce) == hash, computed on the host; see mh_sched_result. */
#define MH_SCHED_MAX_DEPTH 64 /* = the most payloads minehip-miner takes for one batch */
typedef struct mh_sched_queue_opts {
    uint32_t depth, reserved; /* most chunks one miner holds at once, 1..MH_SCHED_MAX_DEPTH; default 1 */
    uint64_t queue_ns;        /* work one miner may hold, as time at its measured rate; 0 = target_ns */
} mh_sched_queue_opts;

/* depth 1, queue_ns 0. */
void mh_sched_default_queue_opts(mh_sched_queue_opts *q);

/* mh_sched_create with queue options; NULL q = defaults, which is mh_sched_create itself.  NULL
 * (MH_EINVAL) also for depth 0 or above MH_SCHED_MAX_DEPTH, or reserved != 0. */
mh_sched *mh_sched_create_ex(const mh_sched_opts *opts, const mh_sched_queue_opts *q);

/* A miner joined (message.go:47 Join).  MH_EINVAL if the id is already known. */
int mh_sched_add_miner(mh_sched *s, int64_t miner);

/* A miner was lost: every chunk it holds goes back to the front of its job, the oldest first.
 * MH_EINVAL if the id is unknown. */
int mh_sched_remove_miner(mh_sched *s, int64_t miner);

/* A client's Request: returns the new job id (>= 0) or MH_E*. */
int64_t mh_sched_submit(mh_sched *s, int64_t client, const uint8_t *msg, size_t len, uint64_t lower,
                        uint64_t upper);

/* ---- target jobs: the proof-of-work question (mh_search_first) through the scheduler ----
 *
 * A client's Request with a Target (minehip.h mh_message_ex): the answer is the smallest nonce n
 * of [lower, upper] with Hash(msg, n) <= target and its hash, or the range's minimum when no nonce
 * qualifies -- exactly mh_search_first's found / hash / nonce, with found = (hash <= target).
 * Returns the new job id (>= 0) or MH_E*.  A job from mh_sched_submit behaves as it always did.
 *   Hand-out order.  The pending chunk with the lowest nonces goes out first: requeued chunks in
 *     ascending order of their first nonce (they always lie below the fresh nonces), then fresh
 *     nonces.  Sizing, round-robin over jobs, eligibility and queue depth are unchanged.
 *   Results.  A Result with hash <= target is a hit at its nonce; the job keeps the hit with the
 *     smallest nonce, b.  A Result without a hit feeds the lexicographic minimum.
 *   Once a hit is known, nothing above b is handed out: the fresh remainder is dropped, requeued
 *     chunks that start above b are dropped, and a lost miner's chunk that starts above b is not
 *     requeued.
 *   Completion.  The job completes the moment a hit exists and no pending or outstanding chunk
 *     starts below b; mh_completion's hash / nonce are the hit at b.  It does not wait for the
 *     chunks still out above the hit (the protocol has no message to recall them): the job stays
 *     on, finished and draining, until they are back, and their late Results are validated as any
 *     other, counted off and ignored (mh_sched_result returns 0).  Without a hit the job completes
 *     when every chunk is back, with the minimum.
 *   Validation of Results is unchanged (nonce in the chunk; at depth > 1 the host Hash check that
 *     removes the miner); MH_ERANGE / MH_EREJECTED on a chunk of a finished job only counts it off.
 * Why the answer is mh_search_first's whatever the chunking, the order, the depth or the losses:
 * let n* be the smallest qualifying nonce of the range and C the chunk that holds it.  C's miner
 * returns n*, the smallest qualifying nonce in C; every reported hit is >= n*; and the job cannot
 * complete on a hit b > n* while C is pending or out, because C's first nonce <= n* < b.
 * This needs every miner to answer a chunk that carries a Target as mh_miner_handle does: with the
 * chunk's FIRST hit.  A reference Go miner ignores the key and returns the chunk's minimum -- a hit
 * if the chunk has one, but not necessarily its first.  In a mixed cluster the job still completes
 * with a qualifying nonce whenever one exists, but not always the smallest. */
int64_t mh_sched_submit_first(mh_sched *s, int64_t client, const uint8_t *msg, size_t len, uint64_t lower,
                              uint64_t upper, uint64_t target);

/* *has_target = 1 and *target for a job from mh_sched_submit_first, 0 and 0 for one from
 * mh_sched_submit: what the server needs to encode the chunk Requests (mh_assignment does not
 * carry it).  MH_EINVAL for an unknown job or a NULL pointer. */
int mh_sched_job_target(mh_sched *s, int64_t job, int *has_target, uint64_t *target);

/* A client was lost: its jobs are cancelled; chunks already out are ignored
 * when they come back.  Returns the number of jobs cancelled. */
int mh_sched_drop_client(mh_sched *s, int64_t client);

/* One chunk to send as a Request to a miner. */
typedef struct mh_assignment {
    int64_t miner, job;
    uint64_t lower, upper; /* inclusive */
    size_t msg_len;        /* the job's Data: mh_sched_job_msg */
} mh_assignment;

/* Hand one chunk to a miner that may take one (idle; with depth > 1 see "Queueing" above):
 * `miner` = a specific miner, or -1 for the eligible miner with the fewest chunks out (ties in
 * join order, so every miner gets its first chunk before any gets a second; jobs served
 * round-robin in submission order).  Returns 1 and fills *out, or 0 when no eligible miner / no
 * pending chunk. */
int mh_sched_next(mh_sched *s, int64_t miner, uint64_t now_ns, mh_assignment *out);

/* Host only: the chunks `miner` holds, oldest first, into out[0..cap); returns their count, or
 * cap + 1 when there are more than cap (out holds the first cap).  MH_EINVAL if the id is unknown. */
int64_t mh_sched_miner_queue(mh_sched *s, int64_t miner, mh_assignment *out, int64_t cap);

/* Copy job `job`'s Data into buf (cap bytes); *len receives its size. */
int mh_sched_job_msg(mh_sched *s, int64_t job, uint8_t *buf, size_t cap, size_t *len);

/* A job whose every chunk is back. */
typedef struct mh_completion {
    int64_t job, client;
    uint64_t hash, nonce;
} mh_completion;

/* A miner's Result for its oldest outstanding chunk.  Returns 1 when that finished
 * its job (*out filled), 0 otherwise.  MH_EINVAL: the miner has no chunk out;
 * MH_ERANGE (depth 1): nonce outside the chunk (the chunk is requeued, the miner idle).
 * MH_EREJECTED (depth > 1): nonce outside the chunk, or hash != Hash(job's Data, nonce) -- the
 * miner skipped or reordered an answer, so its later Results would be credited to the wrong
 * chunks: it is removed as if lost (every chunk it holds is requeued) and the caller should close
 * its connection. */
int mh_sched_result(mh_sched *s, int64_t miner, uint64_t hash, uint64_t nonce, uint64_t now_ns,
                    mh_completion *out);

typedef struct mh_sched_stats {
    uint64_t miners, idle_miners;
    uint64_t jobs;           /* live (incl. cancelled with chunks still out) */
    uint64_t chunks_assigned, chunks_done, chunks_requeued;
    uint64_t nonces_done;    /* nonces of completed chunks */
    uint64_t jobs_done, jobs_cancelled;
} mh_sched_stats;

int mh_sched_stats_read(mh_sched *s, mh_sched_stats *out);

/* Counters of the target jobs (mh_sched_stats itself does not grow). */
typedef struct mh_sched_first_stats {
    uint64_t jobs_first;      /* jobs from mh_sched_submit_first */
    uint64_t jobs_found;      /* of those, completed with a hit */
    uint64_t nonces_dropped;  /* nonces never handed out because they lay above a hit */
    uint64_t results_ignored; /* late Results of finished jobs */
} mh_sched_first_stats;

int mh_sched_first_stats_read(mh_sched *s, mh_sched_first_stats *out);

/* ---- the server loop (server.go:62 TODO) ------------------------------ */

typedef struct mh_server mh_server;

mh_server *mh_server_create(const mh_sched_opts *opts);
/* The same over mh_sched_create_ex's scheduler (NULL q = depth 1). */
mh_server *mh_server_create_ex(const mh_sched_opts *opts, const mh_sched_queue_opts *q);
void mh_server_destroy(mh_server *v);

/* lsp.Server.Read returned (conn, payload, nil).  Join registers a miner,
 * Request submits a job for the client `conn`, Result completes the miner's
 * chunk.  Queues the resulting writes.  MH_EINVAL for a payload that is not a
 * Message, or a Result from a connection with no chunk out.  MH_EREJECTED for
 * a client Request that can never be answered (Lower > Upper, Data longer
 * than MH_MAX_MSG_LEN): nothing is queued, and the caller should close that
 * connection (lsp.Server.CloseConn) so the client sees it end instead of
 * waiting forever for a Result.  MH_EREJECTED also for a miner's Result that
 * mh_sched_result refused at depth > 1: the miner is gone from the server and
 * its chunks are handed out again; close that connection too.
 * A client Request with a Target becomes a target job (mh_sched_submit_first): its chunk Requests
 * carry the Target, and the client gets a plain Result -- the first hit, or the minimum when
 * nothing qualifies; the client tells them apart by hash <= target. */
int mh_server_read(mh_server *v, int64_t conn, const char *payload, size_t len, uint64_t now_ns);

/* lsp.Server.Read returned (conn, nil, err): the connection is lost. */
int mh_server_lost(mh_server *v, int64_t conn, uint64_t now_ns);

/* Next queued lsp.Server.Write(conn, payload): returns 1 and fills it, 0 when
 * the queue is empty, MH_EINVAL when cap is short (*len = needed size; the
 * write stays queued). */
int mh_server_pop_write(mh_server *v, int64_t *conn, char *out, size_t cap, size_t *len);

int mh_server_stats(mh_server *v, mh_sched_stats *out);
int mh_server_first_stats(mh_server *v, mh_sched_first_stats *out);

#ifdef __cplusplus
}
#endif

#endif /* MINEHIP_SERVER_H */

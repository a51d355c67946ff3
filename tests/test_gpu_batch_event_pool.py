"""A profiled mh_search_batch of more passes than the profile has event pairs (kEventPairs = 512 in
csrc/host_ctx.hpp): the pass that finds the pool full drains first -- results so far copied out,
timings harvested -- and the batch goes on.  Nothing else reaches that drain of a batch pass."""
import pytest

pytestmark = pytest.mark.gpu

EVENT_PAIRS = 512
N = EVENT_PAIRS + 1     # the smallest count with a pass per request that fills the pool: pass 513 drains
NONCES = 10_000         # 1,000 whole decades from a multiple of 10: 4 tiles of 256 decades


def test_profiled_batch_with_more_passes_than_event_pairs(gpu, monkeypatch):
    """513 requests of 10^4 nonces under MINEHIP_BATCH_SLOTS=4, a pass per request.  Every result is
    search()'s of the same request.  The profile has no launch counter for the generic class; its
    nonce counter is added to once per pass, by the pass's planned nonces, so a rise of exactly
    513 x 10^4 is every pass counted once, the drained ones and the one after the drain included."""
    reqs = [(b"pool%d" % (i % 7), NONCES * i, NONCES * i + NONCES - 1) for i in range(N)]
    want = [gpu.search(*r) for r in reqs]
    monkeypatch.setenv("MINEHIP_BATCH_SLOTS", "4")
    plan = gpu.batch_plan(reqs)
    assert [(it["req"], it["kind"], it["pass"], it["slots"]) for it in plan] == [(i, 0, i, 4) for i in range(N)]
    passes = 1 + max(it["pass"] for it in plan)
    assert passes == N > EVENT_PAIRS
    gpu.profile_enable(0, True)
    try:
        before = gpu.profile_read(0)
        got = gpu.search_batch(reqs)
        after = gpu.profile_read(0)
    finally:
        gpu.profile_enable(0, False)
    assert got == want
    assert after["generic_nonces"] - before["generic_nonces"] == passes * NONCES
    assert after["generic_ns"] > before["generic_ns"]
    assert after["fast_launches"] == before["fast_launches"] == 0

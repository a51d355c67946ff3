// batch_fast_host.cpp -- the host plan and table checks of mh_search_batch_ex(MH_BATCH_FUSE_FAST)
// (bitcoin-miner_amd/csrc/plan.cpp: plan_batch_ex, build_batch_tables_ex, batch_tables_ex_ok),
// driven on the host, to be built with -fsanitize=address,undefined (tests/test_batch_fast_plan.py).
// No HIP.
//
//   batch_fast_host <seed> <batches>
//
// Per random batch (messages of 0..129 bytes, 1..20 digits, ranges of up to 3 * 10^8 nonces, one at
// the top of u64), under both lane rules, small min_lanes, no Early layouts and a small slot
// capacity in turn: the tables of every pass pass the check, and tables corrupted on purpose -- an
// item's slot, chunk offset or run count, a chunk's item, an entry's slot, one slot too few of
// capacity -- are refused.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../../bitcoin-miner_amd/csrc/plan.hpp"

using namespace mh;

static int failures = 0;
static void fail(const char* what, int batch, int pass) {
    ++failures;
    printf("%s (batch %d, pass %d)\n", what, batch, pass);
}

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 440;
    const int batches = argc > 2 ? atoi(argv[2]) : 60;
    std::mt19937_64 rng(seed);
    size_t npass = 0, nitems = 0;
    for (int it = 0; it < batches; ++it) {
        const size_t n = 1 + rng() % 50;
        std::vector<BatchRequest> reqs(n);
        for (size_t i = 0; i < n; ++i) {
            const std::string m(rng() % 130, (char)('a' + rng() % 26));
            absorb_prefix((const uint8_t*)m.data(), m.size(), &reqs[i].pre);
            const int d = 1 + (int)(rng() % 20);
            uint64_t lo = 1;
            for (int k = 1; k < d; ++k) lo *= 10;
            lo += rng() % lo;
            const uint64_t span = rng() % 4 == 0 ? rng() % 3000 : rng() % 3 == 0 ? rng() % 300000000ull : rng() % 6000000;
            uint64_t hi = lo + span < lo ? ~0ull : lo + span;
            if (i == 0 && it % 7 == 0) {
                lo = ~0ull - 3000000;
                hi = ~0ull;
            }
            reqs[i].lower = lo;
            reqs[i].upper = hi;
            reqs[i].id = i;
        }
        PlanOpts opt;
        if (it % 3 == 1) opt.min_lanes = 16;
        if (it % 5 == 2) opt.early = 0;
        const uint32_t cap = it % 4 == 3 ? 700u : kMaxBlocksPerLaunch;
        std::vector<BatchPiece> pieces;
        std::vector<FastArgs> args;
        plan_batch_ex(reqs.data(), n, opt, cap, it % 2 == 0, kBatchFastMaxNonces, &pieces, &args);
        int passes = 0;
        for (const BatchPiece& p : pieces)
            if (p.kind != 1) passes = std::max(passes, p.pass + 1);
        BatchTables t;
        BatchFastTables f;
        for (int p = 0; p < passes; ++p) {
            build_batch_tables_ex(reqs.data(), pieces, args, p, &t, &f);
            ++npass;
            nitems += f.items.size();
            if (!batch_tables_ex_ok(t, f, cap)) fail("good tables refused", it, p);
            if (!f.items.empty()) {
                BatchFastTables g = f;
                g.items[0].slot0 += 1;
                if (batch_tables_ex_ok(t, g, cap)) fail("an item's slot0 off by one accepted", it, p);
                g = f;
                g.chunk_item.back() = (uint32_t)g.items.size();
                if (batch_tables_ex_ok(t, g, cap)) fail("a chunk of no item accepted", it, p);
                g = f;
                g.items[0].args.n_runs += 256;
                if (batch_tables_ex_ok(t, g, cap)) fail("an item with more runs than chunks accepted", it, p);
                g = f;
                g.items[0].chunk0 += 1;
                if (batch_tables_ex_ok(t, g, cap)) fail("an item's chunk0 off by one accepted", it, p);
                if (batch_tables_ex_ok(t, f, (uint32_t)(t.tile_entry.size() + f.chunk_item.size() - 1)))
                    fail("more slots than the capacity accepted", it, p);
            }
            if (!t.entries.empty()) {
                BatchTables u = t;
                u.entries[0].slot0 += 1;
                if (batch_tables_ex_ok(u, f, cap)) fail("an entry's slot0 off by one accepted", it, p);
            }
        }
    }
    printf("passes=%zu items=%zu failures=%d\n", npass, nitems, failures);
    return failures != 0;
}

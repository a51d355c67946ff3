// cli.cpp -- native command-line front ends of libminehip (C++ callers of the
// C-ABI in include/minehip.h; no Python, no torch).
//
//   minehip-search <message> <maxNonce> [lower [target [cap [first]]]]
//       scans [lower (default 0), maxNonce] on every visible GPU and prints
//       "Result <hash> <nonce>" -- the output format of the reference client
//       (bitcoin/client/client.go:41-43), whose argument convention
//       (client.go:12-19: <message> <maxNonce>) it follows minus the hostport.
//       With a target (no reference counterpart): the smallest nonce of the range
//       whose hash is <= target, on device 0 (mh_search_first): "First <hash> <nonce>",
//       or "None <hash> <nonce>" with the range's minimum when no nonce qualifies.
//       With a target and a cap: every nonce of the range whose hash is <= target, on device 0
//       (mh_search_hits): "Hits <count> <min hash> <min nonce>", then one "<hash> <nonce>" line
//       for each of the min(count, cap) smallest of them, in increasing nonce order.
//       With the literal word "first" after the cap, here k: the k smallest such nonces from a scan
//       that stops once they are known (mh_search_first_hits): "FirstHits <stored> <hash> <nonce>",
//       then one "<hash> <nonce>" line per entry; k is 1..MH_HITS_MAX_CAP.
//
// The miner, server and client processes over LSP are apps/*_main.cpp.
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/minehip.h"

namespace {

bool parse_u64(const char* s, uint64_t* out) {  // strconv.ParseUint(s, 10, 64)
    if (!s || !*s) return false;
    for (const char* p = s; *p; ++p)
        if (*p < '0' || *p > '9') return false;
    errno = 0;
    char* end = nullptr;
    const unsigned long long v = strtoull(s, &end, 10);
    if (errno == ERANGE || *end) return false;
    *out = v;
    return true;
}

std::vector<int> all_devices() {
    std::vector<int> d;
    for (int i = 0; i < mh_device_count(); ++i) d.push_back(i);
    return d;
}

int run_search(int argc, char** argv) {
    if (argc < 3 || argc > 7 || (argc == 7 && strcmp(argv[6], "first") != 0)) {
        printf("Usage: ./%s <message> <maxNonce> [lower [target [cap [first]]]]", argv[0]);
        return 2;
    }
    uint64_t hi = 0, lo = 0, target = 0, cap = 0;
    if (!parse_u64(argv[2], &hi)) {
        printf("%s is not a number.\n", argv[2]);
        return 2;
    }
    if (argc >= 4 && !parse_u64(argv[3], &lo)) {
        printf("%s is not a number.\n", argv[3]);
        return 2;
    }
    if (argc >= 5 && !parse_u64(argv[4], &target)) {
        printf("%s is not a number.\n", argv[4]);
        return 2;
    }
    if (argc >= 6 && !parse_u64(argv[5], &cap)) {
        printf("%s is not a number.\n", argv[5]);
        return 2;
    }
    if (argc == 7 && (cap < 1 || cap > MH_HITS_MAX_CAP)) {
        printf("k is 1 to %u.\n", MH_HITS_MAX_CAP);
        return 2;
    }
    const std::vector<int> devs = all_devices();
    if (devs.empty()) {
        fprintf(stderr, "minehip: no HIP device\n");
        return 1;
    }
    if (argc == 7) {
        std::vector<mh_hit> hits((size_t)cap);
        mh_first_hits r;
        if (mh_search_first_hits(0, (const uint8_t*)argv[1], strlen(argv[1]), lo, hi, target, hits.data(), (size_t)cap,
                                 &r) != MH_OK) {
            fprintf(stderr, "minehip: %s\n", mh_last_error());
            return 1;
        }
        printf("FirstHits %llu %llu %llu\n", (unsigned long long)r.stored, (unsigned long long)r.hash,
               (unsigned long long)r.nonce);
        for (uint64_t i = 0; i < r.stored; ++i)
            printf("%llu %llu\n", (unsigned long long)hits[(size_t)i].hash, (unsigned long long)hits[(size_t)i].nonce);
        return 0;
    }
    if (argc == 6) {
        if (cap > MH_HITS_MAX_CAP) {
            printf("cap is at most %u.\n", MH_HITS_MAX_CAP);
            return 2;
        }
        std::vector<mh_hit> hits((size_t)cap);
        mh_hits r;
        if (mh_search_hits(0, (const uint8_t*)argv[1], strlen(argv[1]), lo, hi, target, cap ? hits.data() : nullptr,
                           (size_t)cap, &r) != MH_OK) {
            fprintf(stderr, "minehip: %s\n", mh_last_error());
            return 1;
        }
        printf("Hits %llu %llu %llu\n", (unsigned long long)r.count, (unsigned long long)r.hash,
               (unsigned long long)r.nonce);
        for (uint64_t i = 0; i < r.stored; ++i)
            printf("%llu %llu\n", (unsigned long long)hits[(size_t)i].hash, (unsigned long long)hits[(size_t)i].nonce);
        return 0;
    }
    if (argc == 5) {
        mh_first f;
        if (mh_search_first(0, (const uint8_t*)argv[1], strlen(argv[1]), lo, hi, target, &f) != MH_OK) {
            fprintf(stderr, "minehip: %s\n", mh_last_error());
            return 1;
        }
        printf("%s %llu %llu\n", f.found ? "First" : "None", (unsigned long long)f.hash, (unsigned long long)f.nonce);
        return 0;
    }
    uint64_t h = 0, n = 0;
    const int rc = mh_search_multi(devs.data(), (int)devs.size(), (const uint8_t*)argv[1], strlen(argv[1]), lo,
                                   hi, 0, &h, &n);
    if (rc != MH_OK) {
        fprintf(stderr, "minehip: %s\n", mh_last_error());
        return 1;
    }
    printf("Result %llu %llu\n", (unsigned long long)h, (unsigned long long)n);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    return run_search(argc, argv);
}

// miner_main.cpp -- minehip-miner: the GPU-backed miner process.
//
// Reference: bitcoin/miner/miner.go -- `miner <hostport>` (:18-24) joins the
// server (joinWithServer, :11-15: lsp.NewClient + Join, message.go:47-49),
// then (:33, TODO in the reference; spec SURVEY.md §8(a) A2) loops: Read a
// Request (message.go:27-34), scan [Lower, Upper], Write NewResult(hash,
// nonce) (message.go:38-44).  A Read error (server lost / closed) ends it.
// The scan is libminehip's mh_miner_handle over every visible GPU (one miner
// process per GPU: HIP_VISIBLE_DEVICES).  When more Requests are already queued
// on the connection (up to 64), they go together through
// mh_miner_handle_batch_ex -- the small ones in one fused GPU pass -- and their
// Results are written in arrival order.  A Request with a Target (minehip.h
// mh_message_ex: a chunk of one of the server's target jobs) is answered with
// the chunk's first hit, by the same two calls.  LSP is liblsp440 (wire compatible
// with the reference's lsp package, include/lsp440.h).
//
//   minehip-miner <hostport>     the miner over LSP
//   minehip-miner --stdio        the per-message step alone: one JSON
//                                Message per stdin line -> Result line
//
// Environment:
//   MINEHIP_MINER_FUSE_FAST=1    batches go through mh_miner_handle_batch_ex(MH_BATCH_FUSE_FAST): the
//                                fast pieces of queued Requests of up to 10^9 nonces fuse too
//   MINEHIP_MINER_STOP_RUNNING=1 Requests with a Target run through the stopping forms: one alone through
//                                mh_search_first_ex(MH_FIRST_STOP_RUNNING) (several devices:
//                                mh_search_first_multi with that flag), several together through one
//                                mh_search_first_batch_stop.  The same Results; off by default, like
//                                every stop-running form.
//   MINEHIP_MINER_STATS=1        on exit, one line to stderr:
//                                minehip-miner: requests=<n> batches=<n> largest=<n>
//                                (payloads read, handle calls made, most payloads in one call)
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <string>
#include <vector>

#include "../../../include/minehip.h"
#include "common.hpp"

namespace {

constexpr size_t kMaxBatch = 64;  // payloads taken from the connection's queue for one batch

bool env_on(const char* name) {
    const char* e = getenv(name);
    return e && !strcmp(e, "1");
}

std::vector<int> all_devices() {
    std::vector<int> d;
    for (int i = 0; i < mh_device_count(); ++i) d.push_back(i);
    return d;
}

int run_stdio(const std::vector<int>& devs) {
    std::string line;
    char out[256];
    while (std::getline(std::cin, line)) {
        size_t n = 0;
        const int rc = mh_miner_handle(devs.data(), (int)devs.size(), line.data(), line.size(), out, sizeof out, &n);
        if (rc == MH_ENOTREQ || rc == MH_ERANGE) continue;  // not a (valid) Request: ignored
        if (rc != MH_OK) {
            fprintf(stderr, "minehip: %s\n", mh_last_error());
            return 1;
        }
        fwrite(out, 1, n, stdout);
        fputc('\n', stdout);
        fflush(stdout);
    }
    return 0;
}

// mh_miner_handle_batch_ex for MINEHIP_MINER_STOP_RUNNING=1: the valid Requests with a Target are
// taken out and answered here through the stopping forms; every other payload goes through the
// library's step as always.  Outputs and return code as mh_miner_handle_batch_ex.
int handle_batch_stop(const std::vector<int>& devs, const char* const* ptrs, const size_t* lens, size_t k,
                      uint32_t flags, char* outs, size_t cap_each, size_t* olens, int* st) {
    std::vector<mh_message_ex> ms(k);
    std::vector<std::vector<uint8_t>> data(k);
    std::vector<size_t> tgt, plain;
    for (size_t i = 0; i < k; ++i) {
        data[i].resize(lens[i] + 16);  // Data is never longer than its payload
        const int rc = mh_msg_decode_ex(ptrs[i], lens[i], &ms[i], data[i].data(), data[i].size());
        const bool t = rc == MH_OK && ms[i].type == 1 && ms[i].has_target && ms[i].lower <= ms[i].upper;
        (t ? tgt : plain).push_back(i);
    }
    if (!plain.empty()) {
        const size_t n = plain.size();
        std::vector<const char*> p(n);
        std::vector<size_t> l(n), ol(n);
        std::vector<int> s(n);
        std::vector<char> o(n * cap_each);
        for (size_t j = 0; j < n; ++j) {
            p[j] = ptrs[plain[j]];
            l[j] = lens[plain[j]];
        }
        const int rc = mh_miner_handle_batch_ex(devs.data(), (int)devs.size(), p.data(), l.data(), n, flags, o.data(),
                                                cap_each, ol.data(), s.data());
        if (rc != MH_OK) return rc;
        for (size_t j = 0; j < n; ++j) {
            st[plain[j]] = s[j];
            olens[plain[j]] = ol[j];
            if (s[j] == MH_OK) memcpy(outs + plain[j] * cap_each, o.data() + j * cap_each, ol[j]);
        }
    }
    if (tgt.empty()) return MH_OK;
    std::vector<mh_first_result> res(tgt.size());
    if (tgt.size() == 1) {
        const mh_message_ex& m = ms[tgt[0]];
        mh_first f;
        const int rc = devs.size() == 1
                           ? mh_search_first_ex(devs[0], data[tgt[0]].data(), m.data_len, m.lower, m.upper, m.target,
                                                MH_FIRST_STOP_RUNNING, &f)
                           : mh_search_first_multi(devs.data(), (int)devs.size(), data[tgt[0]].data(), m.data_len, m.lower,
                                                   m.upper, m.target, 0, MH_FIRST_STOP_RUNNING, &f);
        if (rc != MH_OK) return rc;
        res[0] = mh_first_result{MH_OK, f.found, f.hash, f.nonce, f.scanned};
    } else {
        std::vector<mh_first_request> reqs;
        for (size_t i : tgt)
            reqs.push_back(mh_first_request{data[i].data(), ms[i].data_len, ms[i].lower, ms[i].upper, ms[i].target});
        const int rc = mh_search_first_batch_stop(devs[0], reqs.data(), reqs.size(), res.data());
        if (rc != MH_OK) return rc;
    }
    for (size_t j = 0; j < tgt.size(); ++j) {
        const size_t i = tgt[j];
        st[i] = res[j].status;
        if (st[i] == MH_OK)  // NewResult(hash, nonce)
            st[i] = mh_msg_encode(2, nullptr, 0, 0, 0, res[j].hash, res[j].nonce, outs + i * cap_each, cap_each, &olens[i]);
    }
    return MH_OK;
}

int run_lsp(const char* hostport, const std::vector<int>& devs) {
    const lsp_params p = apps::params_from_env();
    lsp_client* c = nullptr;
    int rc = lsp_client_new(hostport, &p, &c);  // joinWithServer (miner.go:11-15)
    if (rc != LSP_OK) {
        printf("Failed to join with server: %s\n", apps::lsp_strerror(rc));
        return 1;
    }
    char join[128];
    size_t jn = 0;
    mh_msg_encode(0, nullptr, 0, 0, 0, 0, 0, join, sizeof join, &jn);  // NewJoin()
    if (lsp_client_write(c, (const uint8_t*)join, jn) != LSP_OK) {
        lsp_client_close(c);
        return 1;
    }
    const uint32_t flags = env_on("MINEHIP_MINER_FUSE_FAST") ? (uint32_t)MH_BATCH_FUSE_FAST : 0u;
    const bool stop_running = env_on("MINEHIP_MINER_STOP_RUNNING");
    unsigned long long n_requests = 0, n_batches = 0, largest = 0;
    std::vector<uint8_t> buf(1 << 16);
    char out[256];
    int status = 0;
    std::vector<std::string> more;  // the payloads already queued behind the one just read
    for (;;) {
        size_t n = 0;
        rc = lsp_client_read(c, buf.data(), buf.size(), &n, -1);
        if (rc == LSP_ESHORT) {
            buf.resize(n);
            continue;
        }
        if (rc != LSP_OK) break;  // server lost or closed: the miner is done
        // What the connection already holds goes to the GPU as one batch (mh_miner_handle_batch_ex:
        // the small Requests in one fused pass) instead of one blocking search each.  A read that
        // finds nothing (or the connection's end, which the next blocking read reports) ends it.
        more.clear();
        while (more.size() + 1 < kMaxBatch) {
            std::vector<uint8_t> b2(4096);
            size_t n2 = 0;
            int r2 = lsp_client_read(c, b2.data(), b2.size(), &n2, 0);
            if (r2 == LSP_ESHORT) {
                b2.resize(n2);
                r2 = lsp_client_read(c, b2.data(), b2.size(), &n2, 0);
            }
            if (r2 != LSP_OK) break;
            more.emplace_back((const char*)b2.data(), n2);
        }
        n_requests += more.size() + 1;
        n_batches += 1;
        if (more.size() + 1 > largest) largest = more.size() + 1;
        if (more.empty() && !stop_running) {  // one payload: the single-request path
            size_t on = 0;
            const int hr = mh_miner_handle(devs.data(), (int)devs.size(), (const char*)buf.data(), n, out, sizeof out,
                                           &on);
            if (hr == MH_ENOTREQ || hr == MH_ERANGE) {  // not a Request, or Lower > Upper: no answer
                fprintf(stderr, "minehip-miner: ignored a message: %s\n", mh_last_error());
                continue;
            }
            if (hr != MH_OK) {  // the search failed: leave, so the server reassigns the chunk
                fprintf(stderr, "minehip-miner: %s\n", mh_last_error());
                status = 1;
                break;
            }
            if (lsp_client_write(c, (const uint8_t*)out, on) != LSP_OK) break;
            continue;
        }
        const size_t k = more.size() + 1;
        std::vector<const char*> ptrs(k);
        std::vector<size_t> lens(k), olens(k);
        std::vector<int> st(k);
        std::vector<char> outs(k * sizeof out);
        ptrs[0] = (const char*)buf.data();
        lens[0] = n;
        for (size_t i = 1; i < k; ++i) {
            ptrs[i] = more[i - 1].data();
            lens[i] = more[i - 1].size();
        }
        const int hr = stop_running
                           ? handle_batch_stop(devs, ptrs.data(), lens.data(), k, flags, outs.data(), sizeof out,
                                               olens.data(), st.data())
                           : mh_miner_handle_batch_ex(devs.data(), (int)devs.size(), ptrs.data(), lens.data(), k, flags,
                                                      outs.data(), sizeof out, olens.data(), st.data());
        bool stop = false;
        for (size_t i = 0; i < k && !stop && hr == MH_OK; ++i) {  // Results in arrival order
            if (st[i] == MH_ENOTREQ || st[i] == MH_ERANGE) {
                fprintf(stderr, "minehip-miner: ignored a message\n");
                continue;
            }
            if (st[i] != MH_OK) {
                fprintf(stderr, "minehip-miner: a request failed with %d\n", st[i]);
                status = 1;
                stop = true;
            } else if (lsp_client_write(c, (const uint8_t*)outs.data() + i * sizeof out, olens[i]) != LSP_OK) {
                stop = true;
            }
        }
        if (hr != MH_OK) {
            fprintf(stderr, "minehip-miner: %s\n", mh_last_error());
            status = 1;
            break;
        }
        if (stop) break;
    }
    lsp_client_close(c);
    if (env_on("MINEHIP_MINER_STATS"))
        fprintf(stderr, "minehip-miner: requests=%llu batches=%llu largest=%llu\n", n_requests, n_batches, largest);
    return status;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("Usage: ./%s <hostport>", argv[0]);  // miner.go:19-21
        return 2;
    }
    const std::vector<int> devs = all_devices();
    if (devs.empty()) {
        fprintf(stderr, "minehip: no HIP device\n");
        return 1;
    }
    if (!strcmp(argv[1], "--stdio")) return run_stdio(devs);
    return run_lsp(argv[1], devs);
}

// plan.cpp -- see plan.hpp.
#include "plan.hpp"

#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <cmath>

namespace mh {
namespace {

constexpr uint32_t kK[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
constexpr uint32_t kIV[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                             0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};

inline uint32_t ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

constexpr uint64_t kPow10[20] = {1ull,
                                 10ull,
                                 100ull,
                                 1000ull,
                                 10000ull,
                                 100000ull,
                                 1000000ull,
                                 10000000ull,
                                 100000000ull,
                                 1000000000ull,
                                 10000000000ull,
                                 100000000000ull,
                                 1000000000000ull,
                                 10000000000000ull,
                                 100000000000000ull,
                                 1000000000000000ull,
                                 10000000000000000ull,
                                 100000000000000000ull,
                                 1000000000000000000ull,
                                 10000000000000000000ull};

// big-endian byte i of a 32-word tail image
inline void put_byte(uint32_t* w, uint32_t pos, uint32_t v) { w[pos >> 2] |= v << (24u - 8u * (pos & 3u)); }

void schedule(const uint32_t w16[16], uint32_t w[64]) {
    for (int i = 0; i < 16; ++i) w[i] = w16[i];
    for (int i = 16; i < 64; ++i) {
        const uint32_t s0 = ror(w[i - 15], 7) ^ ror(w[i - 15], 18) ^ (w[i - 15] >> 3);
        const uint32_t s1 = ror(w[i - 2], 17) ^ ror(w[i - 2], 19) ^ (w[i - 2] >> 10);
        w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
}

}  // namespace

int decimal_digits(uint64_t n) {
    int d = 1;
    while (d < 20 && n >= kPow10[d]) ++d;
    return d;
}

void host_compress(uint32_t st[8], const uint32_t w16[16]) {
    uint32_t w[64];
    schedule(w16, w);
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    for (int i = 0; i < 64; ++i) {
        const uint32_t t1 = h + (ror(e, 6) ^ ror(e, 11) ^ ror(e, 25)) + ((e & f) ^ (~e & g)) + kK[i] + w[i];
        const uint32_t t2 = (ror(a, 2) ^ ror(a, 13) ^ ror(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g; g = f; f = e; e = d + t1;
        d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d;
    st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

void absorb_prefix(const uint8_t* msg, size_t len, Prefix* out) {
    memcpy(out->mid, kIV, sizeof kIV);
    out->plen = (uint64_t)len + 1u;
    const uint64_t nfull = out->plen / 64u;
    uint32_t w[16];
    for (uint64_t blk = 0; blk < nfull; ++blk) {
        for (int i = 0; i < 16; ++i) {
            uint32_t v = 0;
            for (int k = 0; k < 4; ++k) {
                const uint64_t p = blk * 64u + (uint64_t)(4 * i + k);
                const uint32_t byte = (p < len) ? msg[p] : (uint32_t)' ';
                v = (v << 8) | byte;
            }
            w[i] = v;
        }
        host_compress(out->mid, w);
    }
    out->t = (uint32_t)(out->plen % 64u);
    memset(out->tail, 0, sizeof out->tail);
    for (uint32_t i = 0; i < out->t; ++i) {
        const uint64_t p = nfull * 64u + i;
        out->tail[i] = (p < len) ? msg[p] : (uint8_t)' ';
    }
}

uint64_t host_hash(const uint8_t* msg, size_t len, uint64_t nonce) {
    Prefix pre;
    absorb_prefix(msg, len, &pre);
    uint8_t buf[128] = {0};  // tail (< 64) + digits (<= 20) + 0x80 + length (8): one or two blocks
    memcpy(buf, pre.tail, pre.t);
    const int d = decimal_digits(nonce);
    for (int i = d - 1; i >= 0; --i, nonce /= 10u) buf[pre.t + (uint32_t)i] = (uint8_t)('0' + nonce % 10u);
    const uint32_t used = pre.t + (uint32_t)d;
    buf[used] = 0x80;
    const uint32_t total = used + 9u <= 64u ? 64u : 128u;
    const uint64_t bits = (pre.plen + (uint64_t)d) * 8u;
    for (int i = 0; i < 8; ++i) buf[total - 1u - (uint32_t)i] = (uint8_t)(bits >> (8 * i));
    for (uint32_t blk = 0; blk < total; blk += 64u) {
        uint32_t w[16];
        for (int i = 0; i < 16; ++i) {
            const uint8_t* p = buf + blk + 4 * i;
            w[i] = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
        }
        host_compress(pre.mid, w);
    }
    return (uint64_t)pre.mid[0] << 32 | pre.mid[1];
}

void make_gen_args(const Prefix& pre, GenArgs* ga) {
    memset(ga, 0, sizeof *ga);
    memcpy(ga->mid, pre.mid, sizeof pre.mid);
    for (uint32_t i = 0; i < pre.t; ++i) put_byte(ga->tail, i, pre.tail[i]);
    ga->plen = pre.plen;
    ga->t = pre.t;
}

NonceCost nonce_cost(int J, int mode) {
    // Two counts of the same work:
    //   ops   VALU instructions with gfx950's 3-input ops (v_alignbit, v_bitop3, v_add3);
    //   slots issue slots of a SIMD-32 (2 cycles per wave64): full-rate ops
    //         (v_bitop3, 2-input adds, shifts) take 1, v_alignbit takes 2, and a
    //         sum costs one slot per addition (v_add3: 2 slots, 2 additions).
    // nonce-level words: those depending on word J (same rule as the kernel)
    uint64_t dep = 1ull << J;
    for (int t = 16; t < 64; ++t)
        if (((dep >> (t - 2)) | (dep >> (t - 7)) | (dep >> (t - 15)) | (dep >> (t - 16))) & 1ull) dep |= 1ull << t;
    auto is = [&](int t) { return (dep >> t) & 1ull; };
    uint32_t ops = 0, slots = 0;
    for (int t = 16; t < 64; ++t) {
        if (!is(t)) continue;
        // sigma: 2 alignbit + shift + xor3 (4 ops, 6 slots); a sum of n terms:
        // ceil((n-1)/2) add3 ops, n-1 slots
        const int s0 = (int)is(t - 15), s1 = (int)is(t - 2), a16 = (int)is(t - 16), a7 = (int)is(t - 7);
        const int hoisted = (s0 && s1 && a16 && a7) ? 0 : 1;  // group/run-level partial sum
        const int terms = s0 + s1 + a16 + a7 + hoisted;
        // sigma(W[J]) = sigma(wJ) ^ sigma(digit): one xor (the last digit never carries)
        const bool x0 = s0 && t - 15 == J, x1 = s1 && t - 2 == J;
        ops += (uint32_t)((s0 ? (x0 ? 1 : 4) : 0) + (s1 ? (x1 ? 1 : 4) : 0)) + (uint32_t)terms / 2u;
        slots += (uint32_t)((s0 ? (x0 ? 1 : 6) : 0) + (s1 ? (x1 ? 1 : 6) : 0)) + (uint32_t)(terms - 1);
    }
    // round J: T1 = hoisted + digit, e' and a' one add each
    ops += 3u;
    slots += 3u;
    // rounds J+1..63: 3+3 rotations, 2 xor3, Ch, Maj (16 slots) and the sums
    //   T1 = h + S1 + Ch + K + W (4 additions; 3 when K+W is hoisted, 2 when h+K+W is),
    //   e' = d + T1 (1), a' = T1 + S0 + Maj (2)
    for (int t = J + 1; t < 64; ++t) {
        const bool inv_w = !is(t), inv_h = inv_w && t <= J + 3;
        ops += inv_h ? 13u : 14u;
        slots += 16u + (inv_h ? 5u : inv_w ? 6u : 7u);
    }
    if (mode % 3 == kModeTwo) {
        ops += 8u;                   // feed-forward into block 1
        slots += 8u;
        ops += 64u * 14u - 1u;       // block 1: schedule host-known, no e' in its last round;
        slots += 64u * 22u - 1u;     // its last round also absorbs st0 (5 additions, 21 slots)
    } else {
        ops -= 1u;                   // last round: e' is dead, and K[63] + st0 rides in its sum
        slots -= 1u;
    }
    // H1 and the 64-bit compare run only on the rare new-best branch.
    ops += 2u;                       // last digit into W[J], compare H0
    slots += 2u;
    return NonceCost{ops, slots};
}

uint32_t nonce_ops(int J, int mode) { return nonce_cost(J, mode).ops; }

namespace {

// The instantiated fast kernels (layout.hpp MH_FAST_KERNELS, the launcher's list too).
bool kernel_exists(int J, int mode) { return fast_kernel_exists(J, mode); }

// Fast-kernel launch template for bucket d with L lower digits.  early: the digit ending the word
// before the last digit's is enumerated innermost (layout.hpp kMode*Early) -- false when the
// layout does not allow it.  *block_out: the nonces of one block of lanes, the unit a piece is cut
// in: 10^L, or for an Early layout 10^(p+L) (p: the innermost digit's decimal position).
bool make_fast_args(const Prefix& pre, int d, int L, bool early, int* J_out, int* mode_out, int* blocks_out,
                    uint64_t* block_out, FastArgs* fa) {
    const uint32_t t = pre.t;
    const uint32_t total = t + (uint32_t)d;
    const int nb = (total + 9u <= 64u) ? 1 : 2;
    const uint32_t pl = total - 1u;  // tail byte of the last digit
    int mode;
    uint32_t base;
    if (nb == 1) {
        mode = kModeOne;
        base = 0;
    } else if (pl >= 64u) {
        mode = kModePre;
        base = 64;
        // every enumerated digit must sit in block 1 (the Early layouts check theirs below)
        if (!early && pl - (uint32_t)L + 1u < 64u) return false;
    } else {
        mode = kModeTwo;
        base = 0;
    }
    const uint32_t lo = pl - (uint32_t)L + 1u - base;  // first lower digit, per-nonce-block relative
    int J = (int)((pl - base) >> 2);
    uint32_t p = 0, ib = 0;  // early: the innermost digit's decimal position and tail byte
    if (!early) {
        if ((int)(lo >> 2) < J - 1) return false;  // lower digits must span words J-1..J only
    } else {
        if (J < 1) return false;
        ib = base + 4u * (uint32_t)J - 1u;  // the byte ending word J - 1
        if (ib < t || ib < base) return false;  // no digit there, or not in the per-nonce block
        p = pl - ib;
        if (p < 1u || p >= (uint32_t)d) return false;
        // the group digits right before the innermost one, in its word (positions p+1 .. p+L-1):
        // the group then changes word J-1 only and no schedule word is group-level
        if (L > 4 || p + (uint32_t)L > (uint32_t)d || ib - (uint32_t)(L - 1) < t || ib - (uint32_t)(L - 1) < base)
            return false;
        J -= 1;
        mode += 3;
    }
    if (!kernel_exists(J, mode)) return false;

    memset(fa, 0, sizeof *fa);
    memcpy(fa->mid, pre.mid, sizeof pre.mid);
    for (uint32_t i = 0; i < t; ++i) put_byte(fa->blk, i, pre.tail[i]);
    for (uint32_t i = 0; i < (uint32_t)d; ++i) put_byte(fa->blk, t + i, 0x30u);  // '0' in every digit byte
    put_byte(fa->blk, total, 0x80u);
    const uint64_t bits = (pre.plen + (uint64_t)d) * 8u;
    const int lw = nb * 16 - 2;
    fa->blk[lw] = (uint32_t)(bits >> 32);
    fa->blk[lw + 1] = (uint32_t)bits;
    fa->pow10L = kPow10[L];
    fa->hi_end = total - (uint32_t)L;
    fa->n_hi = (uint32_t)(d - L);
    fa->lo_pos = lo;
    fa->L = (uint32_t)L;
    fa->n_groups = (uint32_t)kPow10[L - 1];
    fa->mode = (uint32_t)mode;
    fa->hole = kNoHole;
    fa->g_hole = kNoHole;
    fa->hole_w = 1;
    fa->g_mul = 1;
    uint64_t block = kPow10[L];
    if (early) {
        fa->inner = ib - base;
        fa->i_mul = kPow10[p];
        // positions p..p+L-1 enumerated (p: per nonce, p+1..: the group), U around them: its low
        // p digits, then its high digits from position p+L; a block of 10^(p+L) nonces is 10^p
        // interleaved lanes
        fa->g_last = ib - 1u - base;
        fa->hi_end = total;
        fa->hole = p;
        fa->hole_w = (uint32_t)L;
        fa->u_mul = 1;
        fa->g_mul = kPow10[p + 1u];
        block = kPow10[p + (uint32_t)L];
    }
    *block_out = block;
    if (mode % 3 == kModeTwo) {
        uint32_t w[64];
        schedule(fa->blk + 16, w);
        for (int i = 0; i < 64; ++i) fa->kw1[i] = kK[i] + w[i];
    }
    *J_out = J;
    *mode_out = mode;
    *blocks_out = nb;
    return true;
}

// The layout of bucket d's nonces [A, B] at L lower digits: the last digit innermost, or (opt.early)
// the digit ending the word before the last digit's, when that makes a nonce cheaper and the range
// still holds two blocks of its lanes.  False when no fast kernel takes the bucket at this L.
bool pick_layout(const Prefix& pre, int d, int L, uint64_t A, uint64_t B, const PlanOpts& opt, int* J, int* mode,
                 int* nb, uint64_t* block, FastArgs* fa) {
    if (!make_fast_args(pre, d, L, false, J, mode, nb, block, fa)) return false;
    if (opt.early) {
        int Je, me, nbe;
        uint64_t be;
        FastArgs fe;
        // a launch holds whole blocks (emit_runs), so an Early block must fit the launch caps: the
        // caps are then kept exactly, rounded up only to one 10^L-nonce lane
        const uint64_t max_gen = (uint64_t)std::min(opt.max_blocks, kMaxBlocksPerLaunch) * kBlockThreads;
        if (make_fast_args(pre, d, L, true, &Je, &me, &nbe, &be, &fe) &&
            nonce_cost(Je, me).slots < nonce_cost(*J, *mode).slots && B - A >= 2u * be &&
            be <= opt.max_nonces_per_launch && be / kPow10[L] <= max_gen) {
            *J = Je;
            *mode = me;
            *nb = nbe;
            *block = be;
            *fa = fe;
        }
    }
    return true;
}

// The fast layout of bucket d's nonces [A, B] (A <= B, all of [lower, upper] that lies in the
// bucket): L as the planner picks it and its layout (pick_layout), or false when the bucket goes
// to the generic kernel.
bool bucket_layout(const Prefix& pre, int d, uint64_t A, uint64_t B, const PlanOpts& opt, int* L_out, int* J,
                   int* mode, int* nb, uint64_t* block, FastArgs* fa) {
    int L = std::min(opt.lower_digits, d - 1);
    L = std::min(L, 5);
    // A lane runs 10^L nonces serially: a bucket with few runs would leave
    // most SIMDs idle and end in a long tail, so shorten the runs until
    // the bucket has min_lanes of them (2^19: ~8 workgroups per CU, one generation of the grid).
    while (L > 1 && (B - A) / kPow10[L] + 1u < opt.min_lanes) --L;
    while (L >= 1 && !pick_layout(pre, d, L, A, B, opt, J, mode, nb, block, fa)) --L;
    *L_out = L;
    return L >= 1 && B - A >= opt.generic_below;
}

inline uint64_t bucket_lo(int d) { return d == 1 ? 0u : kPow10[d - 1]; }
inline uint64_t bucket_hi(int d) { return d == 20 ? ~(uint64_t)0 : kPow10[d] - 1u; }

}  // namespace

void cost_segments(const Prefix& pre, uint64_t lower, uint64_t upper, const PlanOpts& opt,
                   std::vector<CostSeg>* out) {
    out->clear();
    const int d_lo = decimal_digits(lower), d_hi = decimal_digits(upper);
    for (int d = d_lo; d <= d_hi; ++d) {
        const uint64_t A = std::max(lower, bucket_lo(d)), B = std::min(upper, bucket_hi(d));
        int L = 0, J = 0, mode = 0, nb = 1;
        uint64_t blk = 1;
        FastArgs fa;
        double per;
        bool steady = false;
        if (bucket_layout(pre, d, A, B, opt, &L, &J, &mode, &nb, &blk, &fa)) {
            steady = L == opt.lower_digits && (B - A) / kPow10[L] + 1u >= (1u << 21);
            // the fast kernel's issue slots per nonce, plus the per-run / per-group work that shorter
            // lanes amortise over fewer nonces (L = 2: ~3%, L = 1: ~6% per nonce)
            per = (double)nonce_cost(J, mode).slots * (1.0 + 0.03 * (double)(3 - std::min(L, 3)));
            // a bucket of few generations of workgroups ends in a drain only partly back-filled:
            // the one-GPU model measured configs[3]'s d = 7..9 buckets in an 8-GPU shard ~15-20%
            // over the steady rate (profiles/r04o_inproc_model.json)
            if (!steady) per *= kUnsteadyFactor;
        } else {
            // generic kernel: every nonce formatted and hashed from the midstate
            const int blocks = (pre.t + (uint32_t)d + 9u <= 64u) ? 1 : 2;
            per = (double)kGenericSlotsPerBlock * blocks;
        }
        out->push_back(CostSeg{A, B, per, steady});
    }
}

double unsteady_share(const std::vector<CostSeg>& segs, uint64_t lo, uint64_t hi) {
    double all = 0.0, unsteady = 0.0;
    for (const CostSeg& s : segs) {
        const uint64_t a = std::max(s.a, lo), b = std::min(s.b, hi);
        if (a > b) continue;
        const double c = ((double)(b - a) + 1.0) * s.per;
        all += c;
        if (!s.steady) unsteady += c;
    }
    return all > 0.0 ? unsteady / all : 0.0;
}

double segments_cost(const std::vector<CostSeg>& segs, uint64_t lo, uint64_t hi) {
    double c = 0.0;
    for (const CostSeg& s : segs) {
        const uint64_t a = std::max(s.a, lo), b = std::min(s.b, hi);
        if (a <= b) c += ((double)(b - a) + 1.0) * s.per;
    }
    return c;
}

void split_by_cost(const std::vector<CostSeg>& segs, const std::vector<double>& w, std::vector<Span>* out) {
    out->assign(w.size(), Span{0, 0, true});
    if (segs.empty() || w.empty()) return;
    using u128 = unsigned __int128;
    double wsum = 0.0;
    for (double x : w) wsum += std::max(0.0, x);
    double total = 0.0;
    for (const CostSeg& s : segs) total += ((double)(s.b - s.a) + 1.0) * s.per;
    const uint64_t lower = segs.front().a;
    const u128 n_all = (u128)(segs.back().b - lower) + 1u;
    // Cut k (k = 1..n-1) after the nonce where the cost so far reaches total x (w_0 + .. + w_{k-1}) /
    // wsum; positions are nonce counts from lower (integers, monotone, the last one n_all), so the
    // spans tile [lower, upper] exactly whatever the rounding of the costs.
    u128 prev = 0;
    double acc_w = 0.0;
    for (size_t k = 0; k < w.size(); ++k) {
        acc_w += std::max(0.0, w[k]);
        u128 pos;
        if (k + 1 == w.size() || wsum <= 0.0) {
            pos = (k + 1 == w.size()) ? n_all : prev;
        } else {
            double target = total * (acc_w / wsum), cum = 0.0;
            pos = n_all;
            for (const CostSeg& s : segs) {
                const double len = (double)(s.b - s.a) + 1.0, c = len * s.per;
                if (cum + c >= target) {
                    double n = std::floor((target - cum) / s.per);
                    n = std::min(std::max(n, 0.0), len);
                    pos = (u128)(s.a - lower) + (u128)n;
                    break;
                }
                cum += c;
            }
            if (pos > n_all) pos = n_all;
        }
        if (pos < prev) pos = prev;
        if (pos > prev) (*out)[k] = Span{(uint64_t)(lower + (prev)), (uint64_t)(lower + (pos - 1u)), false};
        prev = pos;
    }
}

void plan_search(const Prefix& pre, uint64_t lower, uint64_t upper, const PlanOpts& opt,
                 const std::function<bool(const Piece&)>& cb) {
    GenArgs gbase;
    make_gen_args(pre, &gbase);
    const int d_lo = decimal_digits(lower), d_hi = decimal_digits(upper);
    const uint64_t max_gen = (uint64_t)std::min(opt.max_blocks, kMaxBlocksPerLaunch) * kBlockThreads;

    // Generic pieces are coalesced across buckets (the generic kernel formats
    // every nonce itself): small buckets and the ragged edges next to them go
    // out as one launch instead of one launch + merge each.
    bool have_gen = false;
    uint64_t gen_a = 0, gen_b = 0;  // pending generic range, inclusive
    auto flush_generic = [&]() -> bool {
        if (!have_gen) return true;
        have_gen = false;
        Piece p;
        memset(&p, 0, sizeof p);
        p.first = gen_a;
        p.count = gen_b - gen_a + 1u;
        p.kind = 1;
        p.digits = decimal_digits(gen_a);
        p.blocks = ((pre.t + (uint32_t)decimal_digits(gen_b) + 9u) <= 64u) ? 1 : 2;
        p.ga = gbase;
        p.ga.first = gen_a;
        p.ga.count = p.count;
        return cb(p);
    };
    auto emit_generic = [&](uint64_t a, uint64_t b, int) -> bool {  // [a, b] inclusive, a <= b
        for (;;) {
            if (have_gen && gen_b - gen_a < max_gen - 1u && gen_b + 1u == a) {
                const uint64_t room = max_gen - 1u - (gen_b - gen_a);  // nonces the pending piece can take
                if (b - a < room) {
                    gen_b = b;
                    return true;
                }
                gen_b = a + (room - 1u);
                a = gen_b + 1u;
            }
            if (!flush_generic()) return false;
            const uint64_t left = b - a;
            const uint64_t cnt = (left >= max_gen - 1u) ? max_gen : left + 1u;
            have_gen = true;
            gen_a = a;
            gen_b = a + (cnt - 1u);
            if (cnt - 1u == left) return true;
            a += cnt;
        }
    };

    // blocks [ua, ub) of Bx nonces of bucket d, each 10^Lx-nonce lanes [ua * lpb, ub * lpb)
    auto emit_runs = [&](int d, unsigned __int128 ua, unsigned __int128 ub, uint64_t Bx, int Lx, int Jx, int modex,
                         int nbx, const FastArgs& fax) -> bool {
        const unsigned __int128 Rx = kPow10[Lx];
        const uint64_t lpb = Bx / (uint64_t)Rx;  // lanes per block
        uint64_t max_runs = std::min<uint64_t>(max_gen, opt.max_nonces_per_launch / (uint64_t)Rx);
        // whole blocks per launch; pick_layout takes an Early layout (lpb > 1) only when one block
        // fits the caps, so this rounds up only a cap below one 10^L-nonce lane
        max_runs = std::max<uint64_t>(lpb, max_runs / lpb * lpb);
        ua *= lpb;
        ub *= lpb;
        for (unsigned __int128 u = ua; u < ub;) {
            const unsigned __int128 left = ub - u;
            const uint64_t runs = (left > max_runs) ? max_runs : (uint64_t)left;
            Piece p;
            memset(&p, 0, sizeof p);
            p.first = (uint64_t)(u * Rx);
            p.count = (uint64_t)((unsigned __int128)runs * Rx);
            p.kind = 0;
            p.digits = d;
            p.L = Lx;
            p.J = Jx;
            p.mode = modex;
            p.blocks = nbx;
            p.fa = fax;
            { const NonceCost nc = nonce_cost(Jx, modex); p.ops = nc.ops; p.slots = nc.slots; }
            p.fa.u_start = (uint64_t)u;
            p.fa.n_runs = (uint32_t)runs;
            p.ga = gbase;
            if (!flush_generic() || !cb(p)) return false;
            u += runs;
        }
        return true;
    };
    // [a, b] (a <= b) of bucket d outside the whole blocks of an Early layout (< 10^(p+L) nonces
    // at each end): 10-nonce runs of the last-digit layout -- short workgroups, on the low-
    // priority stream, so that an edge never ends a search with a few 1,000-nonce lanes -- and
    // the ragged rest on the generic kernel
    auto emit_edge = [&](int d, uint64_t a, uint64_t b) -> bool {
        FastArgs fs;
        int Js = 0, ms = 0, nbs = 1;
        uint64_t bs = 1;
        const int L = 1;
        if (!make_fast_args(pre, d, L, false, &Js, &ms, &nbs, &bs, &fs)) return emit_generic(a, b, d);
        const unsigned __int128 R = bs;
        const unsigned __int128 u0 = ((unsigned __int128)a + R - 1u) / R, u1 = ((unsigned __int128)b + 1u) / R;
        if (u0 >= u1) return emit_generic(a, b, d);
        if (a < (uint64_t)(u0 * R) && !emit_generic(a, (uint64_t)(u0 * R) - 1u, d)) return false;
        if (!emit_runs(d, u0, u1, bs, L, Js, ms, nbs, fs)) return false;
        return u1 * R > (unsigned __int128)b || emit_generic((uint64_t)(u1 * R), b, d);
    };

    for (int d = d_lo; d <= d_hi; ++d) {
        const uint64_t A = std::max(lower, bucket_lo(d)), B = std::min(upper, bucket_hi(d));
        FastArgs fa;
        int L = 0, J = 0, mode = 0, nb = 1;
        uint64_t blk = 1;
        if (!bucket_layout(pre, d, A, B, opt, &L, &J, &mode, &nb, &blk, &fa)) {
            if (!emit_generic(A, B, d)) return;
            continue;
        }
        // whole blocks of lanes: a block is one run of 10^L nonces, or (an Early layout) the
        // 10^(p+L) nonces its 10^p lanes interleave; an Early layout's ragged ends go to the
        // last-digit layout's runs first (emit_edge)
        const bool early = mode >= 3;
        const unsigned __int128 R = blk;
        const unsigned __int128 U0 = ((unsigned __int128)A + R - 1u) / R;
        const unsigned __int128 U1p = ((unsigned __int128)B + 1u) / R;  // one past the last full block
        if (U0 >= U1p) {
            if (!(early ? emit_edge(d, A, B) : emit_generic(A, B, d))) return;
            continue;
        }
        const uint64_t fast_first = (uint64_t)(U0 * R);
        const unsigned __int128 fast_end = U1p * R;  // exclusive, may be 2^64
        if (A < fast_first && !(early ? emit_edge(d, A, fast_first - 1u) : emit_generic(A, fast_first - 1u, d)))
            return;
        // Tail split (opt.fine_tail): the last runs of a full-L bucket at L - 1, so that their
        // short workgroups can back-fill the drain of the coarse launches (streams = 2).
        unsigned __int128 U_split = U1p;  // coarse blocks [U0, U_split), then the tail at L - 1
        int Lf = 0, Jf = 0, modef = 0, nbf = 1;
        uint64_t blkf = 1;
        FastArgs faf;
        if (opt.fine_tail && L == opt.lower_digits && L >= 2) {
            const unsigned __int128 tail_blocks = opt.fine_tail / (uint64_t)R;
            if (tail_blocks >= 1 && (U1p - U0) > 4 * tail_blocks &&
                pick_layout(pre, d, L - 1, A, B, opt, &Jf, &modef, &nbf, &blkf, &faf) && R % blkf == 0u) {
                U_split = U1p - tail_blocks;
                Lf = L - 1;
            }
        }
        if (!emit_runs(d, U0, U_split, blk, L, J, mode, nb, fa)) return;
        if (U_split < U1p && !emit_runs(d, U_split * (R / blkf), U1p * (R / blkf), blkf, Lf, Jf, modef, nbf, faf))
            return;
        if (fast_end <= (unsigned __int128)B &&
            !(early ? emit_edge(d, (uint64_t)fast_end, B) : emit_generic((uint64_t)fast_end, B, d)))
            return;
    }
    flush_generic();
}

// ---- batched search ----

uint64_t batch_tiles(uint64_t first, uint64_t count) {
    const uint64_t last = first + (count - 1u);
    const uint64_t decades = last / 10u - first / 10u + 1u;  // <= 2^64 / 10: no overflow below
    return (decades + (kBatchTileDecades - 1u)) / kBatchTileDecades;
}

void plan_batch(const BatchRequest* reqs, size_t n, const PlanOpts& opt, uint32_t slot_cap,
                std::vector<BatchItem>* items) {
    items->clear();
    slot_cap = std::min(slot_cap, kMaxBlocksPerLaunch);
    int pass = 0;
    uint32_t used_slots = 0, used_reqs = 0, used_entries = 0;
    std::vector<BatchItem> mine;  // the entries of one request
    for (size_t i = 0; i < n; ++i) {
        const BatchRequest& r = reqs[i];
        mine.clear();
        bool fused = true;
        uint64_t tiles = 0;
        plan_search(r.pre, r.lower, r.upper, opt, [&](const Piece& p) {
            if (p.kind != 1 || mine.size() == kBatchMaxEntries) return fused = false;
            const uint64_t t = batch_tiles(p.first, p.count);
            tiles += t;
            if (tiles > slot_cap) return fused = false;
            mine.push_back(BatchItem{r.id, p.first, p.count, 0, 0, 0, (uint32_t)t, i});
            return true;
        });
        if (!fused) {
            items->push_back(BatchItem{r.id, r.lower, r.upper - r.lower + 1u, 1, -1, 0, 0, i});
            continue;
        }
        if (used_reqs && (used_slots + tiles > slot_cap || used_reqs == kBatchMaxRequests ||
                          used_entries + mine.size() > kBatchMaxEntries)) {
            ++pass;
            used_slots = used_reqs = used_entries = 0;
        }
        for (BatchItem& it : mine) {
            it.pass = pass;
            it.slot = used_slots;
            used_slots += it.slots;
            items->push_back(it);
        }
        ++used_reqs;
        used_entries += (uint32_t)mine.size();
    }
}

void build_batch_tables(const BatchRequest* reqs, const std::vector<BatchItem>& items, int pass, BatchTables* out) {
    out->entries.clear();
    out->tile_entry.clear();
    out->seg.clear();
    out->req_idx.clear();
    out->nonces = 0;
    uint32_t slots = 0;
    for (const BatchItem& it : items) {
        if (it.kind != 0 || it.pass != pass) continue;
        if (out->req_idx.empty() || out->req_idx.back() != it.idx) {
            out->req_idx.push_back(it.idx);
            out->seg.push_back(it.slot);
        }
        BatchEntry e;
        make_gen_args(reqs[it.idx].pre, &e.g);
        e.g.first = it.first;
        e.g.count = it.count;
        e.tile0 = it.slot;
        e.slot0 = it.slot;
        out->tile_entry.insert(out->tile_entry.end(), it.slots, (uint32_t)out->entries.size());
        out->entries.push_back(e);
        out->nonces += it.count;
        slots = it.slot + it.slots;
    }
    out->seg.push_back(slots);
}

bool batch_tables_ok(const BatchTables& t, uint32_t slot_cap) {
    const size_t tiles = t.tile_entry.size(), nreq = t.req_idx.size();
    if (tiles == 0 || tiles > slot_cap || tiles > kMaxBlocksPerLaunch) return false;
    if (t.entries.empty() || t.entries.size() > kBatchMaxEntries || t.entries.size() > tiles) return false;
    if (nreq == 0 || nreq > kBatchMaxRequests || nreq > t.entries.size() || t.seg.size() != nreq + 1u) return false;
    // entries: in tile order, each with exactly its tiles, together all tiles
    uint64_t next = 0;
    for (const BatchEntry& e : t.entries) {
        if (e.g.count == 0 || e.g.first + (e.g.count - 1u) < e.g.first || e.g.t > 63u) return false;
        if (e.tile0 != next || e.slot0 != e.tile0) return false;
        next += batch_tiles(e.g.first, e.g.count);
        if (next > tiles) return false;
    }
    if (next != tiles) return false;
    // tiles: each inside its entry's tiles
    for (size_t i = 0; i < tiles; ++i) {
        const uint32_t ei = t.tile_entry[i];
        if (ei >= t.entries.size()) return false;
        const BatchEntry& e = t.entries[ei];
        if (i < e.tile0 || i - e.tile0 >= batch_tiles(e.g.first, e.g.count)) return false;
    }
    // segments: contiguous, non-empty, each starting at an entry, together all slots
    if (t.seg.front() != 0 || t.seg.back() != tiles) return false;
    for (size_t r = 0; r < nreq; ++r) {
        if (t.seg[r] >= t.seg[r + 1]) return false;
        if (t.entries[t.tile_entry[t.seg[r]]].tile0 != t.seg[r]) return false;
    }
    return true;
}

// ---- batched search with fused fast pieces ----

uint64_t batch_min_lanes(uint64_t min_lanes, size_t fast_requests) {
    if (fast_requests < 2) return min_lanes;
    uint64_t share = min_lanes / fast_requests, p = 1;
    while (p <= share / 2u) p *= 2u;  // the largest power of two <= share (1 for share <= 1)
    share = std::max<uint64_t>(p, (uint64_t)kBlockThreads);  // at least one chunk's runs
    return std::min(min_lanes, share);  // never more than the caller's own
}

void plan_batch_ex(const BatchRequest* reqs, size_t n, const PlanOpts& opt, uint32_t slot_cap, bool shared_lanes,
                   uint64_t max_nonces, std::vector<BatchPiece>* pieces, std::vector<FastArgs>* args) {
    pieces->clear();
    args->clear();
    slot_cap = std::min(slot_cap, kMaxBlocksPerLaunch);
    // One request's plan under o: its pieces if they fit a pass (fused), and whether it holds a
    // fast piece at all.  may_fast false (over the size cap): a fast piece makes it a fallback.
    struct One {
        bool fused = true, saw_fast = false;
        uint64_t slots = 0;
        uint32_t entries = 0, fast = 0;
        std::vector<BatchPiece> pieces;
        std::vector<FastArgs> args;
    };
    auto plan_one = [&](size_t i, const PlanOpts& o, bool may_fast, One* out) {
        const BatchRequest& r = reqs[i];
        *out = One();
        plan_search(r.pre, r.lower, r.upper, o, [&](const Piece& p) {
            BatchPiece b;
            memset(&b, 0, sizeof b);
            b.req = r.id;
            b.first = p.first;
            b.count = p.count;
            b.launch = -1;
            b.idx = i;
            if (p.kind == 1) {
                if (out->entries == kBatchMaxEntries) return out->fused = false;
                ++out->entries;
                b.kind = 0;
                b.slots = (uint32_t)std::min<uint64_t>(batch_tiles(p.first, p.count), (uint64_t)slot_cap + 1u);
            } else {
                out->saw_fast = true;
                if (!may_fast || out->fast == kBatchMaxFastItems) return out->fused = false;
                ++out->fast;
                b.kind = 2;
                b.slots = (p.fa.n_runs + (uint32_t)kBlockThreads - 1u) / (uint32_t)kBlockThreads;
                b.J = p.J;
                b.mode = p.mode;
                b.L = p.L;
                b.ops = p.ops;
                b.nslots = p.slots;
                b.fa = out->args.size();
                out->args.push_back(p.fa);
                out->args.back().n_chunks = b.slots;
                out->args.back().counter = nullptr;
            }
            out->slots += b.slots;
            if (out->slots > slot_cap) return out->fused = false;
            out->pieces.push_back(b);
            return true;
        });
    };
    // every request under its own plan first: the generic-only ones are done with it, and the
    // candidates -- a fast piece in the own plan, no more nonces than the cap -- are counted
    std::vector<One> one(n);
    std::vector<char> cand(n, 0);
    size_t ncand = 0;
    for (size_t i = 0; i < n; ++i) {
        const BatchRequest& r = reqs[i];
        const bool over = r.upper - r.lower >= max_nonces;  // count - 1; the whole of u64 included
        plan_one(i, opt, !over, &one[i]);
        if (over) continue;
        if (!one[i].fused && !one[i].saw_fast)  // stopped for its size before a fast piece: look on
            plan_search(r.pre, r.lower, r.upper, opt, [&](const Piece& p) { return !(one[i].saw_fast = p.kind == 0); });
        if (one[i].saw_fast) cand[i] = 1, ++ncand;
    }
    PlanOpts shared = opt;
    if (shared_lanes) shared.min_lanes = batch_min_lanes(opt.min_lanes, ncand);
    if (shared.min_lanes != opt.min_lanes)
        for (size_t i = 0; i < n; ++i)
            if (cand[i]) plan_one(i, shared, true, &one[i]);

    int pass = 0;
    uint32_t used_slots = 0, used_reqs = 0, used_entries = 0, used_fast = 0;
    std::vector<size_t> pass_fast; // the fast pieces (indices into *pieces) of the pass being packed
    // launches and chunk offsets of a finished pass: groups in order of first appearance, inside a
    // group L descending, then request order (the order the pieces were planned in)
    auto close_pass = [&]() {
        std::vector<std::pair<int, int>> groups;
        for (size_t k : pass_fast) {
            const std::pair<int, int> g{(*pieces)[k].J, (*pieces)[k].mode};
            if (std::find(groups.begin(), groups.end(), g) == groups.end()) groups.push_back(g);
        }
        for (size_t gi = 0; gi < groups.size(); ++gi) {
            std::vector<size_t> in;
            for (size_t k : pass_fast)
                if ((*pieces)[k].J == groups[gi].first && (*pieces)[k].mode == groups[gi].second) in.push_back(k);
            std::stable_sort(in.begin(), in.end(), [&](size_t a, size_t b) { return (*pieces)[a].L > (*pieces)[b].L; });
            uint32_t chunk = 0;
            for (size_t k : in) {
                (*pieces)[k].launch = (int)gi;
                (*pieces)[k].chunk0 = chunk;
                chunk += (*pieces)[k].slots;
            }
        }
        pass_fast.clear();
    };
    for (size_t i = 0; i < n; ++i) {
        const BatchRequest& r = reqs[i];
        const One& o = one[i];
        if (!o.fused) {
            BatchPiece b;
            memset(&b, 0, sizeof b);
            b.req = r.id;
            b.first = r.lower;
            b.count = r.upper - r.lower + 1u;
            b.kind = 1;
            b.pass = b.launch = -1;
            b.idx = i;
            pieces->push_back(b);
            continue;
        }
        if (used_reqs && (used_slots + o.slots > slot_cap || used_reqs == kBatchMaxRequests ||
                          used_entries + o.entries > kBatchMaxEntries || used_fast + o.fast > kBatchMaxFastItems)) {
            close_pass();
            ++pass;
            used_slots = used_reqs = used_entries = used_fast = 0;
        }
        for (BatchPiece b : o.pieces) {
            b.pass = pass;
            b.slot = used_slots;
            used_slots += b.slots;
            if (b.kind == 2) {
                pass_fast.push_back(pieces->size());
                args->push_back(o.args[b.fa]);
                b.fa = args->size() - 1u;
            }
            pieces->push_back(b);
        }
        ++used_reqs;
        used_entries += o.entries;
        used_fast += o.fast;
    }
    close_pass();
}

void build_batch_tables_ex(const BatchRequest* reqs, const std::vector<BatchPiece>& pieces,
                           const std::vector<FastArgs>& args, int pass, BatchTables* t, BatchFastTables* f) {
    t->entries.clear();
    t->tile_entry.clear();
    t->seg.clear();
    t->req_idx.clear();
    t->nonces = 0;
    f->items.clear();
    f->chunk_item.clear();
    f->launches.clear();
    f->piece.clear();
    uint32_t slots = 0;
    std::vector<size_t> fast;  // the pass's fast pieces
    bool any = false;
    size_t last_idx = 0;
    for (size_t k = 0; k < pieces.size(); ++k) {
        const BatchPiece& p = pieces[k];
        if (p.kind == 1 || p.pass != pass) continue;
        if (!any || last_idx != p.idx) {
            t->req_idx.push_back(p.idx);
            t->seg.push_back(p.slot);
            any = true;
            last_idx = p.idx;
        }
        if (p.kind == 0) {
            BatchEntry e;
            make_gen_args(reqs[p.idx].pre, &e.g);
            e.g.first = p.first;
            e.g.count = p.count;
            e.tile0 = (uint32_t)t->tile_entry.size();
            e.slot0 = p.slot;
            t->tile_entry.insert(t->tile_entry.end(), p.slots, (uint32_t)t->entries.size());
            t->entries.push_back(e);
            t->nonces += p.count;
        } else {
            fast.push_back(k);
        }
        slots = p.slot + p.slots;
    }
    t->seg.push_back(slots);
    // items in launch order, then chunk order (plan_batch_ex numbered both)
    std::stable_sort(fast.begin(), fast.end(), [&](size_t a, size_t b) {
        return pieces[a].launch != pieces[b].launch ? pieces[a].launch < pieces[b].launch
                                                    : pieces[a].chunk0 < pieces[b].chunk0;
    });
    for (size_t k : fast) {
        const BatchPiece& p = pieces[k];
        if (f->launches.empty() || (int)f->launches.size() - 1 != p.launch)
            f->launches.push_back(BatchFastLaunch{p.J, p.mode, (uint32_t)f->items.size(), 0u,
                                                  (uint32_t)f->chunk_item.size(), 0u});
        BatchFastLaunch& l = f->launches.back();
        BatchFastItem it;
        it.args = args[p.fa];
        it.chunk0 = p.chunk0;
        it.slot0 = p.slot;
        f->chunk_item.insert(f->chunk_item.end(), p.slots, (uint32_t)f->items.size());
        f->items.push_back(it);
        f->piece.push_back(k);
        l.items += 1u;
        l.chunks += p.slots;
    }
}

bool batch_tables_ex_ok(const BatchTables& t, const BatchFastTables& f, uint32_t slot_cap) {
    const size_t tiles = t.tile_entry.size(), chunks = f.chunk_item.size(), nreq = t.req_idx.size();
    const size_t slots = tiles + chunks;
    if (slots == 0 || slots > slot_cap || slots > kMaxBlocksPerLaunch) return false;
    if (t.entries.size() > kBatchMaxEntries || t.entries.size() > tiles || (tiles && t.entries.empty())) return false;
    if (f.items.size() > kBatchMaxFastItems || f.items.size() > chunks || (chunks && f.items.empty())) return false;
    if (nreq == 0 || nreq > kBatchMaxRequests || nreq > slots || t.seg.size() != nreq + 1u) return false;
    std::vector<uint8_t> written(slots, 0);  // per slot: tiles and chunks that write it
    auto write = [&](uint64_t slot) {
        if (slot >= slots || written[(size_t)slot]) return false;
        written[(size_t)slot] = 1;
        return true;
    };
    // entries: in tile order, each with exactly its tiles, together all tiles
    uint64_t next = 0;
    for (const BatchEntry& e : t.entries) {
        if (e.g.count == 0 || e.g.first + (e.g.count - 1u) < e.g.first || e.g.t > 63u) return false;
        if (e.tile0 != next) return false;
        next += batch_tiles(e.g.first, e.g.count);
        if (next > tiles) return false;
    }
    if (next != tiles) return false;
    // tiles: each inside its entry's tiles, writing a slot of its own
    for (size_t i = 0; i < tiles; ++i) {
        const uint32_t ei = t.tile_entry[i];
        if (ei >= t.entries.size()) return false;
        const BatchEntry& e = t.entries[ei];
        if (i < e.tile0 || i - e.tile0 >= batch_tiles(e.g.first, e.g.count)) return false;
        if (!write((uint64_t)e.slot0 + (i - e.tile0))) return false;
    }
    // launches: together all items and all chunks, in order; every item of its launch's layout, its
    // chunks exactly its runs' and behind the launch's earlier items'
    uint64_t item = 0, chunk = 0;
    for (const BatchFastLaunch& l : f.launches) {
        if (!fast_kernel_exists(l.J, l.mode) || l.items == 0 || l.chunks == 0) return false;
        if (l.item0 != item || l.chunk0 != chunk) return false;
        item += l.items;
        chunk += l.chunks;
        if (item > f.items.size() || chunk > chunks) return false;
        uint64_t c = 0;
        for (uint32_t k = l.item0; k < l.item0 + l.items; ++k) {
            const BatchFastItem& it = f.items[k];
            const FastArgs& a = it.args;
            if (a.mode != (uint32_t)l.mode || a.counter != nullptr || a.n_runs == 0 || a.L < 1 || a.L > 5 ||
                a.n_hi + a.L > 20)
                return false;
            if (a.n_chunks != (a.n_runs + (uint32_t)kBlockThreads - 1u) / (uint32_t)kBlockThreads) return false;
            if (it.chunk0 != c) return false;
            c += a.n_chunks;
            if (c > l.chunks) return false;
        }
        if (c != l.chunks) return false;
        // chunks: each names an item of this launch and lies inside that item's chunks
        for (uint32_t b = 0; b < l.chunks; ++b) {
            const uint32_t ii = f.chunk_item[l.chunk0 + b];
            if (ii < l.item0 || ii >= l.item0 + l.items) return false;
            const BatchFastItem& it = f.items[ii];
            if (b < it.chunk0 || b - it.chunk0 >= it.args.n_chunks) return false;
            if (!write((uint64_t)it.slot0 + (b - it.chunk0))) return false;
        }
    }
    if (item != f.items.size() || chunk != chunks) return false;
    // every slot written exactly once (none twice above; as many writers as slots)
    for (uint8_t w : written)
        if (!w) return false;
    // segments: contiguous, non-empty, together all slots
    if (t.seg.front() != 0 || t.seg.back() != slots) return false;
    for (size_t r = 0; r < nreq; ++r)
        if (t.seg[r] >= t.seg[r + 1]) return false;
    return true;
}

// ---- batched first-hit search ----

namespace {
// Per entry of a pass its request (index into seg / req_idx), for the kernels whose tiles find
// per-request device words; and the check that every entry's request owns the entry's slots.
void entry_requests(const BatchTables& t, std::vector<uint32_t>* entry_req) {
    const size_t nreq = t.req_idx.size();
    entry_req->assign(t.entries.size(), 0u);
    size_t r = 0;
    for (size_t ei = 0; ei < t.entries.size(); ++ei) {  // entries and segments are both in slot order
        while (r + 1 < nreq && t.seg[r + 1] <= t.entries[ei].slot0) ++r;
        (*entry_req)[ei] = (uint32_t)r;
    }
}
bool entry_requests_ok(const BatchTables& t, const std::vector<uint32_t>& entry_req) {
    const size_t nreq = t.req_idx.size();
    if (entry_req.size() != t.entries.size() || t.seg.size() != nreq + 1u) return false;
    for (size_t ei = 0; ei < t.entries.size(); ++ei) {
        const uint32_t r = entry_req[ei];
        if (r >= nreq || t.entries[ei].slot0 < t.seg[r] || t.entries[ei].slot0 >= t.seg[r + 1]) return false;
    }
    return true;
}
}  // namespace

void build_first_batch_tables(const BatchTables& t, bool rank_major, FirstBatchTables* out) {
    const size_t tiles = t.tile_entry.size(), nreq = t.req_idx.size();
    entry_requests(t, &out->entry_req);
    out->order.clear();
    out->order.reserve(tiles);
    if (!rank_major) {
        for (size_t i = 0; i < tiles; ++i) out->order.push_back((uint32_t)i);
        return;
    }
    // the requests that still have a tile of the current rank, in request order: each round emits
    // one tile per such request, so the whole costs O(tiles + requests)
    std::vector<uint32_t> active(nreq);
    for (size_t i = 0; i < nreq; ++i) active[i] = (uint32_t)i;
    for (uint32_t rank = 0; !active.empty(); ++rank) {
        size_t keep = 0;
        for (const uint32_t q : active) {
            const uint32_t slot = t.seg[q] + rank;  // < seg[q + 1]: q is active
            out->order.push_back(slot);
            if (slot + 1u < t.seg[q + 1]) active[keep++] = q;
        }
        active.resize(keep);
    }
}

bool first_batch_tables_ok(const BatchTables& t, const FirstBatchTables& f) {
    const size_t tiles = t.tile_entry.size();
    if (!entry_requests_ok(t, f.entry_req) || f.order.size() != tiles) return false;
    std::vector<bool> seen(tiles, false);
    for (const uint32_t s : f.order) {
        if (s >= tiles || seen[s]) return false;
        seen[s] = true;
    }
    return true;  // tiles distinct values below tiles: a permutation
}

// ---- batched first-hit search with fused fast pieces ----

namespace {
// n distinct values below n: a permutation of 0 .. n - 1
bool is_permutation(const uint32_t* p, size_t n) {
    std::vector<bool> seen(n, false);
    for (size_t i = 0; i < n; ++i) {
        if (p[i] >= n || seen[p[i]]) return false;
        seen[p[i]] = true;
    }
    return true;
}
// the request whose segment holds `slot` (the segments are contiguous and non-empty)
uint32_t slot_request(const BatchTables& t, uint32_t slot) {
    const size_t nreq = t.req_idx.size();
    size_t lo = 0, hi = nreq;  // seg[lo] <= slot < seg[hi]
    while (lo + 1 < hi) {
        const size_t mid = (lo + hi) / 2;
        (t.seg[mid] <= slot ? lo : hi) = mid;
    }
    return (uint32_t)lo;
}
// x zero-extended by w decimal digits at digit index k (fast_search.hip spread)
uint64_t spread_host(uint64_t x, uint32_t k, uint32_t w) {
    if (k >= 20u) return x;
    uint64_t lo = 0, p = 1;
    for (uint32_t j = 0; j < k; ++j) {
        lo += (x % 10u) * p;
        p *= 10u;
        x /= 10u;
    }
    for (uint32_t j = 0; j < w; ++j) p *= 10u;
    return x * p + lo;
}
}  // namespace

uint64_t chunk_floor_host(const FastArgs& a, uint32_t blk) {
    const uint64_t u0 = a.u_start + (uint64_t)blk * kBlockThreads;
    return a.mode < kModeOneEarly ? u0 * a.pow10L : spread_host(u0, a.hole, a.hole_w) * a.u_mul;
}

void build_first_batch_tables_ex(const BatchTables& t, const BatchFastTables& f, bool rank_major,
                                 FirstBatchFastTables* out) {
    const size_t tiles = t.tile_entry.size(), nreq = t.req_idx.size();
    entry_requests(t, &out->entry_req);
    out->item_req.clear();
    for (const BatchFastItem& it : f.items) out->item_req.push_back(slot_request(t, it.slot0));
    out->tile_order.clear();
    out->tile_order.reserve(tiles);
    out->chunk_order.clear();
    out->chunk_order.reserve(f.chunk_item.size());
    if (!rank_major) {
        for (size_t i = 0; i < tiles; ++i) out->tile_order.push_back((uint32_t)i);
        for (const BatchFastLaunch& l : f.launches)
            for (uint32_t b = 0; b < l.chunks; ++b) out->chunk_order.push_back(b);
        return;
    }
    // generic launch: per request its tiles [first, end) -- entries, and so tiles, are in request
    // and nonce order -- and each round emits one tile per request that still has one
    {
        std::vector<uint32_t> first(nreq, 0u), end(nreq, 0u);
        std::vector<bool> any(nreq, false);
        for (size_t ei = 0; ei < t.entries.size(); ++ei) {
            const uint32_t r = out->entry_req[ei];
            const uint32_t t0 = t.entries[ei].tile0;
            const uint32_t t1 = ei + 1 < t.entries.size() ? t.entries[ei + 1].tile0 : (uint32_t)tiles;
            if (!any[r]) first[r] = t0;
            any[r] = true;
            end[r] = t1;
        }
        std::vector<uint32_t> active;
        for (size_t r = 0; r < nreq; ++r)
            if (any[r] && first[r] < end[r]) active.push_back((uint32_t)r);
        for (uint32_t rank = 0; !active.empty(); ++rank) {
            size_t keep = 0;
            for (const uint32_t q : active) {
                out->tile_order.push_back(first[q] + rank);
                if (first[q] + rank + 1u < end[q]) active[keep++] = q;
            }
            active.resize(keep);
        }
    }
    // batch_first launches: each round emits one chunk per item that still has one
    for (const BatchFastLaunch& l : f.launches) {
        std::vector<uint32_t> active;
        for (uint32_t k = l.item0; k < l.item0 + l.items; ++k)
            if (f.items[k].args.n_chunks) active.push_back(k);
        for (uint32_t rank = 0; !active.empty(); ++rank) {
            size_t keep = 0;
            for (const uint32_t k : active) {
                out->chunk_order.push_back(f.items[k].chunk0 + rank);
                if (rank + 1u < f.items[k].args.n_chunks) active[keep++] = k;
            }
            active.resize(keep);
        }
    }
}

bool first_batch_tables_ex_ok(const BatchTables& t, const BatchFastTables& f, const FirstBatchFastTables& x,
                              uint32_t slot_cap) {
    if (!batch_tables_ex_ok(t, f, slot_cap)) return false;
    const size_t tiles = t.tile_entry.size(), nreq = t.req_idx.size();
    // every entry's request owns all of the entry's slots
    if (!entry_requests_ok(t, x.entry_req)) return false;
    for (size_t ei = 0; ei < t.entries.size(); ++ei) {
        const BatchEntry& e = t.entries[ei];
        if ((uint64_t)e.slot0 + batch_tiles(e.g.first, e.g.count) > t.seg[x.entry_req[ei] + 1u]) return false;
    }
    // and every item's request all of the item's
    if (x.item_req.size() != f.items.size()) return false;
    for (size_t k = 0; k < f.items.size(); ++k) {
        const uint32_t r = x.item_req[k];
        const BatchFastItem& it = f.items[k];
        if (r >= nreq || it.slot0 < t.seg[r] || (uint64_t)it.slot0 + it.args.n_chunks > t.seg[r + 1]) return false;
    }
    if (x.tile_order.size() != tiles || !is_permutation(x.tile_order.data(), tiles)) return false;
    if (x.chunk_order.size() != f.chunk_item.size()) return false;
    for (const BatchFastLaunch& l : f.launches)  // l.chunk0 + l.chunks <= chunk_item.size() (batch_tables_ex_ok)
        if (!is_permutation(x.chunk_order.data() + l.chunk0, l.chunks)) return false;
    return true;
}

uint32_t first_batch_order_slot(const BatchTables& t, const BatchFastTables& f, int launch, uint32_t v) {
    if (launch < 0) {
        const BatchEntry& e = t.entries[t.tile_entry[v]];
        return e.slot0 + (v - e.tile0);
    }
    const BatchFastLaunch& l = f.launches[(size_t)launch];
    const BatchFastItem& it = f.items[f.chunk_item[l.chunk0 + v]];
    return it.slot0 + (v - it.chunk0);
}

// ---- batched hits ----

namespace {
inline size_t align16(size_t x) { return (x + 15u) & ~(size_t)15u; }
// nonces of a request, saturating (a fused request is far smaller)
inline uint64_t request_size(const BatchRequest& r) {
    const uint64_t d = r.upper - r.lower;
    return d == ~(uint64_t)0 ? d : d + 1u;
}
}  // namespace

size_t hits_batch_table_bytes(size_t entries, size_t requests, size_t tiles) {
    return align16(entries * sizeof(BatchEntry)) + align16((requests + 1u) * sizeof(uint32_t)) +
           align16(tiles * sizeof(uint32_t)) + align16(entries * sizeof(uint32_t)) +
           align16(requests * sizeof(BatchHitsWords));
}

void hits_batch_drained(HitsBatchState* st) {
    st->toff = st->nres = 0;
    st->used = 0;
    ++st->window;
}

namespace {
// plan_hits_batch_pass for a pass whose tables take `bytes` of the table buffer
bool plan_hits_pass(const BatchTables& t, size_t bytes, const BatchRequest* reqs, const uint64_t* caps,
                    const HitsBatchLimits& lim, HitsBatchState* st, HitsBatchTables* out) {
    const size_t nreq = t.req_idx.size();
    uint64_t want = 0;  // <= kBatchMaxRequests * MH_HITS_MAX_CAP-sized caps: no overflow
    for (size_t r = 0; r < nreq; ++r) want += std::min(caps[t.req_idx[r]], request_size(reqs[t.req_idx[r]]));
    const bool in_flight = st->toff != 0 || st->nres != 0 || st->used != 0;
    const bool drain = in_flight && (st->toff + bytes > lim.table_bytes || st->nres + nreq > lim.results ||
                                     (st->used != 0 && want > lim.window_slots - std::min(st->used, lim.window_slots)));
    if (drain) hits_batch_drained(st);
    entry_requests(t, &out->entry_req);
    out->region.clear();
    out->region.reserve(nreq);
    for (size_t r = 0; r < nreq; ++r) {
        const uint64_t left = lim.window_slots - std::min(st->used, lim.window_slots);
        const uint64_t slots = std::min(std::min(caps[t.req_idx[r]], request_size(reqs[t.req_idx[r]])), left);
        out->region.push_back(HitsRegion{st->used, slots});
        st->used += slots;
    }
    st->toff += bytes;
    st->nres += nreq;
    return drain;
}
}  // namespace

bool plan_hits_batch_pass(const BatchTables& t, const BatchRequest* reqs, const uint64_t* caps,
                          const HitsBatchLimits& lim, HitsBatchState* st, HitsBatchTables* out) {
    return plan_hits_pass(t, hits_batch_table_bytes(t.entries.size(), t.req_idx.size(), t.tile_entry.size()), reqs, caps,
                          lim, st, out);
}

bool hits_batch_tables_ok(const BatchTables& t, const BatchRequest* reqs, const HitsBatchTables& h,
                          uint64_t used_before, uint64_t window_slots) {
    const size_t nreq = t.req_idx.size();
    if (!entry_requests_ok(t, h.entry_req) || h.region.size() != nreq) return false;
    uint64_t next = used_before;
    for (size_t r = 0; r < nreq; ++r) {
        const HitsRegion& g = h.region[r];
        if (g.offset < next || g.offset > window_slots || g.slots > window_slots - g.offset) return false;
        if (g.slots > request_size(reqs[t.req_idx[r]])) return false;
        next = g.offset + g.slots;
    }
    return true;
}

// ---- batched hits with fused fast pieces ----

size_t hits_batch_table_bytes_ex(size_t entries, size_t requests, size_t tiles, size_t items, size_t chunks) {
    return hits_batch_table_bytes(entries, requests, tiles) + items * sizeof(BatchHitsItem) +
           align16(chunks * sizeof(uint32_t));
}

bool plan_hits_batch_pass_ex(const BatchTables& t, const BatchFastTables& f, const BatchRequest* reqs,
                             const uint64_t* caps, const HitsBatchLimits& lim, HitsBatchState* st,
                             HitsBatchFastTables* out) {
    const size_t bytes = hits_batch_table_bytes_ex(t.entries.size(), t.req_idx.size(), t.tile_entry.size(),
                                                   f.items.size(), f.chunk_item.size());
    const bool drain = plan_hits_pass(t, bytes, reqs, caps, lim, st, &out->h);
    out->item_req.clear();
    for (const BatchFastItem& it : f.items) out->item_req.push_back(slot_request(t, it.slot0));
    return drain;
}

bool hits_batch_tables_ex_ok(const BatchTables& t, const BatchFastTables& f, const BatchRequest* reqs,
                             const HitsBatchFastTables& x, uint32_t slot_cap, uint64_t used_before,
                             uint64_t window_slots) {
    if (!batch_tables_ex_ok(t, f, slot_cap)) return false;
    if (!hits_batch_tables_ok(t, reqs, x.h, used_before, window_slots)) return false;
    const size_t nreq = t.req_idx.size();
    // every entry's request owns all of the entry's slots
    for (size_t ei = 0; ei < t.entries.size(); ++ei) {
        const BatchEntry& e = t.entries[ei];
        const uint32_t r = x.h.entry_req[ei];  // < nreq (entry_requests_ok)
        if (e.slot0 < t.seg[r] || (uint64_t)e.slot0 + batch_tiles(e.g.first, e.g.count) > t.seg[r + 1u]) return false;
    }
    // and every item's request all of the item's
    if (x.item_req.size() != f.items.size()) return false;
    for (size_t k = 0; k < f.items.size(); ++k) {
        const uint32_t r = x.item_req[k];
        const BatchFastItem& it = f.items[k];
        if (r >= nreq || it.slot0 < t.seg[r] || (uint64_t)it.slot0 + it.args.n_chunks > t.seg[r + 1]) return false;
    }
    return true;
}

// ---- batched first k hits ----

FirstHitsBatchLayout first_hits_batch_layout(size_t entries, size_t requests, size_t tiles, size_t items, size_t chunks) {
    static_assert(sizeof(BatchBoundItem) % 16 == 0 && sizeof(BatchBoundWords) % 16 == 0, "tables stay 16-byte aligned");
    FirstHitsBatchLayout l;
    l.o_seg = align16(entries * sizeof(BatchEntry));
    l.o_tile = l.o_seg + align16((requests + 1u) * sizeof(uint32_t));
    l.o_ereq = l.o_tile + align16(tiles * sizeof(uint32_t));
    l.o_order = l.o_ereq + align16(entries * sizeof(uint32_t));
    l.o_words = l.o_order + align16(tiles * sizeof(uint32_t));
    l.o_item = l.o_words + requests * sizeof(BatchBoundWords);
    l.o_chunk = l.o_item + items * sizeof(BatchBoundItem);
    l.o_corder = l.o_chunk + align16(chunks * sizeof(uint32_t));
    l.bytes = l.o_corder + align16(chunks * sizeof(uint32_t));
    return l;
}

bool plan_first_hits_batch_pass(const BatchTables& t, const BatchFastTables& f, const BatchRequest* reqs,
                                const uint64_t* wants, const HitsBatchLimits& lim, bool rank_major,
                                HitsBatchState* st, FirstHitsBatchTables* out) {
    const size_t bytes = first_hits_batch_layout(t.entries.size(), t.req_idx.size(), t.tile_entry.size(), f.items.size(),
                                                 f.chunk_item.size()).bytes;
    HitsBatchTables h;
    const bool drain = plan_hits_pass(t, bytes, reqs, wants, lim, st, &h);
    build_first_batch_tables_ex(t, f, rank_major, &out->o);
    out->region.swap(h.region);
    return drain;
}

bool first_hits_batch_tables_ok(const BatchTables& t, const BatchFastTables& f, const BatchRequest* reqs,
                                const FirstHitsBatchTables& x, uint32_t slot_cap, uint64_t used_before,
                                uint64_t window_slots) {
    if (f.items.empty()) {
        if (!f.chunk_item.empty() || !f.launches.empty() || !batch_tables_ok(t, slot_cap)) return false;
    } else if (!batch_tables_ex_ok(t, f, slot_cap)) {
        return false;
    }
    const size_t tiles = t.tile_entry.size(), nreq = t.req_idx.size();
    if (nreq > kBatchMaxRequests) return false;  // one set of slice counters per request of a pass
    HitsBatchTables h;
    h.entry_req = x.o.entry_req;
    h.region = x.region;
    if (!hits_batch_tables_ok(t, reqs, h, used_before, window_slots)) return false;
    for (size_t ei = 0; ei < t.entries.size(); ++ei) {  // every entry's request owns all of the entry's slots
        const BatchEntry& e = t.entries[ei];
        const uint32_t r = x.o.entry_req[ei];  // < nreq (entry_requests_ok)
        if (e.slot0 < t.seg[r] || (uint64_t)e.slot0 + batch_tiles(e.g.first, e.g.count) > t.seg[r + 1u]) return false;
    }
    if (x.o.item_req.size() != f.items.size()) return false;
    for (size_t k = 0; k < f.items.size(); ++k) {  // and every item's request all of the item's
        const uint32_t r = x.o.item_req[k];
        const BatchFastItem& it = f.items[k];
        if (r >= nreq || it.slot0 < t.seg[r] || (uint64_t)it.slot0 + it.args.n_chunks > t.seg[r + 1]) return false;
    }
    if (x.o.tile_order.size() != tiles || !is_permutation(x.o.tile_order.data(), tiles)) return false;
    if (x.o.chunk_order.size() != f.chunk_item.size()) return false;
    for (const BatchFastLaunch& l : f.launches)  // l.chunk0 + l.chunks <= chunk_item.size() (batch_tables_ex_ok)
        if (!is_permutation(x.o.chunk_order.data() + l.chunk0, l.chunks)) return false;
    return true;
}

namespace {
// memcpy / memcmp that take an empty table (a null pointer with n == 0)
inline void copy_table(void* dst, const void* src, size_t n) {
    if (n) memcpy(dst, src, n);
}
inline bool same_table(const void* a, const void* b, size_t n) { return n == 0 || memcmp(a, b, n) == 0; }
// the device address of field `member` of request r's words in an image at `image`
#define MH_WORD_ADDR(image, lay, r, member) \
    ((image) + (lay).o_words + (uint64_t)(r) * sizeof(BatchBoundWords) + offsetof(BatchBoundWords, member))
}  // namespace

void build_first_hits_batch_image(const BatchTables& t, const BatchFastTables& f, const FirstHitsBatchTables& x,
                                  const BatchRequest* reqs, const uint64_t* targets, const uint64_t* ks,
                                  const FirstHitsBatchAddrs& at, uint8_t* image) {
    const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
    const size_t ni = f.items.size(), chunks = f.chunk_item.size();
    const FirstHitsBatchLayout l = first_hits_batch_layout(ne, nreq, tiles, ni, chunks);
    memset(image, 0, l.bytes);
    copy_table(image, t.entries.data(), ne * sizeof(BatchEntry));
    copy_table(image + l.o_seg, t.seg.data(), (nreq + 1u) * sizeof(uint32_t));
    copy_table(image + l.o_tile, t.tile_entry.data(), tiles * sizeof(uint32_t));
    copy_table(image + l.o_ereq, x.o.entry_req.data(), ne * sizeof(uint32_t));
    copy_table(image + l.o_order, x.o.tile_order.data(), tiles * sizeof(uint32_t));
    BatchBoundWords* w = (BatchBoundWords*)(image + l.o_words);
    for (size_t r = 0; r < nreq; ++r) {
        const BatchRequest& q = reqs[t.req_idx[r]];
        const uint64_t span = q.upper - q.lower;
        w[r] = BatchBoundWords{targets[t.req_idx[r]], 0ull, x.region[r].offset, x.region[r].slots, ks[t.req_idx[r]], ~0ull,
                               q.lower, span, first_hits_shift(span), 0u, 0ull};
    }
    BatchBoundItem* items = (BatchBoundItem*)(image + l.o_item);
    for (size_t k = 0; k < ni; ++k) {
        const uint32_t r = x.o.item_req[k];
        BatchBoundItem it;
        memset(&it, 0, sizeof it);
        it.args = f.items[k].args;
        it.unused = nullptr;
        it.h.h = HitsArgs{w[r].target, (unsigned long long*)MH_WORD_ADDR(at.image, l, r, cursor),
                          (Hit*)(at.hits + w[r].offset * sizeof(Hit)), w[r].slots};
        it.h.k = w[r].k;
        it.h.bound = (unsigned long long*)MH_WORD_ADDR(at.image, l, r, bound);
        it.h.slices = (uint32_t*)(at.slices + (uint64_t)r * kFirstHitsSlices * sizeof(uint32_t));
        it.h.lower = w[r].lower;
        it.h.span = w[r].span;
        it.h.shift = w[r].shift;
        it.h.pad_ = 0u;
        it.h.scanned = (unsigned long long*)MH_WORD_ADDR(at.image, l, r, scanned);
        it.chunk0 = f.items[k].chunk0;
        it.slot0 = f.items[k].slot0;
        items[k] = it;
    }
    copy_table(image + l.o_chunk, f.chunk_item.data(), chunks * sizeof(uint32_t));
    copy_table(image + l.o_corder, x.o.chunk_order.data(), chunks * sizeof(uint32_t));
}

bool first_hits_batch_image_ok(const BatchTables& t, const BatchFastTables& f, const FirstHitsBatchTables& x,
                               const BatchRequest* reqs, const FirstHitsBatchAddrs& at, uint64_t window_slots,
                               const uint8_t* image) {
    const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
    const size_t ni = f.items.size(), chunks = f.chunk_item.size();
    if (nreq > kBatchMaxRequests || x.region.size() != nreq || x.o.item_req.size() != ni) return false;
    if (x.o.entry_req.size() != ne || x.o.tile_order.size() != tiles || x.o.chunk_order.size() != chunks) return false;
    const FirstHitsBatchLayout l = first_hits_batch_layout(ne, nreq, tiles, ni, chunks);
    if (!same_table(image + l.o_ereq, x.o.entry_req.data(), ne * sizeof(uint32_t)) ||
        !same_table(image + l.o_order, x.o.tile_order.data(), tiles * sizeof(uint32_t)) ||
        !same_table(image + l.o_chunk, f.chunk_item.data(), chunks * sizeof(uint32_t)) ||
        !same_table(image + l.o_corder, x.o.chunk_order.data(), chunks * sizeof(uint32_t)))
        return false;
    const BatchBoundWords* w = (const BatchBoundWords*)(image + l.o_words);
    for (size_t r = 0; r < nreq; ++r) {
        const BatchRequest& q = reqs[t.req_idx[r]];
        const uint64_t span = q.upper - q.lower;
        if (w[r].offset != x.region[r].offset || w[r].slots != x.region[r].slots) return false;
        if (w[r].offset > window_slots || w[r].slots > window_slots - w[r].offset) return false;
        if (w[r].lower != q.lower || w[r].span != span || w[r].shift != first_hits_shift(span) || w[r].pad_ != 0u) return false;
        if (first_hits_slices(span, w[r].shift) > kFirstHitsSlices) return false;
        if (w[r].k == 0u || w[r].cursor != 0ull || w[r].bound != ~0ull || w[r].scanned != 0ull) return false;
    }
    const BatchBoundItem* items = (const BatchBoundItem*)(image + l.o_item);
    for (size_t k = 0; k < ni; ++k) {
        const uint32_t r = x.o.item_req[k];
        if (r >= nreq) return false;
        const BatchBoundItem& it = items[k];
        if (memcmp(&it.args, &f.items[k].args, sizeof(FastArgs)) || it.unused != nullptr) return false;
        if (it.chunk0 != f.items[k].chunk0 || it.slot0 != f.items[k].slot0) return false;
        if (it.h.h.target != w[r].target || it.h.k != w[r].k || it.h.lower != w[r].lower || it.h.span != w[r].span ||
            it.h.shift != w[r].shift || it.h.pad_ != 0u)
            return false;
        if ((uint64_t)it.h.h.cursor != MH_WORD_ADDR(at.image, l, r, cursor) ||
            (uint64_t)it.h.bound != MH_WORD_ADDR(at.image, l, r, bound) ||
            (uint64_t)it.h.scanned != MH_WORD_ADDR(at.image, l, r, scanned))
            return false;
        if ((uint64_t)it.h.h.hits != at.hits + w[r].offset * sizeof(Hit) || it.h.h.cap != w[r].slots) return false;
        if ((uint64_t)it.h.slices != at.slices + (uint64_t)r * kFirstHitsSlices * sizeof(uint32_t)) return false;
    }
    return true;
}
#undef MH_WORD_ADDR

bool read_first_hits_batch(Hit* got, uint64_t count, uint64_t slots, uint64_t k, uint64_t* stored, uint64_t* hash,
                           uint64_t* nonce) {
    if (count > slots) return false;
    std::sort(got, got + count, [](const Hit& x, const Hit& y) { return x.nonce < y.nonce; });
    *stored = std::min(count, k);
    if (*stored == k && k != 0u) {
        *hash = got[0].hash;
        *nonce = got[0].nonce;
        for (uint64_t i = 1; i < k; ++i)
            if (got[i].hash < *hash || (got[i].hash == *hash && got[i].nonce < *nonce)) {
                *hash = got[i].hash;
                *nonce = got[i].nonce;
            }
    }
    return true;
}

}  // namespace mh

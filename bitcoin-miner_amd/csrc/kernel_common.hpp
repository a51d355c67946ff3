// kernel_common.hpp -- device helpers shared by the search kernels
// (search_kernels.hip) and the fast run kernel (fast_search.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "layout.hpp"

namespace mh {
namespace dev {


__device__ __forceinline__ bool lex_less(uint64_t ha, uint64_t na, uint64_t hb, uint64_t nb) {
    return ha < hb || (ha == hb && na < nb);
}

// One exchange step of the wave reduction: the partner's (hash, nonce),
// fetched dword by dword by a DPP move (CTRL < 0x200: CTRL is the dpp_ctrl)
// or by a ds_swizzle (CTRL >= 0x200: the swizzle offset is CTRL - 0x200).
template <int CTRL>
__device__ __forceinline__ uint32_t xlane(uint32_t v) {
    if constexpr (CTRL < 0x200)
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
    else
        return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, CTRL - 0x200);
}

template <int CTRL>
__device__ __forceinline__ void wave_step(uint64_t& h, uint64_t& n) {
    const uint64_t oh = ((uint64_t)xlane<CTRL>((uint32_t)(h >> 32)) << 32) | xlane<CTRL>((uint32_t)h);
    const uint64_t on = ((uint64_t)xlane<CTRL>((uint32_t)(n >> 32)) << 32) | xlane<CTRL>((uint32_t)n);
    if (lex_less(oh, on, h, n)) {
        h = oh;
        n = on;
    }
}

// Wave-wide minimum of a u32 (every lane active): DPP butterfly within each
// 16-lane row (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror),
// then the four rows' minima through readlane and scalar mins.  Wave-uniform.
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    return min(min(a, b), min(c, d));
}

// Workgroup lexicographic min; the result is valid in thread 0.
// Wave level: DPP quad_perm [1,0,3,2] and [2,3,0,1], row_half_mirror,
// row_mirror (each step joins two groups whose lanes already agree, so after
// it every lane of the doubled group holds its min), then ds_swizzle xor 16
// (bit mode, within 32 lanes), then lane 0 takes lane 32's value.  Then LDS
// across the workgroup's waves.
template <int NT = kBlockThreads>
__device__ __forceinline__ void block_min(uint64_t& h, uint64_t& n) {
    wave_step<0xB1>(h, n);              // quad_perm [1,0,3,2]: lane ^ 1
    wave_step<0x4E>(h, n);              // quad_perm [2,3,0,1]: lane ^ 2
    wave_step<0x141>(h, n);             // row_half_mirror: quads of 8 lanes
    wave_step<0x140>(h, n);             // row_mirror: halves of 16-lane rows
    wave_step<0x200 + 0x401F>(h, n);    // ds_swizzle and 0x1F, xor 0x10: rows 0<->1, 2<->3
    {
        const uint64_t oh = ((uint64_t)__builtin_amdgcn_readlane((int)(h >> 32), 32) << 32) |
                            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)h, 32);
        const uint64_t on = ((uint64_t)__builtin_amdgcn_readlane((int)(n >> 32), 32) << 32) |
                            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)n, 32);
        if (lex_less(oh, on, h, n)) {
            h = oh;
            n = on;
        }
    }
    __shared__ uint64_t sh[NT / 64], sn[NT / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        sh[wv] = h;
        sn[wv] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 1; i < NT / 64; ++i)
            if (lex_less(sh[i], sn[i], h, n)) {
                h = sh[i];
                n = sn[i];
            }
    }
}

// w[wi] += v for a word index that is not a compile-time constant, without
// dynamic register indexing (which would go to scratch).
template <int NW>
__device__ __forceinline__ void add_word(uint32_t (&w)[NW], uint32_t wi, uint32_t v) {
#pragma unroll
    for (int x = 0; x < NW; ++x) w[x] += (wi == (uint32_t)x) ? v : 0u;
}

// mh_search_first_hits (layout.hpp HitsStopArgs): lower the search's bound word from the slice
// counters.  Called by a whole wave (every lane active) that has just appended hits and got back a
// cursor value which, with its own hits, reaches k -- on the rare hit branch only.  Lane l sums
// counters 16 l .. 16 l + 15 (relaxed agent-scope vector loads, past this CU's L1: other
// workgroups' atomics write them), a scalar walk over the lanes' sums finds the lane whose slices
// take the prefix sum to k, and that lane reads its counters again to find the slice and lowers
// the word to the slice's last nonce (first_hits_slice_end: no 64-bit overflow).  The counters only
// grow, and any values no larger than the true counts give a valid bound, so the two readings need
// not agree.  Every appending wave adds its hits to their slices, and has the counts back, before
// it advances the cursor, so the counts read here hold at least k hits; were they seen lower all
// the same, nothing is published: never a wrong bound.  The counters are summed, not kept, and the
// owner's loop stays rolled: sixteen counters held in VGPRs across the walk cost the kernel around
// this rare branch registers, and its per-nonce loop two or three VALU instructions.
__device__ __forceinline__ void publish_first_hits_bound(const HitsStopArgs& hs, uint32_t lane) {
    constexpr uint32_t PER = kFirstHitsSlices / 64u;
    const uint32_t k = (uint32_t)hs.k;  // <= MH_HITS_MAX_CAP = 2^20
    const uint32_t* mine = hs.slices + lane * PER;
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < PER; ++i) sum += __hip_atomic_load(mine + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t ls = sum < (uint64_t)k ? (uint32_t)sum : k;  // clamped: the walk's sums stay below 2^21
    uint32_t acc = 0u, owner = 64u;
    for (uint32_t l = 0; l < 64u; ++l) {
        const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)ls, (int)l);
        if (acc + v >= k) {
            owner = l;
            break;
        }
        acc += v;
    }
    if (lane == owner) {  // owner == 64: the counts seen hold fewer than k hits
        uint64_t pre = acc;
        uint32_t s = 0u;
#pragma nounroll
        for (; s < PER - 1u; ++s) {  // (the last counter is not read: the prefix reaches k there at the latest)
            pre += __hip_atomic_load(mine + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (pre >= (uint64_t)k) break;
        }
        atomicMin(hs.bound, (unsigned long long)first_hits_slice_end(hs.lower, hs.span, hs.shift, lane * PER + s));
    }
}

// The slice counter of nonce n, for the add of an appended hit (n lies in the range; the index is
// cut to the counters all the same).
__device__ __forceinline__ uint32_t* first_hits_slice(const HitsStopArgs& hs, uint64_t n) {
    const uint64_t s = (n - hs.lower) >> hs.shift;
    return hs.slices + (s < (uint64_t)kFirstHitsSlices ? (uint32_t)s : kFirstHitsSlices - 1u);
}

}  // namespace dev
}  // namespace mh

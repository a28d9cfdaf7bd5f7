// gns_coldmask.cuh -- K1's cold-packet mask (one 64-bit word per 64 packets of
// a K1 block, bit l of word i = packet 64 i + l is inserted and has a row that
// is not designated) expanded into the list of those packets' offsets, which
// K3s takes in sub-passes.  Pure functions, host and device (tests/test_coldmask_cpu.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GNS_CM_HD __host__ __device__ inline
#else
#define GNS_CM_HD inline
#endif

namespace gns {

constexpr uint32_t kColdNone = 0xFFFFu;  // list entry of a rank past the block's cold packets

// rank of bit l of `word` among the set bits of the block's mask, given the
// popcount of the words before it
GNS_CM_HD uint32_t cold_rank(uint64_t word, uint32_t prefix, uint32_t l) {
    return prefix + (uint32_t)__builtin_popcountll(word & ((1ull << l) - 1ull));
}

// Lane l's share of expanding words [i0, i1) into list[]: the packets of ranks
// [lo, lo + cap) get list[rank - lo] = 64 i + l.  prefix[i] = set bits in
// words 0..i-1.  All 64 lanes together write each rank of the window that
// exists exactly once; nothing else is written.
GNS_CM_HD void cold_expand_lane(const uint64_t *words, const uint32_t *prefix, uint32_t i0, uint32_t i1, uint32_t l,
                                uint32_t lo, uint32_t cap, uint16_t *list) {
#pragma unroll 1  // (unrolled, K3s would carry every word's addresses through its main loop)
    for (uint32_t i = i0; i < i1; i++) {
        const uint64_t w = words[i];
        const uint32_t rk = cold_rank(w, prefix[i], l) - lo;  // below lo: wraps past cap
        if (((w >> l) & 1ull) && rk < cap) list[rk] = (uint16_t)(64u * i + l);
    }
}

}  // namespace gns

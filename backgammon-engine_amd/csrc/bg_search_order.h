// bg_search_order.h -- the search's order of candidates and its roll count: what bg_search.h (inside bgamd.hip) and the 3-ply step's
// kernels (bgamd_search3.hip, a translation unit of its own) must agree on.  Included inside the anonymous namespace of either file.
#pragma once

constexpr int SRCH_ROLLS = 21;

// larger = better for the mover, then smaller key (the greedy step's best_atomic_max order)
__device__ __forceinline__ unsigned long long srch_pack(float v, uint32_t key, int mover)
{
    uint32_t bits = __float_as_uint(v);
    bits = mover ? ~bits : bits;
    return ((unsigned long long)bits << 32) | (uint32_t)~key;
}

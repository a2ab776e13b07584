// bg_stream_store.h -- the write-through store of the root terms that the boundary launch's root pass writes (bg_root_resident.h): the
// launch never reads them again, their reader is the value net a launch later.  A plain store leaves its line dirty in the XCD's L2, to
// be written back when the launch ends, on the next launch's critical path; the sc1 bit makes the store write through and drop the line.
// Inline asm: hipcc counts no memory operation of an asm statement -- nothing in the launch may read the bytes back (no wait covers the
// store; the end of the wave does); the compiler's own vmcnt waits stay safe (the counter is in order: an uncounted store only makes a
// wait longer); the statement ends with the wait states the data register needs before it is overwritten (s_nop 1).
// Where the flavour was tried and what it measured (it pays only for stores spread under other work): profiles/ab_kernel_tails.txt.
// -DBG_STREAM_STORES=0: a plain store (the A/B of the flavour alone).
#pragma once
#include <hip/hip_runtime.h>

#ifndef BG_STREAM_STORES
#define BG_STREAM_STORES 1
#endif

namespace bg {

__device__ __forceinline__ void stream_store(float *p, float v)
{
#if BG_STREAM_STORES
    asm volatile("global_store_dword %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
#else
    *p = v;
#endif
}

}  // namespace bg

// The owner of a handle's device memory (bgamd_env, bgamd_td).  Host-only, plain C++17, no HIP headers: g++ compiles it, and
// tests/sanitize/devmem_driver.cpp runs it over a fake backend with every allocation failing in turn.
// THE RULE: a new buffer is a pointer member and one allocation call; destroy frees what was handed out.  The owner records every
// block it hands out BY VALUE, so release_all() needs no list of members, does not care who else holds a copy of a pointer (the *View
// structs, a scratch env's borrowed tables, sv.tops moving between its two sets) and frees each block exactly once.
// Backend: int alloc(void **p, size_t bytes, const char *name), int alloc_pinned(the same), void free(void *), void free_pinned(void *).
// The allocators return 0, or the error code the owner passes on after recording a text that names the buffer: how is theirs alone.
#pragma once
#include <cstddef>
#include <initializer_list>
#include <vector>

namespace bg {
struct DevBuf { void **ptr; size_t bytes; const char *name; };     // (where the pointer goes, bytes -- grow(): per element --, its name)
#define BG_BUF(p, bytes) bg::DevBuf{(void **)&(p), (size_t)(bytes), #p}

template <class Backend> class DevMemOwner {
public:
    Backend backend;
    DevMemOwner() = default;
    DevMemOwner(const DevMemOwner &) = delete;         // (a copy would free the same blocks again)
    DevMemOwner &operator=(const DevMemOwner &) = delete;
    // One block of device / of pinned host memory.  On failure *b.ptr is null.
    int alloc(const DevBuf &b) { return take(b.ptr, b.bytes, b.name, false); }
    int alloc_pinned(const DevBuf &b) { return take(b.ptr, b.bytes, b.name, true); }
    // All of these (n x bytes each) or none: on failure what this call allocated is freed again and EVERY pointer of the group is null,
    // so "the first pointer is there" says that all are.  The pointers are overwritten, not freed: null (or stale) on entry.
    int alloc_group(std::initializer_list<DevBuf> bufs, size_t n = 1)
    {
        for (const DevBuf *b = bufs.begin(); b != bufs.end(); ++b)
            if (const int rc = take(b->ptr, n * b->bytes, b->name, false)) {
                for (const DevBuf *u = bufs.begin(); u != b; ++u) give_back(*u->ptr);
                for (const DevBuf &u : bufs) *u.ptr = nullptr;
                return rc;
            }
        return 0;
    }
    // Buffers that grow on demand: `need` elements of b.bytes each in every one of bufs.  A no-op when need <= cap; else the old blocks
    // are freed and all allocated anew, and cap is set only once every allocation has succeeded.  After a failure every pointer is null
    // and cap is 0 -- the state of a handle that never grew, which the next call repairs.
    int grow(long long need, long long &cap, std::initializer_list<DevBuf> bufs)
    {
        if (need <= cap) return 0;
        for (const DevBuf &b : bufs) { give_back(*b.ptr); *b.ptr = nullptr; }
        cap = 0;
        if (const int rc = alloc_group(bufs, (size_t)need)) return rc;
        cap = need;
        return 0;
    }
    // Frees everything still owned.  Idempotent; the members that pointed at the blocks are the caller's to forget (destroy deletes them).
    void release_all()
    {
        for (const Block &k : owned) k.pinned ? backend.free_pinned(k.p) : backend.free(k.p);
        owned.clear();
    }
private:
    struct Block { void *p; bool pinned; };
    std::vector<Block> owned;
    int take(void **p, size_t bytes, const char *name, bool pinned)
    {
        *p = nullptr;
        const int rc = pinned ? backend.alloc_pinned(p, bytes, name) : backend.alloc(p, bytes, name);
        if (rc) *p = nullptr;
        else if (*p) owned.push_back(Block{*p, pinned});
        return rc;
    }
    void give_back(void *p)                            // a device block of ours (or null): freed and forgotten
    {
        for (size_t i = owned.size(); p && i-- > 0;)
            if (owned[i].p == p) { backend.free(p); owned.erase(owned.begin() + (long)i); return; }
    }
};
}  // namespace bg

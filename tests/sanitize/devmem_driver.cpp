// Driver for the owner of a handle's device memory (csrc/bg_devmem.h, plain C++), built by tests/test_devmem_cpu.py and, with
// g++ -fsanitize=address,undefined, by tests/test_sanitizers_cpu.py.  The owner runs over a fake backend on malloc/free that counts its
// live blocks, aborts on a free of what it did not hand out (a double free is one) or through the wrong one of its two calls, and
// fails the k-th allocation on request.  Scripted sequences shaped like the library's walk it: an env_allocate-like run of single
// allocations, a first-use group behind a one-pointer guard, grows whose needs rise, fall and repeat, a pinned block; then all of them
// as one handle's life.  Every sequence runs clean once and then once per allocation k with that allocation failing:
//   - every pointer of a failed group is null, and the guarded call after it allocates the whole group;
//   - after a failed grow cap is 0 and every pointer null (the documented contract), and the same grow again succeeds;
//   - the error text names the buffer whose allocation failed;
//   - release_all leaves no live block, and a second release_all frees nothing twice.
// Prints "OK <cases>".
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>
#include "bg_devmem.h"

namespace {
struct Fake {                                          // the backend's state: one for the whole program, reset per case
    std::set<void *> device, pinned;
    std::vector<std::string> log;                      // the names of the allocation calls, in order
    size_t fail_at = 0;                                // fail the k-th allocation call (1-based; 0: none)
    std::string error;
} fake;

[[noreturn]] void die(const char *what, const std::string &detail = "")
{
    std::printf("FAILED: %s %s\n", what, detail.c_str());
    std::exit(1);
}
#define CHECK(cond) do { if (!(cond)) die(#cond, "(line " + std::to_string(__LINE__) + ")"); } while (0)

struct FakeBackend {
    static int take(std::set<void *> &live, void **p, size_t bytes, const char *name)
    {
        fake.log.push_back(name);
        if (fake.log.size() == fake.fail_at) { fake.error = std::string("fake alloc(") + name + "): out of memory"; return -2; }
        *p = std::malloc(bytes ? bytes : 1);
        if (!*p) die("malloc");
        live.insert(*p);
        return 0;
    }
    static void give(std::set<void *> &live, void *p)
    {
        if (!live.erase(p)) { std::printf("FAILED: free of a block that is not live\n"); std::abort(); }
        std::free(p);
    }
    int alloc(void **p, size_t bytes, const char *name) { return take(fake.device, p, bytes, name); }
    int alloc_pinned(void **p, size_t bytes, const char *name) { return take(fake.pinned, p, bytes, name); }
    void free(void *p) { give(fake.device, p); }
    void free_pinned(void *p) { give(fake.pinned, p); }
};
using Owner = bg::DevMemOwner<FakeBackend>;

struct Handle {                                        // the members a handle would have
    Owner mem;
    char *single[40] = {};
    int *group[11] = {};
    char *a = nullptr, *b = nullptr, *d = nullptr, *e = nullptr;
    int *c = nullptr, *f = nullptr, *g = nullptr, *h = nullptr;
    long long cap_a = 0, cap_bc = 0, cap_dh = 0, cap_tmp = 0;
    void *tmp = nullptr;
    unsigned long long *host = nullptr;
    float *after_host = nullptr;
};

// ---- the sequences: each returns 0, or the error code at which the library would have given up ----------------------------------

int run_singles(Handle &x)                             // env_allocate: one allocation after the other, out at the first failure
{
    static std::string names[40];
    for (int i = 0; i < 40; ++i) {
        names[i] = "single" + std::to_string(i);
        if (const int rc = x.mem.alloc({(void **)&x.single[i], (size_t)(16 + 8 * i), names[i].c_str()})) {
            for (int j = 0; j < 40; ++j) CHECK((x.single[j] != nullptr) == (j < i));
            return rc;
        }
    }
    return 0;
}

int first_use_group(Handle &x)                         // SearchCall::buffers: `if (!se.cnt)`, then eleven buffers
{
    int *(&p)[11] = x.group;
    if (p[0]) return 0;
    return x.mem.alloc_group({BG_BUF(p[0], 36), BG_BUF(p[1], 36), BG_BUF(p[2], 36), BG_BUF(p[3], 36), BG_BUF(p[4], 36), BG_BUF(p[5], 36),
                              BG_BUF(p[6], 36), BG_BUF(p[7], 8), BG_BUF(p[8], 32), BG_BUF(p[9], 400), BG_BUF(p[10], 400)});
}
int run_group(Handle &x)
{
    const size_t live = fake.device.size();
    int rc = first_use_group(x);
    if (rc) {                                          // all or none: the guard pointer tells the truth, the next call allocates all
        for (int *p : x.group) CHECK(p == nullptr);
        CHECK(fake.device.size() == live);             // (what the failed call had allocated is freed, not merely forgotten)
        rc = first_use_group(x);
    }
    CHECK(rc == 0);
    for (int *p : x.group) CHECK(p != nullptr);
    const size_t calls = fake.log.size();
    CHECK(first_use_group(x) == 0 && fake.log.size() == calls);        // there: not allocated again
    return 0;
}

// one grow, held to its contract whether it fails or not
template <class Grow, class Ptrs> void checked_grow(long long need, long long &cap, Grow grow, Ptrs ptrs)
{
    const long long cap0 = cap;
    const std::vector<void *> before = ptrs();
    const size_t calls = fake.log.size(), live = fake.device.size();
    size_t held = 0;
    for (void *p : before) held += p != nullptr;
    int rc = grow();
    if (need <= cap0) {                                // a no-op: nothing allocated, nothing moved
        CHECK(rc == 0 && cap == cap0 && fake.log.size() == calls && ptrs() == before);
        return;
    }
    if (rc) {                                          // failed: cap 0 and every pointer null, and the same grow again succeeds
        CHECK(cap == 0);
        for (void *p : ptrs()) CHECK(p == nullptr);
        CHECK(fake.device.size() == live - held);      // (the old blocks and what the failed call had allocated: freed)
        rc = grow();
    }
    CHECK(rc == 0 && cap == need && fake.log.size() > calls && fake.device.size() == live - held + before.size());
    for (void *p : ptrs()) CHECK(p != nullptr);
}
int run_grows(Handle &x)                               // the rollout's and the search's buffers, and the scalar surface's d_tmp
{
    Owner &mem = x.mem;
    for (long long n : {3, 10, 10, 4, 25, 1, 25, 40}) {
        checked_grow(n, x.cap_a, [&] { return mem.grow(n, x.cap_a, {BG_BUF(x.a, 32)}); }, [&] { return std::vector<void *>{x.a}; });
        checked_grow(2 * n, x.cap_bc, [&] { return mem.grow(2 * n, x.cap_bc, {BG_BUF(x.b, 32), BG_BUF(x.c, 4)}); },
                     [&] { return std::vector<void *>{x.b, x.c}; });
        const long long m = 30 - n / 2;                // falls while the others rise: grows at the first call and at n = 1
        checked_grow(m, x.cap_dh, [&] { return mem.grow(m, x.cap_dh, {BG_BUF(x.d, 4), BG_BUF(x.e, 32), BG_BUF(x.f, 4), BG_BUF(x.g, 4), BG_BUF(x.h, 84)}); },
                     [&] { return std::vector<void *>{x.d, x.e, x.f, x.g, x.h}; });
        checked_grow(n * 124, x.cap_tmp, [&] { return mem.grow(n * 124, x.cap_tmp, {BG_BUF(x.tmp, 1)}); }, [&] { return std::vector<void *>{x.tmp}; });
    }
    return 0;
}

int run_pinned(Handle &x)                              // RolloutState::host, and a device block behind it
{
    if (!x.host) if (const int rc = x.mem.alloc_pinned(BG_BUF(x.host, 64))) { CHECK(x.host == nullptr); return rc; }
    CHECK(fake.pinned.size() == 1 && fake.pinned.count(x.host));
    if (const int rc = x.mem.alloc(BG_BUF(x.after_host, 84))) { CHECK(x.after_host == nullptr); return rc; }
    return 0;
}

int run_life(Handle &x)                                // create, then every feature once
{
    int rc;
    if ((rc = run_singles(x)) || (rc = run_group(x)) || (rc = run_grows(x)) || (rc = run_pinned(x))) return rc;
    return 0;
}

// ---- one sequence: clean, then with each of its allocations failing ------------------------------------------------------------
long long cases = 0;

std::vector<std::string> one_case(int (*sequence)(Handle &), size_t fail_at)
{
    fake = Fake{};
    fake.fail_at = fail_at;
    {
        Handle x;
        const int rc = sequence(x);
        if (fail_at) {
            CHECK(fake.log.size() >= fail_at);         // the failure happened ...
            CHECK(fake.error.find("(" + fake.log[fail_at - 1] + ")") != std::string::npos);      // ... and its text names the buffer
        } else CHECK(rc == 0 && fake.error.empty());
        x.mem.release_all();
        CHECK(fake.device.empty() && fake.pinned.empty());
        x.mem.release_all();                           // idempotent: the backend aborts on a second free
    }
    ++cases;
    return fake.log;
}

void walk(const char *name, int (*sequence)(Handle &), size_t want_allocations)
{
    const std::vector<std::string> clean = one_case(sequence, 0);
    if (clean.size() != want_allocations) die(name, "allocates " + std::to_string(clean.size()) + " times");
    for (size_t k = 1; k <= clean.size(); ++k) {
        const std::vector<std::string> log = one_case(sequence, k);
        for (size_t i = 0; i < k; ++i) CHECK(log[i] == clean[i]);      // (the same run up to the failure: the k-th call is the clean run's)
    }
}
}  // namespace

int main()
{
    walk("singles", run_singles, 40);
    walk("group", run_group, 11);
    walk("grows", run_grows, 4 * 1 + 4 * 2 + 2 * 5 + 4 * 1);            // a, b c and tmp grow at 3, 10, 25, 40; d .. h twice
    walk("pinned", run_pinned, 2);
    walk("life", run_life, 40 + 11 + 26 + 2);
    std::printf("OK %lld\n", cases);
    return 0;
}

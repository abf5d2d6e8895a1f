// The scratch holder of the host code (pa::Bufs, csrc/pa_internal.h) against a
// malloc-backed allocator: what it frees, when, and in which order.  Built with
// -fsanitize=address,undefined by tests/test_bufs_host.py, so a double free, a
// leak or a use after free ends the program with a report; exit status 0 means
// every check held.  No GPU and no HIP runtime: the three functions the holder
// calls are defined here.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pa_internal.h"

namespace {
std::vector<std::string> g_log;   // "sync", "free <n>": the order of events
std::vector<void *> g_given;      // allocation n is g_given[n]
int g_fail_at = -1;               // the allocation that is to fail (-1: none)
int g_failed = 0;

int number_of(void *p) {
    for (size_t i = 0; i < g_given.size(); i++)
        if (g_given[i] == p) return (int)i;
    return -1;
}

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                   \
        }                                                                 \
    } while (0)

void expect_log(std::vector<std::string> want, int line) {
    if (g_log != want) {
        fprintf(stderr, "line %d: events", line);
        for (auto &s : g_log) fprintf(stderr, " [%s]", s.c_str());
        fprintf(stderr, ", expected");
        for (auto &s : want) fprintf(stderr, " [%s]", s.c_str());
        fprintf(stderr, "\n");
        g_failed++;
    }
    g_log.clear();
}
#define EXPECT_LOG(...) expect_log({__VA_ARGS__}, __LINE__)
}  // namespace

namespace pa {
hipError_t dev_malloc_raw(void **p, size_t n) {
    if ((int)g_given.size() == g_fail_at) {
        g_fail_at = -1;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(n);
    g_given.push_back(*p);
    return hipSuccess;
}
hipError_t dev_free(void *p) {
    if (!p) return hipSuccess;
    g_log.push_back("free " + std::to_string(number_of(p)));
    std::free(p);
    return hipSuccess;
}
}  // namespace pa

extern "C" hipError_t hipStreamSynchronize(hipStream_t) {
    g_log.push_back("sync");
    return hipSuccess;
}

int main() {
    using pa::Bufs;
    {  // an empty holder does nothing
        Bufs b(nullptr);
    }
    EXPECT_LOG();
    {  // the destructor: one wait for the stream, then everything, newest first
        Bufs b(nullptr);
        char *a = nullptr;
        uint64_t *c = nullptr;
        uint32_t *d = nullptr;
        CHECK(b.get(&a, 100) == hipSuccess && a);
        CHECK(b.get(&c, 0) == hipSuccess && c);  // (never a zero-byte allocation)
        CHECK(b.get(&d, 4) == hipSuccess && d);
        a[99] = 1, c[1] = 2, d[3] = 3;            // 0 and 4 bytes are rounded up to 16
        EXPECT_LOG();
    }
    EXPECT_LOG("sync", "free 2", "free 1", "free 0");
    char *kept = nullptr;
    {  // release: out of the holder, still allocated
        Bufs b(nullptr);
        char *tmp = nullptr;
        CHECK(b.get(&kept, 64) == hipSuccess);
        CHECK(b.get(&tmp, 64) == hipSuccess);
        CHECK(b.release(kept) == kept);
    }
    EXPECT_LOG("sync", "free 4");
    kept[63] = 7;  // (a use after free here is an ASan report)
    pa::dev_free(kept);
    EXPECT_LOG("free 3");
    {  // the early free: now, after a wait, the pointer cleared; not again at the end
        Bufs b(nullptr);
        char *big = nullptr, *small = nullptr, *none = nullptr;
        CHECK(b.get(&big, 1 << 20) == hipSuccess);
        CHECK(b.get(&small, 8) == hipSuccess);
        b.free(big);
        CHECK(big == nullptr);
        EXPECT_LOG("sync", "free 5");
        b.free(big);   // (cleared: nothing)
        b.free(none);  // (never allocated: nothing)
        EXPECT_LOG();
        CHECK(b.get(&big, 1 << 10) == hipSuccess);  // the grow loop's next size
    }
    EXPECT_LOG("sync", "free 7", "free 6");
    {  // a failed allocation: the error returned, the pointer null, nothing held for it
        Bufs b(nullptr);
        char *a = nullptr, *f = (char *)1;
        CHECK(b.get(&a, 32) == hipSuccess);
        g_fail_at = (int)g_given.size();
        CHECK(b.get(&f, 32) == hipErrorOutOfMemory);
        CHECK(f == nullptr);
    }
    EXPECT_LOG("sync", "free 8");
    {  // adopt: a buffer taken elsewhere is the holder's from then on (null: nothing)
        Bufs b(nullptr);
        void *p = nullptr;
        CHECK(pa::dev_malloc_raw(&p, 48) == hipSuccess);
        b.adopt(p);
        b.adopt(nullptr);
    }
    EXPECT_LOG("sync", "free 9");
    {  // with_temp: the size query, the temporary in the holder, the run
        Bufs b(nullptr);
        int calls = 0;
        void *seen = nullptr;
        const hipError_t e = pa::with_temp(b, [&](void *tmp, size_t &bytes) {
            calls++;
            if (!tmp) {
                bytes = 256;
                return hipSuccess;
            }
            seen = tmp;
            static_cast<char *>(tmp)[255] = 1;
            return bytes == 256 ? hipSuccess : hipErrorInvalidValue;
        });
        CHECK(e == hipSuccess && calls == 2 && seen == g_given.back());
        // ... and a failed allocation between the two ends it with that error
        g_fail_at = (int)g_given.size();
        calls = 0;
        CHECK(pa::with_temp(b, [&](void *, size_t &bytes) {
                  calls++;
                  bytes = 8;
                  return hipSuccess;
              }) == hipErrorOutOfMemory);
        CHECK(calls == 1);
    }
    EXPECT_LOG("sync", "free 10");
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("bufs ok\n");
    return 0;
}

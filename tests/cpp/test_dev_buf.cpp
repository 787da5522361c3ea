// Host test of the ownership rules of the device buffer (csrc/dev_buf.h): the template over a counting allocator that wraps
// malloc / free.  Stand-alone: built with -fsanitize=address,undefined by dev_buf.mk, so a double free, a leak or a use of a
// freed block is reported by the sanitizer as well as by the counts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

#include "dev_buf.h"

static int failures = 0;
#define CHECK_EQ(a, b)                                                                                          \
    do {                                                                                                        \
        const long long x_ = (long long)(a), y_ = (long long)(b);                                               \
        if (x_ != y_) { printf("FAIL %s:%d  %s = %lld, expected %lld\n", __FILE__, __LINE__, #a, x_, y_); failures++; } \
    } while (0)

// malloc / free with the sizes kept in a small table: calls, live blocks and bytes, the last request, N failures on demand
struct Counting {
    static constexpr int kErr = 7, kFailed = 2;
    static inline long allocs = 0, frees = 0, live = 0, live_bytes = 0, forgotten = 0, reported = 0;
    static inline size_t last_request = 0, last_failed_bytes = 0;
    static inline int fail_next = 0;
    struct Block { void* p; size_t n; };
    static inline Block blocks[16] = {};
    static int alloc(void** p, size_t bytes) {
        allocs++;
        last_request = bytes;
        if (fail_next > 0) { fail_next--; return kErr; }
        *p = malloc(bytes);
        memset(*p, 0xAB, bytes);       // the whole block is the buffer's: a short allocation would be written past
        for (Block& b : blocks) if (!b.p) { b.p = *p; b.n = bytes; break; }
        live++;
        live_bytes += (long)bytes;
        return 0;
    }
    static void free(void* p) {
        frees++;
        live--;
        for (Block& b : blocks) if (b.p == p) { live_bytes -= (long)b.n; b.p = nullptr; break; }
        ::free(p);
    }
    static void forget(int e) { if (e == kErr) forgotten++; }
    static int failed(size_t bytes, int e) { reported += e == kErr; last_failed_bytes = bytes; return kFailed; }
};
typedef vlq_detail::BasicDevBuf<Counting> Buf;

static_assert(!std::is_copy_constructible<Buf>::value, "a buffer owns its block: no copy construction");
static_assert(!std::is_copy_assignable<Buf>::value, "a buffer owns its block: no copy assignment");
static_assert(std::is_nothrow_move_constructible<Buf>::value && std::is_nothrow_move_assignable<Buf>::value, "moves");

int main() {
    typedef Counting C;
    {
        Buf b;
        CHECK_EQ(b.p == nullptr, 1);
        CHECK_EQ(b.cap, 0);
        CHECK_EQ(b.reserve(0), 0);                 // nothing asked, nothing allocated
        CHECK_EQ(C::allocs, 0);
        // growth asks for bytes + bytes / 8 + 256
        CHECK_EQ(b.reserve(1000), 0);
        CHECK_EQ(C::allocs, 1);
        CHECK_EQ(C::last_request, 1000 + 125 + 256);
        CHECK_EQ(b.cap, 1381);
        CHECK_EQ(b.as<char>() == (char*)b.p, 1);
        // within the capacity: no allocation, the same block
        void* p0 = b.p;
        CHECK_EQ(b.reserve(10), 0);
        CHECK_EQ(b.reserve(1381), 0);
        CHECK_EQ(C::allocs, 1);
        CHECK_EQ(b.p == p0, 1);
        // one byte more: the old block is freed, the new one is padded again
        CHECK_EQ(b.reserve(1382), 0);
        CHECK_EQ(C::allocs, 2);
        CHECK_EQ(C::frees, 1);
        CHECK_EQ(C::last_request, 1382 + 172 + 256);
        CHECK_EQ(C::live, 1);
        CHECK_EQ(C::live_bytes, 1810);
        // the padded allocation fails: the exact one is tried
        C::fail_next = 1;
        CHECK_EQ(b.reserve(4000), 0);
        CHECK_EQ(C::allocs, 4);
        CHECK_EQ(C::forgotten, 1);
        CHECK_EQ(C::last_request, 4000);
        CHECK_EQ(b.cap, 4000);
        CHECK_EQ(C::live, 1);
        CHECK_EQ(C::live_bytes, 4000);
        // both fail: an error, the buffer is empty, the old block is gone (growth discards it first)
        C::fail_next = 2;
        CHECK_EQ(b.reserve(5000), C::kFailed);
        CHECK_EQ(C::reported, 1);
        CHECK_EQ(C::last_failed_bytes, 5000);
        CHECK_EQ(b.p == nullptr, 1);
        CHECK_EQ(b.cap, 0);
        CHECK_EQ(C::live, 0);
        // ... and usable again
        CHECK_EQ(b.reserve(64), 0);
        CHECK_EQ(C::live, 1);
        b.release();
        CHECK_EQ(C::live, 0);
        CHECK_EQ(b.p == nullptr, 1);
        CHECK_EQ(b.cap, 0);
        b.release();                               // an empty buffer frees nothing
        CHECK_EQ(b.reserve(64), 0);
    }
    // the destructor frees exactly once
    CHECK_EQ(C::live, 0);
    CHECK_EQ(C::allocs, 8);
    CHECK_EQ(C::frees, 5);
    {
        // move construction: the source is left empty and frees nothing
        const long frees0 = C::frees;
        {
            Buf a;
            CHECK_EQ(a.reserve(100), 0);
            void* pa = a.p;
            const size_t ca = a.cap;
            {
                Buf b(std::move(a));
                CHECK_EQ(b.p == pa, 1);
                CHECK_EQ(b.cap, ca);
                CHECK_EQ(a.p == nullptr, 1);
                CHECK_EQ(a.cap, 0);
                CHECK_EQ(C::frees, frees0);
            }
            CHECK_EQ(C::frees, frees0 + 1);        // b's destructor
            CHECK_EQ(C::live, 0);
        }
        CHECK_EQ(C::frees, frees0 + 1);            // the moved-from a: nothing
    }
    {
        // move assignment frees the target's old block and takes the source's
        Buf a, b;
        CHECK_EQ(a.reserve(100), 0);
        CHECK_EQ(b.reserve(200), 0);
        void* pa = a.p;
        const long frees0 = C::frees, allocs0 = C::allocs;
        b = std::move(a);
        CHECK_EQ(C::frees, frees0 + 1);
        CHECK_EQ(C::allocs, allocs0);
        CHECK_EQ(C::live, 1);
        CHECK_EQ(C::live_bytes, 100 + 12 + 256);
        CHECK_EQ(b.p == pa, 1);
        CHECK_EQ(a.p == nullptr, 1);
        CHECK_EQ(a.cap, 0);
        // self-move-assignment keeps the block
        Buf& self = b;
        b = std::move(self);
        CHECK_EQ(b.p == pa, 1);
        CHECK_EQ(b.cap, 100 + 12 + 256);
        CHECK_EQ(C::frees, frees0 + 1);
        memset(b.p, 0, b.cap);                     // still this buffer's block
    }
    CHECK_EQ(C::live, 0);
    {
        // std::swap exchanges the blocks: no allocation, no free (lists.hip exchanges the lists' arrays this way)
        Buf a, b, e;
        CHECK_EQ(a.reserve(100), 0);
        CHECK_EQ(b.reserve(300), 0);
        void *pa = a.p, *pb = b.p;
        const size_t ca = a.cap, cb = b.cap;
        const long frees0 = C::frees, allocs0 = C::allocs;
        std::swap(a, b);
        CHECK_EQ(a.p == pb, 1);
        CHECK_EQ(b.p == pa, 1);
        CHECK_EQ(a.cap, cb);
        CHECK_EQ(b.cap, ca);
        std::swap(a, e);                           // with an empty one
        CHECK_EQ(a.p == nullptr, 1);
        CHECK_EQ(e.p == pb, 1);
        CHECK_EQ(C::frees, frees0);
        CHECK_EQ(C::allocs, allocs0);
        CHECK_EQ(C::live, 2);
    }
    CHECK_EQ(C::live, 0);
    CHECK_EQ(C::live_bytes, 0);
    CHECK_EQ(C::allocs - (C::forgotten + C::reported), C::frees);      // every block that was handed out was freed once
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("all ok\n");
    return 0;
}

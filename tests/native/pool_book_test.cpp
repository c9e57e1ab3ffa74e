// Stand-alone host program for padne_amd/csrc/pool_book.hpp, the bookkeeping of the device allocator: driven with
// aligned_alloc / free in place of the device's allocate / free pair, built with -fsanitize=address,undefined by
// tests/test_pool_book_host.py.  No device code is involved.
#include "../../padne_amd/csrc/pool_book.hpp"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>

using padne::PoolBook;

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                      \
        }                                                                    \
    } while (0)

static std::set<void *> g_device;       // what the fake device has handed out and not got back

static void *fake_alloc(size_t bytes) {
    void *p = aligned_alloc(256, bytes);       // hipMalloc's alignment
    memset(p, 0x11, bytes);
    g_device.insert(p);
    return p;
}
static void fake_free(void *p) {
    CHECK(g_device.erase(p) == 1);             // freed once, and only what was allocated
    free(p);
}

// what pool_alloc does with the book
static void *alloc(PoolBook &book, size_t bytes, bool guarded, unsigned char canary = 0xa5) {
    void *p = book.take(bytes, guarded, canary);
    if (p == nullptr) p = book.adopt(fake_alloc(PoolBook::underlying(bytes, guarded)), bytes, guarded, canary);
    const PoolBook::Block *b = book.find(p);
    CHECK(b != nullptr && !b->cached && b->guarded == guarded);
    if (guarded) {       // the three fills of pool_guard_arm stay inside the underlying allocation (ASan watches)
        memset(b->base, canary, b->front());
        memset(p, 0xff, b->requested);
        memset((char *)b->base + b->back_begin(), canary, b->back_bytes());
    }
    return p;
}

static void test_rounding() {
    CHECK(PoolBook::round(0) == 256 && PoolBook::round(1) == 256 && PoolBook::round(256) == 256);
    CHECK(PoolBook::round(257) == 512 && PoolBook::round(1000) == 1024);
    CHECK(PoolBook::round(((size_t)1 << 20) - 1) == (size_t)1 << 20 && PoolBook::round((size_t)1 << 20) == (size_t)1 << 20);
    CHECK(PoolBook::round(((size_t)1 << 20) + 1) == (size_t)2 << 20);
    CHECK(PoolBook::underlying(1000, false) == 1024 && PoolBook::underlying(1000, true) == 2048);
    CHECK(PoolBook::underlying(256, true) == 1024 && PoolBook::underlying(0, true) == 512);
    CHECK(PoolBook::underlying(((size_t)1 << 20) - 512, true) == (size_t)1 << 20);
    CHECK(PoolBook::underlying(((size_t)1 << 20) - 511, true) == (size_t)2 << 20);
}

static void test_guard_layout() {
    PoolBook book;
    const size_t sizes[] = {0, 1, 8, 255, 256, 257, 1000, 1024, 4096 - 512, 4096 - 511, 65536, ((size_t)1 << 20) - 512,
                            ((size_t)1 << 20) - 511, (size_t)1 << 20, ((size_t)3 << 20) + 12345};
    for (size_t bytes : sizes) {
        char *p = (char *)alloc(book, bytes, true);
        const PoolBook::Block b = *book.find(p);
        CHECK((uintptr_t)p % 256 == 0);                                // the pointer handed out keeps the alignment
        CHECK(p == (char *)b.base + PoolBook::kGuard && b.front() == PoolBook::kGuard);
        CHECK(b.requested == bytes);                                   // the requested size is remembered
        CHECK(b.back_begin() == PoolBook::kGuard + bytes);             // the back zone starts at the first byte past it
        CHECK(b.back_bytes() >= PoolBook::kGuard && b.back_begin() + b.back_bytes() == b.size);
        CHECK(b.size == PoolBook::underlying(bytes, true));
        CHECK(book.give_back(p, (size_t)1 << 40));
    }
    CHECK(book.cached_bytes > 0);
    book.release_cached(fake_free);
    CHECK(book.cached_bytes == 0 && book.blocks.empty() && g_device.empty());
}

static void test_reuse_and_mode_switch() {
    PoolBook book;
    const size_t limit = (size_t)1 << 40;
    // plain mode: a block comes back from the cache at the same address, whatever the size within the rounding
    void *a = alloc(book, 1000, false);
    CHECK(book.find(a)->base == a && book.find(a)->requested == 0);
    CHECK(book.give_back(a, limit) && book.find(a)->cached && book.cached_bytes == 1024);
    CHECK(!book.give_back(a, limit));                                  // a second free changes nothing
    CHECK(book.cached_bytes == 1024);
    void *a2 = alloc(book, 600, false);
    CHECK(a2 == a && book.cached_bytes == 0);
    CHECK(book.give_back(a2, limit));
    // the mode goes on with a plain block still cached: it is never handed out as a guarded one
    void *live_plain = alloc(book, 5000, false);                        // ... and one plain block still live
    void *g = alloc(book, 500, true);                                   // underlying 1024: the cached plain block would fit
    CHECK(g != a && book.find(g)->guarded && book.find(a)->cached);
    CHECK(book.find(g)->requested == 500 && book.find(g)->canary == 0xa5);
    CHECK(book.give_back(live_plain, limit));                           // freed under the mode: cached as what it is
    CHECK(!book.find(live_plain)->guarded);
    void *g5 = alloc(book, 5000, true);
    CHECK(g5 != live_plain && book.find(g5)->guarded);
    // a guarded block is reused guarded, with the new requested size and canary
    CHECK(book.give_back(g, limit) && book.find(g)->requested == 0);
    void *g2 = alloc(book, 300, true, 0xc3);
    CHECK(g2 == g && book.find(g2)->requested == 300 && book.find(g2)->canary == 0xc3);
    CHECK(book.find(g2)->back_begin() == PoolBook::kGuard + 300 && book.find(g2)->back_bytes() == 1024 - 256 - 300);
    // the mode goes off with a guarded block cached and one live: neither is handed out plain
    CHECK(book.give_back(g2, limit));
    void *p = alloc(book, 1000, false);                                 // the cached plain block of 1024, not the guarded one
    CHECK(p == a && !book.find(p)->guarded);
    void *p2 = alloc(book, 1000, false);                                // (the plain 8192: within the waste allowed below 1 MiB)
    CHECK(p2 == live_plain && !book.find(p2)->guarded && book.find(g2)->cached);
    CHECK(book.give_back(g5, limit) && book.find(g5)->guarded);
    // the switch releases the cache: live blocks stay, cached ones go back to the device once
    const size_t live_before = book.blocks.size();
    book.release_cached(fake_free);
    CHECK(book.cached_bytes == 0 && book.blocks.size() == 2 && live_before == 4);
    CHECK(book.find(p) != nullptr && book.find(p2) != nullptr && book.find(g2) == nullptr);
    // the cache limit: the caller frees the base and forgets the block
    CHECK(!book.give_back(p, 1000) && !book.find(p)->cached);
    fake_free(book.find(p)->base);
    book.forget(p);
    CHECK(book.find(p) == nullptr);
    CHECK(!book.give_back(p2, 8191) && book.give_back(p2, 8192));
    // a cached block that would waste more than half of itself plus 1 MiB is not taken
    void *big = alloc(book, (size_t)8 << 20, false);
    CHECK(book.give_back(big, limit));
    void *small = alloc(book, (size_t)2 << 20, false);
    CHECK(small != big);
    void *mid = alloc(book, (size_t)6 << 20, false);
    CHECK(mid == big);
    CHECK(book.give_back(small, limit) && book.give_back(mid, limit));
    book.release_cached(fake_free);
    CHECK(book.blocks.empty() && g_device.empty());
}

int main() {
    test_rounding();
    test_guard_layout();
    test_reuse_and_mode_switch();
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("pool_book ok\n");
    return 0;
}

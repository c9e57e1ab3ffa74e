// Bookkeeping of the per-context caching allocator (capi.hip: pool_alloc / pool_free), without a device call in it: which
// blocks exist, which are cached for reuse, and -- in the guarded mode, PADNE_POOL_GUARD -- where a block's guard zones lie.
// Host-only C++ so that a stand-alone program can drive it with a fake allocate / free pair (tests/native/pool_book_test.cpp).
//
// A PLAIN block is handed out at its base address.  A GUARDED block of `requested` bytes lies in an underlying allocation of
// round(requested + 2 * kGuard) bytes:
//     [base, base + kGuard)                      front zone
//     [base + kGuard, base + kGuard + requested) what the caller asked for (pointer handed out: base + kGuard)
//     [base + kGuard + requested, base + size)   back zone: starts at the first byte past the REQUESTED size and takes all the
//                                                slack of the rounding, at least kGuard bytes
// The two kinds are cached apart and never handed out as one another.
#pragma once

#include <stddef.h>

#include <map>
#include <unordered_map>

namespace padne {

struct PoolBook {
    static constexpr size_t kGuard = 256;       // bytes of the front zone; keeps the 256-byte alignment of hipMalloc

    struct Block {
        void *base = nullptr;       // what the device allocator returned
        size_t size = 0;            // bytes of the underlying allocation
        size_t requested = 0;       // guarded and handed out: bytes the caller asked for
        bool guarded = false;
        unsigned char canary = 0;   // guarded and handed out: the byte its zones were filled with
        bool cached = false;
        size_t front() const { return guarded ? kGuard : 0; }
        size_t back_begin() const { return front() + requested; }      // offsets from base
        size_t back_bytes() const { return size - back_begin(); }
    };

    std::unordered_map<void *, Block> blocks;               // every block, live or cached, by the pointer handed out
    std::multimap<size_t, void *> cache[2];                 // cached blocks by size: [0] plain, [1] guarded
    size_t cached_bytes = 0;

    // a power of two from 256 bytes to 1 MiB, MiB granules above
    static size_t round(size_t bytes) {
        if (bytes < 256) bytes = 256;
        if (bytes >= ((size_t)1 << 20)) return (bytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
        size_t p = 256;
        while (p < bytes) p <<= 1;
        return p;
    }
    static size_t underlying(size_t bytes, bool guarded) { return round(guarded ? bytes + 2 * kGuard : bytes); }

    // a cached block of the kind for `bytes`, or nullptr: the smallest that fits, unless it wastes more than half + 1 MiB
    void *take(size_t bytes, bool guarded, unsigned char canary) {
        const size_t want = underlying(bytes, guarded);
        auto &c = cache[guarded ? 1 : 0];
        auto it = c.lower_bound(want);
        if (it == c.end() || it->first > want + want / 2 + ((size_t)1 << 20)) return nullptr;
        void *p = it->second;
        cached_bytes -= it->first;
        c.erase(it);
        Block &b = blocks[p];
        b.cached = false;
        b.requested = guarded ? bytes : 0;
        b.canary = canary;
        return p;
    }

    // a fresh allocation of underlying(bytes, guarded) bytes at `base` becomes a live block; returns the pointer to hand out
    void *adopt(void *base, size_t bytes, bool guarded, unsigned char canary) {
        Block b;
        b.base = base;
        b.size = underlying(bytes, guarded);
        b.requested = guarded ? bytes : 0;
        b.guarded = guarded;
        b.canary = canary;
        void *p = (char *)base + b.front();
        blocks[p] = b;
        return p;
    }

    const Block *find(void *p) const {
        auto it = blocks.find(p);
        return it == blocks.end() ? nullptr : &it->second;
    }

    // a live block goes to the cache of its kind; false (and nothing changes) when the cache would pass `limit` bytes
    bool give_back(void *p, size_t limit) {
        auto it = blocks.find(p);
        if (it == blocks.end() || it->second.cached || cached_bytes + it->second.size > limit) return false;
        it->second.cached = true;
        it->second.requested = 0;
        cache[it->second.guarded ? 1 : 0].emplace(it->second.size, p);
        cached_bytes += it->second.size;
        return true;
    }

    // the caller has freed the block's base
    void forget(void *p) { blocks.erase(p); }

    template <typename Free> void release_cached(Free free_base) {
        for (auto &c : cache) {
            for (auto &kv : c) {
                auto it = blocks.find(kv.second);
                free_base(it->second.base);
                blocks.erase(it);
            }
            c.clear();
        }
        cached_bytes = 0;
    }
};

}  // namespace padne

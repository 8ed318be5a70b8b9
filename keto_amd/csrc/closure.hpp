// closure.hpp — the closure and the list finishes of the listing kernels, shared by lookup.hip
// (backward, over the reverse rows) and subjects.hip (forward, over the rows the check engine
// sees).  Next to paged_finish.hpp, and in its idiom: plain templates, the member filter a
// caller-supplied ok(u).
//
// Nothing here knows the direction.  A direction is data: `Rows` names the CSR to walk, and the
// member bound comes with it (ids below it can be members: num_expandable backwards, num_nodes
// forwards).
// Only interior entries (ids < Ni) have rows that can be reached, so only they go on a worklist.
//
//   tier 1  one wave per request.  The closure lives in an LDS open-addressing set (set_insert:
//           LDS compare-and-swap) that is visited set and result at once; the interior members
//           also go on an LDS worklist (each enters once, so it needs no more room than the
//           set).  Rows are read 64 entries per step.  tier1_closure reports a set that passed
//           kSetCap; tier1_finish writes the list.
//   tier 2  one workgroup of kT2Block per request.  A bitmap over the member bound and a
//           worklist of Ni entries in global memory; tier2_closure's level loop with
//           __syncthreads() runs the closure to its end whatever its size.  scan_count / scan_write
//           write the list from the bitmap and clear it; page_count_clear is the paged call's scan.
//   (wide.hpp holds a third way to run a closure, spread over the whole device, over tier 2's
//   bitmaps and with the same reservation.)
//
// Both list finishes end the same way (reserve): count the members, reserve exactly that many
// ids of `out` with one device-scope atomicAdd on a cursor, and write the list with plain
// vector stores if it fits below `capacity` (else begin = TRUNCATED; the count is exact either
// way).  The cursor ends at the sum of the counts, so a capacity of at least that sum
// truncates nothing.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ketogpu.h"
#include "paged_finish.hpp"

namespace ketogpu {
namespace closure {

constexpr uint32_t kSetCap = 1024;           // tier 1: nodes a set may hold (the stats' set_capacity)
constexpr uint32_t kSlotsLds = 2 * kSetCap;  // hash slots: a load of at most (kSetCap + 64) / kSlotsLds
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr unsigned kT2Block = 256;
static_assert(kT2Block == paged::kBlock, "the paged selection assumes tier 2's workgroup");
static_assert(kEmpty == paged::kEmpty, "the paged finish reads tier 1's set");

// a handle's device graph, as its kernels take it.  The closures read off, col and Ni, and take
// the member bound next to it (Nx or N: row entries >= bound are no members and are dropped
// before a set or a bitmap is touched); the rest is for the handle's own filter and classification.
struct Rows {
    const uint64_t *off;  // one more than there are rows
    const uint32_t *col;
    const uint32_t *filter_key;  // per node, what the member filter compares: object type or class
    uint32_t N, Nx, Ni;
    // null: row v ends at off[v + 1] (a dense CSR).  Else row v is col[off[v] .. end[v]): rows
    // that can grow lie in an arena with free words behind each (hip_host.hpp "arena")
    const uint64_t *end = nullptr;
};

// the entries of row v are col[b .. e).  The branch is on a kernel argument: uniform
__device__ __forceinline__ void row_bounds(const Rows &g, uint32_t v, uint64_t &b, uint64_t &e) {
    b = g.off[v];
    e = g.end ? g.end[v] : g.off[v + 1];
}

struct ListOut {
    uint32_t *out;
    unsigned long long capacity;
    unsigned long long *begin, *count;
    unsigned long long *cursor;  // ids reserved so far: ends at `needed`
    unsigned long long *truncated;
};

// one thread: reserve `cnt` ids for list i -> where to write it, or TRUNCATED
__device__ inline unsigned long long reserve(const ListOut &o, uint32_t i, unsigned long long cnt) {
    const unsigned long long base = atomicAdd(o.cursor, cnt);
    const bool fits = base + cnt <= o.capacity;
    o.count[i] = cnt;
    o.begin[i] = fits ? base : KETOGPU_LOOKUP_TRUNCATED;
    if (!fits) atomicAdd(o.truncated, 1ull);
    return fits ? base : KETOGPU_LOOKUP_TRUNCATED;
}

// ---------------------------------------------------------------------- tier 1
__device__ inline uint32_t slot_of(uint32_t u) { return (u * 0x9E3779B1u) >> 21; }  // 11 bits
static_assert(kSlotsLds == 1u << 11, "slot_of yields 11 bits");

// u (never kEmpty) into the LDS set -> fresh: this lane put it there, the first visit; `slot`:
// where u is.  At most kSetCap + 64 of the 2 x kSetCap slots are ever taken, so the probe ends
// at a free slot.
__device__ __forceinline__ bool set_insert(uint32_t *set, uint32_t u, uint32_t &slot) {
    bool fresh = false;
    slot = slot_of(u);
    for (;;) {
        const uint32_t old = atomicCAS(&set[slot], kEmpty, u);
        if (old == kEmpty) {
            fresh = true;
            break;
        }
        if (old == u) break;
        slot = (slot + 1) & (kSlotsLds - 1);
    }
    return fresh;
}

// tier 1's closure, by one wave: the closure of v's row into `set` (all kSlotsLds slots are
// initialised here), its interior members through `work`.  False when the set passed kSetCap:
// the request overflows.
__device__ __forceinline__ bool tier1_closure(const Rows &g, uint32_t bound, uint32_t v, uint32_t lane, uint32_t *set,
                                              uint32_t *work) {
    for (uint32_t s = lane; s < kSlotsLds; s += 64) set[s] = kEmpty;
    __syncthreads();
    uint32_t size = 0, head = 0, tail = 0;  // wave-uniform
    bool over = false;
    for (;;) {
        uint64_t b, e;
        row_bounds(g, v, b, e);
        for (uint64_t base = b; base < e && !over; base += 64) {
            const uint64_t j = base + lane;
            const uint32_t u = j < e ? g.col[j] : kEmpty;
            bool fresh = false;
            uint32_t slot;
            if (u < bound) fresh = set_insert(set, u, slot);  // (the bound also drops kEmpty)
            const unsigned long long mf = __ballot(fresh), mi = __ballot(fresh && u < g.Ni);
            if (fresh && u < g.Ni) work[tail + __popcll(mi & ((1ull << lane) - 1))] = u;
            tail += __popcll(mi);
            size += __popcll(mf);
            over = size > kSetCap;
        }
        __syncthreads();  // the worklist entries of this row are visible to every lane
        if (over || head == tail) break;
        v = work[head++];
    }
    return !over;
}

// tier 1's cursor finish, by the same wave: the members ok(u) of `set` to list i
template <class Ok>
__device__ __forceinline__ void tier1_finish(const uint32_t *set, uint32_t lane, uint32_t i, const ListOut &o, Ok ok) {
    uint32_t cnt = 0;
    for (uint32_t s = lane; s < kSlotsLds; s += 64) cnt += __popcll(__ballot(ok(set[s])));
    unsigned long long base = 0;
    if (lane == 0) base = reserve(o, i, cnt);
    base = __shfl(base, 0);
    if (base == KETOGPU_LOOKUP_TRUNCATED || !cnt) return;
    uint32_t w = 0;
    for (uint32_t s = lane; s < kSlotsLds; s += 64) {
        const uint32_t u = set[s];
        const bool m = ok(u);
        const unsigned long long mm = __ballot(m);
        if (m) o.out[base + w + __popcll(mm & ((1ull << lane) - 1))] = u;
        w += __popcll(mm);
    }
}

// ---------------------------------------------------------------------- tier 2
// tier 2's closure, by the whole workgroup: the closure of v's row into the slot's bitmap `bm`
// (all zero on entry), its interior members through the worklist `wl`.  *s_tail is an LDS
// counter, zero on entry and published by a barrier.  first(u, v) is called once per member, by
// the winner of the atomicOr: u's first visit, in the row of v.  stop() is read behind each
// level's barrier: true ends the search there.  Ends behind a barrier: every thread sees the
// whole bitmap and what the hooks wrote.
template <class First, class Stop>
__device__ __forceinline__ void tier2_closure(const Rows &g, uint32_t bound, uint32_t v0, uint32_t *bm, uint32_t *wl,
                                              unsigned int *s_tail, First first, Stop stop) {
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = kT2Block / 64;
    auto visit = [&](uint32_t u, uint32_t v) {
        if (u >= bound) return;
        const uint32_t bit = 1u << (u & 31);
        if (atomicOr(&bm[u >> 5], bit) & bit) return;
        first(u, v);
        if (u < g.Ni) wl[atomicAdd(s_tail, 1u)] = u;  // each interior node enters once: <= Ni entries
    };
    {  // the start's own row, by the whole workgroup
        uint64_t b, e;
        row_bounds(g, v0, b, e);
        for (uint64_t j = b + tid; j < e; j += kT2Block) visit(g.col[j], v0);
    }
    __syncthreads();
    uint32_t lb = 0, le = *s_tail;
    bool done = stop();
    while (lb < le && !done) {  // one level: a wave per row
        __syncthreads();        // everyone has read s_tail and the stop condition before they move
        for (uint32_t k = lb + wave; k < le; k += nwaves) {
            const uint32_t v = wl[k];
            uint64_t b, e;
            row_bounds(g, v, b, e);
            for (uint64_t j = b + lane; j < e; j += 64) visit(g.col[j], v);
        }
        __syncthreads();  // the level is complete
        lb = le;
        le = *s_tail;
        done = stop();
    }
}

// tier 2's finish by a scan of the bitmap, by the whole workgroup, in its two passes.
// scan_count: this thread's share of the members ok(u).  scan_write: the members to
// out[base ..) (base TRUNCATED: none) in the pass that clears the bitmap; *s_pos is an LDS
// counter, zero on entry.
template <class Ok>
__device__ __forceinline__ uint32_t scan_count(const uint32_t *bm, uint64_t bm_words, Ok ok) {
    uint32_t c = 0;
    for (uint64_t w = threadIdx.x; w < bm_words; w += kT2Block) {
        uint32_t bits = bm[w];
        while (bits) {
            const uint32_t u = (uint32_t)(w << 5) + (uint32_t)__ffs(bits) - 1;
            bits &= bits - 1;
            c += ok(u);
        }
    }
    return c;
}

template <class Ok>
__device__ __forceinline__ void scan_write(uint32_t *bm, uint64_t bm_words, unsigned long long base, uint32_t *out,
                                           Ok ok, unsigned int *s_pos) {
    for (uint64_t w = threadIdx.x; w < bm_words; w += kT2Block) {
        uint32_t bits = bm[w];
        if (!bits) continue;
        bm[w] = 0;
        if (base == KETOGPU_LOOKUP_TRUNCATED) continue;
        uint32_t ids[32], k = 0;
        while (bits) {
            const uint32_t u = (uint32_t)(w << 5) + (uint32_t)__ffs(bits) - 1;
            bits &= bits - 1;
            if (ok(u)) ids[k++] = u;
        }
        if (!k) continue;
        const uint32_t p = atomicAdd(s_pos, k);
        for (uint32_t x = 0; x < k; x++) out[base + p + x] = ids[x];
    }
}

// ... and what lies between the passes, for any tier-2 finish: every thread's count c summed in
// the LDS counter *s_cnt (zero on entry), one reservation -> base or TRUNCATED, for all threads
__device__ __forceinline__ unsigned long long reserve_block(const ListOut &o, uint32_t i, uint32_t c,
                                                            unsigned int *s_cnt, unsigned long long *s_base) {
    if (c) atomicAdd(s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) *s_base = reserve(o, i, *s_cnt);
    __syncthreads();
    return *s_base;
}

// the paged call's scan, behind the selection of paged_finish.hpp: this thread's share of the
// members ok(u) and of those >= lo, counted from the bitmap words it clears
struct PageCount {
    uint32_t count, remaining;
};

template <class Ok>
__device__ __forceinline__ PageCount page_count_clear(uint32_t *bm, uint64_t bm_words, uint32_t lo, Ok ok) {
    PageCount n{0, 0};
    for (uint64_t w = threadIdx.x; w < bm_words; w += kT2Block) {
        uint32_t bits = bm[w];
        if (!bits) continue;
        bm[w] = 0;
        while (bits) {
            const uint32_t u = (uint32_t)(w << 5) + (uint32_t)__ffs(bits) - 1;
            bits &= bits - 1;
            const bool m = ok(u);
            n.count += m;
            n.remaining += m && u >= lo;
        }
    }
    return n;
}

// ... and the page's report, by the whole workgroup: every thread's share (of the scan above or
// of a walk of its own) summed in the LDS counters *s_cnt and *s_rem, zero on entry
__device__ __forceinline__ void page_report(const paged::PageOut &o, uint32_t i, PageCount mine, unsigned int *s_cnt,
                                            unsigned int *s_rem) {
    if (mine.count) atomicAdd(s_cnt, mine.count);
    if (mine.remaining) atomicAdd(s_rem, mine.remaining);
    __syncthreads();
    if (threadIdx.x == 0) {
        o.count[i] = *s_cnt;
        o.remaining[i] = *s_rem;
        o.returned[i] = *s_rem < o.limit ? *s_rem : o.limit;
    }
}

}  // namespace closure
}  // namespace ketogpu

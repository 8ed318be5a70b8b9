// wide.hpp — the wide tier of the listing kernels: one closure spread over the whole device.
// Next to closure.hpp and in its idiom: plain templates over closure::Rows, a member bound and
// a caller-supplied ok(u); nothing here knows the direction.
//
// Tier 2 gives a request one workgroup, whatever the size of its closure, and a row one wave,
// whatever its length.  The wide tier is level-synchronous across the device instead, one launch
// per level, and its unit of work is not a row but a CHUNK of a row:
//
//   item    (slot, node v, chunk c): entries [c * kChunk, min((c + 1) * kChunk, len(v))) of v's
//           row, read by one wave.  A row of a million entries is about 500 items for about 500
//           waves.
//   queue   one append-only array of items for the whole round (`slots` requests).  An interior
//           node enters it once per slot, at its first visit, as ceil(len / kChunk) items
//           reserved on the queue's tail; the start's row is seeded once more.  So
//           slots x (Ni + 1 + 2 x ceil(col_words / kChunk)) items always suffice (queue_items).
//           A kernel that would write past the end sets the error word instead and writes nothing.
//   state   per slot a bitmap over the bound (tier 2's: every kernel leaves it all zero), a
//           member counter, a write cursor and the list's base.
//
//   seed    per slot, the items of the start's row.  The start itself is not marked: it is
//           listed only when a cycle leads back to it.
//   level   one launch over the items [lb, le) the launches before it appended; the host reads
//           the tail behind each.  A wave per item, grid-stride; lanes read the chunk
//           coalesced, a device-scope atomicOr on the slot's bitmap decides the first visit, the
//           first visits that pass ok(u) are counted by ballot (one atomicAdd per wave and item
//           on the slot's counter), the first visits below Ni reserve their items (one atomicAdd
//           per wave and step on the tail) and write them.
//   finish  reserve: one thread per slot reserves the slot's count (closure::reserve).  write: a
//           workgroup per tile of bitmap words of one slot extracts the members ok(u), takes its
//           place in the list (one LDS counter per workgroup, one atomicAdd per workgroup on the
//           slot's cursor), writes them with plain stores and stores every non-zero word back as
//           zero, also when the list is truncated or the call only counts.
//
// The depth and the paged calls (ketogpu_*_ids_depth_wide, ketogpu_*_page_wide) run the same
// rounds with two variations:
//
//   depth   level L is launch L (the seed's items are read by launch 1, so launch L yields the
//           members at distance L).  An item of a slot whose request has the limit k appends as
//           above while L < k; at L == k it appends nothing and counts its first visits that are
//           interior members into the request's frontier (one atomicAdd per wave and item): what
//           depth.hpp's tier 2 reads off its worklist.  The slot then has no items left; the
//           other slots of the round go on.  No item carries a level.
//   page    select: one workgroup per slot runs paged::page_select_block over the slot's bitmap,
//           reading only, and writes the page to the request's stride.  clear: a workgroup per
//           tile of kClearTile bitmap words of one slot stores every non-zero word back as zero
//           and counts the members ok(u) below the request's `from` (one LDS counter per
//           workgroup, one atomicAdd per workgroup on the slot's `below` word); it runs behind
//           the select, in a launch of its own.  final: one thread per slot: count is what the
//           levels counted, remaining = count - below, returned = min(limit, remaining).
//
// Within a launch, workgroups meet only in those atomics.  Everything else (the items, the tail
// the host reads, the counters the reservation reads, the bitmap the write kernel reads) crosses
// a kernel boundary.  There is no cooperative launch, no spinning on memory and no grid barrier:
// no workgroup ever waits for another.  The closure ends because each (slot, interior node)
// pair enters the queue once; there is no level cap.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "closure.hpp"
#include "depth.hpp"

#ifndef KETOGPU_WIDE_CHUNK
#define KETOGPU_WIDE_CHUNK 2048
#endif

namespace ketogpu {
namespace wide {

constexpr uint32_t kChunk = KETOGPU_WIDE_CHUNK;  // entries per work item (the stats' chunk)
static_assert(kChunk >= 64 && kChunk % 64 == 0, "a chunk is read in steps of one wave");
constexpr unsigned kBlock = 256;       // level and write kernels: four waves
constexpr unsigned kWriteWords = 8;    // write kernel: bitmap words per thread
constexpr unsigned kTile = kBlock * kWriteWords;  // ... and per workgroup
constexpr unsigned kLevelGridMax = 2048;          // level kernel: 8 workgroups per CU, grid-stride beyond
constexpr unsigned kClearWords = 4;    // clear kernel: bitmap words per thread
constexpr unsigned kClearTile = kBlock * kClearWords;  // ... and per workgroup: 32768 ids
static_assert(kBlock == paged::kBlock, "the paged selection assumes the wide tier's workgroup");
static_assert(kClearTile * 32u < KETOGPU_PAGE_LIMIT_MAX, "a page can span more than one clear tile");

struct Item {
    uint32_t slot, v, chunk;
};

// the head of the round's counters: ctr[kTail] items appended so far, ctr[kError] non-zero once a
// kernel found the queue too small; then three words per slot; behind them one more word per slot,
// the paged finish's `below`
constexpr uint32_t kTail = 0, kError = 1, kHead = 2, kPerSlot = 3;

struct State {
    uint32_t *bitmaps;  // nslots x bm_words, all zero between rounds
    uint64_t bm_words;
    Item *queue;
    unsigned long long qcap;  // items the queue has room for
    unsigned long long *ctr;  // kHead + kPerSlot x nslots words, all zero when a round begins
    uint32_t nslots;          // the requests of this round
    uint32_t rows;            // ids below it have a row: a start or an item at or above it is not read

    __device__ unsigned long long *count(uint32_t s) const { return ctr + kHead + kPerSlot * (uint64_t)s; }
    __device__ unsigned long long *cursor(uint32_t s) const { return count(s) + 1; }
    __device__ unsigned long long *base(uint32_t s) const { return count(s) + 2; }
    __device__ unsigned long long *below(uint32_t s) const { return ctr + kHead + kPerSlot * (uint64_t)nslots + s; }
};

// what a round of `slots` requests can append at most (see above)
inline uint64_t queue_items(uint64_t slots, uint64_t Ni, uint64_t col_words) {
    return slots * (Ni + 1 + 2 * ((col_words + kChunk - 1) / kChunk));
}
inline uint64_t ctr_words(uint64_t slots) { return kHead + kPerSlot * slots; }
inline uint64_t round_words(uint64_t slots) { return ctr_words(slots) + slots; }  // ... with the `below` words

__device__ __forceinline__ uint64_t chunks_of(uint64_t len) { return (len + kChunk - 1) / kChunk; }

// chunks first, first + step, ... < n of node v for slot s to queue[at ..): the caller has
// checked at + n against the queue's end
__device__ __forceinline__ void put_items(const State &w, unsigned long long at, uint32_t s, uint32_t v, uint64_t first,
                                          uint64_t n, uint64_t step) {
    for (uint64_t c = first; c < n; c += step) w.queue[at + c] = Item{s, v, (uint32_t)c};
}

// ---------------------------------------------------------------------- seed
// One wave per slot: request ovf_list[first + slot]'s start row as items.
static __global__ __launch_bounds__(64) void seed_kernel(closure::Rows g, const uint32_t *req, const uint32_t *ovf_list,
                                                         uint32_t first, State w) {
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    if (s >= w.nslots) return;
    const uint32_t v = req[ovf_list[first + s]];
    if (v >= w.rows) return;  // (tier 1 sends only starts that have a row)
    uint64_t b, e;
    closure::row_bounds(g, v, b, e);
    const uint64_t n = e > b ? chunks_of(e - b) : 0;
    if (!n) return;
    unsigned long long at = 0;
    if (lane == 0) at = atomicAdd(&w.ctr[kTail], (unsigned long long)n);
    at = __shfl(at, 0);
    if (at + n > w.qcap) {
        if (lane == 0) atomicOr(&w.ctr[kError], 1ull);
        return;
    }
    put_items(w, at, s, v, lane, n, 64);
}

// ---------------------------------------------------------------------- level
// A depth call's launch: its number L (1-based), the limits per request (null: none), which request
// a slot serves, and the frontier words per request (zero before the round's seed).
struct Cut {
    uint32_t L;
    const uint32_t *max_depth;
    const uint32_t *ovf_list;
    uint32_t first;
    unsigned long long *frontier;
};

// The body of a handle's level kernel: the items [lb, le), a wave each, grid-stride.  kCut: a
// depth call's (see above); member(u): what the frontier counts, the handle's filter at "any".
template <bool kCut, class Ok, class Member>
__device__ __forceinline__ void level_body(const closure::Rows &g, uint32_t bound, const State &w,
                                           unsigned long long lb, unsigned long long le, const Cut &cut, Ok ok,
                                           Member member) {
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const unsigned long long nwaves = (unsigned long long)gridDim.x * (kBlock / 64);
    if (le > w.qcap) le = w.qcap;
    for (unsigned long long k = lb + wave; k < le; k += nwaves) {
        const Item it = w.queue[k];
        if (it.slot >= w.nslots || it.v >= w.rows) continue;  // (wave-uniform)
        uint64_t b, e;
        closure::row_bounds(g, it.v, b, e);
        const uint64_t from = b + (uint64_t)it.chunk * kChunk;
        if (from >= e) continue;
        const uint64_t to = e - from > kChunk ? from + kChunk : e;
        uint32_t *bm = w.bitmaps + (uint64_t)it.slot * w.bm_words;
        uint32_t members = 0;  // wave-uniform
        uint32_t req = 0, front = 0;  // (depth calls) the slot's request and this item's share of its frontier
        bool last = false;            // ... whose limit this launch has reached: nothing is appended
        if (kCut) {
            req = cut.ovf_list[cut.first + it.slot];
            const uint32_t k = depth::limit_of(cut.max_depth, req);
            last = k != KETOGPU_DEPTH_ALL && cut.L >= k;
        }
        for (uint64_t at = from; at < to; at += 64) {
            const uint64_t j = at + lane;
            const uint32_t u = j < to ? g.col[j] : closure::kEmpty;
            bool fresh = false;
            if (u < bound) {  // (the bound also drops kEmpty)
                const uint32_t bit = 1u << (u & 31);
                fresh = !(atomicOr(&bm[u >> 5], bit) & bit);
            }
            members += __popcll(__ballot(fresh && ok(u)));
            if (kCut && last) {  // (wave-uniform) the interior members of the last level: the frontier
                front += __popcll(__ballot(fresh && u < g.Ni && member(u)));
                continue;
            }
            // the first visits below Ni: each one's items, reserved for the whole wave at once
            uint64_t mine = 0;
            if (fresh && u < g.Ni) {
                uint64_t ub, ue;
                closure::row_bounds(g, u, ub, ue);
                mine = ue > ub ? chunks_of(ue - ub) : 0;
            }
            if (!__ballot(mine != 0)) continue;
            uint64_t upto = mine;  // inclusive prefix sum over the lanes
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint64_t t = __shfl_up(upto, d);
                if (lane >= d) upto += t;
            }
            const uint64_t total = __shfl(upto, 63);
            unsigned long long q = 0;
            if (lane == 0) q = atomicAdd(&w.ctr[kTail], (unsigned long long)total);
            q = __shfl(q, 0);
            if (q + total > w.qcap) {
                if (lane == 0) atomicOr(&w.ctr[kError], 1ull);
                continue;
            }
            if (mine) put_items(w, q + (upto - mine), it.slot, u, 0, mine, 1);
        }
        if (lane == 0 && members) atomicAdd(w.count(it.slot), (unsigned long long)members);
        if (kCut && lane == 0 && front) atomicAdd(&cut.frontier[req], (unsigned long long)front);
    }
}

template <class Ok>
__device__ __forceinline__ void level(const closure::Rows &g, uint32_t bound, const State &w, unsigned long long lb,
                                      unsigned long long le, Ok ok) {
    level_body<false>(g, bound, w, lb, le, Cut{}, ok, [](uint32_t) { return false; });
}

template <class Ok, class Member>
__device__ __forceinline__ void level_depth(const closure::Rows &g, uint32_t bound, const State &w,
                                            unsigned long long lb, unsigned long long le, const Cut &cut, Ok ok,
                                            Member member) {
    level_body<true>(g, bound, w, lb, le, cut, ok, member);
}

inline unsigned level_grid(unsigned long long items) {
    const unsigned long long blocks = (items + kBlock / 64 - 1) / (kBlock / 64);
    return (unsigned)(blocks < kLevelGridMax ? (blocks ? blocks : 1) : kLevelGridMax);
}

// ---------------------------------------------------------------------- finish
// One thread per slot: the slot's count reserved for its request.
static __global__ __launch_bounds__(64) void reserve_kernel(const uint32_t *ovf_list, uint32_t first, State w,
                                                            closure::ListOut o) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= w.nslots) return;
    *w.base(s) = closure::reserve(o, ovf_list[first + s], *w.count(s));
}

// The body of a handle's write kernel: workgroup (x, y) serves tile x of slot y's bitmap.
// *s_cnt is an LDS counter, *s_at an LDS word.
template <class Ok>
__device__ __forceinline__ void write(const State &w, const closure::ListOut &o, unsigned int *s_cnt,
                                      unsigned long long *s_at, Ok ok) {
    const uint32_t s = blockIdx.y;
    if (s >= w.nslots) return;  // (uniform)
    uint32_t *bm = w.bitmaps + (uint64_t)s * w.bm_words;
    const unsigned long long base = *w.base(s);
    const bool listed = base != KETOGPU_LOOKUP_TRUNCATED;
    if (threadIdx.x == 0) *s_cnt = 0;
    __syncthreads();
    uint32_t bits[kWriteWords];
    uint32_t c = 0;
    const uint64_t w0 = (uint64_t)blockIdx.x * kTile + threadIdx.x;
    for (unsigned x = 0; x < kWriteWords; x++) {
        const uint64_t word = w0 + (uint64_t)x * kBlock;
        uint32_t b = word < w.bm_words ? bm[word] : 0;
        if (b) bm[word] = 0;
        uint32_t keep = 0;  // the members ok(u) of this word
        for (uint32_t r = listed ? b : 0; r; r &= r - 1) {
            const uint32_t k = (uint32_t)__ffs(r) - 1;
            if (ok((uint32_t)(word << 5) + k)) keep |= 1u << k;
        }
        bits[x] = keep;
        c += __popc(keep);
    }
    uint32_t mine = 0;
    if (c) mine = atomicAdd(s_cnt, c);
    __syncthreads();
    if (!*s_cnt) return;  // (uniform)
    if (threadIdx.x == 0) *s_at = atomicAdd(w.cursor(s), (unsigned long long)*s_cnt);
    __syncthreads();
    unsigned long long p = base + *s_at + mine;
    for (unsigned x = 0; x < kWriteWords; x++) {
        const uint64_t word = w0 + (uint64_t)x * kBlock;
        for (uint32_t r = bits[x]; r; r &= r - 1, p++)
            if (p < o.capacity) o.out[p] = (uint32_t)(word << 5) + (uint32_t)__ffs(r) - 1;
    }
}

// ---------------------------------------------------------------------- paged finish
// select: workgroup s serves slot s: the page of its request to the request's stride.  Reads the
// bitmap only.  s_wave: kBlock / 64 LDS words.
template <class Ok>
__device__ __forceinline__ void page_select(const State &w, const uint32_t *ovf_list, uint32_t first,
                                            const uint32_t *from, const paged::PageOut &o, uint32_t *s_wave, Ok ok) {
    const uint32_t s = blockIdx.x;
    if (s >= w.nslots) return;  // (uniform)
    const uint32_t i = ovf_list[first + s];
    paged::page_select_block(w.bitmaps + (uint64_t)s * w.bm_words, w.bm_words, from[i], o.limit,
                             o.out + (uint64_t)i * o.limit, s_wave, ok);
}

// clear: workgroup (x, y) serves tile x of slot y's bitmap: every non-zero word stored back as
// zero, the members ok(u) below the request's `from` counted into the slot's `below` word.  Words
// entirely below from >> 5 count whole, the word that holds `from` is masked below from & 31, the
// words above it are cleared only.  *s_cnt is an LDS counter.
template <class Ok>
__device__ __forceinline__ void page_clear(const State &w, const uint32_t *ovf_list, uint32_t first,
                                           const uint32_t *from, unsigned int *s_cnt, Ok ok) {
    const uint32_t s = blockIdx.y;
    if (s >= w.nslots) return;  // (uniform)
    uint32_t *bm = w.bitmaps + (uint64_t)s * w.bm_words;
    const uint32_t lo = from[ovf_list[first + s]];
    const uint64_t wlo = lo >> 5;
    if (threadIdx.x == 0) *s_cnt = 0;
    __syncthreads();
    uint32_t c = 0;
    const uint64_t w0 = (uint64_t)blockIdx.x * kClearTile + threadIdx.x;
    for (unsigned x = 0; x < kClearWords; x++) {
        const uint64_t word = w0 + (uint64_t)x * kBlock;
        uint32_t b = word < w.bm_words ? bm[word] : 0;
        if (b) bm[word] = 0;
        if (word > wlo) continue;
        if (word == wlo) b &= (1u << (lo & 31)) - 1;
        for (; b; b &= b - 1) c += ok((uint32_t)(word << 5) + (uint32_t)__ffs(b) - 1);
    }
    if (c) atomicAdd(s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0 && *s_cnt) atomicAdd(w.below(s), (unsigned long long)*s_cnt);
}

// final: one thread per slot reports its request's page
static __global__ __launch_bounds__(64) void page_final_kernel(const uint32_t *ovf_list, uint32_t first, State w,
                                                               paged::PageOut o) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= w.nslots) return;
    const uint32_t i = ovf_list[first + s];
    const unsigned long long count = *w.count(s), remaining = count - *w.below(s);
    o.count[i] = count;
    o.remaining[i] = remaining;
    o.returned[i] = remaining < o.limit ? (uint32_t)remaining : o.limit;
}

}  // namespace wide
}  // namespace ketogpu

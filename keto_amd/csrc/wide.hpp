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
// Within a launch, workgroups meet only in those atomics.  Everything else (the items, the tail
// the host reads, the counters the reservation reads, the bitmap the write kernel reads) crosses
// a kernel boundary.  There is no cooperative launch, no spinning on memory and no grid barrier:
// no workgroup ever waits for another.  The closure ends because each (slot, interior node)
// pair enters the queue once; there is no level cap.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "closure.hpp"

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

struct Item {
    uint32_t slot, v, chunk;
};

// the head of the round's counters: ctr[kTail] items appended so far, ctr[kError] non-zero once a
// kernel found the queue too small; then three words per slot
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
};

// what a round of `slots` requests can append at most (see above)
inline uint64_t queue_items(uint64_t slots, uint64_t Ni, uint64_t col_words) {
    return slots * (Ni + 1 + 2 * ((col_words + kChunk - 1) / kChunk));
}
inline uint64_t ctr_words(uint64_t slots) { return kHead + kPerSlot * slots; }

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
// The body of a handle's level kernel: the items [lb, le), a wave each, grid-stride.
template <class Ok>
__device__ __forceinline__ void level(const closure::Rows &g, uint32_t bound, const State &w, unsigned long long lb,
                                      unsigned long long le, Ok ok) {
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
        for (uint64_t at = from; at < to; at += 64) {
            const uint64_t j = at + lane;
            const uint32_t u = j < to ? g.col[j] : closure::kEmpty;
            bool fresh = false;
            if (u < bound) {  // (the bound also drops kEmpty)
                const uint32_t bit = 1u << (u & 31);
                fresh = !(atomicOr(&bm[u >> 5], bit) & bit);
            }
            members += __popcll(__ballot(fresh && ok(u)));
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
    }
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

}  // namespace wide
}  // namespace ketogpu

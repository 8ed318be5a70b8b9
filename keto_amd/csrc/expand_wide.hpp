// expand_wide.hpp — BuildTree with the copying spread over the chip (include/ketogpu.h
// ketogpu_subjects_expand_wide): the bodies of subjects.hip's wide expand kernels.  Next to
// expand_tree.hpp, whose walk this is, with one step added in front of it.
//
// The walk is ordered and stays with one wave per tree.  What it has to LOOK at is little: an
// entry of a row does more than emit a leaf only when it has a row of its own or its bit is set
// in the bad-row bitmap (expand_tree.hpp's step).  Everything between two such entries is a run
// of leaves, whose place in the output is known once the walk stands in front of it and whose
// content is a plain copy of the row.
//
//   mask    one bit per word of the handle's col allocation, arena slack included: bit j is set
//           iff col[j] is such an "attention" entry.  Built across the chip, a wave per 64 words:
//           a coalesced load, one ballot, one 64-bit store by lane 0.  Free arena words hold
//           anything, so every index is validated as in the walk.  The host rebuilds it in full
//           whenever rows, bounds or bad bits changed (subjects.hip need_expand_mask).
//   run     for the frame (v, off) with row [b, e), lane l reads mask word ((b + off) >> 6) + l
//           if that word holds bits of the row; the bits before b + off and from e on are
//           cleared.  z is the number of attention-free entries from `off` to the first set bit,
//           the end of the 64 words or the end of the row.  z >= 64, or z reaching the row's
//           end, is a RUN STEP: z leaves, with no set access and no HOST test.  Else the 64-entry
//           step of expand_tree.hpp runs as it is.  The mask does not change within a call, so
//           the counting and the writing walk take the same steps.
//   queue   the writing walk copies a run below kSelfCopy itself.  A longer one becomes
//           ceil(z / wide::kChunk) items (source index in col, destination index in the output,
//           length) behind one atomicAdd on the call's queue tail.  A reservation that would
//           pass the end appends nothing and the wave copies the run itself: slower, counted,
//           never an error.  A count-only call, a tree that is TRUNCATED and a HOST request
//           have no writing walk and so queue nothing.
//   fill    launched in-stream behind the walk kernel, reading the tail from device memory: a
//           wave per item, grid-stride, coalesced reads of col, plain stores of the ids and of
//           zero child counts, behind put()'s capacity guard.
//
// A request that opens more than kSetCap nodes overflows as in the plain call and runs
// expand_tree.hpp's tier 2 unchanged; it queues nothing.
#pragma once

#include "expand_tree.hpp"
#include "wide.hpp"

#ifndef KETOGPU_EXPAND_SELF_COPY
#define KETOGPU_EXPAND_SELF_COPY 1024
#endif

namespace ketogpu {
namespace expand {
namespace xwide {

constexpr unsigned kMaskBlock = 256;     // mask kernel: four waves, a mask word each
constexpr unsigned kMaskGridMax = 4096;  // ... grid-stride beyond
constexpr uint32_t kWindow = 64 * 64;    // entries one run step can pass: 64 mask words
// Runs below this are copied by the walking wave, longer ones go to the queue
// (-DKETOGPU_EXPAND_SELF_COPY for a build_variant).  Chosen on the MI355X among 64, 256, 1024 and
// never (DESIGN.md "Chip-wide BuildTree"): never queueing costs config #2's call 2.4 ms of 5.7;
// 64 and 256 cost the folder trees, whose runs are all shorter than 1024, 0.14 ms of 1.29 for
// items that save the walk nothing; 1024 costs config #2 0.1 to 0.2 ms against 256.
constexpr uint32_t kSelfCopy = KETOGPU_EXPAND_SELF_COPY;
constexpr unsigned kFillBlock = 256;   // fill kernel: four waves, an item each
constexpr unsigned kFillGrid = 1024;   // four workgroups per CU, grid-stride over the items
constexpr uint64_t kQueueDefault = 1u << 16;  // items: 1.5 MB (config #2's call appends 6 511)

struct Item {
    unsigned long long src, dst;  // the first entry in col, the first node in the output
    uint32_t len, pad;
};

// the call's counters, all zero when it begins
enum Ctr { kTail, kRunSteps, kSkipped, kRunsQueued, kItemsQueued, kRunsSelf, kRunsFull, kCtrWords };

struct Queue {
    Item *items;
    unsigned long long cap;
    unsigned long long *ctr;  // kCtrWords
};

// what one wave counted in its walks (uniform), added to the call's counters by lane 0
struct Counted {
    unsigned long long skipped = 0;
    uint32_t run_steps = 0, queued = 0, items = 0, self = 0, full = 0;
};

__device__ __forceinline__ void flush(const Queue &q, const Counted &c) {
    if (c.run_steps) atomicAdd(q.ctr + kRunSteps, (unsigned long long)c.run_steps);
    if (c.skipped) atomicAdd(q.ctr + kSkipped, c.skipped);
    if (c.queued) atomicAdd(q.ctr + kRunsQueued, (unsigned long long)c.queued);
    if (c.items) atomicAdd(q.ctr + kItemsQueued, (unsigned long long)c.items);
    if (c.self) atomicAdd(q.ctr + kRunsSelf, (unsigned long long)c.self);
    if (c.full) atomicAdd(q.ctr + kRunsFull, (unsigned long long)c.full);
}

// ---------------------------------------------------------------------- mask
// mask word w covers col[64 w .. 64 w + 64); words: how many there are
__device__ __forceinline__ void mask_build(const Graph &x, uint64_t col_words, unsigned long long *mask,
                                           uint64_t words) {
    const Rows &g = x.g;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (kMaskBlock / 64) + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (kMaskBlock / 64);
    for (uint64_t w = wave; w < words; w += nwaves) {
        const uint64_t j = w * 64 + lane;
        const uint32_t u = j < col_words ? g.col[j] : kEmpty;
        const bool attention = (u < g.Nx && row_len(g, u) > 0) || is_bad(x, u);
        const unsigned long long m = __ballot(attention);
        if (lane == 0) mask[w] = m;
    }
}

// The attention-free entries in front of col[p], within the row that ends at e (p < e), by one
// wave -> z <= kWindow, uniform
__device__ __forceinline__ uint32_t run_length(const unsigned long long *mask, uint64_t p, uint64_t e, uint32_t lane) {
    const uint64_t w = (p >> 6) + lane;
    unsigned long long m = w * 64 < e ? mask[w] : 0;
    if (lane == 0) m &= ~0ull << (p & 63);
    if (w * 64 < e && e - w * 64 < 64) m &= (1ull << (e - w * 64)) - 1;
    const unsigned long long any = __ballot(m != 0);
    const uint64_t window_end = ((p >> 6) + 64) * 64;
    uint64_t stop = e < window_end ? e : window_end;
    if (any) {
        const uint32_t f = (uint32_t)__ffsll((long long)any) - 1;
        const uint32_t bit = (uint32_t)__shfl(m ? __ffsll((long long)m) - 1 : 0, f);
        stop = ((p >> 6) + f) * 64 + bit;
    }
    return (uint32_t)(stop - p);
}

// the writing walk's run: col[p .. p + z) go out as leaves from node `at` on
__device__ __forceinline__ void run_write(const Graph &x, const TreeOut &o, const Queue &q, uint64_t p, uint32_t z,
                                          unsigned long long at, uint32_t lane, Counted &c) {
    bool self = z < kSelfCopy;
    if (!self) {
        const uint32_t items = (z + wide::kChunk - 1) / wide::kChunk;  // (at most kWindow / kChunk)
        unsigned long long t = 0;
        if (lane == 0) {
            // (a reservation that passes the end leaves the tail behind the end for good: every
            // later one fails too, and the words it took below the end become empty items)
            t = atomicAdd(q.ctr + kTail, (unsigned long long)items);
            if (t + items > q.cap) {
                for (; t < q.cap; t++) q.items[t] = Item{0, 0, 0, 0};
                t = ~0ull;
            }
        }
        t = __shfl(t, 0);
        if (t == ~0ull) {
            self = true, c.full++;
        } else {
            for (uint32_t k = lane; k < items; k += 64) {
                const uint32_t first = k * wide::kChunk;
                q.items[t + k] = Item{p + first, at + first, z - first < wide::kChunk ? z - first : wide::kChunk, 0};
            }
            c.queued++, c.items += items;
        }
    }
    if (self) {
        for (uint32_t k = lane; k < z; k += 64) put(o, at + k, x.g.col[p + k], 0);
        c.self++;
    }
}

// ---------------------------------------------------------------------- tier 1
// expand_tree.hpp's tier1_walk with the run step in front of its step
template <bool kWrite>
__device__ __forceinline__ Walk tier1_walk(const Graph &x, const unsigned long long *mask, const Queue &q, uint32_t r,
                                           uint32_t depth, uint32_t lane, T1Lds &s, const TreeOut &o,
                                           unsigned long long base, unsigned long long &total, Counted &c) {
    const Rows &g = x.g;
    for (uint32_t k = lane; k < kSlotsLds; k += 64) s.set[k] = kEmpty;
    __syncthreads();
    if (lane == 0) {
        uint32_t slot;
        set_insert(s.set, r, slot);
        s.v[0] = r, s.off[0] = 0;
        if (kWrite) put(o, base, r, row_len(g, r));
    }
    __syncthreads();
    uint32_t size = 1, sp = 1;   // wave-uniform: opened nodes, stack height
    unsigned long long pos = 1;  // ... and nodes emitted
    while (sp) {
        const uint32_t v = s.v[sp - 1], off = s.off[sp - 1];
        uint64_t b, e;
        row_bounds(g, v, b, e);
        const uint32_t len = (uint32_t)(e - b);
        if (off >= len) {
            sp--;
            continue;
        }
        const uint32_t z = run_length(mask, b + off, e, lane);
        if (z >= 64 || off + z == len) {  // a run step: z entries that are neither bad nor have a row
            if (kWrite) run_write(x, o, q, b + off, z, base + pos, lane, c);
            c.run_steps++, c.skipped += z;
            pos += z;
            if (lane == 0) s.off[sp - 1] = off + z;
            __syncthreads();
            continue;
        }
        const uint32_t cnt = len - off < 64 ? len - off : 64;
        const uint32_t u = lane < cnt ? g.col[b + off + lane] : kEmpty;
        const uint32_t ulen = u < g.Nx ? row_len(g, u) : 0;
        const bool has_row = ulen > 0, bad = is_bad(x, u);
        if (depth - sp == 1) {  // the children's rest depth: all leaves, marked all the same
            bool fresh = false;
            uint32_t slot;
            if (has_row) fresh = set_insert(s.set, u, slot);
            if (__ballot(bad && (!has_row || fresh))) return kHost;
            size += __popcll(__ballot(fresh));
            if (size > kSetCap) return kOver;
            if (kWrite && lane < cnt) put(o, base + pos + lane, u, 0);
            pos += cnt;
            if (lane == 0) s.off[sp - 1] = off + cnt;
        } else {
            const unsigned long long fresh = __ballot(has_row && !set_has(s.set, u));
            const uint32_t k = fresh ? (uint32_t)__ffsll((long long)fresh) - 1 : 64;  // the recursion point
            const uint32_t leaves = k < cnt ? k : cnt;
            if (__ballot(bad && ((lane < leaves && !has_row) || lane == k))) return kHost;
            if (kWrite && lane < leaves) put(o, base + pos + lane, u, 0);
            if (k < 64) {
                if (size == kSetCap) return kOver;
                size++;
                if (lane == k) {
                    uint32_t slot;
                    set_insert(s.set, u, slot);
                    if (kWrite) put(o, base + pos + k, u, ulen);
                    s.off[sp - 1] = off + k + 1;
                    s.v[sp] = u, s.off[sp] = 0;  // (sp < size <= kSetCap)
                }
                pos += k + 1;
                sp++;
            } else {
                pos += cnt;
                if (lane == 0) s.off[sp - 1] = off + cnt;
            }
        }
        __syncthreads();  // the set and the stack as this step left them
    }
    total = pos;
    return kDone;
}

// expand_tree.hpp's tier1_tree over the walk above
__device__ __forceinline__ void tier1_tree(const Graph &x, const unsigned long long *mask, const Queue &q,
                                           const uint32_t *roots, const uint32_t *depths, uint32_t i, uint32_t lane,
                                           int force_tier2, const TreeOut &o, uint32_t *ovf_list,
                                           unsigned int *ovf_count, T1Lds &s) {
    const uint32_t r = roots[i], depth = depths[i];
    if (root_answered(x, r, depth, i, lane == 0, o)) return;
    unsigned long long total = 0;
    Counted c;
    const Walk w = force_tier2 ? kOver : tier1_walk<false>(x, mask, q, r, depth, lane, s, o, 0, total, c);
    if (w == kOver) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i, flush(q, c);
        return;
    }
    if (w == kHost) {
        if (lane == 0) no_tree(o, i, 0, KETOGPU_EXPAND_HOST), flush(q, c);
        return;
    }
    unsigned long long base = 0;
    if (lane == 0) {
        base = reserve(o.l, i, total);
        o.status[i] = KETOGPU_EXPAND_OK;
    }
    base = __shfl(base, 0);
    if (base != KETOGPU_LOOKUP_TRUNCATED) tier1_walk<true>(x, mask, q, r, depth, lane, s, o, base, total, c);
    if (lane == 0) flush(q, c);
}

// ---------------------------------------------------------------------- fill
// the queue's items, a wave each: the tail is what the walk kernel in front left behind
__device__ __forceinline__ void fill(const Graph &x, const Queue &q, const TreeOut &o) {
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long tail = q.ctr[kTail] < q.cap ? q.ctr[kTail] : q.cap;
    const unsigned long long nwaves = (unsigned long long)gridDim.x * (kFillBlock / 64);
    for (unsigned long long k = (unsigned long long)blockIdx.x * (kFillBlock / 64) + (threadIdx.x >> 6); k < tail;
         k += nwaves) {
        const Item it = q.items[k];
        for (uint32_t j = lane; j < it.len; j += 64) put(o, it.dst + j, x.g.col[it.src + j], 0);
    }
}

}  // namespace xwide
}  // namespace expand
}  // namespace ketogpu

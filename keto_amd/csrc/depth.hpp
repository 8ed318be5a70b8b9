// depth.hpp — depth-limited listings (include/ketogpu.h ketogpu_*_depth): the members of a
// closure within max_depth hops of its start, shared by lookup.hip and subjects.hip.  Next to
// closure.hpp and combine.hpp, and in their idiom: plain templates, the direction as data.
//
// Both closures of closure.hpp visit in level order (DESIGN.md "Explain"): level 1 is the start's
// own row, level d + 1 what the rows of the interior members of level d add for the first time.
// A depth limit therefore needs no per-member distance, only where a level ends:
//
//   tier 1  tier1_closure's set, worklist and 64 entries per step, plus wave-uniform scalars:
//           the level of the row at hand, and where that level ends on the worklist.  The
//           search stops before a row of level max_depth is read; what then remains on the
//           worklist is that level's interior entries, the frontier.  Only entries within the
//           limit ever enter the set, so a request overflows exactly when they pass kSetCap.
//   tier 2  tier2_closure as it is, with LevelStop as its stop(): it counts its own calls (one
//           behind each level's barrier, by every thread) and reads the frontier off the
//           worklist tail: the tail now minus the tail at the previous call.
//
// The frontier counts MEMBERS: a writable snapshot pads its rows with placeholder nodes, which
// are interior ids with empty rows and belong to no list.  So where a search stops, the
// worklist entries of the last level are counted under a caller-supplied member(u) (the
// handle's filter at "any"), once, over the frontier alone.
//
// KETOGPU_DEPTH_ALL (0) is no limit: no level ever compares equal to it.  There is no finish
// here; the finishes of closure.hpp and paged_finish.hpp follow unchanged.
#pragma once

#include "closure.hpp"

namespace ketogpu {
namespace depth {

using namespace closure;

// request i's limit: a null array is no limit for every request
__device__ inline uint32_t limit_of(const uint32_t *max_depth, uint32_t i) {
    return max_depth ? max_depth[i] : KETOGPU_DEPTH_ALL;
}

// tier1_closure with a depth limit, by one wave: the entries within max_depth hops of v into
// `set` (all kSlotsLds slots are initialised here).  `frontier`: the interior members at
// exactly max_depth hops, whose rows were left unread (0 without a limit, or when the closure
// ended within it).  False when the set passed kSetCap: the request overflows.
template <class Member>
__device__ __forceinline__ bool tier1_closure(const Rows &g, uint32_t bound, uint32_t v, uint32_t max_depth,
                                              uint32_t lane, uint32_t *set, uint32_t *work, uint32_t &frontier,
                                              Member member) {
    for (uint32_t s = lane; s < kSlotsLds; s += 64) set[s] = kEmpty;
    __syncthreads();
    uint32_t size = 0, head = 0, tail = 0;  // wave-uniform
    uint32_t level = 0, level_end = 0;      // the row at hand is of `level` (the start: 0), which ends at work[level_end)
    bool over = false;
    frontier = 0;
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
        if (over) break;
        if (head == level_end) {  // the last row of `level` is read: work[head, tail) is the next level
            level++;
            level_end = tail;
            if (head == tail) break;
            if (level == max_depth) {  // work[head, tail) stays unread
                for (uint32_t k0 = head; k0 < tail; k0 += 64) {
                    const uint32_t k = k0 + lane;
                    frontier += __popcll(__ballot(k < tail && member(work[k])));
                }
                break;
            }
        }
        v = work[head++];
    }
    return !over;
}

// tier2_closure's stop() under a depth limit.  Call c comes behind the barrier that completes
// level c, from every thread equally often, so the answer is uniform: true at call max_depth.
// The worklist entries between the previous call's tail and this one's are level c's interior
// entries: at the stop, wl[prev - frontier, prev) is the frontier.
struct LevelStop {
    const unsigned int *s_tail;
    uint32_t max_depth;
    uint32_t calls = 0, prev = 0, frontier = 0;  // (uniform: every thread reads the same tails)
    __device__ LevelStop(const unsigned int *tail, uint32_t k) : s_tail(tail), max_depth(k) {}
    __device__ bool operator()() {
        const uint32_t tail = *s_tail;
        const bool cut = ++calls == max_depth;
        if (cut) frontier = tail - prev;
        prev = tail;
        return cut;
    }
};

// tier2_closure takes its hooks by value: this passes the caller's LevelStop by reference, so
// the frontier it found can be read afterwards
struct LevelStopRef {
    LevelStop *s;
    __device__ bool operator()() const { return (*s)(); }
};

// the frontier of a tier-2 search that LevelStop ended, by the whole workgroup, behind
// tier2_closure's last barrier: the members among the last level's worklist entries to *out
// (left alone when there are none).  *s_fr is an LDS counter, zero on entry.
template <class Member>
__device__ __forceinline__ void tier2_frontier(const LevelStop &stop, const uint32_t *wl, unsigned long long *out,
                                               unsigned int *s_fr, Member member) {
    if (!stop.frontier) return;  // (uniform)
    uint32_t c = 0;
    for (uint32_t k = stop.prev - stop.frontier + threadIdx.x; k < stop.prev; k += kT2Block) c += member(wl[k]);
    if (c) atomicAdd(s_fr, c);
    __syncthreads();
    if (threadIdx.x == 0 && *s_fr) *out = *s_fr;
}

}  // namespace depth
}  // namespace ketogpu

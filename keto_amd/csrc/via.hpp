// via.hpp — listings that say why (include/ketogpu.h ketogpu_*_via): next to every member of a
// depth-limited listing, the node whose row granted it (`via`) and its distance from the start
// (`hops`), shared by lookup.hip and subjects.hip.  Next to depth.hpp and combine.hpp, and in
// their idiom: plain templates, the direction as data (the rows, the member bound, and `rows`:
// ids below it have a row to start from, N backwards and Nx forwards).
//
// Both closures of closure.hpp visit in level order, so the row a member is first seen in
// belongs to a node one hop nearer the start: the first visit's row is a breadth-first parent,
// and the level at hand plus one is the exact distance.  What the plain and the depth kernels
// pass once and throw away is kept here, per member:
//
//   tier 1  depth::tier1_closure's loop (the set, the worklist, 64 entries per step, wave-uniform
//           level / level_end) with two 16-bit words per set slot, written by the lane that wins
//           set_insert: the parent as the slot of the row's node, or kParStart for the start's
//           own row, and the hop, level + 1 (at most kSetCap + 64 members: 16 bits suffice).  The
//           worklist holds slots, as in the path kernel, so the row at hand knows its own.  The
//           start as a parent (the marker) is not the start as a member (a slot of its own,
//           reached through a cycle, with its predecessor as parent).
//           LDS: set 8192 + parents 4096 + hops 4096 + worklist 2176 = 18560 bytes for a list
//           kernel; a page kernel keeps a copy of the set to probe after the ordered finish has
//           sorted the original away: 26752 bytes.
//   tier 2  tier2_closure as it is.  first(u, v) stores v and the level as one pair of words in
//           an array of `bound` pairs per slot, indexed by u (one 8-byte store per first visit,
//           one 8-byte gather per written id); the level is depth::LevelStop's call count,
//           uniform within a level.  Hops are 32 bits here: a chain of thousands must pass.  A
//           pair is valid exactly where the bitmap bit is set (written by the winner of the
//           atomicOr), so the array is never cleared: 8 bytes x bound per slot on top of the
//           bitmap and the worklist.  The finishes are scan_write's and the seen list's with the
//           two parallel stores; a page gathers the words of the returned ids behind the
//           selection (the bitmap is clear by then; the words stay).
//
// via[k] and hops[k] belong to out[k]; either array may be null and is then not written.
#pragma once

#include "depth.hpp"

namespace ketogpu {
namespace via {

using namespace closure;

constexpr uint16_t kParStart = 0xFFFFu;  // tier 1's parent word: seen in the start's own row
static_assert(kSlotsLds <= kParStart, "a slot index fits a parent word");
static_assert(kSetCap + 64 < 0xFFFFu, "a hop count of tier 1 fits 16 bits");

// the arrays parallel to ListOut::out / PageOut::out (null: not wanted)
struct ViaOut {
    uint32_t *via, *hops;
};

struct T1Lds {
    uint32_t set[kSlotsLds];
    uint16_t par[kSlotsLds], hop[kSlotsLds];
    uint16_t work[kSetCap + 64];
};

// a start that is answered before any row is read (ids below `rows` have one): true for an id
// outside the snapshot, which is INVALID; NONE and a start without a row give the empty answer
__device__ inline bool outside(const Rows &g, uint32_t x) { return x >= g.N && x != KETOGPU_NODE_NONE; }

// ---------------------------------------------------------------------- tier 1
// depth::tier1_closure with a parent and a hop word per slot, by one wave.  False when the set
// passed kSetCap: the request overflows.
template <class Member>
__device__ __forceinline__ bool tier1_closure(const Rows &g, uint32_t bound, uint32_t v, uint32_t max_depth,
                                              uint32_t lane, T1Lds &s, uint32_t &frontier, Member member) {
    for (uint32_t k = lane; k < kSlotsLds; k += 64) s.set[k] = kEmpty;
    __syncthreads();
    uint32_t size = 0, head = 0, tail = 0;  // wave-uniform
    uint32_t level = 0, level_end = 0;      // the row at hand is of `level` (the start: 0), ending at work[level_end)
    uint32_t pv = kParStart;                // the slot of the row's node
    bool over = false;
    frontier = 0;
    for (;;) {
        uint64_t b, e;
        row_bounds(g, v, b, e);
        for (uint64_t base = b; base < e && !over; base += 64) {
            const uint64_t j = base + lane;
            const uint32_t u = j < e ? g.col[j] : kEmpty;
            bool fresh = false;
            uint32_t slot = 0;
            if (u < bound) fresh = set_insert(s.set, u, slot);  // (the bound also drops kEmpty)
            if (fresh) s.par[slot] = (uint16_t)pv, s.hop[slot] = (uint16_t)(level + 1);  // the first visit
            const unsigned long long mf = __ballot(fresh), mi = __ballot(fresh && u < g.Ni);
            if (fresh && u < g.Ni) s.work[tail + __popcll(mi & ((1ull << lane) - 1))] = (uint16_t)slot;
            tail += __popcll(mi);
            size += __popcll(mf);
            over = size > kSetCap;
        }
        __syncthreads();  // the worklist entries and the words of this row are visible to every lane
        if (over) break;
        if (head == level_end) {  // the last row of `level` is read: work[head, tail) is the next level
            level++;
            level_end = tail;
            if (head == tail) break;
            if (level == max_depth) {  // work[head, tail) stays unread
                for (uint32_t k0 = head; k0 < tail; k0 += 64) {
                    const uint32_t k = k0 + lane;
                    frontier += __popcll(__ballot(k < tail && member(s.set[s.work[k]])));
                }
                break;
            }
        }
        pv = s.work[head++];
        v = s.set[pv];
    }
    return !over;
}

// the start of request i, classified; the closure; the overflow list -> true when the set holds
// the answer.  frontier[i] is all zero on entry.
template <class Member>
__device__ __forceinline__ bool tier1_search(const Rows &g, uint32_t bound, uint32_t x, uint32_t max_depth,
                                             uint32_t i, uint32_t lane, int force_tier2, T1Lds &s,
                                             unsigned long long *frontier, uint32_t *ovf_list,
                                             unsigned int *ovf_count, Member member) {
    uint32_t fr = 0;
    if (force_tier2 || !tier1_closure(g, bound, x, max_depth, lane, s, fr, member)) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return false;
    }
    if (lane == 0 && fr) frontier[i] = fr;
    return true;
}

// tier1_finish with the two parallel stores: the members ok(u) of the set to list i
template <class Ok>
__device__ __forceinline__ void tier1_finish(const T1Lds &s, uint32_t start, uint32_t lane, uint32_t i,
                                             const ListOut &o, const ViaOut &vo, Ok ok) {
    uint32_t cnt = 0;
    for (uint32_t k = lane; k < kSlotsLds; k += 64) cnt += __popcll(__ballot(ok(s.set[k])));
    unsigned long long base = 0;
    if (lane == 0) base = reserve(o, i, cnt);
    base = __shfl(base, 0);
    if (base == KETOGPU_LOOKUP_TRUNCATED || !cnt) return;
    uint32_t w = 0;
    for (uint32_t k = lane; k < kSlotsLds; k += 64) {
        const uint32_t u = s.set[k];
        const bool m = ok(u);
        const unsigned long long mm = __ballot(m);
        if (m) {
            const unsigned long long at = base + w + __popcll(mm & ((1ull << lane) - 1));
            const uint32_t p = s.par[k];
            o.out[at] = u;
            if (vo.via) vo.via[at] = p == kParStart ? start : s.set[p];
            if (vo.hops) vo.hops[at] = s.hop[k];
        }
        w += __popcll(mm);
    }
}

// the body of a tier-1 list kernel, by one wave
template <class Ok, class Member>
__device__ __forceinline__ void tier1_list(const Rows &g, uint32_t bound, uint32_t rows, const uint32_t *starts,
                                           const uint32_t *max_depth, uint32_t i, uint32_t lane, int force_tier2,
                                           const ListOut &o, const ViaOut &vo, unsigned long long *frontier,
                                           uint32_t *ovf_list, unsigned int *ovf_count, T1Lds &s, Ok ok,
                                           Member member) {
    const uint32_t x = starts[i];
    if (x >= rows) {
        if (lane == 0) {
            o.begin[i] = outside(g, x) ? KETOGPU_LOOKUP_INVALID : 0ull;
            o.count[i] = 0;
        }
        return;
    }
    if (!tier1_search(g, bound, x, depth::limit_of(max_depth, i), i, lane, force_tier2, s, frontier, ovf_list,
                      ovf_count, member))
        return;
    tier1_finish(s, x, lane, i, o, vo, ok);
}

// the body of a tier-1 page kernel, by one wave.  `keys`: kSlotsLds words, the copy of the set
// that outlives the ordered finish; each returned id is probed in it for its slot.
template <class Ok, class Member>
__device__ __forceinline__ void tier1_page(const Rows &g, uint32_t bound, uint32_t rows, const uint32_t *starts,
                                           const uint32_t *max_depth, const uint32_t *from, uint32_t i,
                                           uint32_t lane, int force_tier2, const paged::PageOut &o, const ViaOut &vo,
                                           unsigned long long *frontier, uint32_t *ovf_list,
                                           unsigned int *ovf_count, T1Lds &s, uint32_t *keys, Ok ok, Member member) {
    const uint32_t x = starts[i];
    if (x >= rows) {
        if (lane == 0) paged::page_invalid(o, i, outside(g, x));
        return;
    }
    if (!tier1_search(g, bound, x, depth::limit_of(max_depth, i), i, lane, force_tier2, s, frontier, ovf_list,
                      ovf_count, member))
        return;
    for (uint32_t k = lane; k < kSlotsLds; k += 64) keys[k] = s.set[k];
    __syncthreads();
    paged::page_finish_wave(s.set, kSlotsLds, lane, i, from[i], o, ok);
    __syncthreads();  // lane 0's `returned` and every lane's ids are visible to the wave
    const uint32_t ret = o.returned[i];
    const uint64_t row = (uint64_t)i * o.limit;
    for (uint32_t k = lane; k < ret; k += 64) {
        const uint32_t u = o.out[row + k];  // a member: the probe ends at its slot
        uint32_t slot = slot_of(u);
        while (keys[slot] != u) slot = (slot + 1) & (kSlotsLds - 1);
        const uint32_t p = s.par[slot];
        if (vo.via) vo.via[row + k] = p == kParStart ? x : keys[p];
        if (vo.hops) vo.hops[row + k] = s.hop[slot];
    }
}

// ---------------------------------------------------------------------- tier 2
struct T2Lds {
    unsigned int tail, seen, cnt, pos, rem, fr;
    unsigned long long base;
    uint32_t wave[kT2Block / 64];
};

// one slot's state.  why: `bound` pairs (x: the parent, y: the hop count).  The seen list and the finish counters are
// the subjects handle's (kSeen); the lookup handle leaves them null.
struct Slot {
    uint32_t *bm;
    uint64_t bm_words;
    uint32_t *wl;
    uint2 *why;
    uint32_t *seen;
    uint32_t list_cap;
    unsigned long long *list_finishes, *scan_finishes;
};

__device__ __forceinline__ void tier2_begin(T2Lds &s) {
    if (threadIdx.x == 0) s.tail = 0, s.seen = 0, s.cnt = 0, s.pos = 0, s.rem = 0, s.fr = 0;
    __syncthreads();
}

// tier2_closure under a depth limit with the parent and the level of every first visit kept,
// and the frontier of the search to *frontier.  kSeen: the first visits are also counted and,
// while there is room, appended to the seen list.
template <bool kSeen, class Member>
__device__ __forceinline__ void tier2_search(const Rows &g, uint32_t bound, uint32_t x, uint32_t max_depth,
                                             const Slot &sl, T2Lds &s, unsigned long long *frontier, Member member) {
    depth::LevelStop stop(&s.tail, max_depth);
    tier2_closure(
        g, bound, x, sl.bm, sl.wl, &s.tail,
        [&](uint32_t u, uint32_t v) {
            sl.why[u] = make_uint2(v, stop.calls + 1);  // stop() was called once behind every completed level
            if (kSeen) {
                const uint32_t k = atomicAdd(&s.seen, 1u);
                if (k < sl.list_cap) sl.seen[k] = u;
            }
        },
        depth::LevelStopRef{&stop});
    depth::tier2_frontier(stop, sl.wl, frontier, &s.fr, member);
}

// scan_write with the two parallel stores, in the pass that clears the bitmap
template <class Ok>
__device__ __forceinline__ void scan_write(const Slot &sl, unsigned long long base, uint32_t *out, const ViaOut &vo,
                                           Ok ok, unsigned int *s_pos) {
    for (uint64_t w = threadIdx.x; w < sl.bm_words; w += kT2Block) {
        uint32_t bits = sl.bm[w];
        if (!bits) continue;
        sl.bm[w] = 0;
        if (base == KETOGPU_LOOKUP_TRUNCATED) continue;
        uint32_t ids[32], k = 0;
        while (bits) {
            const uint32_t u = (uint32_t)(w << 5) + (uint32_t)__ffs(bits) - 1;
            bits &= bits - 1;
            if (ok(u)) ids[k++] = u;
        }
        if (!k) continue;
        const unsigned long long at = base + atomicAdd(s_pos, k);
        for (uint32_t x = 0; x < k; x++) {
            out[at + x] = ids[x];
            if (!vo.via && !vo.hops) continue;
            const uint2 w = sl.why[ids[x]];
            if (vo.via) vo.via[at + x] = w.x;
            if (vo.hops) vo.hops[at + x] = w.y;
        }
    }
}

// the body of a tier-2 list kernel, by the whole workgroup; the bitmap is all zero on entry and
// is cleared again on the way out, by either finish
template <bool kSeen, class Ok, class Member>
__device__ __forceinline__ void tier2_list(const Rows &g, uint32_t bound, uint32_t rows, uint32_t x,
                                           uint32_t max_depth, uint32_t i, const ListOut &o, const ViaOut &vo,
                                           unsigned long long *frontier, const Slot &sl, T2Lds &s, Ok ok,
                                           Member member) {
    const unsigned tid = threadIdx.x, lane = tid & 63;
    tier2_begin(s);
    if (x >= rows) return;  // (tier 1 lists starts with a row only)
    tier2_search<kSeen>(g, bound, x, max_depth, sl, s, frontier + i, member);
    const uint32_t total = s.seen;
    const bool by_list = kSeen && sl.list_cap && total <= sl.list_cap;  // the seen list holds every member
    uint32_t c = 0;
    if (by_list) {
        for (uint32_t k = tid; k < total; k += kT2Block) {
            const uint32_t u = sl.seen[k];
            c += ok(u);
            sl.bm[u >> 5] = 0;  // every set bit of the word is some member's: all of them store the same zero
        }
    } else {
        c = scan_count(sl.bm, sl.bm_words, ok);
    }
    const unsigned long long base = reserve_block(o, i, c, &s.cnt, &s.base);
    if (kSeen && tid == 0) atomicAdd(by_list ? sl.list_finishes : sl.scan_finishes, 1ull);
    if (!by_list) {
        scan_write(sl, base, o.out, vo, ok, &s.pos);
        return;
    }
    if (base == KETOGPU_LOOKUP_TRUNCATED) return;
    for (uint32_t k0 = 0; k0 < total; k0 += kT2Block) {  // (a uniform trip count: the ballot sees whole waves)
        const uint32_t k = k0 + tid;
        const uint32_t u = k < total ? sl.seen[k] : kEmpty;
        const bool m = ok(u);
        const unsigned long long mm = __ballot(m);
        uint32_t p = 0;
        if (lane == 0 && mm) p = atomicAdd(&s.pos, (unsigned)__popcll(mm));
        p = __shfl(p, 0);
        if (m) {
            const unsigned long long at = base + p + __popcll(mm & ((1ull << lane) - 1));
            o.out[at] = u;
            if (vo.via || vo.hops) {
                const uint2 w = sl.why[u];
                if (vo.via) vo.via[at] = w.x;
                if (vo.hops) vo.hops[at] = w.y;
            }
        }
    }
}

// the body of a tier-2 page kernel: selection in id order, the count that clears the bitmap,
// then the words of the returned ids
template <bool kSeen, class Ok, class Member>
__device__ __forceinline__ void tier2_page(const Rows &g, uint32_t bound, uint32_t rows, uint32_t x,
                                           uint32_t max_depth, uint32_t lo, uint32_t i, const paged::PageOut &o,
                                           const ViaOut &vo, unsigned long long *frontier, const Slot &sl, T2Lds &s,
                                           Ok ok, Member member) {
    const unsigned tid = threadIdx.x;
    tier2_begin(s);
    if (x >= rows) return;  // (tier 1 lists starts with a row only)
    tier2_search<kSeen>(g, bound, x, max_depth, sl, s, frontier + i, member);
    const uint32_t total = s.seen;
    const bool by_list = kSeen && sl.list_cap && total <= sl.list_cap;
    const uint64_t row = (uint64_t)i * o.limit;
    paged::page_select_block(sl.bm, sl.bm_words, lo, o.limit, o.out + row, s.wave, ok);
    __syncthreads();  // the selection has read the bitmap, and its ids are visible to the workgroup
    PageCount mine{0, 0};
    if (by_list) {
        for (uint32_t k = tid; k < total; k += kT2Block) {
            const uint32_t u = sl.seen[k];
            const bool m = ok(u);
            mine.count += m;
            mine.remaining += m && u >= lo;
            sl.bm[u >> 5] = 0;  // every set bit of the word is some member's: all of them store the same zero
        }
    } else {
        mine = page_count_clear(sl.bm, sl.bm_words, lo, ok);
    }
    page_report(o, i, mine, &s.cnt, &s.rem);  // (behind its barrier s.rem is final)
    if (kSeen && tid == 0) atomicAdd(by_list ? sl.list_finishes : sl.scan_finishes, 1ull);
    const uint32_t ret = s.rem < o.limit ? s.rem : o.limit;
    if (!vo.via && !vo.hops) return;  // (uniform)
    for (uint32_t k = tid; k < ret; k += kT2Block) {
        const uint2 w = sl.why[o.out[row + k]];  // a member: below the bound
        if (vo.via) vo.via[row + k] = w.x;
        if (vo.hops) vo.hops[row + k] = w.y;
    }
}

}  // namespace via
}  // namespace ketogpu

// combine.hpp — combined listings (include/ketogpu.h ketogpu_*_combine*): the list of a pair of
// ids (a, b) under an operator, M(a) AND / ANDNOT / OR M(b), shared by lookup.hip and
// subjects.hip.  Next to closure.hpp, and in its idiom: plain templates, the direction as data,
// the member filter a caller-supplied ok(u).
//
// A combined request is two closures into two visited structures with closure.hpp's finishes
// behind them; there is no finish of its own here.
//
//   tier 1  one wave per pair, two LDS sets of kSlotsLds words and one worklist that both
//           closures use in turn.  AND / ANDNOT: tier1_closure of a into set A, then of b into
//           set B; the finish runs over set A with the filter member(): ok(u) and u in / not in
//           set B (set_has: a read-only probe in set_insert's order).  The paged finish compacts
//           the set it runs over, so B is the one that is only probed.  OR: tier1_closure_pair,
//           one closure from both start rows into set A, so a pair overflows exactly when the
//           union passes kSetCap.  A pair either of whose closures passes kSetCap overflows.
//   tier 2  one workgroup of kT2Block per overflow pair, the slot's bitmap and worklist plus a
//           second bitmap of bm_words.  tier2_closure of a into the first bitmap, of b into the
//           second (OR: into the first again, over the same worklist started anew), then one
//           pass bm &= b2 or bm &= ~b2 that leaves the second bitmap all zero; the scan finishes
//           of closure.hpp then read and clear the first as they do for a plain request.
//
// A side that the plain call answers before it reads a row (KETOGPU_NODE_NONE; a root without a
// row) is the empty set and no closure runs for it: kNoRow.  Nothing is skipped beyond that, so
// the tier of a pair depends on its closures alone.
#pragma once

#include "closure.hpp"

namespace ketogpu {
namespace combine {

using namespace closure;

constexpr uint32_t kNoRow = kEmpty;  // a side that is the empty set by classification

// a pair as the plain calls classify its sides.  rb: the ids below it have a row to read (N
// backwards, Nx forwards); an id in [rb, N) and NONE are the empty set, anything else is INVALID
struct Pair {
    uint32_t va, vb;  // the start rows, or kNoRow
    bool invalid;     // an id outside the snapshot on either side
    bool unlisted;    // invalid, or no side has a row: answered here, in neither tier
};

__device__ inline Pair classify(const Rows &g, uint32_t rb, uint32_t a, uint32_t b) {
    Pair p;
    p.invalid = (a >= g.N && a != KETOGPU_NODE_NONE) || (b >= g.N && b != KETOGPU_NODE_NONE);
    p.va = a < rb ? a : kNoRow;
    p.vb = b < rb ? b : kNoRow;
    p.unlisted = p.invalid || (p.va == kNoRow && p.vb == kNoRow);
    return p;
}

// ---------------------------------------------------------------------- tier 1
// is u (never kEmpty) in the LDS set?  Reads only; set_insert's hash and probe order, and like
// it ends at a free slot.
__device__ __forceinline__ bool set_has(const uint32_t *set, uint32_t u) {
    uint32_t slot = slot_of(u);
    for (;;) {
        const uint32_t x = set[slot];
        if (x == u) return true;
        if (x == kEmpty) return false;
        slot = (slot + 1) & (kSlotsLds - 1);
    }
}

// the combined member filter over set A: ok(u), and for AND / ANDNOT u in / not in set B
template <class Ok>
__device__ __forceinline__ auto member(const uint32_t *set_b, uint32_t op, Ok ok) {
    return [=](uint32_t u) {
        return ok(u) && (op == KETOGPU_COMBINE_OR || set_has(set_b, u) == (op == KETOGPU_COMBINE_AND));
    };
}

// tier1_closure from two start rows (either may be kNoRow): both are worked before the worklist
// is drained, so `set` ends as the union of the two closures.  False when it passed kSetCap.
__device__ __forceinline__ bool tier1_closure_pair(const Rows &g, uint32_t bound, uint32_t va, uint32_t vb,
                                                   uint32_t lane, uint32_t *set, uint32_t *work) {
    for (uint32_t s = lane; s < kSlotsLds; s += 64) set[s] = kEmpty;
    __syncthreads();
    uint32_t v = va != kNoRow ? va : vb, next = va != kNoRow ? vb : kNoRow;
    if (v == kNoRow) return true;
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
        if (over) break;
        if (next != kNoRow) {
            v = next, next = kNoRow;
            continue;
        }
        if (head == tail) break;
        v = work[head++];
    }
    return !over;
}

// one side of AND / ANDNOT: tier1_closure, or the empty set for kNoRow
__device__ __forceinline__ bool tier1_side(const Rows &g, uint32_t bound, uint32_t v, uint32_t lane, uint32_t *set,
                                           uint32_t *work) {
    if (v != kNoRow) return tier1_closure(g, bound, v, lane, set, work);
    for (uint32_t s = lane; s < kSlotsLds; s += 64) set[s] = kEmpty;
    __syncthreads();
    return true;
}

// both closures of a pair, by one wave: what member() filters set A by is in set B.  False when
// a closure passed kSetCap: the pair overflows.
__device__ __forceinline__ bool tier1_pair(const Rows &g, uint32_t bound, const Pair &p, uint32_t op, uint32_t lane,
                                           uint32_t *set_a, uint32_t *set_b, uint32_t *work) {
    if (op == KETOGPU_COMBINE_OR) return tier1_closure_pair(g, bound, p.va, p.vb, lane, set_a, work);
    return tier1_side(g, bound, p.va, lane, set_a, work) && tier1_side(g, bound, p.vb, lane, set_b, work);
}

// tier 1 of a combined cursor call, the whole kernel body: request i of the wave at hand
template <class Ok>
__device__ __forceinline__ void tier1_list(const Rows &g, uint32_t bound, uint32_t rb, const uint32_t *a,
                                           const uint32_t *b, uint32_t i, uint32_t lane, uint32_t op,
                                           int force_tier2, const ListOut &o, uint32_t *ovf_list,
                                           unsigned int *ovf_count, uint32_t *set_a, uint32_t *set_b, uint32_t *work,
                                           Ok ok) {
    const Pair p = classify(g, rb, a[i], b[i]);
    if (p.unlisted) {
        if (lane == 0) {
            o.begin[i] = p.invalid ? KETOGPU_LOOKUP_INVALID : 0ull;
            o.count[i] = 0;
        }
        return;
    }
    if (force_tier2 || !tier1_pair(g, bound, p, op, lane, set_a, set_b, work)) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    tier1_finish(set_a, lane, i, o, member(set_b, op, ok));
}

// ... and of a combined paged call
template <class Ok>
__device__ __forceinline__ void tier1_page(const Rows &g, uint32_t bound, uint32_t rb, const uint32_t *a,
                                           const uint32_t *b, const uint32_t *from, uint32_t i, uint32_t lane,
                                           uint32_t op, int force_tier2, const paged::PageOut &o, uint32_t *ovf_list,
                                           unsigned int *ovf_count, uint32_t *set_a, uint32_t *set_b, uint32_t *work,
                                           Ok ok) {
    const Pair p = classify(g, rb, a[i], b[i]);
    if (p.unlisted) {
        if (lane == 0) paged::page_invalid(o, i, p.invalid);
        return;
    }
    if (force_tier2 || !tier1_pair(g, bound, p, op, lane, set_a, set_b, work)) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    paged::page_finish_wave(set_a, kSlotsLds, lane, i, from[i], o, member(set_b, op, ok));
}

// ---------------------------------------------------------------------- tier 2
// a tier-2 kernel's LDS counters, all zero on entry to tier2_pair
struct T2Lds {
    unsigned int tail, cnt, pos, rem;
    unsigned long long base;
    uint32_t wave[kT2Block / 64];
};

__device__ __forceinline__ void t2_lds_clear(T2Lds &s) {
    if (threadIdx.x == 0) s.tail = 0, s.cnt = 0, s.pos = 0, s.rem = 0;
    __syncthreads();
}

// both closures of a pair and the operator, by the whole workgroup: the combined set ends in
// `bm`; `b2` (all zero on entry) is all zero again on the way out.  Ends behind a barrier.
__device__ __forceinline__ void tier2_pair(const Rows &g, uint32_t bound, const Pair &p, uint32_t op, uint32_t *bm,
                                           uint32_t *b2, uint64_t bm_words, uint32_t *wl, unsigned int *s_tail) {
    auto none = [](uint32_t, uint32_t) {};
    auto never = [] { return false; };
    if (p.va != kNoRow) tier2_closure(g, bound, p.va, bm, wl, s_tail, none, never);
    __syncthreads();  // everyone has read a's last tail
    if (threadIdx.x == 0) *s_tail = 0;
    __syncthreads();  // the worklist starts anew
    if (p.vb != kNoRow) tier2_closure(g, bound, p.vb, op == KETOGPU_COMBINE_OR ? bm : b2, wl, s_tail, none, never);
    if (op != KETOGPU_COMBINE_OR) {
        for (uint64_t w = threadIdx.x; w < bm_words; w += kT2Block) {
            const uint32_t x = b2[w], m = bm[w];
            const uint32_t r = op == KETOGPU_COMBINE_AND ? m & x : m & ~x;
            if (r != m) bm[w] = r;
            if (x) b2[w] = 0;
        }
    }
    __syncthreads();  // the finishes read words that other threads combined
}

// tier 2 of a combined cursor call, the whole kernel body: the pair of overflow request i with
// the state of the slot at hand.  Both bitmaps are all zero on entry and on every way out.
template <class Ok>
__device__ __forceinline__ void tier2_list(const Rows &g, uint32_t bound, uint32_t rb, uint32_t a, uint32_t b,
                                           uint32_t i, uint32_t op, const ListOut &o, uint32_t *bm, uint32_t *b2,
                                           uint64_t bm_words, uint32_t *wl, T2Lds &s, Ok ok) {
    t2_lds_clear(s);
    const Pair p = classify(g, rb, a, b);
    if (p.unlisted) return;  // (tier 1 lists pairs with a row to read only)
    tier2_pair(g, bound, p, op, bm, b2, bm_words, wl, &s.tail);
    const unsigned long long base = reserve_block(o, i, scan_count(bm, bm_words, ok), &s.cnt, &s.base);
    scan_write(bm, bm_words, base, o.out, ok, &s.pos);
}

// ... and of a combined paged call: selection in id order first, then one scan that counts and
// clears
template <class Ok>
__device__ __forceinline__ void tier2_page(const Rows &g, uint32_t bound, uint32_t rb, uint32_t a, uint32_t b,
                                           uint32_t lo, uint32_t i, uint32_t op, const paged::PageOut &o, uint32_t *bm,
                                           uint32_t *b2, uint64_t bm_words, uint32_t *wl, T2Lds &s, Ok ok) {
    t2_lds_clear(s);
    const Pair p = classify(g, rb, a, b);
    if (p.unlisted) return;  // (tier 1 lists pairs with a row to read only)
    tier2_pair(g, bound, p, op, bm, b2, bm_words, wl, &s.tail);
    paged::page_select_block(bm, bm_words, lo, o.limit, o.out + (uint64_t)i * o.limit, s.wave, ok);
    __syncthreads();  // the selection has read the bitmap
    page_report(o, i, page_count_clear(bm, bm_words, lo, ok), &s.cnt, &s.rem);
}

}  // namespace combine
}  // namespace ketogpu

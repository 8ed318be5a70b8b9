// subjects.hip — subject listing on the device (include/ketogpu.h ketogpu_subjects_*).
//
// subjects(r, C) lists F(r), the nodes reached from r in >= 1 edge over the rows the check
// engine sees, restricted to the class C: the least set that holds row(r) and row(x) for every
// interior x in it (DESIGN.md "Subject listing").  The rows live in HBM as a CSR over the
// expandable nodes (fwd_off / fwd_col), built at upload from the snapshot's host rows: compact
// on a snapshot that cannot change in place, an arena of rows with room to grow on a writable
// one, which in-place writes are patched into (DESIGN.md "Listing handles and writes").  The
// rows are neither sorted nor deduplicated, the sets dedup.  The closure, its two tiers and the list
// finishes are closure.hpp's, over these rows with the member bound num_nodes; the host side of
// the handle is hip_host.hpp's ListHandle.  What is here: the class filter, the classification
// of a root, the seen list and the finish by it, the kernels as bodies over the shared pieces,
// the upload and the statistics.
//
//   tier 1  one wave per request, the closure in an LDS set.  A request whose set passes
//           kSetCap is appended to the overflow list and leaves no output.
//   tier 2  one workgroup per overflow request, `slots` requests per launch.  Each slot has a
//           bitmap over all N nodes, a worklist of Ni entries and a seen list of `list_cap`
//           entries in global memory.  Every first visit is counted and, while there is room,
//           appended to the seen list.  A closure that stayed within list_cap finishes BY LIST
//           (count, reserve, write and clear the bitmap by walking the list: 4 bytes per
//           member); a larger one finishes BY SCAN of the bitmap (two passes over N / 8 bytes
//           whatever the answer is).
//
// The paged call (ketogpu_subjects_page) runs the same two closures and ends with the ordered
// finish of paged_finish.hpp instead: the `limit` smallest members >= from[i] to the stride
// out + i * limit, ascending, with the exact count and what remains; no cursor, no truncation.
//
// The depth calls (ketogpu_subjects_ids_depth / _page_depth) list the members within
// max_depth[i] hops of the root: the full-list and the paged kernels with depth.hpp's level
// bookkeeping in the closures, both tier-2 finishes, and frontier[i], the interior members the
// limit left unread, next to the count.
//
// The via calls (ketogpu_subjects_ids_via / _page_via) are the depth calls with, next to every
// member, the node whose row granted it and its hop count: via.hpp's bodies, which keep a parent
// and a level per first visit.
//
// The expand call (ketogpu_subjects_expand) is no listing: it writes BuildTree's tree of each
// root as two preorder arrays, word for word what the host walk gives.  The bodies are
// expand_tree.hpp's: an ordered depth-first walk over the same rows, with the sets, slots and
// reservations of the closures.
//
// The wide call (ketogpu_subjects_ids_wide) is the full-list call with tier 1's overflows run by
// wide.hpp's level-synchronous tier, spread over the whole device, instead of tier 2.  The wide
// depth and paged calls (ketogpu_subjects_ids_depth_wide / _page_wide) are the depth calls with
// the same replacement: level L of the wide tier is its launch L, and the paged finish is
// wide.hpp's select, clear and report.
//
// Every index is validated before it is used: roots against N, and against Nx before fwd_off
// is touched; row entries against N before the class array or a bitmap is.
#include <hip/hip_runtime.h>

#include "combine.hpp"
#include "depth.hpp"
#include "expand_tree.hpp"
#include "expand_wide.hpp"
#include "hip_host.hpp"
#include "subjects.hpp"
#include "via.hpp"

using namespace ketogpu;
using namespace ketogpu::closure;

namespace {

constexpr uint32_t kListCapDefault = 65536;  // tier 2: 256 KiB of seen list per slot

// The graph g of every kernel: fwd_off (Nx + 1 offsets), fwd_col, the rows' ends where they lie
// in an arena (Rows::end), the class of each of the N nodes as the filter key, and the bound N.

struct SOut {
    ListOut l;
    unsigned long long *list_finishes, *scan_finishes;
};

__device__ inline bool class_ok(const Rows &g, uint32_t u, uint32_t want) {
    if (u >= g.N) return false;
    const uint32_t c = g.filter_key[u];
    return want == KETOGPU_TYPE_ANY
               ? c != KETOGPU_TYPE_NONE
               : (want != KETOGPU_TYPE_NONE && want != KETOGPU_CLASS_UNTYPED_SET && c == want);
}

// tier 2's closure with the seen list: every first visit is counted in *s_seen (an LDS counter,
// zero on entry) and, while there is room, appended to `seen`
__device__ __forceinline__ void tier2_closure_seen(const Rows &g, uint32_t r, uint32_t *bm, uint32_t *wl,
                                                   uint32_t *seen, uint32_t list_cap, unsigned int *s_tail,
                                                   unsigned int *s_seen) {
    tier2_closure(
        g, g.N, r, bm, wl, s_tail,
        [&](uint32_t u, uint32_t) {
            const uint32_t k = atomicAdd(s_seen, 1u);
            if (k < list_cap) seen[k] = u;
        },
        [] { return false; });
}

// ---------------------------------------------------------------------- full lists
__global__ __launch_bounds__(64) void subjects_tier1_kernel(Rows g, const uint32_t *roots, uint32_t n, uint32_t cls,
                                                            int force_tier2, SOut o, uint32_t *ovf_list,
                                                            unsigned int *ovf_count) {
    __shared__ uint32_t set[kSlotsLds];
    __shared__ uint32_t work[kSetCap + 64];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const uint32_t r = roots[i];
    if (r >= g.Nx) {  // NONE and the never-expanded nodes: the empty list; an id outside the snapshot: INVALID
        if (lane == 0) {
            o.l.begin[i] = (r < g.N || r == KETOGPU_NODE_NONE) ? 0ull : KETOGPU_LOOKUP_INVALID;
            o.l.count[i] = 0;
        }
        return;
    }
    if (force_tier2) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    const bool over = !tier1_closure(g, g.N, r, lane, set, work);
    if (over) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    tier1_finish(set, lane, i, o.l, [&](uint32_t u) { return class_ok(g, u, cls); });
}

// Block s of round r serves overflow request ovf_list[first + s] with slot s's state.  The
// bitmap is all zero on entry and is cleared again on the way out, by either finish.
__global__ __launch_bounds__(kT2Block) void subjects_tier2_kernel(Rows g, const uint32_t *roots, uint32_t cls, SOut o,
                                                                  const uint32_t *ovf_list, uint32_t first,
                                                                  uint32_t *bitmaps, uint64_t bm_words,
                                                                  uint32_t *worklists, uint32_t *seen_lists,
                                                                  uint32_t list_cap) {
    __shared__ unsigned int s_tail, s_seen, s_cnt, s_pos;
    __shared__ unsigned long long s_base;
    const uint32_t i = ovf_list[first + blockIdx.x];
    const uint32_t r = roots[i];
    uint32_t *bm = bitmaps + (uint64_t)blockIdx.x * bm_words;
    uint32_t *wl = worklists + (uint64_t)blockIdx.x * g.Ni;
    uint32_t *seen = seen_lists + (uint64_t)blockIdx.x * list_cap;
    const unsigned tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_tail = 0, s_seen = 0, s_cnt = 0, s_pos = 0;
    __syncthreads();
    if (r >= g.Nx) return;  // (tier 1 lists expandable roots only)
    tier2_closure_seen(g, r, bm, wl, seen, list_cap, &s_tail, &s_seen);
    const uint32_t total = s_seen;
    const bool by_list = list_cap && total <= list_cap;  // the seen list holds the whole closure
    auto ok = [&](uint32_t u) { return class_ok(g, u, cls); };
    uint32_t c = 0;  // count the members of the class
    if (by_list) {
        for (uint32_t k = tid; k < total; k += kT2Block) {
            const uint32_t u = seen[k];
            c += ok(u);
            bm[u >> 5] = 0;  // every set bit of the word is some member's: all of them store the same zero
        }
    } else {
        c = scan_count(bm, bm_words, ok);
    }
    const unsigned long long base = reserve_block(o.l, i, c, &s_cnt, &s_base);
    if (tid == 0) atomicAdd(by_list ? o.list_finishes : o.scan_finishes, 1ull);
    if (!by_list) {
        scan_write(bm, bm_words, base, o.l.out, ok, &s_pos);
        return;
    }
    if (base == KETOGPU_LOOKUP_TRUNCATED) return;
    for (uint32_t k0 = 0; k0 < total; k0 += kT2Block) {  // (a uniform trip count: the ballot sees whole waves)
        const uint32_t k = k0 + tid;
        const uint32_t u = k < total ? seen[k] : kEmpty;
        const bool m = ok(u);
        const unsigned long long mm = __ballot(m);
        uint32_t p = 0;
        if (lane == 0 && mm) p = atomicAdd(&s_pos, (unsigned)__popcll(mm));
        p = __shfl(p, 0);
        if (m) o.l.out[base + p + __popcll(mm & ((1ull << lane) - 1))] = u;
    }
}

// ---------------------------------------------------------------------- paged finish
// The same closures with the ordered finish of paged_finish.hpp: request i reports count,
// remaining and returned, and writes its page to the stride out + i * limit.
__global__ __launch_bounds__(64) void subjects_page_tier1_kernel(Rows g, const uint32_t *roots, const uint32_t *from,
                                                                 uint32_t n, uint32_t cls, int force_tier2,
                                                                 paged::PageOut o, uint32_t *ovf_list,
                                                                 unsigned int *ovf_count) {
    __shared__ uint32_t set[kSlotsLds];
    __shared__ uint32_t work[kSetCap + 64];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const uint32_t r = roots[i];
    if (r >= g.Nx) {  // NONE and the never-expanded nodes: the empty page; an id outside the snapshot: INVALID
        if (lane == 0) paged::page_invalid(o, i, !(r < g.N || r == KETOGPU_NODE_NONE));
        return;
    }
    if (force_tier2 || !tier1_closure(g, g.N, r, lane, set, work)) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    paged::page_finish_wave(set, kSlotsLds, lane, i, from[i], o, [&](uint32_t u) { return class_ok(g, u, cls); });
}

// Selection in id order first; then the members are counted and the bitmap cleared, by the
// seen list if it holds the whole closure and by one scan otherwise: the slot is left all zero
// for whichever kernel of the handle uses it next.
__global__ __launch_bounds__(kT2Block) void subjects_page_tier2_kernel(Rows g, const uint32_t *roots,
                                                                       const uint32_t *from, uint32_t cls,
                                                                       paged::PageOut o, unsigned long long *list_finishes,
                                                                       unsigned long long *scan_finishes,
                                                                       const uint32_t *ovf_list, uint32_t first,
                                                                       uint32_t *bitmaps, uint64_t bm_words,
                                                                       uint32_t *worklists, uint32_t *seen_lists,
                                                                       uint32_t list_cap) {
    __shared__ unsigned int s_tail, s_seen, s_cnt, s_rem;
    __shared__ uint32_t s_wave[kT2Block / 64];
    const uint32_t i = ovf_list[first + blockIdx.x];
    const uint32_t r = roots[i];
    uint32_t *bm = bitmaps + (uint64_t)blockIdx.x * bm_words;
    uint32_t *wl = worklists + (uint64_t)blockIdx.x * g.Ni;
    uint32_t *seen = seen_lists + (uint64_t)blockIdx.x * list_cap;
    const unsigned tid = threadIdx.x;
    if (tid == 0) s_tail = 0, s_seen = 0, s_cnt = 0, s_rem = 0;
    __syncthreads();
    if (r >= g.Nx) return;  // (tier 1 lists expandable roots only)
    tier2_closure_seen(g, r, bm, wl, seen, list_cap, &s_tail, &s_seen);
    const uint32_t total = s_seen;
    const bool by_list = list_cap && total <= list_cap;  // the seen list holds the whole closure
    const uint32_t lo = from[i];
    auto ok = [&](uint32_t u) { return class_ok(g, u, cls); };
    paged::page_select_block(bm, bm_words, lo, o.limit, o.out + (uint64_t)i * o.limit, s_wave, ok);
    __syncthreads();  // the selection has read the bitmap
    PageCount mine{0, 0};
    if (by_list) {
        for (uint32_t k = tid; k < total; k += kT2Block) {
            const uint32_t u = seen[k];
            const bool m = ok(u);
            mine.count += m;
            mine.remaining += m && u >= lo;
            bm[u >> 5] = 0;  // every set bit of the word is some member's: all of them store the same zero
        }
    } else {
        mine = page_count_clear(bm, bm_words, lo, ok);
    }
    page_report(o, i, mine, &s_cnt, &s_rem);
    if (tid == 0) atomicAdd(by_list ? list_finishes : scan_finishes, 1ull);
}

// ---------------------------------------------------------------------- combined listings
// ketogpu_subjects_combine / _combine_page: subjects(a, C) AND / ANDNOT / OR subjects(b, C).
// The bodies are combine.hpp's, over the forward rows: the ids below Nx have a row, the member
// bound is N.  Tier 2 finishes by scan only: the seen list is not used.
__global__ __launch_bounds__(64) void subjects_combine_tier1_kernel(Rows g, const uint32_t *a, const uint32_t *b,
                                                                    uint32_t n, uint32_t op, uint32_t cls,
                                                                    int force_tier2, ListOut o, uint32_t *ovf_list,
                                                                    unsigned int *ovf_count) {
    __shared__ uint32_t set_a[kSlotsLds], set_b[kSlotsLds];
    __shared__ uint32_t work[kSetCap + 64];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    combine::tier1_list(g, g.N, g.Nx, a, b, i, lane, op, force_tier2, o, ovf_list, ovf_count, set_a, set_b, work,
                        [&](uint32_t u) { return class_ok(g, u, cls); });
}

__global__ __launch_bounds__(kT2Block) void subjects_combine_tier2_kernel(Rows g, const uint32_t *a, const uint32_t *b,
                                                                          uint32_t op, uint32_t cls, ListOut o,
                                                                          const uint32_t *ovf_list, uint32_t first,
                                                                          uint32_t *bitmaps, uint32_t *bitmaps2,
                                                                          uint64_t bm_words, uint32_t *worklists) {
    __shared__ combine::T2Lds s;
    const uint32_t i = ovf_list[first + blockIdx.x];
    combine::tier2_list(g, g.N, g.Nx, a[i], b[i], i, op, o, bitmaps + (uint64_t)blockIdx.x * bm_words,
                        bitmaps2 + (uint64_t)blockIdx.x * bm_words, bm_words, worklists + (uint64_t)blockIdx.x * g.Ni,
                        s, [&](uint32_t u) { return class_ok(g, u, cls); });
}

__global__ __launch_bounds__(64) void subjects_combine_page_tier1_kernel(Rows g, const uint32_t *a, const uint32_t *b,
                                                                         const uint32_t *from, uint32_t n, uint32_t op,
                                                                         uint32_t cls, int force_tier2,
                                                                         paged::PageOut o, uint32_t *ovf_list,
                                                                         unsigned int *ovf_count) {
    __shared__ uint32_t set_a[kSlotsLds], set_b[kSlotsLds];
    __shared__ uint32_t work[kSetCap + 64];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    combine::tier1_page(g, g.N, g.Nx, a, b, from, i, lane, op, force_tier2, o, ovf_list, ovf_count, set_a, set_b,
                        work, [&](uint32_t u) { return class_ok(g, u, cls); });
}

__global__ __launch_bounds__(kT2Block) void subjects_combine_page_tier2_kernel(
    Rows g, const uint32_t *a, const uint32_t *b, const uint32_t *from, uint32_t op, uint32_t cls, paged::PageOut o,
    const uint32_t *ovf_list, uint32_t first, uint32_t *bitmaps, uint32_t *bitmaps2, uint64_t bm_words,
    uint32_t *worklists) {
    __shared__ combine::T2Lds s;
    const uint32_t i = ovf_list[first + blockIdx.x];
    combine::tier2_page(g, g.N, g.Nx, a[i], b[i], from[i], i, op, o, bitmaps + (uint64_t)blockIdx.x * bm_words,
                        bitmaps2 + (uint64_t)blockIdx.x * bm_words, bm_words, worklists + (uint64_t)blockIdx.x * g.Ni,
                        s, [&](uint32_t u) { return class_ok(g, u, cls); });
}

// ---------------------------------------------------------------------- depth-limited listings
// ketogpu_subjects_ids_depth / _page_depth: the members of subjects(r, C) within max_depth[i]
// hops of r (DESIGN.md "Depth-limited listings").  The kernels of the plain calls with
// depth.hpp's closure in tier 1 and its LevelStop in tier 2; both tier-2 finishes are kept: a
// depth-limited answer is the short list the seen list exists for.  frontier[i] is all zero on
// entry and is written where a search stopped at its limit.

// a member under any filter: what the frontier counts (a placeholder has no class)
__device__ inline bool any_class(const Rows &g, uint32_t u) { return class_ok(g, u, KETOGPU_TYPE_ANY); }

// tier2_closure_seen under a depth limit (a sibling: the plain kernels keep theirs), and the
// frontier of the search to *frontier.  *s_fr is an LDS counter, zero on entry.
__device__ __forceinline__ void tier2_closure_seen_depth(const Rows &g, uint32_t r, uint32_t max_depth, uint32_t *bm,
                                                         uint32_t *wl, uint32_t *seen, uint32_t list_cap,
                                                         unsigned int *s_tail, unsigned int *s_seen,
                                                         unsigned int *s_fr, unsigned long long *frontier) {
    depth::LevelStop stop(s_tail, max_depth);
    tier2_closure(
        g, g.N, r, bm, wl, s_tail,
        [&](uint32_t u, uint32_t) {
            const uint32_t k = atomicAdd(s_seen, 1u);
            if (k < list_cap) seen[k] = u;
        },
        depth::LevelStopRef{&stop});
    depth::tier2_frontier(stop, wl, frontier, s_fr, [&](uint32_t u) { return any_class(g, u); });
}

__global__ __launch_bounds__(64) void subjects_depth_tier1_kernel(Rows g, const uint32_t *roots,
                                                                  const uint32_t *max_depth, uint32_t n, uint32_t cls,
                                                                  int force_tier2, SOut o,
                                                                  unsigned long long *frontier, uint32_t *ovf_list,
                                                                  unsigned int *ovf_count) {
    __shared__ uint32_t set[kSlotsLds];
    __shared__ uint32_t work[kSetCap + 64];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const uint32_t r = roots[i];
    if (r >= g.Nx) {  // NONE and the never-expanded nodes: the empty list; an id outside the snapshot: INVALID
        if (lane == 0) {
            o.l.begin[i] = (r < g.N || r == KETOGPU_NODE_NONE) ? 0ull : KETOGPU_LOOKUP_INVALID;
            o.l.count[i] = 0;
        }
        return;
    }
    uint32_t fr = 0;
    if (force_tier2 || !depth::tier1_closure(g, g.N, r, depth::limit_of(max_depth, i), lane, set, work, fr,
                                              [&](uint32_t u) { return any_class(g, u); })) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    if (lane == 0 && fr) frontier[i] = fr;
    tier1_finish(set, lane, i, o.l, [&](uint32_t u) { return class_ok(g, u, cls); });
}

__global__ __launch_bounds__(kT2Block) void subjects_depth_tier2_kernel(Rows g, const uint32_t *roots,
                                                                        const uint32_t *max_depth, uint32_t cls,
                                                                        SOut o, unsigned long long *frontier,
                                                                        const uint32_t *ovf_list, uint32_t first,
                                                                        uint32_t *bitmaps, uint64_t bm_words,
                                                                        uint32_t *worklists, uint32_t *seen_lists,
                                                                        uint32_t list_cap) {
    __shared__ unsigned int s_tail, s_seen, s_cnt, s_pos, s_fr;
    __shared__ unsigned long long s_base;
    const uint32_t i = ovf_list[first + blockIdx.x];
    const uint32_t r = roots[i];
    uint32_t *bm = bitmaps + (uint64_t)blockIdx.x * bm_words;
    uint32_t *wl = worklists + (uint64_t)blockIdx.x * g.Ni;
    uint32_t *seen = seen_lists + (uint64_t)blockIdx.x * list_cap;
    const unsigned tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_tail = 0, s_seen = 0, s_cnt = 0, s_pos = 0, s_fr = 0;
    __syncthreads();
    if (r >= g.Nx) return;  // (tier 1 lists expandable roots only)
    tier2_closure_seen_depth(g, r, depth::limit_of(max_depth, i), bm, wl, seen, list_cap, &s_tail, &s_seen, &s_fr,
                             frontier + i);
    const uint32_t total = s_seen;
    const bool by_list = list_cap && total <= list_cap;  // the seen list holds every member within the limit
    auto ok = [&](uint32_t u) { return class_ok(g, u, cls); };
    uint32_t c = 0;  // count the members of the class
    if (by_list) {
        for (uint32_t k = tid; k < total; k += kT2Block) {
            const uint32_t u = seen[k];
            c += ok(u);
            bm[u >> 5] = 0;  // every set bit of the word is some member's: all of them store the same zero
        }
    } else {
        c = scan_count(bm, bm_words, ok);
    }
    const unsigned long long base = reserve_block(o.l, i, c, &s_cnt, &s_base);
    if (tid == 0) atomicAdd(by_list ? o.list_finishes : o.scan_finishes, 1ull);
    if (!by_list) {
        scan_write(bm, bm_words, base, o.l.out, ok, &s_pos);
        return;
    }
    if (base == KETOGPU_LOOKUP_TRUNCATED) return;
    for (uint32_t k0 = 0; k0 < total; k0 += kT2Block) {  // (a uniform trip count: the ballot sees whole waves)
        const uint32_t k = k0 + tid;
        const uint32_t u = k < total ? seen[k] : kEmpty;
        const bool m = ok(u);
        const unsigned long long mm = __ballot(m);
        uint32_t p = 0;
        if (lane == 0 && mm) p = atomicAdd(&s_pos, (unsigned)__popcll(mm));
        p = __shfl(p, 0);
        if (m) o.l.out[base + p + __popcll(mm & ((1ull << lane) - 1))] = u;
    }
}

__global__ __launch_bounds__(64) void subjects_depth_page_tier1_kernel(Rows g, const uint32_t *roots,
                                                                       const uint32_t *max_depth, const uint32_t *from,
                                                                       uint32_t n, uint32_t cls, int force_tier2,
                                                                       paged::PageOut o, unsigned long long *frontier,
                                                                       uint32_t *ovf_list, unsigned int *ovf_count) {
    __shared__ uint32_t set[kSlotsLds];
    __shared__ uint32_t work[kSetCap + 64];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const uint32_t r = roots[i];
    if (r >= g.Nx) {  // NONE and the never-expanded nodes: the empty page; an id outside the snapshot: INVALID
        if (lane == 0) paged::page_invalid(o, i, !(r < g.N || r == KETOGPU_NODE_NONE));
        return;
    }
    uint32_t fr = 0;
    if (force_tier2 || !depth::tier1_closure(g, g.N, r, depth::limit_of(max_depth, i), lane, set, work, fr,
                                              [&](uint32_t u) { return any_class(g, u); })) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    if (lane == 0 && fr) frontier[i] = fr;
    paged::page_finish_wave(set, kSlotsLds, lane, i, from[i], o, [&](uint32_t u) { return class_ok(g, u, cls); });
}

__global__ __launch_bounds__(kT2Block) void subjects_depth_page_tier2_kernel(
    Rows g, const uint32_t *roots, const uint32_t *max_depth, const uint32_t *from, uint32_t cls, paged::PageOut o,
    unsigned long long *frontier, unsigned long long *list_finishes, unsigned long long *scan_finishes,
    const uint32_t *ovf_list, uint32_t first, uint32_t *bitmaps, uint64_t bm_words, uint32_t *worklists,
    uint32_t *seen_lists, uint32_t list_cap) {
    __shared__ unsigned int s_tail, s_seen, s_cnt, s_rem, s_fr;
    __shared__ uint32_t s_wave[kT2Block / 64];
    const uint32_t i = ovf_list[first + blockIdx.x];
    const uint32_t r = roots[i];
    uint32_t *bm = bitmaps + (uint64_t)blockIdx.x * bm_words;
    uint32_t *wl = worklists + (uint64_t)blockIdx.x * g.Ni;
    uint32_t *seen = seen_lists + (uint64_t)blockIdx.x * list_cap;
    const unsigned tid = threadIdx.x;
    if (tid == 0) s_tail = 0, s_seen = 0, s_cnt = 0, s_rem = 0, s_fr = 0;
    __syncthreads();
    if (r >= g.Nx) return;  // (tier 1 lists expandable roots only)
    tier2_closure_seen_depth(g, r, depth::limit_of(max_depth, i), bm, wl, seen, list_cap, &s_tail, &s_seen, &s_fr,
                             frontier + i);
    const uint32_t total = s_seen;
    const bool by_list = list_cap && total <= list_cap;  // the seen list holds every member within the limit
    const uint32_t lo = from[i];
    auto ok = [&](uint32_t u) { return class_ok(g, u, cls); };
    paged::page_select_block(bm, bm_words, lo, o.limit, o.out + (uint64_t)i * o.limit, s_wave, ok);
    __syncthreads();  // the selection has read the bitmap
    PageCount mine{0, 0};
    if (by_list) {
        for (uint32_t k = tid; k < total; k += kT2Block) {
            const uint32_t u = seen[k];
            const bool m = ok(u);
            mine.count += m;
            mine.remaining += m && u >= lo;
            bm[u >> 5] = 0;  // every set bit of the word is some member's: all of them store the same zero
        }
    } else {
        mine = page_count_clear(bm, bm_words, lo, ok);
    }
    page_report(o, i, mine, &s_cnt, &s_rem);
    if (tid == 0) atomicAdd(by_list ? list_finishes : scan_finishes, 1ull);
}

// ---------------------------------------------------------------------- listings that say why
// ketogpu_subjects_ids_via / _page_via: the depth-limited listings with via[k], the node in
// whose row out[k] was first seen (out[k] is an entry of row(via[k]), one hop nearer the root),
// and hops[k], its distance (DESIGN.md "Grant trees").  The bodies are via.hpp's, over the
// forward rows: the ids below Nx have a row, the member bound is N; both tier-2 finishes are
// kept.  A slot adds 2 x N words.
__device__ inline via::Slot subjects_via_slot(const Rows &g, uint32_t *bitmaps, uint64_t bm_words,
                                              uint32_t *worklists, uint32_t *seen_lists, uint32_t list_cap,
                                              uint32_t *words, unsigned long long *list_finishes,
                                              unsigned long long *scan_finishes) {
    uint2 *why = reinterpret_cast<uint2 *>(words) + (uint64_t)blockIdx.x * g.N;
    return {bitmaps + (uint64_t)blockIdx.x * bm_words, bm_words, worklists + (uint64_t)blockIdx.x * g.Ni, why,
            seen_lists + (uint64_t)blockIdx.x * list_cap, list_cap, list_finishes, scan_finishes};
}

__global__ __launch_bounds__(64) void subjects_via_tier1_kernel(Rows g, const uint32_t *roots,
                                                                const uint32_t *max_depth, uint32_t n, uint32_t cls,
                                                                int force_tier2, ListOut o, via::ViaOut vo,
                                                                unsigned long long *frontier, uint32_t *ovf_list,
                                                                unsigned int *ovf_count) {
    __shared__ via::T1Lds s;
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    via::tier1_list(
        g, g.N, g.Nx, roots, max_depth, i, lane, force_tier2, o, vo, frontier, ovf_list, ovf_count, s,
        [&](uint32_t u) { return class_ok(g, u, cls); }, [&](uint32_t u) { return any_class(g, u); });
}

__global__ __launch_bounds__(kT2Block) void subjects_via_tier2_kernel(Rows g, const uint32_t *roots,
                                                                      const uint32_t *max_depth, uint32_t cls, SOut o,
                                                                      via::ViaOut vo, unsigned long long *frontier,
                                                                      const uint32_t *ovf_list, uint32_t first,
                                                                      uint32_t *bitmaps, uint64_t bm_words,
                                                                      uint32_t *worklists, uint32_t *seen_lists,
                                                                      uint32_t list_cap, uint32_t *words) {
    __shared__ via::T2Lds s;
    const uint32_t i = ovf_list[first + blockIdx.x];
    via::tier2_list<true>(
        g, g.N, g.Nx, roots[i], depth::limit_of(max_depth, i), i, o.l, vo, frontier,
        subjects_via_slot(g, bitmaps, bm_words, worklists, seen_lists, list_cap, words, o.list_finishes,
                          o.scan_finishes),
        s, [&](uint32_t u) { return class_ok(g, u, cls); }, [&](uint32_t u) { return any_class(g, u); });
}

__global__ __launch_bounds__(64) void subjects_via_page_tier1_kernel(Rows g, const uint32_t *roots,
                                                                     const uint32_t *max_depth, const uint32_t *from,
                                                                     uint32_t n, uint32_t cls, int force_tier2,
                                                                     paged::PageOut o, via::ViaOut vo,
                                                                     unsigned long long *frontier, uint32_t *ovf_list,
                                                                     unsigned int *ovf_count) {
    __shared__ via::T1Lds s;
    __shared__ uint32_t keys[kSlotsLds];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    via::tier1_page(
        g, g.N, g.Nx, roots, max_depth, from, i, lane, force_tier2, o, vo, frontier, ovf_list, ovf_count, s, keys,
        [&](uint32_t u) { return class_ok(g, u, cls); }, [&](uint32_t u) { return any_class(g, u); });
}

__global__ __launch_bounds__(kT2Block) void subjects_via_page_tier2_kernel(
    Rows g, const uint32_t *roots, const uint32_t *max_depth, const uint32_t *from, uint32_t cls, paged::PageOut o,
    via::ViaOut vo, unsigned long long *frontier, unsigned long long *list_finishes,
    unsigned long long *scan_finishes, const uint32_t *ovf_list, uint32_t first, uint32_t *bitmaps, uint64_t bm_words,
    uint32_t *worklists, uint32_t *seen_lists, uint32_t list_cap, uint32_t *words) {
    __shared__ via::T2Lds s;
    const uint32_t i = ovf_list[first + blockIdx.x];
    via::tier2_page<true>(
        g, g.N, g.Nx, roots[i], depth::limit_of(max_depth, i), from[i], i, o, vo, frontier,
        subjects_via_slot(g, bitmaps, bm_words, worklists, seen_lists, list_cap, words, list_finishes, scan_finishes),
        s, [&](uint32_t u) { return class_ok(g, u, cls); }, [&](uint32_t u) { return any_class(g, u); });
}

// ---------------------------------------------------------------------- expand
// ketogpu_subjects_expand: the bodies are expand_tree.hpp's.  Tier 2 uses the slot's bitmap and
// seen list and adds a DFS stack of stack_words words per slot.
__global__ __launch_bounds__(64) void subjects_expand_tier1_kernel(expand::Graph x, const uint32_t *roots,
                                                                   const uint32_t *depths, uint32_t n,
                                                                   int force_tier2, expand::TreeOut o,
                                                                   uint32_t *ovf_list, unsigned int *ovf_count) {
    __shared__ expand::T1Lds s;
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    expand::tier1_tree(x, roots, depths, i, lane, force_tier2, o, ovf_list, ovf_count, s);
}

__global__ __launch_bounds__(kT2Block) void subjects_expand_tier2_kernel(expand::Graph x, const uint32_t *roots,
                                                                         const uint32_t *depths, expand::TreeOut o,
                                                                         const uint32_t *ovf_list, uint32_t first,
                                                                         uint32_t *bitmaps, uint64_t bm_words,
                                                                         uint32_t *seen_lists, uint32_t list_cap,
                                                                         uint32_t *stacks, uint64_t stack_words) {
    __shared__ expand::T2Lds s;
    __shared__ unsigned long long s_base;
    const uint32_t i = ovf_list[first + blockIdx.x];
    const expand::Slot sl{bitmaps + (uint64_t)blockIdx.x * bm_words, bm_words,
                          seen_lists + (uint64_t)blockIdx.x * list_cap, list_cap,
                          stacks + (uint64_t)blockIdx.x * stack_words};
    expand::tier2_tree(x, roots[i], depths[i], i, sl, s, &s_base, o);
}

// ketogpu_subjects_expand_wide: the bodies are expand_wide.hpp's.  The mask kernel runs when the
// rows changed, the fill kernel in-stream behind tier 1; tier 2 is the kernel above.
__global__ __launch_bounds__(expand::xwide::kMaskBlock) void subjects_expand_mask_kernel(expand::Graph x,
                                                                                        uint64_t col_words,
                                                                                        unsigned long long *mask,
                                                                                        uint64_t words) {
    expand::xwide::mask_build(x, col_words, mask, words);
}

__global__ __launch_bounds__(64) void subjects_expand_wide_tier1_kernel(expand::Graph x,
                                                                        const unsigned long long *mask,
                                                                        expand::xwide::Queue q, const uint32_t *roots,
                                                                        const uint32_t *depths, uint32_t n,
                                                                        int force_tier2, expand::TreeOut o,
                                                                        uint32_t *ovf_list, unsigned int *ovf_count) {
    __shared__ expand::T1Lds s;
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    expand::xwide::tier1_tree(x, mask, q, roots, depths, i, lane, force_tier2, o, ovf_list, ovf_count, s);
}

__global__ __launch_bounds__(expand::xwide::kFillBlock) void subjects_expand_fill_kernel(expand::Graph x,
                                                                                        expand::xwide::Queue q,
                                                                                        expand::TreeOut o) {
    expand::xwide::fill(x, q, o);
}

// ---------------------------------------------------------------------- the wide tier
// ketogpu_subjects_ids_wide: the bodies are wide.hpp's, over the forward rows: the ids below Nx
// have a row, the member bound is N.  The slot's bitmap is tier 2's; seen lists and worklists
// are not used.
__global__ __launch_bounds__(wide::kBlock) void subjects_wide_level_kernel(Rows g, uint32_t cls, wide::State w,
                                                                           unsigned long long lb,
                                                                           unsigned long long le) {
    wide::level(g, g.N, w, lb, le, [&](uint32_t u) { return class_ok(g, u, cls); });
}

__global__ __launch_bounds__(wide::kBlock) void subjects_wide_write_kernel(Rows g, uint32_t cls, wide::State w,
                                                                           ListOut o) {
    __shared__ unsigned int s_cnt;
    __shared__ unsigned long long s_at;
    wide::write(w, o, &s_cnt, &s_at, [&](uint32_t u) { return class_ok(g, u, cls); });
}

// ketogpu_subjects_ids_depth_wide / _page_wide: the level under a depth limit, and the paged
// finish's select and clear (wide.hpp "depth", "page")
__global__ __launch_bounds__(wide::kBlock) void subjects_wide_level_depth_kernel(Rows g, uint32_t cls, wide::State w,
                                                                                 unsigned long long lb,
                                                                                 unsigned long long le,
                                                                                 wide::Cut cut) {
    wide::level_depth(
        g, g.N, w, lb, le, cut, [&](uint32_t u) { return class_ok(g, u, cls); },
        [&](uint32_t u) { return any_class(g, u); });
}

__global__ __launch_bounds__(wide::kBlock) void subjects_wide_select_kernel(Rows g, uint32_t cls, wide::State w,
                                                                            const uint32_t *ovf_list, uint32_t first,
                                                                            const uint32_t *from, paged::PageOut o) {
    __shared__ uint32_t s_wave[wide::kBlock / 64];
    wide::page_select(w, ovf_list, first, from, o, s_wave, [&](uint32_t u) { return class_ok(g, u, cls); });
}

__global__ __launch_bounds__(wide::kBlock) void subjects_wide_clear_kernel(Rows g, uint32_t cls, wide::State w,
                                                                           const uint32_t *ovf_list, uint32_t first,
                                                                           const uint32_t *from) {
    __shared__ unsigned int s_cnt;
    wide::page_clear(w, ovf_list, first, from, &s_cnt, [&](uint32_t u) { return class_ok(g, u, cls); });
}

}  // namespace

struct ketogpu_subjects : ListHandle {
    uint32_t list_cap = kListCapDefault;  // tier 2: a seen list of list_cap per slot (d_aux)
    std::vector<uint64_t> h_off, h_end;   // upload staging
    std::vector<uint32_t> h_col;
    ketogpu_subjects_stats st{};
    ketogpu_combine_stats cst{};
    ketogpu_depth_stats dst{};
    ketogpu_via_stats vst{};
    ketogpu_expand_stats xst{};
    // expand calls: a bit per node whose query has a row with an unknown namespace
    // (node_row[v].first_bad >= 0).  It spans all N nodes, since a node whose rows are all bad
    // has no row here and still fails on the host.  The host keeps a mirror; the device array is
    // used only while some bit is set, so a snapshot without bad rows pays nothing
    std::vector<uint32_t> h_bad;
    DBuf<uint32_t> d_bad;
    bool has_bad = false;
    uint32_t bad_n = 0;  // the nodes the mirror covers
    // wide expand calls (expand_wide.hpp): the attention mask over d_col, as of rows_epoch
    // mask_epoch; the call's queue of copy items and its counters
    ketogpu_expand_wide_stats xwst{};
    DBuf<unsigned long long> d_xmask, d_xwctr;
    DBuf<expand::xwide::Item> d_xwq;
    uint64_t mask_epoch = ~0ull;
    uint64_t xwq_cap = expand::xwide::kQueueDefault;

    ketogpu_subjects() : ListHandle("subject listing") {}
    ~ketogpu_subjects() { d_bad.drop(), d_xmask.drop(), d_xwctr.drop(), d_xwq.drop(); }

    void push_bad() {
        has_bad = std::any_of(h_bad.begin(), h_bad.end(), [](uint32_t w) { return w != 0; });
        if (!has_bad) return;
        d_bad.need(h_bad.size());
        HIP_CHECK(hipMemcpyAsync(d_bad.p, h_bad.data(), h_bad.size() * 4, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }

    // v's bit from the snapshot's current rows -> it changed
    bool put_bad(const Snapshot &s, uint32_t v) {
        const uint32_t bit = 1u << (v & 31), want = s.node_row[v].first_bad >= 0 ? bit : 0;
        const bool changed = (h_bad[v >> 5] & bit) != want;
        h_bad[v >> 5] = (h_bad[v >> 5] & ~bit) | want;
        return changed;
    }

    void upload_bad(const Snapshot &s) {
        h_bad.assign(((size_t)std::max(s.N, s.n_cap) + 31) / 32 + 1, 0);
        for (uint32_t v = 0; v < s.N; v++) put_bad(s, v);
        bad_n = s.N;
        push_bad();
    }

    // what a patched refresh asks of the handle: the bits of the rows it rewrote and of new nodes
    void patched(const Snapshot &s) {
        bool changed = h_bad.size() < ((size_t)s.N + 31) / 32 + 1;  // (the device array must span N too)
        if (changed) h_bad.resize(((size_t)s.N + 31) / 32 + 1, 0);
        for (uint32_t v : patch_nodes)
            if (v < s.N) changed |= put_bad(s, v);
        for (uint32_t v = bad_n; v < s.N; v++) changed |= put_bad(s, v);
        bad_n = s.N;
        if (changed) push_bad();
    }

    // the rows and classes of the snapshot's current version (caller holds its shared lock):
    // the first `len` entries of every expandable node's row.  Packed back to back on a
    // snapshot that cannot change in place (and under KETOGPU_LIST_REFRESH=full).  On a writable
    // one every row gets the host's growth rule, room for len + len / 4 + 4 entries, in an
    // arena with `slack` free words behind the last row: a written row is patched where it
    // lies, or moved to the tail once it has outgrown its room (ListHandle::try_patch).  The
    // class array has room for the reserved ids.
    void upload(const Snapshot &s) {
        if (s.has_ambiguous) throw Error(KETOGPU_EINVAL, what + ": the snapshot has shared Subject.String() keys (R4)");
        auto classes = class_index_of(s);
        arena = s.writable && !refresh_full;
        h_off.assign((size_t)s.Nx + 1, 0);
        if (arena) {
            m_begin.resize(s.Nx), m_cap.resize(s.Nx), h_end.resize(s.Nx);
            for (uint32_t v = 0; v < s.Nx; v++) {
                const uint64_t len = s.node_row[v].len, cap = std::min<uint64_t>(len + len / 4 + 4, 0xffffffffu);
                m_begin[v] = h_off[v], m_cap[v] = (uint32_t)cap;
                h_end[v] = h_off[v] + len, h_off[v + 1] = h_off[v] + cap;
            }
        } else {
            for (uint32_t v = 0; v < s.Nx; v++) h_off[v + 1] = h_off[v] + s.node_row[v].len;
        }
        const uint64_t used = h_off[s.Nx];
        const uint64_t slack =
            !arena ? 0 : slack_knob != ~0ull ? slack_knob : std::max<uint64_t>(s.stats.num_edges / 8, 1u << 16);
        h_col.resize(used);
        for (uint32_t v = 0; v < s.Nx; v++)
            if (s.node_row[v].len) memcpy(h_col.data() + h_off[v], s.row_ptr(v), (size_t)s.node_row[v].len * 4);
        upload_rows(s, h_off.data(), arena ? h_end.data() : nullptr, h_off.size(), h_col.data(), h_col.size(),
                    used + slack, classes->node_class.data(), s.N, arena ? std::max(s.N, s.n_cap) : s.N, bound_of(s));
        arena_tail = used, arena_garbage = 0;
        std::vector<uint32_t>().swap(h_col);  // (the larger staging arrays are not kept between uploads)
        std::vector<uint64_t>().swap(h_end);
        upload_bad(s);
        st.uploads++;
    }

    // ---- what ListHandle::try_patch asks of a handle: the full forward rows the log names
    // (KETOGPU_PATCH_FORWARD_FULL) go into the arena; new subjects bring a class each and
    // raise the bound N
    static constexpr uint8_t kPatchKind = KETOGPU_PATCH_FORWARD_FULL;
    void host_row(const Snapshot &s, uint32_t v, const uint32_t *&p, uint64_t &len, uint64_t &at) const {
        at = 0, len = s.node_row[v].len, p = s.row_ptr(v);
    }
    const uint32_t *host_keys(const Snapshot &s) const { return class_index_of(s)->node_class.data(); }
    // the bitmaps span the bound; the kernels take the member bound itself, g.N, which the span
    // is never below.  With the arena the span is rounded up (ListHandle::bound_step)
    uint32_t bound_of(const Snapshot &s) const { return arena ? bound_above(s.N) : s.N; }
    void moved() {}

    uint64_t seen_words() const { return std::max<uint32_t>(list_cap, 1); }

    uint64_t slot_words() const {
        return std::max<uint64_t>(bm_words, 1) + std::max<uint32_t>(g.Ni, 1) + seen_words();
    }

    uint32_t alloc_slots(uint32_t wanted) { return ListHandle::need_slots(wanted, slot_words(), seen_words()); }

    uint32_t need_slots(uint32_t wanted) { return st.slots = alloc_slots(wanted); }

    // tier 2's state for a combined call (ListHandle::need_pair_slots): the handle's slots as
    // they are, seen lists included, since the plain calls share them
    uint32_t need_combine_slots(uint32_t wanted) {
        return cst.slots = need_pair_slots(wanted, slot_words(), [&](uint32_t k) { return alloc_slots(k); });
    }

    SOut subjects_out(uint64_t capacity) { return {list_out(capacity), d_ctr.p + 3, d_ctr.p + 4}; }

    void run(const uint32_t *roots, size_t n, uint32_t cls, uint32_t *out, uint64_t capacity, uint64_t *begin,
             uint64_t *count, uint64_t *needed) {
        count_finishes(run_cursor(
            st, roots, n, out, capacity, begin, count, needed,
            [&](size_t i) { return begin[i] == KETOGPU_LOOKUP_INVALID || roots[i] == NONE; },
            [&](unsigned int *ovf_count) {
                KLAUNCH(subjects_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, (uint32_t)n, cls,
                        force_tier2 ? 1 : 0, subjects_out(capacity), d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) { return need_slots(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(subjects_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, cls,
                        subjects_out(capacity), d_ovf.p, first, d_bm.p, bm_words, d_wl.p, d_aux.p, list_cap);
            }));
    }

    // ketogpu_subjects_ids_wide: run() with tier 1's overflows in rounds of the wide tier
    void run_ids_wide(const uint32_t *roots, size_t n, uint32_t cls, uint32_t *out, uint64_t capacity,
                      uint64_t *begin, uint64_t *count, uint64_t *needed) {
        ListHandle::run_wide(
            roots, n, out, capacity, begin, count, needed,
            [&](size_t i) { return begin[i] == KETOGPU_LOOKUP_INVALID || roots[i] == NONE; },
            [&](unsigned int *ovf_count) {
                KLAUNCH(subjects_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, (uint32_t)n, cls,
                        force_tier2 ? 1 : 0, subjects_out(capacity), d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) {
                return wst.slots = need_wide_slots(ovf, slot_words(), [&](uint32_t k) { return alloc_slots(k); });
            },
            [&](uint32_t first, uint32_t k) {
                wide_round(
                    first, k, g.Nx,
                    [&](const wide::State &w, uint32_t, unsigned long long lb, unsigned long long le) {
                        KLAUNCH(subjects_wide_level_kernel, dim3(wide::level_grid(le - lb)), dim3(wide::kBlock), 0,
                                stream, g, cls, w, lb, le);
                    },
                    [&](const wide::State &w) { wide_list_finish(w, first, cls, capacity); });
            });
    }

    // the wide tier's full-list finish: reserve, then the write kernel
    void wide_list_finish(const wide::State &w, uint32_t first, uint32_t cls, uint64_t capacity) {
        wide_reserve(w, first, capacity);
        KLAUNCH(subjects_wide_write_kernel, wide_write_grid(w.nslots), dim3(wide::kBlock), 0, stream, g, cls, w,
                list_out(capacity));
    }

    uint32_t need_wide_state(uint32_t wanted) {
        return wst.slots = need_wide_slots(wanted, slot_words(), [&](uint32_t k) { return alloc_slots(k); });
    }

    // a wide round's level launch under the limits d_depth (null: none)
    void wide_level_depth(const wide::State &w, uint32_t L, unsigned long long lb, unsigned long long le, uint32_t cls,
                          const uint32_t *d_depth, uint32_t first) {
        KLAUNCH(subjects_wide_level_depth_kernel, dim3(wide::level_grid(le - lb)), dim3(wide::kBlock), 0, stream, g,
                cls, w, lb, le, wide::Cut{L, d_depth, d_ovf.p, first, d_front.p});
    }

    // ketogpu_subjects_ids_depth_wide: run_depth() with tier 1's overflows in rounds of the wide
    // tier, counted in wst alone
    void run_depth_wide(const uint32_t *roots, const uint32_t *max_depth, size_t n, uint32_t cls, uint32_t *out,
                        uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *frontier, uint64_t *needed) {
        const uint32_t *d_depth = upload_depth(max_depth, n);
        ListHandle::run_wide(
            roots, n, out, capacity, begin, count, needed,
            [&](size_t i) { return begin[i] == KETOGPU_LOOKUP_INVALID || roots[i] == NONE; },
            [&](unsigned int *ovf_count) {
                KLAUNCH(subjects_depth_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_depth,
                        (uint32_t)n, cls, force_tier2 ? 1 : 0, subjects_out(capacity), d_front.p, d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) { return need_wide_state(ovf); },
            [&](uint32_t first, uint32_t k) {
                wide_round(
                    first, k, g.Nx,
                    [&](const wide::State &w, uint32_t L, unsigned long long lb, unsigned long long le) {
                        wide_level_depth(w, L, lb, le, cls, d_depth, first);
                    },
                    [&](const wide::State &w) { wide_list_finish(w, first, cls, capacity); });
            });
        read_frontier(frontier, n);
        wst.last_call_ms = ms_of_call();
    }

    // ketogpu_subjects_page_wide: run_page_depth() with tier 1's overflows in rounds of the wide
    // tier and the paged finish of wide.hpp, counted in wst alone
    void run_page_wide(const uint32_t *roots, const uint32_t *max_depth, const uint32_t *from, size_t n, uint32_t cls,
                       uint32_t limit, uint32_t *out, uint32_t *returned, uint64_t *count, uint64_t *remaining,
                       uint64_t *frontier) {
        const uint32_t *d_depth = upload_depth(max_depth, n);
        ListHandle::run_page_wide(
            roots, from, n, limit, out, returned, count, remaining,
            [&](unsigned int *ovf_count) {
                KLAUNCH(subjects_depth_page_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_depth,
                        d_from.p, (uint32_t)n, cls, force_tier2 ? 1 : 0, page_out(limit), d_front.p, d_ovf.p,
                        ovf_count);
            },
            [&](uint32_t ovf) { return need_wide_state(ovf); },
            [&](uint32_t first, uint32_t k) {
                wide_round(
                    first, k, g.Nx,
                    [&](const wide::State &w, uint32_t L, unsigned long long lb, unsigned long long le) {
                        wide_level_depth(w, L, lb, le, cls, d_depth, first);
                    },
                    [&](const wide::State &w) {
                        wide_page_finish(
                            w, first, limit,
                            [&](const wide::State &w) {
                                KLAUNCH(subjects_wide_select_kernel, dim3(k), dim3(wide::kBlock), 0, stream, g, cls, w,
                                        d_ovf.p, first, d_from.p, page_out(limit));
                            },
                            [&](const wide::State &w) {
                                KLAUNCH(subjects_wide_clear_kernel, wide_clear_grid(k), dim3(wide::kBlock), 0, stream,
                                        g, cls, w, d_ovf.p, first, d_from.p);
                            });
                    });
            });
        read_frontier(frontier, n);
        wst.last_call_ms = ms_of_call();
    }

    // the paged call: run() with the ordered finish
    void run_page(const uint32_t *roots, const uint32_t *from, size_t n, uint32_t cls, uint32_t limit, uint32_t *out,
                  uint32_t *returned, uint64_t *count, uint64_t *remaining) {
        count_finishes(ListHandle::run_page(
            st, roots, from, n, limit, out, returned, count, remaining,
            [&](unsigned int *ovf_count) {
                KLAUNCH(subjects_page_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_from.p,
                        (uint32_t)n, cls, force_tier2 ? 1 : 0, page_out(limit), d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) { return need_slots(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(subjects_page_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, d_from.p, cls,
                        page_out(limit), d_ctr.p + 3, d_ctr.p + 4, d_ovf.p, first, d_bm.p, bm_words, d_wl.p,
                        d_aux.p, list_cap);
            },
            [&](Tally &t) { read_ctrs(t); }));  // (the finish counters)
    }

    // a pair answered before any row was read: no side has one (an INVALID pair is counted by
    // its marker)
    bool no_row(uint32_t a, uint32_t b) const { return a >= g.Nx && b >= g.Nx; }

    // ketogpu_subjects_combine: run()'s output contract, one list per pair (a, b)
    void run_combine(const uint32_t *a, const uint32_t *b, size_t n, uint32_t op, uint32_t cls, uint32_t *out,
                     uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *needed) {
        run_cursor(
            cst, a, b, n, out, capacity, begin, count, needed,
            [&](size_t i) { return begin[i] == KETOGPU_LOOKUP_INVALID || no_row(a[i], b[i]); },
            [&](unsigned int *ovf_count) {
                KLAUNCH(subjects_combine_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_req2.p,
                        (uint32_t)n, op, cls, force_tier2 ? 1 : 0, list_out(capacity), d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) { return need_combine_slots(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(subjects_combine_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, d_req2.p, op,
                        cls, list_out(capacity), d_ovf.p, first, d_bm.p, d_bm2.p, bm_words, d_wl.p);
            });
        cst.last_call_ms = ms_of_call();
    }

    // ketogpu_subjects_combine_page: run_page()'s output contract, one page per pair (a, b)
    void run_combine_page(const uint32_t *a, const uint32_t *b, const uint32_t *from, size_t n, uint32_t op,
                          uint32_t cls, uint32_t limit, uint32_t *out, uint32_t *returned, uint64_t *count,
                          uint64_t *remaining) {
        ListHandle::run_page(
            cst, a, b, from, n, limit, out, returned, count, remaining, [&](size_t i) { return no_row(a[i], b[i]); },
            [&](unsigned int *ovf_count) {
                KLAUNCH(subjects_combine_page_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p,
                        d_req2.p, d_from.p, (uint32_t)n, op, cls, force_tier2 ? 1 : 0, page_out(limit), d_ovf.p,
                        ovf_count);
            },
            [&](uint32_t ovf) { return need_combine_slots(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(subjects_combine_page_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, d_req2.p,
                        d_from.p, op, cls, page_out(limit), d_ovf.p, first, d_bm.p, d_bm2.p, bm_words, d_wl.p);
            },
            [](Tally &) {});
        cst.last_call_ms = ms_of_call();
    }

    // ketogpu_subjects_ids_depth: run() with a limit per request (null: none) and the frontier
    void run_depth(const uint32_t *roots, const uint32_t *max_depth, size_t n, uint32_t cls, uint32_t *out,
                   uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *frontier, uint64_t *needed) {
        const uint32_t *d_depth = upload_depth(max_depth, n);
        count_depth_finishes(
            run_cursor(
                dst, roots, n, out, capacity, begin, count, needed,
                [&](size_t i) { return begin[i] == KETOGPU_LOOKUP_INVALID || roots[i] == NONE; },
                [&](unsigned int *ovf_count) {
                    KLAUNCH(subjects_depth_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_depth,
                            (uint32_t)n, cls, force_tier2 ? 1 : 0, subjects_out(capacity), d_front.p, d_ovf.p,
                            ovf_count);
                },
                [&](uint32_t ovf) { return dst.slots = alloc_slots(ovf); },
                [&](uint32_t first, uint32_t k) {
                    KLAUNCH(subjects_depth_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, d_depth, cls,
                            subjects_out(capacity), d_front.p, d_ovf.p, first, d_bm.p, bm_words, d_wl.p, d_aux.p,
                            list_cap);
                }),
            frontier, n);
    }

    // ketogpu_subjects_page_depth: run_page() with a limit per request and the frontier
    void run_page_depth(const uint32_t *roots, const uint32_t *max_depth, const uint32_t *from, size_t n, uint32_t cls,
                        uint32_t limit, uint32_t *out, uint32_t *returned, uint64_t *count, uint64_t *remaining,
                        uint64_t *frontier) {
        const uint32_t *d_depth = upload_depth(max_depth, n);
        count_depth_finishes(
            ListHandle::run_page(
                dst, roots, from, n, limit, out, returned, count, remaining,
                [&](unsigned int *ovf_count) {
                    KLAUNCH(subjects_depth_page_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p,
                            d_depth, d_from.p, (uint32_t)n, cls, force_tier2 ? 1 : 0, page_out(limit), d_front.p,
                            d_ovf.p, ovf_count);
                },
                [&](uint32_t ovf) { return dst.slots = alloc_slots(ovf); },
                [&](uint32_t first, uint32_t k) {
                    KLAUNCH(subjects_depth_page_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, d_depth,
                            d_from.p, cls, page_out(limit), d_front.p, d_ctr.p + 3, d_ctr.p + 4, d_ovf.p, first,
                            d_bm.p, bm_words, d_wl.p, d_aux.p, list_cap);
                },
                [&](Tally &t) { read_ctrs(t); }),  // (the finish counters)
            frontier, n);
    }

    // tier 2's state for a via call (ListHandle::need_via_slots): the handle's slots as they are,
    // seen lists included
    uint32_t need_via_state(uint32_t wanted) {
        return vst.slots = need_via_slots(wanted, slot_words(), [&](uint32_t k) { return alloc_slots(k); });
    }

    // ketogpu_subjects_ids_via: run_depth() with via and hops next to out
    void run_via(const uint32_t *roots, const uint32_t *max_depth, size_t n, uint32_t cls, uint32_t *out,
                 uint32_t *via, uint32_t *hops, uint64_t capacity, uint64_t *begin, uint64_t *count,
                 uint64_t *frontier, uint64_t *needed) {
        const uint32_t *d_depth = upload_depth(max_depth, n);
        const via::ViaOut vo = via_out(via, hops, capacity);
        const Tally t = run_cursor(
            vst, roots, n, nullptr, capacity, begin, count, needed,  // (the ids come back with via and hops)
            [&](size_t i) { return begin[i] == KETOGPU_LOOKUP_INVALID || roots[i] == NONE; },
            [&](unsigned int *ovf_count) {
                KLAUNCH(subjects_via_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_depth,
                        (uint32_t)n, cls, force_tier2 ? 1 : 0, list_out(capacity), vo, d_front.p, d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) { return need_via_state(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(subjects_via_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, d_depth, cls,
                        subjects_out(capacity), vo, d_front.p, d_ovf.p, first, d_bm.p, bm_words, d_wl.p, d_aux.p,
                        list_cap, d_viast.p);
            });
        read_via(out, via, hops, written_end(begin, count, n));
        count_via_finishes(t, frontier, n);
    }

    // ketogpu_subjects_page_via: run_page_depth() with via and hops at the stride of out
    void run_page_via(const uint32_t *roots, const uint32_t *max_depth, const uint32_t *from, size_t n, uint32_t cls,
                      uint32_t limit, uint32_t *out, uint32_t *via, uint32_t *hops, uint32_t *returned,
                      uint64_t *count, uint64_t *remaining, uint64_t *frontier) {
        const uint32_t *d_depth = upload_depth(max_depth, n);
        const via::ViaOut vo = via_out(via, hops, n * (uint64_t)limit);
        const Tally t = ListHandle::run_page(
            vst, roots, from, n, limit, out, returned, count, remaining,
            [&](unsigned int *ovf_count) {
                KLAUNCH(subjects_via_page_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_depth,
                        d_from.p, (uint32_t)n, cls, force_tier2 ? 1 : 0, page_out(limit), vo, d_front.p, d_ovf.p,
                        ovf_count);
            },
            [&](uint32_t ovf) { return need_via_state(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(subjects_via_page_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, d_depth,
                        d_from.p, cls, page_out(limit), vo, d_front.p, d_ctr.p + 3, d_ctr.p + 4, d_ovf.p, first,
                        d_bm.p, bm_words, d_wl.p, d_aux.p, list_cap, d_viast.p);
            },
            [&](Tally &t) { read_ctrs(t); });  // (the finish counters)
        read_via(nullptr, via, hops, n * (uint64_t)limit);
        count_via_finishes(t, frontier, n);
    }

    // tier 2's state for an expand call (ListHandle::need_expand_slots): the handle's slots as
    // they are, seen lists included
    uint32_t need_expand_state(uint32_t wanted) {
        return xst.slots = need_expand_slots(wanted, slot_words(), [&](uint32_t k) { return alloc_slots(k); });
    }

    // is the snapshot one with shared Subject.String() keys now?  (in-place writes can make it one)
    bool snapshot_ambiguous() {
        const Snapshot *sp;
        {
            std::lock_guard<std::mutex> lk(link->mu);
            sp = link->snap;
        }
        if (!sp) throw Error(KETOGPU_EINVAL, what + ": the snapshot was freed");
        std::shared_lock<std::shared_mutex> rd(sp->mu);
        return sp->has_ambiguous;
    }

    // ... then the visited map is not keyed by node: every request is the host's
    template <class Stats>
    void expand_all_host(Stats &xst, size_t n, uint64_t *begin, uint64_t *count, uint32_t *status, uint64_t *needed) {
        *needed = 0;
        for (size_t i = 0; i < n; i++) begin[i] = 0, count[i] = 0, status[i] = KETOGPU_EXPAND_HOST;
        xst.requests += n, xst.host_requests += n;
        xst.last_call_ms = ms_of_call();
    }

    // ketogpu_subjects_expand: run()'s output contract with two output arrays and a status
    void run_expand(const uint32_t *roots, const uint32_t *depths, size_t n, uint32_t *out_nodes,
                    uint32_t *out_children, uint64_t capacity, uint64_t *begin, uint64_t *count, uint32_t *status,
                    uint64_t *needed) {
        Tally t{};
        *needed = 0;
        xst.requests += n;
        if (!n) return;
        d_req.need(n), d_req2.need(n), d_ovf.need(n), d_begin.need(n), d_count.need(n), d_ret.need(n);
        d_ctr.need(kCtrs), d_out.need(capacity), d_via.need(capacity);
        HIP_CHECK(hipMemcpyAsync(d_req.p, roots, n * 4, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_req2.p, depths, n * 4, hipMemcpyHostToDevice, stream));
        const expand::Graph x{g, has_bad ? d_bad.p : nullptr};
        const expand::TreeOut o{list_out(capacity), d_via.p, d_ret.p};
        run_tiers(
            xst, t,
            [&](unsigned int *ovf_count) {
                KLAUNCH(subjects_expand_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, x, d_req.p, d_req2.p,
                        (uint32_t)n, force_tier2 ? 1 : 0, o, d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) { return need_expand_state(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(subjects_expand_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, x, d_req.p, d_req2.p, o,
                        d_ovf.p, first, d_bm.p, bm_words, d_aux.p, list_cap, d_xstack.p, expand_stack_words);
            },
            [&](Tally &t) { read_ctrs(t); });  // (the cursor has moved)
        HIP_CHECK(hipMemcpyAsync(begin, d_begin.p, n * 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(count, d_count.p, n * 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(status, d_ret.p, n * 4, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        // (the written trees tile a prefix of both arrays: no word outside a written tree is touched)
        const uint64_t written = std::min<uint64_t>(written_end(begin, count, n), capacity);
        if (written && out_nodes) {
            HIP_CHECK(hipMemcpyAsync(out_nodes, d_out.p, written * 4, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(out_children, d_via.p, written * 4, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
        }
        *needed = t.ctr[0];
        uint64_t unlisted = 0;
        for (size_t i = 0; i < n; i++) {
            unlisted += begin[i] == KETOGPU_LOOKUP_INVALID || roots[i] == NONE;
            xst.host_requests += status[i] == KETOGPU_EXPAND_HOST;
        }
        xst.tier2_requests += t.ovf;
        xst.tier1_requests += n - t.ovf - unlisted;
        xst.nodes_produced += t.ctr[0];
        xst.truncated_trees += t.ctr[1];
        xst.last_call_ms = ms_of_call();
    }

    // the attention mask of the rows as they are now (expand_wide.hpp "mask"): rebuilt in full
    // when an upload or a patched refresh has moved rows_epoch, which covers col, off / end,
    // N / Nx and the bad-row bitmap; a call behind which nothing changed builds nothing.  A full
    // rebuild is one pass over col: patching the mask would have to find every occurrence of a
    // node whose row became empty or non-empty, which is a pass over col too
    const unsigned long long *need_expand_mask(const expand::Graph &x) {
        if (mask_epoch == rows_epoch && d_xmask.p) return d_xmask.p;
        const uint64_t words = (col_words + 63) / 64;
        d_xmask.need(words);
        HIP_CHECK(hipStreamSynchronize(stream));  // (the refresh's copies and patch kernel: not the mask's time)
        const auto m0 = std::chrono::steady_clock::now();
        if (words) {
            const uint64_t groups = (words + expand::xwide::kMaskBlock / 64 - 1) / (expand::xwide::kMaskBlock / 64);
            KLAUNCH(subjects_expand_mask_kernel, dim3((unsigned)std::min<uint64_t>(groups, expand::xwide::kMaskGridMax)),
                    dim3(expand::xwide::kMaskBlock), 0, stream, x, col_words, d_xmask.p, words);
            HIP_CHECK(hipStreamSynchronize(stream));
        }
        xwst.last_mask_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - m0).count();
        xwst.mask_builds++, xwst.mask_words = words;
        mask_epoch = rows_epoch;
        return d_xmask.p;
    }

    // ketogpu_subjects_expand_wide: run_expand() with the wide walk in tier 1's place and the
    // fill kernel right behind it, counted in xwst alone
    void run_expand_wide(const uint32_t *roots, const uint32_t *depths, size_t n, uint32_t *out_nodes,
                         uint32_t *out_children, uint64_t capacity, uint64_t *begin, uint64_t *count,
                         uint32_t *status, uint64_t *needed) {
        namespace xw = expand::xwide;
        Tally t{};
        *needed = 0;
        xwst.requests += n;
        if (!n) return;
        d_req.need(n), d_req2.need(n), d_ovf.need(n), d_begin.need(n), d_count.need(n), d_ret.need(n);
        d_ctr.need(kCtrs), d_out.need(capacity), d_via.need(capacity);
        d_xwq.need(xwq_cap), d_xwctr.need(xw::kCtrWords);
        const expand::Graph x{g, has_bad ? d_bad.p : nullptr};
        const unsigned long long *mask = need_expand_mask(x);
        HIP_CHECK(hipMemcpyAsync(d_req.p, roots, n * 4, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_req2.p, depths, n * 4, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemsetAsync(d_xwctr.p, 0, xw::kCtrWords * 8, stream));
        const expand::TreeOut o{list_out(capacity), d_via.p, d_ret.p};
        const xw::Queue q{d_xwq.p, xwq_cap, d_xwctr.p};
        run_tiers(
            xwst, t,
            [&](unsigned int *ovf_count) {
                KLAUNCH(subjects_expand_wide_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, x, mask, q, d_req.p,
                        d_req2.p, (uint32_t)n, force_tier2 ? 1 : 0, o, d_ovf.p, ovf_count);
                if (capacity && !force_tier2)  // (a count-only call queues nothing)
                    KLAUNCH(subjects_expand_fill_kernel, dim3(xw::kFillGrid), dim3(xw::kFillBlock), 0, stream, x, q, o);
            },
            [&](uint32_t ovf) {
                return xwst.slots = need_expand_slots(ovf, slot_words(), [&](uint32_t k) { return alloc_slots(k); });
            },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(subjects_expand_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, x, d_req.p, d_req2.p, o,
                        d_ovf.p, first, d_bm.p, bm_words, d_aux.p, list_cap, d_xstack.p, expand_stack_words);
            },
            [&](Tally &t) { read_ctrs(t); });  // (the cursor has moved)
        unsigned long long c[xw::kCtrWords];
        HIP_CHECK(hipMemcpyAsync(begin, d_begin.p, n * 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(count, d_count.p, n * 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(status, d_ret.p, n * 4, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(c, d_xwctr.p, sizeof c, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        // (the written trees tile a prefix of both arrays: no word outside a written tree is touched)
        const uint64_t written = std::min<uint64_t>(written_end(begin, count, n), capacity);
        if (written && out_nodes) {
            HIP_CHECK(hipMemcpyAsync(out_nodes, d_out.p, written * 4, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(out_children, d_via.p, written * 4, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
        }
        *needed = t.ctr[0];
        uint64_t unlisted = 0;
        for (size_t i = 0; i < n; i++) {
            unlisted += begin[i] == KETOGPU_LOOKUP_INVALID || roots[i] == NONE;
            xwst.host_requests += status[i] == KETOGPU_EXPAND_HOST;
        }
        xwst.tier2_requests += t.ovf;
        xwst.tier1_requests += n - t.ovf - unlisted;
        xwst.nodes_produced += t.ctr[0];
        xwst.truncated_trees += t.ctr[1];
        xwst.run_steps += c[xw::kRunSteps], xwst.skipped_entries += c[xw::kSkipped];
        xwst.runs_queued += c[xw::kRunsQueued], xwst.items_queued += c[xw::kItemsQueued];
        xwst.runs_self_copied += c[xw::kRunsSelf], xwst.runs_queue_full += c[xw::kRunsFull];
        xwst.last_call_ms = ms_of_call();
    }

    void count_via_finishes(const Tally &t, uint64_t *frontier, size_t n) {
        vst.list_finishes += t.ctr[3];
        vst.scan_finishes += t.ctr[4];
        vst.cut_requests += read_frontier(frontier, n);
        vst.last_call_ms = ms_of_call();
    }

    void count_depth_finishes(const Tally &t, uint64_t *frontier, size_t n) {
        dst.list_finishes += t.ctr[3];
        dst.scan_finishes += t.ctr[4];
        dst.cut_requests += read_frontier(frontier, n);
        dst.last_call_ms = ms_of_call();
    }

    void count_finishes(const Tally &t) {
        st.list_finishes += t.ctr[3];
        st.scan_finishes += t.ctr[4];
        st.last_call_ms = ms_of_call();
    }
};

extern "C" {

int ketogpu_subjects_new(const ketogpu_snapshot *sp, const ketogpu_subjects_opts *opts, ketogpu_subjects **out) {
    return list_new(sp, opts, out, "KETOGPU_SUBJECTS_TIER", "KETOGPU_SUBJECTS_SLOTS", [](ketogpu_subjects &h) {
        if (const char *e = getenv("KETOGPU_SUBJECTS_LIST_CAP"))
            h.list_cap = (uint32_t)std::min<long long>(std::max<long long>(atoll(e), 0), 1ll << 28);
        h.st.set_capacity = kSetCap;
        h.st.list_capacity = h.list_cap;
        if (const char *e = getenv("KETOGPU_EXPAND_WIDE_QUEUE"))
            h.xwq_cap = (uint64_t)std::min<long long>(std::max<long long>(atoll(e), 1), 1ll << 26);
        h.xwst.queue_capacity = h.xwq_cap;
        h.xwst.chunk = wide::kChunk;
    });
}

void ketogpu_subjects_free(ketogpu_subjects *h) { delete h; }

int ketogpu_subjects_stats_get(const ketogpu_subjects *h, ketogpu_subjects_stats *out) {
    return list_stats_get(h, &ketogpu_subjects::st, out);
}

int ketogpu_subjects_refresh_stats_get(const ketogpu_subjects *h, ketogpu_list_refresh_stats *out) {
    return list_stats_get<ListHandle>(h, &ListHandle::rst, out);
}

int ketogpu_subjects_ids(ketogpu_subjects *h, const uint32_t *roots, size_t n, uint32_t cls, uint32_t *out,
                         uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *needed) {
    return list_call(h, !needed || (n && (!roots || !begin || !count)) || (capacity && !out), n, "roots", nullptr,
                     [&] { h->run(roots, n, cls, out, capacity, begin, count, needed); });
}

int ketogpu_subjects_wide_stats_get(const ketogpu_subjects *h, ketogpu_wide_stats *out) {
    return list_stats_get<ListHandle>(h, &ListHandle::wst, out);
}

int ketogpu_subjects_ids_wide(ketogpu_subjects *h, const uint32_t *roots, size_t n, uint32_t cls, uint32_t *out,
                              uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *needed) {
    return list_call(h, !needed || (n && (!roots || !begin || !count)) || (capacity && !out), n, "roots", nullptr,
                     [&] { h->run_ids_wide(roots, n, cls, out, capacity, begin, count, needed); });
}

int ketogpu_subjects_ids_depth_wide(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *max_depth, size_t n,
                                    uint32_t cls, uint32_t *out, uint64_t capacity, uint64_t *begin, uint64_t *count,
                                    uint64_t *frontier, uint64_t *needed) {
    return list_call(h, !needed || (n && (!roots || !begin || !count)) || (capacity && !out), n, "roots", nullptr, [&] {
        h->run_depth_wide(roots, max_depth, n, cls, out, capacity, begin, count, frontier, needed);
    });
}

int ketogpu_subjects_page_wide(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *max_depth,
                               const uint32_t *from, size_t n, uint32_t cls, uint32_t limit, uint32_t *out,
                               uint32_t *returned, uint64_t *count, uint64_t *remaining, uint64_t *frontier) {
    return list_call(h, n && (!roots || !out || !returned || !count || !remaining), n, "roots", &limit, [&] {
        h->run_page_wide(roots, max_depth, from, n, cls, limit, out, returned, count, remaining, frontier);
    });
}

uint32_t ketogpu_wide_clear_tile_ids(void) { return wide::kClearTile * 32u; }

int ketogpu_subjects_page(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *from, size_t n, uint32_t cls,
                          uint32_t limit, uint32_t *out, uint32_t *returned, uint64_t *count, uint64_t *remaining) {
    return list_call(h, n && (!roots || !out || !returned || !count || !remaining), n, "roots", &limit,
                     [&] { h->run_page(roots, from, n, cls, limit, out, returned, count, remaining); });
}

int ketogpu_subjects_combine_stats_get(const ketogpu_subjects *h, ketogpu_combine_stats *out) {
    return list_stats_get(h, &ketogpu_subjects::cst, out);
}

int ketogpu_subjects_combine(ketogpu_subjects *h, const uint32_t *a, const uint32_t *b, size_t n, uint32_t op,
                             uint32_t cls, uint32_t *out, uint64_t capacity, uint64_t *begin, uint64_t *count,
                             uint64_t *needed) {
    if (h && op > KETOGPU_COMBINE_OR) return einval(h->what + ": an unknown combine operator");
    return list_call(h, !needed || (n && (!a || !b || !begin || !count)) || (capacity && !out), n, "pairs", nullptr,
                     [&] { h->run_combine(a, b, n, op, cls, out, capacity, begin, count, needed); });
}

int ketogpu_subjects_combine_page(ketogpu_subjects *h, const uint32_t *a, const uint32_t *b, const uint32_t *from,
                                  size_t n, uint32_t op, uint32_t cls, uint32_t limit, uint32_t *out,
                                  uint32_t *returned, uint64_t *count, uint64_t *remaining) {
    if (h && op > KETOGPU_COMBINE_OR) return einval(h->what + ": an unknown combine operator");
    return list_call(h, n && (!a || !b || !out || !returned || !count || !remaining), n, "pairs", &limit, [&] {
        h->run_combine_page(a, b, from, n, op, cls, limit, out, returned, count, remaining);
    });
}

int ketogpu_subjects_depth_stats_get(const ketogpu_subjects *h, ketogpu_depth_stats *out) {
    return list_stats_get(h, &ketogpu_subjects::dst, out);
}

int ketogpu_subjects_ids_depth(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *max_depth, size_t n,
                               uint32_t cls, uint32_t *out, uint64_t capacity, uint64_t *begin, uint64_t *count,
                               uint64_t *frontier, uint64_t *needed) {
    return list_call(h, !needed || (n && (!roots || !begin || !count)) || (capacity && !out), n, "roots", nullptr,
                     [&] { h->run_depth(roots, max_depth, n, cls, out, capacity, begin, count, frontier, needed); });
}

int ketogpu_subjects_page_depth(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *max_depth,
                                const uint32_t *from, size_t n, uint32_t cls, uint32_t limit, uint32_t *out,
                                uint32_t *returned, uint64_t *count, uint64_t *remaining, uint64_t *frontier) {
    return list_call(h, n && (!roots || !out || !returned || !count || !remaining), n, "roots", &limit, [&] {
        h->run_page_depth(roots, max_depth, from, n, cls, limit, out, returned, count, remaining, frontier);
    });
}

int ketogpu_subjects_via_stats_get(const ketogpu_subjects *h, ketogpu_via_stats *out) {
    return list_stats_get(h, &ketogpu_subjects::vst, out);
}

int ketogpu_subjects_ids_via(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *max_depth, size_t n,
                             uint32_t cls, uint32_t *out, uint32_t *via, uint32_t *hops, uint64_t capacity,
                             uint64_t *begin, uint64_t *count, uint64_t *frontier, uint64_t *needed) {
    return list_call(h, !needed || (n && (!roots || !begin || !count)) || (capacity && !out), n, "roots", nullptr,
                     [&] {
                         h->run_via(roots, max_depth, n, cls, out, capacity ? via : nullptr,
                                    capacity ? hops : nullptr, capacity, begin, count, frontier, needed);
                     });
}

int ketogpu_subjects_page_via(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *max_depth,
                              const uint32_t *from, size_t n, uint32_t cls, uint32_t limit, uint32_t *out,
                              uint32_t *via, uint32_t *hops, uint32_t *returned, uint64_t *count, uint64_t *remaining,
                              uint64_t *frontier) {
    return list_call(h, n && (!roots || !out || !returned || !count || !remaining), n, "roots", &limit, [&] {
        h->run_page_via(roots, max_depth, from, n, cls, limit, out, via, hops, returned, count, remaining, frontier);
    });
}

int ketogpu_subjects_expand_stats_get(const ketogpu_subjects *h, ketogpu_expand_stats *out) {
    return list_stats_get(h, &ketogpu_subjects::xst, out);
}

int ketogpu_subjects_expand(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *rest_depth, size_t n,
                            uint32_t *out_nodes, uint32_t *out_children, uint64_t capacity, uint64_t *begin,
                            uint64_t *count, uint32_t *status, uint64_t *needed) {
    if (!h || !needed || (n && (!roots || !rest_depth || !begin || !count || !status)) ||
        (capacity && (!out_nodes || !out_children)))
        return einval("null argument");
    if (n >= (1ull << 31)) return einval(h->what + ": more than 2^31 - 1 roots in one call");
    return guarded([&] {
        std::lock_guard<std::mutex> lk(h->mu);
        h->t0 = std::chrono::steady_clock::now();
        HIP_CHECK(hipSetDevice(h->device));
        if (h->snapshot_ambiguous()) return h->expand_all_host(h->xst, n, begin, count, status, needed);
        h->refresh(*h);
        h->run_expand(roots, rest_depth, n, out_nodes, out_children, capacity, begin, count, status, needed);
    });
}

int ketogpu_subjects_expand_wide_stats_get(const ketogpu_subjects *h, ketogpu_expand_wide_stats *out) {
    return list_stats_get(h, &ketogpu_subjects::xwst, out);
}

int ketogpu_subjects_expand_wide(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *rest_depth, size_t n,
                                 uint32_t *out_nodes, uint32_t *out_children, uint64_t capacity, uint64_t *begin,
                                 uint64_t *count, uint32_t *status, uint64_t *needed) {
    if (!h || !needed || (n && (!roots || !rest_depth || !begin || !count || !status)) ||
        (capacity && (!out_nodes || !out_children)))
        return einval("null argument");
    if (n >= (1ull << 31)) return einval(h->what + ": more than 2^31 - 1 roots in one call");
    return guarded([&] {
        std::lock_guard<std::mutex> lk(h->mu);
        h->t0 = std::chrono::steady_clock::now();
        HIP_CHECK(hipSetDevice(h->device));
        if (h->snapshot_ambiguous()) return h->expand_all_host(h->xwst, n, begin, count, status, needed);
        h->refresh(*h);
        h->run_expand_wide(roots, rest_depth, n, out_nodes, out_children, capacity, begin, count, status, needed);
    });
}

}  // extern "C"

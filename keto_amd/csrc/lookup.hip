// lookup.hip — reverse lookup on the device (include/ketogpu.h ketogpu_lookup_*).
//
// lookup(t, T) lists B(t), the expandable nodes that reach t in >= 1 edge, restricted to the
// object type T: the least set that holds rev(t) and rev(x) for every x in it (DESIGN.md
// "Reverse lookup").  The closure, its two tiers and the list finishes are closure.hpp's, over
// the reverse rows with the member bound num_expandable; the host side of the handle is
// hip_host.hpp's ListHandle.  What is here: the type filter, the classification of a target,
// the kernels as bodies over the shared pieces, the upload and the statistics.
//
//   tier 1  one wave per request, the closure in an LDS set.  A request whose set passes
//           kSetCap is appended to the overflow list and leaves no output.
//   tier 2  one workgroup per overflow request, `slots` requests per launch.  Each slot has a
//           bitmap over the expandable nodes and a worklist of Ni entries in global memory.
//
// The full-list call (ketogpu_lookup_ids) ends both tiers with the cursor finish.  The paged
// call (ketogpu_lookup_page) runs the same two closures and ends with the ordered finish of
// paged_finish.hpp instead: the `limit` smallest members >= from[i] to the stride
// out + i * limit, ascending, with the exact count and what remains; no cursor, no truncation.
//
// The path call (ketogpu_lookup_paths) searches in the same order (path_tier1_kernel,
// path_tier2_kernel below): every first visit records its parent, and the search ends when
// the root is visited.
//
// The depth calls (ketogpu_lookup_ids_depth / _page_depth) list the members within max_depth[i]
// hops of the target: the full-list and the paged kernels with depth.hpp's level bookkeeping in
// the closures and frontier[i], the interior members the limit left unread, next to the count.
//
// The via calls (ketogpu_lookup_ids_via / _page_via) are the depth calls with, next to every
// member, the node whose row granted it and its hop count: via.hpp's bodies, which keep a parent
// and a level per first visit.
//
// The wide call (ketogpu_lookup_ids_wide) is the full-list call with tier 1's overflows run by
// wide.hpp's level-synchronous tier, spread over the whole device, instead of tier 2.  The wide
// depth and paged calls (ketogpu_lookup_ids_depth_wide / _page_wide) are the depth calls with the
// same replacement: level L of the wide tier is its launch L, and the paged finish is wide.hpp's
// select, clear and report.
//
// Every index is validated before it is used: targets against num_nodes before rev_off is
// touched, row entries against num_expandable before the type array or a bitmap is.
#include <hip/hip_runtime.h>

#include "combine.hpp"
#include "depth.hpp"
#include "hip_host.hpp"
#include "lookup.hpp"
#include "via.hpp"

using namespace ketogpu;
using namespace ketogpu::closure;

namespace {

// The graph g of every kernel: rev_off (N + 1 offsets; a writable snapshot: n_cap + 1), rev_col,
// the object type of each of the Nx expandable nodes as the filter key, and the bound Nx.
__device__ inline bool type_ok(const Rows &g, uint32_t u, uint32_t want) {
    if (u >= g.Nx) return false;
    const uint32_t ty = g.filter_key[u];
    return want == KETOGPU_TYPE_ANY ? ty != KETOGPU_TYPE_NONE : (want != KETOGPU_TYPE_NONE && ty == want);
}

// ---------------------------------------------------------------------- full lists
__global__ __launch_bounds__(64) void lookup_tier1_kernel(Rows g, const uint32_t *targets, uint32_t n, uint32_t type,
                                                          int force_tier2, ListOut o, uint32_t *ovf_list,
                                                          unsigned int *ovf_count) {
    __shared__ uint32_t set[kSlotsLds];
    __shared__ uint32_t work[kSetCap + 64];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const uint32_t t = targets[i];
    if (t >= g.N) {  // NONE: the empty list; any other id outside the snapshot: INVALID
        if (lane == 0) {
            o.begin[i] = t == KETOGPU_NODE_NONE ? 0ull : KETOGPU_LOOKUP_INVALID;
            o.count[i] = 0;
        }
        return;
    }
    if (force_tier2) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    const bool over = !tier1_closure(g, g.Nx, t, lane, set, work);
    if (over) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    tier1_finish(set, lane, i, o, [&](uint32_t u) { return type_ok(g, u, type); });
}

// Block s of round r serves overflow request ovf_list[first + s] with slot s's state.  The
// bitmap is all zero on entry and is cleared again on the way out.
__global__ __launch_bounds__(kT2Block) void lookup_tier2_kernel(Rows g, const uint32_t *targets, uint32_t type,
                                                                ListOut o, const uint32_t *ovf_list, uint32_t first,
                                                                uint32_t *bitmaps, uint64_t bm_words, uint32_t *worklists) {
    __shared__ unsigned int s_tail, s_cnt, s_pos;
    __shared__ unsigned long long s_base;
    const uint32_t i = ovf_list[first + blockIdx.x];
    const uint32_t t = targets[i];
    uint32_t *bm = bitmaps + (uint64_t)blockIdx.x * bm_words;
    uint32_t *wl = worklists + (uint64_t)blockIdx.x * g.Ni;
    if (threadIdx.x == 0) s_tail = 0, s_cnt = 0, s_pos = 0;
    __syncthreads();
    if (t >= g.N) return;  // (tier 1 lists valid targets only)
    tier2_closure(g, g.Nx, t, bm, wl, &s_tail, [](uint32_t, uint32_t) {}, [] { return false; });
    auto ok = [&](uint32_t u) { return type_ok(g, u, type); };
    const unsigned long long base = reserve_block(o, i, scan_count(bm, bm_words, ok), &s_cnt, &s_base);
    scan_write(bm, bm_words, base, o.out, ok, &s_pos);
}

// ---------------------------------------------------------------------- paged finish
// The same closures with the ordered finish of paged_finish.hpp: request i reports count,
// remaining and returned, and writes its page to the stride out + i * limit.
__global__ __launch_bounds__(64) void lookup_page_tier1_kernel(Rows g, const uint32_t *targets, const uint32_t *from,
                                                               uint32_t n, uint32_t type, int force_tier2,
                                                               paged::PageOut o, uint32_t *ovf_list,
                                                               unsigned int *ovf_count) {
    __shared__ uint32_t set[kSlotsLds];
    __shared__ uint32_t work[kSetCap + 64];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const uint32_t t = targets[i];
    if (t >= g.N) {  // NONE: the empty page; any other id outside the snapshot: INVALID
        if (lane == 0) paged::page_invalid(o, i, t != KETOGPU_NODE_NONE);
        return;
    }
    if (force_tier2 || !tier1_closure(g, g.Nx, t, lane, set, work)) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    paged::page_finish_wave(set, kSlotsLds, lane, i, from[i], o, [&](uint32_t u) { return type_ok(g, u, type); });
}

// Selection in id order first, then one scan that counts and clears: the slot is left all zero
// for whichever kernel of the handle uses it next.
__global__ __launch_bounds__(kT2Block) void lookup_page_tier2_kernel(Rows g, const uint32_t *targets,
                                                                     const uint32_t *from, uint32_t type,
                                                                     paged::PageOut o, const uint32_t *ovf_list,
                                                                     uint32_t first, uint32_t *bitmaps,
                                                                     uint64_t bm_words, uint32_t *worklists) {
    __shared__ unsigned int s_tail, s_cnt, s_rem;
    __shared__ uint32_t s_wave[kT2Block / 64];
    const uint32_t i = ovf_list[first + blockIdx.x];
    const uint32_t t = targets[i];
    uint32_t *bm = bitmaps + (uint64_t)blockIdx.x * bm_words;
    uint32_t *wl = worklists + (uint64_t)blockIdx.x * g.Ni;
    if (threadIdx.x == 0) s_tail = 0, s_cnt = 0, s_rem = 0;
    __syncthreads();
    if (t >= g.N) return;  // (tier 1 lists valid targets only)
    tier2_closure(g, g.Nx, t, bm, wl, &s_tail, [](uint32_t, uint32_t) {}, [] { return false; });
    const uint32_t lo = from[i];
    auto ok = [&](uint32_t u) { return type_ok(g, u, type); };
    paged::page_select_block(bm, bm_words, lo, o.limit, o.out + (uint64_t)i * o.limit, s_wave, ok);
    __syncthreads();  // the selection has read the bitmap
    page_report(o, i, page_count_clear(bm, bm_words, lo, ok), &s_cnt, &s_rem);
}

// ---------------------------------------------------------------------- shortest path
// ketogpu_lookup_paths: one path r = v0, ..., vk = t with the fewest hops, v(i) in rev(v(i+1)).
// Both closures visit in level order (tier 1 works its rows first in, first out; tier 2 runs
// level by level between barriers), so the search below is theirs with two additions: each
// first visit records the node whose row it was found in, and the search stops once r is seen.
// The first visit of r then lies on a shortest path, and walking the recorded parents from r
// leads to t.  Only the target's own row records t as a parent: whatever a later expansion of
// t (t on a cycle) finds was seen in that first row already, so the walk ends at the first t.
constexpr uint16_t kParTarget = 0xFFFFu;  // tier 1's parent word: seen in the target's own row
static_assert(kSlotsLds <= kParTarget, "a slot index fits a parent word");

// r and t as ketogpu_lookup_paths classifies them before any row is read
__device__ inline bool path_trivial(const Rows &g, uint32_t r, uint32_t t, uint32_t i, uint32_t lane, const ListOut &o) {
    const bool bad = (r >= g.N && r != KETOGPU_NODE_NONE) || (t >= g.N && t != KETOGPU_NODE_NONE);
    if (!bad && r < g.Nx && t < g.N) return false;
    if (lane == 0) {  // an id outside the snapshot: INVALID; NONE or a never-expanded root: denied
        o.begin[i] = bad ? KETOGPU_LOOKUP_INVALID : 0ull;
        o.count[i] = 0;
    }
    return true;
}

// one thread: reserve `cnt` ids for path i -> where to write it, or TRUNCATED.  A denied pair
// reserves nothing and reports begin = 0.
__device__ inline unsigned long long path_reserve(const ListOut &o, uint32_t i, uint32_t cnt) {
    if (cnt) return reserve(o, i, cnt);
    o.count[i] = 0;
    o.begin[i] = 0;
    return KETOGPU_LOOKUP_TRUNCATED;
}

// tier 1: tier1_closure's set and worklist with a loop of its own: a parent word per slot (the
// slot of the node whose row the member was first seen in, or kParTarget), and the worklist
// holds slots, so the row at hand knows its own.  A ballot on u == r after every 64-entry step
// ends the search.
__global__ __launch_bounds__(64) void path_tier1_kernel(Rows g, const uint32_t *roots, const uint32_t *targets,
                                                        uint32_t n, int force_tier2, ListOut o, uint32_t *ovf_list,
                                                        unsigned int *ovf_count) {
    __shared__ uint32_t set[kSlotsLds];
    __shared__ uint16_t par[kSlotsLds];
    __shared__ uint16_t work[kSetCap + 64];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const uint32_t r = roots[i], t = targets[i];
    if (path_trivial(g, r, t, i, lane, o)) return;
    if (force_tier2) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    for (uint32_t s = lane; s < kSlotsLds; s += 64) set[s] = kEmpty;
    __syncthreads();
    uint32_t size = 0, head = 0, tail = 0, hit_slot = 0;  // wave-uniform
    bool over = false, hit = false;
    uint32_t v = t, pv = kParTarget;
    for (;;) {
        uint64_t b, e;
        row_bounds(g, v, b, e);
        for (uint64_t base = b; base < e && !over && !hit; base += 64) {
            const uint64_t j = base + lane;
            const uint32_t u = j < e ? g.col[j] : kEmpty;
            bool fresh = false;
            uint32_t s = 0;
            if (u < g.Nx) fresh = set_insert(set, u, s);  // (also drops kEmpty)
            if (fresh) par[s] = (uint16_t)pv;  // the winner of the compare-and-swap: the first visit
            const unsigned long long mf = __ballot(fresh), mi = __ballot(fresh && u < g.Ni);
            if (fresh && u < g.Ni) work[tail + __popcll(mi & ((1ull << lane) - 1))] = (uint16_t)s;
            tail += __popcll(mi);
            size += __popcll(mf);
            const unsigned long long mh = __ballot(u == r);  // (r < Nx: never kEmpty)
            if (mh) {
                hit = true;
                hit_slot = __shfl(s, __ffsll(mh) - 1);
            }
            over = size > kSetCap;  // a hit in the same step still finishes here
        }
        __syncthreads();  // the worklist entries and parent words of this row are visible to every lane
        if (hit || over || head == tail) break;
        pv = work[head++];
        v = set[pv];
    }
    if (!hit && over) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    if (lane != 0) return;
    uint32_t cnt = 0;  // nodes on the path: the members from r down to the target's row, and t
    if (hit) {
        cnt = 2;
        for (uint32_t s = hit_slot; par[s] != kParTarget; s = par[s]) cnt++;
    }
    const unsigned long long base = path_reserve(o, i, cnt);
    if (base == KETOGPU_LOOKUP_TRUNCATED) return;
    uint32_t k = 0;
    for (uint32_t s = hit_slot;; s = par[s]) {
        o.out[base + k++] = set[s];
        if (par[s] == kParTarget) break;
    }
    o.out[base + k] = t;
}

// tier 2: lookup_tier2_kernel's slot state plus a parent array of Nx words.  A parent word is
// valid exactly where the bitmap bit is set (written by the winner of the atomicOr), so the
// array is never cleared.  The bitmap is all zero on entry and is cleared again on the way out.
__global__ __launch_bounds__(kT2Block) void path_tier2_kernel(Rows g, const uint32_t *roots, const uint32_t *targets,
                                                              ListOut o, const uint32_t *ovf_list, uint32_t first,
                                                              uint32_t *bitmaps, uint64_t bm_words, uint32_t *worklists,
                                                              uint32_t *parents) {
    __shared__ unsigned int s_tail, s_hit;
    const uint32_t i = ovf_list[first + blockIdx.x];
    const uint32_t r = roots[i], t = targets[i];
    uint32_t *bm = bitmaps + (uint64_t)blockIdx.x * bm_words;
    uint32_t *wl = worklists + (uint64_t)blockIdx.x * g.Ni;
    uint32_t *par = parents + (uint64_t)blockIdx.x * g.Nx;
    const unsigned tid = threadIdx.x;
    if (tid == 0) s_tail = 0, s_hit = 0;
    __syncthreads();
    if (t >= g.N || r >= g.Nx) return;  // (tier 1 lists pairs that need a search only)
    tier2_closure(
        g, g.Nx, t, bm, wl, &s_tail,
        [&](uint32_t u, uint32_t v) {
            par[u] = v;
            if (u == r) s_hit = 1;
        },
        [&] { return s_hit != 0; });  // (behind a level's barrier: its parent words are visible)
    if (tid == 0) {  // the chain r -> ... -> t: every node on it but t has its bit set
        uint32_t cnt = 0;
        if (s_hit) {
            uint32_t x = r;
            cnt = 1;
            do {
                x = par[x];
                cnt++;
            } while (x != t);
        }
        const unsigned long long base = path_reserve(o, i, cnt);
        if (base != KETOGPU_LOOKUP_TRUNCATED) {
            uint32_t x = r, k = 0;
            o.out[base + k++] = x;
            do {
                x = par[x];
                o.out[base + k++] = x;
            } while (x != t);
        }
    }
    // (the walk reads parent words only: the bitmap may go meanwhile)
    for (uint64_t w = tid; w < bm_words; w += kT2Block)
        if (bm[w]) bm[w] = 0;
}

// ---------------------------------------------------------------------- combined listings
// ketogpu_lookup_combine / _combine_page: lookup(a, T) AND / ANDNOT / OR lookup(b, T).  The
// bodies are combine.hpp's, over the reverse rows: every id below N has a row, the member bound
// is Nx.
__global__ __launch_bounds__(64) void lookup_combine_tier1_kernel(Rows g, const uint32_t *a, const uint32_t *b,
                                                                  uint32_t n, uint32_t op, uint32_t type,
                                                                  int force_tier2, ListOut o, uint32_t *ovf_list,
                                                                  unsigned int *ovf_count) {
    __shared__ uint32_t set_a[kSlotsLds], set_b[kSlotsLds];
    __shared__ uint32_t work[kSetCap + 64];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    combine::tier1_list(g, g.Nx, g.N, a, b, i, lane, op, force_tier2, o, ovf_list, ovf_count, set_a, set_b, work,
                        [&](uint32_t u) { return type_ok(g, u, type); });
}

__global__ __launch_bounds__(kT2Block) void lookup_combine_tier2_kernel(Rows g, const uint32_t *a, const uint32_t *b,
                                                                        uint32_t op, uint32_t type, ListOut o,
                                                                        const uint32_t *ovf_list, uint32_t first,
                                                                        uint32_t *bitmaps, uint32_t *bitmaps2,
                                                                        uint64_t bm_words, uint32_t *worklists) {
    __shared__ combine::T2Lds s;
    const uint32_t i = ovf_list[first + blockIdx.x];
    combine::tier2_list(g, g.Nx, g.N, a[i], b[i], i, op, o, bitmaps + (uint64_t)blockIdx.x * bm_words,
                        bitmaps2 + (uint64_t)blockIdx.x * bm_words, bm_words, worklists + (uint64_t)blockIdx.x * g.Ni,
                        s, [&](uint32_t u) { return type_ok(g, u, type); });
}

__global__ __launch_bounds__(64) void lookup_combine_page_tier1_kernel(Rows g, const uint32_t *a, const uint32_t *b,
                                                                       const uint32_t *from, uint32_t n, uint32_t op,
                                                                       uint32_t type, int force_tier2,
                                                                       paged::PageOut o, uint32_t *ovf_list,
                                                                       unsigned int *ovf_count) {
    __shared__ uint32_t set_a[kSlotsLds], set_b[kSlotsLds];
    __shared__ uint32_t work[kSetCap + 64];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    combine::tier1_page(g, g.Nx, g.N, a, b, from, i, lane, op, force_tier2, o, ovf_list, ovf_count, set_a, set_b,
                        work, [&](uint32_t u) { return type_ok(g, u, type); });
}

__global__ __launch_bounds__(kT2Block) void lookup_combine_page_tier2_kernel(
    Rows g, const uint32_t *a, const uint32_t *b, const uint32_t *from, uint32_t op, uint32_t type, paged::PageOut o,
    const uint32_t *ovf_list, uint32_t first, uint32_t *bitmaps, uint32_t *bitmaps2, uint64_t bm_words,
    uint32_t *worklists) {
    __shared__ combine::T2Lds s;
    const uint32_t i = ovf_list[first + blockIdx.x];
    combine::tier2_page(g, g.Nx, g.N, a[i], b[i], from[i], i, op, o, bitmaps + (uint64_t)blockIdx.x * bm_words,
                        bitmaps2 + (uint64_t)blockIdx.x * bm_words, bm_words, worklists + (uint64_t)blockIdx.x * g.Ni,
                        s, [&](uint32_t u) { return type_ok(g, u, type); });
}

// ---------------------------------------------------------------------- depth-limited listings
// ketogpu_lookup_ids_depth / _page_depth: the members of lookup(t, T) within max_depth[i] hops
// of t (DESIGN.md "Depth-limited listings").  The kernels of the plain calls with depth.hpp's
// closure in tier 1 and its LevelStop in tier 2; the finishes are the plain ones.  frontier[i]
// is all zero on entry and is written where a search stopped at its limit.

// a member under any filter: what the frontier counts (a placeholder has no type)
__device__ inline bool any_type(const Rows &g, uint32_t u) { return type_ok(g, u, KETOGPU_TYPE_ANY); }
__global__ __launch_bounds__(64) void lookup_depth_tier1_kernel(Rows g, const uint32_t *targets,
                                                                const uint32_t *max_depth, uint32_t n, uint32_t type,
                                                                int force_tier2, ListOut o,
                                                                unsigned long long *frontier, uint32_t *ovf_list,
                                                                unsigned int *ovf_count) {
    __shared__ uint32_t set[kSlotsLds];
    __shared__ uint32_t work[kSetCap + 64];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const uint32_t t = targets[i];
    if (t >= g.N) {  // NONE: the empty list; any other id outside the snapshot: INVALID
        if (lane == 0) {
            o.begin[i] = t == KETOGPU_NODE_NONE ? 0ull : KETOGPU_LOOKUP_INVALID;
            o.count[i] = 0;
        }
        return;
    }
    uint32_t fr = 0;
    if (force_tier2 || !depth::tier1_closure(g, g.Nx, t, depth::limit_of(max_depth, i), lane, set, work, fr,
                                              [&](uint32_t u) { return any_type(g, u); })) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    if (lane == 0 && fr) frontier[i] = fr;
    tier1_finish(set, lane, i, o, [&](uint32_t u) { return type_ok(g, u, type); });
}

__global__ __launch_bounds__(kT2Block) void lookup_depth_tier2_kernel(Rows g, const uint32_t *targets,
                                                                      const uint32_t *max_depth, uint32_t type,
                                                                      ListOut o, unsigned long long *frontier,
                                                                      const uint32_t *ovf_list, uint32_t first,
                                                                      uint32_t *bitmaps, uint64_t bm_words,
                                                                      uint32_t *worklists) {
    __shared__ unsigned int s_tail, s_cnt, s_pos, s_fr;
    __shared__ unsigned long long s_base;
    const uint32_t i = ovf_list[first + blockIdx.x];
    const uint32_t t = targets[i];
    uint32_t *bm = bitmaps + (uint64_t)blockIdx.x * bm_words;
    uint32_t *wl = worklists + (uint64_t)blockIdx.x * g.Ni;
    if (threadIdx.x == 0) s_tail = 0, s_cnt = 0, s_pos = 0, s_fr = 0;
    __syncthreads();
    if (t >= g.N) return;  // (tier 1 lists valid targets only)
    depth::LevelStop stop(&s_tail, depth::limit_of(max_depth, i));
    tier2_closure(g, g.Nx, t, bm, wl, &s_tail, [](uint32_t, uint32_t) {}, depth::LevelStopRef{&stop});
    depth::tier2_frontier(stop, wl, frontier + i, &s_fr, [&](uint32_t u) { return any_type(g, u); });
    auto ok = [&](uint32_t u) { return type_ok(g, u, type); };
    const unsigned long long base = reserve_block(o, i, scan_count(bm, bm_words, ok), &s_cnt, &s_base);
    scan_write(bm, bm_words, base, o.out, ok, &s_pos);
}

__global__ __launch_bounds__(64) void lookup_depth_page_tier1_kernel(Rows g, const uint32_t *targets,
                                                                     const uint32_t *max_depth, const uint32_t *from,
                                                                     uint32_t n, uint32_t type, int force_tier2,
                                                                     paged::PageOut o, unsigned long long *frontier,
                                                                     uint32_t *ovf_list, unsigned int *ovf_count) {
    __shared__ uint32_t set[kSlotsLds];
    __shared__ uint32_t work[kSetCap + 64];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const uint32_t t = targets[i];
    if (t >= g.N) {  // NONE: the empty page; any other id outside the snapshot: INVALID
        if (lane == 0) paged::page_invalid(o, i, t != KETOGPU_NODE_NONE);
        return;
    }
    uint32_t fr = 0;
    if (force_tier2 || !depth::tier1_closure(g, g.Nx, t, depth::limit_of(max_depth, i), lane, set, work, fr,
                                              [&](uint32_t u) { return any_type(g, u); })) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    if (lane == 0 && fr) frontier[i] = fr;
    paged::page_finish_wave(set, kSlotsLds, lane, i, from[i], o, [&](uint32_t u) { return type_ok(g, u, type); });
}

__global__ __launch_bounds__(kT2Block) void lookup_depth_page_tier2_kernel(
    Rows g, const uint32_t *targets, const uint32_t *max_depth, const uint32_t *from, uint32_t type, paged::PageOut o,
    unsigned long long *frontier, const uint32_t *ovf_list, uint32_t first, uint32_t *bitmaps, uint64_t bm_words,
    uint32_t *worklists) {
    __shared__ unsigned int s_tail, s_cnt, s_rem, s_fr;
    __shared__ uint32_t s_wave[kT2Block / 64];
    const uint32_t i = ovf_list[first + blockIdx.x];
    const uint32_t t = targets[i];
    uint32_t *bm = bitmaps + (uint64_t)blockIdx.x * bm_words;
    uint32_t *wl = worklists + (uint64_t)blockIdx.x * g.Ni;
    if (threadIdx.x == 0) s_tail = 0, s_cnt = 0, s_rem = 0, s_fr = 0;
    __syncthreads();
    if (t >= g.N) return;  // (tier 1 lists valid targets only)
    depth::LevelStop stop(&s_tail, depth::limit_of(max_depth, i));
    tier2_closure(g, g.Nx, t, bm, wl, &s_tail, [](uint32_t, uint32_t) {}, depth::LevelStopRef{&stop});
    depth::tier2_frontier(stop, wl, frontier + i, &s_fr, [&](uint32_t u) { return any_type(g, u); });
    const uint32_t lo = from[i];
    auto ok = [&](uint32_t u) { return type_ok(g, u, type); };
    paged::page_select_block(bm, bm_words, lo, o.limit, o.out + (uint64_t)i * o.limit, s_wave, ok);
    __syncthreads();  // the selection has read the bitmap
    page_report(o, i, page_count_clear(bm, bm_words, lo, ok), &s_cnt, &s_rem);
}

// ---------------------------------------------------------------------- listings that say why
// ketogpu_lookup_ids_via / _page_via: the depth-limited listings with via[k], the node in whose
// reverse row out[k] was first seen (an entry of row(out[k]), one hop nearer the target), and
// hops[k], its distance (DESIGN.md "Grant trees").  The bodies are via.hpp's, over the reverse
// rows: every id below N has a row, the member bound is Nx.  A slot adds 2 x Nx words.
__device__ inline via::Slot lookup_via_slot(const Rows &g, uint32_t *bitmaps, uint64_t bm_words, uint32_t *worklists,
                                            uint32_t *words) {
    uint2 *why = reinterpret_cast<uint2 *>(words) + (uint64_t)blockIdx.x * g.Nx;
    return {bitmaps + (uint64_t)blockIdx.x * bm_words, bm_words, worklists + (uint64_t)blockIdx.x * g.Ni, why,
            nullptr, 0, nullptr, nullptr};
}

__global__ __launch_bounds__(64) void lookup_via_tier1_kernel(Rows g, const uint32_t *targets,
                                                              const uint32_t *max_depth, uint32_t n, uint32_t type,
                                                              int force_tier2, ListOut o, via::ViaOut vo,
                                                              unsigned long long *frontier, uint32_t *ovf_list,
                                                              unsigned int *ovf_count) {
    __shared__ via::T1Lds s;
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    via::tier1_list(
        g, g.Nx, g.N, targets, max_depth, i, lane, force_tier2, o, vo, frontier, ovf_list, ovf_count, s,
        [&](uint32_t u) { return type_ok(g, u, type); }, [&](uint32_t u) { return any_type(g, u); });
}

__global__ __launch_bounds__(kT2Block) void lookup_via_tier2_kernel(Rows g, const uint32_t *targets,
                                                                    const uint32_t *max_depth, uint32_t type,
                                                                    ListOut o, via::ViaOut vo,
                                                                    unsigned long long *frontier,
                                                                    const uint32_t *ovf_list, uint32_t first,
                                                                    uint32_t *bitmaps, uint64_t bm_words,
                                                                    uint32_t *worklists, uint32_t *words) {
    __shared__ via::T2Lds s;
    const uint32_t i = ovf_list[first + blockIdx.x];
    via::tier2_list<false>(
        g, g.Nx, g.N, targets[i], depth::limit_of(max_depth, i), i, o, vo, frontier,
        lookup_via_slot(g, bitmaps, bm_words, worklists, words), s, [&](uint32_t u) { return type_ok(g, u, type); },
        [&](uint32_t u) { return any_type(g, u); });
}

__global__ __launch_bounds__(64) void lookup_via_page_tier1_kernel(Rows g, const uint32_t *targets,
                                                                   const uint32_t *max_depth, const uint32_t *from,
                                                                   uint32_t n, uint32_t type, int force_tier2,
                                                                   paged::PageOut o, via::ViaOut vo,
                                                                   unsigned long long *frontier, uint32_t *ovf_list,
                                                                   unsigned int *ovf_count) {
    __shared__ via::T1Lds s;
    __shared__ uint32_t keys[kSlotsLds];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    via::tier1_page(
        g, g.Nx, g.N, targets, max_depth, from, i, lane, force_tier2, o, vo, frontier, ovf_list, ovf_count, s, keys,
        [&](uint32_t u) { return type_ok(g, u, type); }, [&](uint32_t u) { return any_type(g, u); });
}

__global__ __launch_bounds__(kT2Block) void lookup_via_page_tier2_kernel(
    Rows g, const uint32_t *targets, const uint32_t *max_depth, const uint32_t *from, uint32_t type, paged::PageOut o,
    via::ViaOut vo, unsigned long long *frontier, const uint32_t *ovf_list, uint32_t first, uint32_t *bitmaps,
    uint64_t bm_words, uint32_t *worklists, uint32_t *words) {
    __shared__ via::T2Lds s;
    const uint32_t i = ovf_list[first + blockIdx.x];
    via::tier2_page<false>(
        g, g.Nx, g.N, targets[i], depth::limit_of(max_depth, i), from[i], i, o, vo, frontier,
        lookup_via_slot(g, bitmaps, bm_words, worklists, words), s, [&](uint32_t u) { return type_ok(g, u, type); },
        [&](uint32_t u) { return any_type(g, u); });
}

// ---------------------------------------------------------------------- the wide tier
// ketogpu_lookup_ids_wide: the bodies are wide.hpp's, over the reverse rows: the ids below N
// have a row, the member bound is Nx.  The slot's bitmap is tier 2's; worklists are not used.
__global__ __launch_bounds__(wide::kBlock) void lookup_wide_level_kernel(Rows g, uint32_t type, wide::State w,
                                                                         unsigned long long lb,
                                                                         unsigned long long le) {
    wide::level(g, g.Nx, w, lb, le, [&](uint32_t u) { return type_ok(g, u, type); });
}

__global__ __launch_bounds__(wide::kBlock) void lookup_wide_write_kernel(Rows g, uint32_t type, wide::State w,
                                                                         ListOut o) {
    __shared__ unsigned int s_cnt;
    __shared__ unsigned long long s_at;
    wide::write(w, o, &s_cnt, &s_at, [&](uint32_t u) { return type_ok(g, u, type); });
}

// ketogpu_lookup_ids_depth_wide / _page_wide: the level under a depth limit, and the paged
// finish's select and clear (wide.hpp "depth", "page")
__global__ __launch_bounds__(wide::kBlock) void lookup_wide_level_depth_kernel(Rows g, uint32_t type, wide::State w,
                                                                               unsigned long long lb,
                                                                               unsigned long long le, wide::Cut cut) {
    wide::level_depth(
        g, g.Nx, w, lb, le, cut, [&](uint32_t u) { return type_ok(g, u, type); },
        [&](uint32_t u) { return any_type(g, u); });
}

__global__ __launch_bounds__(wide::kBlock) void lookup_wide_select_kernel(Rows g, uint32_t type, wide::State w,
                                                                          const uint32_t *ovf_list, uint32_t first,
                                                                          const uint32_t *from, paged::PageOut o) {
    __shared__ uint32_t s_wave[wide::kBlock / 64];
    wide::page_select(w, ovf_list, first, from, o, s_wave, [&](uint32_t u) { return type_ok(g, u, type); });
}

__global__ __launch_bounds__(wide::kBlock) void lookup_wide_clear_kernel(Rows g, uint32_t type, wide::State w,
                                                                         const uint32_t *ovf_list, uint32_t first,
                                                                         const uint32_t *from) {
    __shared__ unsigned int s_cnt;
    wide::page_clear(w, ovf_list, first, from, &s_cnt, [&](uint32_t u) { return type_ok(g, u, type); });
}

}  // namespace

struct ketogpu_lookup : ListHandle {
    uint32_t path_slots = 0, path_slot_max = 0;  // `slots` for path calls: a slot has a parent array too
    ketogpu_lookup_stats st{};
    ketogpu_lookup_path_stats pst{};
    ketogpu_combine_stats cst{};
    ketogpu_depth_stats dst{};
    ketogpu_via_stats vst{};

    ketogpu_lookup() : ListHandle("reverse lookup") {}

    // the rows and types of the snapshot's current version (caller holds its shared lock)
    void upload(const Snapshot &s) {
        if (s.has_ambiguous) throw Error(KETOGPU_EINVAL, what + ": the snapshot has shared Subject.String() keys (R4)");
        auto types = type_index_of(s);
        if (upload_rows(s, s.rev_off.data(), nullptr, s.rev_off.size(), s.rev_col.data(), s.rev_col.size(), 0,
                        types->node_type.data(), types->node_type.size(), 0, s.Nx))
            moved();
        st.uploads++;
    }

    // ---- what ListHandle::try_patch asks of a handle.  The reverse rows are uploaded as the
    // snapshot lays them out, free slots included, and rev_off never moves between rebuilds: a
    // changed row (KETOGPU_PATCH_REVERSE) is overwritten where it lies.  The types cover the
    // ids below Nx, which gain no members in place, and the bound is Nx: only g.N follows a
    // new subject (its reserved reverse row is in the upload already).
    static constexpr uint8_t kPatchKind = KETOGPU_PATCH_REVERSE;
    void host_row(const Snapshot &s, uint32_t v, const uint32_t *&p, uint64_t &len, uint64_t &at) const {
        at = s.rev_off[v], len = s.rev_off[v + 1] - at, p = s.rev_col.data() + at;
    }
    const uint32_t *host_keys(const Snapshot &) const { return nullptr; }
    uint32_t bound_of(const Snapshot &s) const { return s.Nx; }
    void moved() { path_slots = 0, path_slot_max = 0; }
    void patched(const Snapshot &) {}

    uint64_t slot_words() const { return ((uint64_t)g.Nx + 31) / 32 + std::max<uint32_t>(g.Ni, 1); }

    uint32_t alloc_slots(uint32_t wanted) { return ListHandle::need_slots(wanted, slot_words(), 0); }

    uint32_t need_slots(uint32_t wanted) { return st.slots = alloc_slots(wanted); }

    // tier 2's state for a combined call (ListHandle::need_pair_slots)
    uint32_t need_combine_slots(uint32_t wanted) {
        return cst.slots = need_pair_slots(wanted, slot_words(), [&](uint32_t k) { return alloc_slots(k); });
    }

    // tier 2's state for a path call: need_slots' bitmaps and worklists plus Nx parent words per
    // slot (d_aux), all three counted against the budget, so a path round may have fewer slots
    uint32_t need_path_slots(uint32_t wanted) {
        const uint64_t parw = std::max<uint32_t>(g.Nx, 1);
        uint64_t k = slots_for(wanted, slot_words() + parw, path_slot_max);
        if (k <= path_slots) return path_slots;
        path_slots = 0;
        k = std::min<uint64_t>(k, need_slots((uint32_t)k));  // (at least one)
        d_aux.need(k * parw);  // never cleared: a bitmap bit says which words hold
        return path_slots = (uint32_t)k;
    }

    void run(const uint32_t *targets, size_t n, uint32_t type, uint32_t *out, uint64_t capacity, uint64_t *begin,
             uint64_t *count, uint64_t *needed) {
        run_cursor(
            st, targets, n, out, capacity, begin, count, needed,
            [&](size_t i) { return begin[i] == KETOGPU_LOOKUP_INVALID || targets[i] == NONE; },
            [&](unsigned int *ovf_count) {
                KLAUNCH(lookup_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, (uint32_t)n, type,
                        force_tier2 ? 1 : 0, list_out(capacity), d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) { return need_slots(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(lookup_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, type, list_out(capacity),
                        d_ovf.p, first, d_bm.p, bm_words, d_wl.p);
            });
        st.last_call_ms = ms_of_call();
    }

    // ketogpu_lookup_ids_wide: run() with tier 1's overflows in rounds of the wide tier
    void run_ids_wide(const uint32_t *targets, size_t n, uint32_t type, uint32_t *out, uint64_t capacity,
                      uint64_t *begin, uint64_t *count, uint64_t *needed) {
        ListHandle::run_wide(
            targets, n, out, capacity, begin, count, needed,
            [&](size_t i) { return begin[i] == KETOGPU_LOOKUP_INVALID || targets[i] == NONE; },
            [&](unsigned int *ovf_count) {
                KLAUNCH(lookup_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, (uint32_t)n, type,
                        force_tier2 ? 1 : 0, list_out(capacity), d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) {
                return wst.slots = need_wide_slots(ovf, slot_words(), [&](uint32_t k) { return alloc_slots(k); });
            },
            [&](uint32_t first, uint32_t k) {
                wide_round(
                    first, k, g.N,
                    [&](const wide::State &w, uint32_t, unsigned long long lb, unsigned long long le) {
                        KLAUNCH(lookup_wide_level_kernel, dim3(wide::level_grid(le - lb)), dim3(wide::kBlock), 0,
                                stream, g, type, w, lb, le);
                    },
                    [&](const wide::State &w) { wide_list_finish(w, first, type, capacity); });
            });
    }

    // the wide tier's full-list finish: reserve, then the write kernel
    void wide_list_finish(const wide::State &w, uint32_t first, uint32_t type, uint64_t capacity) {
        wide_reserve(w, first, capacity);
        KLAUNCH(lookup_wide_write_kernel, wide_write_grid(w.nslots), dim3(wide::kBlock), 0, stream, g, type, w,
                list_out(capacity));
    }

    uint32_t need_wide_state(uint32_t wanted) {
        return wst.slots = need_wide_slots(wanted, slot_words(), [&](uint32_t k) { return alloc_slots(k); });
    }

    // a wide round's level launch under the limits d_depth (null: none)
    void wide_level_depth(const wide::State &w, uint32_t L, unsigned long long lb, unsigned long long le,
                          uint32_t type, const uint32_t *d_depth, uint32_t first) {
        KLAUNCH(lookup_wide_level_depth_kernel, dim3(wide::level_grid(le - lb)), dim3(wide::kBlock), 0, stream, g,
                type, w, lb, le, wide::Cut{L, d_depth, d_ovf.p, first, d_front.p});
    }

    // ketogpu_lookup_ids_depth_wide: run_depth() with tier 1's overflows in rounds of the wide
    // tier, counted in wst alone
    void run_depth_wide(const uint32_t *targets, const uint32_t *max_depth, size_t n, uint32_t type, uint32_t *out,
                        uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *frontier, uint64_t *needed) {
        const uint32_t *d_depth = upload_depth(max_depth, n);
        ListHandle::run_wide(
            targets, n, out, capacity, begin, count, needed,
            [&](size_t i) { return begin[i] == KETOGPU_LOOKUP_INVALID || targets[i] == NONE; },
            [&](unsigned int *ovf_count) {
                KLAUNCH(lookup_depth_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_depth,
                        (uint32_t)n, type, force_tier2 ? 1 : 0, list_out(capacity), d_front.p, d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) { return need_wide_state(ovf); },
            [&](uint32_t first, uint32_t k) {
                wide_round(
                    first, k, g.N,
                    [&](const wide::State &w, uint32_t L, unsigned long long lb, unsigned long long le) {
                        wide_level_depth(w, L, lb, le, type, d_depth, first);
                    },
                    [&](const wide::State &w) { wide_list_finish(w, first, type, capacity); });
            });
        read_frontier(frontier, n);
        wst.last_call_ms = ms_of_call();
    }

    // ketogpu_lookup_page_wide: run_page_depth() with tier 1's overflows in rounds of the wide
    // tier and the paged finish of wide.hpp, counted in wst alone
    void run_page_wide(const uint32_t *targets, const uint32_t *max_depth, const uint32_t *from, size_t n,
                       uint32_t type, uint32_t limit, uint32_t *out, uint32_t *returned, uint64_t *count,
                       uint64_t *remaining, uint64_t *frontier) {
        const uint32_t *d_depth = upload_depth(max_depth, n);
        ListHandle::run_page_wide(
            targets, from, n, limit, out, returned, count, remaining,
            [&](unsigned int *ovf_count) {
                KLAUNCH(lookup_depth_page_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_depth,
                        d_from.p, (uint32_t)n, type, force_tier2 ? 1 : 0, page_out(limit), d_front.p, d_ovf.p,
                        ovf_count);
            },
            [&](uint32_t ovf) { return need_wide_state(ovf); },
            [&](uint32_t first, uint32_t k) {
                wide_round(
                    first, k, g.N,
                    [&](const wide::State &w, uint32_t L, unsigned long long lb, unsigned long long le) {
                        wide_level_depth(w, L, lb, le, type, d_depth, first);
                    },
                    [&](const wide::State &w) {
                        wide_page_finish(
                            w, first, limit,
                            [&](const wide::State &w) {
                                KLAUNCH(lookup_wide_select_kernel, dim3(k), dim3(wide::kBlock), 0, stream, g, type, w,
                                        d_ovf.p, first, d_from.p, page_out(limit));
                            },
                            [&](const wide::State &w) {
                                KLAUNCH(lookup_wide_clear_kernel, wide_clear_grid(k), dim3(wide::kBlock), 0, stream, g,
                                        type, w, d_ovf.p, first, d_from.p);
                            });
                    });
            });
        read_frontier(frontier, n);
        wst.last_call_ms = ms_of_call();
    }

    // the paged call: run() with the ordered finish
    void run_page(const uint32_t *targets, const uint32_t *from, size_t n, uint32_t type, uint32_t limit, uint32_t *out,
                  uint32_t *returned, uint64_t *count, uint64_t *remaining) {
        ListHandle::run_page(
            st, targets, from, n, limit, out, returned, count, remaining,
            [&](unsigned int *ovf_count) {
                KLAUNCH(lookup_page_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_from.p,
                        (uint32_t)n, type, force_tier2 ? 1 : 0, page_out(limit), d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) { return need_slots(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(lookup_page_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, d_from.p, type,
                        page_out(limit), d_ovf.p, first, d_bm.p, bm_words, d_wl.p);
            },
            [](Tally &) {});
        st.last_call_ms = ms_of_call();
    }

    // ketogpu_lookup_paths: run()'s output contract, one path per (root, target) pair
    void run_paths(const uint32_t *roots, const uint32_t *targets, size_t n, uint32_t *out, uint64_t capacity,
                   uint64_t *begin, uint64_t *count, uint64_t *needed) {
        if (n) {
            d_req2.need(n);
            HIP_CHECK(hipMemcpyAsync(d_req2.p, roots, n * 4, hipMemcpyHostToDevice, stream));
        }
        run_cursor(
            pst, targets, n, out, capacity, begin, count, needed,
            [&](size_t i) { return roots[i] >= g.Nx || targets[i] >= g.N; },  // answered before any row was read
            [&](unsigned int *ovf_count) {
                KLAUNCH(path_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req2.p, d_req.p, (uint32_t)n,
                        force_tier2 ? 1 : 0, list_out(capacity), d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) { return need_path_slots(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(path_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req2.p, d_req.p, list_out(capacity),
                        d_ovf.p, first, d_bm.p, bm_words, d_wl.p, d_aux.p);
            });
        for (size_t i = 0; i < n; i++) pst.allowed += count[i] != 0;
    }

    // a pair answered before any row was read: no side has one (an INVALID pair is counted by
    // its marker)
    bool no_row(uint32_t a, uint32_t b) const { return a >= g.N && b >= g.N; }

    // ketogpu_lookup_combine: run()'s output contract, one list per pair (a, b)
    void run_combine(const uint32_t *a, const uint32_t *b, size_t n, uint32_t op, uint32_t type, uint32_t *out,
                     uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *needed) {
        run_cursor(
            cst, a, b, n, out, capacity, begin, count, needed,
            [&](size_t i) { return begin[i] == KETOGPU_LOOKUP_INVALID || no_row(a[i], b[i]); },
            [&](unsigned int *ovf_count) {
                KLAUNCH(lookup_combine_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_req2.p,
                        (uint32_t)n, op, type, force_tier2 ? 1 : 0, list_out(capacity), d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) { return need_combine_slots(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(lookup_combine_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, d_req2.p, op, type,
                        list_out(capacity), d_ovf.p, first, d_bm.p, d_bm2.p, bm_words, d_wl.p);
            });
        cst.last_call_ms = ms_of_call();
    }

    // ketogpu_lookup_combine_page: run_page()'s output contract, one page per pair (a, b)
    void run_combine_page(const uint32_t *a, const uint32_t *b, const uint32_t *from, size_t n, uint32_t op,
                          uint32_t type, uint32_t limit, uint32_t *out, uint32_t *returned, uint64_t *count,
                          uint64_t *remaining) {
        ListHandle::run_page(
            cst, a, b, from, n, limit, out, returned, count, remaining, [&](size_t i) { return no_row(a[i], b[i]); },
            [&](unsigned int *ovf_count) {
                KLAUNCH(lookup_combine_page_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_req2.p,
                        d_from.p, (uint32_t)n, op, type, force_tier2 ? 1 : 0, page_out(limit), d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) { return need_combine_slots(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(lookup_combine_page_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, d_req2.p,
                        d_from.p, op, type, page_out(limit), d_ovf.p, first, d_bm.p, d_bm2.p, bm_words, d_wl.p);
            },
            [](Tally &) {});
        cst.last_call_ms = ms_of_call();
    }
    // ketogpu_lookup_ids_depth: run() with a limit per request (null: none) and the frontier
    void run_depth(const uint32_t *targets, const uint32_t *max_depth, size_t n, uint32_t type, uint32_t *out,
                   uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *frontier, uint64_t *needed) {
        const uint32_t *d_depth = upload_depth(max_depth, n);
        run_cursor(
            dst, targets, n, out, capacity, begin, count, needed,
            [&](size_t i) { return begin[i] == KETOGPU_LOOKUP_INVALID || targets[i] == NONE; },
            [&](unsigned int *ovf_count) {
                KLAUNCH(lookup_depth_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_depth,
                        (uint32_t)n, type, force_tier2 ? 1 : 0, list_out(capacity), d_front.p, d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) { return dst.slots = alloc_slots(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(lookup_depth_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, d_depth, type,
                        list_out(capacity), d_front.p, d_ovf.p, first, d_bm.p, bm_words, d_wl.p);
            });
        dst.cut_requests += read_frontier(frontier, n);
        dst.last_call_ms = ms_of_call();
    }

    // ketogpu_lookup_page_depth: run_page() with a limit per request and the frontier
    void run_page_depth(const uint32_t *targets, const uint32_t *max_depth, const uint32_t *from, size_t n,
                        uint32_t type, uint32_t limit, uint32_t *out, uint32_t *returned, uint64_t *count,
                        uint64_t *remaining, uint64_t *frontier) {
        const uint32_t *d_depth = upload_depth(max_depth, n);
        ListHandle::run_page(
            dst, targets, from, n, limit, out, returned, count, remaining,
            [&](unsigned int *ovf_count) {
                KLAUNCH(lookup_depth_page_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_depth,
                        d_from.p, (uint32_t)n, type, force_tier2 ? 1 : 0, page_out(limit), d_front.p, d_ovf.p,
                        ovf_count);
            },
            [&](uint32_t ovf) { return dst.slots = alloc_slots(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(lookup_depth_page_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, d_depth,
                        d_from.p, type, page_out(limit), d_front.p, d_ovf.p, first, d_bm.p, bm_words, d_wl.p);
            },
            [](Tally &) {});
        dst.cut_requests += read_frontier(frontier, n);
        dst.last_call_ms = ms_of_call();
    }

    // tier 2's state for a via call (ListHandle::need_via_slots)
    uint32_t need_via_state(uint32_t wanted) {
        return vst.slots = need_via_slots(wanted, slot_words(), [&](uint32_t k) { return alloc_slots(k); });
    }

    // ketogpu_lookup_ids_via: run_depth() with via and hops next to out
    void run_via(const uint32_t *targets, const uint32_t *max_depth, size_t n, uint32_t type, uint32_t *out,
                 uint32_t *via, uint32_t *hops, uint64_t capacity, uint64_t *begin, uint64_t *count,
                 uint64_t *frontier, uint64_t *needed) {
        const uint32_t *d_depth = upload_depth(max_depth, n);
        const via::ViaOut vo = via_out(via, hops, capacity);
        run_cursor(
            vst, targets, n, nullptr, capacity, begin, count, needed,  // (the ids come back with via and hops)
            [&](size_t i) { return begin[i] == KETOGPU_LOOKUP_INVALID || targets[i] == NONE; },
            [&](unsigned int *ovf_count) {
                KLAUNCH(lookup_via_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_depth,
                        (uint32_t)n, type, force_tier2 ? 1 : 0, list_out(capacity), vo, d_front.p, d_ovf.p, ovf_count);
            },
            [&](uint32_t ovf) { return need_via_state(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(lookup_via_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, d_depth, type,
                        list_out(capacity), vo, d_front.p, d_ovf.p, first, d_bm.p, bm_words, d_wl.p, d_viast.p);
            });
        read_via(out, via, hops, written_end(begin, count, n));
        vst.cut_requests += read_frontier(frontier, n);
        vst.last_call_ms = ms_of_call();
    }

    // ketogpu_lookup_page_via: run_page_depth() with via and hops at the stride of out
    void run_page_via(const uint32_t *targets, const uint32_t *max_depth, const uint32_t *from, size_t n,
                      uint32_t type, uint32_t limit, uint32_t *out, uint32_t *via, uint32_t *hops, uint32_t *returned,
                      uint64_t *count, uint64_t *remaining, uint64_t *frontier) {
        const uint32_t *d_depth = upload_depth(max_depth, n);
        const via::ViaOut vo = via_out(via, hops, n * (uint64_t)limit);
        ListHandle::run_page(
            vst, targets, from, n, limit, out, returned, count, remaining,
            [&](unsigned int *ovf_count) {
                KLAUNCH(lookup_via_page_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_req.p, d_depth,
                        d_from.p, (uint32_t)n, type, force_tier2 ? 1 : 0, page_out(limit), vo, d_front.p, d_ovf.p,
                        ovf_count);
            },
            [&](uint32_t ovf) { return need_via_state(ovf); },
            [&](uint32_t first, uint32_t k) {
                KLAUNCH(lookup_via_page_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_req.p, d_depth,
                        d_from.p, type, page_out(limit), vo, d_front.p, d_ovf.p, first, d_bm.p, bm_words, d_wl.p,
                        d_viast.p);
            },
            [](Tally &) {});
        read_via(nullptr, via, hops, n * (uint64_t)limit);
        vst.cut_requests += read_frontier(frontier, n);
        vst.last_call_ms = ms_of_call();
    }
};

extern "C" {

int ketogpu_lookup_new(const ketogpu_snapshot *sp, const ketogpu_lookup_opts *opts, ketogpu_lookup **out) {
    return list_new(sp, opts, out, "KETOGPU_LOOKUP_TIER", "KETOGPU_LOOKUP_SLOTS",
                    [](ketogpu_lookup &l) { l.st.set_capacity = kSetCap; });
}

void ketogpu_lookup_free(ketogpu_lookup *l) { delete l; }

int ketogpu_lookup_stats_get(const ketogpu_lookup *l, ketogpu_lookup_stats *out) {
    return list_stats_get(l, &ketogpu_lookup::st, out);
}

int ketogpu_lookup_refresh_stats_get(const ketogpu_lookup *l, ketogpu_list_refresh_stats *out) {
    return list_stats_get<ListHandle>(l, &ListHandle::rst, out);
}

int ketogpu_lookup_ids(ketogpu_lookup *l, const uint32_t *targets, size_t n, uint32_t type, uint32_t *out,
                       uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *needed) {
    return list_call(l, !needed || (n && (!targets || !begin || !count)) || (capacity && !out), n, "targets", nullptr,
                     [&] { l->run(targets, n, type, out, capacity, begin, count, needed); });
}

int ketogpu_lookup_wide_stats_get(const ketogpu_lookup *l, ketogpu_wide_stats *out) {
    return list_stats_get<ListHandle>(l, &ListHandle::wst, out);
}

int ketogpu_lookup_ids_wide(ketogpu_lookup *l, const uint32_t *targets, size_t n, uint32_t type, uint32_t *out,
                            uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *needed) {
    return list_call(l, !needed || (n && (!targets || !begin || !count)) || (capacity && !out), n, "targets", nullptr,
                     [&] { l->run_ids_wide(targets, n, type, out, capacity, begin, count, needed); });
}

int ketogpu_lookup_ids_depth_wide(ketogpu_lookup *l, const uint32_t *targets, const uint32_t *max_depth, size_t n,
                                  uint32_t type, uint32_t *out, uint64_t capacity, uint64_t *begin, uint64_t *count,
                                  uint64_t *frontier, uint64_t *needed) {
    return list_call(l, !needed || (n && (!targets || !begin || !count)) || (capacity && !out), n, "targets", nullptr,
                     [&] {
                         l->run_depth_wide(targets, max_depth, n, type, out, capacity, begin, count, frontier, needed);
                     });
}

int ketogpu_lookup_page_wide(ketogpu_lookup *l, const uint32_t *targets, const uint32_t *max_depth,
                             const uint32_t *from, size_t n, uint32_t type, uint32_t limit, uint32_t *out,
                             uint32_t *returned, uint64_t *count, uint64_t *remaining, uint64_t *frontier) {
    return list_call(l, n && (!targets || !out || !returned || !count || !remaining), n, "targets", &limit, [&] {
        l->run_page_wide(targets, max_depth, from, n, type, limit, out, returned, count, remaining, frontier);
    });
}

int ketogpu_lookup_page(ketogpu_lookup *l, const uint32_t *targets, const uint32_t *from, size_t n, uint32_t type,
                        uint32_t limit, uint32_t *out, uint32_t *returned, uint64_t *count, uint64_t *remaining) {
    return list_call(l, n && (!targets || !out || !returned || !count || !remaining), n, "targets", &limit,
                     [&] { l->run_page(targets, from, n, type, limit, out, returned, count, remaining); });
}

int ketogpu_lookup_path_stats_get(const ketogpu_lookup *l, ketogpu_lookup_path_stats *out) {
    return list_stats_get(l, &ketogpu_lookup::pst, out);
}

int ketogpu_lookup_paths(ketogpu_lookup *l, const uint32_t *roots, const uint32_t *targets, size_t n, uint32_t *out,
                         uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *needed) {
    return list_call(l, !needed || (n && (!roots || !targets || !begin || !count)) || (capacity && !out), n, "pairs",
                     nullptr, [&] { l->run_paths(roots, targets, n, out, capacity, begin, count, needed); });
}

int ketogpu_lookup_combine_stats_get(const ketogpu_lookup *l, ketogpu_combine_stats *out) {
    return list_stats_get(l, &ketogpu_lookup::cst, out);
}

int ketogpu_lookup_combine(ketogpu_lookup *l, const uint32_t *a, const uint32_t *b, size_t n, uint32_t op,
                           uint32_t type, uint32_t *out, uint64_t capacity, uint64_t *begin, uint64_t *count,
                           uint64_t *needed) {
    if (l && op > KETOGPU_COMBINE_OR) return einval(l->what + ": an unknown combine operator");
    return list_call(l, !needed || (n && (!a || !b || !begin || !count)) || (capacity && !out), n, "pairs", nullptr,
                     [&] { l->run_combine(a, b, n, op, type, out, capacity, begin, count, needed); });
}

int ketogpu_lookup_combine_page(ketogpu_lookup *l, const uint32_t *a, const uint32_t *b, const uint32_t *from,
                                size_t n, uint32_t op, uint32_t type, uint32_t limit, uint32_t *out,
                                uint32_t *returned, uint64_t *count, uint64_t *remaining) {
    if (l && op > KETOGPU_COMBINE_OR) return einval(l->what + ": an unknown combine operator");
    return list_call(l, n && (!a || !b || !out || !returned || !count || !remaining), n, "pairs", &limit, [&] {
        l->run_combine_page(a, b, from, n, op, type, limit, out, returned, count, remaining);
    });
}

int ketogpu_lookup_depth_stats_get(const ketogpu_lookup *l, ketogpu_depth_stats *out) {
    return list_stats_get(l, &ketogpu_lookup::dst, out);
}

int ketogpu_lookup_ids_depth(ketogpu_lookup *l, const uint32_t *targets, const uint32_t *max_depth, size_t n,
                             uint32_t type, uint32_t *out, uint64_t capacity, uint64_t *begin, uint64_t *count,
                             uint64_t *frontier, uint64_t *needed) {
    return list_call(l, !needed || (n && (!targets || !begin || !count)) || (capacity && !out), n, "targets", nullptr,
                     [&] { l->run_depth(targets, max_depth, n, type, out, capacity, begin, count, frontier, needed); });
}

int ketogpu_lookup_page_depth(ketogpu_lookup *l, const uint32_t *targets, const uint32_t *max_depth,
                              const uint32_t *from, size_t n, uint32_t type, uint32_t limit, uint32_t *out,
                              uint32_t *returned, uint64_t *count, uint64_t *remaining, uint64_t *frontier) {
    return list_call(l, n && (!targets || !out || !returned || !count || !remaining), n, "targets", &limit, [&] {
        l->run_page_depth(targets, max_depth, from, n, type, limit, out, returned, count, remaining, frontier);
    });
}

int ketogpu_lookup_via_stats_get(const ketogpu_lookup *l, ketogpu_via_stats *out) {
    return list_stats_get(l, &ketogpu_lookup::vst, out);
}

int ketogpu_lookup_ids_via(ketogpu_lookup *l, const uint32_t *targets, const uint32_t *max_depth, size_t n,
                           uint32_t type, uint32_t *out, uint32_t *via, uint32_t *hops, uint64_t capacity,
                           uint64_t *begin, uint64_t *count, uint64_t *frontier, uint64_t *needed) {
    return list_call(l, !needed || (n && (!targets || !begin || !count)) || (capacity && !out), n, "targets", nullptr,
                     [&] {
                         l->run_via(targets, max_depth, n, type, out, capacity ? via : nullptr,
                                    capacity ? hops : nullptr, capacity, begin, count, frontier, needed);
                     });
}

int ketogpu_lookup_page_via(ketogpu_lookup *l, const uint32_t *targets, const uint32_t *max_depth,
                            const uint32_t *from, size_t n, uint32_t type, uint32_t limit, uint32_t *out,
                            uint32_t *via, uint32_t *hops, uint32_t *returned, uint64_t *count, uint64_t *remaining,
                            uint64_t *frontier) {
    return list_call(l, n && (!targets || !out || !returned || !count || !remaining), n, "targets", &limit, [&] {
        l->run_page_via(targets, max_depth, from, n, type, limit, out, via, hops, returned, count, remaining,
                        frontier);
    });
}

}  // extern "C"

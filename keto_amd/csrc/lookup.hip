// lookup.hip — reverse lookup on the device (include/ketogpu.h ketogpu_lookup_*).
//
// lookup(t, T) lists B(t), the expandable nodes that reach t in >= 1 edge, restricted to the
// object type T: the least set that holds rev(t) and rev(x) for every x in it (DESIGN.md
// "Reverse lookup").  Only interior entries (ids < Ni) have reverse rows, so only they are put
// on a worklist.  Two kernels:
//
//   tier 1  one wave per request.  B(t) lives in an LDS open-addressing set (insert by LDS
//           compare-and-swap) that is visited set and result at once; the interior members
//           also go on an LDS worklist (each enters once, so it needs no more room than the
//           set).  Rows are read 64 entries per step.  A request whose set passes kSetCap is
//           appended to the overflow list and leaves no output.
//   tier 2  one workgroup per overflow request, `slots` requests per launch.  Each slot has a
//           bitmap over the expandable nodes and a worklist of Ni entries in global memory; a
//           level loop with __syncthreads() runs the closure to its end whatever its size.
//
// Both end the same way: count the members of type T, reserve exactly that many ids of `out`
// with one device-scope atomicAdd on a cursor, and write the list with plain vector stores if
// it fits below `capacity` (else begin = TRUNCATED; the count is exact either way).  The cursor
// ends at the sum of the counts, so a capacity of at least that sum truncates nothing.
//
// The paged call (ketogpu_lookup_page) runs the same two closures (tier1_closure, tier2_closure: one
// implementation each, called by the full-list and the paged kernel) and ends with the ordered
// finish of paged_finish.hpp instead: the `limit` smallest members >= from[i] to the stride
// out + i * limit, ascending, with the exact count and what remains; no cursor, no truncation.
//
// The path call (ketogpu_lookup_paths) searches in the same order with kernels of its own
// (path_tier1_kernel, path_tier2_kernel below): every first visit records its parent, and the
// search ends when the root is visited.
//
// Every index is validated before it is used: targets against num_nodes before rev_off is
// touched, row entries against num_expandable before the type array or a bitmap is.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>

#include "hip_host.hpp"
#include "lookup.hpp"
#include "paged_finish.hpp"

using namespace ketogpu;

namespace {

constexpr uint32_t kSetCap = 1024;         // tier 1: nodes a set may hold (ketogpu_lookup_stats.set_capacity)
constexpr uint32_t kSlotsLds = 2 * kSetCap;  // hash slots: a load of at most (kSetCap + 64) / kSlotsLds
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr unsigned kT2Block = 256;
static_assert(kT2Block == paged::kBlock, "the paged selection assumes tier 2's workgroup");

struct LGraph {
    const uint64_t *rev_off;   // N + 1 (a writable snapshot: n_cap + 1)
    const uint32_t *rev_col;
    const uint32_t *node_type; // Nx
    uint32_t N, Nx, Ni;
};

struct LOut {
    uint32_t *out;
    unsigned long long capacity;
    unsigned long long *begin, *count;
    unsigned long long *cursor;  // ids reserved so far: ends at `needed`
    unsigned long long *truncated;
};

__device__ inline bool type_ok(const LGraph &g, uint32_t u, uint32_t want) {
    if (u >= g.Nx) return false;
    const uint32_t ty = g.node_type[u];
    return want == KETOGPU_TYPE_ANY ? ty != KETOGPU_TYPE_NONE : (want != KETOGPU_TYPE_NONE && ty == want);
}

__device__ inline uint32_t slot_of(uint32_t u) { return (u * 0x9E3779B1u) >> 21; }  // 11 bits
static_assert(kSlotsLds == 1u << 11, "slot_of yields 11 bits");

// ---------------------------------------------------------------------- tier 1
// tier 1's closure, by one wave: B(t) into `set` (all kSlotsLds slots are initialised here), its
// interior members through `work`.  False when the set passed kSetCap: the request overflows.
__device__ __forceinline__ bool tier1_closure(const LGraph &g, uint32_t t, uint32_t lane, uint32_t *set,
                                              uint32_t *work) {
    for (uint32_t s = lane; s < kSlotsLds; s += 64) set[s] = kEmpty;
    __syncthreads();
    uint32_t size = 0, head = 0, tail = 0;  // wave-uniform
    bool over = false;
    uint32_t v = t;
    for (;;) {
        const uint64_t b = g.rev_off[v], e = g.rev_off[v + 1];
        for (uint64_t base = b; base < e && !over; base += 64) {
            const uint64_t j = base + lane;
            const uint32_t u = j < e ? g.rev_col[j] : kEmpty;
            bool fresh = false;
            if (u < g.Nx) {  // (also drops kEmpty) — the set never holds more than kSetCap + 64 of
                             // its 2 x kSetCap slots, so the probe ends at a free slot
                uint32_t s = slot_of(u);
                for (;;) {
                    const uint32_t old = atomicCAS(&set[s], kEmpty, u);
                    if (old == kEmpty) {
                        fresh = true;
                        break;
                    }
                    if (old == u) break;
                    s = (s + 1) & (kSlotsLds - 1);
                }
            }
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

__global__ __launch_bounds__(64) void lookup_tier1_kernel(LGraph g, const uint32_t *targets, uint32_t n, uint32_t type,
                                                          int force_tier2, LOut o, uint32_t *ovf_list,
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
    const bool over = !tier1_closure(g, t, lane, set, work);
    if (over) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    uint32_t cnt = 0;
    for (uint32_t s = lane; s < kSlotsLds; s += 64) cnt += __popcll(__ballot(type_ok(g, set[s], type)));
    unsigned long long base = 0;
    if (lane == 0) {
        base = atomicAdd(o.cursor, (unsigned long long)cnt);
        const bool fits = base + cnt <= o.capacity;
        o.count[i] = cnt;
        o.begin[i] = fits ? base : KETOGPU_LOOKUP_TRUNCATED;
        if (!fits) atomicAdd(o.truncated, 1ull);
    }
    base = __shfl(base, 0);
    if (base + cnt > o.capacity || !cnt) return;
    uint32_t w = 0;
    for (uint32_t s = lane; s < kSlotsLds; s += 64) {
        const uint32_t u = set[s];
        const bool m = type_ok(g, u, type);
        const unsigned long long mm = __ballot(m);
        if (m) o.out[base + w + __popcll(mm & ((1ull << lane) - 1))] = u;
        w += __popcll(mm);
    }
}

// ---------------------------------------------------------------------- tier 2
// tier 2's closure, by the whole workgroup: B(t) into the slot's bitmap `bm` (all zero on entry),
// its interior members through the worklist `wl`.  *s_tail is an LDS counter, zero on entry and
// published by a barrier.  Ends behind a barrier: every thread sees the whole bitmap.
__device__ __forceinline__ void tier2_closure(const LGraph &g, uint32_t t, uint32_t *bm, uint32_t *wl,
                                              unsigned int *s_tail) {
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = kT2Block / 64;
    auto visit = [&](uint32_t u) {
        if (u >= g.Nx) return;
        const uint32_t bit = 1u << (u & 31);
        if (atomicOr(&bm[u >> 5], bit) & bit) return;
        if (u < g.Ni) wl[atomicAdd(s_tail, 1u)] = u;  // each interior node enters once: <= Ni entries
    };
    {  // the target's own row, by the whole workgroup
        const uint64_t b = g.rev_off[t], e = g.rev_off[t + 1];
        for (uint64_t j = b + tid; j < e; j += kT2Block) visit(g.rev_col[j]);
    }
    __syncthreads();
    uint32_t lb = 0, le = *s_tail;
    while (lb < le) {  // one level: a wave per row
        __syncthreads();  // everyone has read s_tail before it moves
        for (uint32_t k = lb + wave; k < le; k += nwaves) {
            const uint32_t v = wl[k];
            const uint64_t b = g.rev_off[v], e = g.rev_off[v + 1];
            for (uint64_t j = b + lane; j < e; j += 64) visit(g.rev_col[j]);
        }
        __syncthreads();
        lb = le;
        le = *s_tail;
    }
}

// Block s of round r serves overflow request ovf_list[first + s] with slot s's state.  The
// bitmap is all zero on entry and is cleared again on the way out.
__global__ __launch_bounds__(kT2Block) void lookup_tier2_kernel(LGraph g, const uint32_t *targets, uint32_t type,
                                                                LOut o, const uint32_t *ovf_list, uint32_t first,
                                                                uint32_t *bitmaps, uint64_t bm_words, uint32_t *worklists) {
    __shared__ unsigned int s_tail, s_cnt, s_pos;
    __shared__ unsigned long long s_base;
    const uint32_t i = ovf_list[first + blockIdx.x];
    const uint32_t t = targets[i];
    uint32_t *bm = bitmaps + (uint64_t)blockIdx.x * bm_words;
    uint32_t *wl = worklists + (uint64_t)blockIdx.x * g.Ni;
    const unsigned tid = threadIdx.x;
    if (tid == 0) s_tail = 0, s_cnt = 0, s_pos = 0;
    __syncthreads();
    if (t >= g.N) return;  // (tier 1 lists valid targets only)
    tier2_closure(g, t, bm, wl, &s_tail);
    // count the members of the type
    uint32_t c = 0;
    for (uint64_t w = tid; w < bm_words; w += kT2Block) {
        uint32_t bits = bm[w];
        while (bits) {
            const uint32_t u = (uint32_t)(w << 5) + (uint32_t)__ffs(bits) - 1;
            bits &= bits - 1;
            c += type_ok(g, u, type);
        }
    }
    if (c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (tid == 0) {
        const unsigned long long cnt = s_cnt, base = atomicAdd(o.cursor, cnt);
        const bool fits = base + cnt <= o.capacity;
        o.count[i] = cnt;
        o.begin[i] = fits ? base : KETOGPU_LOOKUP_TRUNCATED;
        if (!fits) atomicAdd(o.truncated, 1ull);
        s_base = fits ? base : KETOGPU_LOOKUP_TRUNCATED;
    }
    __syncthreads();
    const unsigned long long base = s_base;
    for (uint64_t w = tid; w < bm_words; w += kT2Block) {
        uint32_t bits = bm[w];
        if (!bits) continue;
        bm[w] = 0;
        if (base == KETOGPU_LOOKUP_TRUNCATED) continue;
        uint32_t ids[32], k = 0;
        while (bits) {
            const uint32_t u = (uint32_t)(w << 5) + (uint32_t)__ffs(bits) - 1;
            bits &= bits - 1;
            if (type_ok(g, u, type)) ids[k++] = u;
        }
        if (!k) continue;
        const uint32_t p = atomicAdd(&s_pos, k);
        for (uint32_t x = 0; x < k; x++) o.out[base + p + x] = ids[x];
    }
}

// ---------------------------------------------------------------------- paged finish
// The same closures with the ordered finish of paged_finish.hpp: request i reports count,
// remaining and returned, and writes its page to the stride out + i * limit.
__global__ __launch_bounds__(64) void lookup_page_tier1_kernel(LGraph g, const uint32_t *targets, const uint32_t *from,
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
    if (force_tier2 || !tier1_closure(g, t, lane, set, work)) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    paged::page_finish_wave(set, kSlotsLds, lane, i, from[i], o, [&](uint32_t u) { return type_ok(g, u, type); });
}

// Selection in id order first, then one scan that counts and clears: the slot is left all zero
// for whichever kernel of the handle uses it next.
__global__ __launch_bounds__(kT2Block) void lookup_page_tier2_kernel(LGraph g, const uint32_t *targets,
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
    const unsigned tid = threadIdx.x;
    if (tid == 0) s_tail = 0, s_cnt = 0, s_rem = 0;
    __syncthreads();
    if (t >= g.N) return;  // (tier 1 lists valid targets only)
    tier2_closure(g, t, bm, wl, &s_tail);
    const uint32_t lo = from[i];
    auto ok = [&](uint32_t u) { return type_ok(g, u, type); };
    paged::page_select_block(bm, bm_words, lo, o.limit, o.out + (uint64_t)i * o.limit, s_wave, ok);
    __syncthreads();  // the selection has read the bitmap
    uint32_t c = 0, r = 0;
    for (uint64_t w = tid; w < bm_words; w += kT2Block) {
        uint32_t bits = bm[w];
        if (!bits) continue;
        bm[w] = 0;
        while (bits) {
            const uint32_t u = (uint32_t)(w << 5) + (uint32_t)__ffs(bits) - 1;
            bits &= bits - 1;
            const bool m = ok(u);
            c += m;
            r += m && u >= lo;
        }
    }
    if (c) atomicAdd(&s_cnt, c);
    if (r) atomicAdd(&s_rem, r);
    __syncthreads();
    if (tid == 0) {
        o.count[i] = s_cnt;
        o.remaining[i] = s_rem;
        o.returned[i] = s_rem < o.limit ? s_rem : o.limit;
    }
}

// ---------------------------------------------------------------------- shortest path
// ketogpu_lookup_paths: one path r = v0, ..., vk = t with the fewest hops, v(i) in rev(v(i+1)).
// Both closures above visit in level order (tier 1 works its rows first in, first out; tier 2
// runs level by level between barriers), so the search below is theirs with two additions: each
// first visit records the node whose row it was found in, and the search stops once r is seen.
// The first visit of r then lies on a shortest path, and walking the recorded parents from r
// leads to t.  Only the target's own row records t as a parent: whatever a later expansion of
// t (t on a cycle) finds was seen in that first row already, so the walk ends at the first t.
constexpr uint16_t kParTarget = 0xFFFFu;  // tier 1's parent word: seen in the target's own row
static_assert(kSlotsLds <= kParTarget, "a slot index fits a parent word");

// r and t as ketogpu_lookup_paths classifies them before any row is read
__device__ inline bool path_trivial(const LGraph &g, uint32_t r, uint32_t t, uint32_t i, uint32_t lane, const LOut &o) {
    const bool bad = (r >= g.N && r != KETOGPU_NODE_NONE) || (t >= g.N && t != KETOGPU_NODE_NONE);
    if (!bad && r < g.Nx && t < g.N) return false;
    if (lane == 0) {  // an id outside the snapshot: INVALID; NONE or a never-expanded root: denied
        o.begin[i] = bad ? KETOGPU_LOOKUP_INVALID : 0ull;
        o.count[i] = 0;
    }
    return true;
}

// one thread: reserve `cnt` ids for path i (a denied pair reserves nothing) -> where to write
// it, or TRUNCATED
__device__ inline unsigned long long path_reserve(const LOut &o, uint32_t i, uint32_t cnt) {
    o.count[i] = cnt;
    if (!cnt) {
        o.begin[i] = 0;
        return KETOGPU_LOOKUP_TRUNCATED;
    }
    const unsigned long long base = atomicAdd(o.cursor, (unsigned long long)cnt);
    const bool fits = base + cnt <= o.capacity;
    o.begin[i] = fits ? base : KETOGPU_LOOKUP_TRUNCATED;
    if (!fits) atomicAdd(o.truncated, 1ull);
    return fits ? base : KETOGPU_LOOKUP_TRUNCATED;
}

// tier 1: lookup_tier1_kernel's set and worklist, a parent word per slot (the slot of the node
// whose row the member was first seen in, or kParTarget), and the worklist holds slots, so the
// row at hand knows its own.  A ballot on u == r after every 64-entry step ends the search.
__global__ __launch_bounds__(64) void path_tier1_kernel(LGraph g, const uint32_t *roots, const uint32_t *targets,
                                                        uint32_t n, int force_tier2, LOut o, uint32_t *ovf_list,
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
        const uint64_t b = g.rev_off[v], e = g.rev_off[v + 1];
        for (uint64_t base = b; base < e && !over && !hit; base += 64) {
            const uint64_t j = base + lane;
            const uint32_t u = j < e ? g.rev_col[j] : kEmpty;
            bool fresh = false;
            uint32_t s = 0;
            if (u < g.Nx) {  // (also drops kEmpty) — at most kSetCap + 64 of the 2 x kSetCap slots are
                             // ever taken, so the probe ends at a free slot
                s = slot_of(u);
                for (;;) {
                    const uint32_t old = atomicCAS(&set[s], kEmpty, u);
                    if (old == kEmpty) {
                        fresh = true;
                        break;
                    }
                    if (old == u) break;
                    s = (s + 1) & (kSlotsLds - 1);
                }
            }
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
__global__ __launch_bounds__(kT2Block) void path_tier2_kernel(LGraph g, const uint32_t *roots, const uint32_t *targets,
                                                              LOut o, const uint32_t *ovf_list, uint32_t first,
                                                              uint32_t *bitmaps, uint64_t bm_words, uint32_t *worklists,
                                                              uint32_t *parents) {
    __shared__ unsigned int s_tail, s_hit;
    const uint32_t i = ovf_list[first + blockIdx.x];
    const uint32_t r = roots[i], t = targets[i];
    uint32_t *bm = bitmaps + (uint64_t)blockIdx.x * bm_words;
    uint32_t *wl = worklists + (uint64_t)blockIdx.x * g.Ni;
    uint32_t *par = parents + (uint64_t)blockIdx.x * g.Nx;
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = kT2Block / 64;
    if (tid == 0) s_tail = 0, s_hit = 0;
    __syncthreads();
    if (t >= g.N || r >= g.Nx) return;  // (tier 1 lists pairs that need a search only)
    auto visit = [&](uint32_t u, uint32_t v) {
        if (u >= g.Nx) return;
        const uint32_t bit = 1u << (u & 31);
        if (atomicOr(&bm[u >> 5], bit) & bit) return;
        par[u] = v;  // the winner of the atomicOr: the first visit
        if (u < g.Ni) wl[atomicAdd(&s_tail, 1u)] = u;  // each interior node enters once: <= Ni entries
        if (u == r) s_hit = 1;
    };
    {  // the target's own row, by the whole workgroup
        const uint64_t b = g.rev_off[t], e = g.rev_off[t + 1];
        for (uint64_t j = b + tid; j < e; j += kT2Block) visit(g.rev_col[j], t);
    }
    __syncthreads();
    uint32_t lb = 0, le = s_tail;
    bool hit = s_hit != 0;
    while (lb < le && !hit) {  // one level: a wave per row
        __syncthreads();  // everyone has read s_tail and s_hit before they move
        for (uint32_t k = lb + wave; k < le; k += nwaves) {
            const uint32_t v = wl[k];
            const uint64_t b = g.rev_off[v], e = g.rev_off[v + 1];
            for (uint64_t j = b + lane; j < e; j += 64) visit(g.rev_col[j], v);
        }
        __syncthreads();  // the level is complete: its parent words are visible
        lb = le;
        le = s_tail;
        hit = s_hit != 0;
    }
    if (tid == 0) {  // the chain r -> ... -> t: every node on it but t has its bit set
        uint32_t cnt = 0;
        if (hit) {
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

}  // namespace

struct ketogpu_lookup {
    std::shared_ptr<Snapshot::ReaderLink> link;  // cleared when the snapshot is freed first
    int device = 0;
    uint64_t budget = 0;
    bool force_tier2 = false;
    uint32_t slot_cap = 0;  // KETOGPU_LOOKUP_SLOTS (0: no cap)
    hipStream_t stream = nullptr;
    std::mutex mu;          // one call at a time per handle
    uint64_t version = ~0ull;
    LGraph g{};
    DBuf<uint64_t> d_off;
    DBuf<uint32_t> d_col, d_type, d_targets, d_ovf, d_out, d_bm, d_wl;
    DBuf<unsigned long long> d_begin, d_count, d_ctr;  // d_ctr: cursor, truncated, overflow count
    DBuf<uint32_t> d_from, d_ret;                       // paged calls: lower bounds, returned
    DBuf<uint32_t> d_roots, d_par;                      // path calls: roots, tier 2's parent words
    uint32_t slots = 0, slot_max = 0;  // tier 2: allocated slots; what budget and knob allow (0: not yet known)
    uint32_t path_slots = 0, path_slot_max = 0;  // the same for path calls: a slot has a parent array too
    uint64_t bm_words = 0;
    ketogpu_lookup_stats st{};
    ketogpu_lookup_path_stats pst{};

    // the rows and types of the snapshot's current version (caller holds its shared lock)
    void upload(const Snapshot &s) {
        if (s.has_ambiguous)
            throw Error(KETOGPU_EINVAL, "reverse lookup: the snapshot has shared Subject.String() keys (R4)");
        auto types = type_index_of(s);
        d_off.need(s.rev_off.size());
        d_col.need(s.rev_col.size());
        d_type.need(types->node_type.size());
        HIP_CHECK(hipMemcpyAsync(d_off.p, s.rev_off.data(), s.rev_off.size() * 8, hipMemcpyHostToDevice, stream));
        if (!s.rev_col.empty())
            HIP_CHECK(hipMemcpyAsync(d_col.p, s.rev_col.data(), s.rev_col.size() * 4, hipMemcpyHostToDevice, stream));
        if (!types->node_type.empty())
            HIP_CHECK(hipMemcpyAsync(d_type.p, types->node_type.data(), types->node_type.size() * 4,
                                     hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        if (s.Nx != g.Nx || s.Ni != g.Ni) {  // tier 2's state follows the sizes
            slots = 0, slot_max = 0, d_bm.drop(), d_wl.drop();
            path_slots = 0, path_slot_max = 0, d_par.drop();
        }
        g = LGraph{d_off.p, d_col.p, d_type.p, s.N, s.Nx, s.Ni};
        version = s.version;
        st.uploads++;
    }

    // tier 2's state: as many slots as the batch at hand can use, within what the budget allows
    // (at least one); a later batch with more overflows allocates again
    void need_slots(uint32_t wanted) {
        if (!slot_max) {
            bm_words = ((uint64_t)g.Nx + 31) / 32;
            const uint64_t per = (bm_words + std::max<uint32_t>(g.Ni, 1)) * 4;
            uint64_t b = budget;
            if (!b) {
                size_t fr = 0, tot = 0;
                HIP_CHECK(hipMemGetInfo(&fr, &tot));
                b = fr / 8;
            }
            slot_max = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(b / per, 1), 1024);
            if (slot_cap) slot_max = std::min(slot_max, slot_cap);
        }
        uint64_t k = 1;
        while (k < wanted) k *= 2;
        k = std::min<uint64_t>(k, slot_max);
        if (k <= slots) return;
        slots = 0;  // (an allocation that fails below leaves no half-prepared state behind)
        d_bm.need(k * std::max<uint64_t>(bm_words, 1));
        d_wl.need(k * std::max<uint32_t>(g.Ni, 1));
        HIP_CHECK(hipMemsetAsync(d_bm.p, 0, k * std::max<uint64_t>(bm_words, 1) * 4, stream));
        slots = (uint32_t)k;
        st.slots = slots;
    }

    // the rows of the snapshot's current version, uploaded again if a write moved it
    void refresh() {
        // (the link's lock is not held together with the snapshot's: a snapshot is not
        // freed while a call on it runs, only before or after)
        const Snapshot *sp;
        {
            std::lock_guard<std::mutex> lk(link->mu);
            sp = link->snap;
        }
        if (!sp) throw Error(KETOGPU_EINVAL, "reverse lookup: the snapshot was freed");
        std::shared_lock<std::shared_mutex> rd(sp->mu);
        if (sp->version != version) upload(*sp);
    }

    void run(const uint32_t *targets, size_t n, uint32_t type, uint32_t *out, uint64_t capacity, uint64_t *begin,
             uint64_t *count, uint64_t *needed) {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_CHECK(hipSetDevice(device));
        refresh();
        *needed = 0;
        st.requests += n;
        if (n) {
            d_targets.need(n), d_ovf.need(n), d_begin.need(n), d_count.need(n), d_ctr.need(4), d_out.need(capacity);
            HIP_CHECK(hipMemcpyAsync(d_targets.p, targets, n * 4, hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, 4 * sizeof(unsigned long long), stream));
            LOut o{d_out.p, capacity, d_begin.p, d_count.p, d_ctr.p, d_ctr.p + 1};
            unsigned int *ovf_count = (unsigned int *)(d_ctr.p + 2);
            KLAUNCH(lookup_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_targets.p, (uint32_t)n, type,
                    force_tier2 ? 1 : 0, o, d_ovf.p, ovf_count);
            unsigned long long ctr[4];
            HIP_CHECK(hipMemcpyAsync(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            const uint32_t ovf = (uint32_t)(ctr[2] & 0xFFFFFFFFu);
            if (ovf) {
                need_slots(ovf);
                for (uint32_t first = 0; first < ovf; first += slots) {
                    const uint32_t k = std::min<uint32_t>(slots, ovf - first);
                    KLAUNCH(lookup_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_targets.p, type, o, d_ovf.p,
                            first, d_bm.p, bm_words, d_wl.p);
                    st.tier2_rounds++;
                }
                HIP_CHECK(hipMemcpyAsync(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
            }
            HIP_CHECK(hipMemcpyAsync(begin, d_begin.p, n * 8, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(count, d_count.p, n * 8, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            const uint64_t written = std::min<uint64_t>(ctr[0], capacity);  // every written list ends below both
            if (written && out) {
                HIP_CHECK(hipMemcpyAsync(out, d_out.p, written * 4, hipMemcpyDeviceToHost, stream));
                HIP_CHECK(hipStreamSynchronize(stream));
            }
            *needed = ctr[0];
            st.tier2_requests += ovf;
            uint64_t invalid = 0;
            for (size_t i = 0; i < n; i++) invalid += begin[i] == KETOGPU_LOOKUP_INVALID || targets[i] == NONE;
            st.tier1_requests += n - ovf - invalid;
            st.ids_produced += ctr[0];
            st.truncated_lists += ctr[1];
        }
        st.last_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }

    // the paged call: run() with the ordered finish.  `from` may be null (all zero).
    void run_page(const uint32_t *targets, const uint32_t *from, size_t n, uint32_t type, uint32_t limit, uint32_t *out,
                  uint32_t *returned, uint64_t *count, uint64_t *remaining) {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_CHECK(hipSetDevice(device));
        refresh();
        st.requests += n;
        if (n) {
            d_targets.need(n), d_from.need(n), d_ovf.need(n), d_ret.need(n), d_begin.need(n), d_count.need(n),
                d_ctr.need(4), d_out.need(n * (size_t)limit);
            HIP_CHECK(hipMemcpyAsync(d_targets.p, targets, n * 4, hipMemcpyHostToDevice, stream));
            if (from)
                HIP_CHECK(hipMemcpyAsync(d_from.p, from, n * 4, hipMemcpyHostToDevice, stream));
            else
                HIP_CHECK(hipMemsetAsync(d_from.p, 0, n * 4, stream));
            HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, 4 * sizeof(unsigned long long), stream));
            paged::PageOut o{d_out.p, limit, d_ret.p, d_count.p, d_begin.p};  // (d_begin holds `remaining`)
            unsigned int *ovf_count = (unsigned int *)(d_ctr.p + 2);
            KLAUNCH(lookup_page_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_targets.p, d_from.p,
                    (uint32_t)n, type, force_tier2 ? 1 : 0, o, d_ovf.p, ovf_count);
            unsigned long long ctr[4];
            HIP_CHECK(hipMemcpyAsync(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            const uint32_t ovf = (uint32_t)(ctr[2] & 0xFFFFFFFFu);
            if (ovf) {
                need_slots(ovf);
                for (uint32_t first = 0; first < ovf; first += slots) {
                    const uint32_t k = std::min<uint32_t>(slots, ovf - first);
                    KLAUNCH(lookup_page_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_targets.p, d_from.p,
                            type, o, d_ovf.p, first, d_bm.p, bm_words, d_wl.p);
                    st.tier2_rounds++;
                }
            }
            HIP_CHECK(hipMemcpyAsync(returned, d_ret.p, n * 4, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(count, d_count.p, n * 8, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(remaining, d_begin.p, n * 8, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(out, d_out.p, n * (size_t)limit * 4, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            st.tier2_requests += ovf;
            uint64_t unlisted = 0, produced = 0;
            for (size_t i = 0; i < n; i++) {
                unlisted += returned[i] == KETOGPU_PAGE_INVALID || targets[i] == NONE;
                produced += returned[i] == KETOGPU_PAGE_INVALID ? 0 : returned[i];
            }
            st.tier1_requests += n - ovf - unlisted;
            st.ids_produced += produced;
        }
        st.last_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }

    // tier 2's state for a path call: need_slots' bitmaps and worklists plus Nx parent words per
    // slot, all three counted against the budget, so a path round may have fewer slots
    void need_path_slots(uint32_t wanted) {
        if (!path_slot_max) {
            const uint64_t words = ((uint64_t)g.Nx + 31) / 32;
            const uint64_t per = (words + std::max<uint32_t>(g.Ni, 1) + std::max<uint32_t>(g.Nx, 1)) * 4;
            uint64_t b = budget;
            if (!b) {
                size_t fr = 0, tot = 0;
                HIP_CHECK(hipMemGetInfo(&fr, &tot));
                b = fr / 8;
            }
            path_slot_max = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(b / per, 1), 1024);
            if (slot_cap) path_slot_max = std::min(path_slot_max, slot_cap);
        }
        uint64_t k = 1;
        while (k < wanted) k *= 2;
        k = std::min<uint64_t>(k, path_slot_max);
        if (k <= path_slots) return;
        path_slots = 0;
        need_slots((uint32_t)k);
        k = std::min<uint64_t>(k, slots);  // (at least one)
        d_par.need(k * std::max<uint32_t>(g.Nx, 1));  // never cleared: a bitmap bit says which words hold
        path_slots = (uint32_t)k;
    }

    // ketogpu_lookup_paths: run()'s output contract, one path per (root, target) pair
    void run_paths(const uint32_t *roots, const uint32_t *targets, size_t n, uint32_t *out, uint64_t capacity,
                   uint64_t *begin, uint64_t *count, uint64_t *needed) {
        HIP_CHECK(hipSetDevice(device));
        refresh();
        *needed = 0;
        pst.requests += n;
        if (!n) return;
        d_roots.need(n), d_targets.need(n), d_ovf.need(n), d_begin.need(n), d_count.need(n), d_ctr.need(4),
            d_out.need(capacity);
        HIP_CHECK(hipMemcpyAsync(d_roots.p, roots, n * 4, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_targets.p, targets, n * 4, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, 4 * sizeof(unsigned long long), stream));
        LOut o{d_out.p, capacity, d_begin.p, d_count.p, d_ctr.p, d_ctr.p + 1};
        unsigned int *ovf_count = (unsigned int *)(d_ctr.p + 2);
        KLAUNCH(path_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_roots.p, d_targets.p, (uint32_t)n,
                force_tier2 ? 1 : 0, o, d_ovf.p, ovf_count);
        unsigned long long ctr[4];
        HIP_CHECK(hipMemcpyAsync(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        const uint32_t ovf = (uint32_t)(ctr[2] & 0xFFFFFFFFu);
        if (ovf) {
            need_path_slots(ovf);
            for (uint32_t first = 0; first < ovf; first += path_slots) {
                const uint32_t k = std::min<uint32_t>(path_slots, ovf - first);
                KLAUNCH(path_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_roots.p, d_targets.p, o, d_ovf.p,
                        first, d_bm.p, bm_words, d_wl.p, d_par.p);
                pst.tier2_rounds++;
            }
            HIP_CHECK(hipMemcpyAsync(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
        }
        HIP_CHECK(hipMemcpyAsync(begin, d_begin.p, n * 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(count, d_count.p, n * 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        const uint64_t written = std::min<uint64_t>(ctr[0], capacity);  // every written path ends below both
        if (written && out) {
            HIP_CHECK(hipMemcpyAsync(out, d_out.p, written * 4, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
        }
        *needed = ctr[0];
        uint64_t unsearched = 0, allowed = 0;  // pairs answered before any row was read
        for (size_t i = 0; i < n; i++) {
            unsearched += roots[i] >= g.Nx || targets[i] >= g.N;
            allowed += count[i] != 0;
        }
        pst.tier2_requests += ovf;
        pst.tier1_requests += n - ovf - unsearched;
        pst.allowed += allowed;
        pst.ids_produced += ctr[0];
        pst.truncated_lists += ctr[1];
    }

    ~ketogpu_lookup() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream), (void)hipStreamDestroy(stream);
        d_off.drop(), d_col.drop(), d_type.drop(), d_targets.drop(), d_ovf.drop(), d_out.drop(), d_bm.drop(), d_wl.drop();
        d_begin.drop(), d_count.drop(), d_ctr.drop(), d_from.drop(), d_ret.drop(), d_roots.drop(), d_par.drop();
    }
};

extern "C" {

int ketogpu_lookup_new(const ketogpu_snapshot *sp, const ketogpu_lookup_opts *opts, ketogpu_lookup **out) {
    if (!sp || !out) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    *out = nullptr;
    return guarded([&] {
        const Snapshot &s = *reinterpret_cast<const Snapshot *>(sp);
        auto l = std::make_unique<ketogpu_lookup>();
        l->device = opts ? opts->device : 0;
        l->budget = opts ? opts->state_budget_bytes : 0;
        if (const char *e = getenv("KETOGPU_LOOKUP_TIER")) l->force_tier2 = atoi(e) == 2;
        if (const char *e = getenv("KETOGPU_LOOKUP_SLOTS")) l->slot_cap = (uint32_t)std::max(atoi(e), 0);
        l->st.set_capacity = kSetCap;
        l->link = s.link;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || l->device < 0 || l->device >= ndev)
            throw Error(KETOGPU_EDEVICE, "reverse lookup: no such HIP device");
        HIP_CHECK(hipSetDevice(l->device));
        HIP_CHECK(hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking));
        std::shared_lock<std::shared_mutex> rd(s.mu);
        l->upload(s);
        {
            std::lock_guard<std::mutex> lk(s.link->mu);
            s.link->snap = &s;  // the way back to the snapshot; its destructor clears it
        }
        *out = l.release();
    });
}

void ketogpu_lookup_free(ketogpu_lookup *l) { delete l; }

int ketogpu_lookup_stats_get(const ketogpu_lookup *l, ketogpu_lookup_stats *out) {
    if (!l || !out) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    std::lock_guard<std::mutex> lk(const_cast<ketogpu_lookup *>(l)->mu);
    *out = l->st;
    return KETOGPU_OK;
}

int ketogpu_lookup_ids(ketogpu_lookup *l, const uint32_t *targets, size_t n, uint32_t type, uint32_t *out,
                       uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *needed) {
    if (!l || !needed || (n && (!targets || !begin || !count)) || (capacity && !out)) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    if (n >= (1ull << 31)) {
        set_last_error("reverse lookup: more than 2^31 - 1 targets in one call");
        return KETOGPU_EINVAL;
    }
    return guarded([&] {
        std::lock_guard<std::mutex> lk(l->mu);
        l->run(targets, n, type, out, capacity, begin, count, needed);
    });
}

int ketogpu_lookup_page(ketogpu_lookup *l, const uint32_t *targets, const uint32_t *from, size_t n, uint32_t type,
                        uint32_t limit, uint32_t *out, uint32_t *returned, uint64_t *count, uint64_t *remaining) {
    if (!l || (n && (!targets || !out || !returned || !count || !remaining))) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    if (!limit || limit > KETOGPU_PAGE_LIMIT_MAX) {
        set_last_error("reverse lookup: a page limit outside [1, KETOGPU_PAGE_LIMIT_MAX]");
        return KETOGPU_EINVAL;
    }
    if (n >= (1ull << 31)) {
        set_last_error("reverse lookup: more than 2^31 - 1 targets in one call");
        return KETOGPU_EINVAL;
    }
    return guarded([&] {
        std::lock_guard<std::mutex> lk(l->mu);
        l->run_page(targets, from, n, type, limit, out, returned, count, remaining);
    });
}

int ketogpu_lookup_path_stats_get(const ketogpu_lookup *l, ketogpu_lookup_path_stats *out) {
    if (!l || !out) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    std::lock_guard<std::mutex> lk(const_cast<ketogpu_lookup *>(l)->mu);
    *out = l->pst;
    return KETOGPU_OK;
}

int ketogpu_lookup_paths(ketogpu_lookup *l, const uint32_t *roots, const uint32_t *targets, size_t n, uint32_t *out,
                         uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *needed) {
    if (!l || !needed || (n && (!roots || !targets || !begin || !count)) || (capacity && !out)) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    if (n >= (1ull << 31)) {
        set_last_error("reverse lookup: more than 2^31 - 1 pairs in one call");
        return KETOGPU_EINVAL;
    }
    return guarded([&] {
        std::lock_guard<std::mutex> lk(l->mu);
        l->run_paths(roots, targets, n, out, capacity, begin, count, needed);
    });
}

}  // extern "C"

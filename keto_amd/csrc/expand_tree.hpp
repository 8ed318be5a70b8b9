// expand_tree.hpp — BuildTree on the device (include/ketogpu.h ketogpu_subjects_expand): the
// bodies of subjects.hip's expand kernels.  Next to depth.hpp and via.hpp, and in their idiom:
// plain templates over closure.hpp's rows, sets and reservations.
//
// A tree is written in preorder as two parallel arrays, node id and child count (DESIGN.md
// "Expand on the device").  The walk is the host's (host_engine.cpp IdExpander), and unlike the
// closures it depends on order: children keep the row's order, and one visited set covers the
// whole tree.  Two facts let it stream with nothing to backpatch: a union's child count is its
// row length, known when it is opened; and only nodes that have a row ever need the visited
// set, so the set and the DFS stack are bounded by the opened nodes, not by the tree.
//
// A frame is (v, next offset in v's row).  The root's rest depth minus the stack height is the
// rest depth of the children of the frame on top, so no depth is stored.  One step reads a
// window of v's row from the frame's offset and classifies its entries:
//   * an entry without a row of its own is a leaf, whatever the state of the walk;
//   * children at rest depth 1 are all leaves, but every entry that has a row is inserted: the
//     reference marks a subject set visited before it looks at the depth;
//   * deeper, the entries that have a row test membership in parallel.  Visited ones are leaves
//     (the set only grows).  The first unvisited one, at window index k, is the recursion point:
//     [0, k) go out as leaves, k as a union with its row length, k is inserted, the frame's
//     offset moves behind k and the walk descends.  On return the frame reads again from that
//     offset and tests again: a later sibling may have been opened inside the subtree.
// Output positions are uniform across the wave (tier 1) or the workgroup (tier 2); every entry
// goes out with a plain vector store.
//
// A first visit to a node whose bit is set in the bad-row bitmap (its query has a row with an
// unknown namespace) ends the request with status HOST.  A node without a row is not in the
// visited set, so each of its occurrences is a first visit, as on the host.
//
// The size of a tree is not known before it is walked, so a request walks twice: once to count,
// then, behind one reservation as the list finishes make it, once to write.  A count-only call
// (capacity 0) and a tree that does not fit walk once.
//
//   tier 1  one wave per request: the visited set is closure.hpp's LDS set, the stack kSetCap
//           frames in LDS, the window 64 entries.  A request whose set would pass kSetCap
//           (which bounds the stack too) is appended to the overflow list.
//   tier 2  one workgroup of kT2Block per overflow request: the slot's bitmap is the visited
//           set, the stack lies in global memory at two words per frame (at most one frame per
//           node that has a row), the window is kT2Block entries, and the state of the walk is
//           uniform: in LDS, behind barriers.  The bitmap is cleared between the walks and on
//           the way out, by the slot's seen list while the opened nodes fit it, else as a span.
//
// Every index is validated before it is used: a root against N and Nx, a row entry against N
// before the bad-row bitmap or the visited bitmap is touched and against Nx before the offsets.
#pragma once

#include "closure.hpp"

namespace ketogpu {
namespace expand {

using namespace closure;

// the rows with what only this call reads: the bad-row bitmap over the N nodes (null: no query
// of the snapshot has a bad row)
struct Graph {
    Rows g;
    const uint32_t *bad;
};

struct TreeOut {
    ListOut l;           // l.out: the node ids
    uint32_t *children;  // parallel to l.out (null in a count-only call)
    uint32_t *status;
};

enum Walk { kDone, kHost, kOver };

__device__ __forceinline__ uint32_t row_len(const Rows &g, uint32_t u) {  // u < g.Nx
    uint64_t b, e;
    row_bounds(g, u, b, e);
    return (uint32_t)(e - b);
}

__device__ __forceinline__ bool is_bad(const Graph &x, uint32_t u) {
    return x.bad && u < x.g.N && (x.bad[u >> 5] >> (u & 31) & 1);
}

// node `at` of the output.  The writing walk repeats the counting walk step for step, so `at`
// lies inside the tree's reservation; the comparison keeps a store inside the arrays whatever
// else may go wrong
__device__ __forceinline__ void put(const TreeOut &o, unsigned long long at, uint32_t u, uint32_t children) {
    if (at < o.l.capacity) o.l.out[at] = u, o.children[at] = children;
}

// request i answered without a tree, by one thread
__device__ inline void no_tree(const TreeOut &o, uint32_t i, unsigned long long begin, uint32_t status) {
    o.l.begin[i] = begin;
    o.l.count[i] = 0;
    o.status[i] = status;
}

// What a root is before any row is read, by every thread alike -> true: answered here (lane
// `first` wrote it).  Else r has a row and rest depth >= 2: the tree is a union, to be walked.
__device__ __forceinline__ bool root_answered(const Graph &x, uint32_t r, uint32_t depth, uint32_t i, bool first,
                                              const TreeOut &o) {
    const Rows &g = x.g;
    if (r >= g.N) {  // NONE: the nil tree; any other id outside the snapshot: INVALID
        if (first) no_tree(o, i, r == KETOGPU_NODE_NONE ? 0ull : KETOGPU_LOOKUP_INVALID, KETOGPU_EXPAND_NIL);
        return true;
    }
    if (!depth) {
        if (first) no_tree(o, i, 0, KETOGPU_EXPAND_NIL);
        return true;
    }
    const bool subject_id = r >= g.Nx && g.filter_key[r] == KETOGPU_CLASS_SUBJECT_ID;
    if (!subject_id && is_bad(x, r)) {
        if (first) no_tree(o, i, 0, KETOGPU_EXPAND_HOST);
        return true;
    }
    const uint32_t len = r < g.Nx ? row_len(g, r) : 0;
    if (!len && !subject_id) {  // a subject set whose query is empty
        if (first) no_tree(o, i, 0, KETOGPU_EXPAND_NIL);
        return true;
    }
    if (subject_id || depth == 1) {  // one leaf
        if (first) {
            const unsigned long long base = reserve(o.l, i, 1);
            o.status[i] = KETOGPU_EXPAND_OK;
            if (base != KETOGPU_LOOKUP_TRUNCATED) put(o, base, r, 0);
        }
        return true;
    }
    return false;
}

// ---------------------------------------------------------------------- tier 1
struct T1Lds {
    uint32_t set[kSlotsLds];
    uint32_t v[kSetCap], off[kSetCap];  // the stack
};

// is u in the LDS set?  (set_insert's probe without the insertion)
__device__ __forceinline__ bool set_has(const uint32_t *set, uint32_t u) {
    uint32_t slot = slot_of(u);
    for (;;) {
        const uint32_t x = set[slot];
        if (x == u) return true;
        if (x == kEmpty) return false;
        slot = (slot + 1) & (kSlotsLds - 1);
    }
}

// One walk of r's tree by one wave (r has a row, depth >= 2).  kWrite: the tree goes to
// out / children from `base` on; else it is only counted.  `total`: its size.
template <bool kWrite>
__device__ __forceinline__ Walk tier1_walk(const Graph &x, uint32_t r, uint32_t depth, uint32_t lane, T1Lds &s,
                                           const TreeOut &o, unsigned long long base, unsigned long long &total) {
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

// tier 1's request, by one wave
__device__ __forceinline__ void tier1_tree(const Graph &x, const uint32_t *roots, const uint32_t *depths, uint32_t i,
                                           uint32_t lane, int force_tier2, const TreeOut &o, uint32_t *ovf_list,
                                           unsigned int *ovf_count, T1Lds &s) {
    const uint32_t r = roots[i], depth = depths[i];
    if (root_answered(x, r, depth, i, lane == 0, o)) return;
    unsigned long long total = 0;
    const Walk w = force_tier2 ? kOver : tier1_walk<false>(x, r, depth, lane, s, o, 0, total);
    if (w == kOver) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    if (w == kHost) {
        if (lane == 0) no_tree(o, i, 0, KETOGPU_EXPAND_HOST);
        return;
    }
    unsigned long long base = 0;
    if (lane == 0) {
        base = reserve(o.l, i, total);
        o.status[i] = KETOGPU_EXPAND_OK;
    }
    base = __shfl(base, 0);
    if (base == KETOGPU_LOOKUP_TRUNCATED) return;
    tier1_walk<true>(x, r, depth, lane, s, o, base, total);
}

// ---------------------------------------------------------------------- tier 2
constexpr uint32_t kNoLane = kT2Block;

struct T2Lds {
    uint32_t sp, v, off;      // the stack height and the frame on top
    unsigned int seen, host;  // first visits so far; a bad row was met
    unsigned long long pos;
    uint32_t first[kT2Block / 64];  // per wave: its lowest unvisited entry
};

// a slot's state: the bitmap over the member bound (all zero on entry and on exit), the seen
// list, and the stack: frame f is stack[2f], stack[2f + 1]
struct Slot {
    uint32_t *bm;
    uint64_t bm_words;
    uint32_t *seen;
    uint32_t list_cap;
    uint32_t *stack;
};

// u's first visit: into the bitmap and, while there is room, onto the seen list
__device__ __forceinline__ bool t2_mark(const Slot &sl, T2Lds &s, uint32_t u) {
    const uint32_t bit = 1u << (u & 31);
    if (atomicOr(&sl.bm[u >> 5], bit) & bit) return false;
    const uint32_t k = atomicAdd(&s.seen, 1u);
    if (k < sl.list_cap) sl.seen[k] = u;
    return true;
}

// the bitmap back to all zero, by the whole workgroup, behind a barrier and ending at one
__device__ __forceinline__ void t2_clear(const Slot &sl, T2Lds &s) {
    const uint32_t total = s.seen;
    if (total <= sl.list_cap) {
        for (uint32_t k = threadIdx.x; k < total; k += kT2Block) sl.bm[sl.seen[k] >> 5] = 0;
    } else {
        for (uint64_t w = threadIdx.x; w < sl.bm_words; w += kT2Block) sl.bm[w] = 0;
    }
    __syncthreads();
}

// tier1_walk by the whole workgroup.  Ends behind a barrier; s.pos is the size.
template <bool kWrite>
__device__ __forceinline__ Walk tier2_walk(const Graph &x, uint32_t r, uint32_t depth, const Slot &sl, T2Lds &s,
                                           const TreeOut &o, unsigned long long base) {
    const Rows &g = x.g;
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        s.sp = 1, s.v = r, s.off = 0, s.seen = 0, s.host = 0, s.pos = 1;
        sl.stack[0] = r;
        if (kWrite) put(o, base, r, row_len(g, r));
    }
    __syncthreads();
    if (tid == 0) t2_mark(sl, s, r);
    for (;;) {
        __syncthreads();  // the state as the last step left it
        const uint32_t sp = s.sp, v = s.v, off = s.off;
        const unsigned long long pos = s.pos;
        const bool host = s.host;  // (read here and written only behind the step's next barrier: uniform)
        if (host || !sp) break;
        uint64_t b, e;
        row_bounds(g, v, b, e);
        const uint32_t len = (uint32_t)(e - b);
        if (off >= len) {     // pop
            __syncthreads();  // everyone has read the state
            if (tid == 0) {
                s.sp = sp - 1;
                if (sp > 1) s.v = sl.stack[2 * (sp - 2)], s.off = sl.stack[2 * (sp - 2) + 1];
            }
            continue;
        }
        const uint32_t cnt = len - off < kT2Block ? len - off : kT2Block;
        const uint32_t u = tid < cnt ? g.col[b + off + tid] : kEmpty;
        const uint32_t ulen = u < g.Nx ? row_len(g, u) : 0;
        const bool has_row = ulen > 0, bad = is_bad(x, u);
        if (depth - sp == 1) {
            const bool fresh = has_row && t2_mark(sl, s, u);
            if (kWrite && tid < cnt) put(o, base + pos + tid, u, 0);
            __syncthreads();  // everyone has read the state
            if (bad && (!has_row || fresh)) s.host = 1;
            if (tid == 0) s.off = off + cnt, s.pos = pos + cnt;
            continue;
        }
        const bool cand = has_row && !(sl.bm[u >> 5] >> (u & 31) & 1);
        const unsigned long long fresh = __ballot(cand);
        if (lane == 0) s.first[wave] = fresh ? wave * 64 + (uint32_t)__ffsll((long long)fresh) - 1 : kNoLane;
        __syncthreads();  // ... and everyone has read the state
        uint32_t k = kNoLane;
        for (uint32_t w = 0; w < kT2Block / 64; w++) k = s.first[w] < k ? s.first[w] : k;
        const uint32_t leaves = k < cnt ? k : cnt;
        if (bad && ((tid < leaves && !has_row) || tid == k)) s.host = 1;
        if (kWrite && tid < leaves) put(o, base + pos + tid, u, 0);
        if (tid == k) {  // open u: the frame below keeps where it goes on
            t2_mark(sl, s, u);
            if (kWrite) put(o, base + pos + k, u, ulen);
            sl.stack[2 * (sp - 1) + 1] = off + k + 1;
            sl.stack[2 * sp] = u;  // (at most one frame per node that has a row)
            s.sp = sp + 1, s.v = u, s.off = 0, s.pos = pos + k + 1;
        }
        if (k == kNoLane && tid == 0) s.off = off + cnt, s.pos = pos + cnt;
    }
    __syncthreads();  // everyone has read the end of the walk
    return s.host ? kHost : kDone;
}

// tier 2's request, by the whole workgroup (tier 1 sends roots that have a row and depth >= 2)
__device__ __forceinline__ void tier2_tree(const Graph &x, uint32_t r, uint32_t depth, uint32_t i, const Slot &sl,
                                           T2Lds &s, unsigned long long *s_base, const TreeOut &o) {
    if (r >= x.g.Nx || depth < 2) return;
    const Walk w = tier2_walk<false>(x, r, depth, sl, s, o, 0);
    const unsigned long long total = s.pos;
    t2_clear(sl, s);
    if (threadIdx.x == 0) {
        if (w == kHost) {
            no_tree(o, i, 0, KETOGPU_EXPAND_HOST);
            *s_base = KETOGPU_LOOKUP_TRUNCATED;
        } else {
            *s_base = reserve(o.l, i, total);
            o.status[i] = KETOGPU_EXPAND_OK;
        }
    }
    __syncthreads();
    const unsigned long long base = *s_base;
    if (base == KETOGPU_LOOKUP_TRUNCATED) return;
    tier2_walk<true>(x, r, depth, sl, s, o, base);
    t2_clear(sl, s);
}

}  // namespace expand
}  // namespace ketogpu

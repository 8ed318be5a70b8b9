// subjects.hip — subject listing on the device (include/ketogpu.h ketogpu_subjects_*).
//
// subjects(r, C) lists F(r), the nodes reached from r in >= 1 edge over the rows the check
// engine sees, restricted to the class C: the least set that holds row(r) and row(x) for every
// interior x in it (DESIGN.md "Subject listing").  The rows live in HBM as a compact CSR over
// the expandable nodes (fwd_off / fwd_col), built at upload from the snapshot's host rows; they
// are neither sorted nor deduplicated, the sets below dedup.  Only interior entries (ids < Ni)
// have rows that can be reached, so only they are put on a worklist.  Two kernels:
//
//   tier 1  one wave per request.  F(r) lives in an LDS open-addressing set (insert by LDS
//           compare-and-swap) that is visited set and result at once; the interior members
//           also go on an LDS worklist.  Rows are read 64 entries per step.  A request whose
//           set passes kSetCap is appended to the overflow list and leaves no output.
//   tier 2  one workgroup per overflow request, `slots` requests per launch.  Each slot has a
//           bitmap over all N nodes, a worklist of Ni entries and a seen list of `list_cap`
//           entries in global memory; a level loop with __syncthreads() runs the closure to
//           its end whatever its size.  Every first visit is counted and, while there is room,
//           appended to the seen list.  A closure that stayed within list_cap finishes BY LIST
//           (count, reserve, write and clear the bitmap by walking the list: 4 bytes per
//           member); a larger one finishes BY SCAN of the bitmap (two passes over N / 8 bytes
//           whatever the answer is).
//
// Both tiers end the same way: count the members of class C, reserve exactly that many ids of
// `out` with one device-scope atomicAdd on a cursor, and write the list with plain vector
// stores if it fits below `capacity` (else begin = TRUNCATED; the count is exact either way).
//
// The paged call (ketogpu_subjects_page) runs the same two closures (tier1_closure, tier2_closure: one
// implementation each, called by the full-list and the paged kernel) and ends with the ordered
// finish of paged_finish.hpp instead: the `limit` smallest members >= from[i] to the stride
// out + i * limit, ascending, with the exact count and what remains; no cursor, no truncation.
//
// Every index is validated before it is used: roots against N, and against Nx before fwd_off
// is touched; row entries against N before the class array or a bitmap is.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>

#include "hip_host.hpp"
#include "paged_finish.hpp"
#include "subjects.hpp"

using namespace ketogpu;

namespace {

constexpr uint32_t kSetCap = 1024;           // tier 1: nodes a set may hold (ketogpu_subjects_stats.set_capacity)
constexpr uint32_t kSlotsLds = 2 * kSetCap;  // hash slots: a load of at most (kSetCap + 64) / kSlotsLds
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr unsigned kT2Block = 256;
static_assert(kT2Block == paged::kBlock, "the paged selection assumes tier 2's workgroup");
constexpr uint32_t kListCapDefault = 65536;  // tier 2: 256 KiB of seen list per slot

struct SGraph {
    const uint64_t *fwd_off;     // Nx + 1
    const uint32_t *fwd_col;
    const uint32_t *node_class;  // N
    uint32_t N, Nx, Ni;
};

struct SOut {
    uint32_t *out;
    unsigned long long capacity;
    unsigned long long *begin, *count;
    unsigned long long *cursor;  // ids reserved so far: ends at `needed`
    unsigned long long *truncated;
    unsigned long long *list_finishes, *scan_finishes;
};

__device__ inline bool class_ok(const SGraph &g, uint32_t u, uint32_t want) {
    if (u >= g.N) return false;
    const uint32_t c = g.node_class[u];
    return want == KETOGPU_TYPE_ANY
               ? c != KETOGPU_TYPE_NONE
               : (want != KETOGPU_TYPE_NONE && want != KETOGPU_CLASS_UNTYPED_SET && c == want);
}

__device__ inline uint32_t slot_of(uint32_t u) { return (u * 0x9E3779B1u) >> 21; }  // 11 bits
static_assert(kSlotsLds == 1u << 11, "slot_of yields 11 bits");

// ---------------------------------------------------------------------- tier 1
// tier 1's closure, by one wave: F(r) into `set` (all kSlotsLds slots are initialised here), its
// interior members through `work`.  False when the set passed kSetCap: the request overflows.
__device__ __forceinline__ bool tier1_closure(const SGraph &g, uint32_t r, uint32_t lane, uint32_t *set,
                                              uint32_t *work) {
    for (uint32_t s = lane; s < kSlotsLds; s += 64) set[s] = kEmpty;
    __syncthreads();
    uint32_t size = 0, head = 0, tail = 0;  // wave-uniform
    bool over = false;
    uint32_t v = r;
    for (;;) {
        const uint64_t b = g.fwd_off[v], e = g.fwd_off[v + 1];
        for (uint64_t base = b; base < e && !over; base += 64) {
            const uint64_t j = base + lane;
            const uint32_t u = j < e ? g.fwd_col[j] : kEmpty;
            bool fresh = false;
            if (u < g.N) {  // (also drops kEmpty) — the set never holds more than kSetCap + 64 of
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

__global__ __launch_bounds__(64) void subjects_tier1_kernel(SGraph g, const uint32_t *roots, uint32_t n, uint32_t cls,
                                                            int force_tier2, SOut o, uint32_t *ovf_list,
                                                            unsigned int *ovf_count) {
    __shared__ uint32_t set[kSlotsLds];
    __shared__ uint32_t work[kSetCap + 64];
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const uint32_t r = roots[i];
    if (r >= g.Nx) {  // NONE and the never-expanded nodes: the empty list; an id outside the snapshot: INVALID
        if (lane == 0) {
            o.begin[i] = (r < g.N || r == KETOGPU_NODE_NONE) ? 0ull : KETOGPU_LOOKUP_INVALID;
            o.count[i] = 0;
        }
        return;
    }
    if (force_tier2) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    const bool over = !tier1_closure(g, r, lane, set, work);
    if (over) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    uint32_t cnt = 0;
    for (uint32_t s = lane; s < kSlotsLds; s += 64) cnt += __popcll(__ballot(class_ok(g, set[s], cls)));
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
        const bool m = class_ok(g, u, cls);
        const unsigned long long mm = __ballot(m);
        if (m) o.out[base + w + __popcll(mm & ((1ull << lane) - 1))] = u;
        w += __popcll(mm);
    }
}

// ---------------------------------------------------------------------- tier 2
// tier 2's closure, by the whole workgroup: F(r) into the slot's bitmap `bm` (all zero on entry),
// its interior members through the worklist `wl`; every first visit is counted in *s_seen and,
// while there is room, appended to `seen`.  *s_tail and *s_seen are LDS counters, zero on entry
// and published by a barrier.  Ends behind a barrier: every thread sees the whole state.
__device__ __forceinline__ void tier2_closure(const SGraph &g, uint32_t r, uint32_t *bm, uint32_t *wl, uint32_t *seen,
                                              uint32_t list_cap, unsigned int *s_tail, unsigned int *s_seen) {
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = kT2Block / 64;
    auto visit = [&](uint32_t u) {
        if (u >= g.N) return;
        const uint32_t bit = 1u << (u & 31);
        if (atomicOr(&bm[u >> 5], bit) & bit) return;
        const uint32_t k = atomicAdd(s_seen, 1u);  // every first visit is counted
        if (k < list_cap) seen[k] = u;
        if (u < g.Ni) wl[atomicAdd(s_tail, 1u)] = u;  // each interior node enters once: <= Ni entries
    };
    {  // the root's own row, by the whole workgroup
        const uint64_t b = g.fwd_off[r], e = g.fwd_off[r + 1];
        for (uint64_t j = b + tid; j < e; j += kT2Block) visit(g.fwd_col[j]);
    }
    __syncthreads();
    uint32_t lb = 0, le = *s_tail;
    while (lb < le) {  // one level: a wave per row
        __syncthreads();  // everyone has read s_tail before it moves
        for (uint32_t k = lb + wave; k < le; k += nwaves) {
            const uint32_t v = wl[k];
            const uint64_t b = g.fwd_off[v], e = g.fwd_off[v + 1];
            for (uint64_t j = b + lane; j < e; j += 64) visit(g.fwd_col[j]);
        }
        __syncthreads();
        lb = le;
        le = *s_tail;
    }
}

// Block s of round r serves overflow request ovf_list[first + s] with slot s's state.  The
// bitmap is all zero on entry and is cleared again on the way out, by either finish.
__global__ __launch_bounds__(kT2Block) void subjects_tier2_kernel(SGraph g, const uint32_t *roots, uint32_t cls, SOut o,
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
    tier2_closure(g, r, bm, wl, seen, list_cap, &s_tail, &s_seen);
    const uint32_t total = s_seen;
    const bool by_list = list_cap && total <= list_cap;  // the seen list holds the whole closure
    // count the members of the class
    uint32_t c = 0;
    if (by_list) {
        for (uint32_t k = tid; k < total; k += kT2Block) {
            const uint32_t u = seen[k];
            c += class_ok(g, u, cls);
            bm[u >> 5] = 0;  // every set bit of the word is some member's: all of them store the same zero
        }
    } else {
        for (uint64_t w = tid; w < bm_words; w += kT2Block) {
            uint32_t bits = bm[w];
            while (bits) {
                const uint32_t u = (uint32_t)(w << 5) + (uint32_t)__ffs(bits) - 1;
                bits &= bits - 1;
                c += class_ok(g, u, cls);
            }
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
        atomicAdd(by_list ? o.list_finishes : o.scan_finishes, 1ull);
        s_base = fits ? base : KETOGPU_LOOKUP_TRUNCATED;
    }
    __syncthreads();
    const unsigned long long base = s_base;
    if (by_list) {
        if (base == KETOGPU_LOOKUP_TRUNCATED) return;
        for (uint32_t k0 = 0; k0 < total; k0 += kT2Block) {  // (a uniform trip count: the ballot sees whole waves)
            const uint32_t k = k0 + tid;
            const uint32_t u = k < total ? seen[k] : kEmpty;
            const bool m = class_ok(g, u, cls);
            const unsigned long long mm = __ballot(m);
            uint32_t p = 0;
            if (lane == 0 && mm) p = atomicAdd(&s_pos, (unsigned)__popcll(mm));
            p = __shfl(p, 0);
            if (m) o.out[base + p + __popcll(mm & ((1ull << lane) - 1))] = u;
        }
        return;
    }
    for (uint64_t w = tid; w < bm_words; w += kT2Block) {
        uint32_t bits = bm[w];
        if (!bits) continue;
        bm[w] = 0;
        if (base == KETOGPU_LOOKUP_TRUNCATED) continue;
        uint32_t ids[32], k = 0;
        while (bits) {
            const uint32_t u = (uint32_t)(w << 5) + (uint32_t)__ffs(bits) - 1;
            bits &= bits - 1;
            if (class_ok(g, u, cls)) ids[k++] = u;
        }
        if (!k) continue;
        const uint32_t p = atomicAdd(&s_pos, k);
        for (uint32_t x = 0; x < k; x++) o.out[base + p + x] = ids[x];
    }
}

// ---------------------------------------------------------------------- paged finish
// The same closures with the ordered finish of paged_finish.hpp: request i reports count,
// remaining and returned, and writes its page to the stride out + i * limit.
__global__ __launch_bounds__(64) void subjects_page_tier1_kernel(SGraph g, const uint32_t *roots, const uint32_t *from,
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
    if (force_tier2 || !tier1_closure(g, r, lane, set, work)) {
        if (lane == 0) ovf_list[atomicAdd(ovf_count, 1u)] = i;
        return;
    }
    paged::page_finish_wave(set, kSlotsLds, lane, i, from[i], o, [&](uint32_t u) { return class_ok(g, u, cls); });
}

// Selection in id order first; then the members are counted and the bitmap cleared, by the
// seen list if it holds the whole closure and by one scan otherwise: the slot is left all zero
// for whichever kernel of the handle uses it next.
__global__ __launch_bounds__(kT2Block) void subjects_page_tier2_kernel(SGraph g, const uint32_t *roots,
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
    tier2_closure(g, r, bm, wl, seen, list_cap, &s_tail, &s_seen);
    const uint32_t total = s_seen;
    const bool by_list = list_cap && total <= list_cap;  // the seen list holds the whole closure
    const uint32_t lo = from[i];
    auto ok = [&](uint32_t u) { return class_ok(g, u, cls); };
    paged::page_select_block(bm, bm_words, lo, o.limit, o.out + (uint64_t)i * o.limit, s_wave, ok);
    __syncthreads();  // the selection has read the bitmap
    uint32_t c = 0, q = 0;
    if (by_list) {
        for (uint32_t k = tid; k < total; k += kT2Block) {
            const uint32_t u = seen[k];
            const bool m = ok(u);
            c += m;
            q += m && u >= lo;
            bm[u >> 5] = 0;  // every set bit of the word is some member's: all of them store the same zero
        }
    } else {
        for (uint64_t w = tid; w < bm_words; w += kT2Block) {
            uint32_t bits = bm[w];
            if (!bits) continue;
            bm[w] = 0;
            while (bits) {
                const uint32_t u = (uint32_t)(w << 5) + (uint32_t)__ffs(bits) - 1;
                bits &= bits - 1;
                const bool m = ok(u);
                c += m;
                q += m && u >= lo;
            }
        }
    }
    if (c) atomicAdd(&s_cnt, c);
    if (q) atomicAdd(&s_rem, q);
    __syncthreads();
    if (tid == 0) {
        o.count[i] = s_cnt;
        o.remaining[i] = s_rem;
        o.returned[i] = s_rem < o.limit ? s_rem : o.limit;
        atomicAdd(by_list ? list_finishes : scan_finishes, 1ull);
    }
}

}  // namespace

struct ketogpu_subjects {
    std::shared_ptr<Snapshot::ReaderLink> link;  // cleared when the snapshot is freed first
    int device = 0;
    uint64_t budget = 0;
    bool force_tier2 = false;
    uint32_t slot_cap = 0;  // KETOGPU_SUBJECTS_SLOTS (0: no cap)
    uint32_t list_cap = kListCapDefault;
    hipStream_t stream = nullptr;
    std::mutex mu;          // one call at a time per handle
    uint64_t version = ~0ull;
    SGraph g{};
    DBuf<uint64_t> d_off;
    DBuf<uint32_t> d_col, d_class, d_roots, d_ovf, d_out, d_bm, d_wl, d_seen;
    DBuf<unsigned long long> d_begin, d_count, d_ctr;  // d_ctr: cursor, truncated, overflow count, list / scan finishes
    DBuf<uint32_t> d_from, d_ret;      // paged calls: lower bounds, returned
    uint32_t slots = 0, slot_max = 0;  // tier 2: allocated slots; what budget and knob allow (0: not yet known)
    uint64_t bm_words = 0;
    std::vector<uint64_t> h_off;  // upload staging
    std::vector<uint32_t> h_col;
    ketogpu_subjects_stats st{};

    // the rows and classes of the snapshot's current version (caller holds its shared lock):
    // the first `len` entries of every expandable node's row, packed back to back
    void upload(const Snapshot &s) {
        if (s.has_ambiguous)
            throw Error(KETOGPU_EINVAL, "subject listing: the snapshot has shared Subject.String() keys (R4)");
        auto classes = class_index_of(s);
        h_off.assign((size_t)s.Nx + 1, 0);
        for (uint32_t v = 0; v < s.Nx; v++) h_off[v + 1] = h_off[v] + s.node_row[v].len;
        h_col.resize(h_off[s.Nx]);
        for (uint32_t v = 0; v < s.Nx; v++)
            if (s.node_row[v].len) memcpy(h_col.data() + h_off[v], s.row_ptr(v), (size_t)s.node_row[v].len * 4);
        d_off.need(h_off.size());
        d_col.need(h_col.size());
        d_class.need(classes->node_class.size());
        HIP_CHECK(hipMemcpyAsync(d_off.p, h_off.data(), h_off.size() * 8, hipMemcpyHostToDevice, stream));
        if (!h_col.empty())
            HIP_CHECK(hipMemcpyAsync(d_col.p, h_col.data(), h_col.size() * 4, hipMemcpyHostToDevice, stream));
        if (!classes->node_class.empty())
            HIP_CHECK(hipMemcpyAsync(d_class.p, classes->node_class.data(), classes->node_class.size() * 4,
                                     hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        std::vector<uint32_t>().swap(h_col);  // (the larger staging array is not kept between uploads)
        if (s.N != g.N || s.Ni != g.Ni) slots = 0, slot_max = 0, d_bm.drop(), d_wl.drop(), d_seen.drop();  // tier 2's state follows the sizes
        g = SGraph{d_off.p, d_col.p, d_class.p, s.N, s.Nx, s.Ni};
        version = s.version;
        st.uploads++;
    }

    // tier 2's state: as many slots as the batch at hand can use, within what the budget allows
    // (at least one); a later batch with more overflows allocates again
    void need_slots(uint32_t wanted) {
        const uint64_t bmw = std::max<uint64_t>(((uint64_t)g.N + 31) / 32, 1), wlw = std::max<uint32_t>(g.Ni, 1),
                       snw = std::max<uint32_t>(list_cap, 1);
        if (!slot_max) {
            bm_words = ((uint64_t)g.N + 31) / 32;
            const uint64_t per = (bmw + wlw + snw) * 4;
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
        d_bm.need(k * bmw);
        d_wl.need(k * wlw);
        d_seen.need(k * snw);
        HIP_CHECK(hipMemsetAsync(d_bm.p, 0, k * bmw * 4, stream));
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
        if (!sp) throw Error(KETOGPU_EINVAL, "subject listing: the snapshot was freed");
        std::shared_lock<std::shared_mutex> rd(sp->mu);
        if (sp->version != version) upload(*sp);
    }

    void run(const uint32_t *roots, size_t n, uint32_t cls, uint32_t *out, uint64_t capacity, uint64_t *begin,
             uint64_t *count, uint64_t *needed) {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_CHECK(hipSetDevice(device));
        refresh();
        *needed = 0;
        st.requests += n;
        if (n) {
            d_roots.need(n), d_ovf.need(n), d_begin.need(n), d_count.need(n), d_ctr.need(8), d_out.need(capacity);
            HIP_CHECK(hipMemcpyAsync(d_roots.p, roots, n * 4, hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, 8 * sizeof(unsigned long long), stream));
            SOut o{d_out.p, capacity, d_begin.p, d_count.p, d_ctr.p, d_ctr.p + 1, d_ctr.p + 3, d_ctr.p + 4};
            unsigned int *ovf_count = (unsigned int *)(d_ctr.p + 2);
            KLAUNCH(subjects_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_roots.p, (uint32_t)n, cls,
                    force_tier2 ? 1 : 0, o, d_ovf.p, ovf_count);
            unsigned long long ctr[8];
            HIP_CHECK(hipMemcpyAsync(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            const uint32_t ovf = (uint32_t)(ctr[2] & 0xFFFFFFFFu);
            if (ovf) {
                need_slots(ovf);
                for (uint32_t first = 0; first < ovf; first += slots) {
                    const uint32_t k = std::min<uint32_t>(slots, ovf - first);
                    KLAUNCH(subjects_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_roots.p, cls, o, d_ovf.p,
                            first, d_bm.p, bm_words, d_wl.p, d_seen.p, list_cap);
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
            uint64_t unlisted = 0;  // INVALID and NONE roots belong to neither tier
            for (size_t i = 0; i < n; i++) unlisted += begin[i] == KETOGPU_LOOKUP_INVALID || roots[i] == NONE;
            st.tier1_requests += n - ovf - unlisted;
            st.list_finishes += ctr[3];
            st.scan_finishes += ctr[4];
            st.ids_produced += ctr[0];
            st.truncated_lists += ctr[1];
        }
        st.last_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }

    // the paged call: run() with the ordered finish.  `from` may be null (all zero).
    void run_page(const uint32_t *roots, const uint32_t *from, size_t n, uint32_t cls, uint32_t limit, uint32_t *out,
                  uint32_t *returned, uint64_t *count, uint64_t *remaining) {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_CHECK(hipSetDevice(device));
        refresh();
        st.requests += n;
        if (n) {
            d_roots.need(n), d_from.need(n), d_ovf.need(n), d_ret.need(n), d_begin.need(n), d_count.need(n),
                d_ctr.need(8), d_out.need(n * (size_t)limit);
            HIP_CHECK(hipMemcpyAsync(d_roots.p, roots, n * 4, hipMemcpyHostToDevice, stream));
            if (from)
                HIP_CHECK(hipMemcpyAsync(d_from.p, from, n * 4, hipMemcpyHostToDevice, stream));
            else
                HIP_CHECK(hipMemsetAsync(d_from.p, 0, n * 4, stream));
            HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, 8 * sizeof(unsigned long long), stream));
            paged::PageOut o{d_out.p, limit, d_ret.p, d_count.p, d_begin.p};  // (d_begin holds `remaining`)
            unsigned int *ovf_count = (unsigned int *)(d_ctr.p + 2);
            KLAUNCH(subjects_page_tier1_kernel, dim3((unsigned)n), dim3(64), 0, stream, g, d_roots.p, d_from.p,
                    (uint32_t)n, cls, force_tier2 ? 1 : 0, o, d_ovf.p, ovf_count);
            unsigned long long ctr[8];
            HIP_CHECK(hipMemcpyAsync(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            const uint32_t ovf = (uint32_t)(ctr[2] & 0xFFFFFFFFu);
            if (ovf) {
                need_slots(ovf);
                for (uint32_t first = 0; first < ovf; first += slots) {
                    const uint32_t k = std::min<uint32_t>(slots, ovf - first);
                    KLAUNCH(subjects_page_tier2_kernel, dim3(k), dim3(kT2Block), 0, stream, g, d_roots.p, d_from.p, cls,
                            o, d_ctr.p + 3, d_ctr.p + 4, d_ovf.p, first, d_bm.p, bm_words, d_wl.p, d_seen.p, list_cap);
                    st.tier2_rounds++;
                }
                HIP_CHECK(hipMemcpyAsync(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
            }
            HIP_CHECK(hipMemcpyAsync(returned, d_ret.p, n * 4, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(count, d_count.p, n * 8, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(remaining, d_begin.p, n * 8, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipMemcpyAsync(out, d_out.p, n * (size_t)limit * 4, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            st.tier2_requests += ovf;
            uint64_t unlisted = 0, produced = 0;  // INVALID and NONE roots belong to neither tier
            for (size_t i = 0; i < n; i++) {
                unlisted += returned[i] == KETOGPU_PAGE_INVALID || roots[i] == NONE;
                produced += returned[i] == KETOGPU_PAGE_INVALID ? 0 : returned[i];
            }
            st.tier1_requests += n - ovf - unlisted;
            st.list_finishes += ctr[3];
            st.scan_finishes += ctr[4];
            st.ids_produced += produced;
        }
        st.last_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }

    ~ketogpu_subjects() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream), (void)hipStreamDestroy(stream);
        d_off.drop(), d_col.drop(), d_class.drop(), d_roots.drop(), d_ovf.drop(), d_out.drop(), d_bm.drop(), d_wl.drop();
        d_seen.drop(), d_begin.drop(), d_count.drop(), d_ctr.drop(), d_from.drop(), d_ret.drop();
    }
};

extern "C" {

int ketogpu_subjects_new(const ketogpu_snapshot *sp, const ketogpu_subjects_opts *opts, ketogpu_subjects **out) {
    if (!sp || !out) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    *out = nullptr;
    return guarded([&] {
        const Snapshot &s = *reinterpret_cast<const Snapshot *>(sp);
        auto h = std::make_unique<ketogpu_subjects>();
        h->device = opts ? opts->device : 0;
        h->budget = opts ? opts->state_budget_bytes : 0;
        if (const char *e = getenv("KETOGPU_SUBJECTS_TIER")) h->force_tier2 = atoi(e) == 2;
        if (const char *e = getenv("KETOGPU_SUBJECTS_SLOTS")) h->slot_cap = (uint32_t)std::max(atoi(e), 0);
        if (const char *e = getenv("KETOGPU_SUBJECTS_LIST_CAP"))
            h->list_cap = (uint32_t)std::min<long long>(std::max<long long>(atoll(e), 0), 1ll << 28);
        h->st.set_capacity = kSetCap;
        h->st.list_capacity = h->list_cap;
        h->link = s.link;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || h->device < 0 || h->device >= ndev)
            throw Error(KETOGPU_EDEVICE, "subject listing: no such HIP device");
        HIP_CHECK(hipSetDevice(h->device));
        HIP_CHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        std::shared_lock<std::shared_mutex> rd(s.mu);
        h->upload(s);
        {
            std::lock_guard<std::mutex> lk(s.link->mu);
            s.link->snap = &s;  // the way back to the snapshot; its destructor clears it
        }
        *out = h.release();
    });
}

void ketogpu_subjects_free(ketogpu_subjects *h) { delete h; }

int ketogpu_subjects_stats_get(const ketogpu_subjects *h, ketogpu_subjects_stats *out) {
    if (!h || !out) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    std::lock_guard<std::mutex> lk(const_cast<ketogpu_subjects *>(h)->mu);
    *out = h->st;
    return KETOGPU_OK;
}

int ketogpu_subjects_ids(ketogpu_subjects *h, const uint32_t *roots, size_t n, uint32_t cls, uint32_t *out,
                         uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *needed) {
    if (!h || !needed || (n && (!roots || !begin || !count)) || (capacity && !out)) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    if (n >= (1ull << 31)) {
        set_last_error("subject listing: more than 2^31 - 1 roots in one call");
        return KETOGPU_EINVAL;
    }
    return guarded([&] {
        std::lock_guard<std::mutex> lk(h->mu);
        h->run(roots, n, cls, out, capacity, begin, count, needed);
    });
}

int ketogpu_subjects_page(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *from, size_t n, uint32_t cls,
                          uint32_t limit, uint32_t *out, uint32_t *returned, uint64_t *count, uint64_t *remaining) {
    if (!h || (n && (!roots || !out || !returned || !count || !remaining))) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    if (!limit || limit > KETOGPU_PAGE_LIMIT_MAX) {
        set_last_error("subject listing: a page limit outside [1, KETOGPU_PAGE_LIMIT_MAX]");
        return KETOGPU_EINVAL;
    }
    if (n >= (1ull << 31)) {
        set_last_error("subject listing: more than 2^31 - 1 roots in one call");
        return KETOGPU_EINVAL;
    }
    return guarded([&] {
        std::lock_guard<std::mutex> lk(h->mu);
        h->run_page(roots, from, n, cls, limit, out, returned, count, remaining);
    });
}

}  // extern "C"

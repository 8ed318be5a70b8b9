// hip_host.hpp — the host side shared by the listing handles (lookup.hip, subjects.hip): checked
// HIP calls and launches, a device array that only grows, the C ABI's error guard, and
// ListHandle: the state both handles carry, the drivers of their calls (tier 1, the read of the
// overflow count, tier 2 in rounds of `slots`, the copies back) and the shared parts of their
// ABI entry points, and how a handle follows in-place writes: the patched refresh (try_patch,
// list_patch_kernel) with the full upload as its fallback, and the wide tier's state and round
// (wide.hpp: need_wide_slots, wide_round, run_wide, run_page_wide).  A handle adds its graph struct, its
// upload, what the patched refresh asks of it, its launches (passed to the drivers as callables)
// and its statistics.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <string>
#include <vector>

#include "closure.hpp"
#include "ketogpu_internal.hpp"
#include "paged_finish.hpp"
#include "via.hpp"
#include "wide.hpp"

namespace ketogpu {

#define HIP_CHECK(x)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (x);                                                                           \
        if (_e != hipSuccess)                                                                          \
            throw Error(KETOGPU_EDEVICE, std::string(#x) + ": " + hipGetErrorString(_e));              \
    } while (0)

// every launch is checked: a failed launch must fail its call, not a later one
#define KLAUNCH(...)                                 \
    do {                                             \
        hipLaunchKernelGGL(__VA_ARGS__);             \
        HIP_CHECK(hipGetLastError());                \
    } while (0)

// a device array that only grows
template <class T>
struct DBuf {
    T *p = nullptr;
    size_t cap = 0;
    void need(size_t n) {
        if (n <= cap && p) return;
        if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
        void *q = nullptr;
        n = std::max<size_t>(n, 1);
        hipError_t e = hipMalloc(&q, n * sizeof(T));
        if (e != hipSuccess) throw Error(KETOGPU_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
        p = (T *)q, cap = n;
    }
    void drop() {
        if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
    }
};

// a pinned host array that only grows: the staging of a patched refresh
template <class T>
struct PBuf {
    T *p = nullptr;
    size_t cap = 0;
    void need(size_t n) {
        if (n <= cap && p) return;
        drop();
        void *q = nullptr;
        n = std::max<size_t>(n + n / 2, 1024);
        hipError_t e = hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) throw Error(KETOGPU_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
        p = (T *)q, cap = n;
    }
    void drop() {
        if (p) (void)hipHostFree(p);
        p = nullptr, cap = 0;
    }
};

// One segment of a patched refresh, four words: where its words go, where they lie in the
// staging array, how many there are, and (what << 32 | node).  kSegRow: a row copied into col
// where it lies already; kSegRowBounds: ... with off[node] and end[node] rewritten (the arena);
// kSegKeys: the filter keys of new nodes, copied into the key array.
constexpr uint64_t kSegRow = 0, kSegRowBounds = 1, kSegKeys = 2;
constexpr size_t kSegWords = 4;
constexpr unsigned kPatchBlock = 256;

// The scatter of a patched refresh: one workgroup per segment, grid-stride over the segments;
// consecutive threads copy consecutive words.  The host has checked every segment against the
// sizes of stage, col, off / end and key before the launch (ListHandle::try_patch).
static __global__ __launch_bounds__(kPatchBlock) void list_patch_kernel(const uint64_t *seg, uint64_t nseg,
                                                                        const uint32_t *stage, uint32_t *col,
                                                                        uint64_t *off, uint64_t *end, uint32_t *key) {
    for (uint64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const uint64_t dst = seg[kSegWords * s], src = seg[kSegWords * s + 1], len = seg[kSegWords * s + 2];
        const uint64_t what = seg[kSegWords * s + 3] >> 32;
        const uint32_t node = (uint32_t)seg[kSegWords * s + 3];
        uint32_t *to = what == kSegKeys ? key : col;
        for (uint64_t k = threadIdx.x; k < len; k += kPatchBlock) to[dst + k] = stage[src + k];
        if (what == kSegRowBounds && threadIdx.x == 0) off[node] = dst, end[node] = dst + len;
    }
}

template <class F>
int guarded(F &&f) {
    try {
        f();
        return KETOGPU_OK;
    } catch (const Error &e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc &) {
        set_last_error("out of host memory");
        return KETOGPU_ENOMEM;
    }
}

inline int einval(const std::string &msg) {
    set_last_error(msg);
    return KETOGPU_EINVAL;
}

// a call's device counters as read back: [0] the cursor, [1] truncated lists, [2] the overflow
// count (its low 32 bits), [3 ..] the handle's own
constexpr size_t kCtrs = 8;
struct Tally {
    unsigned long long ctr[kCtrs];
    uint32_t ovf;  // tier 2's requests
};

struct ListHandle {
    const std::string what;                      // the subsystem, as the error texts name it
    std::shared_ptr<Snapshot::ReaderLink> link;  // cleared when the snapshot is freed first
    int device = 0;
    uint64_t budget = 0;
    bool force_tier2 = false;
    uint32_t slot_cap = 0;  // the handle's SLOTS knob (0: no cap)
    hipStream_t stream = nullptr;
    std::mutex mu;  // one call at a time per handle
    std::chrono::steady_clock::time_point t0;  // when the call at hand began
    uint64_t version = ~0ull;
    uint64_t rows_epoch = 0;  // moves whenever the rows, their bounds or N / Nx changed on the device
    closure::Rows g{};      // the rows and per-node labels of the snapshot's current version
    DBuf<uint64_t> d_off;
    DBuf<uint32_t> d_col, d_label;
    DBuf<uint32_t> d_req, d_req2, d_ovf, d_out;  // d_req2: a call with pairs of ids (paths: the roots)
    DBuf<unsigned long long> d_begin, d_count, d_ctr;
    DBuf<uint32_t> d_from, d_ret;      // paged calls: lower bounds, returned
    DBuf<uint32_t> d_bm, d_wl;         // tier 2: a bitmap over `bound` and a worklist of Ni per slot
    DBuf<uint32_t> d_aux;              // ... and the handle's own (paths: parent words; subjects: seen lists)
    DBuf<uint32_t> d_bm2;              // combined calls: a second bitmap per slot
    DBuf<unsigned long long> d_front;  // depth calls: the frontier per request
    DBuf<uint32_t> d_via, d_hops;      // via calls: the arrays parallel to d_out
    DBuf<uint32_t> d_viast;            // ... and tier 2's parent and hop words: 2 x bound per slot
    DBuf<uint32_t> d_xstack;           // expand calls: tier 2's DFS stack, 2 x Nx words per slot
    uint32_t slots = 0, slot_max = 0;  // tier 2: allocated slots; what budget and knob allow (0: not yet known)
    uint32_t pair_slots = 0, pair_slot_max = 0;  // `slots` for combined calls: a slot has a second bitmap too
    uint32_t via_slots = 0, via_slot_max = 0;    // `slots` for via calls: a slot has parent and hop words too
    uint32_t expand_slots = 0, expand_slot_max = 0;  // `slots` for expand calls: a slot has a DFS stack too
    uint64_t expand_stack_words = 0;                 // ... of this many words
    // the wide tier (wide.hpp): the round's queue of work items and its counters; the bitmaps
    // are tier 2's.  The queue's size follows (Ni, col_words)
    DBuf<wide::Item> d_wq;
    DBuf<unsigned long long> d_wctr;
    PBuf<unsigned long long> h_wtail;  // the tail and the error word, as read behind each level
    uint32_t wide_slots = 0, wide_slot_max = 0;
    uint64_t wide_col_words = 0, wide_qcap = 0;
    ketogpu_wide_stats wst{};
    uint32_t bound = 0;                // the member bound the closures take: the bitmaps span it
    uint64_t bm_words = 0;

    // ---- following in-place writes (DESIGN.md "Listing handles and writes").  A handle over a
    // writable snapshot reads the snapshot's patch log from patch_pos on and rewrites the rows
    // it names (try_patch); upload_rows is the fallback, and the only path otherwise.
    ketogpu_list_refresh_stats rst{};
    bool refresh_full = false;    // KETOGPU_LIST_REFRESH=full: every version change uploads everything
    uint64_t slack_knob = ~0ull;  // KETOGPU_LIST_ARENA_SLACK: the arena's tail headroom in words (~0: the default)
    uint64_t garbage_knob = ~0ull;  // KETOGPU_LIST_ARENA_GARBAGE: the garbage words a patch may leave (~0: the default)
    // A handle whose bound follows N (subjects) sizes tier 2's bitmaps for N rounded up to a
    // multiple of this (KETOGPU_LIST_BOUND_STEP; at most 1024 more zero words per bitmap), so that
    // a write that adds a subject seldom moves the bound: dropping tier 2's state costs the next
    // tier-2 call its allocation and zeroing, which is proportional to slots x N
    uint32_t bound_step = 32768;
    uint32_t bound_above(uint32_t n) const {
        return (uint32_t)std::min<uint64_t>(((uint64_t)n + bound_step - 1) / bound_step * bound_step, 0xfffffffeu);
    }
    bool registered = false;      // a reader of the log, at patch_pos
    uint64_t patch_pos = 0;
    uint64_t n_rows = 0, col_words = 0, key_words = 0;  // the device arrays' sizes: segments are checked against them
    uint64_t full_bytes = 0;                            // what the last full upload copied
    // the arena (subjects handle, writable snapshots): row v lies at m_begin[v] with room for
    // m_cap[v] words; rows that outgrow it move to arena_tail, and their old words are garbage
    bool arena = false;
    std::vector<uint64_t> m_begin;
    std::vector<uint32_t> m_cap;
    uint64_t arena_tail = 0, arena_garbage = 0;
    DBuf<uint64_t> d_end, d_seg;
    DBuf<uint32_t> d_stage;
    PBuf<uint32_t> h_stage;  // the patched rows back to back, then the new nodes' keys
    PBuf<uint64_t> h_seg;
    std::vector<uint32_t> patch_nodes;  // (kept between refreshes: no allocation per write)

    explicit ListHandle(const char *subsystem) : what(subsystem) {}

    ~ListHandle() {
        if (registered && link) {  // (a snapshot freed first has cleared the link: nothing of it is touched)
            std::lock_guard<std::mutex> lk(link->mu);
            if (link->snap) link->snap->reader_gone(this);
        }
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream), (void)hipStreamDestroy(stream);
        d_end.drop(), d_seg.drop(), d_stage.drop(), h_stage.drop(), h_seg.drop();
        d_off.drop(), d_col.drop(), d_label.drop(), d_req.drop(), d_req2.drop(), d_ovf.drop(), d_out.drop();
        d_begin.drop(), d_count.drop(), d_ctr.drop(), d_from.drop(), d_ret.drop(), d_bm.drop(), d_wl.drop();
        d_aux.drop(), d_bm2.drop(), d_front.drop(), d_via.drop(), d_hops.drop(), d_viast.drop(), d_xstack.drop();
        d_wq.drop(), d_wctr.drop(), h_wtail.drop();
    }

    double ms_of_call() const {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }

    // tier 2's state follows (bound, Ni): dropped when they move
    void drop_tier2() {
        slots = 0, slot_max = 0, d_bm.drop(), d_wl.drop(), d_aux.drop();
        pair_slots = 0, pair_slot_max = 0, d_bm2.drop();
        via_slots = 0, via_slot_max = 0, d_viast.drop();
        expand_slots = 0, expand_slot_max = 0, d_xstack.drop();
        wide_slots = 0, wide_slot_max = 0, d_wq.drop(), d_wctr.drop();
    }

    // one version's rows and labels to the device, all of them: a full upload.  `end`: the rows'
    // ends when they lie in an arena (null: a dense CSR); col_room and label_room: the words
    // to allocate, at least what is copied.  The handle then stands at the log's end.  True when
    // (bound, Ni) moved, and tier 2's state, which follows the sizes, was dropped
    bool upload_rows(const Snapshot &s, const uint64_t *off, const uint64_t *end, size_t n_off, const uint32_t *col,
                     size_t n_col, size_t col_room, const uint32_t *label, size_t n_label, size_t label_room,
                     uint32_t new_bound) {
        col_room = std::max(col_room, n_col), label_room = std::max(label_room, n_label);
        d_off.need(n_off), d_col.need(col_room), d_label.need(label_room);
        if (end) d_end.need(n_off);
        HIP_CHECK(hipMemcpyAsync(d_off.p, off, n_off * 8, hipMemcpyHostToDevice, stream));
        if (end) HIP_CHECK(hipMemcpyAsync(d_end.p, end, (n_off - 1) * 8, hipMemcpyHostToDevice, stream));
        if (n_col) HIP_CHECK(hipMemcpyAsync(d_col.p, col, n_col * 4, hipMemcpyHostToDevice, stream));
        if (n_label) HIP_CHECK(hipMemcpyAsync(d_label.p, label, n_label * 4, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        const bool moved = new_bound != bound || s.Ni != g.Ni;
        if (moved) drop_tier2();
        g = closure::Rows{d_off.p, d_col.p, d_label.p, s.N, s.Nx, s.Ni, end ? d_end.p : nullptr};
        bound = new_bound, bm_words = ((uint64_t)bound + 31) / 32;
        version = s.version, rows_epoch++;
        n_rows = n_off - 1, col_words = col_room, key_words = label_room;
        full_bytes = (uint64_t)n_off * 8 * (end ? 2 : 1) + (uint64_t)n_col * 4 + (uint64_t)n_label * 4;
        rst.full_uploads++;
        if (s.writable && !refresh_full) {  // what the log holds so far is in these rows
            patch_pos = s.patch_end();
            s.reader_at(this, patch_pos);
            registered = true;
        }
        return moved;
    }

    // The patched refresh (caller holds the snapshot's shared lock): the rows of H::kPatchKind
    // that the log names from patch_pos on, packed into the pinned staging array from the
    // snapshot's current host rows, copied once with their segment table and scattered by
    // list_patch_kernel on the handle's stream, ahead of the call's kernels.  Host and device
    // work is O(the patched rows' entries + new nodes).  False: the handle must upload
    // everything instead (counted with its reason); nothing was changed then.
    // H supplies
    //   host_row(s, v, p, len, at)  the entries of row v, and where the row lies on the device
    //                               when that never moves (no arena)
    //   host_keys(s)                the filter keys of all N nodes when new nodes have one, else null
    //   bound_of(s)                 the member bound
    //   moved()                     (bound, Ni) moved: the handle's own tier-2 state goes too
    //   patched(s)                  a patched refresh succeeded: patch_nodes are the rows it rewrote
    template <class H>
    bool try_patch(const Snapshot &s, H &h) {
        if (!s.writable || refresh_full || !registered) return false;
        if (patch_pos < s.patch_base) {
            rst.fallbacks_trimmed++;
            return false;
        }
        patch_nodes.clear();
        for (uint64_t i = patch_pos; i < s.patch_end(); i++) {
            const Snapshot::Patch &pt = s.patches[i - s.patch_base];
            if (pt.kind == H::kPatchKind) patch_nodes.push_back(pt.node);
        }
        std::sort(patch_nodes.begin(), patch_nodes.end());
        patch_nodes.erase(std::unique(patch_nodes.begin(), patch_nodes.end()), patch_nodes.end());
        const uint32_t *keys = h.host_keys(s);
        if (s.N < g.N) throw Error(KETOGPU_EINVAL, what + ": the snapshot lost nodes in place");
        const uint64_t new_keys = keys ? s.N - g.N : 0;
        if (new_keys && g.N + new_keys > key_words) throw Error(KETOGPU_EINVAL, what + ": more nodes than the key array has room for");
        // the plan: where every row goes.  Nothing of the handle is changed before it is complete
        struct Move {
            uint32_t v, cap;
            uint64_t at;
        };
        std::vector<Move> moves;
        uint64_t words = 0, tail = arena_tail, garbage = arena_garbage;
        const size_t nseg = patch_nodes.size() + (new_keys ? 1 : 0);
        h_seg.need(kSegWords * std::max<size_t>(nseg, 1));
        for (size_t k = 0; k < patch_nodes.size(); k++) {
            const uint32_t v = patch_nodes[k];
            if (v >= n_rows) throw Error(KETOGPU_EINVAL, what + ": the log names a row the handle does not have");
            const uint32_t *p;
            uint64_t len, at;
            h.host_row(s, v, p, len, at);
            if (arena) {
                at = m_begin[v];
                if (len > m_cap[v]) {  // outgrown: to the tail, with the host's growth rule
                    const uint64_t cap = len + len / 4 + 4;
                    if (cap > 0xffffffffull || tail + cap > col_words) {
                        rst.compactions++;  // the tail is exhausted
                        return false;
                    }
                    at = tail, tail += cap, garbage += m_cap[v];
                    moves.push_back({v, (uint32_t)cap, at});
                }
            }
            if (at + len > col_words) throw Error(KETOGPU_EINVAL, what + ": a patched row ends outside the rows");
            uint64_t *sg = h_seg.p + kSegWords * k;
            sg[0] = at, sg[1] = words, sg[2] = len, sg[3] = (arena ? kSegRowBounds : kSegRow) << 32 | v;
            words += len;
        }
        const uint64_t garbage_max =
            garbage_knob != ~0ull ? garbage_knob : std::max<uint64_t>(s.stats.num_edges / 4, 1ull << 20);
        if (arena && garbage > garbage_max) {
            rst.compactions++;
            return false;
        }
        if (words * 4 > full_bytes / 4) {
            rst.fallbacks_backlog++;
            return false;
        }
        // (the staging arrays are free: every call ends with the stream drained, and an earlier
        // call that threw is waited for here)
        HIP_CHECK(hipStreamSynchronize(stream));
        h_stage.need(std::max<uint64_t>(words + new_keys, 1));
        for (size_t k = 0; k < patch_nodes.size(); k++) {
            const uint32_t *p;
            uint64_t len, at;
            h.host_row(s, patch_nodes[k], p, len, at);
            if (len) memcpy(h_stage.p + h_seg.p[kSegWords * k + 1], p, len * 4);
        }
        if (new_keys) {
            uint64_t *sg = h_seg.p + kSegWords * patch_nodes.size();
            sg[0] = g.N, sg[1] = words, sg[2] = new_keys, sg[3] = kSegKeys << 32;
            memcpy(h_stage.p + words, keys + g.N, new_keys * 4);
        }
        if (nseg) {
            d_stage.need(words + new_keys), d_seg.need(kSegWords * nseg);
            if (words + new_keys)
                HIP_CHECK(hipMemcpyAsync(d_stage.p, h_stage.p, (words + new_keys) * 4, hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(d_seg.p, h_seg.p, kSegWords * nseg * 8, hipMemcpyHostToDevice, stream));
            KLAUNCH(list_patch_kernel, dim3((unsigned)std::min<size_t>(nseg, 4096)), dim3(kPatchBlock), 0, stream, d_seg.p,
                    (uint64_t)nseg, d_stage.p, d_col.p, d_off.p, d_end.p, d_label.p);
        }
        for (const Move &m : moves) m_begin[m.v] = m.at, m_cap[m.v] = m.cap;
        arena_tail = tail, arena_garbage = garbage;
        g.N = s.N;
        const uint32_t new_bound = h.bound_of(s);
        if (new_bound != bound) {  // a new subject raised N: as upload_rows does
            drop_tier2();
            h.moved();
            bound = new_bound, bm_words = ((uint64_t)bound + 31) / 32;
        }
        patch_pos = s.patch_end();
        s.reader_at(this, patch_pos);
        version = s.version, rows_epoch++;
        rst.patched_refreshes++;
        rst.rows_patched += patch_nodes.size();
        rst.rows_moved += moves.size();
        rst.words_uploaded += words + new_keys + 2 * kSegWords * nseg;
        return true;
    }

    // the rows of the snapshot's current version: patched if a write moved it, or uploaded
    // again by the handle's upload(snapshot)
    template <class H>
    void refresh(H &h) {
        // (the link's lock is not held together with the snapshot's: a snapshot is not
        // freed while a call on it runs, only before or after)
        const Snapshot *sp;
        {
            std::lock_guard<std::mutex> lk(link->mu);
            sp = link->snap;
        }
        if (!sp) throw Error(KETOGPU_EINVAL, what + ": the snapshot was freed");
        std::shared_lock<std::shared_mutex> rd(sp->mu);
        if (sp->version == version) return;
        const auto r0 = std::chrono::steady_clock::now();
        if (try_patch(*sp, h))
            h.st.uploads++, h.patched(*sp);  // (+1 per version change seen, whichever path served it)
        else
            h.upload(*sp);
        rst.last_refresh_ms =
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - r0).count();
    }

    // how many slots of `words` words each serve `wanted` requests: the power of two >= wanted,
    // within what the budget, 1024 and the knob allow (kept in `max`), at least one
    uint32_t slots_for(uint32_t wanted, uint64_t words, uint32_t &max) {
        if (!max) {
            uint64_t b = budget;
            if (!b) {
                size_t fr = 0, tot = 0;
                HIP_CHECK(hipMemGetInfo(&fr, &tot));
                b = fr / 8;
            }
            max = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(b / (words * 4), 1), 1024);
            if (slot_cap) max = std::min(max, slot_cap);
        }
        uint64_t k = 1;
        while (k < wanted) k *= 2;
        return (uint32_t)std::min<uint64_t>(k, max);
    }

    // tier 2's state: as many slots as the batch at hand can use (a later batch with more
    // overflows allocates again).  `words`: what a slot takes in all, aux_words of them in d_aux
    // -> slots
    uint32_t need_slots(uint32_t wanted, uint64_t words, uint64_t aux_words) {
        const uint64_t k = slots_for(wanted, words, slot_max);
        if (k <= slots) return slots;
        slots = 0;  // (an allocation that fails below leaves no half-prepared state behind)
        d_bm.need(k * std::max<uint64_t>(bm_words, 1));
        d_wl.need(k * std::max<uint32_t>(g.Ni, 1));
        if (aux_words) d_aux.need(k * aux_words);
        HIP_CHECK(hipMemsetAsync(d_bm.p, 0, k * std::max<uint64_t>(bm_words, 1) * 4, stream));
        return slots = (uint32_t)k;
    }

    // tier 2's state for a combined call: need(k)'s slots (the handle's own need_slots: bitmaps,
    // worklists and whatever else its slots carry, `words` words in all) plus a second bitmap per
    // slot in d_bm2, zeroed here and left zero by every kernel; all of it counted against the
    // budget, so a combined round may have fewer slots
    template <class Need>
    uint32_t need_pair_slots(uint32_t wanted, uint64_t words, Need &&need) {
        const uint64_t b2w = std::max<uint64_t>(bm_words, 1);
        uint64_t k = slots_for(wanted, words + b2w, pair_slot_max);
        if (k <= pair_slots && pair_slots <= slots) return pair_slots;
        pair_slots = 0;
        k = std::min<uint64_t>(k, need((uint32_t)k));  // (at least one)
        d_bm2.need(k * b2w);
        HIP_CHECK(hipMemsetAsync(d_bm2.p, 0, k * b2w * 4, stream));
        return pair_slots = (uint32_t)k;
    }

    // tier 2's state for a via call: need(k)'s slots (the handle's own need_slots, `words` words
    // in all) plus a parent and a hop word per id below the bound in d_viast: 8 bytes x bound per
    // slot, counted against the budget with the rest, so a via round may have fewer slots.  The
    // words are never cleared: a bitmap bit says which of them hold.
    template <class Need>
    uint32_t need_via_slots(uint32_t wanted, uint64_t words, Need &&need) {
        const uint64_t vw = 2 * std::max<uint64_t>(bound, 1);
        uint64_t k = slots_for(wanted, words + vw, via_slot_max);
        if (k <= via_slots && via_slots <= slots) return via_slots;
        via_slots = 0;
        k = std::min<uint64_t>(k, need((uint32_t)k));  // (at least one)
        d_viast.need(k * vw);
        return via_slots = (uint32_t)k;
    }

    // tier 2's state for an expand call: need(k)'s slots (the handle's own need_slots, `words`
    // words in all) plus a DFS stack of two words per frame in d_xstack.  A frame is a node that
    // has a row and each is opened once, so 2 x Nx words per slot hold any walk; they are counted
    // against the budget with the rest, so an expand round may have fewer slots.  The words are
    // never cleared: the stack height says which of them hold.
    template <class Need>
    uint32_t need_expand_slots(uint32_t wanted, uint64_t words, Need &&need) {
        const uint64_t sw = 2 * std::max<uint64_t>(g.Nx, 1);
        if (sw != expand_stack_words) expand_slots = 0, expand_slot_max = 0;
        uint64_t k = slots_for(wanted, words + sw, expand_slot_max);
        if (k <= expand_slots && expand_slots <= slots) return expand_slots;
        expand_slots = 0;
        k = std::min<uint64_t>(k, need((uint32_t)k));  // (at least one)
        d_xstack.need(k * sw);
        expand_stack_words = sw;
        return expand_slots = (uint32_t)k;
    }

    // the wide tier's state: need(k)'s slots (the handle's own need_slots, `words` words in all:
    // the wide tier uses their bitmaps) plus the round's queue, wide::queue_items items of three
    // words, and its counters; all of it counted against the budget, so a wide round may have
    // fewer slots.  The queue is allocated again when col_words moved (an upload with more
    // edges); drop_tier2 drops it when (bound, Ni) move.  Neither is ever cleared: the tail says
    // which items hold, and a round zeroes its counters itself, the paged finish's `below` word
    // per slot among them (wide::round_words: full-list and paged rounds share this state).
    template <class Need>
    uint32_t need_wide_slots(uint32_t wanted, uint64_t words, Need &&need) {
        if (col_words != wide_col_words) wide_slots = 0, wide_slot_max = 0;
        const uint64_t per = 3 * wide::queue_items(1, g.Ni, col_words) + 2 * wide::kPerSlot;
        uint64_t k = slots_for(wanted, words + per, wide_slot_max);
        if (k <= wide_slots && wide_slots <= slots) return wide_slots;
        wide_slots = 0;
        k = std::min<uint64_t>(k, need((uint32_t)k));  // (at least one)
        wide_qcap = wide::queue_items(k, g.Ni, col_words);
        d_wq.need(wide_qcap), d_wctr.need(wide::round_words(k)), h_wtail.need(wide::kHead);
        wide_col_words = col_words;
        return wide_slots = (uint32_t)k;
    }

    // the queue's tail behind what is enqueued so far: the wide tier's one host wait per level
    unsigned long long wide_tail() {
        HIP_CHECK(hipMemcpyAsync(h_wtail.p, d_wctr.p, wide::kHead * 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        return h_wtail.p[wide::kTail];
    }

    // One round of the wide tier: the requests d_ovf[first .. first + k) with slots 0 .. k - 1.
    // rows: the ids below it have a row.  level(w, L, lb, le) launches the handle's level kernel
    // over the items [lb, le) as launch L of the round (1-based: the members at distance L);
    // finish(w) is either wide_reserve and the handle's write kernel or wide_page_finish.  The
    // seed is wide.hpp's own.  A depth call's frontier words are zero before the seed
    // (upload_depth; tier 1 writes only those of the requests it answers).  A queue that proved
    // too small fails the call before anything is written, bitmaps zeroed.
    template <class Level, class Finish>
    void wide_round(uint32_t first, uint32_t k, uint32_t rows, Level &&level, Finish &&finish) {
        const wide::State w{d_bm.p, bm_words, d_wq.p, wide_qcap, d_wctr.p, k, rows};
        HIP_CHECK(hipMemsetAsync(d_wctr.p, 0, wide::round_words(k) * 8, stream));
        KLAUNCH(wide::seed_kernel, dim3(k), dim3(64), 0, stream, g, d_req.p, d_ovf.p, first, w);
        unsigned long long lb = 0, le = wide_tail();
        for (uint32_t L = 1; lb < le && !h_wtail.p[wide::kError]; L++) {
            level(w, L, lb, le);
            wst.levels++, wst.items += le - lb;
            lb = le, le = wide_tail();
        }
        if (h_wtail.p[wide::kError]) {
            HIP_CHECK(hipMemsetAsync(d_bm.p, 0, (uint64_t)k * std::max<uint64_t>(bm_words, 1) * 4, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            throw Error(KETOGPU_EDEVICE, what + ": the wide tier's queue is too small for this round");
        }
        finish(w);
    }

    // the full-list finish's first half: every slot's count reserved for its request
    void wide_reserve(const wide::State &w, uint32_t first, uint64_t capacity) {
        KLAUNCH(wide::reserve_kernel, dim3((w.nslots + 63) / 64), dim3(64), 0, stream, d_ovf.p, first, w,
                list_out(capacity));
    }

    // the write kernel's grid: a workgroup per tile of one slot's bitmap
    dim3 wide_write_grid(uint32_t k) const {
        return dim3((unsigned)std::max<uint64_t>((bm_words + wide::kTile - 1) / wide::kTile, 1), k);
    }

    // ... and the paged finish's clear kernel's
    dim3 wide_clear_grid(uint32_t k) const {
        return dim3((unsigned)std::max<uint64_t>((bm_words + wide::kClearTile - 1) / wide::kClearTile, 1), k);
    }

    // the paged finish: select(w) and clear(w) launch the handle's kernels, each in a launch of
    // its own (the clear kernel stores over what the select reads); the report is wide.hpp's own
    template <class Select, class Clear>
    void wide_page_finish(const wide::State &w, uint32_t first, uint32_t limit, Select &&select, Clear &&clear) {
        select(w);
        clear(w);
        KLAUNCH(wide::page_final_kernel, dim3((w.nslots + 63) / 64), dim3(64), 0, stream, d_ovf.p, first, w,
                page_out(limit));
    }

    // a wide call, counted in wst: run_cursor with rounds of the wide tier in tier 2's place.
    // need(overflows) -> the slots of a round, round(first, k) one round
    template <class Unlisted, class T1, class Need, class Round>
    void run_wide(const uint32_t *req, size_t n, uint32_t *out, uint64_t capacity, uint64_t *begin, uint64_t *count,
                  uint64_t *needed, Unlisted &&unlisted, T1 &&tier1, Need &&need, Round &&round) {
        struct {  // (what run_cursor counts, under tier 2's names)
            uint64_t requests = 0, tier1_requests = 0, tier2_requests = 0, tier2_rounds = 0, ids_produced = 0,
                     truncated_lists = 0;
        } c;
        run_cursor(c, req, n, out, capacity, begin, count, needed, unlisted, tier1, need, round);
        wst.requests += c.requests, wst.tier1_requests += c.tier1_requests, wst.wide_requests += c.tier2_requests;
        wst.wide_rounds += c.tier2_rounds, wst.ids_produced += c.ids_produced;
        wst.truncated_lists += c.truncated_lists;
        wst.last_call_ms = ms_of_call();
    }

    // a wide paged call, counted in wst: run_page with rounds of the wide tier in tier 2's
    // place.  need and round as in run_wide; a page truncates nothing
    template <class T1, class Need, class Round>
    void run_page_wide(const uint32_t *req, const uint32_t *from, size_t n, uint32_t limit, uint32_t *out,
                       uint32_t *returned, uint64_t *count, uint64_t *remaining, T1 &&tier1, Need &&need,
                       Round &&round) {
        struct {  // (what run_page counts, under tier 2's names)
            uint64_t requests = 0, tier1_requests = 0, tier2_requests = 0, tier2_rounds = 0, ids_produced = 0;
        } c;
        run_page(c, req, from, n, limit, out, returned, count, remaining, tier1, need, round, [](Tally &) {});
        wst.requests += c.requests, wst.tier1_requests += c.tier1_requests, wst.wide_requests += c.tier2_requests;
        wst.wide_rounds += c.tier2_rounds, wst.ids_produced += c.ids_produced;
        wst.last_call_ms = ms_of_call();
    }

    // a via call's device arrays next to d_out, `words` each (null where the caller wants none)
    via::ViaOut via_out(const uint32_t *via, const uint32_t *hops, uint64_t words) {
        if (via) d_via.need(words);
        if (hops) d_hops.need(words);
        return {via ? d_via.p : nullptr, hops ? d_hops.p : nullptr};
    }

    // ... and their first `words` words back behind the call, with those of d_out where the
    // driver has not copied them (out null: it has)
    void read_via(uint32_t *out, uint32_t *via, uint32_t *hops, uint64_t words) {
        if (!words || (!out && !via && !hops)) return;
        if (out) HIP_CHECK(hipMemcpyAsync(out, d_out.p, words * 4, hipMemcpyDeviceToHost, stream));
        if (via) HIP_CHECK(hipMemcpyAsync(via, d_via.p, words * 4, hipMemcpyDeviceToHost, stream));
        if (hops) HIP_CHECK(hipMemcpyAsync(hops, d_hops.p, words * 4, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }

    // where the written lists of a cursor call end.  The cursor only grows, so once a list is
    // truncated every later reservation is: the written lists tile a prefix of `out`, and a via
    // call copies back exactly that prefix, so that no word outside a written list is touched
    static uint64_t written_end(const uint64_t *begin, const uint64_t *count, size_t n) {
        uint64_t end = 0;
        for (size_t i = 0; i < n; i++)
            if (begin[i] != KETOGPU_LOOKUP_TRUNCATED && begin[i] != KETOGPU_LOOKUP_INVALID)
                end = std::max<uint64_t>(end, begin[i] + count[i]);
        return end;
    }

    closure::ListOut list_out(uint64_t capacity) {
        return {d_out.p, capacity, d_begin.p, d_count.p, d_ctr.p, d_ctr.p + 1};
    }
    paged::PageOut page_out(uint32_t limit) {
        return {d_out.p, limit, d_ret.p, d_count.p, d_begin.p};  // (d_begin holds `remaining`)
    }

    // the counters to t.ctr: complete at the caller's next synchronise
    void read_ctrs(Tally &t) {
        HIP_CHECK(hipMemcpyAsync(t.ctr, d_ctr.p, sizeof t.ctr, hipMemcpyDeviceToHost, stream));
    }

    // both tiers of one call: tier1(overflow counter) launches over all requests; what it
    // appended to d_ovf runs as tier2(first, k) in rounds of need(overflows) slots, and
    // after(t) enqueues what the caller wants behind them (read_ctrs, if tier 2 moves counters
    // it reports: a call that does not need them does not pay for the copy)
    template <class Stats, class T1, class Need, class T2, class After>
    void run_tiers(Stats &st, Tally &t, T1 &&tier1, Need &&need, T2 &&tier2, After &&after) {
        HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, sizeof t.ctr, stream));
        tier1((unsigned int *)(d_ctr.p + 2));
        read_ctrs(t);
        HIP_CHECK(hipStreamSynchronize(stream));
        t.ovf = (uint32_t)(t.ctr[2] & 0xFFFFFFFFu);
        if (!t.ovf) return;
        const uint32_t per = need(t.ovf);
        for (uint32_t first = 0; first < t.ovf; first += per, st.tier2_rounds++)
            tier2(first, std::min<uint32_t>(per, t.ovf - first));
        after(t);
    }

    // what every call counts the same way.  unlisted: requests answered before any row was
    // read, which belong to neither tier
    template <class Stats>
    static void count_call(Stats &st, const Tally &t, size_t n, uint64_t unlisted, uint64_t produced) {
        st.tier2_requests += t.ovf;
        st.tier1_requests += n - t.ovf - unlisted;
        st.ids_produced += produced;
    }

    // a cursor call, counted in st: begin / count per request, *needed, then the min(cursor,
    // capacity) ids that were written (every written list ends below both).  unlisted(i): see
    // count_call.  -> the call's counters
    template <class Stats, class Unlisted, class T1, class Need, class T2>
    Tally run_cursor(Stats &st, const uint32_t *req, size_t n, uint32_t *out, uint64_t capacity, uint64_t *begin,
                     uint64_t *count, uint64_t *needed, Unlisted &&unlisted, T1 &&tier1, Need &&need, T2 &&tier2) {
        Tally t{};
        *needed = 0;
        st.requests += n;
        if (!n) return t;
        d_req.need(n), d_ovf.need(n), d_begin.need(n), d_count.need(n), d_ctr.need(kCtrs), d_out.need(capacity);
        HIP_CHECK(hipMemcpyAsync(d_req.p, req, n * 4, hipMemcpyHostToDevice, stream));
        run_tiers(st, t, tier1, need, tier2, [&](Tally &t) { read_ctrs(t); });  // (the cursor has moved)
        HIP_CHECK(hipMemcpyAsync(begin, d_begin.p, n * 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(count, d_count.p, n * 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        const uint64_t written = std::min<uint64_t>(t.ctr[0], capacity);
        if (written && out) {
            HIP_CHECK(hipMemcpyAsync(out, d_out.p, written * 4, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
        }
        *needed = t.ctr[0];
        uint64_t skipped = 0;
        for (size_t i = 0; i < n; i++) skipped += unlisted(i);
        count_call(st, t, n, skipped, t.ctr[0]);
        st.truncated_lists += t.ctr[1];
        return t;
    }

    // the second ids of a call with pairs of ids, to d_req2
    void upload_req2(const uint32_t *req2, size_t n) {
        if (!n) return;
        d_req2.need(n);
        HIP_CHECK(hipMemcpyAsync(d_req2.p, req2, n * 4, hipMemcpyHostToDevice, stream));
    }

    // a depth call's limits to d_req2 (null: no limit for any request, and the kernels are told
    // so by a null array), and its frontier words zeroed: a kernel writes the non-zero ones
    // -> the device array of limits
    const uint32_t *upload_depth(const uint32_t *max_depth, size_t n) {
        if (!n) return nullptr;
        d_front.need(n);
        HIP_CHECK(hipMemsetAsync(d_front.p, 0, n * 8, stream));
        if (!max_depth) return nullptr;
        upload_req2(max_depth, n);
        return d_req2.p;
    }

    // ... and the frontier back behind the call (`frontier` may be null) -> requests with a
    // non-zero frontier
    uint64_t read_frontier(uint64_t *frontier, size_t n) {
        if (!n) return 0;
        std::vector<uint64_t> mine;
        if (!frontier) mine.resize(n), frontier = mine.data();
        HIP_CHECK(hipMemcpyAsync(frontier, d_front.p, n * 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        uint64_t cut = 0;
        for (size_t i = 0; i < n; i++) cut += frontier[i] != 0;
        return cut;
    }

    // run_cursor for pairs (a[i], b[i]): a in d_req, b in d_req2
    template <class Stats, class Unlisted, class T1, class Need, class T2>
    Tally run_cursor(Stats &st, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *out, uint64_t capacity,
                     uint64_t *begin, uint64_t *count, uint64_t *needed, Unlisted &&unlisted, T1 &&tier1, Need &&need,
                     T2 &&tier2) {
        upload_req2(b, n);
        return run_cursor(st, a, n, out, capacity, begin, count, needed, unlisted, tier1, need, tier2);
    }

    // a paged call, counted in st (INVALID and NONE ids belong to neither tier).  `from` may be
    // null (all zero).  -> the call's counters
    template <class Stats, class T1, class Need, class T2, class After>
    Tally run_page(Stats &st, const uint32_t *req, const uint32_t *from, size_t n, uint32_t limit, uint32_t *out,
                   uint32_t *returned, uint64_t *count, uint64_t *remaining, T1 &&tier1, Need &&need, T2 &&tier2,
                   After &&after) {
        return run_page(
            st, req, from, n, limit, out, returned, count, remaining, [&](size_t i) { return req[i] == NONE; }, tier1,
            need, tier2, after);
    }

    // run_page for pairs (a[i], b[i]): a in d_req, b in d_req2
    template <class Stats, class Unlisted, class T1, class Need, class T2, class After>
    Tally run_page(Stats &st, const uint32_t *a, const uint32_t *b, const uint32_t *from, size_t n, uint32_t limit,
                   uint32_t *out, uint32_t *returned, uint64_t *count, uint64_t *remaining, Unlisted &&unlisted,
                   T1 &&tier1, Need &&need, T2 &&tier2, After &&after) {
        upload_req2(b, n);
        return run_page(st, a, from, n, limit, out, returned, count, remaining, unlisted, tier1, need, tier2, after);
    }

    // ... with unlisted(i): a valid request answered before any row was read (see count_call)
    template <class Stats, class Unlisted, class T1, class Need, class T2, class After>
    Tally run_page(Stats &st, const uint32_t *req, const uint32_t *from, size_t n, uint32_t limit, uint32_t *out,
                   uint32_t *returned, uint64_t *count, uint64_t *remaining, Unlisted &&unlisted, T1 &&tier1,
                   Need &&need, T2 &&tier2, After &&after) {
        Tally t{};
        st.requests += n;
        if (!n) return t;
        d_req.need(n), d_from.need(n), d_ovf.need(n), d_ret.need(n), d_begin.need(n), d_count.need(n);
        d_ctr.need(kCtrs), d_out.need(n * (size_t)limit);
        HIP_CHECK(hipMemcpyAsync(d_req.p, req, n * 4, hipMemcpyHostToDevice, stream));
        if (from)
            HIP_CHECK(hipMemcpyAsync(d_from.p, from, n * 4, hipMemcpyHostToDevice, stream));
        else
            HIP_CHECK(hipMemsetAsync(d_from.p, 0, n * 4, stream));
        run_tiers(st, t, tier1, need, tier2, after);
        HIP_CHECK(hipMemcpyAsync(returned, d_ret.p, n * 4, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(count, d_count.p, n * 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(remaining, d_begin.p, n * 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(out, d_out.p, n * (size_t)limit * 4, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        uint64_t skipped = 0, produced = 0;
        for (size_t i = 0; i < n; i++) {
            skipped += returned[i] == KETOGPU_PAGE_INVALID || unlisted(i);
            produced += returned[i] == KETOGPU_PAGE_INVALID ? 0 : returned[i];
        }
        count_call(st, t, n, skipped, produced);
        return t;
    }
};

// ---- the ABI entry points' shared parts.  H: a handle struct derived from ListHandle.

// ketogpu_*_new: h->upload(snapshot) is the handle's own; init(h) reads its further knobs
template <class H, class Opts, class Init>
int list_new(const ketogpu_snapshot *sp, const Opts *opts, H **out, const char *tier_knob, const char *slots_knob,
             Init &&init) {
    if (!sp || !out) return einval("null argument");
    *out = nullptr;
    return guarded([&] {
        const Snapshot &s = *reinterpret_cast<const Snapshot *>(sp);
        auto h = std::make_unique<H>();
        h->device = opts ? opts->device : 0;
        h->budget = opts ? opts->state_budget_bytes : 0;
        if (const char *e = getenv(tier_knob)) h->force_tier2 = atoi(e) == 2;
        if (const char *e = getenv(slots_knob)) h->slot_cap = (uint32_t)std::max(atoi(e), 0);
        if (const char *e = getenv("KETOGPU_LIST_REFRESH")) h->refresh_full = std::string(e) == "full";
        if (const char *e = getenv("KETOGPU_LIST_ARENA_SLACK")) h->slack_knob = strtoull(e, nullptr, 10);
        if (const char *e = getenv("KETOGPU_LIST_ARENA_GARBAGE")) h->garbage_knob = strtoull(e, nullptr, 10);
        if (const char *e = getenv("KETOGPU_LIST_BOUND_STEP"))
            h->bound_step = (uint32_t)std::min<unsigned long long>(std::max<unsigned long long>(strtoull(e, nullptr, 10), 1), 1u << 24);
        init(*h);
        h->wst.chunk = wide::kChunk;
        h->link = s.link;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || h->device < 0 || h->device >= ndev)
            throw Error(KETOGPU_EDEVICE, h->what + ": no such HIP device");
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

template <class H, class S>
int list_stats_get(const H *h, S H::*st, S *out) {
    if (!h || !out) return einval("null argument");
    std::lock_guard<std::mutex> lk(const_cast<H *>(h)->mu);
    *out = h->*st;
    return KETOGPU_OK;
}

// a call on a handle: the argument checks (`null`: a required pointer is missing; `noun`: what
// the n requests are; `limit`: a paged call's, else null), then f() under the handle's lock, on
// its device, over the current rows
template <class H, class F>
int list_call(H *h, bool null, size_t n, const char *noun, const uint32_t *limit, F &&f) {
    if (!h || null) return einval("null argument");
    if (limit && (!*limit || *limit > KETOGPU_PAGE_LIMIT_MAX))
        return einval(h->what + ": a page limit outside [1, KETOGPU_PAGE_LIMIT_MAX]");
    if (n >= (1ull << 31)) return einval(h->what + ": more than 2^31 - 1 " + noun + " in one call");
    return guarded([&] {
        std::lock_guard<std::mutex> lk(h->mu);
        h->t0 = std::chrono::steady_clock::now();
        HIP_CHECK(hipSetDevice(h->device));
        h->refresh(*h);
        f();
    });
}

}  // namespace ketogpu

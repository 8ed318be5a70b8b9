// hip_host.hpp — the host side shared by the listing handles (lookup.hip, subjects.hip): checked
// HIP calls and launches, a device array that only grows, the C ABI's error guard, and
// ListHandle: the state both handles carry, the drivers of their calls (tier 1, the read of the
// overflow count, tier 2 in rounds of `slots`, the copies back) and the shared parts of their
// ABI entry points.  A handle adds its graph struct, its upload, its launches (passed to the
// drivers as callables) and its statistics.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
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
    uint32_t slots = 0, slot_max = 0;  // tier 2: allocated slots; what budget and knob allow (0: not yet known)
    uint32_t pair_slots = 0, pair_slot_max = 0;  // `slots` for combined calls: a slot has a second bitmap too
    uint32_t via_slots = 0, via_slot_max = 0;    // `slots` for via calls: a slot has parent and hop words too
    uint32_t bound = 0;                // the member bound the closures take: the bitmaps span it
    uint64_t bm_words = 0;

    explicit ListHandle(const char *subsystem) : what(subsystem) {}

    ~ListHandle() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream), (void)hipStreamDestroy(stream);
        d_off.drop(), d_col.drop(), d_label.drop(), d_req.drop(), d_req2.drop(), d_ovf.drop(), d_out.drop();
        d_begin.drop(), d_count.drop(), d_ctr.drop(), d_from.drop(), d_ret.drop(), d_bm.drop(), d_wl.drop();
        d_aux.drop(), d_bm2.drop(), d_front.drop(), d_via.drop(), d_hops.drop(), d_viast.drop();
    }

    double ms_of_call() const {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }

    // one version's rows and labels to the device; true when (bound, Ni) moved, and tier 2's
    // state, which follows the sizes, was dropped
    bool upload_rows(const Snapshot &s, const uint64_t *off, size_t n_off, const uint32_t *col, size_t n_col,
                     const uint32_t *label, size_t n_label, uint32_t new_bound) {
        d_off.need(n_off), d_col.need(n_col), d_label.need(n_label);
        HIP_CHECK(hipMemcpyAsync(d_off.p, off, n_off * 8, hipMemcpyHostToDevice, stream));
        if (n_col) HIP_CHECK(hipMemcpyAsync(d_col.p, col, n_col * 4, hipMemcpyHostToDevice, stream));
        if (n_label) HIP_CHECK(hipMemcpyAsync(d_label.p, label, n_label * 4, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        const bool moved = new_bound != bound || s.Ni != g.Ni;
        if (moved) slots = 0, slot_max = 0, d_bm.drop(), d_wl.drop(), d_aux.drop();
        if (moved) pair_slots = 0, pair_slot_max = 0, d_bm2.drop();
        if (moved) via_slots = 0, via_slot_max = 0, d_viast.drop();
        g = closure::Rows{d_off.p, d_col.p, d_label.p, s.N, s.Nx, s.Ni};
        bound = new_bound, bm_words = ((uint64_t)bound + 31) / 32;
        version = s.version;
        return moved;
    }

    // the rows of the snapshot's current version, uploaded again (by the handle's
    // upload(snapshot)) if a write moved it
    template <class Upload>
    void refresh(Upload &&upload) {
        // (the link's lock is not held together with the snapshot's: a snapshot is not
        // freed while a call on it runs, only before or after)
        const Snapshot *sp;
        {
            std::lock_guard<std::mutex> lk(link->mu);
            sp = link->snap;
        }
        if (!sp) throw Error(KETOGPU_EINVAL, what + ": the snapshot was freed");
        std::shared_lock<std::shared_mutex> rd(sp->mu);
        if (sp->version != version) upload(*sp);
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
        init(*h);
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
        h->refresh([&](const Snapshot &s) { h->upload(s); });
        f();
    });
}

}  // namespace ketogpu

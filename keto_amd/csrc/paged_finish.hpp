// paged_finish.hpp — the ordered finish of the paged list calls (include/ketogpu.h
// ketogpu_lookup_page, ketogpu_subjects_page), shared by lookup.hip and subjects.hip.
//
// A paged request i has an inclusive lower bound from[i] and a stride of `limit` words at
// out + i * limit.  Of its member set M(i) — the set the full-list kernels produce — it reports
//   count[i]     = |M(i)|
//   remaining[i] = |{m in M(i) : m >= from[i]}|
//   returned[i]  = min(limit, remaining[i])
// and writes the returned[i] smallest members >= from[i] to the stride, ascending.  The stride
// is the reservation: no cursor, no truncation, no re-issue.
//
// Nothing here knows the direction of the closure.  `ok(u)` is the caller's member filter
// (type_ok / class_ok with the graph and the wanted type bound): it validates u itself.
//
//   tier 1  page_finish_wave: one wave, the LDS open-addressing set of 2048 slots.  One pass
//           counts and compacts the members >= from to the front of the same array (writes
//           never pass the reads), the tail up to the next power of two is filled with kEmpty
//           (0xFFFFFFFF: sorts last, never an id), a one-wave bitonic network sorts that
//           prefix, and the first `returned` words go out with coalesced stores.  No LDS
//           beyond the set itself.
//   tier 2  page_select_block: a workgroup of 256, a bitmap that is in id order by
//           construction.  Chunks of 256 consecutive words are walked upwards from word
//           from >> 5; each thread filters the set bits of its word, a workgroup exclusive
//           prefix (wave scan + four wave totals in LDS) gives its place, and it stores its ids
//           while the place is below `limit`.  The walk stops at the first chunk boundary at
//           which `limit` ids are placed.  It reads the bitmap only: the caller counts and
//           clears afterwards.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ketogpu.h"

namespace ketogpu {
namespace paged {

constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr unsigned kBlock = 256;  // tier 2's workgroup

struct PageOut {
    uint32_t *out;  // n * limit words
    uint32_t limit;
    uint32_t *returned;
    unsigned long long *count, *remaining;
};

__device__ inline void page_invalid(const PageOut &o, uint32_t i, bool invalid) {
    o.returned[i] = invalid ? KETOGPU_PAGE_INVALID : 0u;
    o.count[i] = 0;
    o.remaining[i] = 0;
}

// ascending bitonic sort of a[0 .. n) in LDS by one wave (a workgroup of 64); n a power of two
// >= 2.  Every compare-exchange step touches each word once, so the lanes never collide.
__device__ inline void wave_bitonic_sort(uint32_t *a, uint32_t n, uint32_t lane) {
    for (uint32_t k = 2; k <= n; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane; t < (n >> 1); t += 64) {
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const uint32_t x = a[lo], y = a[hi];
                if ((x > y) == ((lo & k) == 0)) a[lo] = y, a[hi] = x;
            }
            __syncthreads();
        }
    }
}

// tier 1: `set` holds the closure in `slots` LDS words (kEmpty: free).  One wave.
template <class Ok>
__device__ inline void page_finish_wave(uint32_t *set, uint32_t slots, uint32_t lane, uint32_t i, uint32_t from,
                                        const PageOut &o, Ok ok) {
    uint32_t cnt = 0, rem = 0;  // wave-uniform
    for (uint32_t s0 = 0; s0 < slots; s0 += 64) {
        const uint32_t u = set[s0 + lane];
        const bool m = ok(u);
        const bool keep = m && u >= from;
        const unsigned long long mm = __ballot(m), mk = __ballot(keep);
        __syncthreads();  // every lane has read its word of this chunk
        // rem <= s0: the write lands at or before this chunk's own words, never in a later chunk
        if (keep) set[rem + __popcll(mk & ((1ull << lane) - 1))] = u;
        cnt += __popcll(mm);
        rem += __popcll(mk);
    }
    const uint32_t ret = rem < o.limit ? rem : o.limit;
    if (lane == 0) {
        o.returned[i] = ret;
        o.count[i] = cnt;
        o.remaining[i] = rem;
    }
    if (!rem) return;
    uint32_t p = 2;
    while (p < rem) p <<= 1;  // rem <= slots, a power of two: p <= slots
    for (uint32_t s = rem + lane; s < p; s += 64) set[s] = kEmpty;
    __syncthreads();
    wave_bitonic_sort(set, p, lane);
    uint32_t *dst = o.out + (uint64_t)i * o.limit;
    for (uint32_t k = lane; k < ret; k += 64) dst[k] = set[k];
}

// tier 2: the `limit` smallest members >= from of the bitmap bm[0 .. bm_words), ascending, to
// dst.  Called by all kBlock threads; s_wave: kBlock / 64 LDS words.  Reads the bitmap only.
template <class Ok>
__device__ inline void page_select_block(const uint32_t *bm, uint64_t bm_words, uint32_t from, uint32_t limit,
                                         uint32_t *dst, uint32_t *s_wave, Ok ok) {
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t w0 = from >> 5;
    uint32_t placed = 0;  // uniform across the workgroup
    for (uint64_t base = w0; base < bm_words && placed < limit; base += kBlock) {
        const uint64_t w = base + tid;
        uint32_t bits = w < bm_words ? bm[w] : 0u;
        if (w == w0) bits &= ~0u << (from & 31);
        uint32_t mine = 0;
        while (bits) {  // the class is read for set bits only
            const uint32_t k = (uint32_t)__ffs(bits) - 1;
            bits &= bits - 1;
            if (ok((uint32_t)(w << 5) + k)) mine |= 1u << k;
        }
        const uint32_t c = __popc(mine);
        uint32_t incl = c;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t v = __shfl_up(incl, d);
            if (lane >= d) incl += v;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (unsigned x = 0; x < kBlock / 64; x++) {
            const uint32_t v = s_wave[x];
            before += x < wave ? v : 0u;
            total += v;
        }
        uint32_t pos = placed + before + incl - c;
        while (mine && pos < limit) {
            dst[pos++] = (uint32_t)(w << 5) + (uint32_t)__ffs(mine) - 1;
            mine &= mine - 1;
        }
        placed += total;  // (cannot wrap: a chunk adds at most 8192 to a value below limit <= 65536)
        __syncthreads();  // s_wave is free again
    }
}

}  // namespace paged
}  // namespace ketogpu

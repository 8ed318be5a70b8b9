// packed24.cpp — host side of the packed 24-bit request format (ketogpu_check_ids_packed24).
//
// Request i occupies bytes [6i, 6i + 6) of one buffer: root then target, three bytes each,
// little-endian; 0xFFFFFF stands for KETOGPU_NODE_NONE.  The buffer is ketogpu_packed24_bytes(n)
// long (6n rounded up to 8: the device reads it in 8-byte words) and its padding is zero.
// A host-to-host check reads 6 bytes per request over PCIe instead of the u32 arrays' 8.
#include <mutex>
#include <shared_mutex>
#include <string>

#include "ketogpu_internal.hpp"

using namespace ketogpu;

namespace {
constexpr uint32_t kNone24 = 0xFFFFFFu;

inline void put24(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
    p[2] = (uint8_t)(v >> 16);
}
inline uint32_t get24(const uint8_t *p) {
    const uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    return v == kNone24 ? KETOGPU_NODE_NONE : v;
}
}  // namespace

extern "C" {

size_t ketogpu_packed24_bytes(size_t n) { return (6 * n + 7) / 8 * 8; }

int ketogpu_pack24(const uint32_t *roots, const uint32_t *targets, size_t n, void *out) {
    if (n && (!roots || !targets || !out)) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    uint8_t *p = static_cast<uint8_t *>(out);
    for (size_t i = 0; i < n; i++) {
        const uint32_t r = roots[i], t = targets[i];
        if ((r != KETOGPU_NODE_NONE && r >= kNone24) || (t != KETOGPU_NODE_NONE && t >= kNone24)) {
            set_last_error("request " + std::to_string(i) + " has a node id outside the packed 24-bit range");
            return KETOGPU_EINVAL;
        }
        put24(p + 6 * i, r == KETOGPU_NODE_NONE ? kNone24 : r);
        put24(p + 6 * i + 3, t == KETOGPU_NODE_NONE ? kNone24 : t);
    }
    for (size_t b = 6 * n; b < ketogpu_packed24_bytes(n); b++) p[b] = 0;
    return KETOGPU_OK;
}

int ketogpu_unpack24(const void *packed, size_t n, uint32_t *roots, uint32_t *targets) {
    if (n && (!packed || !roots || !targets)) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    const uint8_t *p = static_cast<const uint8_t *>(packed);
    for (size_t i = 0; i < n; i++) {
        roots[i] = get24(p + 6 * i);
        targets[i] = get24(p + 6 * i + 3);
    }
    return KETOGPU_OK;
}

int ketogpu_snapshot_packed24_ok(const ketogpu_snapshot *s) {
    if (!s) return 0;
    const Snapshot &S = *reinterpret_cast<const Snapshot *>(s);
    std::shared_lock<std::shared_mutex> rd(S.mu);
    return S.N <= kNone24 ? 1 : 0;
}

}  // extern "C"

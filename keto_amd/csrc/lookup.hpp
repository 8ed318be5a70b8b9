// lookup.hpp — reverse lookup (include/ketogpu.h ketogpu_lookup_*): the object types of the
// expandable nodes, shared by the host implementation (lookup_host.cpp) and the device handle
// (lookup.hip).
#pragma once

#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "ketogpu_internal.hpp"

namespace ketogpu {

// The type of an expandable node: its (namespace id, relation) pair.  Wildcard subject sets
// (R5: an empty field, or the namespace named "") get types of their own (wild = true) that no
// (namespace name, relation) request resolves to.  Ids are dense, in order of first appearance
// among the node ids; node ids below Nx and their names never change under in-place writes
// (node classes are fixed between rebuilds), so the ids are stable for a snapshot's life.
struct TypeIndex {
    std::vector<uint32_t> node_type;  // Nx entries; KETOGPU_TYPE_NONE: never listed (placeholders)
    std::map<std::tuple<int32_t, uint32_t, bool>, uint32_t> ids;
};

// the index of the snapshot (caller holds the snapshot's shared lock): built once and kept for
// every version of the same snapshot object (see lookup_host.cpp for why that is sound)
std::shared_ptr<const TypeIndex> type_index_of(const Snapshot &s);

// the type key of one subject-set node: what type_index_of and class_index_of look up
struct TypeKeys {
    std::map<int32_t, bool> empty_ns;  // namespace id -> its configured name is ""
    explicit TypeKeys(const Snapshot &s) {
        for (const Namespace &n : s.namespaces) empty_ns[n.id] = n.name.empty();
    }
    std::tuple<int32_t, uint32_t, bool> of(const Snapshot &s, uint32_t v) const {
        auto e = empty_ns.find(s.node_ns[v]);
        const bool wild = s.node_a[v] == 0 || s.node_b[v] == 0 || (e != empty_ns.end() && e->second);
        return std::make_tuple(s.node_ns[v], s.node_b[v], wild);
    }
};

inline bool type_matches(uint32_t node_type, uint32_t want) {
    return want == KETOGPU_TYPE_ANY ? node_type != KETOGPU_TYPE_NONE : (want != KETOGPU_TYPE_NONE && node_type == want);
}

// one member of a host via call (ketogpu_snapshot_*_via): its id, the node whose row it was
// first seen in, and its distance from the start
struct ViaEntry {
    uint32_t id, via, hops;
};

// the members, ascending by id, to three malloc'ed arrays of *n words (via and hops may be
// null: not wanted); nothing is left allocated when this throws.  In lookup_host.cpp.
void via_result(std::vector<ViaEntry> &res, uint32_t **ids, uint32_t **via, uint32_t **hops, uint64_t *n);

}  // namespace ketogpu

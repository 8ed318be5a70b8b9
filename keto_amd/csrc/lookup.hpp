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

// the index of the snapshot's current version (caller holds the snapshot's shared lock)
std::shared_ptr<const TypeIndex> type_index_of(const Snapshot &s);

inline bool type_matches(uint32_t node_type, uint32_t want) {
    return want == KETOGPU_TYPE_ANY ? node_type != KETOGPU_TYPE_NONE : (want != KETOGPU_TYPE_NONE && node_type == want);
}

}  // namespace ketogpu

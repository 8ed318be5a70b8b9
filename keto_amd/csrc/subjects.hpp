// subjects.hpp — subject listing (include/ketogpu.h ketogpu_subjects_*): the classes of all
// nodes, shared by the host implementation (subjects_host.cpp) and the device handle
// (subjects.hip).
#pragma once

#include "lookup.hpp"

namespace ketogpu {

// The class of a node extends TypeIndex::node_type to all N nodes: below Nx the type itself
// (placeholders stay KETOGPU_TYPE_NONE); from Nx on KETOGPU_CLASS_SUBJECT_ID for a subject id,
// and for a subject set the type id of its (namespace id, relation, wild) key if an expandable
// node defines it, else KETOGPU_CLASS_UNTYPED_SET.  N grows under in-place writes (reserved
// ids): the array is built once and extended by the new ids (subjects_host.cpp).
struct ClassIndex {
    std::vector<uint32_t> node_class;  // N entries
};

// the class of one node from Nx on: what the full build and the extension both store
uint32_t class_of(const Snapshot &s, const TypeIndex &types, const TypeKeys &keys, uint32_t v);

// the index of the snapshot's current version (caller holds the snapshot's shared lock); read
// ids below the snapshot's N only, and only while that lock is held
std::shared_ptr<const ClassIndex> class_index_of(const Snapshot &s);

// ANY: every class but NONE; NONE and UNTYPED_SET as filters match nothing
inline bool class_matches(uint32_t node_class, uint32_t want) {
    return want == KETOGPU_TYPE_ANY
               ? node_class != KETOGPU_TYPE_NONE
               : (want != KETOGPU_TYPE_NONE && want != KETOGPU_CLASS_UNTYPED_SET && node_class == want);
}

}  // namespace ketogpu

// subjects_host.cpp — subject listing on the host (include/ketogpu.h "subject listing"):
//   * the classes of all nodes (subjects.hpp),
//   * ketogpu_snapshot_subject_class,
//   * ketogpu_snapshot_subjects: F(r) as a worklist closure over node_row.  DESIGN.md states
//     the check contract as allowed(r, t) <=> r in B(t); F(r) = {t : r in B(t)} is the set of
//     nodes reached from r in >= 1 edge over the rows the check engine sees (the first `len`
//     entries of each row).  Only interior entries (ids < Ni) are expanded: nodes in [Ni, Nx)
//     appear in no row and nodes from Nx on have no rows.
#include <unordered_set>

#include "subjects.hpp"

namespace ketogpu {

std::shared_ptr<const ClassIndex> class_index_of(const Snapshot &s) {
    auto types = type_index_of(s);  // (takes derived_mu itself)
    std::lock_guard<std::mutex> lk(s.derived_mu);
    // The classes below Nx are the types, which never change in place (type_index_of), and the
    // class of a node from Nx on follows from its own name fields and the type ids, which do
    // not change either: an in-place write only appends the ids [old N, N).  The cached array
    // is therefore extended by those, at a cost of O(new nodes).  Its storage is reserved up to
    // n_cap, so the extension copies nothing; it happens under derived_mu in the first call of
    // a version, while every holder of an earlier pointer reads ids below the N it saw, under
    // a snapshot lock that excludes writes.
    if (!s.class_cache) {
        auto c = std::make_shared<ClassIndex>();
        c->node_class.reserve(std::max(s.N, s.n_cap));
        c->node_class.assign(types->node_type.begin(), types->node_type.end());
        s.class_cache = c;
    }
    std::vector<uint32_t> &cls = s.class_cache->node_class;
    if (cls.size() < s.N) {
        const TypeKeys keys(s);
        for (uint32_t v = (uint32_t)cls.size(); v < s.N; v++) cls.push_back(class_of(s, *types, keys, v));
    }
    return s.class_cache;
}

uint32_t class_of(const Snapshot &s, const TypeIndex &types, const TypeKeys &keys, uint32_t v) {
    if (s.node_kind[v] != KETOGPU_SUBJECT_SET) return KETOGPU_CLASS_SUBJECT_ID;
    auto it = types.ids.find(keys.of(s, v));
    return it != types.ids.end() ? it->second : KETOGPU_CLASS_UNTYPED_SET;
}

}  // namespace ketogpu

using namespace ketogpu;

extern "C" {

int ketogpu_snapshot_subject_class(const ketogpu_snapshot *sp, uint32_t id, uint32_t *cls) {
    if (!sp || !cls) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    const Snapshot &s = *reinterpret_cast<const Snapshot *>(sp);
    std::shared_lock<std::shared_mutex> rd(s.mu);
    *cls = KETOGPU_TYPE_NONE;
    if (id >= s.N) {
        set_last_error("node id outside the snapshot");
        return KETOGPU_EINVAL;
    }
    *cls = class_index_of(s)->node_class[id];
    return KETOGPU_OK;
}

int ketogpu_snapshot_subjects(const ketogpu_snapshot *sp, uint32_t root, uint32_t cls, uint32_t **ids, uint64_t *n) {
    if (!sp || !ids || !n) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    *ids = nullptr;
    *n = 0;
    try {
        const Snapshot &s = *reinterpret_cast<const Snapshot *>(sp);
        std::shared_lock<std::shared_mutex> rd(s.mu);
        if (s.has_ambiguous)
            throw Error(KETOGPU_EINVAL, "subject listing: the snapshot has shared Subject.String() keys (R4)");
        if (root != NONE && root >= s.N) throw Error(KETOGPU_EINVAL, "root outside the snapshot");
        std::vector<uint32_t> res;
        if (root < s.Nx) {  // (NONE and the never-expanded nodes: the empty list)
            auto classes = class_index_of(s);
            std::unordered_set<uint32_t> seen;
            std::vector<uint32_t> work;
            auto row = [&](uint32_t v) {
                const uint32_t *p = s.row_ptr(v);
                for (uint32_t j = 0; j < s.node_row[v].len; j++) {
                    const uint32_t u = p[j];
                    if (u >= s.N || !seen.insert(u).second) continue;
                    if (u < s.Ni) work.push_back(u);
                    if (class_matches(classes->node_class[u], cls)) res.push_back(u);
                }
            };
            row(root);
            for (size_t h = 0; h < work.size(); h++) row(work[h]);
            std::sort(res.begin(), res.end());
        }
        uint32_t *p = (uint32_t *)malloc(std::max<size_t>(res.size(), 1) * sizeof(uint32_t));
        if (!p) throw std::bad_alloc();
        if (!res.empty()) memcpy(p, res.data(), res.size() * sizeof(uint32_t));
        *ids = p;
        *n = res.size();
        return KETOGPU_OK;
    } catch (const Error &e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc &) {
        set_last_error("out of host memory");
        return KETOGPU_ENOMEM;
    }
}

// ketogpu_snapshot_subjects level by level (DESIGN.md "Depth-limited listings"): the worklist is
// first in, first out, so its entries come in levels; the search stops before a row of level
// max_depth is read, and what is then left on the worklist is that level's interior members.
int ketogpu_snapshot_subjects_depth(const ketogpu_snapshot *sp, uint32_t root, uint32_t cls, uint32_t max_depth,
                                    uint32_t **ids, uint64_t *n, uint64_t *frontier) {
    if (!sp || !ids || !n) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    *ids = nullptr;
    *n = 0;
    if (frontier) *frontier = 0;
    try {
        const Snapshot &s = *reinterpret_cast<const Snapshot *>(sp);
        std::shared_lock<std::shared_mutex> rd(s.mu);
        if (s.has_ambiguous)
            throw Error(KETOGPU_EINVAL, "subject listing: the snapshot has shared Subject.String() keys (R4)");
        if (root != NONE && root >= s.N) throw Error(KETOGPU_EINVAL, "root outside the snapshot");
        std::vector<uint32_t> res;
        if (root < s.Nx) {  // (NONE and the never-expanded nodes: the empty list)
            auto classes = class_index_of(s);
            std::unordered_set<uint32_t> seen;
            std::vector<uint32_t> work;
            auto row = [&](uint32_t v) {
                const uint32_t *p = s.row_ptr(v);
                for (uint32_t j = 0; j < s.node_row[v].len; j++) {
                    const uint32_t u = p[j];
                    if (u >= s.N || !seen.insert(u).second) continue;
                    if (u < s.Ni) work.push_back(u);
                    if (class_matches(classes->node_class[u], cls)) res.push_back(u);
                }
            };
            row(root);
            size_t head = 0, level_end = 0;  // the row at hand is of `level`, which ends at work[level_end)
            for (uint32_t level = 0;;) {
                if (head == level_end) {  // work[head ..) is the next level
                    level++;
                    level_end = work.size();
                    if (head == work.size()) break;
                    if (level == max_depth) {  // (a placeholder is interior, but no member)
                        uint64_t fr = 0;
                        for (size_t k = head; k < work.size(); k++)
                            fr += classes->node_class[work[k]] != KETOGPU_TYPE_NONE;
                        if (frontier) *frontier = fr;
                        break;
                    }
                }
                row(work[head++]);
            }
            std::sort(res.begin(), res.end());
        }
        uint32_t *p = (uint32_t *)malloc(std::max<size_t>(res.size(), 1) * sizeof(uint32_t));
        if (!p) throw std::bad_alloc();
        if (!res.empty()) memcpy(p, res.data(), res.size() * sizeof(uint32_t));
        *ids = p;
        *n = res.size();
        return KETOGPU_OK;
    } catch (const Error &e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc &) {
        set_last_error("out of host memory");
        return KETOGPU_ENOMEM;
    }
}

// ketogpu_snapshot_subjects_depth with the parent and the level of every first visit kept
// (DESIGN.md "Grant trees"): via is the node whose row the member was first seen in, hops the
// level of that row plus one.
int ketogpu_snapshot_subjects_via(const ketogpu_snapshot *sp, uint32_t root, uint32_t cls, uint32_t max_depth,
                                  uint32_t **ids, uint32_t **via, uint32_t **hops, uint64_t *n, uint64_t *frontier) {
    if (!sp || !ids || !n) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    *ids = nullptr;
    if (via) *via = nullptr;
    if (hops) *hops = nullptr;
    *n = 0;
    if (frontier) *frontier = 0;
    try {
        const Snapshot &s = *reinterpret_cast<const Snapshot *>(sp);
        std::shared_lock<std::shared_mutex> rd(s.mu);
        if (s.has_ambiguous)
            throw Error(KETOGPU_EINVAL, "subject listing: the snapshot has shared Subject.String() keys (R4)");
        if (root != NONE && root >= s.N) throw Error(KETOGPU_EINVAL, "root outside the snapshot");
        std::vector<ViaEntry> res;
        if (root < s.Nx) {  // (NONE and the never-expanded nodes: the empty list)
            auto classes = class_index_of(s);
            std::unordered_set<uint32_t> seen;
            std::vector<uint32_t> work;
            uint32_t level = 0;  // of the row at hand (the root's: 0)
            auto row = [&](uint32_t v) {
                const uint32_t *p = s.row_ptr(v);
                for (uint32_t j = 0; j < s.node_row[v].len; j++) {
                    const uint32_t u = p[j];
                    if (u >= s.N || !seen.insert(u).second) continue;
                    if (u < s.Ni) work.push_back(u);
                    if (class_matches(classes->node_class[u], cls)) res.push_back({u, v, level + 1});
                }
            };
            row(root);
            size_t head = 0, level_end = 0;  // the row at hand is of `level`, which ends at work[level_end)
            for (;;) {
                if (head == level_end) {  // work[head ..) is the next level
                    level++;
                    level_end = work.size();
                    if (head == work.size()) break;
                    if (level == max_depth) {  // (a placeholder is interior, but no member)
                        uint64_t fr = 0;
                        for (size_t k = head; k < work.size(); k++)
                            fr += classes->node_class[work[k]] != KETOGPU_TYPE_NONE;
                        if (frontier) *frontier = fr;
                        break;
                    }
                }
                row(work[head++]);
            }
        }
        via_result(res, ids, via, hops, n);
        return KETOGPU_OK;
    } catch (const Error &e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc &) {
        set_last_error("out of host memory");
        return KETOGPU_ENOMEM;
    }
}

}  // extern "C"

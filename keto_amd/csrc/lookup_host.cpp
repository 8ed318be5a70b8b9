// lookup_host.cpp — reverse lookup on the host (include/ketogpu.h "reverse lookup"):
//   * the object types of the expandable nodes (lookup.hpp),
//   * ketogpu_snapshot_type / ketogpu_snapshot_node: names <-> ids for callers that list,
//   * ketogpu_snapshot_lookup: B(t) as a worklist closure over rev_off / rev_col.  DESIGN.md
//     states the check contract as allowed(r, t) <=> r in B(t), B(t) the expandable nodes
//     that reach t in >= 1 edge; listing B(t) answers the reverse question exactly.  Only
//     interior entries (ids < Ni) have reverse rows, so only they are expanded.
//   * ketogpu_snapshot_path: one path root ... target with the fewest hops, by the same closure
//     run breadth first with a parent per first visit (DESIGN.md "Explain").
#include <unordered_map>
#include <unordered_set>

#include "lookup.hpp"

namespace ketogpu {

std::shared_ptr<const TypeIndex> type_index_of(const Snapshot &s) {
    // The index reads Nx, the placeholders, and kind, namespace id, object and relation of the
    // nodes below Nx, and the configured namespaces.  An in-place write changes none of them:
    // Nx, Ni and the placeholders are fixed between rebuilds (a write that would move a node's
    // class is refused with KETOGPU_WRITE_CLASS), new subjects take ids in [N, n_cap), which lie
    // above Nx, the name fields of an existing node are never rewritten, and a new
    // namespace configuration is a new snapshot object.  So the index built for one version is
    // the index of every later version of the same object.
    std::lock_guard<std::mutex> lk(s.derived_mu);
    if (s.type_cache) return s.type_cache;
    auto t = std::make_shared<TypeIndex>();
    t->node_type.assign(s.Nx, KETOGPU_TYPE_NONE);
    const TypeKeys keys(s);
    for (uint32_t v = 0; v < s.Nx; v++) {
        if (v == s.Df || v == s.Dbi || v == s.Dbo || s.node_kind[v] != KETOGPU_SUBJECT_SET) continue;
        const auto key = keys.of(s, v);
        auto it = t->ids.find(key);
        if (it == t->ids.end()) it = t->ids.emplace(key, (uint32_t)t->ids.size()).first;
        t->node_type[v] = it->second;
    }
    s.type_cache = t;
    return t;
}

void via_result(std::vector<ViaEntry> &res, uint32_t **ids, uint32_t **via, uint32_t **hops, uint64_t *n) {
    std::sort(res.begin(), res.end(), [](const ViaEntry &a, const ViaEntry &b) { return a.id < b.id; });
    const size_t bytes = std::max<size_t>(res.size(), 1) * sizeof(uint32_t);
    uint32_t *p = (uint32_t *)malloc(bytes);
    uint32_t *pv = via ? (uint32_t *)malloc(bytes) : nullptr;
    uint32_t *ph = hops ? (uint32_t *)malloc(bytes) : nullptr;
    if (!p || (via && !pv) || (hops && !ph)) {
        free(p), free(pv), free(ph);
        throw std::bad_alloc();
    }
    for (size_t k = 0; k < res.size(); k++) {
        p[k] = res[k].id;
        if (pv) pv[k] = res[k].via;
        if (ph) ph[k] = res[k].hops;
    }
    *ids = p;
    if (via) *via = pv;
    if (hops) *hops = ph;
    *n = res.size();
}

}  // namespace ketogpu

using namespace ketogpu;

extern "C" {

int ketogpu_snapshot_type(const ketogpu_snapshot *sp, const char *ns_name, const char *relation, uint32_t *type) {
    if (!sp || !type) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    const Snapshot &s = *reinterpret_cast<const Snapshot *>(sp);
    std::shared_lock<std::shared_mutex> rd(s.mu);
    *type = KETOGPU_TYPE_NONE;
    std::string_view ns = sv(ns_name), rel = sv(relation);
    if (ns.empty() || rel.empty()) return KETOGPU_OK;  // wildcard types are not addressable by name
    const Namespace *n = s.ns_by_name(ns);
    const uint32_t rid = s.pool.find(rel);
    if (!n || rid == NONE) return KETOGPU_OK;
    auto t = type_index_of(s);
    auto it = t->ids.find(std::make_tuple(n->id, rid, false));
    if (it != t->ids.end()) *type = it->second;
    return KETOGPU_OK;
}

int ketogpu_snapshot_node(const ketogpu_snapshot *sp, uint32_t id, ketogpu_node_info *out) {
    if (!sp || !out) {
        set_last_error("null argument");
        return KETOGPU_EINVAL;
    }
    const Snapshot &s = *reinterpret_cast<const Snapshot *>(sp);
    std::shared_lock<std::shared_mutex> rd(s.mu);
    if (id >= s.N || id == s.Df || id == s.Dbi || id == s.Dbo) {
        set_last_error(id >= s.N ? "node id outside the snapshot" : "placeholder node");
        return KETOGPU_EINVAL;
    }
    *out = ketogpu_node_info{};
    out->kind = s.node_kind[id];
    out->expandable = id < s.Nx;
    out->type = id < s.Nx ? type_index_of(s)->node_type[id] : KETOGPU_TYPE_NONE;
    auto put = [](std::string_view v, const char *&p, size_t &n) { p = v.data(), n = v.size(); };
    put(std::string_view("", 0), out->ns, out->ns_len);
    put(std::string_view("", 0), out->rel, out->rel_len);
    put(s.pool.get(s.node_a[id]), out->id, out->id_len);
    if (out->kind == KETOGPU_SUBJECT_SET) {
        out->namespace_id = s.node_ns[id];
        if (const Namespace *n = s.ns_by_id(s.node_ns[id])) put(n->name, out->ns, out->ns_len);
        put(s.pool.get(s.node_b[id]), out->rel, out->rel_len);
    }
    return KETOGPU_OK;
}

int ketogpu_snapshot_lookup(const ketogpu_snapshot *sp, uint32_t target, uint32_t type, uint32_t **ids, uint64_t *n) {
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
            throw Error(KETOGPU_EINVAL, "reverse lookup: the snapshot has shared Subject.String() keys (R4)");
        if (target != NONE && target >= s.N) throw Error(KETOGPU_EINVAL, "target outside the snapshot");
        std::vector<uint32_t> res;
        if (target != NONE) {
            auto types = type_index_of(s);
            std::unordered_set<uint32_t> seen;
            std::vector<uint32_t> work;
            auto row = [&](uint32_t v) {
                for (uint64_t j = s.rev_off[v]; j < s.rev_off[v + 1]; j++) {
                    const uint32_t u = s.rev_col[j];
                    if (!seen.insert(u).second) continue;
                    if (u < s.Ni) work.push_back(u);
                    if (u < s.Nx && type_matches(types->node_type[u], type)) res.push_back(u);
                }
            };
            row(target);
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

// ketogpu_snapshot_lookup level by level (DESIGN.md "Depth-limited listings"): the worklist is
// first in, first out, so its entries come in levels; the search stops before a row of level
// max_depth is read, and what is then left on the worklist is that level's interior members.
int ketogpu_snapshot_lookup_depth(const ketogpu_snapshot *sp, uint32_t target, uint32_t type, uint32_t max_depth,
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
            throw Error(KETOGPU_EINVAL, "reverse lookup: the snapshot has shared Subject.String() keys (R4)");
        if (target != NONE && target >= s.N) throw Error(KETOGPU_EINVAL, "target outside the snapshot");
        std::vector<uint32_t> res;
        if (target != NONE) {
            auto types = type_index_of(s);
            std::unordered_set<uint32_t> seen;
            std::vector<uint32_t> work;
            auto row = [&](uint32_t v) {
                for (uint64_t j = s.rev_off[v]; j < s.rev_off[v + 1]; j++) {
                    const uint32_t u = s.rev_col[j];
                    if (!seen.insert(u).second) continue;
                    if (u < s.Ni) work.push_back(u);
                    if (u < s.Nx && type_matches(types->node_type[u], type)) res.push_back(u);
                }
            };
            row(target);
            size_t head = 0, level_end = 0;  // the row at hand is of `level`, which ends at work[level_end)
            for (uint32_t level = 0;;) {
                if (head == level_end) {  // work[head ..) is the next level
                    level++;
                    level_end = work.size();
                    if (head == work.size()) break;
                    if (level == max_depth) {  // (a placeholder is interior, but no member)
                        uint64_t fr = 0;
                        for (size_t k = head; k < work.size(); k++) fr += types->node_type[work[k]] != KETOGPU_TYPE_NONE;
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

// ketogpu_snapshot_lookup_depth with the parent and the level of every first visit kept
// (DESIGN.md "Grant trees"): via is the node whose reverse row the member was first seen in,
// hops the level of that row plus one.
int ketogpu_snapshot_lookup_via(const ketogpu_snapshot *sp, uint32_t target, uint32_t type, uint32_t max_depth,
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
            throw Error(KETOGPU_EINVAL, "reverse lookup: the snapshot has shared Subject.String() keys (R4)");
        if (target != NONE && target >= s.N) throw Error(KETOGPU_EINVAL, "target outside the snapshot");
        std::vector<ViaEntry> res;
        if (target != NONE) {
            auto types = type_index_of(s);
            std::unordered_set<uint32_t> seen;
            std::vector<uint32_t> work;
            uint32_t level = 0;  // of the row at hand (the target's: 0)
            auto row = [&](uint32_t v) {
                for (uint64_t j = s.rev_off[v]; j < s.rev_off[v + 1]; j++) {
                    const uint32_t u = s.rev_col[j];
                    if (!seen.insert(u).second) continue;
                    if (u < s.Ni) work.push_back(u);
                    if (u < s.Nx && type_matches(types->node_type[u], type)) res.push_back({u, v, level + 1});
                }
            };
            row(target);
            size_t head = 0, level_end = 0;  // the row at hand is of `level`, which ends at work[level_end)
            for (;;) {
                if (head == level_end) {  // work[head ..) is the next level
                    level++;
                    level_end = work.size();
                    if (head == work.size()) break;
                    if (level == max_depth) {  // (a placeholder is interior, but no member)
                        uint64_t fr = 0;
                        for (size_t k = head; k < work.size(); k++) fr += types->node_type[work[k]] != KETOGPU_TYPE_NONE;
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

// A breadth-first search from the target over the reverse rows: rows are expanded in the order
// their nodes were first seen, so the first visit of the root lies on a path with the fewest
// hops.  parent[u] is the node whose row u was first seen in.
int ketogpu_snapshot_path(const ketogpu_snapshot *sp, uint32_t root, uint32_t target, uint32_t **ids, uint64_t *n) {
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
            throw Error(KETOGPU_EINVAL, "reverse lookup: the snapshot has shared Subject.String() keys (R4)");
        if (target != NONE && target >= s.N) throw Error(KETOGPU_EINVAL, "target outside the snapshot");
        if (root != NONE && root >= s.N) throw Error(KETOGPU_EINVAL, "root outside the snapshot");
        std::vector<uint32_t> res;
        if (target != NONE && root < s.Nx) {
            std::unordered_map<uint32_t, uint32_t> parent;
            std::vector<uint32_t> work;
            bool hit = false;
            auto row = [&](uint32_t v) {
                for (uint64_t j = s.rev_off[v]; j < s.rev_off[v + 1] && !hit; j++) {
                    const uint32_t u = s.rev_col[j];
                    if (u >= s.Nx || !parent.emplace(u, v).second) continue;
                    if (u < s.Ni) work.push_back(u);
                    hit = u == root;
                }
            };
            row(target);
            for (size_t h = 0; h < work.size() && !hit; h++) row(work[h]);
            if (hit) {
                uint32_t x = root;
                res.push_back(x);
                do {  // (only the target's own row gives `target` as a parent: the walk ends there)
                    x = parent.at(x);
                    res.push_back(x);
                } while (x != target);
            }
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

}  // extern "C"

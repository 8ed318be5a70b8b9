/*
 * ketogpu.h — C ABI of the MI355X batched permission-check engine (libketogpu.so).
 *
 * This is the drop-in boundary for Ory Keto's evaluation engines.  Every entry
 * point below replaces a reference interface (paths relative to the reference
 * repository); the Go side binds it through cgo.
 *
 *   ketogpu_builder_*      new persistence-side snapshot loader; replaces the
 *                          per-node SQL reads of (*Persister).GetRelationTuples
 *                          internal/persistence/sql/relationtuples.go:203-258
 *   ketogpu_check          (*check.Engine).SubjectIsAllowed
 *                          internal/check/engine.go:93-95 (recursion :33-91)
 *   ketogpu_resolve /      the same, split into host resolution (strings -> node
 *   ketogpu_check_ids /    ids) and a batched device traversal over ids with
 *   ketogpu_queries_*      inputs resident in HBM
 *   ketogpu_expand         (*expand.Engine).BuildTree internal/expand/engine.go:30-98
 *   ketogpu_tree_*         expand.Tree / its JSON codec internal/expand/tree.go:26-30,85-91,156-162
 *   ketogpu_lookup_*       the reverse question (no reference counterpart): every object a
 *                          subject reaches, by the same SubjectIsAllowed semantics
 *
 * Conventions: plain C types only; all input memory is copied (cgo pointer rules);
 * opaque handles are owned by the library; result buffers are caller-allocated.
 * Functions return KETOGPU_OK or a positive KETOGPU_E* code; ketogpu_last_error()
 * returns a thread-local message for the last failure on the calling thread.
 * Error mapping (herodot): ENOTFOUND -> ErrNotFound (404), EINVAL -> ErrBadRequest
 * (400), EDEVICE/ENOMEM -> ErrInternalServerError (500).
 */
#ifndef KETOGPU_H
#define KETOGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KETOGPU_ABI_VERSION 9 /* (packed24 request batches, ketogpu_*packed24* and
                                    ketogpu_engine_last_request_path, are additions within
                                    9: no existing entry point or struct layout changed)
                                 9: plan label in the two-tier mode (tier stats label_*);
                                 8: 2-hop reachability labels (plan label), run stats
                                    label_* / rest_*;
                                 7: two-tier partitioned mode (ketogpu_core_*, ketogpu_tier_*);
                                 6: partitioned rounds behind the C ABI (comm, part_engine);
                                 5: writable snapshots (in-place writes, engine sync);
                                 4: ketogpu_shard_*, part_new over a shard; 3: host_alloc, multi */

#define KETOGPU_OK 0
#define KETOGPU_ENOTFOUND 1 /* unknown namespace (herodot.ErrNotFound)              */
#define KETOGPU_EINVAL 2    /* malformed input, nil subject, unsorted rows          */
#define KETOGPU_EDEVICE 3   /* HIP runtime / device failure                          */
#define KETOGPU_ENOMEM 4    /* host or device allocation failure                    */
#define KETOGPU_ECOLLISION 5 /* partitioned loader: 64-bit node hash collision; reload
                                with another ketogpu_shard_opts.salt                 */

#define KETOGPU_SUBJECT_ID 0
#define KETOGPU_SUBJECT_SET 1
#define KETOGPU_SUBJECT_NIL (-1)

#define KETOGPU_NODE_NONE 0xFFFFFFFFu /* no such node / root with no tuples      */
#define KETOGPU_NODE_NOT_OWNED 0xFFFFFFFEu /* ketogpu_shard_resolve_batch: another rank
                                              owns this node and resolves it          */

/* builder flags */
#define KETOGPU_BUILD_SORT 1u /* rows are NOT in ORDER BY order: sort them with the
                                  snapshot's row order (below) */
/* Row order of the backend the rows come from.  The ORDER BY of
 * relationtuples.go:215 is executed by the backend, and only NULL placement and string
 * collation differ between backends: SQLite (tests, default), MySQL with a binary
 * collation and CockroachDB put NULLs first; Postgres puts NULLs last — so a Postgres
 * group lists its subject-id rows (subject_id NOT NULL) before its subject-set rows.
 * Strings compare bytewise in both orders (SQLite BINARY, MySQL *_bin, Postgres "C"
 * collation, CockroachDB).  Locale collations are not modelled (expand order under them is
 * unpinned).  The order only matters where the library itself places rows: sorting
 * (KETOGPU_BUILD_SORT) and ketogpu_snapshot_apply; rows appended in order are kept. */
#define KETOGPU_ORDER_NULLS_LAST 2u /* Postgres ORDER BY (NULLS LAST, C collation) */
/* Writable snapshot (ketogpu_snapshot_write): the device rows are laid out with free slots
 * (2 + 1/8 of each row part) and ids are reserved for new subjects,
 * so a write batch patches the rows it touches in place instead of rebuilding the graph. */
#define KETOGPU_BUILD_WRITABLE 4u

typedef struct ketogpu_builder ketogpu_builder;
typedef struct ketogpu_snapshot ketogpu_snapshot;
typedef struct ketogpu_engine ketogpu_engine;
typedef struct ketogpu_queries ketogpu_queries;
typedef struct ketogpu_tree ketogpu_tree;

/* namespace.Namespace{ID, Name} (internal/namespace/definitons.go:8-12), config order */
typedef struct {
    int32_t id;
    const char *name;
} ketogpu_namespace;

/* A batch of keto_relation_tuples rows, columnar (one row per index; string column c of
 * row i is c_data[c_off[i] .. c_off[i+1]), offsets have n+1 entries).  Row layout follows
 * RelationTuple (internal/persistence/sql/relationtuples.go:18-31): subject_kind 0 =
 * subject_id row (ss_* ignored), 1 = subject-set row (subject_id ignored).
 * Rows of one snapshot must arrive in the backend's
 *   ORDER BY nid, namespace_id, object, relation, subject_id, subject_set_namespace_id,
 *            subject_set_object, subject_set_relation, commit_time   (relationtuples.go:215)
 * order across all append calls, for ONE nid (persister.go:117-119), unless the builder
 * was created with KETOGPU_BUILD_SORT. */
typedef struct {
    size_t n;
    const int32_t *namespace_id;
    const char *object_data;
    const uint64_t *object_off;
    const char *relation_data;
    const uint64_t *relation_off;
    const uint8_t *subject_kind;
    const char *subject_id_data;
    const uint64_t *subject_id_off;
    const int32_t *ss_namespace_id;
    const char *ss_object_data;
    const uint64_t *ss_object_off;
    const char *ss_relation_data;
    const uint64_t *ss_relation_off;
} ketogpu_row_batch;

typedef struct {
    int32_t page_size; /* GetRelationTuples page size; 0 -> 100 (persister.go:68-70) */
    uint32_t flags;    /* KETOGPU_BUILD_* */
} ketogpu_build_opts;

typedef struct {
    uint64_t num_rows;           /* rows appended                                  */
    uint64_t num_bad_rows;       /* rows whose namespace ids are not configured    */
    uint64_t num_groups;         /* distinct (namespace_id, object, relation)      */
    uint64_t num_nodes;          /* N: subject nodes (subject ids + subject sets)  */
    uint64_t num_expandable;     /* Nx: nodes whose query returns >= 1 row         */
    uint64_t num_interior;       /* Ni: expandable nodes that are also subjects    */
    uint64_t num_edges;          /* rows kept after page-poison truncation         */
    uint64_t num_interior_edges; /* deduplicated edges into interior nodes         */
    uint64_t num_rev_edges;      /* deduplicated reverse edges                     */
    uint64_t num_wildcard_nodes; /* subject sets with an empty field (R5)           */
    uint64_t num_ambiguous_nodes;/* nodes sharing a Subject.String() key (R4)      */
    double build_seconds;
} ketogpu_snapshot_stats;

/* ----------------------------------------------------------------- snapshot */
int ketogpu_builder_new(const ketogpu_namespace *namespaces, size_t num_namespaces,
                        const ketogpu_build_opts *opts, ketogpu_builder **out);
int ketogpu_builder_append(ketogpu_builder *b, const ketogpu_row_batch *rows);
/* consumes b (also on failure) */
int ketogpu_builder_finish(ketogpu_builder *b, ketogpu_snapshot **out);
void ketogpu_builder_free(ketogpu_builder *b);
void ketogpu_snapshot_free(ketogpu_snapshot *s);
int ketogpu_snapshot_stats_get(const ketogpu_snapshot *s, ketogpu_snapshot_stats *out);

/* Write-path freshness (R14): the next snapshot version = the base's
 * rows with one TransactRelationTuples batch applied (internal/persistence/sql/
 * relationtuples.go:271-278): inserts join their group after equal rows (commit_time
 * order), then every row matching a delete is removed (:178-201).  Row order follows
 * the base snapshot's row order (KETOGPU_ORDER_*).  The base stays valid; engines built on
 * the new version answer with the write applied.  inserts/deletes may be NULL. */
int ketogpu_snapshot_apply(const ketogpu_snapshot *base, const ketogpu_row_batch *inserts,
                           const ketogpu_row_batch *deletes, ketogpu_snapshot **out);

/* Namespace-configuration reload (internal/driver/config/provider.go:87-110: Keto drops
 * its namespace manager whenever KeyNamespaces changes): the next version holds the base's
 * rows under the new configuration, so page poisoning (R7) and name resolution follow it —
 * rows of a namespace id that is no longer configured poison their pages, rows of a
 * re-added one are visible again.  Duplicate names or ids are refused (KETOGPU_EINVAL). */
int ketogpu_snapshot_set_namespaces(const ketogpu_snapshot *base, const ketogpu_namespace *namespaces,
                                    size_t num_namespaces, ketogpu_snapshot **out);

/* In-place write (R14 at O(delta)) on a KETOGPU_BUILD_WRITABLE
 * snapshot: the same TransactRelationTuples semantics as ketogpu_snapshot_apply (inserts
 * after equal rows, then every row matching a delete removed), applied to THIS snapshot:
 * the touched groups' rows (host: expand, exact checks, resolution) and the touched device
 * rows (a patch list each engine uploads at its next call, or at ketogpu_engine_sync).
 * Cost: O(rows of the touched groups + touched device rows), independent of the graph.
 * A batch the free slots cannot represent leaves the snapshot unchanged and reports
 * applied = 0 with a reason; the caller then builds the next version with
 * ketogpu_snapshot_apply (which keeps the snapshot writable).  Not representable: a row
 * that creates a group or makes an expandable node interior (node classes are fixed
 * between rebuilds), rows with unconfigured namespace ids or touching a poisoned group (R7),
 * snapshots with wildcard subject sets (R5) or shared Subject.String() keys (R4), a new
 * subject whose key is shared, a full row, no reserved ids left.  Concurrent calls on the
 * snapshot and its engines are serialized against the write (reader/writer lock).
 * Nodes keep their class after their last row is deleted (an expandable node without rows
 * answers like a non-expandable one). */
#define KETOGPU_WRITE_APPLIED 0
#define KETOGPU_WRITE_NOT_WRITABLE 1
#define KETOGPU_WRITE_WILDCARD 2   /* R5 wildcard subject sets in the snapshot or the batch */
#define KETOGPU_WRITE_POISON 3     /* unconfigured namespace id, or a poisoned group (R7) */
#define KETOGPU_WRITE_CLASS 4      /* a new group, or an expandable node becoming interior */
#define KETOGPU_WRITE_AMBIGUOUS 5  /* shared Subject.String() keys (R4) */
#define KETOGPU_WRITE_FULL 6       /* a touched row has no free slot left */
#define KETOGPU_WRITE_RESERVE 7    /* no reserved node id left for a new subject */
#define KETOGPU_WRITE_FANOUT 8     /* a record count change would re-upload more rows than
                                      KETOGPU_WRITE_FANOUT_MAX (env, default 65536) */
typedef struct {
    int32_t applied;          /* 1: written in place; 0: unchanged, see reason */
    int32_t reason;           /* KETOGPU_WRITE_* */
    uint64_t rows_inserted;   /* rows added to groups */
    uint64_t rows_deleted;    /* rows removed (all duplicates of a deleted tuple) */
    uint64_t groups_touched;
    uint64_t device_rows;     /* device rows patched (forward + reverse) */
    uint64_t new_nodes;       /* subjects that got a reserved id */
    uint64_t version;         /* the snapshot's write version after the call */
    double seconds;           /* host time of the call */
} ketogpu_write_result;
int ketogpu_snapshot_write(ketogpu_snapshot *s, const ketogpu_row_batch *inserts, const ketogpu_row_batch *deletes,
                           ketogpu_write_result *result);
uint64_t ketogpu_snapshot_version(const ketogpu_snapshot *s);

/* Persisted snapshots (fast restart): a versioned binary image of
 * a finished snapshot.  Loading rebuilds only the derived indexes; a file written by a
 * different format version is refused with KETOGPU_EINVAL. */
int ketogpu_snapshot_save(const ketogpu_snapshot *s, const char *path);
int ketogpu_snapshot_load(const char *path, ketogpu_snapshot **out);

/* Read-only view of the device graph as built on the host (for tools and tests; the
 * pointers live as long as the snapshot).  Node ids: [0, num_interior) interior,
 * [num_interior, num_expandable) other expandable nodes, the rest never expand. */
typedef struct {
    uint32_t num_nodes, num_expandable, num_interior;
    const uint64_t *fint_off; /* num_expandable + 1 */
    const uint32_t *fint_col; /* interior successors of each expandable node */
    const uint64_t *rev_off;  /* num_nodes + 1 */
    const uint32_t *rev_col;  /* expandable predecessors of each node */
} ketogpu_graph_view;
int ketogpu_snapshot_graph(const ketogpu_snapshot *s, ketogpu_graph_view *out);

/* Plan "core"'s record arrays (keto_amd/csrc/core_index.hpp), built on the host the way an
 * engine builds them, for tools and tests (the engine builds its own; KETOGPU_UNITS=core).
 * Per direction (0 forward, 1 backward) one array of 16-byte records {node, deg, begin,
 * pad}: core rows (the rows among interior nodes), closure rows (pad bit 31: TERMINAL
 * entries), node blocks of the seed rows (fint(v) / rev(v); the head record of node v's
 * block {count, first record low, high, 0}) and overflow rows.  A record's deg/begin name
 * the node's expansion row in the same array; pad bit 30 = that row is a closure row.
 * closure_cap[d] = 0: no closure rows; block[d] = 0: block size chosen from the rows. */
typedef struct ketogpu_core_index ketogpu_core_index;
typedef struct {
    const uint32_t *records; /* 4 x u32 per record */
    uint64_t num_records;
    uint64_t block_base;     /* record index of node 0's block */
    uint32_t block_records;  /* records per node block: 4, 8, 16 or 32 */
    uint64_t overflow_rows;  /* seed rows kept outside their block */
    uint64_t closure_nodes, closure_entries;
} ketogpu_core_records;
int ketogpu_core_index_build(const ketogpu_snapshot *s, const uint32_t closure_cap[2], const uint32_t block[2],
                             ketogpu_core_index **out);
int ketogpu_core_index_view(const ketogpu_core_index *c, int direction, ketogpu_core_records *out);
void ketogpu_core_index_free(ketogpu_core_index *c);

/* Plan "label"'s 2-hop reachability labels (keto_amd/csrc/labels.hpp) as an engine builds
 * them, for tools and tests.  Interior nodes are ranked; Lin(v) / Lout(v) hold the ranks of
 * the landmarks that reach v / that v reaches (the first 64 landmarks as a bit mask), so
 * that a ->* b <=> Lout(a) meets Lin(b).  Per request:
 *   S(t) = Lin(v) for every interior v in rev(t), plus rev(t)'s other entries (node ids);
 *   P(r) = Lout(r) (r interior), else {r} + Lout(c) for every c in fint(r);
 *   allowed(r, t) <=> S(t) and P(r) share an entry or their masks share a bit.
 * One head per node (S: every node, P: every expandable node) of s_head_words /
 * p_head_words u32 (8, 16 or 32; 0 = chosen from the list lengths):
 *   [count, overflow start / 16, mask lo, mask hi, entries ascending, 0xFFFFFFFF pad];
 * a list longer than head - 4 entries lies whole at words 16 x (overflow start). */
typedef struct ketogpu_label_index ketogpu_label_index;
typedef struct {
    uint32_t s_head_words, p_head_words;
    const uint32_t *s_words, *p_words;
    uint64_t num_s_words, num_p_words;
    uint64_t s_nodes, p_nodes;
    uint64_t s_entries, p_entries;   /* list entries (masks not counted) */
    uint64_t s_overflow, p_overflow; /* lists kept outside their head */
    uint64_t label_entries;          /* Lin + Lout entries */
    double pll_ms, build_ms;         /* the labels / labels and heads (host) */
} ketogpu_label_view;
int ketogpu_label_index_build(const ketogpu_snapshot *s, uint32_t s_head_words, uint32_t p_head_words,
                              ketogpu_label_index **out);
int ketogpu_label_index_view(const ketogpu_label_index *l, ketogpu_label_view *out);
void ketogpu_label_index_free(ketogpu_label_index *l);

/* ------------------------------------------------------------------- check */
/* relationtuple.Subject: SubjectID{ID} or SubjectSet{Namespace, Object, Relation}
 * (internal/relationtuple/definitions.go:39-41,103-118) */
typedef struct {
    int32_t kind; /* KETOGPU_SUBJECT_* */
    const char *id;
    const char *ns;
    const char *obj;
    const char *rel;
} ketogpu_subject;

/* InternalRelationTuple used as a check request (definitions.go:95-100); an empty
 * namespace/object/relation is "no filter", as in GetRelationTuples. */
typedef struct {
    const char *ns;
    const char *obj;
    const char *rel;
    ketogpu_subject subject;
} ketogpu_check_request;

/* Host resolution of one request to node ids.  *root is an expandable node or
 * KETOGPU_NODE_NONE (the query returns no tuples, or its namespace is unknown: false);
 * *target is a node or KETOGPU_NODE_NONE (the subject appears in no tuple: false).
 * Returns KETOGPU_EINVAL for a nil subject; returns KETOGPU_ENOTFOUND with *root =
 * KETOGPU_NODE_NONE when the root is a wildcard query that matches no snapshot node
 * (use ketogpu_check for those). */
int ketogpu_resolve(const ketogpu_snapshot *s, const ketogpu_check_request *req, uint32_t *root,
                    uint32_t *target);

/* A batch of check requests, columnar like ketogpu_row_batch (string column c of request
 * i is c_data[c_off[i] .. c_off[i+1])).  subject_kind: 0 subject id (sid columns), 1
 * subject set (ss_* columns), 255 nil subject; NULL means all subject ids. */
typedef struct {
    size_t n;
    const char *ns_data;
    const uint64_t *ns_off;
    const char *obj_data;
    const uint64_t *obj_off;
    const char *rel_data;
    const uint64_t *rel_off;
    const uint8_t *subject_kind;
    const char *sid_data;
    const uint64_t *sid_off;
    const char *ss_ns_data;
    const uint64_t *ss_ns_off;
    const char *ss_obj_data;
    const uint64_t *ss_obj_off;
    const char *ss_rel_data;
    const uint64_t *ss_rel_off;
} ketogpu_request_batch;

/* ketogpu_resolve for a whole batch; status[i] as ketogpu_resolve's return value
 * (KETOGPU_OK, KETOGPU_EINVAL for nil subjects, KETOGPU_ENOTFOUND for wildcard roots
 * without a node).  status may be NULL. */
int ketogpu_resolve_batch(const ketogpu_snapshot *s, const ketogpu_request_batch *reqs, uint32_t *roots,
                          uint32_t *targets, int32_t *status);

typedef struct {
    int32_t device;             /* HIP device ordinal                                */
    uint32_t max_words_per_round; /* 64-check words traversed together; 0 = auto      */
    uint64_t state_budget_bytes;  /* HBM for traversal state; 0 = auto (<= 1/3 free)  */
} ketogpu_engine_opts;

/* uploads the snapshot's device graph (forward interior CSR + reverse CSR) to HBM */
int ketogpu_engine_new(const ketogpu_snapshot *s, const ketogpu_engine_opts *opts,
                       ketogpu_engine **out);
void ketogpu_engine_free(ketogpu_engine *e);

/* SubjectIsAllowed for n requests: allowed[i] in {0,1}; status[i] = KETOGPU_OK or
 * KETOGPU_EINVAL (nil subject).  Unknown namespaces yield allowed = 0 (engine.go:75-77).
 * The function itself fails only on device/alloc errors. */
int ketogpu_check(ketogpu_engine *e, const ketogpu_check_request *reqs, size_t n, uint8_t *allowed,
                  int32_t *status);

/* id-level batch: roots/targets from ketogpu_resolve; allowed_bits / flagged_bits have
 * ceil(n/64) words, bit i%64 of word i/64 for request i.  A flagged request touched a
 * node whose Subject.String() key is shared with another node (R4 in DESIGN.md): its bit
 * is only exact after re-evaluation with the sequential semantics (ketogpu_check does
 * that itself).  flagged_bits may be NULL.  Host to host: the requests are copied to HBM
 * in chunks that overlap the traversal of the chunks before them, ids are validated on
 * the device (an id outside the snapshot fails the call with KETOGPU_EINVAL), and the
 * result bits come back with the run's one host synchronization.  This is the batch
 * call SURVEY.md 8(d) times. */
int ketogpu_check_ids(ketogpu_engine *e, const uint32_t *roots, const uint32_t *targets, size_t n,
                      uint64_t *allowed_bits, uint64_t *flagged_bits);

/* Packed 24-bit request batches ("packed24"): 6 bytes per request over PCIe instead of 8.
 * Request i occupies bytes [6i, 6i + 6) of one buffer: bytes 0-2 the root, bytes 3-5 the
 * target, both little-endian; 0xFFFFFF stands for KETOGPU_NODE_NONE.  The format serves a
 * snapshot with num_nodes <= 0xFFFFFF (ketogpu_snapshot_packed24_ok; a writable snapshot
 * grows, so every check call tests it again).  The buffer is ketogpu_packed24_bytes(n)
 * bytes long, 6n rounded up to a multiple of 8, and 8-byte aligned; the padding bytes are
 * never interpreted and nothing past them is read. */
size_t ketogpu_packed24_bytes(size_t n);
/* host code.  NONE becomes 0xFFFFFF; any other id >= 0xFFFFFF fails with KETOGPU_EINVAL
 * ("request <i> ..."); the padding bytes are written as 0.  out: ketogpu_packed24_bytes(n) */
int ketogpu_pack24(const uint32_t *roots, const uint32_t *targets, size_t n, void *out);
/* host code, the inverse (0xFFFFFF becomes KETOGPU_NODE_NONE) */
int ketogpu_unpack24(const void *packed, size_t n, uint32_t *roots, uint32_t *targets);
/* 1: the snapshot's ids fit the format now, 0: they do not (or s is NULL) */
int ketogpu_snapshot_packed24_ok(const ketogpu_snapshot *s);
/* ketogpu_check_ids over a packed24 buffer: the same bits and flags, an id outside the
 * snapshot fails the call with KETOGPU_EINVAL and the request's index, flagged_bits may be
 * NULL.  Also KETOGPU_EINVAL: a buffer that is not 8-byte aligned, a snapshot with more than
 * 0xFFFFFF nodes (the message says which).  With plan label and a buffer of
 * ketogpu_host_alloc (or other mapped pinned memory) the first stage reads the packed bytes
 * in place; every other plan and memory kind expands them into u32 arrays in HBM first
 * (pageable memory: after one DMA copy of the packed bytes). */
int ketogpu_check_ids_packed24(ketogpu_engine *e, const void *packed, size_t n, uint64_t *allowed_bits,
                               uint64_t *flagged_bits);
/* how the engine's last check call received its requests: 0 = u32 arrays; 1 = packed24,
 * expanded into HBM ahead of the first stage; 2 = packed24, read in place by the first
 * stage.  (An accessor of its own: ketogpu_run_stats keeps its layout.) */
int ketogpu_engine_last_request_path(const ketogpu_engine *e, int32_t *path);

/* Pinned host memory (hipHostMalloc) for request and result arrays.  A batch whose
 * roots/targets live here is copied by DMA at full PCIe rate; the cgo micro-batcher
 *  fills such a buffer in place instead of a Go slice, which it has to
 * copy into C memory anyway (cgo pointer rules).  Any host memory works with
 * ketogpu_check_ids; pageable memory is staged by the HIP runtime. */
int ketogpu_host_alloc(size_t bytes, void **out);
void ketogpu_host_free(void *p);

/* ------------------------------------------------------ replicated multi-GPU */
/* One engine per listed device over the same snapshot (the graph replicated in every
 * GPU's HBM, SURVEY.md 8(e) "Replicated"); replaces scaling out by more Keto processes
 * (internal/driver/daemon.go:87-159) with one PermissionEngine per process
 * (internal/driver/registry_default.go:158-163) that drives the whole node.
 * ketogpu_multi_check_ids splits the batch into ketogpu_multi_size() contiguous ranges of
 * whole 64-request words (ketogpu_multi_range), runs ketogpu_check_ids on every device
 * concurrently from one host thread per device and writes each range's bits at its
 * offset of allowed_bits / flagged_bits.  No communication between devices. */
typedef struct ketogpu_multi ketogpu_multi;
int ketogpu_multi_new(const ketogpu_snapshot *s, const int32_t *devices, size_t num_devices,
                      const ketogpu_engine_opts *opts, ketogpu_multi **out);
void ketogpu_multi_free(ketogpu_multi *m);
size_t ketogpu_multi_size(const ketogpu_multi *m);
/* the engine of device slot i (statistics); owned by m */
ketogpu_engine *ketogpu_multi_engine(ketogpu_multi *m, size_t i);
int ketogpu_multi_check_ids(ketogpu_multi *m, const uint32_t *roots, const uint32_t *targets, size_t n,
                            uint64_t *allowed_bits, uint64_t *flagged_bits);
/* the same split over a packed24 buffer (ketogpu_check_ids_packed24): a range begins at a
 * multiple of 64 requests, 384 bytes, so every device's part keeps the 8-byte alignment */
int ketogpu_multi_check_ids_packed24(ketogpu_multi *m, const void *packed, size_t n, uint64_t *allowed_bits,
                                     uint64_t *flagged_bits);
/* requests [*begin, *end) of part i when n requests are split into `parts` ranges */
void ketogpu_multi_range(size_t n, size_t parts, size_t i, size_t *begin, size_t *end);

/* device-resident query sets: upload once, run many times (results stay in HBM) */
int ketogpu_queries_upload(ketogpu_engine *e, const uint32_t *roots, const uint32_t *targets,
                           size_t n, ketogpu_queries **out);
int ketogpu_queries_run(ketogpu_engine *e, ketogpu_queries *q);
int ketogpu_queries_download(ketogpu_engine *e, const ketogpu_queries *q, uint64_t *allowed_bits,
                             uint64_t *flagged_bits);
/* the same call as ketogpu_queries_run, enqueued on the engine's stream without waiting for
 * the device when the engine can prove that no request of the batch needs the second stage
 * (plan label, no head marked unlabelled, no wildcard root): batches are then pipelined, the
 * way a server enqueues batch k+1 while batch k runs (Keto's check handler answers each
 * request when its batch's bits are back: internal/check/handler.go).  *queued = 1 when the
 * call returned before the device finished — its results are complete once
 * ketogpu_queries_download or ketogpu_engine_wait returns, and a device error of the call is
 * reported by that later call; 0: it ran as ketogpu_queries_run.  (queued may be NULL.) */
int ketogpu_queries_run_async(ketogpu_engine *e, ketogpu_queries *q, int *queued);
/* waits for every call enqueued on the engine (ketogpu_queries_run_async) */
int ketogpu_engine_wait(ketogpu_engine *e);
/* diagnostics: the requests that the most recent separately launched dense pass of a queued
 * call (plan label) found listed, as read at the engine's last wait or download of such a
 * call; 0 before the first.  Queued calls answer short P overflows in their first stage
 * (KETOGPU_LABEL_TAIL), so this is below ketogpu_run_stats.full_requests of a
 * synchronized call over the same batch. */
int ketogpu_engine_piped_full_requests(ketogpu_engine *e, uint64_t *out);
/* diagnostics: plan label's first-stage launches on this engine so far in which a wave ran two
 * units of 16 requests (KETOGPU_LABEL_PAIR) */
int ketogpu_engine_label_pair_launches(ketogpu_engine *e, uint64_t *out);
/* diagnostics: queued first-stage launches on this engine so far that read the S head first
 * and the P head only where S leaves the answer open (KETOGPU_LABEL_SFIRST: 1, the default,
 * at 32/32 heads; 2 every queued launch but one — at 8/64 heads with two units per wave the
 * flagged kernel would pass 64 VGPRs and lose a wave per SIMD against its unflagged twin, so
 * it is launched as it was; the flag needs the tail phase, KETOGPU_LABEL_TAIL) */
int ketogpu_engine_label_sfirst_launches(ketogpu_engine *e, uint64_t *out);
/* diagnostics: the requests whose P head those launches did not read, summed over the
 * engine's launches so far.  Counted only on an engine created with
 * KETOGPU_LABEL_SFIRST_COUNT=1 (else 0: lean launches carry no counter).  Waits for the
 * engine's queued calls. */
int ketogpu_engine_label_one_head_requests(ketogpu_engine *e, uint64_t *out);
void ketogpu_queries_free(ketogpu_queries *q);

/* statistics of the last run on this engine (for the roofline report) */
typedef struct {
    uint64_t checks;
    uint64_t rounds;
    uint64_t levels;            /* BFS levels summed over rounds                  */
    uint64_t frontier_entries;  /* (word, node) entries expanded                  */
    uint64_t interior_edges;    /* interior edges scanned by the push kernel      */
    uint64_t rev_edges;         /* reverse edges scanned by the pull kernel       */
    uint64_t touched;           /* (word, node) visited entries reset             */
    uint64_t bytes_push;        /* algorithmic bytes of the push (expand) kernel  */
    uint64_t bytes_pull;        /* algorithmic bytes of the pull kernel           */
    uint64_t bytes_total;       /* algorithmic bytes of all kernels               */
    double ms_push;             /* summed device time of push launches (hipEvent) */
    double ms_pull;
    double ms_total;            /* device time, first to last kernel              */
    uint64_t push_launches;
    uint64_t overflow_retries;
    /* LDS unit path (one launch: whole BFS + pull per 16-request unit in LDS) */
    uint64_t spilled_units;     /* units that spilled out of an LDS table (all passes) */
    uint64_t unit_rows;         /* rows opened (forward offsets + reverse offsets) */
    uint64_t unit_edges;        /* interior edges scanned                         */
    uint64_t unit_rev;          /* reverse entries scanned                        */
    uint64_t bytes_unit;        /* algorithmic HBM bytes of the unit kernel       */
    double ms_unit;             /* device time of the unit kernels (hipEvent)     */
    uint64_t spilled_requests;  /* single requests run on the global path         */
    uint64_t unit_launches;     /* unit-kernel launches (cascade passes)          */
    uint64_t main_bytes;        /* algorithmic HBM bytes of the first unit pass   */
    double main_ms;             /* its device time (hipEvent)                     */
    int32_t plan;               /* first stage of the run: 0 global path only, 1 bidi,
                                 * 2 forward unit2 (v2), 3 one-wave units, 4 unit v1,
                                 * 5 lite, 6 core (lite with closure rows), 7 label.
                                 * KETOGPU_UNITS=auto (default) tries bidi (128- and 64-
                                 * entry pending lists), v2 and (with hubs) the global path
                                 * alone on the first two batches of
                                 * >= 65536 requests, then keeps the fastest; those two
                                 * calls run every candidate (same results)              */
    uint32_t plan_lists;        /* bidi: pending-list entries of the first stage        */
    uint32_t hubs;              /* hub index: hubs (0 = off); searches stop at hubs and
                                 * read their precomputed closures (power-law graphs)   */
    uint32_t hub_words;         /* 64-bit words per interior node of the hub closures   */
    double hub_build_ms;        /* one-time hub closure build at engine creation        */
    uint32_t plan_unit;         /* bidi: requests per first-stage unit (16 or 8)        */
    /* plan 6 "core" (lite over its own record arrays with CLOSURE rows: an interior node
     * whose forward / backward closure has at most cap nodes expands into all of it in one
     * level; KETOGPU_CLOSURE="cap_f,cap_b") */
    uint32_t closure_cap_f, closure_cap_b;  /* 0, 0 when the plan is off                */
    uint64_t closure_nodes_f, closure_nodes_b;      /* nodes with a closure row          */
    uint64_t closure_entries_f, closure_entries_b;  /* records in closure rows           */
    double core_build_ms;       /* one-time build of the core arrays at engine creation */
    /* plan 7 "label" (2-hop reachability labels, labels.hpp: one intersection of two short
     * sorted lists per request; requests without labels — wildcard roots — go to a second
     * stage, plan lite over the listed requests) */
    int32_t label_on;           /* 1: labels built                                      */
    double label_coverage;      /* share of the non-empty S heads with a label (1 unless
                                 * KETOGPU_LABEL_REST_PERMILLE marks some for the second stage) */
    double label_build_ms;      /* one-time build at engine creation (labels + heads)   */
    uint32_t label_s_head;      /* S / P head words (8, 16 or 32)                       */
    uint32_t label_p_head;
    double label_pll_ms;        /* of which the 2-hop labels                            */
    uint64_t label_bytes;       /* S + P arrays in HBM                                  */
    uint64_t label_entries;     /* Lin + Lout entries                                   */
    uint64_t rest_requests;     /* requests of this run answered by the second stage    */
    uint64_t full_requests;     /* requests whose overflowing list the dense pass searched */
    double rest_ms;             /* second stage + statistics (events between kernels)   */
    /* plan label on a writable snapshot (label_update: heads rewritten in place per write) */
    uint64_t label_rewritten;   /* heads rewritten after writes                          */
    uint64_t label_marked;      /* heads marked "no label" (second stage) since the build */
    uint64_t label_relabels;    /* rebuilds from the current rows                        */
} ketogpu_run_stats;
int ketogpu_engine_last_stats(const ketogpu_engine *e, ketogpu_run_stats *out);
/* every_kernel = 1: host-to-host batches (ketogpu_check_ids from pinned memory), and plan
 * label's device-resident batches, record a timing event between the call's kernels, so
 * last_stats' main_ms is the first stage's own device time (each event pair costs a few
 * microseconds of idle GPU between the launches); 0 (default): one event pair around the
 * whole call (KETOGPU_EVENTS=all sets 1 at creation) */
int ketogpu_engine_set_events(ketogpu_engine *e, int every_kernel);

/* Upload the device rows patched by ketogpu_snapshot_write since the engine's last sync
 * (every check entry point also does this first).  ms: host time of the sync (may be NULL);
 * rows: device rows uploaded (may be NULL). */
int ketogpu_engine_sync(ketogpu_engine *e, double *ms, uint64_t *rows);
/* Test hook: the engine's device rows and edge records compared entry by entry with the
 * snapshot's host rows (after a sync); mismatches = entries that differ. */
int ketogpu_engine_check_graph(ketogpu_engine *e, uint64_t *mismatches);
/* Test hook: plan label's S (side 0) or P (side 1) head array as the engine built it on the
 * device (the layout of ketogpu_label_view); *words = its length in u32 words (0: no
 * labels), *head_words its head size; copied into out when capacity >= *words. */
int ketogpu_engine_label_heads(ketogpu_engine *e, int side, uint32_t *out, uint64_t capacity, uint64_t *words,
                               uint32_t *head_words);

/* ----------------------------------------------- partition-aware loader */
/* BASELINE config #5 (SURVEY.md 8(e) "Partitioned"): a graph that fits neither one GPU nor
 * one host.  Every rank streams the same ordered row read the single-GPU loader takes
 * (ketogpu_builder_*; internal/persistence/sql/relationtuples.go:203-258 with the ORDER
 * BY of :215, one nid, persister.go:94-96) and keeps only what it owns: node v (a typed
 * subject, internal/relationtuple/definitions.go:253-267) belongs to rank
 * hash(v, salt) % world; a rank keeps the rows of the groups it owns (forward rows) and
 * the rows whose subject it owns (reverse rows), after the reference's page poisoning
 * (R7), so no rank interns or holds the whole graph.  Owners number their nodes; the ids
 * of referenced nodes owned elsewhere come from one exchange the caller carries out
 * (keto_amd/partition.py: torch.distributed all_to_all / all_gather):
 *   builder_new/append.../finish -> counts -> [all_gather] -> set_layout
 *   -> queries -> [all_to_all] -> answer -> [all_to_all] -> apply
 *   -> claims -> [all_to_all] -> check_claims -> [all_reduce: any ambiguous key -> refuse]
 * Graphs the partitioned engine does not evaluate are refused on every rank alike:
 * wildcard subject sets (R5) and rows out of ORDER BY order with KETOGPU_EINVAL, shared
 * Subject.String() keys (R4) by check_claims' count.  Node ids: within each class (interior,
 * other expandable, never expanded) ids interleave the ranks, so owner and local index are
 * arithmetic (partition.hip); interior ids stay the smallest. */
typedef struct ketogpu_shard_builder ketogpu_shard_builder;
typedef struct ketogpu_shard ketogpu_shard;
typedef struct {
    int32_t page_size; /* GetRelationTuples page size; 0 -> 100                        */
    uint32_t flags;    /* KETOGPU_ORDER_* (rows must arrive in ORDER BY order)          */
    int32_t rank, world; /* world <= 64                                                 */
    uint64_t salt;     /* node hash salt; retry another after KETOGPU_ECOLLISION       */
} ketogpu_shard_opts;
typedef struct {
    uint64_t rows, bad_rows;             /* rows streamed; rows with unknown namespaces */
    uint64_t owned_nodes, owned_interior, owned_expandable;
    uint64_t forward_edges;              /* kept forward row entries (before dedup)     */
    uint64_t interior_forward_edges;     /* device forward rows (interior, deduplicated) */
    uint64_t reverse_edges;              /* reverse row entries                         */
    uint64_t queries;                    /* distinct referenced nodes (id exchange)     */
    uint64_t ambiguous_keys;             /* check_claims: shared String() keys found    */
    uint64_t num_interior, num_expandable, num_nodes; /* global id layout (Ni, Nx, N)   */
    uint64_t host_bytes;                 /* peak bytes of the loader's own arrays       */
    double seconds;                      /* streaming time                              */
} ketogpu_shard_stats;
int ketogpu_shard_builder_new(const ketogpu_namespace *namespaces, size_t num_namespaces,
                              const ketogpu_shard_opts *opts, ketogpu_shard_builder **out);
int ketogpu_shard_builder_append(ketogpu_shard_builder *b, const ketogpu_row_batch *rows);
/* consumes b (also on failure) */
int ketogpu_shard_builder_finish(ketogpu_shard_builder *b, ketogpu_shard **out);
void ketogpu_shard_builder_free(ketogpu_shard_builder *b);
void ketogpu_shard_free(ketogpu_shard *s);
/* this rank's node counts per class; every rank's (world x 3, rank order) to set_layout */
int ketogpu_shard_counts(const ketogpu_shard *s, uint64_t counts[3]);
int ketogpu_shard_set_layout(ketogpu_shard *s, const uint64_t *all_counts);
/* distinct node hashes this rank references, grouped by owner (counts[world]) */
uint64_t ketogpu_shard_query_count(const ketogpu_shard *s);
int ketogpu_shard_queries(const ketogpu_shard *s, uint64_t *hashes, uint64_t capacity, uint64_t *counts);
/* owner side: the global ids of received hashes (all owned by this rank) */
int ketogpu_shard_answer(const ketogpu_shard *s, const uint64_t *hashes, uint64_t n, uint32_t *ids);
/* the answers, in the order of ketogpu_shard_queries: builds the device rows */
int ketogpu_shard_apply(ketogpu_shard *s, const uint32_t *ids, uint64_t n);
/* R4: (String() key hash, node hash) pairs of owned nodes whose key another node could
 * share, grouped by the key hash's owner; the receiver counts keys held by >= 2 nodes */
uint64_t ketogpu_shard_claim_count(const ketogpu_shard *s);
int ketogpu_shard_claims(const ketogpu_shard *s, uint64_t *pairs, uint64_t capacity, uint64_t *counts);
int ketogpu_shard_check_claims(ketogpu_shard *s, const uint64_t *pairs, uint64_t n, uint64_t *ambiguous);
/* The whole exchange above in one collective call over a communicator (below: RCCL or a
 * transport; NULL = a single rank), every step's status agreed by all ranks: counts ->
 * set_layout -> queries/answer/apply -> claims/check_claims.  KETOGPU_ECOLLISION: every
 * rank reloads with another salt; KETOGPU_EINVAL: shared Subject.String() keys (R4). */
struct ketogpu_comm;
int ketogpu_shard_exchange(ketogpu_shard *s, struct ketogpu_comm *comm);
/* ketogpu_resolve_batch for a shard: ids of the requests' roots and targets this rank owns,
 * KETOGPU_NODE_NOT_OWNED for the others (the owner's answer is the one that counts);
 * status ENOTFOUND for wildcard roots (not evaluated partitioned), EINVAL nil subjects */
int ketogpu_shard_resolve_batch(const ketogpu_shard *s, const ketogpu_request_batch *reqs, uint32_t *roots,
                                uint32_t *targets, int32_t *status);
int ketogpu_shard_stats_get(const ketogpu_shard *s, ketogpu_shard_stats *out);
/* read-only view of the rank's device rows (tools, tests); global node ids */
typedef struct {
    uint32_t rank, world;
    uint32_t num_interior, num_expandable, num_nodes;       /* Ni, Nx, N (global)      */
    uint32_t owned_interior, owned_expandable, owned_nodes; /* local class bounds      */
    const uint64_t *lf_off; /* owned_expandable + 1: interior successors               */
    const uint32_t *lf_col;
    const uint64_t *lr_off; /* owned_nodes + 1: expandable predecessors, sorted          */
    const uint32_t *lr_col;
    const uint64_t *lb_off; /* owned_interior + 1: interior predecessors                */
    const uint32_t *lb_col;
} ketogpu_shard_graph;
int ketogpu_shard_view(const ketogpu_shard *s, ketogpu_shard_graph *out);

/* ------------------------------------------------------- partitioned mode */
/* Hash-partitioned traversal for graphs that do not fit one GPU (BASELINE config #5,
 * SURVEY.md 8(e)); replaces the same SubjectIsAllowed recursion as ketogpu_check_ids
 * (internal/check/engine.go:33-95), spread over ranks.  A rank's partition is its loaded
 * shard (ketogpu_shard_*): it holds the forward interior rows and traversal state of its
 * expandable nodes and the reverse rows of its nodes; ketogpu_part_owner(v) names the
 * rank that owns global node id v.  These
 * calls are one rank's device steps of a round; the caller moves the records between
 * ranks (keto_amd/partition.py: torch.distributed all_to_all over RCCL):
 *   begin -> { emit -> [all-to-all] -> apply -> [all-reduce frontier; stop at 0] -> expand }
 *         -> pull_emit -> [all-to-all] -> pull_answer -> end   (answer = OR of end() bits)
 * Buffers named *_dev are device memory on the rank's GPU.  A step that returns
 * KETOGPU_ENOMEM (buffers too small for this round) leaves the round to ketogpu_part_abort;
 * every rank must then abort and retry with fewer requests per round.  Snapshots with
 * ambiguous Subject.String() keys are refused (KETOGPU_EINVAL). */
typedef struct ketogpu_part ketogpu_part;
typedef struct {
    uint32_t a; /* BFS: 64-request word of the round; pull: request index of the round */
    uint32_t b; /* node id (global) — its owner receives the record                     */
    uint64_t m; /* BFS: request bits of word a; pull: 0                                  */
} ketogpu_record;
typedef struct {
    int32_t device;
    int32_t rank, world;          /* world <= 64                                       */
    uint64_t record_capacity;     /* outgoing records per step; 0 = auto               */
    uint32_t max_words_per_round; /* 0 = auto (state budget)                           */
    uint64_t state_budget_bytes;  /* 0 = auto                                          */
} ketogpu_part_opts;
/* kernel families of ketogpu_part_stats.ms / bytes / launches */
#define KETOGPU_PART_K_SEED 0
#define KETOGPU_PART_K_EXPAND 1
#define KETOGPU_PART_K_PACK 2        /* count + scatter by destination (world 1: a copy) */
#define KETOGPU_PART_K_APPLY 3
#define KETOGPU_PART_K_GATHER 4
#define KETOGPU_PART_K_PULL_EMIT 5
#define KETOGPU_PART_K_PULL_ANSWER 6
#define KETOGPU_PART_K_RESET 7
typedef struct {
    uint64_t owned_interior, owned_expandable, owned_forward_edges, owned_reverse_edges;
    uint64_t rounds, levels, frontier_entries, forward_edges;
    uint64_t records_sent, records_received, queries_answered;
    /* per kernel family: algorithmic HBM bytes (always counted) and, while timing is on
     * (ketogpu_part_set_timing), summed hipEvent device time and timed launches */
    uint64_t bytes[8];
    double ms[8];
    uint64_t launches[8];
} ketogpu_part_stats;
/* opts->rank / world must match the shard's */
int ketogpu_part_new(const ketogpu_shard *s, const ketogpu_part_opts *opts, ketogpu_part **out);
uint32_t ketogpu_part_owner(const ketogpu_part *p, uint32_t node);
void ketogpu_part_free(ketogpu_part *p);
/* 64-request words one round holds */
uint64_t ketogpu_part_round_words(const ketogpu_part *p);
/* same (roots, targets) host arrays on every rank, n <= 64 * round_words */
int ketogpu_part_begin(ketogpu_part *p, const uint32_t *roots, const uint32_t *targets, size_t n);
/* Same round, in a chosen direction (partition.hip header): KETOGPU_PART_FORWARD grows the
 * roots' closures X(r) (what ketogpu_part_begin does), KETOGPU_PART_BACKWARD grows the
 * targets' ancestor sets B(t) along interior-predecessor rows and pulls from the roots'
 * rows.  Same answers; every rank must use the same direction in a round. */
#define KETOGPU_PART_FORWARD 0
#define KETOGPU_PART_BACKWARD 1
int ketogpu_part_begin_dir(ketogpu_part *p, const uint32_t *roots, const uint32_t *targets, size_t n,
                           int32_t direction);
/* this step's outgoing records grouped by destination rank into send_dev; counts[world].
   world > 1: send_dev is complete on return (any stream may read it).  world == 1: the
   records stay where the kernels wrote them; pass send_dev (and counts[0]) straight to
   ketogpu_part_apply / _pull_answer, which then read them there, or call ketogpu_part_sync
   first: it copies them into send_dev for any other reader. */
int ketogpu_part_emit(ketogpu_part *p, ketogpu_record *send_dev, uint64_t capacity, uint64_t *counts);
/* OR received records into the owned state; *frontier = owned entries of the next level.
   The caller's contract: every record's a is a word of the round (a < ceil(n / 64) of the
   begin call, so a < round_words) — the kernel indexes the state with it unchecked, a record
   outside it is an out-of-bounds store.  b is checked: a node this rank does not own as
   interior (another rank's, a layout gap, an id >= N) fails the call with KETOGPU_EINVAL and
   *frontier = 0; the round is then left to ketogpu_part_abort.  ketogpu_part_pull_answer
   checks both fields (a < n of the begin call) and fails the same way. */
int ketogpu_part_apply(ketogpu_part *p, const ketogpu_record *recv_dev, uint64_t n, uint64_t *frontier);
/* the owned frontier's rows -> the next emit's records */
int ketogpu_part_expand(ketogpu_part *p);
/* after the last level: direct hits of owned targets + queries (request, interior node) */
int ketogpu_part_pull_emit(ketogpu_part *p, ketogpu_record *send_dev, uint64_t capacity, uint64_t *counts);
int ketogpu_part_pull_answer(ketogpu_part *p, const ketogpu_record *recv_dev, uint64_t n);
/* this rank's hit bits of the round (ceil(n/64) host words) and state reset */
int ketogpu_part_end(ketogpu_part *p, uint64_t *allowed_bits);
int ketogpu_part_abort(ketogpu_part *p);
/* wait for the partition's stream (world 1: first copies the last emit's records into its
   send_dev, which makes them readable elsewhere) */
int ketogpu_part_sync(ketogpu_part *p);
int ketogpu_part_stats_get(const ketogpu_part *p, ketogpu_part_stats *out);
/* on: every kernel launch of the partition is bracketed by hipEvents on its stream (a
 * measurement pass; each event costs a few microseconds of GPU idle) */
int ketogpu_part_set_timing(ketogpu_part *p, int32_t on);

/* --------------------------------------------- partitioned mode: whole rounds */
/* The same rounds as above with the exchange inside the library, so a Go host drives a
 * hash-partitioned PermissionEngine through ONE call per batch, like ketogpu_check_ids
 * (the engine is built once per process, internal/driver/registry_default.go:158-163;
 * SubjectIsAllowed's recursion, internal/check/engine.go:33-95, spread over ranks).
 *
 * A communicator joins the ranks of one partitioned network (one process per GPU):
 *   RCCL over xGMI  rank 0: ketogpu_comm_unique_id(id); broadcast id to every rank out of
 *                   band (a Go host: its own channel; tests: torch.distributed); then every
 *                   rank ketogpu_comm_new(id, rank, world, device) (ncclCommInitRank,
 *                   /opt/rocm/include/rccl/rccl.h:220).  Records are exchanged from device
 *                   memory on the partition's stream: grouped ncclSend/ncclRecv per peer
 *                   (rccl.h:700-725), counts and statuses by ncclAllGather.
 *   a transport     ketogpu_comm_from_transport(vtable): the caller moves host bytes (a Go
 *                   transport; the CPU tests use torch.distributed gloo).
 * Per BFS level every rank makes one small all-gather (each rank's per-destination record
 * counts plus its step status — a step that failed anywhere fails the round everywhere,
 * and a level where no rank sends anything ends the closure: no depth cutoff, R2) and one
 * all-to-all of the records; a round ends with one all-gather of the ranks' hit bits (the
 * answer is their OR).  Every rank calls ketogpu_part_check_ids with the same requests and
 * gets the full answer.  Rounds whose buffers overflow are retried with half the requests
 * on every rank; KETOGPU_PART_AUTO times one round in each direction (max over ranks, so
 * every rank decides alike) and keeps the faster. */
typedef struct ketogpu_comm ketogpu_comm;
#define KETOGPU_COMM_ID_BYTES 128
int ketogpu_comm_unique_id(uint8_t id[KETOGPU_COMM_ID_BYTES]);
int ketogpu_comm_new(const uint8_t id[KETOGPU_COMM_ID_BYTES], int32_t rank, int32_t world, int32_t device,
                     ketogpu_comm **out);
#define KETOGPU_REDUCE_MIN 0
#define KETOGPU_REDUCE_MAX 1
/* host-memory transport; every callback returns 0 on success.  Collective: every rank
 * calls the same callbacks in the same order. */
typedef struct {
    void *ctx;
    int32_t rank, world;
    /* every rank's `bytes` -> recv (world * bytes, rank order) */
    int (*allgather)(void *ctx, const void *send, void *recv, uint64_t bytes);
    /* send grouped by destination (send_bytes[world]) -> recv grouped by source
       (recv_bytes[world], known to the caller) */
    int (*alltoallv)(void *ctx, const void *send, const uint64_t *send_bytes, void *recv,
                     const uint64_t *recv_bytes);
    /* n u32 values reduced elementwise in place (KETOGPU_REDUCE_MIN / _MAX) */
    int (*allreduce_u32)(void *ctx, uint32_t *buf, uint64_t n, int32_t op);
} ketogpu_transport;
int ketogpu_comm_from_transport(const ketogpu_transport *t, ketogpu_comm **out);
void ketogpu_comm_free(ketogpu_comm *c);
/* RCCL calls a communicator made (counts since creation; a host transport's are 0).
 * KETOGPU_TEST_RCCL_SELF=1 when an RCCL communicator is made (tests): at world 1 too, the
 * all-to-alls move the rank's own segment with a grouped ncclSend/ncclRecv to itself and
 * the two-tier count gathers run as ncclAllGather, so one GPU executes the multi-GPU
 * data path (default: the own segment is a copy-engine DMA and world-1 gathers are skipped) */
typedef struct {
    int32_t rccl, loop_self;
    uint64_t sends, recvs, allgathers, allreduces, bytes_sent;
} ketogpu_comm_stats;
int ketogpu_comm_stats_get(const ketogpu_comm *c, ketogpu_comm_stats *out);
int ketogpu_comm_rank(const ketogpu_comm *c);
int ketogpu_comm_world(const ketogpu_comm *c);

/* ketogpu_shard_resolve_batch combined over the ranks (the owners' answers win):
 * status ENOTFOUND = a wildcard root (R5), which the partitioned engine does not evaluate;
 * EINVAL = nil subject.  comm NULL: a single rank. */
int ketogpu_part_resolve_batch(const ketogpu_shard *s, ketogpu_comm *c, const ketogpu_request_batch *reqs,
                               uint32_t *roots, uint32_t *targets, int32_t *status);

typedef struct ketogpu_part_engine ketogpu_part_engine;
#define KETOGPU_PART_AUTO (-1)
typedef struct {
    int32_t direction;        /* KETOGPU_PART_FORWARD, _BACKWARD or _AUTO                  */
    uint64_t record_capacity; /* records per exchange buffer; 0 = the partition's own      */
} ketogpu_part_engine_opts;
/* comm NULL: world 1 without any exchange (records stay where the kernels wrote them).
 * The engine borrows p and c (free it first). */
int ketogpu_part_engine_new(ketogpu_part *p, ketogpu_comm *c, const ketogpu_part_engine_opts *opts,
                            ketogpu_part_engine **out);
/* one batch: every rank passes the same requests (host memory), n any size; allowed_bits
 * ceil(n/64) words */
int ketogpu_part_check_ids(ketogpu_part_engine *e, const uint32_t *roots, const uint32_t *targets, size_t n,
                           uint64_t *allowed_bits);
typedef struct {
    int32_t direction;          /* the kept direction (KETOGPU_PART_AUTO before any round) */
    uint64_t trial_ns[2];       /* auto: ns per request of each direction's trial round     */
    uint64_t rounds, levels;    /* rounds run (trials and retries included), BFS levels     */
    uint64_t records_sent, records_received, retries, collectives;
    double exchange_ms;         /* host wall time inside collectives                        */
} ketogpu_part_engine_stats;
int ketogpu_part_engine_stats_get(const ketogpu_part_engine *e, ketogpu_part_engine_stats *out);
void ketogpu_part_engine_free(ketogpu_part_engine *e);

/* Test hook: the same driver over caller-provided steps in host memory (the CPU tests
 * play a rank's device steps with them, tests/part_cpu.py; the product passes a
 * ketogpu_part).  Callbacks mirror ketogpu_part_begin_dir / _emit (pull = 0) /
 * _pull_emit (pull = 1) / _apply / _expand / _pull_answer / _end / _abort. */
typedef struct {
    void *ctx;
    uint64_t round_words;
    int (*begin)(void *ctx, const uint32_t *roots, const uint32_t *targets, uint64_t n, int32_t direction);
    int (*emit)(void *ctx, int32_t pull, ketogpu_record *send, uint64_t capacity, uint64_t *counts);
    int (*apply)(void *ctx, const ketogpu_record *recv, uint64_t n, uint64_t *frontier);
    int (*expand)(void *ctx);
    int (*pull_answer)(void *ctx, const ketogpu_record *recv, uint64_t n);
    int (*end)(void *ctx, uint64_t *allowed_bits);
    int (*abort)(void *ctx);
} ketogpu_part_steps;
int ketogpu_part_engine_new_steps(const ketogpu_part_steps *steps, ketogpu_comm *c,
                                  const ketogpu_part_engine_opts *opts, ketogpu_part_engine **out);

/* ------------------------------------------- partitioned mode: two-tier */
/* The same hash-partitioned network (ketogpu_shard_*) checked with TWO exchanges per batch
 * instead of two per BFS level, when its CORE fits every GPU.  The core is the rows among
 * interior nodes: fint(v) and the interior predecessors of every interior node v (group
 * nesting: ~0.3% of config #5's tuples).  Every path r -> v1 -> ... -> t of the reference's
 * recursion (internal/check/engine.go:33-91) has v1 in fint(r), its last interior node in
 * rev(t) and everything between inside the core, so each rank keeps a copy of the core and
 * only the two seed rows of a request live elsewhere:
 *   queries  request i asks owner(r) for fint(r) and owner(t) for rev(t)  [all-to-all]
 *   replies  the owners send those rows                                     [all-to-all]
 *   evaluate the bidirectional LDS unit of the single-GPU engine over the local core
 * (plan label, the default: the owners reply with their nodes' 2-hop label lists instead
 * and the evaluation is one list intersection per request)
 * A world of one rank reads its own rows in place (no exchange at all).  Unlike
 * ketogpu_part_check_ids, every rank passes ITS OWN requests (any number, 0 included)
 * and gets the answers to them; the call is collective (every rank calls it for each of
 * its batches, as with the per-level engine).  Requests whose search outgrows the LDS
 * tables (none on the benchmark graphs) are answered by the per-level engine, built on
 * first need from the same shard and communicator.  Same answers as ketogpu_check_ids on
 * the whole graph (the R2 formula, no depth cutoff).
 *
 *   ketogpu_core_gather (collective, once per load) -> ketogpu_tier_new -> check_ids ...
 *
 * ketogpu_core_gather fails with KETOGPU_ENOMEM on every rank alike when the core passes
 * core_budget_bytes (the per-level engine is then the partitioned mode to use). */
typedef struct ketogpu_core ketogpu_core;
typedef struct {
    uint32_t num_interior;     /* Ni: core rows                                          */
    const uint64_t *f_off;     /* Ni + 1: interior successors of each interior node      */
    const uint32_t *f_col;
    const uint64_t *b_off;     /* Ni + 1: interior predecessors of each interior node    */
    const uint32_t *b_col;
    uint64_t bytes;            /* device bytes of the core's records                     */
} ketogpu_core_view;
/* opts: the shard's; comm NULL for a single rank.  core_budget_bytes 0: no limit here */
int ketogpu_core_gather(const ketogpu_shard *s, ketogpu_comm *comm, uint64_t core_budget_bytes, ketogpu_core **out);
int ketogpu_core_get_view(const ketogpu_core *c, ketogpu_core_view *out);
void ketogpu_core_free(ketogpu_core *c);

typedef struct ketogpu_tier ketogpu_tier;
typedef struct {
    int32_t device;
    uint64_t max_batch;            /* requests evaluated per step; 0 = 4M                */
    uint64_t fallback_state_bytes; /* the per-level engine's state budget; 0 = 2 GB      */
} ketogpu_tier_opts;
/* a request's query in transit: tag = request index << 1 | 0 (fint(r)) / 1 (rev(t)) */
typedef struct {
    uint32_t tag, node;
} ketogpu_tier_query;
/* a row entry in transit: the entry's node and its request's tag (the receiver looks the
 * entry's core row up in its own copy of the core) */
typedef struct {
    uint32_t node, tag;
} ketogpu_tier_rec;
typedef struct {
    uint64_t calls, batches, requests, overflow_requests, fallback_calls;
    uint64_t queries_sent, records_sent, records_received, collectives;
    uint64_t rows_opened, records_read; /* device statistics of the evaluation      */
    double exchange_ms, evaluate_ms;    /* host wall time inside collectives / evaluation */
    uint64_t core_records, seed_records; /* device records: core (both directions), own rows */
    double eval_kernel_ms;               /* hipEvent time of the first evaluation stage      */
    uint64_t eval_kernel_launches;
    /* plan label (KETOGPU_TIER_LABEL=0 at ketogpu_tier_new: off): owners answer a query with
     * the node's label list (masks + entries) instead of its row, and the evaluation is one
     * intersection per request (no later stage, no per-level fallback).  rows_opened: 2 per
     * request, records_read: list words read */
    uint64_t label;                      /* 1: plan label                                    */
    uint64_t label_words;                /* this rank's S and P list words (masks included)  */
    double label_build_ms;               /* labels of the core + the owned lists             */
} ketogpu_tier_stats;
/* the shard and core stay owned by the caller; the tier borrows s, core and comm */
int ketogpu_tier_new(const ketogpu_shard *s, const ketogpu_core *core, ketogpu_comm *comm,
                     const ketogpu_tier_opts *opts, ketogpu_tier **out);
/* this rank's n requests (host memory — pinned buffers are read in place — or the tier
 * device's memory, read in place by every pass) -> ceil(n/64) words of answer bits (host
 * memory).  An id outside the layout fails the call with
 * KETOGPU_EINVAL on that rank (its peers fail with the same code). */
int ketogpu_tier_check_ids(ketogpu_tier *t, const uint32_t *roots, const uint32_t *targets, size_t n,
                           uint64_t *allowed_bits);
int ketogpu_tier_stats_get(ketogpu_tier *t, ketogpu_tier_stats *out);
void ketogpu_tier_free(ketogpu_tier *t);
/* Test hook: the same protocol over caller steps in host memory (tests/tier_cpu.py).
 * queries: this rank's requests -> queries grouped by owner (counts[world]);
 * reply_sizes: received queries (grouped by source, from[world] each) -> records per
 * destination (counts[world]); reply_emit: those records, in query order;
 * evaluate: the answers (recv NULL: the rank owns every row, world 1) and the indices of
 * requests it could not finish (overflow; none for host steps). */
typedef struct {
    void *ctx;
    int (*queries)(void *ctx, const uint32_t *roots, const uint32_t *targets, uint64_t n, ketogpu_tier_query *send,
                   uint64_t *counts);
    int (*reply_sizes)(void *ctx, const ketogpu_tier_query *recv, uint64_t n, const uint64_t *from,
                       uint64_t *counts);
    int (*reply_emit)(void *ctx, ketogpu_tier_rec *send);
    int (*evaluate)(void *ctx, const uint32_t *roots, const uint32_t *targets, uint64_t n,
                    const ketogpu_tier_rec *recv, uint64_t nrecv, uint64_t *allowed_bits, uint32_t *overflow,
                    uint64_t *n_overflow);
} ketogpu_tier_steps;
int ketogpu_tier_new_steps(const ketogpu_tier_steps *steps, ketogpu_comm *comm, const ketogpu_tier_opts *opts,
                           ketogpu_tier **out);

/* ------------------------------------------------------------------ expand */
/* BuildTree(subject, rest_depth).  *out = NULL is the nil tree (JSON null).
 * KETOGPU_ENOTFOUND when a fetched page references an unknown namespace. */
int ketogpu_expand(const ketogpu_snapshot *s, const ketogpu_subject *subject, int32_t rest_depth,
                   ketogpu_tree **out);

#define KETOGPU_NODE_UNION 0
#define KETOGPU_NODE_LEAF 1
/* flattened tree in preorder; strings are owned by the tree */
typedef struct {
    int32_t type;         /* KETOGPU_NODE_UNION / KETOGPU_NODE_LEAF                */
    uint32_t num_children;/* the children follow in preorder                      */
    ketogpu_subject subject;
} ketogpu_tree_node;
int ketogpu_tree_nodes(const ketogpu_tree *t, const ketogpu_tree_node **nodes, size_t *n);
/* MarshalJSON of the tree (tree.go:156-162); free with ketogpu_free */
int ketogpu_tree_json(const ketogpu_tree *t, char **json);
void ketogpu_tree_free(ketogpu_tree *t);

/* ---------------------------------------------------------- reverse lookup */
/* "Which objects can this subject reach?" (OpenFGA ListObjects, SpiceDB LookupResources; the
 * reference has only the forward question, internal/check/engine.go:93-95).  For a target node
 * t and an object type T, lookup(t, T) is the set of expandable nodes r (r < num_expandable) of
 * type T for which SubjectIsAllowed(r, t) is true, without duplicates: the backward closure
 * B(t) over the reverse rows (DESIGN.md "Reverse lookup"), so its cost follows the answer and
 * not the namespace.  t itself is listed only when a cycle leads back to it (R2).
 *
 * The TYPE of an expandable node is its interned pair (namespace id, relation).  Wildcard
 * subject-set nodes (R5: an empty field) are expandable nodes like any other and are listed
 * under KETOGPU_TYPE_ANY, but have types of their own that no (namespace, relation) pair
 * resolves to, so a concrete type leaves them out.  Dynamic wildcard roots (queries without a
 * snapshot node) are not nodes and are never listed.  The placeholder nodes of a writable
 * snapshot are never listed.  Snapshots with shared Subject.String() keys (R4) are refused with
 * KETOGPU_EINVAL, as in the partitioned mode: the formula does not hold there.
 * (Additions within ABI 9: no existing entry point or struct layout changed.) */
#define KETOGPU_TYPE_ANY 0xFFFFFFFFu  /* no type filter                                      */
#define KETOGPU_TYPE_NONE 0xFFFFFFFEu /* matches nothing: unknown namespace or unused pair
                                         (R6: check maps NotFound to false)                 */
/* (namespace name, relation) -> type id, or KETOGPU_TYPE_NONE (the call still returns
 * KETOGPU_OK).  Type ids are stable for the life of the snapshot. */
int ketogpu_snapshot_type(const ketogpu_snapshot *s, const char *ns_name, const char *relation, uint32_t *type);
/* What a node id stands for.  The strings are pointer + length (not 0-terminated) into memory
 * owned by the snapshot, valid while it lives.  KETOGPU_EINVAL for ids >= num_nodes and for the
 * placeholder nodes of a writable snapshot. */
typedef struct {
    int32_t kind;         /* KETOGPU_SUBJECT_ID / KETOGPU_SUBJECT_SET                      */
    int32_t namespace_id; /* subject set: its namespace id; subject id: 0                  */
    uint32_t type;        /* expandable node: its type; any other node: KETOGPU_TYPE_NONE  */
    uint32_t expandable;  /* 1: id < num_expandable (the node can be listed)               */
    const char *ns;       /* subject set: configured name of namespace_id ("" if none)     */
    size_t ns_len;
    const char *id;       /* subject set: the object; subject id: the id                   */
    size_t id_len;
    const char *rel;      /* subject set: the relation                                     */
    size_t rel_len;
} ketogpu_node_info;
int ketogpu_snapshot_node(const ketogpu_snapshot *s, uint32_t id, ketogpu_node_info *out);
/* lookup(target, type) on the host, over the snapshot's reverse rows: *ids ascending, *n its
 * length; free *ids with ketogpu_free.  target KETOGPU_NODE_NONE: the empty list; any other
 * id >= num_nodes: KETOGPU_EINVAL.  Needs no GPU; the yardstick of ketogpu_lookup_ids. */
int ketogpu_snapshot_lookup(const ketogpu_snapshot *s, uint32_t target, uint32_t type, uint32_t **ids, uint64_t *n);

/* The device side: a handle of its own over the snapshot's reverse rows and type array in HBM.
 * Every call compares ketogpu_snapshot_version with the version it uploaded and uploads the
 * rows again when a ketogpu_snapshot_write moved it (O(reverse rows), not O(delta)). */
typedef struct ketogpu_lookup ketogpu_lookup;
typedef struct {
    int32_t device;              /* HIP device ordinal                                      */
    uint64_t state_budget_bytes; /* HBM for tier 2's per-slot state; 0 = at most 1/8 of the
                                    free HBM                                                */
} ketogpu_lookup_opts;
typedef struct {
    uint64_t requests;       /* since creation: targets passed in                          */
    uint64_t tier1_requests; /* answered by the one-wave LDS kernel                        */
    uint64_t tier2_requests; /* answered by the workgroup-per-request kernel               */
    uint64_t tier2_rounds;   /* tier-2 launches (each serves up to `slots` requests)       */
    uint64_t ids_produced;   /* sum of the exact list sizes                                */
    uint64_t truncated_lists;
    uint64_t uploads;        /* row uploads (1 at creation, +1 per version change seen)    */
    uint32_t set_capacity;   /* tier 1: nodes B(t) may hold before the request moves on    */
    uint32_t slots;          /* tier 2: requests per round (0 before the first round)      */
    double last_call_ms;     /* host wall time of the last ketogpu_lookup_ids              */
} ketogpu_lookup_stats;
/* KETOGPU_LOOKUP_TIER=2 (environment, read here) sends every request to tier 2;
 * KETOGPU_LOOKUP_SLOTS=k caps tier 2's slots. */
int ketogpu_lookup_new(const ketogpu_snapshot *s, const ketogpu_lookup_opts *opts, ketogpu_lookup **out);
void ketogpu_lookup_free(ketogpu_lookup *l);
int ketogpu_lookup_stats_get(const ketogpu_lookup *l, ketogpu_lookup_stats *out);
/* lookup(targets[i], type) for n targets in one call.  count[i] is always the exact size of
 * list i; begin[i] is the offset in `out` of list i, written completely, or a marker:
 * TRUNCATED (the list did not fit in `capacity` ids; nothing of it was written) or INVALID
 * (targets[i] >= num_nodes and not KETOGPU_NODE_NONE; count 0).  KETOGPU_NODE_NONE gives an
 * empty list.  *needed = the sum of all counts; needed <= capacity guarantees that nothing was
 * truncated (every request reserves exactly count[i] ids).  Lists lie in `out` in any order,
 * the ids inside a list in any order, without duplicates.  capacity 0 with out NULL is the
 * count-only call.  Returns KETOGPU_OK also when lists were truncated. */
#define KETOGPU_LOOKUP_TRUNCATED UINT64_MAX
#define KETOGPU_LOOKUP_INVALID (UINT64_MAX - 1)
int ketogpu_lookup_ids(ketogpu_lookup *l, const uint32_t *targets, size_t n, uint32_t type, uint32_t *out,
                       uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *needed);

/* Why is a check allowed?  For a root r and a target t a PATH is a sequence v0 = r, v1, ...,
 * vk = t with k >= 1 in which v(i+1) is an entry of the row of v(i) as the check engine sees it,
 * that is v(i) is in the reverse row of v(i+1).  A path exists exactly when SubjectIsAllowed(r, t)
 * (r in B(t)); the calls below return ONE path with the fewest hops, any of them when there are
 * several.  r == t is answered only through a cycle (R2): the path then starts and ends with r
 * (a self-loop: r, r).  There is no depth cutoff.  A denied pair gives the empty path, and so do
 * KETOGPU_NODE_NONE in either field and a root in [num_expandable, num_nodes); any other id
 * >= num_nodes in either field is invalid.  Under wildcard rows (R5) a hop may stand for a
 * wildcard match rather than a literal tuple.  R4 snapshots are refused with KETOGPU_EINVAL.
 * (Additions within ABI 9: no existing entry point or struct layout changed.)
 *
 * On the host, a breadth-first search over the reverse rows: *ids the path (r ... t), *n its
 * length (0: not allowed); free *ids with ketogpu_free.  An invalid id: KETOGPU_EINVAL.  Needs no
 * GPU; the yardstick of ketogpu_lookup_paths. */
int ketogpu_snapshot_path(const ketogpu_snapshot *s, uint32_t root, uint32_t target, uint32_t **ids, uint64_t *n);
/* On the device, on the lookup handle (its reverse rows are what is needed; no second upload):
 * one path per pair (roots[i], targets[i]).  The output contract is that of ketogpu_lookup_ids:
 * count[i] is the exact number of nodes on path i (hops + 1; 0 for a denied pair); each path
 * makes one reservation; begin[i] is the offset in `out` of path i, written completely in the
 * order r ... t, or KETOGPU_LOOKUP_TRUNCATED (it did not fit in `capacity` ids; nothing of it
 * was written) or KETOGPU_LOOKUP_INVALID (count 0).  *needed = the sum of all counts; capacity 0
 * with out NULL is the count-only call.  Returns KETOGPU_OK also when paths were truncated.  The
 * handle behaves as in its other calls (re-upload when ketogpu_snapshot_version has moved,
 * KETOGPU_EINVAL after the snapshot is freed, one call at a time, the same tier knobs).  A pair
 * whose root turns up before the LDS set passes set_capacity finishes in tier 1, whatever the
 * size of B(t).  Path calls do not move ketogpu_lookup_stats; they count here: */
typedef struct {
    uint64_t requests;       /* since creation: pairs passed in                            */
    uint64_t tier1_requests; /* searched and answered by the one-wave LDS kernel           */
    uint64_t tier2_requests; /* answered by the workgroup-per-request kernel               */
    uint64_t tier2_rounds;   /* tier-2 launches of path calls                              */
    uint64_t allowed;        /* pairs with a path                                          */
    uint64_t ids_produced;   /* sum of the exact path lengths                              */
    uint64_t truncated_lists;
} ketogpu_lookup_path_stats;
int ketogpu_lookup_path_stats_get(const ketogpu_lookup *l, ketogpu_lookup_path_stats *out);
int ketogpu_lookup_paths(ketogpu_lookup *l, const uint32_t *roots, const uint32_t *targets, size_t n, uint32_t *out,
                         uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *needed);

/* ------------------------------------------------------- subject listing */
/* "Who can reach this object?" (OpenFGA ListUsers, SpiceDB LookupSubjects).  For a root node r
 * and a class C, subjects(r, C) is the set of nodes t of class C for which SubjectIsAllowed(r, t)
 * is true, without duplicates: the forward closure F(r) = {t : r in B(t)} over the rows the
 * check engine sees (page-poison truncated, R7; wildcard rows materialized, R5) — the least set
 * that holds row(r) and row(x) for every interior x in it (DESIGN.md "Subject listing").  Its
 * cost follows the answer.  r itself is listed only when a cycle leads back to it (R2); there is
 * no depth cutoff.  Dynamic wildcard roots (queries without a snapshot node) are not nodes and
 * cannot be listed.  Snapshots with shared Subject.String() keys (R4) are refused with
 * KETOGPU_EINVAL, as in the reverse lookup.
 *
 * The CLASS of a node extends the reverse lookup's type to all num_nodes nodes: an expandable
 * node's class is its type (placeholders: KETOGPU_TYPE_NONE, never listed); a never-expanded
 * subject id is KETOGPU_CLASS_SUBJECT_ID; a never-expanded subject set (a group named as a
 * subject that has no rows of its own) has the type id of its (namespace id, relation) pair if
 * an expandable node defines that type, and KETOGPU_CLASS_UNTYPED_SET otherwise.  As a filter,
 * KETOGPU_TYPE_ANY lists every class but NONE, KETOGPU_CLASS_SUBJECT_ID "which users", a type
 * id "which groups#member"; KETOGPU_TYPE_NONE and KETOGPU_CLASS_UNTYPED_SET list nothing (an
 * untyped set shows under ANY only).
 * (Additions within ABI 9: no existing entry point or struct layout changed.) */
#define KETOGPU_CLASS_SUBJECT_ID 0xFFFFFFFDu
#define KETOGPU_CLASS_UNTYPED_SET 0xFFFFFFFCu
/* the class of node `id`; KETOGPU_EINVAL for ids >= num_nodes */
int ketogpu_snapshot_subject_class(const ketogpu_snapshot *s, uint32_t id, uint32_t *cls);
/* subjects(root, cls) on the host, a worklist closure over the snapshot's rows: *ids ascending,
 * *n its length; free *ids with ketogpu_free.  root KETOGPU_NODE_NONE (an unknown namespace, a
 * query no tuple matches) and roots in [num_expandable, num_nodes) give the empty list; any
 * other id >= num_nodes: KETOGPU_EINVAL.  Needs no GPU; the yardstick of ketogpu_subjects_ids. */
int ketogpu_snapshot_subjects(const ketogpu_snapshot *s, uint32_t root, uint32_t cls, uint32_t **ids, uint64_t *n);

/* The device side: a handle of its own over a compact copy of the forward rows (4 bytes per
 * edge) and the class array in HBM.  Every call compares ketogpu_snapshot_version with the
 * version it uploaded and uploads again when a ketogpu_snapshot_write moved it. */
typedef struct ketogpu_subjects ketogpu_subjects;
typedef struct {
    int32_t device;              /* HIP device ordinal                                      */
    uint64_t state_budget_bytes; /* HBM for tier 2's per-slot state; 0 = at most 1/8 of the
                                    free HBM                                                */
} ketogpu_subjects_opts;
typedef struct {
    uint64_t requests;       /* since creation: roots passed in                            */
    uint64_t tier1_requests; /* answered by the one-wave LDS kernel                        */
    uint64_t tier2_requests; /* answered by the workgroup-per-request kernel               */
    uint64_t tier2_rounds;   /* tier-2 launches (each serves up to `slots` requests)       */
    uint64_t list_finishes;  /* tier 2: closures within list_capacity, finished by walking
                                the seen list                                              */
    uint64_t scan_finishes;  /* tier 2: larger closures, finished by scanning the bitmap    */
    uint64_t ids_produced;   /* sum of the exact list sizes                                */
    uint64_t truncated_lists;
    uint64_t uploads;        /* row uploads (1 at creation, +1 per version change seen)    */
    uint32_t set_capacity;   /* tier 1: nodes F(r) may hold before the request moves on    */
    uint32_t slots;          /* tier 2: requests per round (0 before the first round)      */
    uint32_t list_capacity;  /* tier 2: entries of a slot's seen list                      */
    double last_call_ms;     /* host wall time of the last ketogpu_subjects_ids            */
} ketogpu_subjects_stats;
/* Environment, read here: KETOGPU_SUBJECTS_TIER=2 sends every request to tier 2;
 * KETOGPU_SUBJECTS_SLOTS=k caps tier 2's slots; KETOGPU_SUBJECTS_LIST_CAP=k sets list_capacity
 * (0: every tier-2 request finishes by scan). */
int ketogpu_subjects_new(const ketogpu_snapshot *s, const ketogpu_subjects_opts *opts, ketogpu_subjects **out);
void ketogpu_subjects_free(ketogpu_subjects *h);
int ketogpu_subjects_stats_get(const ketogpu_subjects *h, ketogpu_subjects_stats *out);
/* subjects(roots[i], cls) for n roots in one call.  The output contract is that of
 * ketogpu_lookup_ids: count[i] is always the exact size of list i; begin[i] is the offset in
 * `out` of list i, written completely, or KETOGPU_LOOKUP_TRUNCATED (the list did not fit in
 * `capacity` ids; nothing of it was written) or KETOGPU_LOOKUP_INVALID (roots[i] >= num_nodes
 * and not KETOGPU_NODE_NONE; count 0).  *needed = the sum of all counts; needed <= capacity
 * guarantees that nothing was truncated (every request reserves exactly count[i] ids).  Lists
 * lie in `out` in any order, the ids inside a list in any order, without duplicates.
 * capacity 0 with out NULL is the count-only call.  Returns KETOGPU_OK also when lists were
 * truncated. */
int ketogpu_subjects_ids(ketogpu_subjects *h, const uint32_t *roots, size_t n, uint32_t cls, uint32_t *out,
                         uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *needed);

/* ------------------------------------------------------- sorted, paged lists */
/* One page of lookup(targets[i], type) / subjects(roots[i], cls) per request, selected in
 * order on the device (Keto's list convention: page_size / page_token in, next_page_token out).
 * M(i) is the member set of request i exactly as ketogpu_lookup_ids / ketogpu_subjects_ids
 * define it: the filters, KETOGPU_NODE_NONE, never-expanded roots, placeholders and the R4
 * refusal all behave the same.
 *
 *   from         inclusive lower bounds; NULL means 0 for every request
 *   count[i]     = |M(i)|, exact, whatever from[i] is
 *   remaining[i] = |{m in M(i) : m >= from[i]}|
 *   returned[i]  = min(limit, remaining[i])
 *   out[i * limit .. i * limit + returned[i])  the returned[i] smallest members >= from[i],
 *                strictly ascending; the words of a stride past returned[i] are not to be read
 *
 * More pages exist exactly when remaining[i] > returned[i]; the next page starts at from =
 * last id + 1.  Any from >= num_nodes is legal and gives remaining 0.  An id outside the
 * snapshot (>= num_nodes and not KETOGPU_NODE_NONE) gives returned[i] = KETOGPU_PAGE_INVALID and
 * count = remaining = 0; the call still returns KETOGPU_OK.  limit 0, limit >
 * KETOGPU_PAGE_LIMIT_MAX, a null argument with n > 0 and n >= 2^31 give KETOGPU_EINVAL; n == 0
 * is KETOGPU_OK.  There is no truncation protocol: the stride is the reservation.
 *
 * THE ORDER IS BY NODE ID, not by name.  It is total, and stable for the life of a snapshot
 * object, in-place ketogpu_snapshot_write included (node ids never move; new subjects get
 * reserved ids), so a page token — the next `from` — stays meaningful between calls.
 *
 * The handle behaves as for the full-list calls (re-upload when ketogpu_snapshot_version has
 * moved, KETOGPU_EINVAL after the snapshot is freed, one call at a time, the same tier knobs),
 * and paged requests count into the same stats: requests, tier1_requests, tier2_requests,
 * tier2_rounds (and list_finishes / scan_finishes: how the slot was counted and cleared) as
 * for the full-list calls, ids_produced += the sum of returned; truncated_lists never moves.
 * (Additions within ABI 9: no existing entry point or struct layout changed.) */
#define KETOGPU_PAGE_LIMIT_MAX 65536u
#define KETOGPU_PAGE_INVALID 0xFFFFFFFFu /* in returned[i] */
int ketogpu_lookup_page(ketogpu_lookup *l, const uint32_t *targets, const uint32_t *from, size_t n, uint32_t type,
                        uint32_t limit, uint32_t *out /* n * limit words */, uint32_t *returned, uint64_t *count,
                        uint64_t *remaining);
int ketogpu_subjects_page(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *from, size_t n, uint32_t cls,
                          uint32_t limit, uint32_t *out /* n * limit words */, uint32_t *returned, uint64_t *count,
                          uint64_t *remaining);

/* ------------------------------------------------------- combined listings */
/* The list of a PAIR of ids under an operator, computed on the device: who can both submit and
 * approve (subjects AND), what a can see that b cannot (lookup ANDNOT), what a principal sees
 * under either of two identities without duplicates (lookup OR).  With M(x) the member set of
 * the plain call for x under the same filter — lookup(x, type) on the lookup handle,
 * subjects(x, cls) on the subjects handle —
 *
 *   KETOGPU_COMBINE_AND     M = M(a) n M(b)
 *   KETOGPU_COMBINE_ANDNOT  M = M(a) \ M(b)
 *   KETOGPU_COMBINE_OR      M = M(a) u M(b)
 *
 * M(x) keeps every rule of the plain call: x itself is a member only through a cycle,
 * placeholders are never listed, there is no depth cutoff, R4 snapshots are refused by the
 * handle.  A side that the plain call answers before it reads a row (KETOGPU_NODE_NONE; on the
 * subjects handle also a root in [num_expandable, num_nodes)) is the empty set and the operator
 * is applied as written: AND gives the empty list, ANDNOT M(a) or the empty list, OR the other
 * side.  An id >= num_nodes that is not KETOGPU_NODE_NONE, on either side, makes the pair
 * invalid (KETOGPU_LOOKUP_INVALID / KETOGPU_PAGE_INVALID, count 0).  a == b is legal.  An
 * operator outside the three gives KETOGPU_EINVAL for the whole call.
 *
 * ketogpu_*_combine follows the output contract of ketogpu_lookup_ids word for word (count[i]
 * exact, one reservation per list, a list written completely or begin[i] TRUNCATED, *needed the
 * sum of the counts, capacity 0 with out NULL counts only, ids in any order without
 * duplicates); ketogpu_*_combine_page that of ketogpu_lookup_page (ascending by node id, the
 * same from / returned / remaining rules and token meaning).  The argument checks are those of
 * the plain calls, with both id arrays required.
 *
 * Tier 1 runs both closures in LDS; a pair either of whose closures passes set_capacity (OR: whose
 * union does) goes to tier 2, which has a second bitmap per slot.  That buffer is allocated at
 * the first combined call that overflows and is counted against state_budget_bytes with the
 * rest of a slot, so a combined round may have fewer slots than a plain one.  The tier knobs of
 * the handle apply.  Combined calls do not move ketogpu_lookup_stats / ketogpu_subjects_stats;
 * they count here (invalid pairs, and pairs neither side of which has a row to read, belong to
 * neither tier):
 * (Additions within ABI 9: no existing entry point or struct layout changed.) */
#define KETOGPU_COMBINE_AND 0u
#define KETOGPU_COMBINE_ANDNOT 1u
#define KETOGPU_COMBINE_OR 2u
typedef struct {
    uint64_t requests;       /* since creation: pairs passed in                            */
    uint64_t tier1_requests; /* answered by the one-wave LDS kernel                        */
    uint64_t tier2_requests; /* answered by the workgroup-per-pair kernel                  */
    uint64_t tier2_rounds;   /* tier-2 launches of combined calls                          */
    uint64_t ids_produced;   /* sum of the exact list sizes (pages: of returned)           */
    uint64_t truncated_lists;
    uint32_t slots;          /* tier 2: pairs per round (0 before the first round)         */
    double last_call_ms;     /* host wall time of the last combined call                   */
} ketogpu_combine_stats;
int ketogpu_lookup_combine_stats_get(const ketogpu_lookup *l, ketogpu_combine_stats *out);
int ketogpu_subjects_combine_stats_get(const ketogpu_subjects *h, ketogpu_combine_stats *out);
int ketogpu_lookup_combine(ketogpu_lookup *l, const uint32_t *a, const uint32_t *b, size_t n, uint32_t op,
                           uint32_t type, uint32_t *out, uint64_t capacity, uint64_t *begin, uint64_t *count,
                           uint64_t *needed);
int ketogpu_lookup_combine_page(ketogpu_lookup *l, const uint32_t *a, const uint32_t *b, const uint32_t *from,
                                size_t n, uint32_t op, uint32_t type, uint32_t limit,
                                uint32_t *out /* n * limit words */, uint32_t *returned, uint64_t *count,
                                uint64_t *remaining);
int ketogpu_subjects_combine(ketogpu_subjects *h, const uint32_t *a, const uint32_t *b, size_t n, uint32_t op,
                             uint32_t cls, uint32_t *out, uint64_t capacity, uint64_t *begin, uint64_t *count,
                             uint64_t *needed);
int ketogpu_subjects_combine_page(ketogpu_subjects *h, const uint32_t *a, const uint32_t *b, const uint32_t *from,
                                  size_t n, uint32_t op, uint32_t cls, uint32_t limit,
                                  uint32_t *out /* n * limit words */, uint32_t *returned, uint64_t *count,
                                  uint64_t *remaining);

/* -------------------------------------------------- depth-limited listings */
/* The members of a listing within k hops of its start, computed on the device: "who holds this
 * document directly, who through one group, who through any chain" is the closure cut at 1, 2
 * and no limit.  The plain, paged, combined and path calls above have no depth cutoff; these do.
 *
 * A listing starts from a node x: the target t of a lookup, the root r of a subject listing.
 * For a member u, d(x, u) is the number of hops of a shortest path, the one
 * ketogpu_snapshot_path defines: its count - 1, at least 1.  Level 1 is the set of entries of
 * x's own row; level d + 1 is what the rows of the interior members of level d add for the
 * first time.  With M(x) the member set of the plain call under the same type / class filter,
 *
 *   M_k(x) = { u in M(x) : d(x, u) <= k }
 *
 * x itself is a member only through a cycle of at most k hops, placeholders are never members,
 * R4 snapshots are refused by the handle, and KETOGPU_NODE_NONE, never-expanded roots and ids
 * outside the snapshot are classified as in the plain call.
 *
 * max_depth is given PER REQUEST, as an array next to the ids: max_depth[i] hops for request i,
 * KETOGPU_DEPTH_ALL (0) for no limit.  A null array is no limit for every request.  An unlimited
 * request returns the member set of the plain call (order and offsets are free, as always).
 *
 * frontier[i] is the number of interior members (ids < num_interior, as ketogpu_snapshot_graph
 * reports it for the current version) at distance exactly max_depth[i]: the members whose rows
 * the limit left unread.  0 means that the list is the
 * whole closure ("complete"); > 0 means that deeper levels MAY hold more.  It is 0 for every
 * unlimited request and for every request answered before a row is read.  `frontier` may be null.
 *
 * This is NOT Keto's expand at a depth.  BuildTree shares one visited map across a depth-first
 * walk, so which occurrence of a node is expanded, and with it what a depth cuts off, depends on
 * row order; here the distance is the breadth-first one and the answer is a set.  No parity with
 * ketogpu_expand at a max depth is claimed.
 *
 * ketogpu_*_ids_depth follows the output contract of ketogpu_lookup_ids word for word (count[i]
 * exact, one reservation per list, a list written completely or begin[i] TRUNCATED, *needed the
 * sum of the counts, capacity 0 with out NULL counts only); ketogpu_*_page_depth that of
 * ketogpu_lookup_page (ascending by node id, the same from / returned / remaining rules and
 * token meaning; a token belongs to a (request, depth) pair as it belongs to a (request, filter)
 * pair).  The argument checks are those of the plain calls.  The host calls return their ids
 * ascending and give KETOGPU_EINVAL for an id outside the snapshot.
 *
 * Tier 1 stops before it reads a row of level max_depth, so a request goes to tier 2 exactly
 * when its unfiltered M_k, not its whole closure, passes set_capacity.  Tier 2 needs no state
 * beyond the plain calls' slots.  The tier knobs of the handle apply.  Depth calls do not move
 * ketogpu_lookup_stats / ketogpu_subjects_stats; they count here:
 * (Additions within ABI 9: no existing entry point or struct layout changed.) */
#define KETOGPU_DEPTH_ALL 0u
typedef struct {
    uint64_t requests;       /* since creation: requests passed in                         */
    uint64_t tier1_requests; /* answered by the one-wave LDS kernel                        */
    uint64_t tier2_requests; /* answered by the workgroup-per-request kernel               */
    uint64_t tier2_rounds;   /* tier-2 launches of depth calls                             */
    uint64_t list_finishes;  /* subjects handle, tier 2: finished by the seen list ...     */
    uint64_t scan_finishes;  /* ... and by a scan of the bitmap (both 0 on the lookup handle) */
    uint64_t cut_requests;   /* requests with a non-zero frontier                          */
    uint64_t ids_produced;   /* sum of the exact list sizes (pages: of returned)           */
    uint64_t truncated_lists;
    uint32_t slots;          /* tier 2: requests per round (0 before the first round)      */
    double last_call_ms;     /* host wall time of the last depth call                      */
} ketogpu_depth_stats;
int ketogpu_lookup_depth_stats_get(const ketogpu_lookup *l, ketogpu_depth_stats *out);
int ketogpu_subjects_depth_stats_get(const ketogpu_subjects *h, ketogpu_depth_stats *out);
/* host (no GPU): *ids malloc'ed, ascending, free with ketogpu_free; *frontier may be null */
int ketogpu_snapshot_lookup_depth(const ketogpu_snapshot *s, uint32_t target, uint32_t type, uint32_t max_depth,
                                  uint32_t **ids, uint64_t *n, uint64_t *frontier);
int ketogpu_snapshot_subjects_depth(const ketogpu_snapshot *s, uint32_t root, uint32_t cls, uint32_t max_depth,
                                    uint32_t **ids, uint64_t *n, uint64_t *frontier);
int ketogpu_lookup_ids_depth(ketogpu_lookup *l, const uint32_t *targets, const uint32_t *max_depth, size_t n,
                             uint32_t type, uint32_t *out, uint64_t capacity, uint64_t *begin, uint64_t *count,
                             uint64_t *frontier, uint64_t *needed);
int ketogpu_subjects_ids_depth(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *max_depth, size_t n,
                               uint32_t cls, uint32_t *out, uint64_t capacity, uint64_t *begin, uint64_t *count,
                               uint64_t *frontier, uint64_t *needed);
int ketogpu_lookup_page_depth(ketogpu_lookup *l, const uint32_t *targets, const uint32_t *max_depth,
                              const uint32_t *from, size_t n, uint32_t type, uint32_t limit,
                              uint32_t *out /* n * limit words */, uint32_t *returned, uint64_t *count,
                              uint64_t *remaining, uint64_t *frontier);
int ketogpu_subjects_page_depth(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *max_depth,
                                const uint32_t *from, size_t n, uint32_t cls, uint32_t limit,
                                uint32_t *out /* n * limit words */, uint32_t *returned, uint64_t *count,
                                uint64_t *remaining, uint64_t *frontier);

/* -------------------------------------------------- listings that say why */
/* Next to every member of a listing, the node whose row grants it and how far from the start it
 * is: one line per viewer saying through which group and at what distance.  This is the
 * breadth-first grant tree of a closure, computed by the search that produced the list.
 *
 * In the terms of the depth section above (start x, members M_k(x) under the call's type / class
 * filter, d(x, u) the hop count of ketogpu_snapshot_path), for every listed member u:
 *
 *   hops(u) = d(x, u): exact, at least 1, and deterministic.
 *   via(u)  = a node at distance hops(u) - 1 from x that is joined to u by one edge of the
 *             closure.  For hops(u) == 1 it is x; otherwise it is an interior member of the
 *             unfiltered closure.  On the subjects handle u is an entry of row(via): the chain
 *             reads x -> ... -> via -> u.  On the lookup handle via is an entry of row(u): the
 *             chain reads u -> via -> ... -> x.  Where several nodes qualify (a diamond) any of
 *             them is correct, and the device and the host may pick different ones.
 *
 * via is a node id whatever the filter says: under a concrete type or class it may name a node
 * that is not itself listed.  Under KETOGPU_TYPE_ANY every via is x or a listed member whose
 * hops is one less, so the answer is a complete tree: following via from any member ends at x
 * after hops steps.  x as a member (through a cycle, R2) has the cycle's length as hops and its
 * predecessor on the cycle as via; a self-loop gives via == x, hops == 1.  Placeholders are
 * never a via.  R4 snapshots, KETOGPU_NODE_NONE, never-expanded roots and ids outside the
 * snapshot behave as in the plain calls.  No parity with ketogpu_expand is claimed: a member
 * appears once here, and the shape does not depend on row order beyond the choice in a diamond.
 *
 * ketogpu_*_ids_via follows the contract of ketogpu_*_ids_depth word for word (max_depth per
 * request, NULL or KETOGPU_DEPTH_ALL for no limit; count[i] exact; one reservation per list; a
 * list written completely or begin[i] TRUNCATED; needed and frontier as there; capacity 0 with
 * NULL arrays counts only).  via[k] and hops[k] belong to out[k], `capacity` words each; where a
 * list is truncated nothing of the three arrays is written.  via and hops may each be NULL: the
 * NULL array is not written.  ketogpu_*_page_via follows ketogpu_*_page_depth and adds via and
 * hops of n * limit words at the same stride, valid for the first returned[i] entries of row i.
 * The host calls return ids ascending with via and hops parallel to them (each may be NULL);
 * their via is the parent their breadth-first search meets first.
 *
 * The tier rule is the depth calls'.  Tier 2 keeps a parent and a hop word per id below the
 * member bound (num_expandable on the lookup handle, num_nodes on the subjects handle): 8 bytes
 * x bound per slot on top of the plain calls' slots, so under the same state_budget_bytes a via
 * round may have fewer slots; `slots` below reports them.  Via calls count only here: the plain,
 * depth, combine and path statistics do not move.
 * (Additions within ABI 9: no existing entry point or struct layout changed.) */
typedef struct {
    uint64_t requests;       /* since creation: requests passed in                         */
    uint64_t tier1_requests; /* answered by the one-wave LDS kernel                        */
    uint64_t tier2_requests; /* answered by the workgroup-per-request kernel               */
    uint64_t tier2_rounds;   /* tier-2 launches of via calls                               */
    uint64_t list_finishes;  /* subjects handle, tier 2: finished by the seen list ...     */
    uint64_t scan_finishes;  /* ... and by a scan of the bitmap (both 0 on the lookup handle) */
    uint64_t cut_requests;   /* requests with a non-zero frontier                          */
    uint64_t ids_produced;   /* sum of the exact list sizes (pages: of returned)           */
    uint64_t truncated_lists;
    uint32_t slots;          /* tier 2: requests per via round (0 before the first round)  */
    double last_call_ms;     /* host wall time of the last via call                        */
} ketogpu_via_stats;
int ketogpu_lookup_via_stats_get(const ketogpu_lookup *l, ketogpu_via_stats *out);
int ketogpu_subjects_via_stats_get(const ketogpu_subjects *h, ketogpu_via_stats *out);
/* host (no GPU): *ids, *via, *hops malloc'ed, *n words each, free each with ketogpu_free; via,
 * hops and frontier may be null */
int ketogpu_snapshot_lookup_via(const ketogpu_snapshot *s, uint32_t target, uint32_t type, uint32_t max_depth,
                                uint32_t **ids, uint32_t **via, uint32_t **hops, uint64_t *n, uint64_t *frontier);
int ketogpu_snapshot_subjects_via(const ketogpu_snapshot *s, uint32_t root, uint32_t cls, uint32_t max_depth,
                                  uint32_t **ids, uint32_t **via, uint32_t **hops, uint64_t *n, uint64_t *frontier);
int ketogpu_lookup_ids_via(ketogpu_lookup *l, const uint32_t *targets, const uint32_t *max_depth, size_t n,
                           uint32_t type, uint32_t *out, uint32_t *via, uint32_t *hops, uint64_t capacity,
                           uint64_t *begin, uint64_t *count, uint64_t *frontier, uint64_t *needed);
int ketogpu_subjects_ids_via(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *max_depth, size_t n,
                             uint32_t cls, uint32_t *out, uint32_t *via, uint32_t *hops, uint64_t capacity,
                             uint64_t *begin, uint64_t *count, uint64_t *frontier, uint64_t *needed);
int ketogpu_lookup_page_via(ketogpu_lookup *l, const uint32_t *targets, const uint32_t *max_depth,
                            const uint32_t *from, size_t n, uint32_t type, uint32_t limit,
                            uint32_t *out /* n * limit words */, uint32_t *via /* n * limit words or NULL */,
                            uint32_t *hops /* n * limit words or NULL */, uint32_t *returned, uint64_t *count,
                            uint64_t *remaining, uint64_t *frontier);
int ketogpu_subjects_page_via(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *max_depth,
                              const uint32_t *from, size_t n, uint32_t cls, uint32_t limit,
                              uint32_t *out /* n * limit words */, uint32_t *via /* n * limit words or NULL */,
                              uint32_t *hops /* n * limit words or NULL */, uint32_t *returned, uint64_t *count,
                              uint64_t *remaining, uint64_t *frontier);

/* ------------------------------------------------- listing handles and in-place writes
 * A listing handle over a KETOGPU_BUILD_WRITABLE snapshot follows ketogpu_snapshot_write by
 * replaying the snapshot's patch log: the rows a write rewrote are packed on the host, copied
 * once and scattered by one kernel ahead of the call's own, so the first call after a write
 * costs what the write touched.  The lookup handle overwrites reverse rows where they lie;
 * the subjects handle keeps every forward row in an arena with the host's growth rule
 * (capacity len + len / 4 + 4) and moves a row that outgrew its capacity to the arena's tail.
 * The handle uploads everything again (a FULL upload) at creation, when the log was trimmed
 * below its position, when the backlog's rows exceed a quarter of a full upload's bytes, when
 * the arena's tail is exhausted or its garbage passes max(num_edges / 4, 2^20) words (a
 * compaction), and on every version change under KETOGPU_LIST_REFRESH=full (env, read at
 * *_new).  KETOGPU_LIST_ARENA_SLACK (env, words) sets the arena's tail headroom, and
 * KETOGPU_LIST_ARENA_GARBAGE (env, words, read at *_new) replaces the garbage bound
 * max(num_edges / 4, 2^20); unset, the default holds.  fallbacks_trimmed is defensive: a
 * registered reader is never trimmed past.  The
 * subjects handle's tier-2 bitmaps span num_nodes rounded up to a multiple of
 * KETOGPU_LIST_BOUND_STEP (env, default 32768), so that a new subject seldom moves the span:
 * when it does, tier 2's state is dropped and the next tier-2 call allocates it again.
 * (Additions within ABI 9: no existing entry point or struct layout changed.) */
typedef struct {
    uint64_t full_uploads;      /* 1 at creation, +1 per refresh served by a full upload      */
    uint64_t patched_refreshes; /* refreshes served by the patch kernel                       */
    uint64_t rows_patched;      /* rows the patch kernel rewrote                              */
    uint64_t rows_moved;        /* ... of them moved to the arena's tail (subjects handle)    */
    uint64_t words_uploaded;    /* 4-byte words copied to the device by patched refreshes     */
    uint64_t compactions;       /* full uploads because the arena needed compaction           */
    uint64_t fallbacks_trimmed; /* full uploads because the log was trimmed below the handle  */
    uint64_t fallbacks_backlog; /* full uploads because the backlog outweighed them           */
    double last_refresh_ms;     /* host wall time of the last refresh that moved the version  */
} ketogpu_list_refresh_stats;
int ketogpu_lookup_refresh_stats_get(const ketogpu_lookup *l, ketogpu_list_refresh_stats *out);
int ketogpu_subjects_refresh_stats_get(const ketogpu_subjects *h, ketogpu_list_refresh_stats *out);

/* A host-side reader of a writable snapshot's patch log, for tests and integrators that keep
 * state of their own per row.  An entry names a row a committed write rewrote:
 * KETOGPU_PATCH_FORWARD_INTERIOR the interior successors of an expandable node (the check
 * engine's forward row), KETOGPU_PATCH_REVERSE the reverse row of a node (what
 * ketogpu_snapshot_lookup walks), KETOGPU_PATCH_FORWARD_FULL the full forward row of an
 * expandable node (what ketogpu_snapshot_subjects walks).  A reader starts at the log's end,
 * registers like an engine (the log is kept from its position on until it is freed) and
 * advances by what it reads: _next copies up to `capacity` entries, in write order, and sets
 * *n to their number (0: nothing pending).  A refused write logs nothing.  On a snapshot that
 * is not writable the log stays empty. */
#define KETOGPU_PATCH_FORWARD_INTERIOR 0
#define KETOGPU_PATCH_REVERSE 1
#define KETOGPU_PATCH_FORWARD_FULL 2
typedef struct ketogpu_patch_reader ketogpu_patch_reader;
int ketogpu_patch_reader_new(const ketogpu_snapshot *s, ketogpu_patch_reader **out);
int ketogpu_patch_reader_next(ketogpu_patch_reader *r, uint8_t *kinds, uint32_t *nodes, size_t capacity, size_t *n);
/* the reader's absolute position and the range of the log the snapshot still keeps (each may be null) */
int ketogpu_patch_reader_position(const ketogpu_patch_reader *r, uint64_t *position, uint64_t *log_begin,
                                  uint64_t *log_end);
void ketogpu_patch_reader_free(ketogpu_patch_reader *r);

/* ------------------------------------------------------------- expand as id arrays
 * BuildTree in batches.  A tree is two parallel arrays in preorder: nodes[k], a snapshot node
 * id, and num_children[k]; node k is a Union iff num_children[k] > 0 (a Union of ketogpu_expand
 * always has children) and a Leaf otherwise.  It is the layout of ketogpu_tree_nodes with ids
 * in place of strings; ketogpu_tree_from_ids turns it into a ketogpu_tree, so
 * ketogpu_tree_nodes and ketogpu_tree_json read a device answer.
 *
 * ketogpu_snapshot_expand_ids is ketogpu_expand's walk on the host without strings, over a root
 * that is a snapshot node (KETOGPU_EINVAL for any other id): the same visited map (one per tree,
 * keyed by Subject.String()), the same paging, KETOGPU_ENOTFOUND exactly where ketogpu_expand
 * returns it (the arrays are NULL then).  *n == 0 is the nil tree.  *flags bit 0
 * (KETOGPU_EXPAND_NEEDS_HOST): the walk made a first visit to a node whose query has a row
 * with an unknown namespace, whether or not the reference then fails (it fails only when it
 * fetches the page with that row).  rest_depth 0 is the nil tree, KETOGPU_EXPAND_DEPTH_ALL no
 * limit (KETOGPU_DEPTH_ALL is 0, which is the nil tree here).  Free both arrays with
 * ketogpu_free.
 *
 * ketogpu_subjects_expand is the device call, on the subjects handle, with the output contract
 * of ketogpu_subjects_ids: count[i] the exact tree size; begin[i] the tree's offset in both
 * output arrays, or KETOGPU_LOOKUP_TRUNCATED (nothing of the tree was written) or
 * KETOGPU_LOOKUP_INVALID (roots[i] >= num_nodes and not KETOGPU_NODE_NONE; status NIL);
 * *needed the sum of the counts; capacity 0 with NULL outputs only counts.  status[i]:
 * KETOGPU_EXPAND_OK; KETOGPU_EXPAND_NIL (count 0: the nil tree; KETOGPU_NODE_NONE, a subject
 * set without rows, rest_depth 0); KETOGPU_EXPAND_HOST (count 0, nothing written: ask
 * ketogpu_expand), given exactly when the host twin would set KETOGPU_EXPAND_NEEDS_HOST, or
 * when the snapshot has shared Subject.String() keys (R4; every request then).  A subject-id
 * root gives one leaf.  Roots that are no snapshot node (dynamic wildcard queries, unknown
 * names) are ketogpu_expand's business.  Every OK tree equals the host twin's word for word.
 *
 * Tier 1 is one wave per request: a pre-order walk with the visited set and the DFS stack in
 * LDS, 64 row entries per step.  A request that opens more than set_capacity nodes moves to
 * tier 2 (KETOGPU_SUBJECTS_TIER=2 forces it): one workgroup per request, the slot's bitmap as
 * the visited set, 256 entries per step, and a stack of 2 words per node that has rows in
 * global memory, counted against state_budget_bytes.  A request walks twice, once to count and
 * once to write; a count-only call walks once.  Expand calls count only here: no other
 * statistics move.
 * (Additions within ABI 9: no existing entry point or struct layout changed.) */
#define KETOGPU_EXPAND_DEPTH_ALL 0xFFFFFFFFu
#define KETOGPU_EXPAND_NEEDS_HOST 1u
#define KETOGPU_EXPAND_OK 0u
#define KETOGPU_EXPAND_NIL 1u
#define KETOGPU_EXPAND_HOST 2u
int ketogpu_snapshot_expand_ids(const ketogpu_snapshot *s, uint32_t root, uint32_t rest_depth, uint32_t **nodes,
                                uint32_t **num_children, uint64_t *n, uint32_t *flags);
/* KETOGPU_EINVAL for arrays that are no preorder tree of snapshot nodes; n == 0: *tree = NULL */
int ketogpu_tree_from_ids(const ketogpu_snapshot *s, const uint32_t *nodes, const uint32_t *num_children, uint64_t n,
                          ketogpu_tree **tree);
typedef struct {
    uint64_t requests;       /* since creation: requests passed in                         */
    uint64_t tier1_requests; /* walked by the one-wave LDS kernel                          */
    uint64_t tier2_requests; /* walked by the workgroup-per-request kernel                 */
    uint64_t tier2_rounds;   /* tier-2 launches of expand calls                            */
    uint64_t host_requests;  /* status KETOGPU_EXPAND_HOST                                 */
    uint64_t nodes_produced; /* sum of the exact tree sizes                                */
    uint64_t truncated_trees;
    uint32_t slots;          /* tier 2: requests per expand round (0 before the first)     */
    double last_call_ms;     /* host wall time of the last expand call                     */
} ketogpu_expand_stats;
int ketogpu_subjects_expand_stats_get(const ketogpu_subjects *h, ketogpu_expand_stats *out);
int ketogpu_subjects_expand(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *rest_depth, size_t n,
                            uint32_t *out_nodes, uint32_t *out_children, uint64_t capacity, uint64_t *begin,
                            uint64_t *count, uint32_t *status, uint64_t *needed);

/* ------------------------------------------------------- chip-wide closures */
/* ketogpu_subjects_ids / ketogpu_lookup_ids with a third way to run a closure, the wide tier, in
 * place of tier 2 (DESIGN.md "Chip-wide closures").  The output contract is that of the plain
 * calls word for word: count[i] exact; a list written completely or KETOGPU_LOOKUP_TRUNCATED; an
 * id outside the snapshot KETOGPU_LOOKUP_INVALID; KETOGPU_NODE_NONE and ids without rows the
 * empty list; *needed the sum of the counts; capacity 0 with out NULL counts only; ids and lists
 * in any order, without duplicates; the same filters, the same refusal of a snapshot with shared
 * Subject.String() keys, the same following of in-place writes.
 *
 * Tier 1 runs as in the plain calls.  A request whose closure passes set_capacity runs in the
 * wide tier, `slots` requests per round: level-synchronous across the whole device, one launch
 * per level, its work items chunks of `chunk` entries of one row, so that a row of a million
 * entries is read by about 500 waves; the host reads the number of new items behind each level.
 * KETOGPU_SUBJECTS_TIER=2 / KETOGPU_LOOKUP_TIER=2 send every request that has a row to the wide
 * tier, KETOGPU_SUBJECTS_SLOTS / KETOGPU_LOOKUP_SLOTS cap its round.  The round's queue of work
 * items is counted against state_budget_bytes with tier 2's state, whose bitmaps it shares.
 * Wide calls count only here: no other statistics move, and no plain call is routed here.
 * (Additions within ABI 9: no existing entry point or struct layout changed.) */
typedef struct {
    uint64_t requests;       /* since creation: requests passed to wide calls              */
    uint64_t tier1_requests; /* answered by the one-wave LDS kernel                        */
    uint64_t wide_requests;  /* answered by the wide tier                                  */
    uint64_t wide_rounds;    /* rounds of the wide tier (each serves up to `slots`)        */
    uint64_t levels;         /* level launches, summed over the rounds                     */
    uint64_t items;          /* work items processed                                       */
    uint64_t ids_produced;   /* sum of the exact list sizes                                */
    uint64_t truncated_lists;
    uint32_t slots;          /* requests per wide round (0 before the first round)         */
    uint32_t chunk;          /* row entries per work item                                  */
    double last_call_ms;     /* host wall time of the last wide call                       */
} ketogpu_wide_stats;
int ketogpu_subjects_wide_stats_get(const ketogpu_subjects *h, ketogpu_wide_stats *out);
int ketogpu_lookup_wide_stats_get(const ketogpu_lookup *l, ketogpu_wide_stats *out);
int ketogpu_subjects_ids_wide(ketogpu_subjects *h, const uint32_t *roots, size_t n, uint32_t cls, uint32_t *out,
                              uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *needed);
int ketogpu_lookup_ids_wide(ketogpu_lookup *l, const uint32_t *targets, size_t n, uint32_t type, uint32_t *out,
                            uint64_t capacity, uint64_t *begin, uint64_t *count, uint64_t *needed);
/* The depth-limited and the paged calls with the same replacement (DESIGN.md "Chip-wide pages and
 * depths").  ketogpu_*_ids_depth_wide follows ketogpu_*_ids_depth word for word, ketogpu_*_page_wide
 * follows ketogpu_*_page_depth word for word: the same member sets M_k(x), frontier, counts, page
 * rules (ascending by node id; from / returned / remaining; KETOGPU_PAGE_INVALID; the limit
 * checks; no truncation protocol), argument checks and INVALID / NONE / never-expanded
 * classification.  A NULL max_depth array, or KETOGPU_DEPTH_ALL, is no limit: a paged call without
 * a limit is ketogpu_*_page_wide with max_depth NULL, and answers what ketogpu_*_page answers.
 * from and frontier may be NULL.  The depth tier-1 kernels run unchanged and a request overflows
 * exactly as in the depth calls; the overflows run in rounds of the wide tier, whose level L is
 * its launch L: a request with the limit k appends nothing after launch k.  A page is selected
 * by one workgroup per request; the bitmap is then cleared, and the members below `from`
 * counted, by one workgroup per tile of ketogpu_wide_clear_tile_ids() ids.  These calls count in
 * ketogpu_wide_stats alone (ids_produced: the sum of `returned` for pages; truncated_lists moves
 * only in the full-list calls); ketogpu_depth_stats does not move.
 * (Additions within ABI 9: no existing entry point or struct layout changed.) */
int ketogpu_subjects_ids_depth_wide(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *max_depth, size_t n,
                                    uint32_t cls, uint32_t *out, uint64_t capacity, uint64_t *begin, uint64_t *count,
                                    uint64_t *frontier, uint64_t *needed);
int ketogpu_lookup_ids_depth_wide(ketogpu_lookup *l, const uint32_t *targets, const uint32_t *max_depth, size_t n,
                                  uint32_t type, uint32_t *out, uint64_t capacity, uint64_t *begin, uint64_t *count,
                                  uint64_t *frontier, uint64_t *needed);
int ketogpu_subjects_page_wide(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *max_depth,
                               const uint32_t *from, size_t n, uint32_t cls, uint32_t limit,
                               uint32_t *out /* n * limit words */, uint32_t *returned, uint64_t *count,
                               uint64_t *remaining, uint64_t *frontier);
int ketogpu_lookup_page_wide(ketogpu_lookup *l, const uint32_t *targets, const uint32_t *max_depth,
                             const uint32_t *from, size_t n, uint32_t type, uint32_t limit,
                             uint32_t *out /* n * limit words */, uint32_t *returned, uint64_t *count,
                             uint64_t *remaining, uint64_t *frontier);
/* ids one workgroup of the paged finish's clear kernel covers */
uint32_t ketogpu_wide_clear_tile_ids(void);

/* ------------------------------------------------------- chip-wide BuildTree */
/* ketogpu_subjects_expand with the copying spread over the device (DESIGN.md "Chip-wide
 * BuildTree").  The arguments and the output contract are those of ketogpu_subjects_expand word
 * for word: count[i] the exact tree size; begin[i] the tree's offset in both output arrays, or
 * KETOGPU_LOOKUP_TRUNCATED (nothing of the tree was written) or KETOGPU_LOOKUP_INVALID; *needed
 * the sum of the counts; capacity 0 with NULL outputs only counts; status[i] KETOGPU_EXPAND_OK /
 * _NIL / _HOST under the same rules, HOST for every request of a snapshot with shared
 * Subject.String() keys; the same following of in-place writes.  Every OK tree equals the host
 * twin's, and the plain call's, word for word.
 *
 * The walk stays ordered, one wave per request, but it looks only at the row entries that can
 * do more than emit a leaf: those that have a row of their own or whose bit is set in the bad-row
 * bitmap.  A bitmap with one bit per word of the handle's rows (free words of the arena included;
 * mask_words 64-bit words) marks them.  It is rebuilt in full, by one kernel across the device,
 * by the first wide call after the rows changed (upload, patched or full refresh); a call behind
 * which nothing changed builds nothing.  In front of each 64-entry step the walk reads up to 64
 * mask words: at least 64 entries without a mark, or all that is left of the row, are a RUN,
 * passed in one step of up to 4096 entries with no access to the visited set.  The writing walk
 * copies a short run itself and appends a longer one to the call's queue as items of up to
 * `chunk` entries (source, destination, length); a fill kernel launched behind the walk, with no
 * host wait in between, copies the items with the whole device.  The queue holds queue_capacity
 * items (KETOGPU_EXPAND_WIDE_QUEUE; the default, 65536 items of 24 bytes, is about ten times
 * what 1024 trees of 16.4 M nodes append); a run that finds it full is copied by its wave
 * (runs_queue_full): slower, never an error.  A count-only call, a truncated tree and a HOST
 * request queue nothing.  A request that opens more than set_capacity nodes runs tier 2 of
 * ketogpu_subjects_expand unchanged, so KETOGPU_SUBJECTS_TIER=2 makes this call the plain one.
 * Wide expand calls count only here: neither ketogpu_expand_stats nor any listing statistic
 * moves, and no plain call is routed here.
 * (Additions within ABI 9: no existing entry point or struct layout changed.) */
typedef struct {
    uint64_t requests;       /* as in ketogpu_expand_stats, for wide expand calls ...       */
    uint64_t tier1_requests;
    uint64_t tier2_requests;
    uint64_t tier2_rounds;
    uint64_t host_requests;
    uint64_t nodes_produced;
    uint64_t truncated_trees;
    uint64_t mask_builds;      /* full rebuilds of the attention bitmap                     */
    uint64_t mask_words;       /* its 64-bit words as last built: 8 bytes each on the device */
    uint64_t run_steps;        /* run steps of all walks, counting and writing              */
    uint64_t skipped_entries;  /* row entries those steps passed                            */
    uint64_t runs_queued;      /* runs of writing walks that went to the queue ...          */
    uint64_t items_queued;     /* ... as this many items                                    */
    uint64_t runs_self_copied; /* runs of writing walks copied by the walking wave: short
                                  ones, and those that met a full queue                     */
    uint64_t runs_queue_full;  /* ... the latter alone                                      */
    uint64_t queue_capacity;   /* items                                                     */
    uint32_t slots;            /* tier 2: requests per round (0 before the first)           */
    uint32_t chunk;            /* row entries per item at most                              */
    double last_call_ms;       /* host wall time of the last wide expand call               */
    double last_mask_ms;       /* ... and of the last rebuild of the bitmap, kernel and wait */
} ketogpu_expand_wide_stats;
int ketogpu_subjects_expand_wide_stats_get(const ketogpu_subjects *h, ketogpu_expand_wide_stats *out);
int ketogpu_subjects_expand_wide(ketogpu_subjects *h, const uint32_t *roots, const uint32_t *rest_depth, size_t n,
                                 uint32_t *out_nodes, uint32_t *out_children, uint64_t capacity, uint64_t *begin,
                                 uint64_t *count, uint32_t *status, uint64_t *needed);

/* ------------------------------------------------------------------- misc */
const char *ketogpu_last_error(void);
int ketogpu_abi_version(void);
void ketogpu_free(void *p);
/* number of visible HIP devices (0 without a GPU) */
int ketogpu_device_count(void);
/* diagnostics (no Keto counterpart): the random-line ceiling of plan label's first stage —
 * `requests` requests of 16 per wave each reading two random 128-byte lines of a
 * `table_bytes` table plus 8 bytes of request, the reads a check of plan label makes and
 * nothing else; *ms_per_launch averaged over `reps` launches on `device` (keto_amd/csrc/
 * probe.hip; bench.py's roofline.line_ceiling) */
int ketogpu_probe_random_lines(int device, uint64_t table_bytes, uint64_t requests, int reps, double *ms_per_launch);
/* the same kernel under the pipelined calls' conditions: `reps` launches round-robin over
 * `streams` (1..8, else KETOGPU_EINVAL) non-blocking streams, timed from an event ahead of
 * the first launch to one behind every stream's last; *ms_per_launch = that time / reps */
int ketogpu_probe_random_lines_streams(int device, uint64_t table_bytes, uint64_t requests, int reps, int streams,
                                       double *ms_per_launch);

#ifdef __cplusplus
}
#endif
#endif

"""Seeded random relation-tuple tables and requests for parity tests.

Rows are raw keto_relation_tuples rows (namespace ids, not names) so tests can
include ids that are not configured (page poisoning, R7).  `collide=True` uses
names containing ':' and '#' so distinct subjects share Subject.String() keys (R4).
"""
import random


def make_graph(seed, n_rows=200, n_obj=12, n_rel=3, n_users=10, wildcard=True, poison=False, collide=False,
               empty_ns=False, n_ns=3):
    rng = random.Random(seed)
    ns_names = [f"n{i}" for i in range(n_ns)]
    if collide:
        ns_names = ["a", "a:b", "c"][:max(n_ns, 2)]
    if empty_ns:
        ns_names[-1] = ""
    namespaces = [(name, i + 1) for i, name in enumerate(ns_names)]
    ids = [i for _, i in namespaces]
    objs = [f"o{i}" for i in range(n_obj)]
    rels = [f"r{i}" for i in range(n_rel)]
    users = [f"u{i}" for i in range(n_users)]
    if collide:
        objs = objs[: n_obj - 3] + ["b:c", "c", "b"]
        rels = rels[: n_rel - 1] + ["c#d"] if n_rel > 1 else rels
        users = users[: n_users - 3] + ["a:b#c", "a:b:c#r0", "a:b#r0"]
    rows = []
    for _ in range(n_rows):
        ns = rng.choice(ids)
        if poison and rng.random() < 0.03:
            ns = 99  # namespace id that is not configured
        o, r = rng.choice(objs), rng.choice(rels)
        if rng.random() < 0.45:
            rows.append((ns, o, r, rng.choice(users), None, None, None))
        else:
            so = rng.choice(objs)
            sr = rng.choice(rels)
            if wildcard and rng.random() < 0.06:
                so = ""
            if wildcard and rng.random() < 0.06:
                sr = ""
            sns = rng.choice(ids)
            if poison and rng.random() < 0.03:
                sns = 98
            rows.append((ns, o, r, None, sns, so, sr))
    return namespaces, rows


def make_family_graph(seed, families=12, chain=35, docs=3, users=300):
    """groups in chains (family f: g{f}_0 member of g{f}_1 ... of g{f}_{chain-1}), a few
    documents per family viewable by members of a chain group, users members of the chain
    bottoms of 1..4 families.  A user reaches 35 to 140 groups, but plan label's 2-hop lists
    over them are much shorter (a chain needs few landmarks).  Measured with seed 92 (Snapshot.label_index): the longest S list has 30
    entries, the longest P list 25, the chosen heads are 32,32 and 5 S lists pass their 28
    inline entries; seed 91: 60 and 18, heads 64,32, nothing past its head.  So this graph
    covers lists within a 32-word head (and the overflow region when 8- or 16-word heads are
    forced); no list reaches the dense pass's 64 prefetched entries or its stage.  Lists past
    those: make_comb_graph.  -> (namespaces, rows, requests)"""
    rng = random.Random(seed)
    rows = []
    for f in range(families):
        for k in range(chain - 1):
            rows.append((1, f"g{f}_{k + 1}", "member", None, 1, f"g{f}_{k}", "member"))
        for d in range(docs):
            rows.append((1, f"d{f}_{d}", "view", None, 1, f"g{f}_{rng.randrange(chain)}", "member"))
    for u in range(users):
        for f in rng.sample(range(families), 1 + u % 4):
            rows.append((1, f"g{f}_0", "member", f"u{u}", None, None, None))
    reqs = []
    for _ in range(4 * users):
        f = rng.randrange(families)
        o, r = (f"d{f}_{rng.randrange(docs)}", "view") if rng.random() < 0.4 else (f"g{f}_{rng.randrange(chain)}",
                                                                                  "member")
        reqs.append(("n", o, r, {"subject_id": f"u{rng.randrange(users)}"}))
    return [("n", 1)], rows, reqs


COMB_LENGTHS = (1, 3, 4, 5, 12, 13, 28, 29, 60, 61, 64, 65, 70, 128, 129, 140, 256, 257, 330)


def make_comb_graph(seed, comps=420, lengths=COMB_LENGTHS, doc_copies=1, leaf_counts=(5, 30, 70, 150, 300)):
    """plan label's lists of chosen lengths, from disjoint components.

    `comps` components g{i} -member-> h{i} (h{i} holds one private user): both interior, no
    edge between components.  A document D (never a subject set: a non-interior root) holds
    the subject sets g{i} for i in a circular range A of chosen length, a user U is a direct
    member of h{i} for i in a circular range B; allowed(D, U) <=> A and B meet, or a direct
    row D <- U exists.  A hub cluster (64 nodes c{x} -member-> z0, z1, all held by the
    document M000) is more central than any comb node, so it takes the 64 mask landmarks and every comb node is a list entry;
    names are zero-padded, so every g ranks before every h, further apart than any batch of
    the label build on up to 16 threads: P(D) = {g{i}: i in A} and S(U)'s landmarks =
    {g{i}, h{i}: i in B}, then S(U)'s raw entries (the documents and leaf objects E{x} that
    hold U directly).  The lengths straddle the inline capacities (4, 12, 28, 60), the device
    build's 64 entries, the dense pass's stages (128, 256) and its 64 prefetched walked
    entries.  The realised lengths depend on the landmark ranking: tests take them from the
    built index (tests/label_census.py), not from here.  -> (namespaces, rows, requests)"""
    rng = random.Random(seed)
    rows = []
    g, h = (lambda i: f"g{i % comps:03d}"), (lambda i: f"h{i % comps:03d}")
    for i in range(comps):
        rows.append((1, g(i), "member", None, 1, h(i), "member"))
        rows.append((1, h(i), "member", f"p{i:03d}", None, None, None))
    for x in range(64):  # the hub cluster: the mask landmarks
        for z in ("z0", "z1"):
            rows.append((1, f"c{x:02d}", "member", None, 1, z, "member"))
        rows.append((1, "M000", "view", None, 1, f"c{x:02d}", "member"))  # (a subject set: c{x} is interior)
    rows.append((1, "z0", "member", "pz0", None, None, None))
    rows.append((1, "z1", "member", "pz1", None, None, None))

    docs, users = [], []  # (name, first component, length)

    def add_doc(a, n):
        docs.append((f"D{len(docs):03d}", a % comps, n))
        for i in range(a, a + n):
            rows.append((1, docs[-1][0], "view", None, 1, g(i), "member"))
        return docs[-1][0]

    def add_user(b, n):
        users.append((f"U{len(users):03d}", b % comps, n))
        for i in range(b, b + n):
            rows.append((1, h(i), "member", users[-1][0], None, None, None))
        return users[-1][0]

    leaves = []

    def add_leaves(u, n):  # u a direct subject of n leaf objects (raw entries of S(u))
        for _ in range(n):
            leaves.append((f"E{len(leaves):03d}", u))
            rows.append((1, leaves[-1][0], "view", u, None, None, None))

    direct = lambda d, u: rows.append((1, d, "view", u, None, None, None))
    # documents: every length, at random places
    for n in lengths:
        for _ in range(doc_copies):
            add_doc(rng.randrange(comps), n)
    # users: S(U) has two landmarks per component and `raw` raw entries, so a list of n
    # entries is n // 2 components and n % 2 leaf objects; then every length again as the
    # number of components (lists of up to 2 x 330 landmarks)
    for n in lengths:
        u = add_user(rng.randrange(comps), n // 2)
        add_leaves(u, n % 2)
    for n in lengths:
        if n <= 140:
            add_user(rng.randrange(comps), n)
    # ranges that meet in exactly one component, at an end of both: the hit is the last
    # entry of one list and the first of the other
    for n, m in ((13, 29), (61, 70), (65, 129), (129, 257), (257, 140), (70, 330), (330, 33), (3, 2), (5, 1), (29, 2)):
        a = rng.randrange(comps)
        add_doc(a, n)
        add_user(a + n - 1, m)
        add_doc(a + n - 1 + m - 1, n)
    # the one-edge test with S the shorter (walked) list and past its head: users next to a
    # long document's range (no common component), held directly by that document
    for k, d in enumerate([d for d in docs if d[2] >= 128][:6]):
        direct(d[0], add_user(d[1] + d[2] + 3, (33, 45, 52)[k % 3]))
    # long raw lists: users held directly by leaf objects, with few or many landmarks
    # before them, and by some documents (the one-edge test decides)
    for k, n in enumerate(leaf_counts):
        u = add_user(rng.randrange(comps), (0, 1, 6, 14, 40)[k % 5])
        add_leaves(u, n)
        for d in rng.sample(docs, 6):
            direct(d[0], u)
    for u in rng.sample(users, 14):  # direct rows behind long landmark lists too
        add_leaves(u[0], rng.choice((1, 2, 3, 7)))
        for d in rng.sample(docs, 5):
            direct(d[0], u[0])
    # mask hits: some documents also hold a hub node, some users are members of z0
    for d in rng.sample(docs, 4):
        rows.append((1, d[0], "view", None, 1, f"c{rng.randrange(64):02d}", "member"))
    for u in rng.sample(users, 4):
        rows.append((1, "z0", "member", u[0], None, None, None))

    sub = lambda u: {"subject_id": u}
    reqs = [("n", d[0], "view", sub(u[0])) for d in docs for u in users]
    holder = dict(leaves)
    for x in range(0, len(leaves), 7):  # one-edge requests: the holder (true) and another user (false)
        reqs.append(("n", leaves[x][0], "view", sub(holder[leaves[x][0]])))
        reqs.append(("n", leaves[x][0], "view", sub(users[(3 * x) % len(users)][0])))
    for i in range(0, comps, 9):  # interior roots
        for u in users[i % 5::11]:
            reqs.append(("n", g(i), "member", sub(u[0])))
    for u in users[::8]:  # an interior root inside the user's range
        reqs.append(("n", g(u[1] + u[2] // 2), "member", sub(u[0])))
    for d in docs[::10]:
        reqs.append(("n", d[0], "view", sub("nobody")))  # users that appear nowhere
    return [("n", 1)], rows, reqs


def make_requests(seed, namespaces, rows, n=300, wildcard=True):
    rng = random.Random(seed + 7)
    names = [n for n, _ in namespaces] + ["unknown"]
    objs = sorted({r[1] for r in rows}) or ["o0"]
    rels = sorted({r[2] for r in rows}) or ["r0"]
    sids = sorted({r[3] for r in rows if r[3] is not None}) or ["u0"]
    sets = sorted({(r[4], r[5], r[6]) for r in rows if r[3] is None})
    id2name = {i: n for n, i in namespaces}
    reqs = []
    for _ in range(n):
        ns, o, r = rng.choice(names), rng.choice(objs), rng.choice(rels)
        if wildcard and rng.random() < 0.05:
            o = ""
        if wildcard and rng.random() < 0.05:
            r = ""
        if wildcard and rng.random() < 0.03:
            ns = ""
        if sets and rng.random() < 0.3:
            sns, so, sr = rng.choice(sets)
            subj = {"subject_set": {"namespace": id2name.get(sns, "unknown"), "object": so, "relation": sr}}
        elif rng.random() < 0.05:
            subj = {"subject_id": "nobody"}
        else:
            subj = {"subject_id": rng.choice(sids)}
        reqs.append((ns, o, r, subj))
    return reqs


def oracle_store_columns(namespaces, cols, page_size=100, presorted=True):
    from oracle import oracle as O
    st = O.Store(namespaces, page_size)
    st.add_columnar(cols)
    return st.finalize(presorted=presorted)


def oracle_store(namespaces, rows, page_size=100, order="sqlite"):
    from oracle import oracle as O
    st = O.Store(namespaces, page_size, order=order)
    for (ns, o, r, sid, sns, so, sr) in rows:
        if sid is not None:
            st.add_row(ns, o, r, subject_id=sid)
        else:
            st.add_row(ns, o, r, ss_ns_id=sns, ss_obj=so, ss_rel=sr)
    return st.finalize()


def backend_sorted(rows, order="sqlite"):
    """rows as the backend returns them for the reference's ORDER BY (relationtuples.go:215),
    bytewise strings; NULLs first (sqlite) or last (postgres).  Stable: equal rows keep
    their insertion (commit_time) order."""
    def key(r):
        ns, o, rel, sid, sns, so, sr = r
        null_sid = sid is None
        first = null_sid if order == "postgres" else not null_sid  # False sorts first
        return (ns, o.encode(), rel.encode(), first, (sid or "").encode(), sns or 0, (so or "").encode(),
                (sr or "").encode())
    return sorted(rows, key=key)

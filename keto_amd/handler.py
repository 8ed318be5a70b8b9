"""Check / expand request handling over the MI355X engines, and the batch-check endpoint.

Mirrors the reference's REST handlers (status mapping and request parsing), which stay
unchanged in a Go deployment — here they are the harness that shows a
caller gets the reference's responses from the new engines:

    GET  /check    internal/check/handler.go:85-107   200 {"allowed":true} | 403 {"allowed":false} | 400
    POST /check    internal/check/handler.go:128-146  same; a JSON decode error is 400
    GET  /expand   internal/expand/handler.go:78-92   200 tree | null, 400 bad max-depth, 404 unknown namespace
    POST /expand/batch   (no Keto counterpart) a list of {subject, max-depth} -> per item what GET /expand answers
    POST /check/batch  (new)    200 {"results": [{"allowed": bool} | {"error": ...}]}
    GET  /list/objects   (new, DESIGN.md "Sorted, paged lists")  200 {"objects": [...], "next_page_token", "total"}
    GET  /list/subjects  (new, same section)                     200 {"subjects": [...], "next_page_token", "total"}
         both take max-depth (Keto's spelling; DESIGN.md "Depth-limited listings"): a positive integer, else 400;
         the list within that many hops, and the body gains "complete": true | false
         both take via=true (DESIGN.md "Grant trees"; any other value is 400): every entry becomes
         {"object" | "subject": ..., "via": the granting subject, "hops": n}
         both take wide=true (DESIGN.md "Chip-wide pages and depths"; any other value is 400, and so is
         wide=true together with via=true): the same body, the large closures run in the wide tier
    GET  /list/objects/combined, /list/subjects/combined  (new, DESIGN.md "Combined listings")  the same bodies for
         the list of two subjects / two objects under op = and | andnot | or
    GET  /check/explain  (new, DESIGN.md "Explain")  200 {"allowed":true,"path":[...]} | 403 {"allowed":false,"path":[]}

URL parsing restates RelationQuery.FromURLQuery (internal/relationtuple/definitions.go:
458-493): a bare "subject" key, both subject forms, or an incomplete subject_set are 400;
missing namespace/object/relation are "" (no filter, R5).  Deliberate divergence: the
reference's postCheck writes its 400 for a bad body and then goes on to evaluate a zero
tuple (handler.go:130-132); here the 400 is the whole response.

The batch endpoint takes many tuples in one request and answers them through the engine's
throughput path (check.Engine.check_batch: ketogpu_resolve_batch, then ONE
ketogpu_check_ids — chunked H2D overlapped with the traversal, one D2H — with only
wildcard-root and R4-flagged requests re-answered sequentially), per-tuple errors inline.
`python -m keto_amd.handler --port P --tuples FILE --namespaces a:1,b:2` serves these
routes with http.server (a demo harness; the production server is Keto's own).
"""
import json
from urllib.parse import parse_qs

from . import _lib, check, expand
from .relationtuple import InternalRelationTuple, NilSubject, SubjectID, SubjectSet

SUBJECT_ID = "subject_id"
SS_KEYS = ("subject_set.namespace", "subject_set.object", "subject_set.relation")


class BadRequest(ValueError):
    """herodot.ErrBadRequest (HTTP 400)"""


def _get(q, k):
    v = q.get(k)
    if v is None:
        return None
    return v[0] if isinstance(v, (list, tuple)) else v


def relation_query_from_url(q):
    """RelationQuery.FromURLQuery (definitions.go:458-493) -> (namespace, object, relation, subject|None)"""
    if "subject" in q:
        raise BadRequest('provide "subject_id" or "subject_set.*"; support for "subject" was dropped')
    has_id = SUBJECT_ID in q
    has_ss = [k in q for k in SS_KEYS]
    subject = None
    if not has_id and not any(has_ss):
        pass
    elif has_id and all(has_ss):
        raise BadRequest("exactly one of subject_set or subject_id has to be provided")
    elif has_id:
        subject = SubjectID(_get(q, SUBJECT_ID))
    elif all(has_ss):
        subject = SubjectSet(*(_get(q, k) for k in SS_KEYS))
    else:
        raise BadRequest('incomplete subject, provide "subject_id" or a complete "subject_set.*"')
    return _get(q, "namespace") or "", _get(q, "object") or "", _get(q, "relation") or "", subject


def tuple_from_url(q):
    """InternalRelationTuple.FromURLQuery (definitions.go:378-395): the subject is required"""
    ns, obj, rel, subject = relation_query_from_url(q)
    if subject is None:
        raise BadRequest("Subject has to be specified.")
    return InternalRelationTuple(ns, obj, rel, subject)


def _json_string(d, k):
    """a string field of the JSON tuple: Go's decoder turns null into "" and rejects any
    other non-string value (json.UnmarshalTypeError -> 400)"""
    v = d.get(k)
    if v is None:
        return ""
    if not isinstance(v, str):
        raise BadRequest(f"json: cannot unmarshal {type(v).__name__} into field {k} of type string")
    return v


def tuple_from_json(d):
    """JSON body of POST /check: {namespace, object, relation, subject_id | subject_set}"""
    if not isinstance(d, dict):
        raise BadRequest("Unable to decode JSON payload: expected an object")
    # the reference decodes into *string / *SubjectSet (definitions.go:316-325): a key
    # holding null is the same as an absent key
    if d.get("subject_id") is not None and d.get("subject_set") is not None:
        raise BadRequest("exactly one of subject_set or subject_id has to be provided")
    ns, obj, rel = (_json_string(d, k) for k in ("namespace", "object", "relation"))
    subject = None
    if d.get("subject_id") is not None:
        subject = SubjectID(_json_string(d, "subject_id"))
    elif d.get("subject_set") is not None:
        ss = d["subject_set"]
        if not isinstance(ss, dict):
            raise BadRequest(f"json: cannot unmarshal {type(ss).__name__} into field subject_set of type object")
        subject = SubjectSet(*(_json_string(ss, k) for k in ("namespace", "object", "relation")))
    return InternalRelationTuple(ns, obj, rel, subject)


def _underscore_ok(s):
    """Go's strconv underscoreOK: '_' only between digits or after a base prefix"""
    saw, i = "^", 0
    if s[:1] in ("-", "+"):
        s = s[1:]
    hexa = False
    if len(s) >= 2 and s[0] == "0" and s[1].lower() in "box":
        i, saw, hexa = 2, "0", s[1].lower() == "x"
    while i < len(s):
        c = s[i]
        if c.isdigit() and c.isascii() or hexa and c.lower() in "abcdef":
            saw = "0"
        elif c == "_":
            if saw != "0":
                return False
            saw = "_"
        else:
            if saw == "_":
                return False
            saw = "!"
        i += 1
    return saw != "_"


def go_parse_int(s):
    """strconv.ParseInt(s, 0, 64), as getExpand parses max-depth (internal/expand/handler.go:79):
    an optional sign, then 0b/0o/0x prefixes or a leading 0 for octal, '_' digit
    separators, no whitespace; ValueError on bad syntax or a value outside int64"""
    if not isinstance(s, str) or not s:
        raise ValueError("invalid syntax")
    neg = s[0] == "-"
    body = s[1:] if s[0] in "+-" else s
    if not body:
        raise ValueError("invalid syntax")
    base, digits = 10, body
    if body[0] == "0":
        p = body[1:2].lower()
        if len(body) >= 3 and p in ("b", "o", "x"):
            base, digits = {"b": 2, "o": 8, "x": 16}[p], body[2:]
        else:
            base, digits = 8, body[1:]
    n, underscores = 0, False
    for c in digits:
        if c == "_":
            underscores = True
            continue
        d = int(c, 16) if c.isascii() and c.lower() in "0123456789abcdef" else 99
        if d >= base:
            raise ValueError("invalid syntax")
        n = n * base + d
    if underscores and not _underscore_ok(s):
        raise ValueError("invalid syntax")
    if (not neg and n >= 1 << 63) or (neg and n > 1 << 63):
        raise ValueError("value out of range")
    return -n if neg else n


class Handler:
    """(status, JSON body) for each route; engines are check.Engine and expand.Engine.  `lookup`
    and `subjects` are any objects with list_objects_page / list_subjects_page (lookup.Lookup /
    lookup.Subjects on the device, lookup.HostLookup / lookup.HostSubjects without one); without
    them the list routes answer 404.  `lookup` also serves /check/explain through its Explain."""

    def __init__(self, check_engine: check.Engine, expand_engine: expand.Engine, lookup=None, subjects=None,
                 expand_batch=None):
        self.check = check_engine
        self.expand = expand_engine
        self.expand_batch = expand_batch  # an expand.DeviceEngine (None: /expand/batch walks on the host)
        self.lookup = lookup
        self.subjects = subjects

    @staticmethod
    def _error(code, reason):
        status = {400: "Bad Request", 404: "Not Found", 500: "Internal Server Error"}[code]
        return code, {"error": {"code": code, "status": status, "reason": reason}}

    def _allowed(self, t):
        try:
            ok = self.check.SubjectIsAllowed(t)
        except NilSubject:
            return self._error(400, "Subject has to be specified.")
        return (200, {"allowed": True}) if ok else (403, {"allowed": False})

    def get_check(self, query):
        q = parse_qs(query, keep_blank_values=True) if isinstance(query, str) else query
        try:
            t = tuple_from_url(q)
        except BadRequest as e:
            return self._error(400, str(e))
        return self._allowed(t)

    def post_check(self, body):
        try:
            t = tuple_from_json(json.loads(body))
        except (ValueError, BadRequest) as e:
            return self._error(400, f"Unable to decode JSON payload: {e}")
        return self._allowed(t)

    def get_expand(self, query):
        q = parse_qs(query, keep_blank_values=True) if isinstance(query, str) else query
        raw = _get(q, "max-depth")
        try:
            depth = go_parse_int(raw)  # strconv.ParseInt(s, 0, 0)
        except ValueError as e:
            # Go's Query().Get gives "" for a missing key; strconv quotes with escapes
            return self._error(400, f"strconv.ParseInt: parsing {json.dumps(raw or '')}: {e}")
        # ketogpu_expand takes an int32: every depth beyond any tree's height acts the same
        depth = max(-1, min(depth, 2**31 - 1))
        subject = SubjectSet(_get(q, "namespace") or "", _get(q, "object") or "", _get(q, "relation") or "")
        try:
            tree = self.expand.BuildTree(subject, depth)
        except expand.NotFound as e:
            return self._error(404, str(e))
        return 200, (tree.to_node() if tree else None)

    def post_expand_batch(self, body):
        """[{"subject_set": {...} | "subject_id": "...", "max-depth": n}, ...] -> a list with,
        per item, what GET /expand answers: the tree, null, or the error body (404 unknown
        namespace, 400 bad max-depth or subject).  max-depth is a JSON integer or a string as
        the query parameter takes it.  One batch of the expand engine serves the trees: on the
        device where self.expand_batch is an expand.DeviceEngine, else the host's id walk.  The
        form {"items": [...], "wide": true} asks the device engine for its chip-wide call."""
        wide = False
        try:
            items = json.loads(body)
            if isinstance(items, dict):
                wide = items.get("wide", False)
                if not isinstance(wide, bool):
                    raise BadRequest("expected a boolean for wide")
                items = items["items"]
            if not isinstance(items, list):
                raise BadRequest("expected a list of {subject, max-depth}")
        except (ValueError, KeyError, TypeError, BadRequest) as e:
            return self._error(400, f"Unable to decode JSON payload: {e}")
        results = [None] * len(items)
        subjects, depths, where = [], [], []
        for i, it in enumerate(items):
            try:
                if not isinstance(it, dict):
                    raise BadRequest("expected an object")
                raw = it.get("max-depth")
                try:
                    depth = raw if isinstance(raw, int) and not isinstance(raw, bool) else go_parse_int(raw)
                except ValueError as e:
                    raise BadRequest(f"strconv.ParseInt: parsing {json.dumps(raw if isinstance(raw, str) else '')}: {e}")
                d = it.get("subject") if isinstance(it.get("subject"), dict) else it
                if d.get("subject_id") is not None and d.get("subject_set") is not None:
                    raise BadRequest("exactly one of subject_set or subject_id has to be provided")
                if d.get("subject_id") is not None:
                    subject = SubjectID(_json_string(d, "subject_id"))
                else:
                    ss = d.get("subject_set", d)
                    if not isinstance(ss, dict):
                        raise BadRequest(f"json: cannot unmarshal {type(ss).__name__} into field subject_set of type object")
                    subject = SubjectSet(*(_json_string(ss, k) if ss.get(k) is not None else ""
                                           for k in ("namespace", "object", "relation")))
            except BadRequest as e:
                results[i] = self._error(400, str(e))[1]
                continue
            subjects.append(subject), depths.append(max(-1, min(depth, 2**31 - 1))), where.append(i)
        engine = self.expand_batch if self.expand_batch is not None else self.expand
        # (wide: the device engine's chip-wide call; the host engine takes and ignores it)
        trees = engine.build_trees_batch(subjects, depths, wide=True) if wide else \
            engine.build_trees_batch(subjects, depths)
        for i, t in zip(where, trees):
            results[i] = self._error(404, str(t))[1] if isinstance(t, expand.NotFound) else (t.to_node() if t else None)
        return 200, results

    def post_check_batch(self, body):
        """{"tuples": [...]} -> {"results": [...]}, one engine call for the whole batch"""
        try:
            d = json.loads(body)
            items = d["tuples"] if isinstance(d, dict) else d
            if not isinstance(items, list):
                raise BadRequest("expected a list of relation tuples")
        except (ValueError, KeyError, TypeError, BadRequest) as e:
            return self._error(400, f"Unable to decode JSON payload: {e}")
        results = [None] * len(items)
        tuples, where = [], []
        for i, it in enumerate(items):
            try:
                t = tuple_from_json(it)
                if t.subject is None:
                    raise BadRequest("Subject has to be specified.")
                tuples.append(t)
                where.append(i)
            except (BadRequest, ValueError, AttributeError) as e:
                results[i] = {"error": {"code": 400, "reason": str(e)}}
        batch = (getattr(self.check, "check_batch", None) or self.check.check_many) if tuples else None
        for i, ok in zip(where, batch(tuples) if tuples else []):
            results[i] = {"allowed": bool(ok)}
        return 200, {"results": results}


    # ---- paged lists (page_size / page_token in, next_page_token out: Keto's list convention,
    # internal/x/pagination.go; the order is by node id)
    def _page_args(self, q):
        """-> (page_size, page_token); page_size defaults to 100 and is parsed as Go parses an int"""
        raw = _get(q, "page_size")
        size = 100
        if raw is not None and raw != "":
            try:
                size = go_parse_int(raw)
            except ValueError as e:
                raise BadRequest(f"strconv.ParseInt: parsing {json.dumps(raw)}: {e}")
        if not 1 <= size <= _lib.PAGE_LIMIT_MAX:
            raise BadRequest(f"page_size {size} is outside [1, {_lib.PAGE_LIMIT_MAX}]")
        return size, _get(q, "page_token") or ""

    @staticmethod
    def _max_depth(q):
        """max-depth -> None when the parameter is absent, else a positive integer that fits the
        library's uint32 (parsed as Go parses an int); anything else is a BadRequest"""
        if "max-depth" not in q:
            return None
        raw = _get(q, "max-depth")
        try:
            depth = go_parse_int(raw)
        except ValueError as e:
            raise BadRequest(f"strconv.ParseInt: parsing {json.dumps(raw or '')}: {e}")
        if depth < 1:
            raise BadRequest(f"max-depth {depth} is not a positive integer")
        return min(depth, 0xFFFFFFFF)  # (every depth beyond any closure's acts the same)

    @staticmethod
    def _via(q):
        """via -> False when the parameter is absent, True for "true"; anything else is a
        BadRequest"""
        if "via" not in q:
            return False
        raw = _get(q, "via")
        if raw != "true":
            raise BadRequest(f'via {json.dumps(raw or "")}: expected "true"')
        return True

    @staticmethod
    def _wide(q, why):
        """wide -> {} when the parameter is absent, {"wide": True} for "true" (the keyword of the
        list calls); anything else, and wide=true together with via=true, is a BadRequest"""
        if "wide" not in q:
            return {}
        raw = _get(q, "wide")
        if raw != "true":
            raise BadRequest(f'wide {json.dumps(raw or "")}: expected "true"')
        if why:
            raise BadRequest("wide=true cannot be combined with via=true")
        return {"wide": True}

    def _list(self, backend, query, call):
        if backend is None:
            return self._error(404, "this server has no list handle")
        q = parse_qs(query, keep_blank_values=True) if isinstance(query, str) else query
        try:
            size, token = self._page_args(q)
            return 200, call(q, size, token)
        except BadRequest as e:
            return self._error(400, str(e))
        except _lib.KetoError as e:  # a malformed token, a wildcard root without a node
            if e.code != _lib.EINVAL:
                raise
            return self._error(400, str(e))

    def get_list_objects(self, query):
        """namespace, relation, subject_id | subject_set.*, page_size, page_token -> the objects o
        with Check(namespace:o#relation@subject); with max-depth, those within that many hops
        of the subject, and "complete"; with via=true every entry is {"object", "via", "hops"};
        wide=true (not with via=true) runs the large closures in the wide tier """
        def call(q, size, token):
            depth = self._max_depth(q)
            why = self._via(q)
            wide = self._wide(q, why)
            t = tuple_from_url(q)  # the subject is required
            if why:
                res = self.lookup.list_objects_page(t.namespace, t.relation, t.subject, size, token, max_depth=depth,
                                                    with_via=True)
                body = {"objects": [{"object": o, "via": v.to_dict(), "hops": h} for o, v, h in res[0]],
                        "next_page_token": res[1], "total": res[2]}
                if depth is not None:
                    body["complete"] = bool(res[3])
                return body
            if depth is not None:
                items, nxt, total, complete = self.lookup.list_objects_page(t.namespace, t.relation, t.subject, size,
                                                                            token, max_depth=depth, **wide)
                return {"objects": items, "next_page_token": nxt, "total": total, "complete": bool(complete)}
            items, nxt, total = self.lookup.list_objects_page(t.namespace, t.relation, t.subject, size, token, **wide)
            return {"objects": items, "next_page_token": nxt, "total": total}
        return self._list(self.lookup, query, call)

    def get_list_subjects(self, query):
        """namespace, object, relation, kind (ids | any | ns#relation), page_size, page_token -> the
        subjects s with Check(namespace:object#relation@s), in the JSON form check requests use;
        with max-depth, those within that many hops of the object, and "complete"; with via=true
        every entry is {"subject", "via", "hops"}; wide=true (not with via=true) runs the large
        closures in the wide tier """
        def call(q, size, token):
            depth = self._max_depth(q)
            why = self._via(q)
            wide = self._wide(q, why)
            kind = _get(q, "kind") or "ids"
            if kind not in ("ids", "any"):
                ns, sep, rel = kind.partition("#")
                if not sep:
                    raise BadRequest(f'kind {kind!r}: expected "ids", "any" or "namespace#relation"')
                kind = (ns, rel)
            root = (_get(q, "namespace") or "", _get(q, "object") or "", _get(q, "relation") or "")
            if why:
                res = self.subjects.list_subjects_page(*root, kind, size, token, max_depth=depth, with_via=True)
                body = {"subjects": [{"subject": s.to_dict(), "via": v.to_dict(), "hops": h} for s, v, h in res[0]],
                        "next_page_token": res[1], "total": res[2]}
                if depth is not None:
                    body["complete"] = bool(res[3])
                return body
            if depth is not None:
                items, nxt, total, complete = self.subjects.list_subjects_page(*root, kind, size, token,
                                                                               max_depth=depth, **wide)
                return {"subjects": [s.to_dict() for s in items], "next_page_token": nxt, "total": total,
                        "complete": bool(complete)}
            items, nxt, total = self.subjects.list_subjects_page(*root, kind, size, token, **wide)
            return {"subjects": [s.to_dict() for s in items], "next_page_token": nxt, "total": total}
        return self._list(self.subjects, query, call)

    # ---- combined lists (DESIGN.md "Combined listings"): the two routes above with an operator
    # and a second side; bodies, paging and the 400 / 404 rules are theirs
    @staticmethod
    def _op(q):
        op = _get(q, "op")
        if op not in ("and", "andnot", "or"):
            raise BadRequest(f'op {op!r}: expected "and", "andnot" or "or"')
        return op

    def get_list_objects_combined(self, query):
        """the query of /list/objects plus op (and | andnot | or) and a second subject,
        other_subject_id | other_subject_set.namespace|object|relation -> the objects o with
        Check(o@subject) op Check(o@other subject)"""
        def call(q, size, token):
            t = tuple_from_url(q)  # the subject is required
            op = self._op(q)
            has_id = "other_" + SUBJECT_ID in q
            has_ss = ["other_" + k in q for k in SS_KEYS]
            if has_id and any(has_ss):
                raise BadRequest("exactly one of other_subject_set or other_subject_id has to be provided")
            if has_id:
                other = SubjectID(_get(q, "other_" + SUBJECT_ID))
            elif all(has_ss):
                other = SubjectSet(*(_get(q, "other_" + k) for k in SS_KEYS))
            else:
                raise BadRequest('the second subject has to be specified: "other_subject_id" or a complete '
                                 '"other_subject_set.*"')
            items, nxt, total = self.lookup.list_objects_combined_page(t.namespace, t.relation, t.subject, other, op,
                                                                       size, token)
            return {"objects": items, "next_page_token": nxt, "total": total}
        return self._list(self.lookup, query, call)

    def get_list_subjects_combined(self, query):
        """the query of /list/subjects plus op (and | andnot | or) and a second object,
        other_namespace, other_object, other_relation -> the subjects s with
        Check(object@s) op Check(other object@s)"""
        def call(q, size, token):
            kind = _get(q, "kind") or "ids"
            if kind not in ("ids", "any"):
                ns, sep, rel = kind.partition("#")
                if not sep:
                    raise BadRequest(f'kind {kind!r}: expected "ids", "any" or "namespace#relation"')
                kind = (ns, rel)
            op = self._op(q)
            other = [_get(q, k) for k in ("other_namespace", "other_object", "other_relation")]
            if any(v is None for v in other):
                raise BadRequest('the second object has to be specified: "other_namespace", "other_object" and '
                                 '"other_relation"')
            root = (_get(q, "namespace") or "", _get(q, "object") or "", _get(q, "relation") or "")
            items, nxt, total = self.subjects.list_subjects_combined_page(root, tuple(other), op, kind, size, token)
            return {"subjects": [s.to_dict() for s in items], "next_page_token": nxt, "total": total}
        return self._list(self.subjects, query, call)

    # ---- why a check is allowed (DESIGN.md "Explain")
    def get_check_explain(self, query):
        """the query of GET /check -> 200 {"allowed": true, "path": [...]} with one shortest chain
        of subjects from namespace:object#relation to the subject (each held by the one before
        it), 403 {"allowed": false, "path": []}"""
        if self.lookup is None:
            return self._error(404, "this server has no lookup handle")
        q = parse_qs(query, keep_blank_values=True) if isinstance(query, str) else query
        try:
            t = tuple_from_url(q)
            path = self.lookup.Explain(t.namespace, t.object, t.relation, t.subject)
        except BadRequest as e:
            return self._error(400, str(e))
        except _lib.KetoError as e:  # a wildcard root without a node
            if e.code != _lib.EINVAL:
                raise
            return self._error(400, str(e))
        body = {"allowed": bool(path), "path": [s.to_dict() for s in path]}
        return (200 if path else 403), body


def serve(handler: Handler, port: int):  # pragma: no cover - demo harness
    from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer
    from urllib.parse import urlsplit

    class H(BaseHTTPRequestHandler):
        def _send(self, code, body):
            data = json.dumps(body).encode()
            self.send_response(code)
            self.send_header("Content-Type", "application/json")
            self.send_header("Content-Length", str(len(data)))
            self.end_headers()
            self.wfile.write(data)

        def do_GET(self):
            u = urlsplit(self.path)
            if u.path == "/check":
                self._send(*handler.get_check(u.query))
            elif u.path == "/check/explain":
                self._send(*handler.get_check_explain(u.query))
            elif u.path == "/expand":
                self._send(*handler.get_expand(u.query))
            elif u.path == "/list/objects":
                self._send(*handler.get_list_objects(u.query))
            elif u.path == "/list/subjects":
                self._send(*handler.get_list_subjects(u.query))
            elif u.path == "/list/objects/combined":
                self._send(*handler.get_list_objects_combined(u.query))
            elif u.path == "/list/subjects/combined":
                self._send(*handler.get_list_subjects_combined(u.query))
            else:
                self._send(404, {"error": {"code": 404, "status": "Not Found"}})

        def do_POST(self):
            body = self.rfile.read(int(self.headers.get("Content-Length", 0) or 0))
            path = urlsplit(self.path).path
            if path == "/check":
                self._send(*handler.post_check(body))
            elif path == "/check/batch":
                self._send(*handler.post_check_batch(body))
            elif path == "/expand/batch":
                self._send(*handler.post_expand_batch(body))
            else:
                self._send(404, {"error": {"code": 404, "status": "Not Found"}})

    ThreadingHTTPServer(("127.0.0.1", port), H).serve_forever()


def main():  # pragma: no cover - demo harness
    import argparse

    from .snapshot import Snapshot
    p = argparse.ArgumentParser()
    p.add_argument("--port", type=int, default=4466)
    p.add_argument("--tuples", required=True, help="file with one relation tuple string per line")
    p.add_argument("--namespaces", required=True, help="name:id,name:id")
    a = p.parse_args()
    ns = [(x.split(":")[0], int(x.split(":")[1])) for x in a.namespaces.split(",")]
    tuples = [InternalRelationTuple.FromString(line.strip()) for line in open(a.tuples) if line.strip()]
    snap = Snapshot.from_tuples(ns, tuples)
    from . import lookup
    try:
        lists = (lookup.Lookup(snap), lookup.Subjects(snap))
    except _lib.KetoError as e:  # shared Subject.String() keys (R4): the list routes answer 404
        print(f"no list routes: {e}")
        lists = (None, None)
    device = expand.DeviceEngine(snap, subjects=lists[1]) if lists[1] is not None else None
    serve(Handler(check.Engine(snap), expand.Engine(snap), *lists, expand_batch=device), a.port)


if __name__ == "__main__":
    main()

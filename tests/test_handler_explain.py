"""GET /check/explain of the REST handler mirror (keto_amd/handler.py get_check_explain) over
the CPU twin of the path call; no GPU."""
from urllib.parse import urlencode

import pytest

from keto_amd import lookup
from keto_amd.handler import Handler
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC


@pytest.fixture(scope="module")
def handler():
    return Handler(None, None, lookup=lookup.HostLookup(Snapshot.from_rows(LC.NS1, LC.structure_rows())))


def sset(obj, rel):
    return {"subject_set": {"namespace": "n", "object": obj, "relation": rel}}


def test_allowed_is_200_with_the_path(handler):
    code, body = handler.get_check_explain("namespace=n&object=top&relation=view&subject_id=ux")
    assert code == 200 and set(body) == {"allowed", "path"} and body["allowed"] is True
    path = body["path"]
    assert len(path) == 4 and path[0] == sset("top", "view") and path[2] == sset("g0", "member")
    assert path[1] in (sset("g1", "member"), sset("g2", "member")) and path[3] == {"subject_id": "ux"}
    # a subject set as the subject, as in /check
    code, body = handler.get_check_explain(urlencode({
        "namespace": "n", "object": "ya", "relation": "member", "subject_set.namespace": "n",
        "subject_set.object": "ya", "subject_set.relation": "member"}))
    assert code == 200 and body == {"allowed": True, "path": [sset("ya", "member"), sset("yb", "member"),
                                                              sset("ya", "member")]}
    code, body = handler.get_check_explain("namespace=n&object=c99&relation=member&subject_id=uc")
    assert code == 200 and len(body["path"]) == 101 and body["path"][-2] == sset("c0", "member")


def test_denied_is_403_with_an_empty_path(handler):
    for query in ("namespace=n&object=top&relation=view&subject_id=uc",  # another part of the graph
                  "namespace=n&object=top&relation=view&subject_id=nobody",
                  "namespace=nowhere&object=top&relation=view&subject_id=ux",
                  "namespace=n&object=no+such+doc&relation=view&subject_id=ux"):
        assert handler.get_check_explain(query) == (403, {"allowed": False, "path": []}), query


def test_bad_requests_are_400_where_check_has_them(handler):
    plain = Handler(None, None)
    for query in ("", "namespace=n&object=top&relation=view",  # a missing subject
                  "subject=not%23a+valid+userset+rewrite", "namespace=n&subject_set.namespace=n",
                  "namespace=n&object=top&relation=view&subject_id=ux&subject_set.namespace=n"
                  "&subject_set.object=g0&subject_set.relation=member"):
        code, body = handler.get_check_explain(query)
        assert code == 400 and body["error"]["code"] == 400 and body["error"]["status"] == "Bad Request", query
        assert (code, body) == plain.get_check(query), query  # the same answer /check gives


def test_wildcard_root_without_a_node_is_400():
    _, rows, snap = LC.table(*LC.TABLES[1])
    obj, rel = rows[0][1], rows[0][2]
    h = Handler(None, None, lookup=lookup.HostLookup(snap))
    code, body = h.get_check_explain(urlencode({"namespace": "", "object": obj, "relation": rel, "subject_id": "u1"}))
    assert code == 400 and "wildcard" in body["error"]["reason"]


def test_no_lookup_backend_is_404():
    for h in (Handler(None, None), Handler(None, None, subjects=object())):
        code, body = h.get_check_explain("namespace=n&object=top&relation=view&subject_id=ux")
        assert code == 404 and body["error"]["code"] == 404 and body["error"]["status"] == "Not Found"

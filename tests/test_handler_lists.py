"""The list routes of the REST handler mirror (keto_amd/handler.py get_list_objects /
get_list_subjects) over the CPU twins of the paged calls; no GPU."""
from urllib.parse import urlencode

import pytest

from keto_amd import expand, lookup
from keto_amd import relationtuple as rt
from keto_amd.handler import Handler
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import subjects_cases as SC


@pytest.fixture(scope="module")
def snap():
    return Snapshot.from_rows(LC.NS1, SC.structure_rows())


@pytest.fixture(scope="module")
def handler(snap):
    return Handler(None, expand.Engine(snap), lookup.HostLookup(snap), lookup.HostSubjects(snap))


def chain(route, **query):
    """follow next_page_token to the end -> the list of 200 bodies"""
    bodies, token = [], ""
    while True:
        code, body = route(urlencode({**query, "page_token": token}))
        assert code == 200, body
        bodies.append(body)
        token = body["next_page_token"]
        if token == "":
            return bodies
        assert len(bodies) < 100


def test_list_objects_route(handler, snap):
    want = lookup.host_list_objects(snap, "n", "view", rt.SubjectID("u129"))
    assert len(want) == 129
    bodies = chain(handler.get_list_objects, namespace="n", relation="view", subject_id="u129", page_size="50")
    assert [len(b["objects"]) for b in bodies] == [50, 50, 29]
    assert all(set(b) == {"objects", "next_page_token", "total"} and b["total"] == 129 for b in bodies)
    assert sorted(o for b in bodies for o in b["objects"]) == want
    twin = lookup.HostLookup(snap).list_objects_page("n", "view", rt.SubjectID("u129"), 50)
    assert bodies[0] == {"objects": twin[0], "next_page_token": twin[1], "total": twin[2]}
    # the default page size is 100; a subject set is a subject as in /check
    code, body = handler.get_list_objects("namespace=n&relation=view&subject_id=u129")
    assert code == 200 and len(body["objects"]) == 100 and body["next_page_token"] != ""
    code, body = handler.get_list_objects("namespace=n&relation=view&subject_set.namespace=n&subject_set.object=g1"
                                          "&subject_set.relation=member")
    assert code == 200 and body == {"objects": ["top"], "next_page_token": "", "total": 1}
    # Go's base-0 integers: 0x10 is 16
    code, body = handler.get_list_objects("namespace=n&relation=view&subject_id=u129&page_size=0x10")
    assert code == 200 and len(body["objects"]) == 16
    # nothing to list is 200 with an empty page
    for query in ("namespace=nowhere&relation=view&subject_id=u129", "namespace=n&relation=view&subject_id=nobody"):
        assert handler.get_list_objects(query) == (200, {"objects": [], "next_page_token": "", "total": 0})


def test_list_subjects_route(handler, snap):
    want = lookup.host_list_subjects(snap, "n", "f129", "view")
    bodies = chain(handler.get_list_subjects, namespace="n", object="f129", relation="view", page_size="64")
    assert [len(b["subjects"]) for b in bodies] == [64, 64, 1]
    assert all(set(b) == {"subjects", "next_page_token", "total"} and b["total"] == 129 for b in bodies)
    got = [s for b in bodies for s in b["subjects"]]
    assert sorted(got, key=lambda s: s["subject_id"]) == [s.to_dict() for s in want]
    # kinds: subject ids by default, every class, the subject sets of one type
    q = "namespace=n&object=two&relation=view"
    assert handler.get_list_subjects(q)[1]["total"] == 40
    code, body = handler.get_list_subjects(q + "&kind=any")
    assert code == 200 and body["total"] == 42
    code, body = handler.get_list_subjects(q + "&kind=n%23member")
    assert code == 200 and body["total"] == 2
    assert sorted(s["subject_set"]["object"] for s in body["subjects"]) == ["two_ga", "two_gb"]
    assert all(s["subject_set"] == {"namespace": "n", "object": s["subject_set"]["object"], "relation": "member"}
               for s in body["subjects"])
    assert handler.get_list_subjects(q + "&kind=n%23nothing")[1] == {"subjects": [], "next_page_token": "",
                                                                     "total": 0}
    assert handler.get_list_subjects("namespace=n&object=no+such+doc&relation=view") == (
        200, {"subjects": [], "next_page_token": "", "total": 0})


def test_bad_requests(handler):
    lo, ls = handler.get_list_objects, handler.get_list_subjects
    code, body = lo("namespace=n&relation=view")  # a missing subject
    assert code == 400 and "Subject has to be specified" in body["error"]["reason"]
    assert lo("namespace=n&relation=view&subject=u129")[0] == 400
    assert lo("namespace=n&relation=view&subject_set.namespace=n")[0] == 400  # an incomplete subject set
    for size in ("x", "1.5", " 5", "08", "0", "-1", "65537", "99999999999999999999"):
        for code, body in (lo(urlencode({"namespace": "n", "relation": "view", "subject_id": "u129",
                                         "page_size": size})),
                           ls(urlencode({"namespace": "n", "object": "f65", "relation": "view", "page_size": size}))):
            assert code == 400 and body["error"]["code"] == 400 and body["error"]["status"] == "Bad Request", size
    assert lo("namespace=n&relation=view&subject_id=u129&page_size=65536")[0] == 200
    for token in ("x", "-1", "4294967296", " 5"):
        assert lo(urlencode({"namespace": "n", "relation": "view", "subject_id": "u129",
                             "page_token": token}))[0] == 400
        assert ls(urlencode({"namespace": "n", "object": "f65", "relation": "view", "page_token": token}))[0] == 400
    assert ls("namespace=n&object=f65&relation=view&kind=users")[0] == 400


def test_wildcard_root_without_a_node_is_400():
    _, rows, snap = LC.table(*LC.TABLES[1])
    obj, rel = rows[0][1], rows[0][2]
    h = Handler(None, None, subjects=lookup.HostSubjects(snap))
    code, body = h.get_list_subjects(urlencode({"namespace": "", "object": obj, "relation": rel}))
    assert code == 400 and "wildcard" in body["error"]["reason"]


def test_no_handle_is_404(snap):
    for h in (Handler(None, None), Handler(None, None, None, None)):
        for code, body in (h.get_list_objects("namespace=n&relation=view&subject_id=u129"),
                           h.get_list_subjects("namespace=n&object=f65&relation=view")):
            assert code == 404 and body["error"]["code"] == 404 and body["error"]["status"] == "Not Found"
    only = Handler(None, None, lookup=lookup.HostLookup(snap))
    assert only.get_list_objects("namespace=n&relation=view&subject_id=u129")[0] == 200
    assert only.get_list_subjects("namespace=n&object=f65&relation=view")[0] == 404


def test_existing_routes_are_unchanged(handler, snap):
    two = Handler(None, expand.Engine(snap))
    for query in ("namespace=n&object=top&relation=view&max-depth=3", "namespace=n&object=top&relation=view",
                  "max-depth=foo", "max-depth=2&namespace=nowhere",
                  "namespace=n&object=nothing&relation=x&max-depth=2"):
        assert handler.get_expand(query) == two.get_expand(query)
    assert handler.get_expand("namespace=n&object=top&relation=view&max-depth=3")[0] == 200
    # /check: the answers that need no engine (the allowed / denied ones run on the GPU in test_handler.py)
    for query in ("", "subject=not%23a+valid+userset+rewrite", "namespace=n&subject_set.namespace=n"):
        assert handler.get_check(query) == two.get_check(query) and handler.get_check(query)[0] == 400
    for body in (b"{not json", b'{"namespace":"n","object":1,"relation":"r","subject_id":"s"}'):
        assert handler.post_check(body) == two.post_check(body) and handler.post_check(body)[0] == 400
    bad = b'{"tuples":[{"namespace":"n","object":1,"relation":"r","subject_id":"s"}]}'
    assert handler.post_check_batch(bad) == two.post_check_batch(bad)

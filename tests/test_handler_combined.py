"""The combined list routes of the REST handler mirror (keto_amd/handler.py
get_list_objects_combined / get_list_subjects_combined) over the CPU twins; no GPU."""
from urllib.parse import urlencode

import pytest

from keto_amd import expand, lookup
from keto_amd import relationtuple as rt
from keto_amd.handler import Handler
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import subjects_cases as SC
from tests.test_handler_lists import chain

OBJ = {"namespace": "n", "relation": "view", "subject_id": "u129"}
SUB = {"namespace": "n", "object": "f129", "relation": "view"}
OTHER_SUB = {"other_namespace": "n", "other_object": "f65", "other_relation": "view"}


@pytest.fixture(scope="module")
def snap():
    return Snapshot.from_rows(LC.NS1, SC.structure_rows())


@pytest.fixture(scope="module")
def handler(snap):
    return Handler(None, expand.Engine(snap), lookup.HostLookup(snap), lookup.HostSubjects(snap))


@pytest.mark.parametrize("op,size", [("or", 194), ("andnot", 129), ("and", 0)])
def test_list_objects_combined_route(handler, snap, op, size):
    twin = lookup.HostLookup(snap)
    ua, ub = rt.SubjectID("u129"), rt.SubjectID("u65")
    bodies = chain(handler.get_list_objects_combined, **OBJ, other_subject_id="u65", op=op, page_size="50")
    assert all(set(b) == {"objects", "next_page_token", "total"} and b["total"] == size for b in bodies)
    assert sorted(o for b in bodies for o in b["objects"]) == twin.ListObjectsCombined("n", "view", ua, ub, op)
    assert len(bodies) == max(1, -(-size // 50))
    first = twin.list_objects_combined_page("n", "view", ua, ub, op, 50)
    assert bodies[0] == {"objects": first[0], "next_page_token": first[1], "total": first[2]}


def test_second_subject_forms(handler, snap):
    twin = lookup.HostLookup(snap)
    g1 = rt.SubjectSet("n", "g1", "member")
    q = {"namespace": "n", "relation": "view", "subject_id": "ux", "other_subject_set.namespace": "n",
         "other_subject_set.object": "g1", "other_subject_set.relation": "member"}
    for op in ("and", "andnot", "or"):
        code, body = handler.get_list_objects_combined(urlencode({**q, "op": op}))
        items, token, total = twin.list_objects_combined_page("n", "view", rt.SubjectID("ux"), g1, op)
        assert code == 200 and body == {"objects": items, "next_page_token": token, "total": total}
    assert handler.get_list_objects_combined(urlencode({**q, "op": "and"}))[1]["objects"] == ["top"]
    # nothing to list is 200 with an empty page
    empty = (200, {"objects": [], "next_page_token": "", "total": 0})
    assert handler.get_list_objects_combined(urlencode({**OBJ, "namespace": "nowhere", "other_subject_id": "u65",
                                                        "op": "or"})) == empty
    assert handler.get_list_objects_combined(urlencode({**OBJ, "subject_id": "nobody", "other_subject_id": "nobody",
                                                        "op": "or"})) == empty


@pytest.mark.parametrize("op,size", [("or", 194), ("andnot", 129), ("and", 0)])
def test_list_subjects_combined_route(handler, snap, op, size):
    twin = lookup.HostSubjects(snap)
    ra, rb = ("n", "f129", "view"), ("n", "f65", "view")
    bodies = chain(handler.get_list_subjects_combined, **SUB, **OTHER_SUB, op=op, page_size="64")
    assert all(set(b) == {"subjects", "next_page_token", "total"} and b["total"] == size for b in bodies)
    got = sorted((s for b in bodies for s in b["subjects"]), key=lambda s: s["subject_id"])
    assert got == [s.to_dict() for s in twin.ListSubjectsCombined(ra, rb, op)]
    first = twin.list_subjects_combined_page(ra, rb, op, "ids", 64)
    assert bodies[0] == {"subjects": [s.to_dict() for s in first[0]], "next_page_token": first[1], "total": first[2]}


def test_kinds(handler):
    q = {"namespace": "n", "object": "two", "relation": "view", "other_namespace": "n", "other_object": "f65",
         "other_relation": "view", "op": "or"}
    assert handler.get_list_subjects_combined(urlencode(q))[1]["total"] == 105
    assert handler.get_list_subjects_combined(urlencode({**q, "kind": "any"}))[1]["total"] == 107
    code, body = handler.get_list_subjects_combined(urlencode({**q, "kind": "n#member"}))
    assert code == 200 and sorted(s["subject_set"]["object"] for s in body["subjects"]) == ["two_ga", "two_gb"]
    assert handler.get_list_subjects_combined(urlencode({**q, "kind": "users"}))[0] == 400


def test_bad_requests(handler):
    lo, ls = handler.get_list_objects_combined, handler.get_list_subjects_combined
    good_o, good_s = {**OBJ, "other_subject_id": "u65", "op": "or"}, {**SUB, **OTHER_SUB, "op": "or"}
    assert lo(urlencode(good_o))[0] == 200 and ls(urlencode(good_s))[0] == 200
    for route, good in ((lo, good_o), (ls, good_s)):
        for bad in ({"op": "xor"}, {"op": ""}, {"op": "AND"}, {"page_size": "0"}, {"page_size": "x"},
                    {"page_size": "65537"}, {"page_token": "x"}, {"page_token": "-1"}, {"page_token": "4294967296"}):
            code, body = route(urlencode({**good, **bad}))
            assert code == 400 and body["error"]["code"] == 400 and body["error"]["status"] == "Bad Request", bad
        missing_op = {k: v for k, v in good.items() if k != "op"}
        assert route(urlencode(missing_op))[0] == 400
    # a missing first or second side
    assert lo(urlencode({k: v for k, v in good_o.items() if k != "subject_id"}))[0] == 400
    assert lo(urlencode({k: v for k, v in good_o.items() if k != "other_subject_id"}))[0] == 400
    assert lo(urlencode({**good_o, "other_subject_set.namespace": "n"}))[0] == 400  # both forms
    assert lo(urlencode({**{k: v for k, v in good_o.items() if k != "other_subject_id"},
                         "other_subject_set.namespace": "n"}))[0] == 400  # an incomplete subject set
    for k in OTHER_SUB:
        assert ls(urlencode({x: v for x, v in good_s.items() if x != k}))[0] == 400


def test_wildcard_root_without_a_node_is_400():
    _, rows, snap = LC.table(*LC.TABLES[1])
    obj, rel = rows[0][1], rows[0][2]
    h = Handler(None, None, subjects=lookup.HostSubjects(snap))
    code, body = h.get_list_subjects_combined(urlencode({"namespace": "", "object": obj, "relation": rel,
                                                         "other_namespace": "", "other_object": obj,
                                                         "other_relation": rel, "op": "and"}))
    assert code == 400 and "wildcard" in body["error"]["reason"]


def test_no_handle_is_404(snap):
    qo, qs = urlencode({**OBJ, "other_subject_id": "u65", "op": "or"}), urlencode({**SUB, **OTHER_SUB, "op": "or"})
    for h in (Handler(None, None), Handler(None, None, None, None)):
        for code, body in (h.get_list_objects_combined(qo), h.get_list_subjects_combined(qs)):
            assert code == 404 and body["error"]["code"] == 404 and body["error"]["status"] == "Not Found"
    only = Handler(None, None, lookup=lookup.HostLookup(snap))
    assert only.get_list_objects_combined(qo)[0] == 200 and only.get_list_subjects_combined(qs)[0] == 404

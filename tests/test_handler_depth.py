"""max-depth on the list routes of the REST handler mirror (keto_amd/handler.py get_list_objects /
get_list_subjects) over the CPU twins of the depth calls; no GPU."""
import json
from urllib.parse import urlencode

import pytest

from keto_amd import expand, lookup
from keto_amd import relationtuple as rt
from keto_amd.handler import Handler
from keto_amd.snapshot import Snapshot
from tests import lookup_cases as LC
from tests import subjects_cases as SC
from tests.test_handler_lists import chain


@pytest.fixture(scope="module")
def snap():
    return Snapshot.from_rows(LC.NS1, SC.structure_rows())


@pytest.fixture(scope="module")
def handler(snap):
    return Handler(None, expand.Engine(snap), lookup.HostLookup(snap), lookup.HostSubjects(snap))


def test_list_objects_with_max_depth(handler):
    # ux is held by g0, g0 by g1 and g2, both by top#view: groups at 1 and 2 hops, the document at 3
    base = "namespace=n&relation=member&subject_id=ux"
    assert handler.get_list_objects(base + "&max-depth=1") == \
        (200, {"objects": ["g0"], "next_page_token": "", "total": 1, "complete": False})
    code, body = handler.get_list_objects(base + "&max-depth=2")
    assert code == 200 and sorted(body["objects"]) == ["g0", "g1", "g2"] and body["complete"] is False
    code, body = handler.get_list_objects(base + "&max-depth=3")
    assert code == 200 and body["total"] == 3 and body["complete"] is True
    view = "namespace=n&relation=view&subject_id=ux"
    assert handler.get_list_objects(view + "&max-depth=2") == \
        (200, {"objects": [], "next_page_token": "", "total": 0, "complete": False})
    assert handler.get_list_objects(view + "&max-depth=0x3") == \
        (200, {"objects": ["top"], "next_page_token": "", "total": 1, "complete": True})
    # a depth beyond any closure, and beyond 32 bits: the whole list
    for deep in ("4000", str(2**40)):
        code, body = handler.get_list_objects(f"namespace=n&relation=member&subject_id=uc&max-depth={deep}"
                                              "&page_size=65536")
        assert code == 200 and body["total"] == 3000 and body["complete"] is True
    # pages of a depth-limited list: the token belongs to the (request, depth) pair
    bodies = chain(handler.get_list_objects, namespace="n", relation="member", subject_id="uc", page_size="7",
                   **{"max-depth": "20"})
    assert [len(b["objects"]) for b in bodies] == [7, 7, 6]
    assert all(b["total"] == 20 and b["complete"] is False for b in bodies)
    assert sorted(o for b in bodies for o in b["objects"]) == sorted(f"c{i}" for i in range(20))
    # nothing to list
    assert handler.get_list_objects("namespace=nowhere&relation=view&subject_id=ux&max-depth=2") == \
        (200, {"objects": [], "next_page_token": "", "total": 0, "complete": True})
    assert handler.get_list_objects("namespace=n&relation=view&subject_id=nobody&max-depth=2") == \
        (200, {"objects": [], "next_page_token": "", "total": 0, "complete": True})


def test_list_subjects_with_max_depth(handler):
    # top#view holds g1 and g2, both hold g0, g0 holds ux
    base = "namespace=n&object=top&relation=view"
    assert handler.get_list_subjects(base + "&max-depth=2") == \
        (200, {"subjects": [], "next_page_token": "", "total": 0, "complete": False})
    assert handler.get_list_subjects(base + "&max-depth=3") == \
        (200, {"subjects": [{"subject_id": "ux"}], "next_page_token": "", "total": 1, "complete": True})
    code, body = handler.get_list_subjects(base + "&kind=any&max-depth=1")
    assert code == 200 and body["total"] == 2 and body["complete"] is False
    assert sorted(s["subject_set"]["object"] for s in body["subjects"]) == ["g1", "g2"]
    code, body = handler.get_list_subjects(base + "&kind=n%23member&max-depth=2")
    assert code == 200 and body["total"] == 3 and body["complete"] is False
    # a document held directly: complete at one hop
    code, body = handler.get_list_subjects("namespace=n&object=f65&relation=view&max-depth=1")
    assert code == 200 and body["total"] == 65 and body["complete"] is True and body["next_page_token"] == ""


@pytest.mark.parametrize("bad", ["0", "-1", "", "x", "1.5", " 2", "0x", str(2**63)])
def test_bad_max_depth_is_400(handler, bad):
    for route, base in ((handler.get_list_objects, {"namespace": "n", "relation": "view", "subject_id": "ux"}),
                        (handler.get_list_subjects, {"namespace": "n", "object": "top", "relation": "view"})):
        code, body = route(urlencode({**base, "max-depth": bad}))
        assert code == 400 and body["error"]["code"] == 400, (bad, body)


def test_other_400s_keep_their_place(handler):
    assert handler.get_list_objects("namespace=n&relation=view&max-depth=2")[0] == 400  # no subject
    assert handler.get_list_objects("namespace=n&relation=view&subject_id=ux&max-depth=2&page_size=0")[0] == 400
    assert handler.get_list_objects("namespace=n&relation=view&subject_id=ux&max-depth=2&page_token=x")[0] == 400
    assert handler.get_list_subjects("namespace=n&object=top&relation=view&kind=bad&max-depth=2")[0] == 400
    none = Handler(None, None)
    assert none.get_list_objects("namespace=n&relation=view&subject_id=ux&max-depth=2")[0] == 404


def test_without_the_parameter_nothing_changes(handler, snap):
    """the bodies are those of the plain paged twins, key for key and byte for byte"""
    twin = lookup.HostLookup(snap).list_objects_page("n", "view", rt.SubjectID("u129"), 50)
    code, body = handler.get_list_objects("namespace=n&relation=view&subject_id=u129&page_size=50")
    assert code == 200 and list(body) == ["objects", "next_page_token", "total"]
    assert json.dumps(body) == json.dumps({"objects": twin[0], "next_page_token": twin[1], "total": twin[2]})
    twin = lookup.HostSubjects(snap).list_subjects_page("n", "f129", "view", "ids", 50)
    code, body = handler.get_list_subjects("namespace=n&object=f129&relation=view&page_size=50")
    assert code == 200 and list(body) == ["subjects", "next_page_token", "total"]
    assert json.dumps(body) == json.dumps({"subjects": [s.to_dict() for s in twin[0]], "next_page_token": twin[1],
                                           "total": twin[2]})
    assert len(twin) == 3  # the plain call's return value keeps its shape

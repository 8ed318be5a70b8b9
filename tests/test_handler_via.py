"""via=true on the list routes of the REST handler mirror (keto_amd/handler.py get_list_objects /
get_list_subjects) over the CPU twins of the via calls; no GPU."""
import pytest

from keto_amd import expand, lookup
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


def sset(obj, rel="member"):
    return {"subject_set": {"namespace": "n", "object": obj, "relation": rel}}


def test_list_objects_with_via(handler):
    # ux is held by g0, g0 by g1 and g2, both by top#view: groups at 1 and 2 hops, the document at 3
    base = "namespace=n&relation=member&subject_id=ux"
    code, body = handler.get_list_objects(base + "&via=true")
    assert code == 200 and body["total"] == 3 and body["next_page_token"] == "" and "complete" not in body
    by = {e["object"]: e for e in body["objects"]}
    assert by["g0"] == {"object": "g0", "via": {"subject_id": "ux"}, "hops": 1}
    assert by["g1"] == {"object": "g1", "via": sset("g0"), "hops": 2} and by["g2"]["via"] == sset("g0")
    code, body = handler.get_list_objects("namespace=n&relation=view&subject_id=ux&via=true")
    assert code == 200 and len(body["objects"]) == 1
    top = body["objects"][0]
    assert top["object"] == "top" and top["hops"] == 3 and top["via"] in (sset("g1"), sset("g2"))  # a diamond
    # it composes with max-depth
    assert handler.get_list_objects(base + "&via=true&max-depth=1") == \
        (200, {"objects": [by["g0"]], "next_page_token": "", "total": 1, "complete": False})
    # pages: the entries of the unpaged answer, in its order
    bodies = chain(handler.get_list_objects, namespace="n", relation="member", subject_id="uc", page_size="7",
                   via="true", **{"max-depth": "20"})
    assert [len(b["objects"]) for b in bodies] == [7, 7, 6] and all(b["total"] == 20 for b in bodies)
    entries = [e for b in bodies for e in b["objects"]]
    assert sorted(e["hops"] for e in entries) == list(range(1, 21))
    names = {e["hops"]: e["object"] for e in entries}
    assert all(e["via"] == ({"subject_id": "uc"} if e["hops"] == 1 else sset(names[e["hops"] - 1])) for e in entries)
    # nothing to list
    assert handler.get_list_objects("namespace=nowhere&relation=view&subject_id=ux&via=true") == \
        (200, {"objects": [], "next_page_token": "", "total": 0})
    assert handler.get_list_objects("namespace=n&relation=view&subject_id=nobody&via=true&max-depth=2") == \
        (200, {"objects": [], "next_page_token": "", "total": 0, "complete": True})


def test_list_subjects_with_via(handler):
    # top#view holds g1 and g2, both hold g0, g0 holds ux
    base = "namespace=n&object=top&relation=view"
    code, body = handler.get_list_subjects(base + "&via=true")
    assert (code, body) == (200, {"subjects": [{"subject": {"subject_id": "ux"}, "via": sset("g0"), "hops": 3}],
                                  "next_page_token": "", "total": 1})
    code, body = handler.get_list_subjects(base + "&kind=any&via=true")
    assert code == 200 and body["total"] == 4
    hops = {e["subject"].get("subject_id") or e["subject"]["subject_set"]["object"]: e for e in body["subjects"]}
    assert {k: e["hops"] for k, e in hops.items()} == {"g1": 1, "g2": 1, "g0": 2, "ux": 3}
    assert hops["g1"]["via"] == hops["g2"]["via"] == sset("top", "view")
    assert hops["g0"]["via"] in (sset("g1"), sset("g2"))  # a diamond
    code, body = handler.get_list_subjects(base + "&kind=any&via=true&max-depth=1")
    assert code == 200 and body["complete"] is False and sorted(e["hops"] for e in body["subjects"]) == [1, 1]
    code, body = handler.get_list_subjects(base + "&kind=n%23member&via=true&max-depth=2")
    assert code == 200 and body["total"] == 3 and body["complete"] is False


@pytest.mark.parametrize("value", ["", "1", "True", "false", "yes", "TRUE", "true "])
def test_any_other_value_is_a_bad_request(handler, value):
    from urllib.parse import quote
    for get, base in ((handler.get_list_objects, "namespace=n&relation=member&subject_id=ux"),
                      (handler.get_list_subjects, "namespace=n&object=top&relation=view")):
        code, body = get(f"{base}&via={quote(value)}")
        assert code == 400 and "via" in body["error"]["reason"]


def test_bodies_without_via_are_unchanged(handler):
    base = "namespace=n&relation=member&subject_id=ux"
    assert handler.get_list_objects(base + "&max-depth=1") == \
        (200, {"objects": ["g0"], "next_page_token": "", "total": 1, "complete": False})
    code, body = handler.get_list_objects(base)
    assert code == 200 and sorted(body["objects"]) == ["g0", "g1", "g2"] and set(body) == \
        {"objects", "next_page_token", "total"}
    assert handler.get_list_subjects("namespace=n&object=top&relation=view") == \
        (200, {"subjects": [{"subject_id": "ux"}], "next_page_token": "", "total": 1})
    assert handler.get_list_subjects("namespace=n&object=top&relation=view&max-depth=3") == \
        (200, {"subjects": [{"subject_id": "ux"}], "next_page_token": "", "total": 1, "complete": True})

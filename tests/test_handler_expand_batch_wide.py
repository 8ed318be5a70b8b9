"""POST /expand/batch with "wide" (keto_amd/handler.py): the {"items": [...], "wide": true} form
asks the expand engine's batch for its chip-wide call; any other value of "wide" is a 400; the
list form and an absent key call the engine as before.  A recording stub stands in for the
device engine; with the host engine behind the route `wide` is taken and ignored."""
import json

from keto_amd import expand
from keto_amd import relationtuple as rt
from keto_amd.handler import Handler
from keto_amd.snapshot import Snapshot
from tests.lookup_cases import NS1, sid, sset


class Recorder:
    """an expand engine that notes how its batch was called and answers from the host engine"""

    def __init__(self, host):
        self.host, self.calls = host, []

    def build_trees_batch(self, subjects, depths, **kw):
        self.calls.append((list(subjects), list(depths), kw))
        return self.host.build_trees_batch(subjects, depths)


def _handlers():
    snap = Snapshot.from_rows(NS1, [sset("doc", "view", "g", "member"), sid("g", "member", "alice")])
    host = expand.Engine(snap)
    rec = Recorder(host)
    return Handler(None, host, expand_batch=rec), Handler(None, host), rec


ITEMS = [{"subject_set": {"namespace": "n", "object": "doc", "relation": "view"}, "max-depth": 3},
         {"subject_id": "somebody", "max-depth": "2"},
         {"subject_set": {"namespace": "nope", "object": "doc", "relation": "view"}, "max-depth": 3}]


def test_wide_true_reaches_the_engine():
    h, plain, rec = _handlers()
    want = plain.post_expand_batch(json.dumps(ITEMS))
    assert want[0] == 200 and want[1][0]["type"] == "union" and want[1][2]["error"]["code"] == 404
    assert h.post_expand_batch(json.dumps({"items": ITEMS, "wide": True})) == want
    subjects = [rt.SubjectSet("n", "doc", "view"), rt.SubjectID("somebody"), rt.SubjectSet("nope", "doc", "view")]
    assert rec.calls == [(subjects, [3, 2, 3], {"wide": True})]


def test_absent_false_and_the_list_form_call_the_engine_as_before():
    h, plain, rec = _handlers()
    want = plain.post_expand_batch(json.dumps(ITEMS))
    for body in (ITEMS, {"items": ITEMS}, {"items": ITEMS, "wide": False}):
        assert h.post_expand_batch(json.dumps(body)) == want
    assert [kw for _, _, kw in rec.calls] == [{}, {}, {}]
    assert h.post_expand_batch(json.dumps({"items": [], "wide": True})) == (200, [])


def test_any_other_value_of_wide_is_a_400():
    h, plain, rec = _handlers()
    refused = plain.post_expand_batch(b'{"a": 1}')
    assert refused[0] == 400
    for bad in (1, 0, "true", "yes", None, [], {}, 1.5):
        code, body = h.post_expand_batch(json.dumps({"items": ITEMS, "wide": bad}))
        assert code == 400 and body["error"]["code"] == 400, bad
        assert body["error"]["reason"].startswith("Unable to decode JSON payload: "), bad
        assert set(body) == set(refused[1]) and set(body["error"]) == set(refused[1]["error"])
    assert rec.calls == []


def test_the_host_engine_takes_wide_and_ignores_it():
    _, plain, _ = _handlers()
    want = plain.post_expand_batch(json.dumps(ITEMS))
    assert plain.post_expand_batch(json.dumps({"items": ITEMS, "wide": True})) == want

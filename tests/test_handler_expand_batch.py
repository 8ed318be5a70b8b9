"""POST /expand/batch (keto_amd/handler.py) against GET /expand, item by item, error bodies
included.  Without a device engine the route walks on the host (the id walk for subjects that
are snapshot nodes, ketogpu_expand for the others); test_expand_gpu.py covers the device
engine behind the same wrapper."""
import json
from urllib.parse import urlencode

from keto_amd import expand
from keto_amd.handler import Handler
from keto_amd.snapshot import Snapshot
from tests import randgraph


def _get(h, ns, obj, rel, depth):
    return h.get_expand(urlencode({"namespace": ns, "object": obj, "relation": rel, "max-depth": depth}))


def _handler(seed, page_size, poison):
    namespaces, rows = randgraph.make_graph(seed, n_rows=200, poison=poison)
    snap = Snapshot.from_rows(namespaces, rows, page_size=page_size, sort=True)
    return Handler(None, expand.Engine(snap)), randgraph.make_requests(seed, namespaces, rows, n=60)


def test_batch_matches_get_expand_item_by_item():
    for seed, page_size, poison in ((21, 100, False), (22, 2, True)):
        h, requests = _handler(seed, page_size, poison)
        items, want = [], []
        for k, (ns, o, r, _) in enumerate(requests):
            for sset, depth in (((ns, o, r), k % 5), ((ns, o, ""), 3), (("no such namespace", o, r), 2)):
                items.append({"subject_set": dict(zip(("namespace", "object", "relation"), sset)),
                              "max-depth": depth if k % 2 else str(depth)})
                want.append(_get(h, *sset, depth))
        code, body = h.post_expand_batch(json.dumps(items))
        assert code == 200 and len(body) == len(items)
        assert body == [w[1] for w in want]
        codes = {w[0] for w in want}
        assert 404 in codes and 200 in codes
        assert any(b is None for b in body) and any(b and b.get("type") == "union" for b in body)
        if poison:
            assert sum(w[0] == 404 for w in want) > len(requests)  # not only the unknown namespace


def test_batch_item_forms_and_errors():
    h, requests = _handler(21, 100, False)
    ns, o, r, _ = requests[0]
    tree = _get(h, ns, o, r, 3)[1]
    code, body = h.post_expand_batch(json.dumps([
        {"subject": {"subject_set": {"namespace": ns, "object": o, "relation": r}}, "max-depth": 3},
        {"namespace": ns, "object": o, "relation": r, "max-depth": "0x3"},
        {"subject_id": "somebody", "max-depth": 2},
        {"subject_set": {"namespace": ns, "object": o, "relation": r}, "max-depth": "foo"},
        {"subject_set": {"namespace": ns, "object": o, "relation": r}},
        {"subject_set": {"namespace": ns, "object": 5, "relation": r}, "max-depth": 1},
        {"subject_id": "u", "subject_set": {"namespace": ns}, "max-depth": 1},
        7,
        {"subject_set": {"namespace": ns, "object": o, "relation": r}, "max-depth": 0},
    ]))
    assert code == 200
    assert body[0] == tree and body[1] == tree
    assert body[2] == {"type": "leaf", "subject_id": "somebody"}
    assert body[3] == h.get_expand("max-depth=foo")[1] and body[3]["error"]["code"] == 400
    assert body[4] == h.get_expand("namespace=n")[1] and body[4]["error"]["code"] == 400
    assert [b["error"]["code"] for b in body[5:8]] == [400, 400, 400]
    assert body[8] is None
    assert h.post_expand_batch(b"{not json")[0] == 400
    assert h.post_expand_batch(b'{"a": 1}')[0] == 400
    assert h.post_expand_batch(b"[]") == (200, [])

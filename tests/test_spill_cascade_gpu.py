"""The spill cascade behind the LDS first stages (device_engine.hip bidi_tail, launch_stage):
every stage shape as the stage that finishes a unit, every KETOGPU_CASCADE order, units that
mix small and huge requests, and rows at the 16-bit edge of the packed pending degree.

Per-stage spill counts come from the `[cascade] units N, spills per stage: c0 c1 ...` line
that KETOGPU_CASCADE_LOG=1 prints per call (c0: units the first stage spilled, ck: units
stage k of the cascade spilled; logging turns the lazy launch of the stages off).
"""
import re

import numpy as np
import pytest

from keto_amd import _lib as L
from keto_amd import check
from keto_amd import relationtuple as rt
from keto_amd.snapshot import Snapshot
from tests import fan_graph, randgraph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if L.lib().ketogpu_device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


# Where a unit stops follows from the stages' tables and pending lists (launch_stage).  A
# level of a fan search makes its n nodes pending at once per side, so the pending list (F
# entries, both sides together; plan lite: a ring per side) is the first limit and the
# table's load limit the second:
#   first stage  512 slots x 7/8 = 448,  F = 128  (lite: 128-entry rings; lite32: 1024 slots, 256)
#   w           2048 slots x 6/8 = 1536, F = 384      h  1024 x 6/8 = 768,  F = 256
#   q           4096 slots x 7/8 = 3584, F = 512      r  2048 x 7/8 = 1792, F = 256
#   s           8192 slots x 7/8 = 7168, F = 1024
# The sweep: one 16-unit per (mix, width), fan_graph.WIDE or MIXED.  Spills per stage
# observed on the MI355X (units spilled by the first stage, then by each cascade stage; the
# stage that finishes the unit is the first 0):
#                  bidi w,q,s   lite w,q,s   bidi h,r,s   bidi w,h,q,r,s   lite32 w,q,s
#   WIDE 40        0 0 0 0      0 0 0 0      0 0 0 0      0 0 0 0 0 0      0 0 0 0
#   MIXED 72       1 0 0 0      0 0 0 0      1 0 0 0      1 0 0 0 0 0      0 0 0 0
#   MIXED 100      1 0 0 0      0 0 0 0      1 1 0 0      1 0 0 0 0 0      0 0 0 0
#   WIDE 160       1 0 0 0      1 0 0 0      1 1 4 0      1 0 0 0 0 0      0 0 0 0
#   WIDE 200       1 1 0 0      1 1 0 0      1 1 4 0      1 1 1 0 0 0      0 0 0 0
#   WIDE 500       1 1 4 0      1 1 4 0      1 1 4 0      1 1 1 4 4 0      1 1 4 0
#   WIDE 2400      1 1 4 8      1 1 4 8      1 1 4 8      1 1 1 4 4 8      1 1 4 8
#   WIDE 160+161   (32 requests, one lite32 unit)                          1 0 0 0
#   WIDE 200+201   (32 requests, one lite32 unit)                          1 2 0 0
# (bidi s: 0 0 | 1 0 from 72 to 500 | 1 8;  q,s: 1 0 0 from 72 to 200, 1 4 0 at 500, 1 4 8;
# r,s: 1 0 0 at 72 and 100, 1 4 0 from 160 to 500, 1 4 8.  The 8 requests left to the global
# path at 2400 are the unit's R -> T and R -> S ones.)  In w,h,q,r,s the one-wave stages
# cannot finish a unit: h is smaller than w and r smaller than q in table and list alike,
# so they spill whatever reaches them; the test asserts that they ran.  lite32's first stage is as large as w and q: those finish the
# halves of a 32-unit that holds two families (160 + 161: w; 200 + 201: q).
SWEEP = (("WIDE", 40), ("MIXED", 72), ("MIXED", 100), ("WIDE", 160), ("WIDE", 200), ("WIDE", 500), ("WIDE", 2400))
PAIRS = ((160, 161), (200, 201))
TOP = ("WIDE", 2400)
WIDTHS = fan_graph.WIDTHS


def stage_counts(err):
    """the per-stage spill counts of every logged call"""
    return [[int(x) for x in m.group(1).split()]
            for m in re.finditer(r"\[cascade\] units \d+, spills per stage:((?: \d+)+)", err)]


@pytest.fixture(scope="module")
def fans():
    rows = fan_graph.fan_rows(WIDTHS)
    snap = Snapshot.from_rows([("n", 1)], rows, sort=True)
    orc = randgraph.oracle_store([("n", 1)], rows)

    def resolved(reqs, truth):
        want = np.asarray(orc.check_batch(fan_graph.as_oracle_requests(reqs)), dtype=bool)
        np.testing.assert_array_equal(want, truth)  # the oracle agrees with the construction
        return snap.resolve_many(reqs) + (want,)
    units = {(mix, n): resolved(*fan_graph.unit_of(n, mix=getattr(fan_graph, mix))) for mix, n in SWEEP}
    for a, b in PAIRS:  # 32 requests: a 16-unit of each family
        ra, ta = fan_graph.unit_of(a, mix=fan_graph.WIDE)
        rb, tb = fan_graph.unit_of(b, mix=fan_graph.WIDE)
        units[("PAIR", a)] = resolved(ra + rb, np.concatenate([ta, tb]))
    return snap, units, resolved(*fan_graph.mixed_batch(WIDTHS))


def sweep(snap, units, capfd, keys=SWEEP):
    """every unit of the sweep as a batch of its own on one engine, each exact
    -> {unit: (spills per stage, spilled_requests)}"""
    eng = check.Engine(snap)
    out = {}
    for key in keys:
        r, t, want = units[key]
        capfd.readouterr()
        got = eng.check_ids(r, t)
        counts = stage_counts(capfd.readouterr().err)
        np.testing.assert_array_equal(got, want, err_msg=str(key))
        assert len(counts) == 1, counts
        out[key] = (counts[0], eng.last_stats()["spilled_requests"])
    print({k: out[k] for k in keys})
    return out


def assert_stages_finish(out, stages):
    """each stage in `stages` (0 = the first stage, k = the cascade's k-th) finishes the
    units of some batch: they spilled every earlier stage, and none spilled from it"""
    for k in stages:
        hit = [u for u, (c, _) in out.items() if all(x > 0 for x in c[:k]) and c[k] == 0]
        assert hit, (k, out)


def assert_top_reaches_global(out):
    c, left = out[TOP]
    assert all(x > 0 for x in c) and left > 0, out[TOP]


def test_label_plan_answers_the_sweep(fans, monkeypatch):
    """the default plan (2-hop labels) over the same batches: exact without a search"""
    snap, units, (r, t, want) = fans
    monkeypatch.delenv("KETOGPU_UNITS", raising=False)
    eng = check.Engine(snap)
    for key, (ur, ut, uw) in units.items():
        np.testing.assert_array_equal(eng.check_ids(ur, ut), uw, err_msg=str(key))
        st = eng.last_stats()
        assert st["plan"] == 7 and st["spilled_requests"] == 0
    np.testing.assert_array_equal(eng.check_ids(r, t), want)


@pytest.mark.parametrize("plan", ["bidi", "lite"])
def test_every_stage_finishes_some_width(fans, plan, monkeypatch, capfd):
    snap, units, _ = fans
    monkeypatch.setenv("KETOGPU_UNITS", plan)
    monkeypatch.setenv("KETOGPU_CASCADE_LOG", "1")
    out = sweep(snap, units, capfd)
    assert all(len(c) == 4 for c, _ in out.values())
    assert_stages_finish(out, range(4))
    assert_top_reaches_global(out)


@pytest.mark.parametrize("cascade", ["s", "q,s", "h,r,s", "w,h,q,r,s", "r,s"])
def test_every_stage_shape_and_order(fans, cascade, monkeypatch, capfd):
    snap, units, _ = fans
    monkeypatch.setenv("KETOGPU_UNITS", "bidi")
    monkeypatch.setenv("KETOGPU_CASCADE_LOG", "1")
    monkeypatch.setenv("KETOGPU_CASCADE", cascade)
    names = cascade.split(",")
    out = sweep(snap, units, capfd)
    assert all(len(c) == len(names) + 1 for c, _ in out.values())
    if cascade == "w,h,q,r,s":
        # h after w and r after q only ever see units that the larger shape spilled: they
        # cannot finish one; they run (and spill on)
        assert_stages_finish(out, [0, 1, 3, 5])
        assert any(c[2] > 0 for c, _ in out.values()) and any(c[4] > 0 for c, _ in out.values())
    else:
        assert_stages_finish(out, range(len(names) + 1))
    assert_top_reaches_global(out)


def test_lite32_first_stage_fans_two_into_w(fans, monkeypatch, capfd):
    """32-request units: a spilled unit is two 16-units for w.  The first stage holds what w
    and q hold of one family, so those stages finish the halves of units that hold two"""
    snap, units, _ = fans
    monkeypatch.setenv("KETOGPU_UNITS", "lite32")
    monkeypatch.setenv("KETOGPU_CASCADE_LOG", "1")
    out = sweep(snap, units, capfd, SWEEP + tuple(("PAIR", a) for a, _ in PAIRS))
    assert all(len(c) == 4 for c, _ in out.values())
    assert_stages_finish(out, range(4))
    assert_top_reaches_global(out)
    c, _ = out[("PAIR", 200)]
    assert c[0] == 1 and c[1] == 2  # one 32-unit spilled, both of its 16-units spilled w


@pytest.mark.parametrize("cascade", ["w,q", "w", "q,s,w", "s,s,s,s,s,s,s", "x"])
def test_cascades_the_engine_refuses(fans, cascade, monkeypatch):
    """a cascade that does not end in the single-request stage, has more than 6 stages or
    names no stage is refused when the engine is created"""
    monkeypatch.setenv("KETOGPU_UNITS", "bidi")
    monkeypatch.setenv("KETOGPU_CASCADE", cascade)
    with pytest.raises(L.KetoError) as e:
        check.Engine(fans[0])
    assert e.value.code == L.EINVAL


@pytest.mark.parametrize("plan", ["bidi", "lite", "core", "v2"])
def test_mixed_units(fans, plan, monkeypatch):
    """all widths interleaved request by request with a tail that is no multiple of 16: a
    spilled 16-unit fans out into 4-units and single requests of which only some are hard"""
    snap, _, (r, t, want) = fans
    monkeypatch.setenv("KETOGPU_UNITS", plan)
    eng = check.Engine(snap)
    q = eng.upload(r, t)
    for _ in range(3):
        q.run()
        ab, _ = q.download_words()
        np.testing.assert_array_equal(check.unpack_bits(ab, len(r)), want)
        assert int(ab[-1]) >> (len(r) % 64) == 0
    assert eng.last_stats()["spilled_units"] > 0
    pr, pt = check.pinned(r), check.pinned(t)
    out = check.PinnedBuffer((len(r) + 63) // 64, np.uint64)
    eng.check_ids_raw(pr.array.ctypes.data, pt.array.ctypes.data, len(r), out.array.ctypes.data)
    np.testing.assert_array_equal(check.unpack_bits(out.array.copy(), len(r)), want)


# ------------------------------------------------------------------ rows of 65535..65537
EDGE = (65535, 65536, 65537)


@pytest.fixture(scope="module")
def long_rows():
    """top{m} holds the first m of 65537 groups c_i (each holding one user).  T{m} is below the
    m groups r_0 .. r_{m-1}, V{m} below the m groups r_1 .. r_m, every r_i below z.  One bridge
    c_0 -> r_0: every top{m} reaches every T{k} over it and no V{k} (r_0 is not above V), so
    each m has top{m} against a target with a reverse row of m entries both with and without
    a path.  -> snapshot, {m: (roots, targets, truth)}, {m: the cheap requests alone}"""
    top = max(EDGE)
    rows = []
    for i in range(top):
        rows.append((1, f"c{i:05d}", "m", f"u{i}", None, None, None))
    for i in range(top + 1):
        rows.append((1, "z", "m", None, 1, f"r{i:05d}", "m"))
    for m in EDGE:
        rows += [(1, f"top{m}", "m", None, 1, f"c{i:05d}", "m") for i in range(m)]
        rows += [(1, f"r{i:05d}", "m", None, 1, f"T{m}", "m") for i in range(m)]
        rows += [(1, f"r{i:05d}", "m", None, 1, f"V{m}", "m") for i in range(1, m + 1)]
    rows.append((1, "c00000", "m", None, 1, "r00000", "m"))
    snap = Snapshot.from_rows([("n", 1)], rows, sort=True)
    orc = randgraph.oracle_store([("n", 1)], rows)
    g = snap.graph()
    batches, cheap = {}, {}
    for m in EDGE:
        reqs, want = [], []

        def add(obj, subj, truth):
            reqs.append(("n", obj, "m", subj))
            want.append(truth)
        T, V = (lambda k: rt.SubjectSet("n", f"T{k}", "m")), (lambda k: rt.SubjectSet("n", f"V{k}", "m"))
        for i in (0, m // 2, m - 1):
            add(f"top{m}", rt.SubjectID(f"u{i}"), True)  # under the first / middle / last successor
        add(f"top{m}", rt.SubjectID(f"u{m}"), False)  # under the first group the root does not hold
        add(f"top{m}", rt.SubjectID("nobody"), False)
        for k in EDGE:  # both seed rows long: with the bridge (T) and without a path (V)
            add(f"top{m}", T(k), True)
            add(f"top{m}", V(k), False)
        add("r00003", T(m), True)  # small roots against the long reverse rows
        add("c00000", T(m), True)
        add("c00000", V(m), False)
        add("c00002", T(m), False)
        add(f"r{m - 1:05d}", T(m), True)  # the rows' last entries
        add(f"r{m:05d}", V(m), True)
        add(f"r{m:05d}", T(m), False)
        add("r00000", V(m), False)
        r, t = snap.resolve_many(reqs)
        batches[m] = (r, t, np.array(want))
        np.testing.assert_array_equal(orc.check_batch(fan_graph.as_oracle_requests(reqs)), want)
        # the rows are as long as they are meant to be
        assert g["fint_off"][r[0] + 1] - g["fint_off"][r[0]] == m
        j = 5 + 2 * EDGE.index(m)  # top{m} against T{m} and V{m}
        for tgt in (t[j], t[j + 1]):
            assert g["rev_off"][tgt + 1] - g["rev_off"][tgt] == m
        cheap[m] = snap.resolve_many([("n", f"top{m}", "m", rt.SubjectID(f"u{i}")) for i in (0, m - 1)] * 8)
    return snap, batches, cheap


@pytest.mark.parametrize("plan", ["bidi", "lite", "core", "v2", "label", "label-rest", "global", "global-nohubs"])
def test_rows_at_the_packed_degree_edge(long_rows, plan, monkeypatch):
    """pending entries pack the row length into 16 bits: a seed row or pushed node of more than
    65535 entries must spill the unit (bidi_unit, bidi_push, the lite unit), whichever side is
    the cheaper one"""
    snap, batches, cheap = long_rows
    if plan.startswith("global"):
        monkeypatch.setenv("KETOGPU_PATH", "global")
        if plan == "global-nohubs":  # (the long roots are hubs otherwise: looked up, not expanded)
            monkeypatch.setenv("KETOGPU_HUBS", "0")
    else:
        monkeypatch.setenv("KETOGPU_UNITS", plan.split("-")[0])
        if plan == "label-rest":
            monkeypatch.setenv("KETOGPU_LABEL_REST_PERMILLE", "400")
    eng = check.Engine(snap)
    for m in EDGE:
        r, t, want = batches[m]
        np.testing.assert_array_equal(eng.check_ids(r, t), want, err_msg=f"m = {m}")
        st = eng.last_stats()
        print(plan, m, {k: st[k] for k in ("plan", "spilled_units", "spilled_requests", "rest_requests")})
        if plan in ("bidi", "lite") and m >= 65536:
            assert st["spilled_requests"] > 0
    # all three at once, resident
    r, t, want = (np.concatenate([batches[m][k] for m in EDGE]) for k in range(3))
    q = eng.upload(r, t)
    q.run()
    np.testing.assert_array_equal(q.download(), want)
    # The cheap requests alone (a user right under the root's first / last successor: the
    # backward side is three nodes): nothing but the root's seed row is long, so the unit
    # spills exactly when that row's length no longer packs, 65536 and up.  65535 packs as
    # 0xFFFF and is answered in the first stage.
    if plan in ("bidi", "lite"):
        for m in EDGE:
            r, t = cheap[m]
            assert eng.check_ids(r, t).all()
            st = eng.last_stats()
            print(plan, "cheap", m, {k: st[k] for k in ("spilled_units", "spilled_requests")})
            if m >= 65536:
                assert st["spilled_requests"] == len(r)
            else:
                assert st["spilled_units"] == 0 and st["spilled_requests"] == 0

"""Two-sided fans of chosen widths for the spill-cascade tests.

Family n: the root R{n} holds n groups a_i, each holding b_i, each holding one user; the
targets T{n} and S{n} are below groups p_i, each below q_i, all below z{n} (T below every
p_i, S below every p_i but p_7); one bridge b_7 -> q_7.  Every fan node has interior
successors or predecessors of its own, so the searches' dead-end rule does not keep them out
of the LDS table.  R{n} reaches T{n} (over the bridge and p_7) and the users under the b_i,
not S{n}: a search of R{n} against T{n} or S{n} is n wide on both sides, level after level.
"""
import numpy as np

from keto_amd import relationtuple as rt


def fan_rows(widths):
    rows = []
    for n in widths:
        for i in range(n):
            rows.append((1, f"R{n}", "m", None, 1, f"a{n}_{i}", "m"))
            rows.append((1, f"a{n}_{i}", "m", None, 1, f"b{n}_{i}", "m"))
            rows.append((1, f"b{n}_{i}", "m", f"u{n}_{i}", None, None, None))
            rows.append((1, f"p{n}_{i}", "m", None, 1, f"T{n}", "m"))
            if i != 7:
                rows.append((1, f"p{n}_{i}", "m", None, 1, f"S{n}", "m"))
            rows.append((1, f"q{n}_{i}", "m", None, 1, f"p{n}_{i}", "m"))
            rows.append((1, f"z{n}", "m", None, 1, f"q{n}_{i}", "m"))
        rows.append((1, f"b{n}_7", "m", None, 1, f"q{n}_7", "m"))
    return rows


def family_requests(n):
    """the request kinds of family n -> [((namespace, object, relation, subject), truth)]"""
    R = lambda s: ("n", f"R{n}", "m", s)
    Z = lambda s: ("n", f"z{n}", "m", s)
    T, S = rt.SubjectSet("n", f"T{n}", "m"), rt.SubjectSet("n", f"S{n}", "m")
    return {"RT": (R(T), True), "RS": (R(S), False), "Ru": (R(rt.SubjectID(f"u{n}_{n // 2}")), True),
            "Rx": (R(rt.SubjectID("nobody")), False), "ZT": (Z(T), True), "ZS": (Z(S), True),
            "Zu": (Z(rt.SubjectID(f"u{n}_3")), False), "aT": (("n", f"a{n}_3", "m", T), False)}


# A 16-unit of one family.  WIDE: every request rooted at R{n}, so all of them make the same
# n nodes pending per side and level.  MIXED: four requests rooted at z{n} as well, whose
# forward side adds the q_i: a 16-request unit then carries three fans at once while the
# 4-request units it splits into carry two (the one-wave stage `r` holds what `h` spilled).
WIDE = ("RT", "RS", "Ru", "Rx", "RT", "RS", "Ru", "Rx") * 2
MIXED = ("RT", "RS", "Ru", "Rx", "RT", "RS", "Ru", "aT", "RS", "RT", "Ru", "Rx", "ZT", "ZS", "Zu", "ZT")
WIDTHS = (40, 72, 100, 160, 161, 200, 201, 500, 2400)


def unit_of(n, k=16, mix=MIXED):
    """k requests of family n (a whole 16-unit of one size) -> (requests, truth)"""
    kinds = family_requests(n)
    reqs = [kinds[mix[i % len(mix)]] for i in range(k)]
    return [r for r, _ in reqs], np.array([w for _, w in reqs])


def mixed_batch(widths, k=203, mix=MIXED):
    """all widths interleaved request by request, k requests (no multiple of 16): every
    16-unit holds small and huge requests -> (requests, truth)"""
    kinds = {n: family_requests(n) for n in widths}
    reqs = [kinds[widths[i % len(widths)]][mix[(i // len(widths)) % len(mix)]] for i in range(k)]
    return [r for r, _ in reqs], np.array([w for _, w in reqs])


def as_oracle_requests(reqs):
    def subj(s):
        if isinstance(s, rt.SubjectID):
            return {"subject_id": s.id}
        return {"subject_set": {"namespace": s.namespace, "object": s.object, "relation": s.relation}}
    return [(ns, o, r, subj(s)) for ns, o, r, s in reqs]

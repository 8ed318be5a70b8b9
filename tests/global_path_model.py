"""A plain model of the global path's frontier-list use (device_engine.hip: seed_kernel,
expand_kernel / push_one, gather_kernel, Engine::round and run_global), over
Snapshot.graph().  No hub index.

A round takes W consecutive 64-request words.  Every word runs a level-synchronous BFS over
the interior subgraph with a 64-bit request mask per node:
  * level 0: one list entry per request whose root r is expandable (r < Nx) with a
    non-empty interior row and whose target is not NODE_NONE (requests of one word with the
    same root get one entry each: the seed does not merge them);
  * every later level: one entry per (word, node) that received at least one new request
    bit in the level before and has a non-empty interior row (two requests of one word that
    reach a node in the same level share the entry; a node reached again in a later level by
    another request is appended again).
The entries of all levels of a round stay in one list: the round needs their sum in slots
and overflows when that exceeds the list capacity.
"""

NODE_NONE = 0xFFFFFFFF


def word_levels(graph, roots, targets):
    """entries per level of one word (up to 64 requests, in batch order)"""
    off, col, nx = graph["fint_off"], graph["fint_col"], graph["Nx"]
    assert len(roots) <= 64
    frontier = []  # (node, mask) entries of the current level
    for b, (r, t) in enumerate(zip(roots, targets)):
        r, t = int(r), int(t)
        if r < nx and t != NODE_NONE and off[r + 1] > off[r]:
            frontier.append((r, 1 << b))
    vis = {}
    levels = []
    while frontier:
        levels.append(len(frontier))
        gained = {}
        for v, m in frontier:
            for u in col[int(off[v]):int(off[v + 1])]:
                u = int(u)
                new = m & ~vis.get(u, 0)
                if new:
                    vis[u] = vis.get(u, 0) | new
                    gained[u] = gained.get(u, 0) | new
        frontier = [(u, m) for u, m in gained.items() if off[u + 1] > off[u]]
    return levels


def round_cost(graph, roots, targets):
    """one round over the given requests (words of 64 in order) -> dict: entries per level
    summed over the round's words, `slots` (their sum: the list slots the round needs) and
    `levels` (the levels the round runs: the deepest word's)"""
    per = []
    for c in range(0, len(roots), 64):
        lv = word_levels(graph, roots[c:c + 64], targets[c:c + 64])
        per += [0] * (len(lv) - len(per))
        for i, x in enumerate(lv):
            per[i] += x
    return {"per_level": per, "slots": sum(per), "levels": len(per)}


def round_width(ni, fe_cap, state_budget_bytes, max_words_per_round=0, hub_words=0):
    """the words per round the engine constructor picks for an explicit state budget"""
    lists = state_budget_bytes // 4
    per_word = 16 * max(ni, 1) + 64 * 8 * hub_words
    w = max(1, (state_budget_bytes - lists) // per_word)
    if max_words_per_round:
        w = min(w, max_words_per_round)
    w = min(w, 1 << 20)
    return max(1, min(w, fe_cap // (ni + 64)))


def list_capacity(state_budget_bytes):
    """fe_cap for an explicit state budget (below the 2^28 entry ceiling)"""
    return max(state_budget_bytes // 4 // 32, 1 << 16)


def plan_rounds(graph, roots, targets, width, cap):
    """run_global over the batch: rounds of `width` words, a round that needs more than
    `cap` slots is retried at half its width (the narrower width is kept); a single word that
    does not fit is run in passes over halves of its requests.  -> dict: `retries` (failed
    rounds and passes), `rounds` (successful ones), `split_words` (words run in passes)"""
    words = (len(roots) + 63) // 64
    slots = [round_cost(graph, roots[64 * w:64 * w + 64], targets[64 * w:64 * w + 64])["slots"] for w in range(words)]
    retries = rounds = split = 0
    widths = []

    def passes(w, bits):  # a word's requests `bits` in two halves
        nonlocal retries, rounds
        assert len(bits) > 1, "a single request does not fit the lists"
        for part in (bits[:len(bits) // 2], bits[len(bits) // 2:]):
            r = [roots[64 * w + b] for b in part]
            t = [targets[64 * w + b] for b in part]
            if round_cost(graph, r, t)["slots"] > cap:
                retries += 1
                passes(w, part)
            else:
                rounds += 1

    w0, W = 0, width
    while w0 < words:
        wn = min(W, words - w0)
        widths.append(wn)
        if sum(slots[w0:w0 + wn]) > cap:
            retries += 1
            if wn == 1:
                split += 1
                passes(w0, list(range(min(64, len(roots) - 64 * w0))))
                w0 += 1
                continue
            W = max(1, wn // 2)
            continue
        rounds += 1
        w0 += wn
    return {"retries": retries, "rounds": rounds, "split_words": split, "widths": widths}

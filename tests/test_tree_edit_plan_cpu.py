"""The host arithmetic of the tree's edit paths (dapol_amd/csrc/tree_edit_plan.inc: the plans of the in-place insert and remove, the
merge of a rebuild, last-wins de-duplication, padding positions) against a SET MODEL of the tree written here: level t of the tree over
leaves X is sorted({x >> t}), a node's position is its rank in its level, and has_pad means the sibling is absent.  The inputs of a plan
(what k_tree_find_paths / k_tree_ins_plan return) come from the model of the old leaf set, the plan is checked against the model of the
new one.  Nothing is recorded.  tests/cpp/tree_edit_plan_host.cpp is a host-only build of the planning, run under ASan + UBSan."""
import bisect
import functools
import json
import os
import random
import subprocess

import pytest
from conftest import ROOT

HEIGHTS = (1, 2, 4, 11, 64)
RANDOM_CASES = 200                     # per height, on top of the directed ones
UNSET = 0xDEADBEEF                     # inspos above a chain's first existing ancestor: the kernel leaves it unwritten


@functools.lru_cache(maxsize=None)
def _exe():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "tree_edit_plan_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "dapol_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "tree_edit_plan_host.cpp"), "-o", exe], check=True)
    return exe


def _plans(lines):
    r = subprocess.run([_exe()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def _words(*lists):
    return " ".join(str(x) for l in lists for x in l)


# ------------------------------------------------------------------------------------------------ the model
def levels_of(X, H):
    return [sorted({x >> t for x in X}) for t in range(H + 1)]


def rank(level, y):
    i = bisect.bisect_left(level, y)
    assert i < len(level) and level[i] == y
    return i


def draw_leaves(rng, H, n):
    """n distinct leaves below 2^H: uniform where the tree is small, otherwise clustered (neighbours, shared subtrees) around a few
    bases, the two ends of the index range among them."""
    U = 1 << H
    n = min(n, U)
    if U <= 4096:
        return set(rng.sample(range(U), n))
    bases = [rng.randrange(U) for _ in range(3)] + [0, U - 1]
    out = set()
    while len(out) < n:
        b = rng.choice(bases)
        out.add(rng.choice((b ^ rng.randrange(1 << rng.randrange(1, 10)), rng.randrange(U))))
    return out


# ------------------------------------------------------------------------------------------------ remove
def remove_line(H, X, R):
    old = levels_of(X, H)
    oldset = [set(l) for l in old]
    R = sorted(R)
    pos = [rank(old[t], x >> t) for x in R for t in range(H + 1)]
    hp = [int(t < H and ((x >> t) ^ 1) not in oldset[t]) for x in R for t in range(H + 1)]
    return "remove %d %d %s" % (H, len(R), _words(R, pos, hp))


def check_remove(H, X, R, P):
    assert R and R < X
    old, new = levels_of(X, H), levels_of(X - R, H)
    oldset, newset = [set(l) for l in old], [set(l) for l in new]
    S1 = H + 1
    assert P["ok"] == 1
    want_dead = [[i for i, y in enumerate(old[t]) if y not in newset[t]] for t in range(S1)]
    assert P["dead"] == want_dead
    assert P["D"] == min(t for t in range(S1) if not want_dead[t])
    assert P["merge"][0] == []
    for t in range(1, S1):
        parents, children = P["merge"][t][0::2], P["merge"][t][1::2]
        assert len(parents) == len(children)
        assert parents == sorted({rank(new[t], x >> t) for x in R if (x >> t) in newset[t]})       # ascending, each once
        for p, c in zip(parents, children):
            assert c < len(new[t - 1]) and new[t - 1][c] >> 1 == new[t][p]
    want_pads = sorted((t, rank(new[t], y)) for t in range(H) for y in new[t] if (y ^ 1) in oldset[t] and (y ^ 1) not in newset[t])
    assert sorted(zip(P["pad_lvl"], P["pad_pos"])) == want_pads
    # the flattened upload: 8 words for the pad seed | dead lists | pad positions | merge pairs
    flat, dead_off, merge_off = P["flat"], P["dead_off"], P["merge_off"]
    assert flat[:8] == [0] * 8 and dead_off[0] == 8 and len(dead_off) == S1 + 1 and len(merge_off) == S1 + 1
    for t in range(S1):
        assert flat[dead_off[t]:dead_off[t + 1]] == P["dead"][t]
        assert flat[merge_off[t]:merge_off[t + 1]] == P["merge"][t]
    assert P["pad_off"] == dead_off[S1] and merge_off[0] == P["pad_off"] + len(P["pad_pos"]) and merge_off[S1] == len(flat)
    assert flat[P["pad_off"]:merge_off[0]] == P["pad_pos"]


def directed_removes(H, rng):
    U = 1 << H
    if H == 1:
        return [({0, 1}, {0}), ({0, 1}, {1})]
    if H == 2:
        return [({0, 1, 2}, {0, 1}), ({0, 1, 2}, {0}), ({0, 1, 2}, {1}), ({0, 1, 2}, {2}), ({0, 2}, {0}), ({0, 2}, {2}), ({0, 1, 2, 3}, {0, 1, 2}),
                ({0, 1, 2, 3}, {1, 2}), ({1, 2, 3}, {1, 3})]
    cases = []
    for a in sorted({0, U - 4, rng.randrange(U) // 4 * 4}):
        far = (a + U // 2) % U                                      # a leaf in the other half of the tree
        blk = {a, a + 1, a + 2, a + 3}
        cases += [({a, far}, {a}), ({a, far}, {far}),                                     # one leaf; a long dead chain
                  ({a, a + 1, far}, {a, a + 1}),                                          # a sibling pair, both children touched, the parent dies
                  ({a, a + 1, far}, {a}), ({a, a + 1, far}, {a + 1}),                     # left / right chain top at the leaves
                  ({a, a + 2, far}, {a}), ({a, a + 2, far}, {a + 2}),                     # the sibling is padding: the parent dies; tops one level up
                  ({a, a + 1, a + 2, far}, {a, a + 1}), ({a, a + 1, a + 2, far}, {a + 2}),
                  (blk | {far}, set(blk)),                                                # a whole aligned subtree
                  (blk | {far}, {a, a + 1, a + 2, far}), (blk | {far}, {a + 1, a + 2}),   # all but one leaf; one of each pair
                  (blk | {far, far ^ 1}, {a, a + 3, far})]
    n = 12 if H == 4 else 600
    X = draw_leaves(rng, H, n) | {U - 1}
    for k in (1, 5, 64, len(X) - 1):
        cases.append((X, set(rng.sample(sorted(X), min(k, len(X) - 1)))))
    return cases


def random_removes(H, rng):
    cases = []
    while len(cases) < RANDOM_CASES:
        X = draw_leaves(rng, H, rng.randrange(2, 41))
        if H == 64 and rng.randrange(2):
            X.add((1 << 64) - 1)
        if len(X) < 2:
            continue
        cases.append((X, set(rng.sample(sorted(X), rng.randrange(1, len(X))))))
    return cases


@pytest.mark.parametrize("H", HEIGHTS)
def test_remove_plan_matches_the_set_model(H):
    rng = random.Random(1000 + H)
    cases = directed_removes(H, rng) + random_removes(H, rng)
    plans = _plans([remove_line(H, X, R) for X, R in cases])
    for (X, R), P in zip(cases, plans):
        check_remove(H, X, R, P)


# ------------------------------------------------------------------------------------------------ insert
def insert_inputs(H, X, N):
    """m / inspos as k_tree_ins_plan defines them, or None when two new chains share a node (the caller rebuilds then)."""
    old = levels_of(X, H)
    m, ins = [], []
    for x in sorted(N):
        row = [UNSET] * (H + 1)
        for t in range(H + 1):
            row[t] = bisect.bisect_left(old[t], x >> t)
            if row[t] < len(old[t]) and old[t][row[t]] == x >> t:
                m.append(t)
                break
        ins += row
    chains = [(t, x >> t) for x, mj in zip(sorted(N), m) for t in range(mj)]
    return None if len(set(chains)) != len(chains) else (m, ins)


def check_insert(H, X, N, m, P):
    assert N and not (N & X)
    old, new = levels_of(X, H), levels_of(X | N, H)
    oldset = [set(l) for l in old]
    S1, max_m = H + 1, max(m)
    assert P["max_m"] == max_m
    for j, x in enumerate(sorted(N)):
        assert 1 <= m[j] <= H
        for t in range(m[j] + 1):                                  # t < m: the chain's new nodes; t = m: the existing ancestor
            assert P["newpos"][j * S1 + t] == rank(new[t], x >> t)
    off = P["lvl_off"]
    assert len(off) == max_m + 2 and off[0] == 0 and off[-1] == len(P["lvl_flat"])
    for t in range(max_m + 1):
        assert P["lvl_flat"][off[t]:off[t + 1]] == [bisect.bisect_left(old[t], y) for y in new[t] if y not in oldset[t]]
    assert new[max_m:] == old[max_m:]                              # (no level from max_m upwards gains a node)


def directed_inserts(H, rng):
    U = 1 << H
    if H == 1:
        return [({0}, {1}), ({1}, {0})]
    cases = [({0}, {U - 1}), ({U - 1}, {0}),                        # a new leaf directly under the root of a one-sided tree: m = H
             ({U - 1}, {0, U - 2}), ({0}, {1, U - 1}),              # a chain that is new at level 1 left / right of an existing ancestor there
             (set(range(U // 2)) if H <= 4 else draw_leaves(rng, H - 1, 30), {U - 1 - rng.randrange(U // 2)})]
    if H >= 3:
        for a in sorted({0, U - 8}):
            X = {a + 3, a + 7} | ({(a + U // 2) % U} if H > 3 else set())
            cases += [(X, {a, a + 2}), (X, {a + 2, a + 4}), (X, {a, a + 2, a + 4}), (X, {a + 2}), (X, {a + 6})]
    X = draw_leaves(rng, H, {2: 2, 4: 12}.get(H, 600)) - {U - 1}
    free = sorted(set(range(U)) - X if H <= 11 else {y ^ 1 for y in X} - X)
    cases += [(X, {U - 1})] + [(X, {x}) for x in rng.sample(free, min(3, len(free)))]
    return cases


def random_inserts(H, rng):
    """Batches whose chains share a node are discarded HERE, before counting: every case returned is planned and checked."""
    U = 1 << H
    cases = []
    while len(cases) < RANDOM_CASES:
        X = draw_leaves(rng, H, rng.randrange(1, 41))
        near = {(x ^ rng.randrange(1 << rng.randrange(1, min(H, 10) + 1))) % U for x in X for _ in range(2)} | draw_leaves(rng, H, 4)
        N = set(rng.sample(sorted(near), min(len(near), rng.randrange(1, 7)))) - X
        if H == 64 and rng.randrange(2) and (U - 1) not in X:
            N.add(U - 1)
        if N and insert_inputs(H, X, N) is not None:
            cases.append((X, N))
    return cases


@pytest.mark.parametrize("H", HEIGHTS)
def test_insert_plan_matches_the_set_model(H):
    rng = random.Random(2000 + H)
    cases = directed_inserts(H, rng) + random_inserts(H, rng)
    inputs = [insert_inputs(H, X, N) for X, N in cases]
    assert all(i is not None for i in inputs), "a directed case has chains that share a node"
    plans = _plans(["insert %d %d %s" % (H, len(N), _words(m, ins)) for (X, N), (m, ins) in zip(cases, inputs)])
    for (X, N), (m, _), P in zip(cases, inputs, plans):
        check_insert(H, X, N, m, P)
    assert len(plans) >= RANDOM_CASES + 2


# ---------------------------------------------------------------- merge_leaf_edits / sorted_last_wins / padding_positions
def _blinding(v):
    return [(v + j) & 0xFF for j in range(32)]


def test_merge_and_last_wins_match_a_dict():
    rng = random.Random(3000)
    cases, lines = [], []
    for H in HEIGHTS:
        for _ in range(40):
            old = sorted(draw_leaves(rng, H, rng.randrange(1, 30)) | ({(1 << H) - 1} if rng.randrange(2) else set()))
            ov = [1000 + i for i in range(len(old))]
            removing = rng.randrange(3) == 0
            pool = old if removing else old + sorted(draw_leaves(rng, H, 8))
            idx = [rng.choice(pool) for _ in range(rng.randrange(1, 12))]            # duplicates on purpose: the last edit of an index wins
            ev = [5000 + u for u in range(len(idx))]
            cases.append((old, ov, idx, None if removing else ev))
            lines.append("merge %d %s %d %s %d %s" % (len(old), _words(old, ov), len(idx), _words(idx), int(removing), "" if removing else _words(ev)))
            lines.append("slw %d %s" % (len(idx), _words(idx)))
    plans = _plans(lines)
    for (old, ov, idx, ev), merged, slw in zip(cases, plans[0::2], plans[1::2]):
        d = dict(zip(old, ov))
        last = {}
        for u, x in enumerate(idx):
            last[x] = u
            if ev is None:
                d.pop(x, None)
            else:
                d[x] = ev[u]
        assert slw["keep"] == [last[x] for x in sorted(last)]
        assert merged["idx"] == sorted(d) and merged["v"] == [d[x] for x in sorted(d)]
        assert merged["r"] == [b for x in sorted(d) for b in _blinding(d[x])]


def test_padding_positions_are_the_missing_siblings_in_tape_order():
    rng = random.Random(4000)
    cases = [(H, sorted(X)) for H in HEIGHTS for X in
             [{0}, {(1 << H) - 1}, {0, (1 << H) - 1}] + [draw_leaves(rng, H, rng.randrange(1, 41)) | {(1 << H) - 1} for _ in range(20)]]
    cases.append((11, sorted(draw_leaves(rng, 11, 600))))
    plans = _plans(["pad %d %d %s" % (H, len(X), _words(X)) for H, X in cases])
    for (H, X), P in zip(cases, plans):
        lv = levels_of(X, H)
        want = sorted((t, y ^ 1) for t in range(H) for y in lv[t] if (y ^ 1) not in set(lv[t]))        # level bottom-up, index ascending
        assert P["count"] == P["again"] == len(want)
        assert list(zip(P["level"], P["index"])) == want

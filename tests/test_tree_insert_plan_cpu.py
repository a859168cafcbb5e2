"""plan_insert_general (dapol_amd/csrc/tree_edit_plan.inc), the host arithmetic of dapol_tree_insert's general in-place path, against a
SET MODEL of the tree written here: level t of the tree over leaves X is sorted({x >> t}), a node's position is its rank in its level,
and has_pad means the sibling is absent.  The plan's inputs (what k_tree_ins_plan<false> returns) come from the model of the old leaf
set; every output is checked against the model of the new one.  Nothing is recorded.  tests/cpp/tree_insert_plan_host.cpp is a
host-only build of the planning, run under ASan + UBSan."""
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
NONE, PAD_SLOT = 0xFFFFFFFF, 0x80000000


@functools.lru_cache(maxsize=None)
def _exe():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "tree_insert_plan_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "dapol_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "tree_insert_plan_host.cpp"), "-o", exe], check=True)
    return exe


def _plans(lines):
    r = subprocess.run([_exe()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


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


def plan_line(H, X, N):
    """What k_tree_ins_plan<false> returns: m = the first level at which the leaf's ancestor exists, and the lower bound of x >> t in the
    OLD level t for every t."""
    old = levels_of(X, H)
    xs = sorted(N)
    m, pos = [], []
    for x in xs:
        row = [bisect.bisect_left(old[t], x >> t) for t in range(H + 1)]
        m.append(next(t for t in range(H + 1) if row[t] < len(old[t]) and old[t][row[t]] == x >> t))
        pos += row
    return "%d %d %s" % (H, len(xs), " ".join(map(str, xs + m + pos))), sum(m)


def check_plan(H, X, N, P):
    assert X and N and not (N & X)
    old, new = levels_of(X, H), levels_of(X | N, H)
    oldset, newset = [set(l) for l in old], [set(l) for l in new]
    fresh = levels_of(N, H)                                        # the new nodes and the existing ancestors of the new leaves
    S1 = H + 1
    # the levels' gains, as k_tree_relayout reads them: an existing node moves up by the number of gains <= its position
    assert P["gain"] == [[bisect.bisect_left(old[t], y) for y in new[t] if y not in oldset[t]] for t in range(S1)]
    assert P["D"] == min(t for t in range(S1) if not P["gain"][t])
    assert new[P["D"]:] == old[P["D"]:]
    for t in range(S1):
        for i, y in enumerate(old[t]):
            assert rank(new[t], y) == i + bisect.bisect_right(P["gain"][t], i)
    # the new nodes: level by level, index ascending
    want = [(t, y) for t in range(S1) for y in new[t] if y not in oldset[t]]
    assert list(zip(P["n_lvl"], P["n_idx"])) == want
    tops = set()
    for i, (t, y) in enumerate(want):
        assert t < H
        assert P["n_pos"][i] == rank(new[t], y)
        assert P["n_parent"][i] == rank(new[t + 1], y >> 1)
        assert P["n_has_pad"][i] == int((y ^ 1) not in newset[t])
        if (y >> 1) in oldset[t + 1]:                              # a top: its sibling is an existing real node next to it
            assert (y ^ 1) in oldset[t] and P["n_sib"][i] == rank(new[t], y ^ 1) and abs(P["n_sib"][i] - P["n_pos"][i]) == 1
            tops.add((t, P["n_sib"][i]))
        else:
            assert P["n_sib"][i] == NONE
    # the existing nodes whose has_pad changes are exactly the tops' siblings (they lose it)
    assert tops == {(t, rank(new[t], y)) for t in range(H) for y in old[t] if ((y ^ 1) not in oldset[t]) != ((y ^ 1) not in newset[t])}
    assert P["leaf_pos"] == [rank(new[0], x) for x in sorted(N)]
    pads = [(t, P["n_pos"][i]) for i, (t, y) in enumerate(want) if P["n_has_pad"][i]]
    assert list(zip(P["pad_lvl"], P["pad_pos"])) == pads
    assert P["max_fresh"] == max(len(f) for f in fresh)
    # the merges: every fresh node above the leaves once, ascending, with its first fresh child and where the other child comes from
    assert P["merge"][0] == []
    for t in range(1, S1):
        e = P["merge"][t]
        assert len(e) == 5 * len(fresh[t])
        for q, y in enumerate(fresh[t]):
            p, c, slot_p, slot_c, other = e[5 * q:5 * q + 5]
            kids = [z for z in (2 * y, 2 * y + 1) if z in set(fresh[t - 1])]
            assert kids and p == rank(new[t], y) and slot_p == q
            assert c == rank(new[t - 1], kids[0]) and slot_c == rank(fresh[t - 1], kids[0])
            sib = kids[0] ^ 1
            if len(kids) == 2:
                assert other == rank(fresh[t - 1], sib)
            elif sib not in newset[t - 1] and kids[0] not in oldset[t - 1]:      # the padding node this call makes
                assert other & PAD_SLOT and other != NONE and pads[other & ~PAD_SLOT] == (t - 1, c)
            else:                                                  # an untouched real node, or a padding record that was there before
                assert other == NONE and (sib in oldset[t - 1] or kids[0] in oldset[t - 1])
    # the flattened upload
    flat, go, mo = P["flat"], P["gain_off"], P["merge_off"]
    assert flat[:8] == [0] * 8 and go[0] == 8 and len(go) == S1 + 1 and len(mo) == S1 + 1 and mo[S1] == len(flat)
    for t in range(S1):
        assert flat[go[t]:go[t + 1]] == P["gain"][t] and flat[mo[t]:mo[t + 1]] == P["merge"][t]
    parts = [P["n_lvl"], P["n_pos"], P["n_parent"], P["n_sib"], [i & 0xFFFFFFFF for i in P["n_idx"]], [i >> 32 for i in P["n_idx"]],
             P["leaf_pos"], P["pad_lvl"], P["pad_pos"]]
    assert P["offs"][0] == go[S1]
    for o, part, end in zip(P["offs"], parts, P["offs"][1:] + [mo[0]]):
        assert flat[o:o + len(part)] == part and o + len(part) == end


def directed(H, rng):
    U = 1 << H
    if H == 1:
        return [({0}, {1}), ({1}, {0})]
    if H == 2:
        return [({0}, {1}), ({0}, {2, 3}), ({3}, {0, 1}), ({0}, {1, 2, 3}), ({1}, {0, 3}), ({2}, {3}), ({3}, {0}), ({0}, {3}), ({0, 3}, {1, 2})]
    cases = []
    for a in sorted({0, U - 8, rng.randrange(U) // 8 * 8}):
        far = (a + U // 2) % U
        blk = {a + i for i in range(8)}
        cases += [({far}, {a, a + 1}), ({far, a + 4}, {a, a + 1}),                  # a sibling pair: under the empty half / beside a cousin
                  ({far}, set(blk)),                                                # a full new subtree of 8
                  ({a, far}, {a + 1}), ({a + 1, far}, {a}),                         # a new leaf beside an existing leaf (m = 1)
                  ({far}, {a}),                                                     # a new leaf in the empty half under the root (m = H)
                  ({a + 3, far}, blk - {a + 3}),                                    # a subtree around an existing leaf
                  ({far, far ^ 1}, blk | {far ^ 2, far ^ 7}),                       # a subtree plus leaves elsewhere
                  ({a + 2}, blk - {a + 2} | {far})]                                 # k larger than the old set
    cases += [({U // 2}, {0, U - 1}), ({0}, {U - 1}), ({U - 1}, {0}), ({1, U - 2}, {0, U - 1})]     # index 0 and index 2^H - 1
    X = draw_leaves(rng, H, 12 if H == 4 else 600)
    for _ in range(3):                                                              # a subtree plus scattered leaves
        base = rng.randrange(U) // 8 * 8
        N = ({base + i for i in range(8)} | draw_leaves(rng, H, 3 if H == 4 else 20)) - X
        if N:
            cases.append((X, N))
    small = set(rng.sample(sorted(X), 3))
    cases.append((small, X - small))                                                # k larger than the old set
    return cases


def random_clustered(H, rng):
    U = 1 << H
    cases = []
    while len(cases) < RANDOM_CASES:
        X = draw_leaves(rng, H, rng.randrange(1, 41))
        near = {(x ^ rng.randrange(1 << rng.randrange(1, min(H, 10) + 1))) % U for x in X for _ in range(3)} | draw_leaves(rng, H, 4)
        N = set(rng.sample(sorted(near), min(len(near), rng.randrange(1, 25)))) - X
        if H == 64 and rng.randrange(2) and (U - 1) not in X:
            N.add(U - 1)
        if N:
            cases.append((X, N))
    return cases


@pytest.mark.parametrize("H", HEIGHTS)
def test_general_insert_plan_matches_the_set_model(H):
    rng = random.Random(5000 + H)
    cases = directed(H, rng) + random_clustered(H, rng)
    lines = [plan_line(H, X, N) for X, N in cases]
    plans = _plans([line for line, _ in lines])
    shared = 0
    for (X, N), (_, chain_nodes), P in zip(cases, lines, plans):
        check_plan(H, X, N, P)
        shared += len(P["n_idx"]) < chain_nodes                    # fewer new nodes than the chains' lengths add up to
    assert len(plans) >= RANDOM_CASES + 2 and (shared >= 20 or H == 1)         # chains that share nodes are what this plan is for

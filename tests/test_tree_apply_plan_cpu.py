"""plan_apply (dapol_amd/csrc/tree_edit_plan.inc), the host arithmetic of dapol_tree_apply's in-place path, against a SET MODEL of the
tree written here: level t of the tree over leaves X is sorted({x >> t}), a node's position is its rank in its level, and has_pad
means the sibling is absent.  The plan's inputs (what k_tree_apply_plan returns) come from the model of the old leaf set; every output
is checked against the models of the old and the new one.  Nothing is recorded.  tests/cpp/tree_apply_plan_host.cpp is a host-only
build of the planning, run under ASan + UBSan.

(One directed shape is read loosely: a node of level 5 is born or dies only with the chain below it, so no batch changes level 5 and
leaves level 0's lists empty.  The case here keeps level 0's SIZE -- one leaf goes, one comes -- while level 5 loses a node, and
replacements alone change no level.)"""
import bisect
import functools
import itertools
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
    exe = os.path.join(out, "tree_apply_plan_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "dapol_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "tree_apply_plan_host.cpp"), "-o", exe], check=True)
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


def plan_line(H, X, R, N):
    """What k_tree_apply_plan returns for the sorted union of the removals R and the puts N: the lower bound of x >> t in the OLD
    level t, whether that node exists, and its has_pad."""
    old = levels_of(X, H)
    oldset = [set(l) for l in old]
    xs = sorted(R | N)
    lb, fl = [], []
    for x in xs:
        for t in range(H + 1):
            y = x >> t
            lb.append(bisect.bisect_left(old[t], y))
            fl.append(0 if y not in oldset[t] else 3 if t < H and (y ^ 1) not in oldset[t] else 1)
    return "%d %d %s" % (H, len(xs), " ".join(map(str, xs + [int(x in N) for x in xs] + lb + fl)))


def check_plan(H, X, R, N, P):
    assert R <= X and not (R & N)
    Y = (X - R) | N
    assert Y and P["ok"] == 1
    S1 = H + 1
    old, new, touched = levels_of(X, H), levels_of(Y, H), levels_of(R | N, H)
    oldset, newset, tset = [set(l) for l in old], [set(l) for l in new], [set(l) for l in touched]
    alive = [[y for y in touched[t] if y in newset[t]] for t in range(S1)]
    # every node that goes or comes is a touched one; the lists are what k_tree_relayout reads
    assert P["dead"] == [[i for i, y in enumerate(old[t]) if y not in newset[t]] for t in range(S1)]
    assert P["born"] == [[bisect.bisect_left(old[t], y) for y in new[t] if y not in oldset[t]] for t in range(S1)]
    for t in range(S1):
        assert all(y in tset[t] for y in set(old[t]) ^ set(new[t]))
        for i, y in enumerate(old[t]):                                              # a survivor moves as the kernel moves it
            if y in newset[t]:
                assert rank(new[t], y) == i + bisect.bisect_right(P["born"][t], i) - bisect.bisect_right(P["dead"][t], i)
    changed = [t for t in range(S1) if P["dead"][t] or P["born"][t]]
    assert P["D"] == (max(changed) + 1 if changed else 0) and P["D"] <= H
    # structure: every alive touched node below the root, and every untouched node whose has_pad changes
    has_pad = lambda sets, t, y: (y ^ 1) not in sets[t]
    want = []
    for t in range(H):
        for pos, y in enumerate(new[t]):
            born = y not in oldset[t]
            if y in tset[t]:
                want.append((t, pos, rank(new[t + 1], y >> 1) if born else NONE, int(born) | 2 * has_pad(newset, t, y), y))
            else:
                assert not born
                if has_pad(oldset, t, y) != has_pad(newset, t, y):
                    want.append((t, pos, NONE, 2 * has_pad(newset, t, y), y))
    assert list(zip(P["s_lvl"], P["s_pos"], P["s_parent"], P["s_flag"], P["s_idx"])) == want
    puts = sorted(N)
    assert P["put_pos"] == [rank(new[0], x) for x in puts] and P["put_new"] == [int(x not in X) for x in puts]
    # padding nodes: wherever has_pad holds afterwards and the old tree did not hold that position's record -- nothing else is made
    pads = [(t, pos) for t in range(H) for pos, y in enumerate(new[t])
            if has_pad(newset, t, y) and not (y in oldset[t] and has_pad(oldset, t, y))]
    assert list(zip(P["pad_lvl"], P["pad_pos"])) == pads
    assert P["max_slots"] == max(len(a) for a in alive)
    # merges: every alive touched node above the leaves once, ascending, with both children and their kinds
    assert P["merge"][0] == []
    for t in range(1, S1):
        e = P["merge"][t]
        assert len(e) == 5 * len(alive[t])
        for q, y in enumerate(alive[t]):
            p, c, slot_p, slot_c, other = e[5 * q:5 * q + 5]
            assert p == rank(new[t], y) and slot_p == q
            kids = [z for z in (2 * y, 2 * y + 1) if z in newset[t - 1]]
            made = [z for z in kids if z in tset[t - 1]]
            anchor = made[0] if made else kids[0]
            assert c == rank(new[t - 1], anchor)
            assert slot_c == (rank(alive[t - 1], anchor) if made else NONE)
            sib = anchor ^ 1
            if sib in newset[t - 1]:
                assert other == (rank(alive[t - 1], sib) if sib in tset[t - 1] else NONE)
            elif anchor in oldset[t - 1] and sib not in oldset[t - 1]:              # the old padding record, still right
                assert other == NONE
            else:
                assert other == PAD_SLOT | pads.index((t - 1, c))
            if not made:                                                            # S beside a dead node: decoded, beside its new padding node
                assert anchor in oldset[t - 1] and sib in oldset[t - 1] and sib not in newset[t - 1] and other & PAD_SLOT and other != NONE
    # the flattened upload
    flat, do, bo, mo = P["flat"], P["dead_off"], P["born_off"], P["merge_off"]
    assert flat[:8] == [0] * 8 and do[0] == 8 and bo[0] == do[S1] and len(do) == len(bo) == len(mo) == S1 + 1 and mo[S1] == len(flat)
    for t in range(S1):
        assert flat[do[t]:do[t + 1]] == P["dead"][t] and flat[bo[t]:bo[t + 1]] == P["born"][t] and flat[mo[t]:mo[t + 1]] == P["merge"][t]
    parts = [P["s_lvl"], P["s_pos"], P["s_parent"], P["s_flag"], [i & 0xFFFFFFFF for i in P["s_idx"]], [i >> 32 for i in P["s_idx"]],
             P["put_pos"], P["pad_lvl"], P["pad_pos"]]
    assert P["offs"][0] == bo[S1]
    for o, part, end in zip(P["offs"], parts, P["offs"][1:] + [mo[0]]):
        assert flat[o:o + len(part)] == part and o + len(part) == end
    # where the shapes coincide, the special plans give the same positions
    if not N:
        Rm = P["remove"]
        assert Rm["ok"] == 1 and Rm["dead"] == P["dead"]
        assert sorted(zip(Rm["pad_lvl"], Rm["pad_pos"])) == pads
        for t in range(1, S1):
            assert Rm["merge"][t][0::2] == P["merge"][t][0::5]
    else:
        assert "remove" not in P
    if not R and not (N & X):
        G = P["insert"]
        assert G["gain"] == P["born"] and G["leaf_pos"] == P["put_pos"]
        assert list(zip(G["n_lvl"], G["n_pos"], G["n_parent"])) == [(a, b, c) for a, b, c, f, _ in want if f & 1]
        assert list(zip(G["pad_lvl"], G["pad_pos"])) == pads
        for t in range(1, S1):
            assert G["merge"][t] == P["merge"][t]
    else:
        assert "insert" not in P


# ------------------------------------------------------------------------------------------------ the cases: (old leaves, removed, put)
def exhaustive(H):
    """Every old set and every edit of it (heights 1 and 2)."""
    U = 1 << H
    cases = []
    for bits in range(1, 1 << U):
        X = {i for i in range(U) if bits >> i & 1}
        for what in itertools.product(range(3), repeat=U):                         # per index: nothing | remove | put
            R = {i for i in range(U) if what[i] == 1}
            N = {i for i in range(U) if what[i] == 2}
            if R <= X and (R or N) and (X - R) | N:
                cases.append((X, R, N))
    return cases


def directed(H, rng):
    U = 1 << H
    cases = []
    for a in sorted({0, U - 16, rng.randrange(U) // 16 * 16}):
        far = (a + U // 2) % U
        blk = {a + i for i in range(8)}
        cases += [
            ({a, far}, {a}, {a + 1}),                                   # a leaf removed, its absent sibling put: level 0 loses and gains at one lower bound
            ({a + 1, far}, {a + 1}, {a}),
            ({a, a + 1, a + 3, far}, {a, a + 1, a + 3}, {a + 2}),       # a subtree emptied and repopulated: its root survives
            (blk | {far}, blk - {a + 5}, {a + 5}),                          # ... by a replacement
            (blk | {far}, set(blk), {a + 8}),                           # ... while its neighbour is born: a dies, a + 8 comes
            ({a, a + 2, far}, {a}, {a + 3}),                            # a chain top dies beside an S under which a put lands
            ({a, a + 2, far}, {a}, {a + 2}),                            # ... which replaces S's leaf
            ({a, a + 4, far}, {a}, {a + 6}),                            # ... one level up
            ({a, a + 1, a + 2, far}, {a + 2}, {a + 3}),                 # a put takes away the has_pad a removal would have given
            ({a, a + 1, a + 2, a + 3, far}, {a + 2, a + 3}, set()),     # ... and without the put it is given
            ({a, a + 1, far}, {a}, set()), ({a, a + 4, far}, {a + 4}, set()), (blk | {far}, set(blk), set()),               # only removals
            ({a, far}, set(), {a + 1}), ({far}, set(), set(blk)), ({a + 3, far}, set(), blk - {a + 3}),                     # only new puts
            ({a, a + 1, far}, set(), {a}), (blk | {far}, set(), set(blk)), (blk | {far}, set(), {a, a + 7, far}),           # only replacements
            (blk | {far, far ^ 1}, blk | {far}, set()),                 # every leaf but one removed
            (blk | {far}, blk | {far}, {a + 9}),                        # every old leaf removed, one new put
            (blk | {far}, blk - {a + 1}, {far ^ 3, a + 1}),
        ]
    cases += [({0, U - 1}, {0}, {1}), ({0, U - 1}, {U - 1}, {U - 2}), ({0, U - 1}, {0, U - 1}, {1, U - 2}), ({1, U - 2}, {1}, {0, U - 1}),
              ({0, 1, U - 2, U - 1}, {0, U - 1}, {1, U - 2}), ({U // 2}, {U // 2}, {0, U - 1})]                  # the two ends of the index range
    if H >= 7:
        a = rng.randrange(U >> 6) << 6                                  # a is alone under its level-5 node, b joins a populated one:
        b = a ^ 32                                                      # level 0 keeps its size, level 5 loses a node
        cases.append(({a, b, b + 1}, {a}, {b + 2}))
    X = draw_leaves(rng, H, 12 if H == 4 else 600)
    for _ in range(3):                                                  # a block removed beside a block added, plus scattered edits
        base = rng.randrange(U) // 16 * 16
        Xb = X | {base + i for i in range(8)}
        R = {base + i for i in range(8)} | set(rng.sample(sorted(X), 3))
        N = ({base + 8 + i for i in range(8)} | draw_leaves(rng, H, 3 if H == 4 else 20) | set(rng.sample(sorted(X), 3))) - R
        cases.append((Xb, R, N))
    keep = set(rng.sample(sorted(X), 1))
    cases.append((X, X - keep, set()))                                  # every leaf but one removed, of a larger tree
    return cases


def random_mixed(H, rng):
    U = 1 << H
    cases = []
    while len(cases) < RANDOM_CASES:
        X = draw_leaves(rng, H, rng.randrange(1, 41))
        near = {(x ^ rng.randrange(1 << rng.randrange(1, min(H, 10) + 1))) % U for x in X for _ in range(3)} | draw_leaves(rng, H, 4)
        R = set(rng.sample(sorted(X), rng.randrange(0, len(X) + 1))) if rng.randrange(4) else set()
        N = set(rng.sample(sorted(near | X), min(len(near | X), rng.randrange(0, 25)))) - R
        if rng.randrange(8) == 0:
            N &= X                                                      # replacements only
        if H == 64 and rng.randrange(2) and (U - 1) not in R:
            N.add(U - 1)
        if (R or N) and (X - R) | N:
            cases.append((X, R, N))
    return cases


@pytest.mark.parametrize("H", HEIGHTS)
def test_apply_plan_matches_the_set_model(H):
    rng = random.Random(7000 + H)
    cases = (exhaustive(H) if H <= 2 else directed(H, rng)) + random_mixed(H, rng)
    plans = _plans([plan_line(H, X, R, N) for X, R, N in cases])
    kinds = set()
    both = survivors = 0
    for (X, R, N), P in zip(cases, plans):
        check_plan(H, X, R, N, P)
        kinds.add((bool(R), bool(N - X), bool(N & X)))
        both += any(d and b for d, b in zip(P["dead"], P["born"]))               # a level that loses and gains at once
        survivors += any(slot_c == NONE for m in P["merge"] for slot_c in m[3::5])     # a merge whose anchor is decoded
    assert len(plans) >= RANDOM_CASES + 2
    assert both >= 1 and survivors >= 1
    if H >= 4:                                                                  # every mix of the three kinds of edit, and the shapes this plan is for
        assert len(kinds) == 7 and both >= 20 and survivors >= 20


def test_apply_plan_directed_shapes():
    """The directed shapes at height 11, by what they must show."""
    H, a, far = 11, 512, 1536
    def plan(X, R, N):
        P = _plans([plan_line(H, X, R, N)])[0]
        check_plan(H, X, R, N, P)
        return P
    P = plan({a + 1, far}, {a + 1}, {a})                                    # loses and gains at the same lower bound; nothing above changes
    assert P["dead"][0] == [0] and P["born"][0] == [0] and P["D"] == 1 and P["pad_pos"] == [0]
    P = plan({a, a + 1, a + 3, far}, {a, a + 1, a + 3}, {a + 2})        # the subtree's root survives: level 2 neither loses nor gains
    assert P["D"] == 2 and P["dead"][1] == [0] and P["born"][1] == [] and P["dead"][2] == [] and P["born"][2] == []
    P = plan({a, a + 2, far}, {a}, {a + 3})                             # the chain top (a >> 1) dies, S = (a + 2) >> 1 is touched: no decoded anchor
    assert P["dead"][1] == [0] and all(s != NONE for s in P["merge"][2][3::5])
    P = plan({a, a + 1, a + 2, far}, {a + 2}, {a + 3})                  # (a + 2) >> 1 survives: its sibling gains no has_pad
    assert P["dead"][1] == [] and [f for l, f in zip(P["s_lvl"], P["s_flag"]) if l == 1] == [0]
    P = plan({a, a + 1, a + 2, a + 3, far}, {a + 2, a + 3}, set())      # without the put S = a >> 1 gains it, decoded beside its new padding node
    assert P["merge"][2][3] == NONE and P["merge"][2][4] & PAD_SLOT
    P = plan({a, a + 1, far}, set(), {a, far})                          # replacements only: no level changes, nothing is made but the paths
    assert P["D"] == 0 and P["pad_pos"] == [] and not any(f & 1 for f in P["s_flag"])
    P = plan({a, a + 32, a + 33}, {a}, {a + 34})                        # level 0 keeps its size, level 5 loses a node
    assert len(P["dead"][0]) == len(P["born"][0]) == 1 and P["dead"][5] == [0] and P["born"][5] == [] and P["D"] == 6

"""dapol_reprove_plan / dapol_reprove_entities_shared without a device: declared, exported and bound; the planner is host-only index
arithmetic and is checked against a brute force written here, which recomputes every sibling's subtree as a SET of (leaf, version)
pairs before and after the edit and compares the two -- no prefix arithmetic shared with the library.  The same cases are replayed
through tests/cpp/reprove_plan_asan.cpp, a host-only build of dapol_amd/csrc/reprove_plan.inc with its own main, run as a child process
under ASan + UBSan (the index arrays live in heap buffers of exactly their size)."""
import ctypes
import functools
import itertools
import json
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT

from test_abi import declared_symbols
from test_shared_plan_abi import H6_CASES, H6_LEAVES, key_depth, plan_of

ABSENT, SAME, REPLACED, INSERTED, REMOVED = range(5)


def test_reprove_symbols_are_declared_exported_and_bound(hip_lib):
    for s in ("dapol_reprove_plan", "dapol_reprove_entities_shared"):
        assert s in declared_symbols()
        assert hasattr(hip_lib.lib(), s)
        assert s in hip_lib.EXPORTED_SYMBOLS
    assert callable(getattr(hip_lib, "reprove_plan", None))
    assert callable(getattr(hip_lib.Tree, "reprove_entities_shared", None))


def test_reprove_without_a_context_is_an_invalid_argument(hip_lib):
    lib = hip_lib.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    idx, seed, out = np.array([5], np.uint64), np.zeros(32, np.uint8), np.full(4096, 0xAB, np.uint8)
    proved = ctypes.c_uint64(12345)
    assert lib.dapol_reprove_entities_shared(None, None, 1, p(idx), 0, 1, 8, p(seed), None, p(out), p(out), None, None, p(out), ctypes.byref(proved), None) == 8
    assert b"null" in lib.dapol_last_error()
    assert (out == 0xAB).all() and proved.value == 12345


# ------------------------------------------------------------------------------------------------ the brute force
class Case:
    """states: {leaf: SAME | REPLACED | INSERTED | REMOVED}.  `null_has_old`: has_old is passed as NULL (every row counts as having old
    data, the inserted ones too)."""

    def __init__(self, H, states, policy, agg, leaf_first, null_has_old=False):
        self.H, self.policy, self.agg, self.leaf_first, self.null = H, policy, agg, leaf_first, null_has_old
        self.before = {x: 1 for x, st in states.items() if st in (SAME, REPLACED, REMOVED)}
        self.after = {x: (2 if st == REPLACED else 1) for x, st in states.items() if st in (SAME, REPLACED, INSERTED)}
        self.leaves = sorted(self.after)
        self.edited = sorted(x for x, st in states.items() if st in (REPLACED, INSERTED, REMOVED))
        self.has_old = [int(self.null or x in self.before) for x in self.leaves]
        self._sub, self._exp = {}, None

    def line(self):
        has = "0" if self.null else "1 " + " ".join(map(str, self.has_old))
        return "plan %d %d %d %d %d %s %s %d %s" % (self.H, self.leaf_first, self.policy, self.agg, len(self.leaves), " ".join(map(str, self.leaves)), has,
                                                     len(self.edited), " ".join(map(str, self.edited)))

    def subtree(self, which, depth, node):
        """The (leaf, version) pairs below the depth-`depth` node `node`, before (0) or after (1) the edit."""
        if (which, depth) not in self._sub:
            by_node = {}
            for x, ver in (self.before, self.after)[which].items():
                by_node.setdefault(x >> (self.H - depth), set()).add((x, ver))
            self._sub[(which, depth)] = by_node
        return self._sub[(which, depth)].get(node, set())

    def expect(self, pyref):
        if self._exp is None:
            self._exp = self._expect(pyref)
        return self._exp

    def _expect(self, pyref):
        H, plan = self.H, plan_of(pyref, self.policy, self.H, self.agg)
        heads, uniq = [0] * len(plan), [0] * len(plan)
        for s, (start, count, m) in enumerate(plan):
            D = key_depth(start, count, H, self.leaf_first)
            key = lambda x: (x >> (H - D)) if D else 0
            prev_dirty = False
            for e, x in enumerate(self.leaves):
                dirty = not self.has_old[e]
                for i in range(start, start + count):
                    d = H - i if self.leaf_first else i + 1               # depth of sibling i below the root
                    node = (x >> (H - d)) ^ 1
                    dirty = dirty or self.subtree(0, d, node) != self.subtree(1, d, node)
                new_key = e == 0 or key(x) != key(self.leaves[e - 1])
                heads[s] += int(dirty and (new_key or not prev_dirty))
                uniq[s] += int(new_key)
                prev_dirty = dirty
        ms = [m for _, _, m in plan]
        return heads, sum(heads), sum(h * m for h, m in zip(heads, ms)), sum(u * m for u, m in zip(uniq, ms))


def _edit_sets(leaves, H):
    """The directed edit sets of one leaf set: none, everything, the first / the last / a middle leaf replaced, a removal, inserted
    leaves (a sibling of a leaf, one inside a key run, the last index), and a mix."""
    top = (1 << H) - 1
    free = [x for x in (leaves[0] ^ 1, leaves[len(leaves) // 2] ^ 1, top, leaves[-1] ^ 1, (leaves[0] + 2) & top) if x not in leaves and 0 <= x <= top]
    base = {x: SAME for x in leaves}
    out = [dict(base), {x: REPLACED for x in leaves}, {**base, **{leaves[0]: REPLACED}}, {**base, **{leaves[-1]: REPLACED}},
           {**base, **{leaves[len(leaves) // 2]: REPLACED}}]
    if len(leaves) > 1:
        out.append({**base, **{leaves[-1]: REMOVED}})
        out.append({**base, **{leaves[0]: REMOVED, leaves[-1]: REPLACED}})
    for x in free[:3]:
        out.append({**base, **{x: INSERTED}})
    if free and len(leaves) > 2:
        out.append({**base, **{free[0]: INSERTED, leaves[1]: REMOVED, leaves[-1]: REPLACED}})
        out.append({**{x: REMOVED for x in leaves[:-1]}, free[-1]: INSERTED, leaves[-1]: SAME})
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    rng = np.random.default_rng(29)
    for leaf_first in (0, 1):
        # H = 1 and 2: every combination of states of every leaf (at least one leaf left), every aggregation
        for H in (1, 2):
            for states in itertools.product((ABSENT, SAME, REPLACED, INSERTED, REMOVED), repeat=1 << H):
                st = {x: s for x, s in enumerate(states) if s != ABSENT}
                if not any(s in (SAME, REPLACED, INSERTED) for s in st.values()):
                    continue
                for policy in (0, 1):
                    for agg in range(H + 1):
                        out.append(Case(H, st, policy, agg, leaf_first))
                        if H == 1:
                            out.append(Case(H, st, policy, agg, leaf_first, null_has_old=True))
        # H = 6: the leaves of the shared plan's tests, every aggregation (H6_CASES among them)
        assert set(H6_CASES) <= {(p, a) for p in (0, 1) for a in range(7)}
        for st in _edit_sets(H6_LEAVES, 6):
            for policy in (0, 1):
                for agg in range(7):
                    out.append(Case(6, st, policy, agg, leaf_first))
                    out.append(Case(6, st, policy, agg, leaf_first, null_has_old=True))
        # H = 10: 52 random leaves with 0, 1 and 1023 among them; directed and random edits
        leaves = sorted(set(int(x) for x in rng.choice(1 << 10, size=49, replace=False)) | {0, 1, 1023})
        sets = _edit_sets(leaves, 10)
        for n_edit in (1, 5, 20):
            st = {x: SAME for x in leaves}
            for x in rng.choice(1 << 10, size=n_edit, replace=False):
                x = int(x)
                st[x] = (REPLACED if rng.random() < 0.6 else REMOVED) if x in st else INSERTED
            if any(s != REMOVED for s in st.values()):
                sets.append(st)
        for st in sets:
            for policy in (0, 1):
                for agg in range(11):
                    out.append(Case(10, st, policy, agg, leaf_first, null_has_old=bool(agg & 1)))
        # H = 64: no shift by 64, the index 2^64 - 1 as a leaf, as an edit and as an inserted leaf
        top = (1 << 64) - 1
        l64 = [0, 1, 1 << 63, top]
        for st in _edit_sets(l64, 64) + [{0: SAME, 1: SAME, (1 << 63): SAME, top: INSERTED}, {0: SAME, 1: REPLACED, (1 << 63): SAME, top: REMOVED}]:
            for policy, agg in ((0, 0), (0, 2), (0, 64), (1, 24), (1, 63)):
                out.append(Case(64, st, policy, agg, leaf_first))
    return out


def test_cases_cover_the_edit_sets_the_planner_must_get_right():
    cs = cases()
    assert any(not c.edited for c in cs) and any(c.edited == c.leaves and all(c.has_old) for c in cs)           # no edit; every leaf edited
    assert any(c.edited == [c.leaves[0]] for c in cs) and any(c.edited == [c.leaves[-1]] for c in cs)          # the first / the last leaf
    assert any(c.H == 64 and (1 << 64) - 1 in c.edited for c in cs)
    assert any(c.null for c in cs) and any(not c.null and 0 in c.has_old for c in cs)
    assert any(set(c.edited) - set(c.leaves) for c in cs)                                                      # removed leaves


@pytest.mark.parametrize("leaf_first", [0, 1])
def test_reprove_plan_matches_the_brute_force(hip_lib, pyref, leaf_first):
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        for c in cases():
            if c.leaf_first != leaf_first:
                continue
            n_proved, tot, sum_m, sum_m_shared = hip_lib.reprove_plan(c.H, c.leaves, c.edited, c.policy, c.agg, None if c.null else c.has_old)
            heads, want_tot, want_m, want_shared = c.expect(pyref)
            assert [int(x) for x in n_proved] == heads, c.line()
            assert (tot, sum_m, sum_m_shared) == (want_tot, want_m, want_shared), c.line()
            if not c.edited and all(c.has_old):
                assert tot == 0                                                       # no edit: nothing to prove
            n_sub, _, _ = hip_lib.shared_plan(c.H, c.leaves, c.policy, c.agg)
            assert sum_m_shared == sum(int(u) * m for u, (_, _, m) in zip(n_sub, plan_of(pyref, c.policy, c.H, c.agg)))
    finally:
        hip_lib.wire_config_restore(old)


def test_reprove_plan_totals_alone_and_no_leaves(hip_lib, pyref):
    lib = hip_lib.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    idx, ed = np.array(H6_LEAVES, np.uint64), np.array([17], np.uint64)
    tot = ctypes.c_uint64()
    assert lib.dapol_reprove_plan(6, 8, p(idx), None, 1, p(ed), 0, 3, None, ctypes.byref(tot), None, None) == 0      # every output but one NULL
    assert tot.value == Case(6, {**{x: SAME for x in H6_LEAVES}, 17: REPLACED}, 0, 3, 0).expect(pyref)[1]
    n, tot, sm, sh = hip_lib.reprove_plan(6, [], [5], 0, 3)
    assert (list(n), tot, sm, sh) == ([0, 0, 0, 0], 0, 0, 0)


def test_reprove_plan_refuses_bad_indexes_and_plans(hip_lib):
    for H, bad in ((6, [2, 1]), (6, [3, 3]), (6, [1, 64]), (6, [0, 5, 4, 9]), (0, [1])):
        with pytest.raises(hip_lib.DapolError) as e:
            hip_lib.reprove_plan(H, bad, [], 0, 0)
        assert e.value.code == 8, (H, bad)
        with pytest.raises(hip_lib.DapolError) as e:                                   # the edited indexes obey the same rule
            hip_lib.reprove_plan(H, [0], bad, 0, 0)
        assert e.value.code == 8, (H, bad)
    for pol, agg in ((0, 7), (1, 7), (0, -1), (2, 1)):
        with pytest.raises(hip_lib.DapolError) as e:
            hip_lib.reprove_plan(6, H6_LEAVES, [3], pol, agg)
        assert e.value.code == 8
    with pytest.raises(hip_lib.DapolError) as e:
        hip_lib.reprove_plan(65, [0], [], 0, 0)
    assert e.value.code == 1                                                           # DAPOL_ERR_TREE_HEIGHT_TOO_BIG, as dapol_shared_plan
    lib = hip_lib.lib()
    assert lib.dapol_reprove_plan(6, 2, None, None, 0, None, 0, 3, None, None, None, None) == 8
    assert lib.dapol_reprove_plan(6, 0, None, None, 1, None, 0, 3, None, None, None, None) == 8


# ------------------------------------------------------------------------------------------------ the replay under ASan + UBSan
@functools.lru_cache(maxsize=None)
def _exe():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "reprove_plan_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "dapol_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "reprove_plan_asan.cpp"), "-o", exe], check=True)
    return exe


def _replay(lines):
    r = subprocess.run([_exe()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def test_planner_replayed_under_asan_matches_the_brute_force(pyref):
    cs = cases()
    got = _replay([c.line() for c in cs])
    for c, g in zip(cs, got):
        heads, tot, sum_m, shared = c.expect(pyref)
        assert g["ok"] == 1 and g["n_proved"] == heads and (g["total"], g["sum_m"], g["sum_m_shared"]) == (tot, sum_m, shared), c.line()
    bad = _replay(["plan 6 0 2 1 1 5 0 0 ", "plan 6 0 0 7 1 5 0 0 ", "plan 65 0 0 0 1 5 0 0 ", "plan 6 0 0 3 2 5 5 0 0 ", "plan 6 0 0 3 1 64 0 0 ",
                   "plan 6 0 0 3 1 5 0 2 9 8", "plan 6 0 0 3 1 5 0 1 64", "plan 6 0 0 3 0 0 1 7"])
    assert [g["ok"] for g in bad] == [0, 0, 0, -1, -1, -1, -1, 1]


def test_compact_layout_with_empty_groups_and_a_kept_first_row():
    """Where the head rows of each group lie: U = 0 groups take no room, the base of a group is the scan's element BEFORE its first pair
    (row 0 may be kept), and a dirty pair's compact row counts the heads before it inside its group."""
    #        n_groups b   base (heads before each group, then all)   s0        m         pieces
    lines = ["layout 3 5  0 0 4 9   0 1 3   4 2 1   36 34 32", "layout 2 7  0 0 0   0 1   8 1   38 32", "layout 1 1  0 1   0   1   42", "layout 0 3  0"]
    got = _replay(lines)
    assert got[0] == {"U": [0, 4, 5], "party_off": [0, 0, 8], "word_off": [0, 0, 4 * 34 * 4], "base_at": [0, 5, 15], "parties": 13,
                      "words": 4 * 34 * 4 + 5 * 32 * 4, "heads": 9, "row": 5}
    assert got[1]["U"] == [0, 0] and (got[1]["parties"], got[1]["words"], got[1]["heads"]) == (0, 0, 0) and got[1]["base_at"] == [0, 7]
    assert got[2] == {"U": [1], "party_off": [0], "word_off": [0], "base_at": [0], "parties": 1, "words": 42 * 4, "heads": 1, "row": 1}
    assert got[3]["heads"] == 0 and got[3]["U"] == []

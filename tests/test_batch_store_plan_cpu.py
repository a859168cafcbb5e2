"""The index arithmetic of dapol_batch_store (dapol_amd/csrc/batch_store_plan.inc) without a device: batch_store_match against a Python
dictionary of leaf lists (lowest equal old row), batch_store_same_list, and the row and offset tables of the move and of the fetch
against dapol_batches_plan's offsets -- through tests/cpp/batch_store_plan_asan.cpp, a host-only build with its own main that runs as a
child process under ASan + UBSan (every array lives in a heap buffer of exactly its size)."""
import functools
import json
import os
import subprocess

import numpy as np
from conftest import ROOT

TOP = 2**64 - 1


@functools.lru_cache(maxsize=None)
def _exe():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "batch_store_plan_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "dapol_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "batch_store_plan_asan.cpp"), "-o", exe], check=True)
    return exe


def _replay(lines):
    r = subprocess.run([_exe()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def _list(a):
    return "%d %s" % (len(a), " ".join(str(int(x)) for x in a))


def _packed(batches):
    off = [0]
    for b in batches:
        off.append(off[-1] + len(b))
    return off, [x for b in batches for x in b]


def _match_line(old, new):
    return "match " + " ".join(_list(a) for a in _packed(old) + _packed(new))


def _cases():
    rng = np.random.default_rng(29)
    pool = [sorted({int(x) for x in rng.integers(0, 64, size=int(rng.integers(1, 6)))}) for _ in range(60)]
    base = [[1], [5], [1, 5], [1, 5, 9], [20, 21], [20, 21, 22, 23], [5], [1, 5]]
    return {
        "empty old": ([], [[0], [5, TOP]]),
        "empty new": ([[1], [2, 3]], []),
        "both empty": ([], []),
        "identical": (base, [list(b) for b in base]),
        "permutation": (base, base[::-1]),
        "rotation": (base, base[3:] + base[:3]),
        "repeated old lists, the lowest wins": ([[7], [7], [1, 2], [7], [1, 2]], [[1, 2], [7], [7], [7], [3]]),
        "a repeated batch added": (base, base + [base[3]]),
        "prefixes of one another": ([[1], [1, 2], [1, 2, 3], [1, 2, 3, 4]], [[1, 2, 3], [1, 2, 3, 4, 5], [1, 2], [2], [1], [1, 3]]),
        "a prefix only": ([[1, 2, 3]], [[1, 2], [1], [1, 2, 3, 4]]),
        "the top index": ([[TOP], [0, TOP], [TOP - 1, TOP]], [[0, TOP], [TOP], [TOP - 1], [TOP - 1, TOP], [0]]),
        "the top index against zero": ([[0]], [[TOP]]),
        "one batch dropped, two added": (base, base[:2] + [[2]] + base[3:] + [[1, 2, 5]]),
        "random": (pool, [pool[i] for i in rng.permutation(len(pool))[:40]] + [[63, 64]]),
    }


def test_match_against_a_dictionary_of_leaf_lists():
    cases = _cases()
    out = _replay([_match_line(old, new) for old, new in cases.values()])
    for (name, (old, new)), got in zip(cases.items(), out):
        lowest = {}
        for r, b in enumerate(old):
            lowest.setdefault(tuple(b), r)
        want = [lowest.get(tuple(b)) for b in new]
        assert got["src"] == [0 if r is None else r + 1 for r in want], name
        assert got["has_old"] == [int(r is not None) for r in want], name
        assert got["with_old"] == sum(r is not None for r in want), name
        assert got["same"] == int(old == new), name


def test_the_in_place_path_is_taken_for_the_same_list_only():
    """Equal row for row: a permutation, a list with one batch more or less, and equal offsets over other leaves are not the same list."""
    a = [[1, 2], [3], [1, 2]]
    got = _replay([_match_line(a, a), _match_line(a, [a[2], a[1], a[0]]), _match_line(a, [[3], [1, 2], [1, 2]]), _match_line(a, a[:2]), _match_line(a[:2], a),
                   _match_line(a, [[1, 2], [4], [1, 2]]), _match_line(a, [[1], [2, 3], [1, 2]])])
    assert [g["same"] for g in got] == [1, 1, 0, 0, 0, 0, 0]
    assert [g["with_old"] for g in got] == [3, 3, 3, 2, 3, 2, 1]
    assert got[0]["src"] == [1, 2, 1]                               # the second [1, 2] continues the LOWEST equal row


def _plan(hip_lib, batches, cfg):
    policy, agg, n_bits = cfg
    _, so, ro, _ = hip_lib.batches_plan(6, batches, policy, agg, n_bits)
    return [int(x) for x in so], [int(x) for x in ro]


CONFIGS = [(0, 0, 8), (0, 4, 8), (1, 3, 64)]
STORED = [[1], [20, 21], [20, 21, 22, 23], [1, 5, 9, 12, 33], [63], [20, 21], [1, 63]]


def test_fetch_offsets_are_the_plan_of_the_queried_batches(hip_lib):
    queries = [[3, 0, 3, 6, 1, 1, 5], [0], [6, 5, 4, 3, 2, 1, 0], []]
    for cfg in CONFIGS:
        so, ro = _plan(hip_lib, STORED, cfg)
        out = _replay(["fetch %s %s %s" % (_list(so), _list(ro), _list(q)) for q in queries] + ["fetch %s %s %s" % (_list(so), _list(ro), _list([2, len(STORED)]))])
        for q, got in zip(queries, out):
            qso, qro = _plan(hip_lib, [STORED[r] for r in q], cfg)
            assert got["ok"] == 1 and got["q_sib_off"] == qso and got["q_piece_off"] == [x // 16 for x in qro], (cfg, q)
        assert out[-1] == {"ok": 0}                                 # a row number == rows


def _pieces(unit, dst_off, frm, src_off):
    """the definition: destination row d owns [dst_off[d], dst_off[d + 1]) x unit pieces, copies of its source row's from src_off on"""
    want = []
    for d, r in enumerate(frm):
        for t in range((dst_off[d + 1] - dst_off[d]) * unit):
            want.append(0 if r is None else src_off[r] * unit + t + 1)
    return want


def test_move_and_fetch_pieces_against_the_plans_offsets(hip_lib):
    """Every 16-byte piece of the destination, for the move (new list <- continued old rows, the others unwritten) and for the fetch
    (staging <- queried rows), blobs (unit 1) and 32-byte records (unit 2): rows with S = 0 and rows without a source included."""
    new = [[2], STORED[2], [0, 1, 2, 3], STORED[0], STORED[5], [1, 2, 5], STORED[1], STORED[6]]
    frm = [None, 2, None, 0, 1, None, 1, 6]                        # the lowest equal old row
    query = [3, 0, 3, 6, 1, 1, 5]
    lines, want = [], []
    for cfg in CONFIGS:
        old_so, old_ro = _plan(hip_lib, STORED, cfg)
        new_so, new_ro = _plan(hip_lib, new, cfg)
        q_so, q_ro = _plan(hip_lib, [STORED[r] for r in query], cfg)
        for unit, dst, src, rows in ((1, [x // 16 for x in new_ro], [x // 16 for x in old_ro], frm), (2, new_so, old_so, frm),
                                     (1, [x // 16 for x in q_ro], [x // 16 for x in old_ro], query), (2, q_so, old_so, query)):
            for d, r in enumerate(rows):
                assert r is None or dst[d + 1] - dst[d] == src[r + 1] - src[r]          # equal lists have equal sizes
            lines.append("pieces %d %s %s %s" % (unit, _list(dst), _list([0 if r is None else r + 1 for r in rows]), _list(src)))
            want.append(_pieces(unit, dst, rows, src))
    out = _replay(lines)
    for line, w, got in zip(lines, want, out):
        assert got["src"] == w, line
        assert len(w) > 0
    # a height-2 tree with all four leaves in one batch: S = 0, its row owns blob pieces and no record at all
    so, ro = (lambda p: ([int(x) for x in p[1]], [int(x) for x in p[2]]))(hip_lib.batches_plan(2, [[0, 1, 2, 3], [1]], 0, 0, 8))
    assert so[1] == 0 and ro[1] > 0
    got = _replay(["pieces 2 %s %s %s" % (_list(so), _list([1, 2]), _list(so)), "pieces 2 %s %s %s" % (_list([0, so[2], so[2]]), _list([2, 1]), _list(so))])
    assert got[0]["src"] == _pieces(2, so, [0, 1], so) and got[1]["src"] == _pieces(2, [0, so[2], so[2]], [1, 0], so)

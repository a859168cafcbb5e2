"""The index arithmetic of dapol_proof_store (dapol_amd/csrc/store_plan.inc) without a device: store_lower_bound and store_align_host are
checked against Python sets and sorted lists through tests/cpp/store_plan_asan.cpp, a host-only build with its own main that runs as a
child process under ASan + UBSan (the index arrays live in heap buffers of exactly their size); the buffer sizes against the layout of
dapol_prove_entities_shared's outputs."""
import bisect
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
    exe = os.path.join(out, "store_plan_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "dapol_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "store_plan_asan.cpp"), "-o", exe], check=True)
    return exe


def _replay(lines):
    r = subprocess.run([_exe()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def _align_line(old, new):
    return "align %d %s %d %s" % (len(old), " ".join(map(str, old)), len(new), " ".join(map(str, new)))


def _cases():
    rng = np.random.default_rng(11)
    big = sorted({int(x) for x in rng.integers(0, 2**63, size=300, dtype=np.uint64)} | {0, TOP})
    cases = {
        "empty old": ([], [0, 5, TOP]),
        "empty new": ([1, 2, 3], []),
        "both empty": ([], []),
        "identical": ([0, 1, 7, 8, 200, TOP], [0, 1, 7, 8, 200, TOP]),
        "disjoint": ([1, 3, 5, 7], [0, 2, 4, 6, 8]),
        "disjoint, all below": ([100, 200], [1, 2, 3]),
        "disjoint, all above": ([1, 2, 3], [100, 200]),
        "interleaved": ([0, 2, 3, 9, 10, 50], [1, 2, 4, 9, 11, 50, 51]),
        "the ends": ([0, TOP], [0, 1, TOP - 1, TOP]),
        "only the top": ([TOP], [TOP]),
        "only zero against the top": ([0], [TOP]),
        "single old row, hit": ([42], [41, 42, 43]),
        "single new row, hit": ([1, 42, 99], [42]),
        "single new row, miss": ([1, 42, 99], [43]),
        "superset": ([2, 4, 6], [1, 2, 3, 4, 5, 6, 7]),
        "subset": ([1, 2, 3, 4, 5, 6, 7], [2, 4, 6]),
        "same size, one leaf swapped": ([1, 2, 3, 4], [1, 2, 3, 5]),
        "random, every second": (big, big[::2]),
        "random, shifted": (big[:150], big[100:]),
    }
    return cases


def test_alignment_and_lower_bound_against_python_sets():
    cases = _cases()
    out = _replay([_align_line(old, new) for old, new in cases.values()])
    for (name, (old, new)), got in zip(cases.items(), out):
        have = set(old)
        row = {x: i for i, x in enumerate(old)}
        assert got["has_old"] == [int(x in have) for x in new], name
        assert got["src"] == [row[x] + 1 if x in have else 0 for x in new], name
        assert got["lower"] == [bisect.bisect_left(old, x) for x in new], name
        assert got["with_old"] == len(have & set(new)), name
        assert got["same"] == int(have == set(new)), name


def test_same_leaf_set_is_exact():
    """The in-place path is taken exactly when the sets are equal: equal sizes alone, or full overlap alone, do not suffice."""
    got = _replay([_align_line([1, 2, 3], [1, 2, 3]), _align_line([1, 2, 3], [1, 2, 4]), _align_line([1, 2, 3], [1, 2]), _align_line([1, 2], [1, 2, 3])])
    assert [g["same"] for g in got] == [1, 0, 0, 0]
    assert [g["with_old"] for g in got] == [3, 2, 2, 2]


def test_buffer_sizes_are_the_shared_calls_layout():
    """[rows][H][32] commitments, [rows][H][hash bytes] hashes, [rows][entity bytes] blobs, 8 bytes of index per row; two sibling sets
    stay resident, a row-moving refresh adds a second blob buffer and the compare buffer; 2^22 rows of 24 KB do not wrap 32 bits."""
    cases = [(8, 6, 32, 2752, 172, 8), (40, 8, 64, 5376, 336, 16), (0, 32, 32, 24576, 1536, 8), (1 << 22, 32, 32, 24576, 1536, 8), (1, 0, 32, 672, 42, 8)]
    out = _replay(["bytes %d %d %d %d %d %d" % c for c in cases])
    for (rows, H, hb, es, ep, hw), got in zip(cases, out):
        assert got["idx"] == rows * 8 and got["path_C"] == rows * H * 32 and got["path_H"] == rows * H * hb and got["range"] == rows * es
        assert got["resident"] == rows * (8 + 2 * H * (32 + hb) + es)
        assert got["move_transient"] == rows * (es + H * 32)
        assert got["row_pieces"] == ep + 2 * H + H * hw // 4 == (es + H * 32 + H * hb) // 16
    assert out[3]["range"] == 103079215104 > 2**32 * 16

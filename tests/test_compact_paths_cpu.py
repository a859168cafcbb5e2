"""The index arithmetic of compact Merkle paths (dapol_amd/csrc/compact_paths_plan.inc: the layout, ref, expand / compress, the link
words that the kernels walk, every refusal) against a brute-force set model written here, at heights 1, 2, 6, 33 and 64 under both
sibling orders and both hash widths.  tests/cpp/compact_paths_host.cpp is a host-only build of that file with its own main, run
directly under ASan + UBSan: every buffer lives on the heap with exactly its size."""
import functools
import json
import os
import random
import subprocess

from conftest import ROOT

JOIN, RIGHT, INDEX = 0x80000000, 0x40000000, 0x3FFFFFFF
BAD_HEIGHT, BAD_INDEX, BAD_HASH, BAD_RECORDS, BAD_WINDOW, BAD_CAP = 1, 2, 3, 4, 5, 6


@functools.lru_cache(maxsize=None)
def _exe():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "compact_paths_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "dapol_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "compact_paths_host.cpp"), "-o", exe], check=True)
    return exe


def _replay(lines):
    r = subprocess.run([_exe()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def line(H, leaf_first, hb, idx, first, count, d_records=0, d_cap=0):
    return "%d %d %d %d %s %d %d %d %d" % (H, leaf_first, hb, len(idx), " ".join(str(x) for x in idx), first, count, d_records, d_cap)


def pattern(i):
    return (i * 131 + (i >> 8) * 7 + (i >> 16) + 3) & 0xFF


def model(H, idx):
    """The definition, as sets: (keys[d] sorted for d = 0 .. H, depth_off [H + 2], ref[d - 1][e], link words)."""
    key = lambda x, d: 0 if d == 0 else x >> (H - d)
    keys = [sorted({key(x, d) for x in idx}) for d in range(H + 1)]
    if not idx:
        keys[0] = [0]
    depth_off = [0, 0]
    for d in range(1, H + 1):
        depth_off.append(depth_off[-1] + len(keys[d]))
    pos = [{k: i for i, k in enumerate(keys[d])} for d in range(H + 1)]
    ref = [[pos[d][key(x, d)] for x in idx] for d in range(1, H + 1)]
    head = [{} for _ in range(H + 1)]                     # head[d][key] = the first row with that key
    for d in range(H + 1):
        for e, x in enumerate(idx):
            head[d].setdefault(key(x, d), e)
    link = []
    for d in range(1, H + 1):
        for k in keys[d]:
            w = pos[d - 1][k >> 1 if d > 1 else 0]
            w |= RIGHT if k & 1 else 0
            w |= JOIN if head[d][k] != head[d - 1][k >> 1 if d > 1 else 0] else 0
            link.append(w)
    return keys, depth_off, ref, link


def check(H, leaf_first, hb, idx, first, count, got):
    b = len(idx)
    keys, depth_off, ref, link = model(H, idx)
    n = depth_off[-1]
    assert got["rc"] == 0 and got["n_records"] == n and got["depth_off"] == depth_off
    assert got["ref"] == [r for row in ref for r in row] and got["link"] == link and got["links_fit"] == 1
    # every record is consumed by exactly one merge: the joins are one per row but the first
    assert sum(1 for w in link if w & JOIN) == max(b - 1, 0)
    assert got["compress_rc"] == 0 and got["round_trip"] == 1 and got["round_trip_poisoned"] == 1
    if first + count > b:
        assert got["expand_rc"] == BAD_WINDOW and got["expand_untouched"] == 1
        return
    assert got["expand_rc"] == 0
    wantC, wantH = bytearray(), bytearray()
    for e in range(first, first + count):
        for slot in range(H):
            d = H - slot if leaf_first else slot + 1
            rec = depth_off[d] + ref[d - 1][e]
            wantC += bytes(pattern(i) for i in range(rec * 32, rec * 32 + 32))
            wantH += bytes(pattern(i + 7777) for i in range(rec * hb, rec * hb + hb))
    assert got["expand_C"] == wantC.hex() and got["expand_H"] == wantH.hex()


def random_indexes(rng, H, b):
    """Strictly increasing, clustered: neighbours that share long prefixes, and the ends of the range."""
    top = (1 << H) - 1
    out = set()
    while len(out) < min(b, top + 1):
        base = rng.choice((0, top, rng.randrange(top + 1)))
        out.add(min(top, max(0, base ^ rng.randrange(1 << rng.randrange(0, min(H, 8) + 1)))))
    return sorted(out)


def test_layout_links_expand_and_compress_match_a_set_model():
    rng = random.Random(53)
    cases = []
    for H in (1, 2, 6, 33, 64):
        top = (1 << H) - 1
        sets = [[], [0], [top], sorted({0, top})]
        sets += [random_indexes(rng, H, b) for b in ((1, 2) if H == 1 else (2, 3, 4) if H == 2 else (5, 9, 20, 40))]
        if H == 6:
            sets.append(list(range(64)))                     # the full set: every sibling is another row's ancestor
        if H >= 6:
            sets.append(sorted({0, 1, top - 1, top, top >> 1, (top >> 1) + 1}))
        for idx in sets:
            for leaf_first in (0, 1):
                for hb in (32, 64):
                    n = len(idx)
                    for first, count in {(0, n), (n - 1 if n else 0, 1 if n else 0), (min(3, n), min(2, n - min(3, n))), (0, 0), (n, 0), (n, 1)}:
                        if n > 20 and (first, count) != (0, n) and hb == 64:
                            continue
                        cases.append((H, leaf_first, hb, idx, first, count))
    got = _replay([line(*c) for c in cases])
    for c, g in zip(cases, got):
        check(*c, g)
    assert any(c[0] == 64 and c[3] and c[3][-1] == 2**64 - 1 for c in cases)
    assert any(g["expand_rc"] == BAD_WINDOW for g in got) and any(len(g.get("expand_C", "")) == 64 * c[0] for c, g in zip(cases, got))     # count = 1 cuts


def test_every_refusal_writes_nothing():
    # indexes: not increasing, equal, out of range; heights 0 and 65
    bad = [line(6, 0, 32, [5, 4], 0, 0), line(6, 0, 32, [4, 4], 0, 0), line(6, 0, 32, [3, 64], 0, 0), line(1, 1, 64, [0, 2], 0, 0),
           line(33, 0, 32, [1, 1 << 33], 0, 0), line(0, 0, 32, [0], 0, 0), line(65, 0, 32, [0], 0, 0)]
    got = _replay(bad)
    assert [g["rc"] for g in got] == [BAD_INDEX] * 5 + [BAD_HEIGHT] * 2
    assert all(g["untouched"] == 1 and g["expand_rc"] == g["rc"] and g["compress_rc"] == g["rc"] for g in got)
    idx = [0, 1, 2, 3, 16, 17, 40, 63]
    got = _replay([line(6, 0, 48, idx, 0, 8), line(6, 1, 0, idx, 0, 8), line(6, 0, 32, idx, 0, 8, d_records=1), line(6, 0, 32, idx, 0, 8, d_records=-1),
                   line(6, 0, 64, idx, 7, 2), line(6, 0, 32, idx, 9, 0), line(6, 0, 32, idx, 0, 8, d_cap=-1), line(6, 1, 64, idx, 0, 8, d_cap=-5),
                   line(6, 1, 64, idx, 0, 8, d_cap=3)])
    assert [g["expand_rc"] for g in got] == [BAD_HASH, BAD_HASH, BAD_RECORDS, BAD_RECORDS, BAD_WINDOW, BAD_WINDOW, 0, 0, 0]
    assert all(g["expand_untouched"] == 1 for g in got[:6])
    assert [g["compress_rc"] for g in got] == [BAD_HASH, BAD_HASH, 0, 0, 0, 0, BAD_CAP, BAD_CAP, 0]
    assert all(g["compress_untouched"] == 1 for g in got if g["compress_rc"]) and all(g["round_trip"] == 1 for g in got if not g["compress_rc"])


def test_the_ratios_of_the_three_leaf_sets():
    """b = 2^12 leaves at H = 24, from the plan: per-entity records b H against distinct records.  Consecutive leaves from 0 share every
    depth down to 12 and halve from there: 12 + (2 + 4 + .. + 4096) records.  Leaves strided by 2^12 differ in their top 12 bits: 2^d
    records at depth d <= 12 and 4096 at each of the 12 depths below.  No set of 4096 leaves has more distinct keys at any depth than
    that, so a random set has at most as many records; it has fewer, because b random keys fill about 2^d (1 - (1 - 2^-d)^b) of the 2^d
    slots of depth d (2589 of 4096 at depth 12), and the sum of that over the depths is what the plan must give to within sampling noise."""
    b, H = 1 << 12, 24
    rng = random.Random(5)
    rand = sorted(rng.sample(range(1 << H), b))
    sets = {"random": rand, "strided": [i << 12 for i in range(b)], "consecutive": list(range(b))}
    got = dict(zip(sets, _replay([line(H, 0, 32, idx, 0, 0) for idx in sets.values()])))
    for name, idx in sets.items():
        keys = model(H, idx)[0]
        assert got[name]["n_records"] == sum(len(k) for k in keys[1:]), name
    assert got["consecutive"]["n_records"] == 12 + (2 << 12) - 2 == 8202
    assert got["strided"]["n_records"] == (2 << 12) - 2 + 12 * 4096 == 57342
    expect = sum(2.0**d * (1.0 - (1.0 - 2.0**-d)**b) for d in range(1, H + 1))
    assert abs(got["random"]["n_records"] - expect) < 0.02 * expect and got["random"]["n_records"] < 57342
    ratio = {k: b * H / g["n_records"] for k, g in got.items()}
    assert 11.9 < ratio["consecutive"] < 12.0 and 1.71 < ratio["strided"] < 1.72 < ratio["random"] < 1.95

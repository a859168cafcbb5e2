"""The grouping of a policy's sub-proofs (dapol_amd/csrc/policy_plan.inc: group_policy_plan) that prove_policy_device and
verify_policy_device (host_policy.inc, host_verify.inc) share: both policies, heights 0..64, every aggregation factor, grouping on and
off, against a restatement in a few lines of Python, and the structure a grouping must have whatever the rule.  And where the groups of
a call live (policy_layout, same file): offsets and sizes for b in {1, 3}, n_bits in {8, 64}, compact and re-used buffers, against
running sums written out here.  tests/cpp/policy_group_host.cpp is the host-only driver (built with ASan + UBSan)."""
import functools
import os
import subprocess

from conftest import ROOT


def _np2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def _plan(policy, height, agg):
    """[(start, count, m)] in blob order: the aggregated proofs, then one individual proof per sibling beyond agg"""
    if policy == 0:
        plan = [(0, agg, _np2(agg))]
    else:
        plan, base, pos = [], _np2(agg), 0
        while pos < agg:
            if agg & base:
                plan.append((pos, base, base))
                pos += base
            base >>= 1
    return plan + [(i, 1, 1) for i in range(agg, height)]


def _groups(plan, group):
    """a sub-proof joins the group before it if both are full (count == m), equally large and adjacent"""
    out = []
    for start, count, m in plan:
        if group and out and out[-1][2] == m == count == out[-1][1] and out[-1][0] + out[-1][3] * m == start:
            out[-1][3] += 1
        else:
            out.append([start, count, m, 1])
    return [tuple(g) for g in out]


@functools.lru_cache(maxsize=None)
def _driver_lines():
    """the driver's output, built and run once: (grouping lines, layout lines)"""
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "policy_group_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "dapol_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "policy_group_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr
    lines = r.stdout.splitlines()
    return [l for l in lines if not l.startswith("L ")], [l[2:] for l in lines if l.startswith("L ")]


def test_grouping_matches_its_restatement_and_tiles_the_plan():
    lines, _ = _driver_lines()
    assert len(lines) == 2 * 2 * sum(h + 1 for h in range(65))
    seen = set()
    for line in lines:
        head, totals, body = line.split("|")
        policy, height, agg, group = map(int, head.split())
        sum_proofs, sum_parties, max_k, max_parties = map(int, totals.split())
        groups = [tuple(map(int, t.split(","))) for t in body.split()]
        seen.add((policy, height, agg, group))
        plan = _plan(policy, height, agg)
        assert groups == _groups(plan, group), line
        # the groups tile the plan in order: expanding every group gives the plan back
        expanded = []
        for start, count, m, k in groups:
            assert k >= 1
            if k > 1:
                assert count == m, line                  # only full sub-proofs are grouped, and their starts are contiguous
            expanded += [(start + j * m, count, m) for j in range(k)]
        assert expanded == plan, line
        assert sum_proofs == sum(k for _, _, _, k in groups) == len(plan)
        assert sum_parties == sum(m * k for _, _, m, k in groups) == sum(m for _, _, m in plan)
        assert max_k == max([1] + [k for _, _, _, k in groups])             # (1: what an empty plan reports)
        assert max_parties == max([1] + [m * k for _, _, m, k in groups])
        if not group:
            assert all(k == 1 for _, _, _, k in groups), line
    assert len(seen) == len(lines)
    # grouping does something: the individual proofs of a height-32 path are one group (with the one-party part of an odd split before them)
    assert _groups(_plan(0, 32, 0), True) == [(0, 0, 1, 1), (0, 1, 1, 32)]
    assert _groups(_plan(1, 32, 25), True) == [(0, 16, 16, 1), (16, 8, 8, 1), (24, 1, 1, 8)]


def _proof_words(n_bits, m):
    """32 bytes x (9 + 2 lg(n_bits m)) of one aggregated proof, in words"""
    return 8 * (9 + 2 * ((n_bits * m).bit_length() - 1))


def test_layout_is_the_running_sums_of_the_groups():
    _, lines = _driver_lines()
    assert len(lines) == 2 * sum(h + 1 for h in range(65)) * 2 * 2 * 2
    seen = set()
    for line in lines:
        head, totals, body = line.split("|")
        policy, height, agg, b, n_bits, reuse = map(int, head.split())
        entity_words, entity_bytes, parties, words, proofs = map(int, totals.split())
        got = [tuple(map(int, t.split(","))) for t in body.split()]
        seen.add((policy, height, agg, b, n_bits, reuse))
        groups = _groups(_plan(policy, height, agg), True)
        assert len(got) == len(groups), line
        word_off = slot = party = gathered = verdict = 0
        sizes = []
        for (start, count, m, k), g in zip(groups, got):
            pw = _proof_words(n_bits, m)
            want = (pw, word_off, slot, party, gathered, verdict) if not reuse else (pw, word_off, slot, 0, 0, 0)
            assert g == want, (line, g, want)
            word_off += k * pw                           # inside an entity's blob
            slot += k * m * (2 * n_bits + 4)             # inside an entity's draws
            party += k * m * b                           # inside the call's gathered arrays
            gathered += k * pw * b
            verdict += k * b
            sizes.append((k * m * b, k * pw * b, k * b))
        assert entity_words == word_off and 4 * entity_words == entity_bytes, line      # the groups' words are dapol_entity_proof_size / 4
        if reuse:
            assert (parties, words, proofs) == tuple(max([0] + [s[i] for s in sizes]) for i in range(3)), line      # (0: an empty plan)
        else:
            assert (parties, words, proofs) == (party, gathered, verdict), line
    assert len(seen) == len(lines)

"""The collision rule of dapol_tree_derive_leaves (dapol_amd/csrc/kernels_leaf.h: k_leaf_claim_first_onto / k_leaf_settle_onto) as a model
on the CPU: tests/test_leaf_collision_model.py's rounds with a set of slots that are taken before the batch starts -- the current
leaves of the tree the batch joins.  In the sequential loop (src/dapol/mod.rs:408-441) `taken` simply starts non-empty.  In the
claim / settle rounds a pre-taken slot reads as owned by entity -1: earlier than every entity of the batch, holding its slot for good,
and never entered into the owner table (the kernel looks it up in the tree's sorted leaf array instead).  Claim: the fixed point is
still the sequential result, including WHICH entity fails, and no entity draws a candidate the sequential loop would not have drawn
for it."""
import random


def sequential(chains, max_tries, pre):
    taken, out = set(pre), []
    for e, ch in enumerate(chains):
        for k in range(max_tries):
            if ch[k] not in taken:
                taken.add(ch[k])
                out.append(ch[k])
                break
        else:
            return out, e                                  # FailedToMapIndex at entity e of the batch
    return out, None


def parallel(chains, max_tries, pre, rng, deepest=None):
    """The rounds.  deepest (a list, optional) receives the number of candidates each entity ever drew."""
    n = len(chains)
    owner = {}                                             # slot -> earliest entity of the BATCH that has claimed it (never a pre-taken slot)
    NO_POS = object()                                      # the entity holds nothing: its candidate is a pre-taken slot

    def claim(slot, e):                                    # atomicMin; returns the previous owner (None: free)
        assert slot not in pre                             # the slot table never sees a current leaf
        prev = owner.get(slot)
        if prev is None or prev > e:
            owner[slot] = e
        return prev

    tries, pos = [1] * n, [None] * n
    for e in rng.sample(range(n), n):
        if chains[e][0] in pre:
            pos[e] = NO_POS
        else:
            claim(chains[e][0], e)
            pos[e] = chains[e][0]
    failed = None
    moved = True
    while moved:
        moved = False
        for e in rng.sample(range(n), n):
            if tries[e] > max_tries:                       # parked: out of candidates
                continue
            if pos[e] is not NO_POS and owner[pos[e]] == e:
                continue
            moved = True
            while True:
                if tries[e] >= max_tries:
                    failed = e if failed is None else min(failed, e)
                    tries[e] = max_tries + 1
                    break
                tries[e] += 1
                s = chains[e][tries[e] - 1]
                if s in pre:                               # owned by entity -1: draw the next one
                    pos[e] = NO_POS
                    continue
                prev = claim(s, e)
                pos[e] = s
                if prev is None or prev > e:
                    break
    if deepest is not None:
        deepest[:] = [min(t, max_tries) for t in tries]
    if failed is not None:
        return None, failed
    return [pos[e] for e in range(n)], None


def test_fixed_point_with_pre_taken_slots_is_the_sequential_result():
    rng = random.Random(4242)
    hopeless = failing = 0
    for case in range(4000):
        n = rng.randint(1, 40)
        slots = rng.randint(max(1, n // 2), 3 * n)
        if case % 10 == 0:
            pre = set(range(slots))                        # hopeless because of the pre-taken slots alone: entity 0 fails
        else:
            pre = set(rng.sample(range(slots), rng.randint(1, slots)))
        max_tries = rng.randint(1, 8)
        chains = [[rng.randrange(slots) for _ in range(max_tries)] for _ in range(n)]
        want, want_fail = sequential(chains, max_tries, pre)
        got, got_fail = parallel(chains, max_tries, pre, rng)
        assert got_fail == want_fail, (case, chains, pre)
        if want_fail is None:
            assert got == want, (case, chains, pre)
            assert not set(got) & pre and len(set(got)) == n
        else:
            failing += 1
        if len(pre) == slots:
            hopeless += 1
            assert want_fail == 0
    assert hopeless >= 400 and failing > hopeless          # both kinds of failure were produced


def test_an_empty_pre_taken_set_is_the_plain_rule():
    rng = random.Random(5)
    for case in range(300):
        n, slots, max_tries = rng.randint(1, 30), rng.randint(10, 60), rng.randint(1, 6)
        chains = [[rng.randrange(slots) for _ in range(max_tries)] for _ in range(n)]
        want, want_fail = sequential(chains, max_tries, set())
        assert parallel(chains, max_tries, set(), rng) == (want if want_fail is None else None, want_fail)


def test_an_entity_only_ever_walks_a_prefix_of_its_sequential_walk():
    """A move is forced by an EARLIER entity that holds the slot for good -- an entity of the batch, or entity -1 for a pre-taken slot --
    so no entity draws more candidates than the sequential loop draws for it."""
    rng = random.Random(77)
    checked = 0
    for case in range(800):
        n, slots, max_tries = 30, 60, 10
        pre = set(rng.sample(range(slots), rng.randint(1, 25)))
        chains = [[rng.randrange(slots) for _ in range(max_tries)] for _ in range(n)]
        want, fail = sequential(chains, max_tries, pre)
        if fail is not None:
            continue
        taken, depth = set(pre), []
        for e in range(n):                                 # how deep the sequential loop went for each entity
            k = next(k for k in range(max_tries) if chains[e][k] not in taken)
            taken.add(chains[e][k])
            depth.append(k + 1)
        deepest = []
        got, _ = parallel(chains, max_tries, pre, rng, deepest)
        assert got == want
        assert all(d <= w for d, w in zip(deepest, depth)), (case, deepest, depth)
        assert deepest == depth                            # (and it ends exactly there)
        checked += 1
    assert checked >= 400

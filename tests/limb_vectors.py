"""Crafted operands that sit on the limb bounds of dapol_amd/csrc/fe.h (nine signed 29-bit limbs), points and scalars for the
group and scalar headers, and a plain big-integer model of the column sums to check them with.  Shared by the host-path tests
(tests/test_limb_bounds_cpu.py) and the device-path tests (tests/test_gpu_device_arith.py).

A field element that went through fe_frombytes has limbs in [0, 2^29); random points keep every column of a product near its
mean.  The header's contract allows far more (f LOOSE = 3 x TIGHT of either sign, g TIGHT) and these inputs go there: raw limbs,
nothing beyond the stated preconditions.  Everything is deterministic (seeded) so that both paths see the same cases."""
import random

import edge_scalars as E

P = 2**255 - 19
L = E.L
NL = 9
M29, M23 = 2**29 - 1, 2**23 - 1
TIGHT = 2**29 + 2**17                # fe.h: |limb| of a tight value
LOOSE = 3 * TIGHT                    # fe.h: |limb| of a loose value (f of fe_mul)
CARRY_STATED = 2**31 // 20           # the bound fe_carry's comment used to state; still a family of its own
CARRY_FULL = 2**31 - 5               # fe_carry: nothing overflows for |limb| < 2^31 - 4
I64 = 2**63


# ------------------------------------------------------------------------------------------------ representation
def value(limbs):
    """The integer a limb vector stands for: sum v_i 2^(29 i)."""
    return sum(int(v) << (29 * i) for i, v in enumerate(limbs))


def limbs_of(x):
    """Canonical-width limbs of 0 <= x < 2^255 (limbs 0..7 of 29 bits, limb 8 of 23)."""
    assert 0 <= x < 2**255
    return [(x >> (29 * i)) & M29 for i in range(NL)]


def words_of(x):
    """The eight little-endian words fe_towords must give for the value x."""
    x %= P
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


# ------------------------------------------------------------------------------------------------ model of fe.h
def _wrap(hi_col):
    """What a high column adds below: (unsigned low half) * 1216 one column down-wrapped, (signed high half) * 9728 the next."""
    return (hi_col & 0xFFFFFFFF) * 1216, (hi_col >> 32) * 9728


def _chain(raw):
    """raw[k] = the plain sum of products of column k (0..16) -> the chained columns c0..c8 as fe_mul / fe_sq hold them
    (carry of the column below, the wrapped high columns), every one checked to fit int64."""
    c = [0] * 9
    for k in range(9):
        lo = _wrap(raw[k + 9])[0] if k + 9 <= 16 else 0
        hi = _wrap(raw[k + 8])[1] if 9 <= k + 8 <= 16 else 0
        c[k] = (c[k - 1] >> 29 if k else 0) + raw[k] + lo + hi
    assert all(-I64 <= x < I64 for x in list(raw) + c), "a column left int64: the input is outside fe.h's precondition"
    return c


def raw_columns_mul(f, g):
    return [sum(f[i] * g[k - i] for i in range(NL) if 0 <= k - i < NL) for k in range(17)]


def columns_mul(f, g):
    """(raw columns 0..16, chained columns c0..c8) of fe_mul(h, f, g)."""
    raw = raw_columns_mul(f, g)
    return raw, _chain(raw)


def columns_sq(f):
    return columns_mul(f, f)


def limbs_from_cols(c):
    """fe_limbs_from_cols."""
    t = (c[8] >> 23) * 19 + (c[0] & M29)
    h = [x & M29 for x in c[:8]] + [c[8] & M23]
    h[0] = t & M29
    h[1] = (c[1] & M29) + (t >> 29)
    return h


def model_mul(f, g):
    return limbs_from_cols(columns_mul(f, g)[1])


def model_sq(f):
    return limbs_from_cols(columns_sq(f)[1])


def model_carry(f):
    """fe_carry."""
    h = [int(v) for v in f]
    for i in range(8):
        h[i + 1] += h[i] >> 29
        h[i] &= M29
    h[0] += 19 * (h[8] >> 23)
    h[8] &= M23
    h[1] += h[0] >> 29
    h[0] &= M29
    return h


# ------------------------------------------------------------------------------------------------ the output contract
def _limb1_excess(product_lo, product_hi, terms):
    """Interval arithmetic over the columns: product_lo / product_hi bound one product, terms[k] = (n_lo, n_hi) says how many
    products of column k can be negative / positive.  Returns (lo, hi) of t >> 29 in fe_limbs_from_cols, i.e. how far limb 1
    can leave [0, 2^29)."""
    lo = [terms[k][0] * product_lo for k in range(17)]
    hi = [terms[k][1] * product_hi for k in range(17)]
    clo = chi = 0
    for k in range(9):
        wl_lo, wl_hi = (0, 1216 * (2**32 - 1)) if k + 9 <= 16 else (0, 0)
        wh_lo, wh_hi = ((lo[k + 8] >> 32) * 9728, (hi[k + 8] >> 32) * 9728) if 9 <= k + 8 <= 16 else (0, 0)
        clo, chi = (clo >> 29 if k else 0) + lo[k] + wl_lo + wh_lo, (chi >> 29 if k else 0) + hi[k] + wl_hi + wh_hi
        assert -I64 <= clo and chi < I64
    return ((clo >> 23) * 19) >> 29, ((chi >> 23) * 19 + M29) >> 29


def _count(k):
    return len([i for i in range(NL) if 0 <= k - i < NL])


def limb1_excess_mul():
    """fe_mul with f LOOSE and g TIGHT: every product lies in [-3 T^2, 3 T^2], column k has _count(k) of them."""
    return _limb1_excess(-LOOSE * TIGHT, LOOSE * TIGHT, [(_count(k), _count(k)) for k in range(17)])


def limb1_excess_sq():
    """fe_sq with f TIGHT: f_i f_j (i != j) appears twice and lies in [-T^2, T^2]; f_i^2 once, in [0, T^2]."""
    return _limb1_excess(-TIGHT * TIGHT, TIGHT * TIGHT, [(_count(k) - (k % 2 == 0), _count(k)) for k in range(17)])


# The numbers the derivation gives (fe.h states them; a change of the bounds above must change them knowingly).
MUL_LIMB1 = (-32849, 32849)
SQ_LIMB1 = (-9733, 10950)
CARRY_LIMB1 = (-1, 1)


def contract_ok(h, excess):
    """The output contract of fe.h: limbs 0, 2..7 in [0, 2^29), limb 8 in [0, 2^23), limb 1 in [lo, 2^29 - 1 + hi]."""
    return (all(0 <= h[i] <= M29 for i in (0, 2, 3, 4, 5, 6, 7)) and 0 <= h[8] <= M23 and excess[0] <= h[1] <= M29 + excess[1])


# ------------------------------------------------------------------------------------------------ field pairs
def _signs(n):
    return [[1 if (m >> i) & 1 else -1 for i in range(n)] for m in range(1 << n)]


def column_extreme_pairs():
    """[(k, sigma, f, g)]: every product of column k is sigma * 3 T^2 -- the column at its bound, either sign -- under EVERY sign
    pattern of the limbs that take part; the limbs that do not take part are zero, so the other columns hold only the
    cross-correlation of the pattern."""
    out = []
    for k in range(17):
        idx = [i for i in range(NL) if 0 <= k - i < NL]
        for sigma in (1, -1):
            for s in _signs(len(idx)):
                f, g = [0] * NL, [0] * NL
                for si, i in zip(s, idx):
                    f[i] = si * LOOSE
                    g[k - i] = si * sigma * TIGHT
                out.append((k, sigma, f, g))
    return out


def high_split_pairs():
    """[(k, zone, f, g)] for k = 9..16: column k NEGATIVE with its low 32 bits exactly 0, just above 0, just below 2^32 and
    2^32 - 1 -- the unsigned (low half) * 1216 and signed (high half) * 9728 split of a negative column, at both ends of the
    low half.  One product f_i g_(k-i) per case, for the lowest and the highest i of the column."""
    rnd = random.Random(29)
    out = []
    for k in range(9, 17):
        for i in sorted({k - 8, 8}):
            for zone, target in (("zero", 0), ("low", 3), ("high", 2**32 - 5), ("ones", 2**32 - 1)):
                while True:
                    a = -rnd.randrange(2 * TIGHT, LOOSE + 1) | 1                     # odd, loose, negative
                    if target == 0:
                        a, b = -(rnd.randrange(2**13, 3 * 2**13) << 16), rnd.randrange(1, 2**13) << 16
                    else:
                        b = target * pow(a, -1, 2**32) % 2**32
                    if 0 < b <= TIGHT and a * b < -2**58:
                        break
                f, g = [0] * NL, [0] * NL
                f[i], g[k - i] = a, b
                assert (a * b) & 0xFFFFFFFF == target
                out.append((k, zone, f, g))
    return out


def limb1_pairs(sign, n=64):
    """sign = -1: c8 >> 23 as negative as it gets while the low 29 bits of c1 are exactly 0, so limb 1 of the result is t >> 29
    itself, NEGATIVE.  sign = +1: the mirror image, c8 >> 23 large with the low 29 bits of c1 all ones: limb 1 above 2^29.
    Eight of column 8's nine products are at sign * 3 T^2 (g8 = 0 keeps f1 out of the high columns, so c1 is linear in f1 and f1
    is solved for: it stays loose, at least 2/3 of the bound)."""
    rnd = random.Random(31 + sign)
    out = []
    while len(out) < n:
        s = [rnd.choice((1, -1)) for _ in range(NL)]
        f = [s[i] * LOOSE for i in range(NL)]
        g = [sign * s[8 - j] * TIGHT for j in range(NL)]
        g[8] = 0
        g[0] = sign * s[8] * (TIGHT - 1)                                             # odd: invertible mod 2^29
        f[1] = 0
        k0 = columns_mul(f, g)[1][1]                                                 # c1 without f1 g0
        r = (((0 if sign < 0 else M29) - k0) * pow(g[0], -1, 2**29)) % 2**29         # f1 = r mod 2^29
        want = sign * g[7]                                                           # the sign that gives f1 g7 the sign of `sign`
        cands = [r + m * 2**29 for m in range(-7, 7)]
        cands = [c for c in cands if abs(c) <= LOOSE and c * want > 0]
        f[1] = max(cands, key=abs)
        assert abs(f[1]) >= 2 * TIGHT and columns_mul(f, g)[1][1] & M29 == (0 if sign < 0 else M29)
        out.append((f, g))
    return out


def special_limbs():
    """{name: limbs}: zero, one, p - 1 and p itself as canonical-width limbs (p is a legal, reduced limb vector of value 0)."""
    p = [2**29 - 19] + [M29] * 7 + [M23]
    return {"zero": [0] * NL, "one": [1] + [0] * 8, "p-1": [2**29 - 20] + [M29] * 7 + [M23], "p": p}


def _rand_limbs(rnd, bound, kind):
    if kind == "uniform":
        return [rnd.randint(-bound, bound) for _ in range(NL)]
    if kind == "edge":                                                               # every limb at or next to +-bound
        return [rnd.choice((1, -1)) * (bound - rnd.choice((0, 0, 1, 2**17))) for _ in range(NL)]
    x = limbs_of(rnd.randrange(P))                                                   # "reduced": what fe_mul returns
    return x


def field_pairs():
    """[(family, f, g)]: every (f, g) fe_mul is run on; f within LOOSE, g within TIGHT."""
    rnd = random.Random(30)
    out = []
    for sf in (1, -1):
        for sg in (1, -1):
            out.append(("allmax", [sf * LOOSE] * NL, [sg * TIGHT] * NL))
    alt = [(-1) ** i for i in range(NL)]
    out.append(("allmax", [a * LOOSE for a in alt], [a * TIGHT for a in alt]))
    out.append(("allmax", [a * LOOSE for a in alt], [-a * TIGHT for a in alt]))
    out += [("column", f, g) for _, _, f, g in column_extreme_pairs()]
    out += [("hisplit", f, g) for _, _, f, g in high_split_pairs()]
    out += [("neglimb1", f, g) for f, g in limb1_pairs(-1)]
    out += [("poslimb1", f, g) for f, g in limb1_pairs(1)]
    for l8 in (2**23, 2**23 + 1, 2**24, 3 * 2**23, LOOSE, -(2**23), -3 * 2**23, -LOOSE):    # limb 8 past its 23 bits
        for g8 in (M23, 2**23, TIGHT, -TIGHT):
            f, g = _rand_limbs(rnd, LOOSE, "reduced"), _rand_limbs(rnd, TIGHT, "reduced")
            f[8], g[8] = l8, g8
            out.append(("limb8", f, g))
    sp = special_limbs()
    for a in sp.values():
        for b in sp.values():
            out.append(("special", a, b))
        out.append(("special", a, _rand_limbs(rnd, TIGHT, "uniform")))
        out.append(("special", _rand_limbs(rnd, LOOSE, "uniform"), a))
    for i in range(600):
        kind = ("uniform", "edge", "reduced")[i % 3]
        out.append(("random", _rand_limbs(rnd, LOOSE, kind), _rand_limbs(rnd, TIGHT, ("edge", "uniform", "reduced")[i % 3])))
    assert all(max(map(abs, f)) <= LOOSE and max(map(abs, g)) <= TIGHT for _, f, g in out)
    return out


def square_column_inputs():
    """[(k, sigma, f)]: column k of f^2 at its bound.  sigma = +1: s_i = s_(k-i), all products + T^2; sigma = -1: s_i = -s_(k-i)
    and a zero middle limb (f_(k/2)^2 cannot be negative), all products - T^2."""
    out = []
    for k in range(17):
        idx = [i for i in range(NL) if 0 <= k - i < NL]
        half = [i for i in idx if 2 * i < k]
        for sigma in (1, -1):
            for s in _signs(len(half)):
                f = [0] * NL
                for si, i in zip(s, half):
                    f[i], f[k - i] = si * TIGHT, si * sigma * TIGHT
                if k % 2 == 0 and sigma == 1:
                    f[k // 2] = TIGHT
                if any(f):
                    out.append((k, sigma, f))
    return out


def square_inputs():
    """[(family, f)]: fe_sq inputs, TIGHT (the doubled limbs fit int32)."""
    out = [("column", f) for _, _, f in square_column_inputs()]
    seen = set()
    for fam, _, g in field_pairs():
        if fam != "column" and tuple(g) not in seen:
            seen.add(tuple(g))
            out.append((fam, g))
    assert all(max(map(abs, f)) <= TIGHT and 2 * max(map(abs, f)) < 2**31 for _, f in out)
    return out


def carry_inputs():
    """[(family, f)]: fe_carry inputs.  "stated": up to |limb| < 2^31 / 20, the bound its comment used to give; "loose": up to
    3 T, what ge.h's formulas hand it (G = D + C); "full": up to |limb| < 2^31 - 4, the precondition the comment states now;
    "neg1": the inputs that leave limb 1 at -1 and at 2^29."""
    rnd = random.Random(32)
    out = []
    for name, b in (("stated", CARRY_STATED), ("loose", LOOSE), ("full", CARRY_FULL)):
        out += [(name, [s * b] * NL) for s in (1, -1)]
        out += [(name, [(-1) ** i * s * b for i in range(NL)]) for s in (1, -1)]
        out += [(name, _rand_limbs(rnd, b, k)) for k in ("uniform", "edge") for _ in range(100)]
    out.append(("neg1", [0, 0, 0, 0, 0, 0, 0, 0, -1]))                               # value -2^232: limb 0 borrows from limb 1 = 0
    out.append(("neg1", [M29, M29, M29, M29, M29, M29, M29, M29, 2**23 + M23]))      # limb 0 overflows into limb 1 = 2^29 - 1
    out += [("special", v) for v in special_limbs().values()]
    return out


def addc_inputs():
    """[(f, g)]: fe_addc on two tight values."""
    rnd = random.Random(33)
    out = [([s * TIGHT] * NL, [t * TIGHT] * NL) for s in (1, -1) for t in (1, -1)]
    out += [(_rand_limbs(rnd, TIGHT, k), _rand_limbs(rnd, TIGHT, k)) for k in ("uniform", "edge", "reduced") for _ in range(60)]
    return out


def encoding_inputs():
    """[(value mod p, limbs)]: fe_towords inputs whose VALUE is 0, p, p +- 1, 2p, -1 (and a few random ones), written with
    negative and loose limbs: canonical limbs of v + m p, then borrows between neighbours (limb i -= d 2^29, limb i+1 += d) and
    through the top (limb 8 -= d 2^23, limb 0 += 19 d), which leave the value mod p alone."""
    rnd = random.Random(34)
    out = []
    for v in (0, P, P + 1, P - 1, 2 * P, -1, 1, 19, -19, 2**255 - 1, rnd.randrange(P), -rnd.randrange(P)):
        for rep in range(12):
            x = v % P + (P if rep % 3 == 1 and v % P + P < 2**255 else 0)
            l = limbs_of(x)
            if rep:
                for i in range(NL):
                    d = rnd.randint(-2, 2)
                    if i < 8:
                        l[i] -= d << 29
                        l[i + 1] += d
                    else:
                        l[8] -= d << 23
                        l[0] += 19 * d
            if rep % 4 == 3:
                l = [-a for a in limbs_of((-v) % P)] if rep == 3 else [3 * a for a in limbs_of(v * pow(3, -1, P) % P)]
            assert max(map(abs, l)) <= LOOSE and value(l) % P == v % P
            out.append((v % P, l))
    return out


def field_values():
    """A few dozen values for fe_invert / fe_pow22523 (canonical limbs)."""
    rnd = random.Random(35)
    return [1, 2, P - 1, P - 2, 19, 2**29 - 1, 2**29, 2**232, 2**254, 2**255 - 20] + [rnd.randrange(1, P) for _ in range(30)]


def sqrt_ratio_inputs():
    """[(u, v)]: squares, non-squares, u = 0, v = 0."""
    rnd = random.Random(36)
    out = [(0, 1), (0, rnd.randrange(1, P)), (1, 0), (rnd.randrange(1, P), 0), (0, 0), (1, 1), (P - 1, 1), (1, P - 1), (2, 1), (1, 2)]
    for _ in range(14):
        r, v = rnd.randrange(1, P), rnd.randrange(1, P)
        out.append((r * r * v % P, v))                                               # u / v = r^2
        out.append((rnd.randrange(1, P), v))
    return out


# ------------------------------------------------------------------------------------------------ points
def point_limbs(pt):
    """A pyref.Point as 36 reduced limbs (X | Y | Z | T)."""
    return limbs_of(pt.X) + limbs_of(pt.Y) + limbs_of(pt.Z) + limbs_of(pt.T)


def point_of_limbs(R, l36):
    return R.Point(*(value(l36[9 * i:9 * i + 9]) for i in range(4)))


def affine(R, pt):
    zi = pow(pt.Z, P - 2, P)
    return R.Point(pt.X * zi, pt.Y * zi, 1, pt.X * zi * pt.Y * zi)


def points(R):
    """{name: pyref.Point}: identity, basepoint, its negative, points with Z != 1 (results of a doubling / an addition),
    decompressed points (|x| returned, Z = 1) and affine points for the niels form."""
    rnd = random.Random(37)
    B = R.BASEPOINT
    pts = {"id": R.IDENTITY, "B": B, "-B": -B, "2B": B.double(), "3B": B.double() + B, "-2B": -(B.double()), "Bb": R.B_BLINDING}
    for i in range(6):
        q = rnd.randrange(R.L) * B
        pts["r%d" % i] = q                                                           # Z != 1
        pts["d%d" % i] = R.decompress(q.compress())                                  # decompressed
        pts["a%d" % i] = affine(R, q)
    pts["l-1"] = (R.L - 1) * B
    return pts


def point_pairs(R):
    """[(name, p, q)] for the additions: identity either side, P + (-P), P + P through the ADDITION formulas, Z != 1 either side."""
    pts = points(R)
    names = [("id", "id"), ("id", "B"), ("B", "id"), ("B", "-B"), ("B", "B"), ("2B", "2B"), ("2B", "-2B"), ("2B", "B"), ("B", "2B"),
             ("r0", "r0"), ("r0", "r1"), ("r1", "d2"), ("d3", "d3"), ("d4", "r5"), ("l-1", "B"), ("Bb", "r2"), ("3B", "-2B")]
    return [(a + "+" + b, pts[a], pts[b]) for a, b in names]


def madd_pairs(R):
    """[(name, p, q affine)] for the mixed additions (q enters as ge_to_niels(x, y))."""
    pts = points(R)
    names = [("id", "id"), ("id", "B"), ("B", "id"), ("B", "-B"), ("B", "B"), ("2B", "B"), ("r0", "a0"), ("r1", "a1"), ("r0", "d0"),
             ("d2", "d2"), ("r3", "a3"), ("l-1", "B"), ("r4", "Bb"), ("3B", "a5"), ("r5", "-B"), ("-2B", "d1")]
    out = [(a + "+" + b, pts[a], affine(R, pts[b])) for a, b in names]
    assert all(q.Z == 1 for _, _, q in out)
    return out


def encodings(R):
    """[32 bytes]: valid and invalid ristretto encodings, the four fixed ones of test_group_law_and_codec among them."""
    rnd = random.Random(38)
    out = [bytes(32), R.P.to_bytes(32, "little"), (1).to_bytes(32, "little"), b"\xff" * 32, (R.P - 1).to_bytes(32, "little"),
           (R.P + 2).to_bytes(32, "little"), (2).to_bytes(32, "little"), (2**255).to_bytes(32, "little")]
    out += [p.compress() for p in points(R).values()]
    out += [bytes(rnd.randrange(256) for _ in range(31)) + bytes([rnd.randrange(128)]) for _ in range(40)]
    return out


def uniform_inputs():
    rnd = random.Random(39)
    return [bytes(64), b"\xff" * 64, bytes([1]) + bytes(63)] + [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(13)]


# ------------------------------------------------------------------------------------------------ scalars
SCALAR_EDGE_PAIRS = [(2**256 - 1, L - 1), (L - 1, L - 1), (0, L - 1), (2**256 - 1, 0), (2**256 - 1, 1), (L, L - 1), (2**255, 2**252),
                     (2**29 - 1, 2**29 - 1), (2**232, 2**232), ((1 << 256) - (1 << 232), L - 2)]     # test_scalar_field's


def scalar_pairs():
    """[(a, b)]: a any 256-bit integer, b < L."""
    rnd = random.Random(40)
    out = list(SCALAR_EDGE_PAIRS) + [(1, 1), (L - 1, 1), (L + 1, 2), (2**252, 2**252 - 1)]
    out += [(rnd.randrange(2**256) if i % 3 else rnd.randrange(L), rnd.randrange(L)) for i in range(200)]
    return out


def wide_inputs():
    rnd = random.Random(41)
    return [bytes(64), b"\xff" * 64, L.to_bytes(64, "little"), (L * L).to_bytes(64, "little"), (L * L - 1).to_bytes(64, "little"),
            (2**256).to_bytes(64, "little"), (2**512 - 2**256).to_bytes(64, "little")] + \
           [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(60)]


def recode_cases():
    """[(W, NW, x, name)]: edge_scalars.families at edge_scalars.WIDTHS, under the window count of their kind (a canonical
    scalar or a 64-bit value is also a legal input of the wider "blinding" convention)."""
    out = []
    for W in E.WIDTHS:
        for kind in E.BOUNDS:
            for name, x in E.families(W, kind).items():
                out.append((W, E.nwin_of(kind, W), x, "%s-%s" % (kind, name)))
                if kind != "blinding":
                    out.append((W, E.nwin_of("blinding", W), x, "%s-as-blinding-%s" % (kind, name)))
    return out

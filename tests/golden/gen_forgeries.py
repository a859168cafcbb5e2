#!/usr/bin/env python3
"""Generates tests/golden/forgeries.json from the Python oracle's forging prover (oracle/pyref.py: range_prove(forge=)).

Every row is a range proof that is CONSISTENT IN THE TRANSCRIPT AND WRONG IN THE ALGEBRA: one element is forged, it is the
forged element that enters the Merlin transcript, and everything after it is computed honestly from the resulting challenges.
A flipped byte changes every later challenge and so fails both halves of the verifier's check at once; these rows fail exactly
the half that is written in their `violates` field -- the polynomial equation that the verifier weighs by c (`t`), the
inner-product equation (`P`), or, for a wrong t_x alone, both -- and leave the identity in the other.  That is asserted here,
row by row, against range_verify(info=), together with the closed form of the residual where one exists:

    residual = the verifier's point sum, acc(c) = acc_P + c acc_t (pyref.range_verify); so a term of the left-hand side
    (V_j, A, S, T_1, T_2, L_k, R_k) keeps its sign and t_x, tau, mu -- which the sum subtracts -- change theirs.  SIGN fixes that once.

Shapes (n, m) = (8,1), (8,4), (8,8): N = 8, 32, 64 generators a side -- lgN odd and even, both branches of rv_q_split's
lb >= lgn (lb = 1, 2 < lgn = 3 and lb = 3 >= 3), both sides of the lazy-scalar condition N >= 64 (verify_plan.inc).
Run:  python3 tests/golden/gen_forgeries.py          (about two minutes)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import pyref as R  # noqa: E402

SEED = bytes(range(32))
SHAPES = [(8, 1), (8, 4), (8, 8)]
IDENT = bytes(32)
SIGN = {"tau": -1, "mu": -1}                         # every other kind +1; t_x: -1 in t, +1 in P (spelled out in predicted())


def hx(b):
    return bytes(b).hex()


def d_name(d, n):
    """The offset d as the fixture spells it: "1", "L-1" or "2^n"."""
    return {1: "1", R.L - 1: "L-1", 2**n: "2^n"}[d]


def witness(n, m):
    """The honest witness of a shape: values inside the range (party 0 holds 0, the last one 2^n - 1 where m >= 2) and blindings."""
    values = [int.from_bytes(R.seed_wide(SEED, 20, n, 16 * m + j)[:8], "little") & (2**n - 1) for j in range(m)]
    if m >= 2:
        values[0], values[m - 1] = 0, 2**n - 1
    bl = [R.scalar_from_wide(R.seed_wide(SEED, 21, n, 16 * m + j)) for j in range(m)]
    return values, bl


def plan(n, m):
    """[forge dict] of a shape: every kind, at parties {0, m-1} (+ the middle for m = 8), generator indexes q in {0, 2^lb - 1, 2^lb,
    N - 1} (lb = lgN / 2, the split of the verifier's power tables), rounds k in {0, lgN - 1}, d in {1, L - 1} (and 2^n for a value).
    The group elements share the four q between them so that G_q and H_q are each moved at every q once."""
    N = n * m
    lgN = N.bit_length() - 1
    lb = lgN // 2
    qs = [0, (1 << lb) - 1, 1 << lb, N - 1]
    parties = sorted({0, m - 1} | ({m // 2 - 1} if m == 8 else set()))
    one, neg = 1, R.L - 1
    kl = lgN - 1
    rows = []
    for i, d in enumerate((2**n, one, neg)):
        rows.append(dict(kind="value", party=parties[i % len(parties)], d=d))
    for i, j in enumerate((0, m - 1) if m > 1 else (0,)):
        rows.append(dict(kind="blinding", party=j, d=(one, neg)[i % 2]))
    for q in qs:
        rows.append(dict(kind="bit", q=q, d=one))                 # (d unused: the bit pair is (2, 1))
    for i, q in enumerate(qs if m == 1 else qs[1:3]):             # (positions cut for the larger shapes: the file stays below 200 KB)
        rows.append(dict(kind="a_R", q=q, d=(one, neg)[i % 2]))
    rows += [dict(kind="A", P="B", d=one), dict(kind="A", P="B_blinding", d=neg), dict(kind="A", P="G", q=qs[0], d=neg), dict(kind="A", P="H", q=qs[3], d=one)]
    rows += [dict(kind="S", P="B", d=neg), dict(kind="S", P="B_blinding", d=one), dict(kind="S", P="G", q=qs[2], d=one), dict(kind="S", P="H", q=qs[1], d=neg)]
    rows += [dict(kind="L_k", k=0, P="B", d=one), dict(kind="L_k", k=0, P="G", q=qs[1], d=neg),
             dict(kind="L_k", k=kl, P="B_blinding", d=neg), dict(kind="L_k", k=kl, P="H", q=qs[2], d=one)]
    rows += [dict(kind="R_k", k=0, P="B_blinding", d=one), dict(kind="R_k", k=0, P="H", q=qs[0], d=neg),
             dict(kind="R_k", k=kl, P="B", d=neg), dict(kind="R_k", k=kl, P="G", q=qs[3], d=one)]
    rows += [dict(kind="T1", P="B", d=one), dict(kind="T1", P="B_blinding", d=neg), dict(kind="T2", P="B", d=neg), dict(kind="T2", P="B_blinding", d=one)]
    rows += [dict(kind="t_x", d=one), dict(kind="t_x", d=neg), dict(kind="tau", d=one), dict(kind="mu", d=neg)]
    rows += [dict(kind="a", d=one), dict(kind="b", d=neg)]
    return rows


def predicted(f, ch, n, m):
    """Closed form of the residual(s) of a forgery from the PROVER's challenges: {"P": point | None, "t": point | None}; None = no
    closed form is claimed for that half (the violates field still says whether it is the identity)."""
    L = R.L
    G, H = R.bp_gens(n, m)
    kind = f["kind"]
    d = SIGN.get(kind, 1) * f["d"] % L
    pt = R._forge_point(f, G, H)
    y, z, x, w, u = ch["y"], ch["z"], ch["x"], ch["w"], ch["u"]
    if kind == "value":
        return dict(t=(pow(z, 2 + f["party"], L) * d % L) * R.BASEPOINT)
    if kind == "blinding":
        return dict(t=(pow(z, 2 + f["party"], L) * d % L) * R.B_BLINDING)
    if kind == "T1":
        return dict(t=(x * d % L) * pt)
    if kind == "T2":
        return dict(t=(x * x * d % L) * pt)
    if kind == "tau":
        return dict(t=d * R.B_BLINDING)
    if kind == "mu":
        return dict(P=d * R.B_BLINDING)
    if kind == "A":
        return dict(P=d * pt)
    if kind == "S":
        return dict(P=(x * d % L) * pt)
    if kind == "L_k":
        return dict(P=(u[f["k"]] ** 2 * d % L) * pt)
    if kind == "R_k":
        return dict(P=(R.inv(u[f["k"]]) ** 2 * d % L) * pt)
    if kind == "t_x":
        return dict(t=((-d) % L) * R.BASEPOINT, P=(w * d % L) * R.BASEPOINT)
    return {}


def violated(res_P, res_t):
    return {(False, True): "P", (True, False): "t", (False, False): "both"}.get((res_P == IDENT, res_t == IDENT))


def rows_for_shape(n, m, verbose=False):
    """The fixture rows of one shape: the honest proof first, then plan()'s forgeries, each from the same witness and nonce stream."""
    values, bl = witness(n, m)
    out = []
    for idx, f in enumerate([None] + plan(n, m)):
        ch, vi = {}, {}
        proof = R.range_prove(values, bl, n, R.Tape(seed=SEED, stream_id=1000 * m + idx), forge=f, info=ch)
        assert len(proof) == R.range_proof_size(n, m)
        ok, res_P, res_t = R.range_verify(proof, ch["V"], n, info=vi)
        assert all(vi[k] == ch[k] for k in ("y", "z", "x", "w", "u")), "the verifier replays the prover's transcript"
        row = {"n": n, "m": m, "stream_id": 1000 * m + idx, "kind": "honest" if f is None else f["kind"]}
        if f is None:
            assert ok and res_P == IDENT and res_t == IDENT
            row.update(position={}, d=None, violates=None, predicted={})
        else:
            v = violated(res_P, res_t)
            assert not ok and v is not None, f
            pred = {k: pt.compress() for k, pt in predicted(f, ch, n, m).items()}
            for half, got in (("P", res_P), ("t", res_t)):
                if half in pred:
                    assert pred[half] == got and got != IDENT, (f, half)        # exactly the one term, with SIGN's sign
                elif pred:
                    assert got == IDENT, (f, half)                             # a closed form for one half: the other half holds
            want = "both" if f["kind"] == "t_x" else ("t" if f["kind"] in ("value", "blinding", "bit", "a_R", "T1", "T2", "tau") else "P")
            assert v == want, (f, v)
            row.update(position={k: f[k] for k in ("party", "q", "k", "P") if k in f}, d=d_name(f["d"], n), violates=v,
                       predicted={k: hx(b) for k, b in pred.items()})
        row.update(commitments=[hx(V) for V in ch["V"]], proof=hx(proof))
        out.append(row)
        if verbose:
            print(n, m, row["kind"], row["position"], row["violates"], flush=True)
    return out


if __name__ == "__main__":
    rows = []
    for n, m in SHAPES:
        rows += rows_for_shape(n, m, verbose=True)
    path = os.path.join(HERE, "forgeries.json")
    with open(path, "w") as fo:
        json.dump({"seed": hx(SEED), "rows": rows}, fo, indent=0, separators=(",", ":"))
        fo.write("\n")
    print("wrote forgeries.json:", len(rows), "rows,", os.path.getsize(path), "bytes")

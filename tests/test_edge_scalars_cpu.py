"""The crafted scalars of tests/edge_scalars.py do hit the edges they are named for (so that the GPU tests built on them cannot
silently miss them), and the two oracles agree on range proofs whose every nonce is such a scalar -- only then may they judge the
GPU (tests/test_gpu_window_widths.py).  CPU only."""
import ctypes

import pytest

import edge_scalars as E


@pytest.mark.parametrize("kind", E.BOUNDS)
@pytest.mark.parametrize("W", E.WIDTHS)
def test_families_round_trip_and_hit_their_digits(W, kind):
    NW, k, half, bound = E.nwin_of(kind, W), E.whole_windows(kind, W), 1 << (W - 1), E.bound_of(kind)
    assert 1 <= k < NW and (1 << (W * k)) <= bound
    fam = E.families(W, kind)
    dig = {}
    for name, x in fam.items():
        d = E.recode(x, W, NW)
        assert len(d) == NW and sum(v << (W * i) for i, v in enumerate(d)) == x, (name, W, kind)
        assert all(-half <= v <= half for v in d) and all(v < half for v in d[:-1]), (name, W, kind)
        dig[name] = d
    # allneg: the row's last entry, negated, in every window below the top one(s); the window above them holds the carry alone
    assert dig["allneg"][:k] == [-half] * k and dig["allneg"][k] == 1 and not any(dig["allneg"][k + 1:])
    assert dig["allneg"].count(-half) >= k - 1
    assert dig["allpos"][:k] == [half - 1] * k and not any(dig["allpos"][k:])
    assert dig["althalf"][:k] == [-half if i % 2 == 0 else 1 for i in range(k)]
    assert dig["althalf"][k] == (1 if k % 2 else 0)
    assert not any(dig["zero"]) and dig["one"] == [1] + [0] * (NW - 1)
    assert dig["lastwin"] == [0] * (k - 1) + [1] + [0] * (NW - k)
    if "topwin" in fam:
        assert dig["topwin"] == [0] * k + [1] + [0] * (NW - k - 1)
    else:
        assert (1 << (W * k)) == bound               # no partial window: 255 = 15 * 17
    # ones = bound - 1: 2^(W k) - 1 below window k is -1 followed by zeros, with a carry that arrives in window k
    top = (bound - 1) >> (W * k)
    if kind != "canonical":
        assert dig["ones"][:k] == [-1] + [0] * (k - 1) and dig["ones"][k] == top + 1
    else:
        assert fam["ones"] == E.L - 1
    if kind == "blinding" and W in (8, 16):
        assert dig["ones"][NW - 1] == half            # +2^(W-1): only the top window can hold it, and only where W divides 256
    if kind == "blinding" and W == 8:                 # 2^255 - 2^247 = 0x7f80 << 240: the smallest input whose top digit is +128
        assert dig["top128"] == [0] * 30 + [-128, 128]
    if kind == "blinding":
        assert fam["l"] == E.L and fam["l+1"] >= E.L and fam["ones"] >= E.L and fam["top128"] >= E.L       # unreduced inputs
    # a top window that can hold nothing but the carry
    if (kind, W) in (("blinding", 15), ("value", 16), ("value", 8)):
        assert NW == k + 1 and (1 << (W * k)) == bound
        assert dig["allneg"][NW - 1] == 1 and dig["ones"][NW - 1] == 1
    if (kind, W) == ("canonical", 11):               # window 22 holds bit 252 alone (2^10 = half), window 23 starts at bit 253
        assert NW == k + 2 and dig["ones"][NW - 2:] == [-half, 1] and dig["allneg"][NW - 2:] == [1, 0]


def test_width_list_covers_what_it_claims():
    assert E.WIDTHS == (8, 11, 15, 16, 17, 20)
    assert E.nwin_of("blinding", 8) == 32
    assert 253 % 11 == 0 and E.nwin_of("canonical", 11) == 24
    assert 255 % 15 == 0 and E.nwin_of("blinding", 15) == 18 and E.nwin_of("canonical", 15) == 17
    assert 64 % 16 == 0 and E.nwin_of("value", 16) == 5 and not -32768 <= (1 << 15) <= 32767
    assert E.nwin_of("blinding", 17) == 16 and E.nwin_of("canonical", 17) == 15
    assert E.nwin_of("blinding", 20) == 13


def test_crafted_tapes_reduce_to_their_scalars(pyref):
    assert E.L == pyref.L
    for W in E.WIDTHS:
        for name in E.TAPES:
            xs = E.tape_scalars(W, name, 40)
            tp = E.tape_bytes(W, name, 40)
            assert len(tp) == 40 * 64
            assert [pyref.scalar_from_wide(tp[64 * s:64 * s + 64]) for s in range(40)] == xs
        assert len(set(E.tape_scalars(W, "mix", 40))) == len(E.families(W, "canonical"))


@pytest.mark.parametrize("n,m", [(8, 1), (8, 2)])
def test_oracles_agree_on_crafted_tapes(ref, pyref, n, m):
    """pyref.range_prove (big integers) and ref_range_prove (the C oracle) with the same crafted tape: the same bytes.  The all-zero
    tape makes S, T_1 and T_2 the identity (its proof does not verify; only the bytes are compared)."""
    slots = m * (2 * n + 4)
    ps = ref.ref_range_proof_size(n, m)
    vals = [0xA5, 0xFF][:m]
    blind = [E.families(16, "blinding")["l-1"], E.families(16, "canonical")["allneg"]][:m]
    v = (ctypes.c_uint64 * m)(*vals)
    r = b"".join(E.le32(x) for x in blind)
    seen = set()
    for W in E.WIDTHS:                      # the tapes depend on the width they were crafted for ...
        for name in E.TAPES:
            if W != E.WIDTHS[0] and name in ("zero", "ones"):
                continue                     # ... except all-zero and all l - 1
            tape = E.tape_bytes(W, name, slots)
            out = ctypes.create_string_buffer(ps)
            rc = ref.ref_range_prove(n, m, v, r, None, ctypes.c_uint64(0), ctypes.c_uint64(0), tape, 0, out)
            assert rc == 0, (W, name)
            want = pyref.range_prove(vals, blind, n, pyref.Tape(draws=[tape[64 * s:64 * s + 64] for s in range(slots)]))
            assert out.raw == want, (W, name, n, m)
            if name == "zero":
                ident = bytes(32)            # the identity's encoding
                assert want[32:64] == ident and want[64:96] == ident and want[96:128] == ident
            seen.add(want)
    assert len(seen) == 2 + 3 * len(E.WIDTHS)    # every tape gave a proof of its own

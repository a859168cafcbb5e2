"""Crafted scalars that sit on the edges of the signed-window recoding (dapol_amd/csrc/sc.h: sc_recode_w and its hand-written
copies in tables.h, kernels_range.h and kernels_range_gs.h), and a plain big-integer recoder to check them with.

A random window is the digit -2^(W-1) with probability 2^-W, so random inputs never read a table row's last entry, never send a
carry through every window and never leave the top window holding the carry alone.  These inputs do, at every width."""

L = 2**252 + 27742317777372353535851937790883648493

# The window widths the tests run, and why each one:
#    8  WBITS_MIN; nwin() = 32 windows fill the 32 lanes of tbl_fixed_mul_wave exactly
#   11  253 = 11 * 23: the top window of a canonical scalar holds nothing but the carry
#   15  255 = 15 * 17: the top window of a blinding holds nothing but the carry; nwin_c() = 17 is odd, so the two halves of a
#       scalar split at hi_split (the high-half rows) are uneven
#   16  what a DAPOL_PROFILE_HOST context gets; 64 = 4 * 16 (a value's top window is carry-only); the digits +-32768 do not fit int16
#   17  the width the bench profile chooses on an idle card (WBITS_AUTO_MAX), pinned here instead of left to the free memory
#   20  WBITS_MAX
WIDTHS = (8, 11, 15, 16, 17, 20)

BOUNDS = ("blinding", "canonical", "value")


def bound_of(kind):
    """The exclusive upper bound of the inputs of one kind."""
    return {"blinding": 2**255, "canonical": L, "value": 2**64}[kind]


def nwin_of(kind, W):
    """Windows the product uses for the kind: TableView::nwin / nwin_c / nwin64 (tables.h)."""
    return {"blinding": 255 // W + 1, "canonical": 253 // W + 1, "value": (64 + W - 1) // W + 1}[kind]


def whole_windows(kind, W):
    """k: the W-bit windows that lie wholly below the bound (2^(W k) <= bound)."""
    return (bound_of(kind).bit_length() - 1) // W


def recode(x, W, NW):
    """Signed radix-2^W digits of x, as sc_recode_w defines them: digits in [-2^(W-1), 2^(W-1)], a window that reaches 2^(W-1)
    borrows 2^W from the next one, and the top digit absorbs the last carry (so it alone may be +2^(W-1))."""
    half, carry, out = 1 << (W - 1), 0, []
    for i in range(NW):
        b = ((x >> (W * i)) & ((1 << W) - 1)) + carry
        carry = 1 if (b >= half and i < NW - 1) else 0
        out.append(b - (carry << W))
    return out


def families(W, kind):
    """{name: scalar} for one width and one kind of input ("blinding", "canonical" or "value"); every scalar is below the bound."""
    bound, k, half = bound_of(kind), whole_windows(kind, W), 1 << (W - 1)
    win = lambda i, d: d << (W * i)
    f = {
        "allneg": win(0, half) + sum(win(i, half - 1) for i in range(1, k)),       # every digit below window k becomes -half by the carry chain
        "allpos": sum(win(i, half - 1) for i in range(k)),                         # the largest positive digits, no carry
        "althalf": sum(win(i, half) for i in range(0, k, 2)),                      # -half, 1, -half, 1, ...
        "ones": bound - 1,                                                         # a carry through every window
        "zero": 0,
        "one": 1,
        "lastwin": win(k - 1, 1),                                                  # 2^(W i) for the last whole window ...
    }
    if win(k, 1) < bound:
        f["topwin"] = win(k, 1)                                                    # ... and for the partial one above it, where there is one
    if kind == "blinding":
        f.update({"l-1": L - 1, "l": L, "l+1": L + 1, "top128": 2**255 - 2**247})
    assert all(0 <= x < bound for x in f.values())
    return f


def le32(x):
    return int(x).to_bytes(32, "little")


def draw(x):
    """A 64-byte tape draw whose reduction is the canonical scalar x itself: x in the low 32 bytes, zeros above."""
    assert 0 <= x < L
    return le32(x) + bytes(32)


def tape_scalars(W, name, slots):
    """The scalars of one crafted tape of `slots` draws: "zero", one family of canonical scalars throughout, or "mix", which
    cycles through all the families slot by slot."""
    fam = families(W, "canonical")
    if name == "mix":
        names = sorted(fam)
        return [fam[names[s % len(names)]] for s in range(slots)]
    return [fam[name]] * slots


TAPES = ("zero", "allneg", "allpos", "ones", "mix")       # "ones" of the canonical scalars is l - 1


def tape_bytes(W, name, slots):
    return b"".join(draw(x) for x in tape_scalars(W, name, slots))

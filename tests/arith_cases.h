// Test-only: ONE case of each arithmetic operation on raw limbs / words, written once for both paths -- tests/host_shim.cpp
// loops over the cases with g++, tests/dev_shim.hip runs one case per lane on the GPU -- so that the two can be compared limb
// for limb.  Nothing here is part of libdapol_hip.so.  (tests/conftest.py rebuilds host_shim.so when host_shim.cpp or a product
// header changes, not when this file does: touch host_shim.cpp after editing it.)
#pragma once
#include "../dapol_amd/csrc/ge.h"
#include "../dapol_amd/csrc/sc.h"
#include "../dapol_amd/csrc/hash.h"

namespace dapol_test {
using namespace dapol;

enum { FEOP_MUL = 0, FEOP_SQ, FEOP_CARRY, FEOP_ADDC, FEOP_TOWORDS, FEOP_ABS, FEOP_INVERT, FEOP_POW22523, FEOP_SQRT_RATIO };
enum { GEOP_MADD = 0, GEOP_ADD, GEOP_DBL, GEOP_ADD_CACHED, GEOP_NEG, GEOP_CHAIN };
enum { SCOP_MUL = 0, SCOP_ADD, SCOP_SUB, SCOP_INVERT, SCOP_INVERT_VARTIME, SCOP_FROM_U64, SCOP_MONTMUL_RAW };
enum { GE_CHAIN_ROUNDS = 4, GE_CHAIN_DBLS = 8 };       // GEOP_CHAIN: (one mixed addition, then W = 8 doublings) four times

DAPOL_HD void fe_load(fe& h, const int32_t* l) {
    for (int i = 0; i < FE_NL; i++) h.v[i] = l[i];
}
DAPOL_HD void fe_store(int32_t* l, const fe& h) {
    for (int i = 0; i < FE_NL; i++) l[i] = h.v[i];
}
DAPOL_HD void ge_load(ge_p3& p, const int32_t* l) {
    fe_load(p.X, l); fe_load(p.Y, l + 9); fe_load(p.Z, l + 18); fe_load(p.T, l + 27);
}
DAPOL_HD void ge_store(int32_t* l, const ge_p3& p) {
    fe_store(l, p.X); fe_store(l + 9, p.Y); fe_store(l + 18, p.Z); fe_store(l + 27, p.T);
}

// f, g: nine raw limbs each -> the result's limbs as the operation left them, and their canonical words.  Returns the
// operation's flag (was_square) or 0.
DAPOL_HD int fe_case(int op, const int32_t* fl, const int32_t* gl, int32_t* ol, uint32_t* ow) {
    fe f, g, r;
    fe_load(f, fl);
    fe_load(g, gl);
    int flag = 0;
    switch (op) {
        case FEOP_MUL: fe_mul(r, f, g); break;
        case FEOP_SQ: fe_sq(r, f); break;
        case FEOP_CARRY: fe_carry(r, f); break;
        case FEOP_ADDC: fe_addc(r, f, g); break;
        case FEOP_ABS: fe_abs(r, f); break;
        case FEOP_INVERT: fe_invert(r, f); break;
        case FEOP_POW22523: fe_pow22523(r, f); break;
        case FEOP_SQRT_RATIO: flag = fe_sqrt_ratio_m1(r, f, g) ? 1 : 0; break;
        default: r = f; break;                                   // FEOP_TOWORDS: the words of f itself
    }
    fe_store(ol, r);
    fe_towords(ow, r);
    return flag;
}

// p, q: 36 reduced limbs each (X | Y | Z | T; q affine, Z = 1, where it enters as a niels entry) -> the result's 36 limbs and
// its ristretto encoding.
DAPOL_HD void ge_case(int op, const int32_t* pl, const int32_t* ql, int neg, int32_t* ol, uint32_t* ow) {
    ge_p3 p, q, r;
    ge_load(p, pl);
    ge_load(q, ql);
    switch (op) {
        case GEOP_MADD: {
            ge_niels n;
            ge_to_niels(n, q.X, q.Y);
            ge_madd(r, p, n, neg != 0);
            break;
        }
        case GEOP_ADD: ge_add(r, p, q); break;
        case GEOP_DBL: ge_dbl(r, p, true); break;
        case GEOP_ADD_CACHED: {
            ge_cached c;
            ge_to_cached(c, q);
            ge_add_cached(r, p, c, neg != 0);
            break;
        }
        case GEOP_NEG: ge_neg(r, p); break;
        default: {                                               // GEOP_CHAIN
            ge_niels n;
            ge_to_niels(n, q.X, q.Y);
            r = p;
            for (int k = 0; k < GE_CHAIN_ROUNDS; k++) {
                ge_p3 t;
                ge_madd(t, r, n, neg != 0);
                r = t;
                for (int d = 0; d < GE_CHAIN_DBLS; d++) { ge_dbl(t, r, true); r = t; }
            }
            break;
        }
    }
    ge_store(ol, r);
    ge_compress(ow, r);
}
// eight words -> ok, the decoded point's limbs and its encoding again
DAPOL_HD int ge_decompress_case(const uint32_t* in, int32_t* ol, uint32_t* ow) {
    ge_p3 p;
    const bool ok = ge_decompress(p, in);
    ge_store(ol, p);
    ge_compress(ow, p);
    return ok ? 1 : 0;
}
DAPOL_HD void ge_uniform_case(const uint32_t* in16, int32_t* ol, uint32_t* ow) {
    ge_p3 p;
    ge_from_uniform(p, in16);
    ge_store(ol, p);
    ge_compress(ow, p);
}

// a: any 256-bit integer, b < L (eight words each) -> canonical words of the result.  SCOP_MONTMUL_RAW is sc_montmul on the
// words as they are (a b / 2^256 mod L); the others enter and leave through sc_to_mont / sc_from_mont.
DAPOL_HD void sc_case(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    sc x, y, r;
    if (op == SCOP_MONTMUL_RAW) {
        for (int i = 0; i < 8; i++) { x.v[i] = a[i]; y.v[i] = b[i]; }
        sc_montmul(r, x, y);
        for (int i = 0; i < 8; i++) out[i] = r.v[i];
        return;
    }
    sc_to_mont(x, a);
    sc_to_mont(y, b);
    switch (op) {
        case SCOP_MUL: sc_montmul(r, x, y); break;
        case SCOP_ADD: sc_add(r, x, y); break;
        case SCOP_SUB: sc_sub(r, x, y); break;
        case SCOP_INVERT: sc_invert_mont(r, x); break;
        case SCOP_INVERT_VARTIME: sc_invert_vartime_mont(r, x); break;
        default: sc_from_u64_mont(r, (uint64_t)a[0] | ((uint64_t)a[1] << 32)); break;
    }
    sc_from_mont(out, r);
}
DAPOL_HD void sc_wide_case(const uint32_t* w16, uint32_t* out) {
    sc r;
    sc_from_wide(r, w16);
    sc_from_mont(out, r);
}
enum { RECODE_MAX_NW = 32 };                                     // 255 / 8 + 1
DAPOL_HD void sc_recode_case(int W, int NW, const uint32_t* x, int32_t* d) {
    sc_recode_w(W, NW, x, [&](int i, int v) { d[i] = v; });
}

// A small Merlin transcript in either holder of the STROBE state (S = Strobe: one lane; S = WStrobe: a wavefront): init,
// append(filler: k bytes), append of nw words (opened up to read the in-block position of the first word; append_words is the
// holder's own word loop), challenge, append_words of the reversed words, challenge.  out32: the two challenges.
template <class S, class AppendWords>
DAPOL_HD uint32_t strobe_replay(S& st, const char* filler, int k, const uint32_t* w, const uint32_t* wrev, int nw, uint32_t* out32,
                                           AppendWords append_words) {
    merlin_init(st, DAPOL_LBL_("dev-shim"));
    merlin_append_bytes(st, DAPOL_LBL_("fill"), filler, k);
    merlin_frame(st, DAPOL_LBL_("words"), (uint32_t)(4 * nw));                 // (append_words, opened up to read the position)
    strobe_begin_op(st, SF_A);
    const uint32_t at = st.pos;
    append_words(st, w, nw);
    merlin_challenge_wide(st, DAPOL_LBL_("c1"), out32);
    merlin_append_words(st, DAPOL_LBL_("more"), wrev, nw);                     // (the holder's own overload, whole)
    merlin_challenge_wide(st, DAPOL_LBL_("c2"), out32 + 16);
    return at;
}

}  // namespace dapol_test

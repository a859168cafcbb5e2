// The COMPACT form of shared proofs as index arithmetic: every distinct sub-proof of a call once, in the order the shared prover
// holds them before its scatter (definition in include/dapol_hip.h, "COMPACT shared proofs").  For strictly increasing leaf indexes
// the compact buffer is, for s = 0 .. n_sub - 1 in plan order, the n_unique[s] proofs of sub-proof s in ascending subtree-key order;
// row e of sub-proof s uses proof ref[s][e] = (distinct keys of s among rows 0 .. e) - 1 of that list.  A GROUP (a run of the plan's
// sub-proofs of equal m, verify_shared_plan.inc) is contiguous in it: one [rows][proof pieces] batch without any gather.
// Pure functions, no HIP call: the host entry points (host_shared.inc, host_verify_compact.inc), the kernels
// (kernels_verify_compact.h) and tests/cpp/shared_compact_host.cpp (ASan + UBSan, tests/test_shared_compact_cpu.py) call them.
#pragma once
#include <cstring>

#include "verify_shared_plan.inc"

// The verifier's plan (spans, groups) plus the key shifts of the prover: shift[s] = H - D of sub-proof s under the sibling order
// (64: the key is 0 -- never used as a shift count).
struct SCompactPlan {
    VSharedPlan V;
    uint8_t shift[VSHARED_MAX_SUB];
};
static inline unsigned scompact_shift(const SubProof& sp, int H, bool leaf_first) {
    const int D = sp.count == 0 ? 0 : leaf_first ? H - sp.start : sp.start + sp.count;
    return (unsigned)(H - D);
}
// 0: built; otherwise vshared_plan_build's code
static int scompact_plan_build(const std::vector<SubProof>& plan, int H, int n_bits, bool leaf_first, SCompactPlan& P) {
    const int rc = vshared_plan_build(plan, H, n_bits, P.V);
    memset(P.shift, 0, sizeof P.shift);
    if (rc) return rc;
    for (size_t s = 0; s < plan.size(); s++) P.shift[s] = (uint8_t)scompact_shift(plan[s], H, leaf_first);
    return 0;
}

VSP_HD uint64_t scompact_key(uint64_t idx, unsigned shift) { return shift >= 64 ? 0ull : (idx >> shift) << shift; }
// Row e opens a new subtree key of a sub-proof with this shift (the prover's rule; row 0 always does).
VSP_HD bool scompact_key_head(const uint64_t* idx, size_t e, unsigned shift) {
    return e == 0 || scompact_key(idx[e], shift) != scompact_key(idx[e - 1], shift);
}
// The OR of the differences between rows e >= 1 and e - 1 over pieces t0, t0 + step, ... of the 2 count commitment pieces that
// sub-proof s covers (pC: [b][2 H] pieces): a lane's share in k_vcompact_heads, the whole span with (0, 1).
VSP_HD uint32_t scompact_com_diff(const VSharedPlan& P, uint32_t s, size_t e, const VsPiece* pC, uint32_t t0, uint32_t step) {
    const VsPiece* a = pC + e * 2 * (size_t)P.H + 2 * (size_t)P.start[s];
    const VsPiece* p = a - 2 * (size_t)P.H;
    uint32_t d = 0;
    for (uint32_t t = t0, n = 2u * P.count[s]; t < n; t += step)
        d |= (a[t].w[0] ^ p[t].w[0]) | (a[t].w[1] ^ p[t].w[1]) | (a[t].w[2] ^ p[t].w[2]) | (a[t].w[3] ^ p[t].w[3]);
    return d;
}
// The verifier's HEAD: a new key, or a covered commitment that differs from row e - 1's.  A head is checked once against its own
// row's commitments; the rows behind it up to the next head inherit its verdict.
VSP_HD bool scompact_is_head(const SCompactPlan& P, uint32_t s, size_t e, const uint64_t* idx, const VsPiece* pC) {
    return scompact_key_head(idx, e, P.shift[s]) || scompact_com_diff(P.V, s, e, pC, 0, 1) != 0;
}

// kref = the inclusive scan of the key flags in plan order (s-major, b per sub-proof): the proof that (s, e) uses is compact row
// kref[s][e] - kref[s0][0] of its group (row 0 of every sub-proof is a key head), and kref[s][e] - kref[s][0] of its own list.
VSP_HD size_t scompact_group_ref(const VSharedGroup& G, const uint32_t* kref, size_t b, uint32_t s, size_t e) {
    return (size_t)(kref[(size_t)s * b + e] - kref[(size_t)G.s0 * b]);
}

// The layout on the host: n_unique[s] by one pass over the indexes, sub_off[s] = byte offset of the list of sub-proof s
// (sub_off[n_sub] = the total length), ref[s * b + e].  sub_off / ref may be null.  The caller has checked the indexes.
static uint64_t scompact_layout(const SCompactPlan& P, size_t b, const uint64_t* idx, uint64_t* sub_off, uint32_t* ref) {
    uint64_t at = 0;
    for (uint32_t s = 0; s < P.V.n_sub; s++) {
        if (sub_off) sub_off[s] = at;
        uint64_t u = 0;
        for (size_t e = 0; e < b; e++) {
            u += scompact_key_head(idx, e, P.shift[s]) ? 1 : 0;
            if (ref) ref[(size_t)s * b + e] = (uint32_t)(u - 1);
        }
        at += u * (uint64_t)P.V.pieces[s] * 16;
    }
    if (sub_off) sub_off[P.V.n_sub] = at;
    return at;
}
// Rows [first, first + count) as per-entity blobs (dapol_entity_proof_size layout) cut out of the compact buffer.
static void scompact_expand(const SCompactPlan& P, size_t b, const uint64_t* idx, const uint8_t* compact, size_t first, size_t count, uint8_t* out) {
    const size_t es = (size_t)P.V.entity_pieces * 16;
    uint64_t at = 0;
    for (uint32_t s = 0; s < P.V.n_sub; s++) {
        const size_t ps = (size_t)P.V.pieces[s] * 16, q = (size_t)P.V.q0[s] * 16;
        uint64_t u = 0;
        for (size_t e = 0; e < b; e++) {
            u += scompact_key_head(idx, e, P.shift[s]) ? 1 : 0;
            if (e >= first && e - first < count) memcpy(out + (e - first) * es + q, compact + at + (u - 1) * ps, ps);
        }
        at += u * ps;
    }
}
// The inverse for a caller who holds expanded blobs: the bytes of the first row of every run of equal keys; the other rows are not read.
static void scompact_compress(const SCompactPlan& P, size_t b, const uint64_t* idx, const uint8_t* blobs, uint8_t* compact) {
    const size_t es = (size_t)P.V.entity_pieces * 16;
    uint64_t at = 0;
    for (uint32_t s = 0; s < P.V.n_sub; s++) {
        const size_t ps = (size_t)P.V.pieces[s] * 16, q = (size_t)P.V.q0[s] * 16;
        for (size_t e = 0; e < b; e++)
            if (scompact_key_head(idx, e, P.shift[s])) { memcpy(compact + at, blobs + e * es + q, ps); at += ps; }
    }
}

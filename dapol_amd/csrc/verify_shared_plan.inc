// dapol_verify_entities_shared as index arithmetic: where each sub-proof of the plan lies inside an entity's blob and which sibling
// commitments it covers, the groups (runs of equal m) and their offsets in the compact buffers, the is-head predicate over two rows,
// and the way from a rank to a compact row and back to an entity's verdict.  Pure functions, no HIP call: the kernels
// (kernels_verify_shared.h) and the host side (host_verify_shared.inc) call them, and tests/cpp/verify_shared_host.cpp replays them
// on the CPU under ASan + UBSan against a brute force (tests/test_verify_shared_cpu.py).  The includer provides the DAPOL_POLICY_*
// constants (include/dapol_hip.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "policy_plan.inc"

#if defined(__HIPCC__)
#define VSP_HD __host__ __device__ __forceinline__
#else
#define VSP_HD inline
#endif

enum { VSHARED_MAX_SUB = 96, VSHARED_MAX_GROUPS = 16 };
enum { VSHARED_FORWARD_MAX = 64 };        // b x plan size up to which a call is the latency regime of verify_policy_device: nothing to gain

// Everything is moved and compared in 16-byte PIECES: a proof of 32 (9 + 2 lg) bytes is 2 (9 + 2 lg) of them, a commitment is 2.
struct alignas(16) VsPiece { uint32_t w[4]; };

// A GROUP is a run of the plan's sub-proofs of equal m (they may have count < m: the gather writes the pads): its distinct rows are
// one batch of the range verifier.
struct VSharedGroup {
    uint32_t s0, k;          // its sub-proofs: s0 .. s0 + k - 1 of the plan
    uint32_t m;              // parties of each
    uint32_t pieces;         // pieces of one proof
    uint32_t q0;             // first piece of sub-proof s0 inside an entity's blob
};
struct VSharedPlan {
    uint32_t n_sub, n_groups;
    uint32_t H;                              // sibling commitments per entity
    uint32_t entity_pieces;                  // pieces of one entity's blob
    uint32_t q0[VSHARED_MAX_SUB];            // first piece of sub-proof s inside the blob
    uint16_t pieces[VSHARED_MAX_SUB];        // pieces of its proof
    uint8_t start[VSHARED_MAX_SUB];          // its first sibling ...
    uint8_t count[VSHARED_MAX_SUB];          // ... and how many (the other m - count parties are pads)
    VSharedGroup g[VSHARED_MAX_GROUPS];
};

// 0: built; 1: more sub-proofs than VSHARED_MAX_SUB; 2: more runs of equal m than VSHARED_MAX_GROUPS; 3: a size that does not exist
static int vshared_plan_build(const std::vector<SubProof>& plan, int H, int n_bits, VSharedPlan& P) {
    P = VSharedPlan{};
    if (plan.size() > VSHARED_MAX_SUB) return 1;
    P.n_sub = (uint32_t)plan.size(); P.H = (uint32_t)H;
    uint32_t q = 0;
    for (size_t s = 0; s < plan.size(); s++) {
        const size_t bytes = dapol_range_proof_size(n_bits, plan[s].m);
        if (bytes == 0 || plan[s].count > plan[s].m || plan[s].start + plan[s].count > H) return 3;
        const uint32_t pieces = (uint32_t)(bytes / 16);
        P.q0[s] = q; P.pieces[s] = (uint16_t)pieces;
        P.start[s] = (uint8_t)plan[s].start; P.count[s] = (uint8_t)plan[s].count;
        if (P.n_groups && P.g[P.n_groups - 1].m == (uint32_t)plan[s].m) P.g[P.n_groups - 1].k++;
        else {
            if (P.n_groups == VSHARED_MAX_GROUPS) return 2;
            VSharedGroup& G = P.g[P.n_groups++];
            G.s0 = (uint32_t)s; G.k = 1; G.m = (uint32_t)plan[s].m; G.pieces = pieces; G.q0 = q;
        }
        q += pieces;
    }
    P.entity_pieces = q;
    return 0;
}

// Entities x (plan size + 1) flags must be countable in 32 bits (the ranks are 32-bit, as the prover's).
static inline bool vshared_call_fits(size_t b, size_t n_sub) { return (uint64_t)b < (1ull << 32) && (uint64_t)b * (uint64_t)(n_sub + 1) < (1ull << 32); }
// ... and the gather of the largest group must fit a launch: one lane per piece of every (sub-proof, row) of the group.
static inline bool vshared_gather_fits(const VSharedPlan& P, size_t b) {
    for (uint32_t gi = 0; gi < P.n_groups; gi++)
        if (b * (size_t)P.g[gi].k * (size_t)(P.g[gi].pieces + 2u * P.g[gi].m) / 256 >= 0x7fffffffull) return false;
    return true;
}
static inline bool vshared_forwards(size_t b, size_t n_sub, size_t forward_max) { return (uint64_t)b * (uint64_t)n_sub <= (uint64_t)forward_max; }

// What the range check of sub-proof s reads of a row: its proof's pieces, then two pieces per sibling commitment it covers.
VSP_HD uint32_t vshared_span_pieces(const VSharedPlan& P, uint32_t s) { return (uint32_t)P.pieces[s] + 2u * (uint32_t)P.count[s]; }
// Piece t < vshared_span_pieces of that span in rows a and b (blob: the row's P.entity_pieces pieces; C: its 2 H commitment pieces):
// zero iff the two rows agree there.
VSP_HD uint32_t vshared_piece_diff(const VSharedPlan& P, uint32_t s, const VsPiece* blob_a, const VsPiece* blob_b, const VsPiece* C_a,
                                   const VsPiece* C_b, uint32_t t) {
    const uint32_t np = P.pieces[s];
    const size_t at = t < np ? (size_t)P.q0[s] + t : 2 * (size_t)P.start[s] + (t - np);
    const VsPiece x = t < np ? blob_a[at] : C_a[at], y = t < np ? blob_b[at] : C_b[at];
    return (x.w[0] ^ y.w[0]) | (x.w[1] ^ y.w[1]) | (x.w[2] ^ y.w[2]) | (x.w[3] ^ y.w[3]);
}
// Rows e >= 1 and e - 1 of the uploaded arrays (blobs: [b][entity_pieces], pC: [b][2 H] pieces), and the OR of the differences over
// pieces t0, t0 + step, ... of the span of sub-proof s: a lane's share in k_vshared_heads, the whole span with (0, 1).
struct VsRowPair { const VsPiece *blob_a, *blob_b, *C_a, *C_b; };
VSP_HD VsRowPair vshared_row_pair(const VSharedPlan& P, size_t e, const VsPiece* blobs, const VsPiece* pC) {
    const VsPiece* ba = blobs + e * (size_t)P.entity_pieces;
    const VsPiece* ca = pC + e * 2 * (size_t)P.H;
    return {ba, ba - P.entity_pieces, ca, ca - 2 * (size_t)P.H};
}
VSP_HD uint32_t vshared_rows_diff(const VSharedPlan& P, uint32_t s, size_t e, const VsPiece* blobs, const VsPiece* pC, uint32_t t0, uint32_t step) {
    const VsRowPair R = vshared_row_pair(P, e, blobs, pC);
    uint32_t d = 0;
    for (uint32_t t = t0, n = vshared_span_pieces(P, s); t < n; t += step) d |= vshared_piece_diff(P, s, R.blob_a, R.blob_b, R.C_a, R.C_b, t);
    return d;
}
// Row e of sub-proof s is a HEAD unless it repeats row e - 1 over the whole span (row 0 always is one).
VSP_HD bool vshared_is_head(const VSharedPlan& P, uint32_t s, size_t e, const VsPiece* blobs, const VsPiece* pC) {
    return e == 0 || vshared_rows_diff(P, s, e, blobs, pC, 0, 1) != 0;
}

// rank = the inclusive scan of flag[s][e] in plan order (s-major).  The head that (s, e) belongs to -- itself, or the head of its run --
// has compact row rank[s][e] - 1 over the whole call, and rank[s][e] - rank[s0][0] inside its group (row 0 of s0 is a head).
VSP_HD size_t vshared_row(const uint32_t* rank, size_t b, uint32_t s, size_t e) { return (size_t)rank[(size_t)s * b + e] - 1; }
VSP_HD size_t vshared_group_row(const VSharedGroup& G, const uint32_t* rank, size_t b, uint32_t s, size_t e) {
    return (size_t)(rank[(size_t)s * b + e] - rank[(size_t)G.s0 * b]);
}
// sub: one verdict byte per head, in compact-row order over the whole call.  The entity's range verdict is the AND over its sub-proofs.
VSP_HD uint8_t vshared_verdict(const VSharedPlan& P, size_t b, const uint32_t* rank, const uint8_t* sub, size_t e) {
    uint8_t ok = 1;
    for (uint32_t s = 0; s < P.n_sub; s++) ok &= sub[vshared_row(rank, b, s, e)] ? 1 : 0;
    return ok;
}

// One lane of the gather of group G: lane t takes piece `piece` of the span of (s, e), proof pieces first, then 2 m party pieces
// (pads included).  false: t is beyond the group.
struct VsGatherLane { size_t e; uint32_t s, piece; };
VSP_HD uint32_t vshared_gather_pieces(const VSharedGroup& G) { return G.pieces + 2u * G.m; }
VSP_HD bool vshared_gather_lane(const VSharedGroup& G, size_t b, size_t t, VsGatherLane& L) {
    const uint32_t tp = vshared_gather_pieces(G);
    if (t >= b * (size_t)G.k * (size_t)tp) return false;
    const size_t p = t / tp;
    L.piece = (uint32_t)(t - p * tp);
    L.e = p / G.k;
    L.s = G.s0 + (uint32_t)(p - L.e * G.k);
    return true;
}

// Where the groups' distinct rows lie in the compact buffers.  rank_at[gi] = rank[g[gi].s0][0] for gi < n_groups, rank_at[n_groups] =
// the scan's last element (the closing zero flag: all heads).
struct VSharedLayout {
    size_t first[VSHARED_MAX_GROUPS + 1];        // compact row at which each group starts; the last one: all heads
    size_t piece_off[VSHARED_MAX_GROUPS];        // its proofs in the compact proof buffer (pieces)
    size_t party_off[VSHARED_MAX_GROUPS];        // its parties in the compact commitment buffer (32-byte records)
    size_t pieces, parties;                      // totals
};
static void vshared_layout(const VSharedPlan& P, const uint32_t* rank_at, VSharedLayout& L) {
    L = VSharedLayout{};
    for (uint32_t gi = 0; gi < P.n_groups; gi++) L.first[gi] = (size_t)rank_at[gi] - 1;
    L.first[P.n_groups] = rank_at[P.n_groups];
    for (uint32_t gi = 0; gi < P.n_groups; gi++) {
        const size_t U = L.first[gi + 1] - L.first[gi];
        L.piece_off[gi] = L.pieces; L.party_off[gi] = L.parties;
        L.pieces += U * (size_t)P.g[gi].pieces; L.parties += U * (size_t)P.g[gi].m;
    }
}

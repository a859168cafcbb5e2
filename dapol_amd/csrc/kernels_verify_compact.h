// Compact shared proofs on the verifier's side (host_verify_compact.inc: dapol_verify_entities_compact): the caller uploads every
// distinct sub-proof once (shared_compact_plan.inc: the layout) and the per-entity sibling commitments; nothing but bytes is trusted.
//   k_vcompact_heads    two flags per (sub-proof, row) in one pass: the KEY flag (the prover's shared_key rule over the leaf indexes --
//                       its scan names the row of the compact buffer) and the HEAD flag (key flag, or a covered commitment that
//                       differs from the row before -- its scan names the row of the verification batch);
//   k_vcompact_gather   the head rows copy their proof from the compact buffer and their parties from their own commitments (pads =
//                       the compressed blinding base) into [V][pieces] / [V][m] batches, one batch of the range verifier per group;
//   k_vcompact_verdict  every entity takes the AND of the verdicts of the heads of its sub-proofs.
// No LDS, no atomics.  The index arithmetic is shared_compact_plan.inc's (replayed on the CPU by tests/cpp/shared_compact_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include "shared_compact_plan.inc"

namespace dapol {

enum { VCOMPACT_LANES = 16 };     // lanes per (sub-proof, row): an aggregated proof over 16 siblings covers 32 pieces, two loads a lane

// kflag[s][e] = 1 where row e opens a new subtree key of sub-proof s, hflag[s][e] = 1 where it is a head (scompact_is_head); element
// [n_sub][0] = 0 closes both arrays, so that a scan's last element is the number of ones.  A sub-group of VCOMPACT_LANES lanes strides
// over the commitment pieces of the span in both rows, ORs the differences and votes; its first lane writes.
__global__ __launch_bounds__(256) void k_vcompact_heads(SCompactPlan P, size_t b, const uint64_t* __restrict__ idx, const VsPiece* __restrict__ pC,
                                                        uint32_t* __restrict__ kflag, uint32_t* __restrict__ hflag) {
    const size_t pair = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / VCOMPACT_LANES, n = (size_t)P.V.n_sub * b;
    const uint32_t lane = threadIdx.x % VCOMPACT_LANES;
    const bool live = pair < n;
    bool key = false;
    uint32_t diff = 0;
    if (live) {
        const uint32_t s = (uint32_t)(pair / b);
        const size_t e = pair - (size_t)s * b;
        key = scompact_key_head(idx, e, P.shift[s]);
        if (e) diff = scompact_com_diff(P.V, s, e, pC, lane, VCOMPACT_LANES);
    }
    // (every lane of the wavefront arrives here: lanes beyond the array vote 0)
    const unsigned long long vote = __ballot(diff != 0);
    if (lane) return;
    const unsigned first = (threadIdx.x & 63u) & ~(unsigned)(VCOMPACT_LANES - 1);
    if (live) {
        kflag[pair] = key ? 1u : 0u;
        hflag[pair] = (key || ((vote >> first) & ((1ull << VCOMPACT_LANES) - 1))) ? 1u : 0u;
    } else if (pair == n) {
        kflag[pair] = 0;
        hflag[pair] = 0;
    }
}

// The head rows of group gi: consecutive lanes take consecutive pieces of (s, e) -- its proof, then its m parties.  The proof comes
// from row kref[s][e] - kref[s0][0] of the group's slice `cproofs` of the uploaded compact buffer, the parties from the row's own
// commitments; both go to row hrank[s][e] - hrank[s0][0] of the group's slices `proofs` ([V][pieces]) and `Vc` ([V][m], 2 pieces a
// party).  On honest input V = U and the proof part is a straight copy.
__global__ __launch_bounds__(256) void k_vcompact_gather(SCompactPlan P, uint32_t gi, size_t b, const uint32_t* __restrict__ hflag,
                                                         const uint32_t* __restrict__ kref, const uint32_t* __restrict__ hrank,
                                                         const VsPiece* __restrict__ cproofs, const VsPiece* __restrict__ pC,
                                                         const uint32_t* __restrict__ Bb_comp, VsPiece* __restrict__ proofs, VsPiece* __restrict__ Vc) {
    const VSharedGroup G = P.V.g[gi];
    VsGatherLane L;
    if (!vshared_gather_lane(G, b, (size_t)blockIdx.x * blockDim.x + threadIdx.x, L)) return;
    if (!hflag[(size_t)L.s * b + L.e]) return;
    const size_t row = vshared_group_row(G, hrank, b, L.s, L.e);
    if (L.piece < G.pieces) {
        proofs[row * G.pieces + L.piece] = cproofs[scompact_group_ref(G, kref, b, L.s, L.e) * G.pieces + L.piece];
        return;
    }
    const uint32_t pp = L.piece - G.pieces, jj = pp >> 1, half = pp & 1;
    VsPiece c;
    if (jj < P.V.count[L.s]) c = pC[(L.e * (size_t)P.V.H + (size_t)(P.V.start[L.s] + jj)) * 2 + half];
    else for (int i = 0; i < 4; i++) c.w[i] = Bb_comp[4 * half + i];
    Vc[(row * G.m + jj) * 2 + half] = c;
}

// ok[e] = AND over the plan's sub-proofs of the verdict at hrank[s][e] - 1 (sub: a byte per head, verification-row order).
__global__ __launch_bounds__(256) void k_vcompact_verdict(SCompactPlan P, size_t b, const uint32_t* __restrict__ hrank, const uint8_t* __restrict__ sub,
                                                          uint8_t* __restrict__ ok) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < b) ok[e] = vshared_verdict(P.V, b, hrank, sub, e);
}

}  // namespace dapol

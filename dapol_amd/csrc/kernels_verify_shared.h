// Shared sub-proofs on the verifier's side (host_verify_shared.inc: dapol_verify_entities_shared): a sub-proof whose bytes AND whose
// sibling commitments repeat those of the row before it gets that row's verdict, so a call checks each run of equal rows once.
//   k_vshared_heads    which (sub-proof, row) pairs differ from the row before -- compared in the uploaded arena, 16 bytes a lane;
//                      an inclusive scan of the flags (rocprim, host side) turns them into the row of the compact buffers;
//   k_vshared_gather   the head rows copy their proof and their parties (pads = the compressed blinding base) into compact
//                      [U][pieces] / [U][m] buffers, one batch of the range verifier per group;
//   k_vshared_verdict  every entity takes the AND of the verdicts of the heads of its sub-proofs.
// No LDS, no atomics.  The index arithmetic is verify_shared_plan.inc's (replayed on the CPU by tests/cpp/verify_shared_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include "verify_shared_plan.inc"

namespace dapol {

enum { VSHARED_LANES = 16 };      // lanes per (sub-proof, row): a 672-byte proof + one commitment is 44 pieces, three loads a lane

// flag[s][e] = 1 where row e of sub-proof s is a head (vshared_is_head); flag[n_sub][0] = 0 closes the array, so that the scan's
// last element is the number of heads.  A sub-group of VSHARED_LANES lanes strides over the pieces of the span in both rows, ORs
// the differences and votes; its first lane writes.  Memory-bound: every blob is read twice, the second time from the cache.
__global__ __launch_bounds__(256) void k_vshared_heads(VSharedPlan P, size_t b, const VsPiece* __restrict__ blobs, const VsPiece* __restrict__ pC,
                                                       uint32_t* __restrict__ flag) {
    const size_t pair = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / VSHARED_LANES, n = (size_t)P.n_sub * b;
    const uint32_t lane = threadIdx.x % VSHARED_LANES;
    const bool live = pair < n;
    size_t e = 0;
    uint32_t diff = 0;
    if (live) {
        const uint32_t s = (uint32_t)(pair / b);
        e = pair - (size_t)s * b;
        if (e) diff = vshared_rows_diff(P, s, e, blobs, pC, lane, VSHARED_LANES);
    }
    // (every lane of the wavefront arrives here: lanes beyond the array vote 0)
    const unsigned long long vote = __ballot(diff != 0);
    if (lane) return;
    const unsigned first = (threadIdx.x & 63u) & ~(unsigned)(VSHARED_LANES - 1);
    if (live) flag[pair] = (e == 0 || ((vote >> first) & ((1ull << VSHARED_LANES) - 1))) ? 1u : 0u;
    else if (pair == n) flag[pair] = 0;
}

// The head rows of group gi: consecutive lanes take consecutive pieces of (s, e) -- its proof, then its m parties -- and write them
// at compact row rank[s][e] - rank[s0][0] of the group's slices `proofs` ([U][pieces]) and `Vc` ([U][m], 2 pieces a party).
__global__ __launch_bounds__(256) void k_vshared_gather(VSharedPlan P, uint32_t gi, size_t b, const uint32_t* __restrict__ flag,
                                                        const uint32_t* __restrict__ rank, const VsPiece* __restrict__ blobs,
                                                        const VsPiece* __restrict__ pC, const uint32_t* __restrict__ Bb_comp,
                                                        VsPiece* __restrict__ proofs, VsPiece* __restrict__ Vc) {
    const VSharedGroup G = P.g[gi];
    VsGatherLane L;
    if (!vshared_gather_lane(G, b, (size_t)blockIdx.x * blockDim.x + threadIdx.x, L)) return;
    if (!flag[(size_t)L.s * b + L.e]) return;
    const size_t row = vshared_group_row(G, rank, b, L.s, L.e);
    if (L.piece < G.pieces) {
        proofs[row * G.pieces + L.piece] = blobs[L.e * (size_t)P.entity_pieces + P.q0[L.s] + L.piece];
        return;
    }
    const uint32_t pp = L.piece - G.pieces, jj = pp >> 1, half = pp & 1;
    VsPiece c;
    if (jj < P.count[L.s]) c = pC[(L.e * (size_t)P.H + (size_t)(P.start[L.s] + jj)) * 2 + half];
    else for (int i = 0; i < 4; i++) c.w[i] = Bb_comp[4 * half + i];
    Vc[(row * G.m + jj) * 2 + half] = c;
}

// ok[e] = AND over the plan's sub-proofs of the verdict of the head of (s, e)'s run (sub: a byte per head, compact-row order).
__global__ __launch_bounds__(256) void k_vshared_verdict(VSharedPlan P, size_t b, const uint32_t* __restrict__ rank, const uint8_t* __restrict__ sub,
                                                         uint8_t* __restrict__ ok) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < b) ok[e] = vshared_verdict(P, b, rank, sub, e);
}

}  // namespace dapol

// Shared sub-proofs (host_shared.inc: dapol_prove_entities_shared): the sub-proofs of a policy's plan whose siblings all lie at
// depth <= D below the root are the same statement for every leaf under one depth-D node, so a call proves each of them once.
//   k_shared_heads    which (sub-proof, row) pairs open a new subtree key (the rows' leaf indexes ascend, so equal keys are adjacent);
//                     an inclusive scan of the flags (rocprim, host side) turns them into the row of the compact buffers;
//   k_shared_gather   the head rows write their parties and their stream id (the subtree key) into compact [U][m] arrays;
//   k_shared_scatter  expands the compact proofs into every entity's blob, 16 bytes a lane.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_ctx_tree.h"

namespace dapol {

enum { SHARED_MAX_SUB = 96, SHARED_MAX_GROUPS = 16 };
// A GROUP is a run of the plan's sub-proofs of equal size m: its distinct rows are one call of the range prover.
struct SharedGroup {
    uint32_t s0, k;          // its sub-proofs: s0 .. s0 + k - 1 of the plan
    uint32_t m;              // parties of each
    uint32_t pieces;         // 16-byte pieces of one proof
    uint32_t q0;             // first piece of sub-proof s0 inside an entity's blob
    uint32_t pad_;
    size_t word_off;         // where the group's proofs start in the compact proof buffer (32-bit words)
};
struct SharedPlanDev {
    uint32_t n_sub, n_groups;
    uint32_t H;                          // siblings per entity
    uint32_t entity_pieces;              // 16-byte pieces of one entity's blob
    uint8_t shift[SHARED_MAX_SUB];       // low bits of the leaf index that the subtree key clears: H - D (64: the key is 0)
    uint8_t start[SHARED_MAX_SUB];       // first sibling of the sub-proof
    uint8_t count[SHARED_MAX_SUB];       // its siblings (the other m - count parties are pads)
    SharedGroup g[SHARED_MAX_GROUPS];
};

__device__ __forceinline__ uint64_t shared_key(uint64_t idx, uint32_t shift) { return shift >= 64 ? 0ull : (idx >> shift) << shift; }

// flag[s][e] = 1 where row e opens a new key of sub-proof s (row 0 always does); flag[n_sub][0] = 0 closes the array, so that the
// scan's last element is the number of heads.
__global__ __launch_bounds__(256) void k_shared_heads(SharedPlanDev P, size_t b, const uint64_t* __restrict__ idx, uint32_t* __restrict__ flag) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n = (size_t)P.n_sub * b;
    if (t > n) return;
    if (t == n) { flag[t] = 0; return; }
    const size_t s = t / b, e = t - s * b;
    const uint32_t sh = P.shift[s];
    flag[t] = (e == 0 || shared_key(idx[e], sh) != shared_key(idx[e - 1], sh)) ? 1u : 0u;
}

// Parties of the head rows of group gi, as k_gather_parties lays them.  rank = the inclusive scan of the flags: the statement of
// (s, e) sits at compact row rank[s][e] - rank[s0][0] of its group (the group's first element is a head, of rank one more than the
// heads before the group).
// vals / blind / Vc / stream point at the group's own slice.
__global__ __launch_bounds__(256) void k_shared_gather(SharedPlanDev P, uint32_t gi, size_t b, const uint64_t* __restrict__ idx,
                                                       const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank,
                                                       const uint64_t* __restrict__ pv, const uint32_t* __restrict__ pr,
                                                       const uint32_t* __restrict__ pC, const uint32_t* __restrict__ Bb_comp,
                                                       uint64_t* __restrict__ vals, uint32_t* __restrict__ blind, uint32_t* __restrict__ Vc,
                                                       uint64_t* __restrict__ stream) {
    const SharedGroup G = P.g[gi];
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b * (size_t)G.k * (size_t)G.m) return;
    const size_t p = t / G.m, e = p / G.k;
    const uint32_t jj = (uint32_t)(t - p * G.m), s = G.s0 + (uint32_t)(p - e * G.k);
    const size_t f = (size_t)s * b + e;
    if (!flag[f]) return;
    const size_t row = (size_t)(rank[f] - rank[(size_t)G.s0 * b]), o = row * G.m + jj;
    uint32_t r[8] = {1, 0, 0, 0, 0, 0, 0, 0}, c[8];
    uint64_t v = 0;
    if (jj < P.count[s]) {
        const size_t sib = e * (size_t)P.H + (size_t)(P.start[s] + jj);
        v = pv[sib];
        ld8(r, pr + sib * 8);
        ld8(c, pC + sib * 8);
    } else {
        for (int i = 0; i < 8; i++) c[i] = Bb_comp[i];
    }
    vals[o] = v;
    st8(blind + o * 8, r);
    st8(Vc + o * 8, c);
    if (jj == 0) stream[row] = shared_key(idx[e], P.shift[s]);
}

// out[e] = the entity's blob: piece q of it is piece (q - q0) % pieces of the proof at compact row rank[s][e] of its group.
// Consecutive lanes take consecutive 16-byte pieces: the stores of a launch are one contiguous stream, the loads of the lanes inside
// one proof are contiguous too (a 672-byte proof is 42 pieces, so a wavefront touches two or three proofs).
__global__ __launch_bounds__(256) void k_shared_scatter(SharedPlanDev P, size_t b, const uint32_t* __restrict__ rank,
                                                        const uint4* __restrict__ proofs, uint4* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b * (size_t)P.entity_pieces) return;
    const size_t e = t / P.entity_pieces;
    const uint32_t q = (uint32_t)(t - e * P.entity_pieces);
    uint32_t gi = 0;
    while (gi + 1 < P.n_groups && q >= P.g[gi + 1].q0) gi++;
    const SharedGroup G = P.g[gi];
    const uint32_t j = (q - G.q0) / G.pieces, piece = (q - G.q0) - j * G.pieces;
    const size_t row = (size_t)(rank[(size_t)(G.s0 + j) * b + e] - rank[(size_t)G.s0 * b]);
    out[t] = proofs[G.word_off / 4 + row * G.pieces + piece];
}

}  // namespace dapol

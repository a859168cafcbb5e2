// Re-proving after an edit of the tree (host_reprove.inc: dapol_reprove_entities_shared): a sub-proof whose sibling commitments are
// byte for byte those the caller's old proof was made over keeps its old bytes; the others are proven once per run of equal subtree
// keys, as dapol_prove_entities_shared proves them.
//   k_reprove_heads    which (sub-proof, row) pairs are DIRTY (no old row, or old commitments that differ from the tree's -- compared
//                      where they were uploaded, 16 bytes a lane) and which of those are HEADS (the first dirty row of a run of equal
//                      keys); an inclusive scan of the head flags (rocprim, host side) gives the row of the compact buffers;
//   k_reprove_gather   the head rows write their parties and their stream id (the subtree key) into compact [U][m] arrays;
//   k_reprove_scatter  the dirty rows copy their proof from its compact row over the old bytes, 16 bytes a lane; kept rows are not
//                      touched.
// No LDS, no atomics.  The index arithmetic is reprove_plan.inc's.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_shared.h"
#include "reprove_plan.inc"

namespace dapol {

enum { REPROVE_LANES = 16 };      // lanes per (sub-proof, row): an aggregated sub-proof of 32 siblings is 64 pieces, four loads a lane
static_assert(REPROVE_MAX_GROUPS == SHARED_MAX_GROUPS, "one layout entry per group of the shared plan");

struct ReproveBases { uint32_t before[SHARED_MAX_GROUPS]; };      // heads before each group (reprove_group_row)

// OR of the differences between the old and the new commitments of sub-proof s in row e over pieces t0, t0 + step, ... (a commitment
// is two pieces; C_old / C_new: [b][2 H] pieces).
__device__ __forceinline__ uint32_t reprove_row_diff(const SharedPlanDev& P, uint32_t s, size_t e, const uint4* __restrict__ C_old,
                                                     const uint4* __restrict__ C_new, uint32_t t0, uint32_t step) {
    const size_t at = e * 2 * (size_t)P.H + 2 * (size_t)P.start[s];
    uint32_t d = 0;
    for (uint32_t t = t0, n = 2u * P.count[s]; t < n; t += step) {
        const uint4 x = C_old[at + t], y = C_new[at + t];
        d |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
    }
    return d;
}

// dirty[s][e] and flag[s][e] (the head flag); flag[n_sub][0] = 0 closes the array, so that the scan's last element is the number of
// heads.  A sub-group of REPROVE_LANES lanes strides over the pieces of the sub-proof's commitments in row e and -- where row e - 1
// has the same key, so that its dirtiness decides whether e is a head -- in row e - 1, ORs the differences and votes; its first lane
// writes.  has_old may be null (every row has old data); C_old may be null when no row has.
__global__ __launch_bounds__(256) void k_reprove_heads(SharedPlanDev P, size_t b, const uint64_t* __restrict__ idx, const uint8_t* __restrict__ has_old,
                                                       const uint4* __restrict__ C_old, const uint4* __restrict__ C_new, uint32_t* __restrict__ dirty,
                                                       uint32_t* __restrict__ flag) {
    const size_t pair = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / REPROVE_LANES, n = (size_t)P.n_sub * b;
    const uint32_t lane = threadIdx.x % REPROVE_LANES;
    const bool live = pair < n;
    bool old_e = false, old_p = false, run = false;               // row e / row e - 1 has old data; e - 1 exists and has e's key
    uint32_t diff_e = 0, diff_p = 0;
    if (live) {
        const uint32_t s = (uint32_t)(pair / b);
        const size_t e = pair - (size_t)s * b;
        old_e = !has_old || has_old[e];
        if (old_e) diff_e = reprove_row_diff(P, s, e, C_old, C_new, lane, REPROVE_LANES);
        run = e > 0 && shared_key(idx[e], P.shift[s]) == shared_key(idx[e - 1], P.shift[s]);
        if (run) {
            old_p = !has_old || has_old[e - 1];
            if (old_p) diff_p = reprove_row_diff(P, s, e - 1, C_old, C_new, lane, REPROVE_LANES);
        }
    }
    // (every lane of the wavefront arrives here: lanes beyond the array vote 0)
    const unsigned long long vote_e = __ballot(diff_e != 0), vote_p = __ballot(diff_p != 0);
    if (lane) return;
    const unsigned first = (threadIdx.x & 63u) & ~(unsigned)(REPROVE_LANES - 1);
    const unsigned long long mask = (1ull << REPROVE_LANES) - 1;
    if (live) {
        const bool dirty_e = !old_e || ((vote_e >> first) & mask) != 0;
        const bool dirty_p = run && (!old_p || ((vote_p >> first) & mask) != 0);
        dirty[pair] = dirty_e ? 1u : 0u;
        flag[pair] = (dirty_e && !dirty_p) ? 1u : 0u;
    } else if (pair == n) flag[pair] = 0;
}

// Parties of the head rows of group gi, as k_shared_gather lays them, at compact row reprove_group_row of the group's own slices.
__global__ __launch_bounds__(256) void k_reprove_gather(SharedPlanDev P, uint32_t gi, uint32_t heads_before, size_t b, const uint64_t* __restrict__ idx,
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
    const size_t row = reprove_group_row(rank[f], heads_before), o = row * G.m + jj;
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

// out = the old blobs as uploaded: piece q of a DIRTY (s, e) is overwritten with piece (q - q0) % pieces of the proof at the compact
// row of the head of its run; a kept (s, e) is left alone.  Consecutive lanes take consecutive 16-byte pieces, as k_shared_scatter.
__global__ __launch_bounds__(256) void k_reprove_scatter(SharedPlanDev P, ReproveBases B, size_t b, const uint32_t* __restrict__ dirty,
                                                         const uint32_t* __restrict__ rank, const uint4* __restrict__ proofs, uint4* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b * (size_t)P.entity_pieces) return;
    const size_t e = t / P.entity_pieces;
    const uint32_t q = (uint32_t)(t - e * P.entity_pieces);
    uint32_t gi = 0;
    while (gi + 1 < P.n_groups && q >= P.g[gi + 1].q0) gi++;
    const SharedGroup G = P.g[gi];
    const uint32_t j = (q - G.q0) / G.pieces, piece = (q - G.q0) - j * G.pieces;
    const size_t f = (size_t)(G.s0 + j) * b + e;
    if (!dirty[f]) return;
    out[t] = proofs[G.word_off / 4 + reprove_group_row(rank[f], B.before[gi]) * G.pieces + piece];
}

}  // namespace dapol

// The device-resident proof store (host_store.inc: dapol_proof_store_*): rows of [leaf index | H sibling commitments | H sibling hashes |
// range-proof blob], sorted by leaf index, kept in HBM between calls.  The proving is kernels_reprove.h's; these kernels only find and
// move rows.  They are bandwidth-bound copies: a lane per 16-byte piece, consecutive lanes on consecutive pieces of a destination row.
//   k_store_align   a lane per NEW row: the old row that holds its leaf (binary search of the old sorted indexes), or none;
//   k_store_move    rows that continue an old row copy its blob into the new blob buffer and its commitments into the compare buffer
//                   of k_reprove_heads; rows without an old row are not written (every sub-proof of them is dirty: k_reprove_scatter
//                   writes every piece);
//   k_store_find    a lane per query: its row, or none;
//   k_store_fetch   the rows of the queries gathered into a staging buffer, zero for "none";
//   k_store_leaves  the leaves' own commitments and hashes from level 0 of the tree (dapol_proof_store_verify);
//   k_store_compact the key-head rows' sub-proofs gathered out of the blobs into the compact layout (dapol_proof_store_read_compact).
// No LDS, no atomics.  All index arithmetic is in size_t: 2^22 rows of 24 KB are more than 2^32 pieces.  The searches are store_plan.inc's.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_shared.h"
#include "store_plan.inc"

namespace dapol {

// src[e] = the old row of new_idx[e] or STORE_NONE; has_old[e] (a byte, k_reprove_heads' has_old) and flag[e] (a word, for the scan that
// counts them) = 1 where there is one.
__global__ __launch_bounds__(256) void k_store_align(size_t b, const uint64_t* __restrict__ new_idx, size_t n_old, const uint64_t* __restrict__ old_idx,
                                                     uint32_t* __restrict__ src, uint8_t* __restrict__ has_old, uint32_t* __restrict__ flag) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= b) return;
    const uint32_t row = store_row_of(old_idx, n_old, new_idx[e]);
    src[e] = row;
    has_old[e] = row != STORE_NONE ? 1 : 0;
    flag[e] = row != STORE_NONE ? 1u : 0u;
}

// Piece q of new row e: q < ep is piece q of the blob (ep = 16-byte pieces of an entity's blob), the others are the 2 H pieces of the
// row's commitments (cp = 2 H).  old_range / new_range: [rows][ep], old_C / cmp_C: [rows][cp].
__global__ __launch_bounds__(256) void k_store_move(size_t b, size_t ep, size_t cp, const uint32_t* __restrict__ src, const uint4* __restrict__ old_range,
                                                    const uint4* __restrict__ old_C, uint4* __restrict__ new_range, uint4* __restrict__ cmp_C) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, per = ep + cp;
    if (t >= b * per) return;
    const size_t e = t / per, q = t - e * per;
    const uint32_t row = src[e];
    if (row == STORE_NONE) return;
    if (q < ep) new_range[e * ep + q] = old_range[(size_t)row * ep + q];
    else cmp_C[e * cp + (q - ep)] = old_C[(size_t)row * cp + (q - ep)];
}

__global__ __launch_bounds__(256) void k_store_find(size_t k, const uint64_t* __restrict__ want, size_t n, const uint64_t* __restrict__ idx,
                                                    uint32_t* __restrict__ row, uint8_t* __restrict__ found) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    const uint32_t r = store_row_of(idx, n, want[i]);
    row[i] = r;
    found[i] = r != STORE_NONE ? 1 : 0;
}

// Piece q of query i, in the order blob (ep pieces), commitments (cp = 2 H), hashes (hp = H x hash words / 4): copied from row[i] of the
// store's arrays into row i of the staging arrays, or zero where the store does not hold the leaf.
__global__ __launch_bounds__(256) void k_store_fetch(size_t k, size_t ep, size_t cp, size_t hp, const uint32_t* __restrict__ row,
                                                     const uint4* __restrict__ range, const uint4* __restrict__ C, const uint4* __restrict__ Hh,
                                                     uint4* __restrict__ out_range, uint4* __restrict__ out_C, uint4* __restrict__ out_H) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, per = ep + cp + hp;
    if (t >= k * per) return;
    const size_t i = t / per, q = t - i * per;
    const uint32_t r = row[i];
    uint4 val = make_uint4(0, 0, 0, 0);
    if (q < ep) {
        if (r != STORE_NONE) val = range[(size_t)r * ep + q];
        out_range[i * ep + q] = val;
    } else if (q < ep + cp) {
        const size_t c = q - ep;
        if (r != STORE_NONE) val = C[(size_t)r * cp + c];
        out_C[i * cp + c] = val;
    } else {
        const size_t h = q - ep - cp;
        if (r != STORE_NONE) val = Hh[(size_t)r * hp + h];
        out_H[i * hp + h] = val;
    }
}

// Leaf e of the store sits at position pos[e] of the tree's level 0: its commitment (2 pieces) and its hash (hq = hash words / 4 pieces).
__global__ __launch_bounds__(256) void k_store_leaves(size_t b, size_t hq, const uint32_t* __restrict__ pos, const uint4* __restrict__ C0,
                                                      const uint4* __restrict__ H0, uint4* __restrict__ leaf_C, uint4* __restrict__ leaf_H) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, per = 2 + hq;
    if (t >= b * per) return;
    const size_t e = t / per, q = t - e * per;
    const size_t p = pos[e];
    if (q < 2) leaf_C[e * 2 + q] = C0[p * 2 + q];
    else leaf_H[e * hq + (q - 2)] = H0[p * hq + (q - 2)];
}

// dapol_proof_store_read_compact: k_shared_scatter the other way round.  Piece q of row e's blob belongs to sub-proof s of group G; where
// (s, e) is a key head (flag, k_shared_heads over the stored indexes) it goes to compact row rank[s][e] - rank[s0][0] of the group's
// slice of the staging buffer, which has exactly the compact length.  The other rows' pieces are copies and are not read.
__global__ __launch_bounds__(256) void k_store_compact(SharedPlanDev P, size_t b, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank,
                                                       const uint4* __restrict__ blobs, uint4* __restrict__ compact) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b * (size_t)P.entity_pieces) return;
    const size_t e = t / P.entity_pieces;
    const uint32_t q = (uint32_t)(t - e * P.entity_pieces);
    uint32_t gi = 0;
    while (gi + 1 < P.n_groups && q >= P.g[gi + 1].q0) gi++;
    const SharedGroup G = P.g[gi];
    const uint32_t j = (q - G.q0) / G.pieces, piece = (q - G.q0) - j * G.pieces;
    const size_t f = (size_t)(G.s0 + j) * b + e;
    if (!flag[f]) return;
    const size_t row = (size_t)(rank[f] - rank[(size_t)G.s0 * b]);
    compact[G.word_off / 4 + row * G.pieces + piece] = blobs[t];
}

}  // namespace dapol

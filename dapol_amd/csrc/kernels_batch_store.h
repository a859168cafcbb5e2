// The device-resident store of batch proofs (host_batch_store.inc: dapol_batch_store_*): rows of [leaf list | S sibling commitments | S
// sibling hashes | range-proof blob] of VARIABLE length, in the caller's batch order at dapol_batches_plan's offsets, kept in HBM
// between calls.  The proving is kernels_reprove_batches.h's; these kernels only move rows.  They are bandwidth-bound copies: a lane per
// 16-byte piece, consecutive lanes on consecutive pieces of a destination row.
//   k_batch_store_move   rows that continue an old row copy its blob into the new blob buffer and its commitments into the compare
//                        buffer of k_reprove_batches_dirty; rows without an old row are not written (every sub-proof of them is dirty:
//                        k_reprove_batches_scatter writes every piece);
//   k_batch_store_fetch  the queried rows gathered into the staging arrays: blobs, commitments, hashes.
// The leaves' own commitments and hashes for dapol_batch_store_verify are k_store_leaves' gather (kernels_store.h), by the positions
// tree_paths_device returns.  No LDS, no atomics.  All index arithmetic is in size_t.  The row search and the source of a piece are
// batch_store_plan.inc's (the "last row with off[row] <= x" search of k_batches_scatter and reprove_batches_row).
#pragma once
#include <hip/hip_runtime.h>
#include "batch_store_plan.inc"

namespace dapol {

// New row j continues old row src[j] (BATCH_STORE_NONE: none).  Lanes [0, n_blob) move blob pieces (new / old piece_off, 16-byte
// pieces), lanes [n_blob, n_blob + 2 T) the two pieces of each of the T new sibling commitments (new / old sib_off, records).
__global__ __launch_bounds__(256) void k_batch_store_move(size_t nb, size_t n_blob, size_t n_sib_pieces, const uint32_t* __restrict__ src,
                                                          const uint64_t* __restrict__ new_piece_off, const uint64_t* __restrict__ old_piece_off,
                                                          const uint64_t* __restrict__ new_sib_off, const uint64_t* __restrict__ old_sib_off,
                                                          const uint4* __restrict__ old_range, const uint4* __restrict__ old_C,
                                                          uint4* __restrict__ new_range, uint4* __restrict__ cmp_C) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_blob + n_sib_pieces) return;
    if (t < n_blob) {
        const size_t s = batch_store_piece_src(t, 1, nb, new_piece_off, src, old_piece_off);
        if (s != (size_t)-1) new_range[t] = old_range[s];
    } else {
        const size_t c = t - n_blob, s = batch_store_piece_src(c, 2, nb, new_sib_off, src, old_sib_off);
        if (s != (size_t)-1) cmp_C[c] = old_C[s];
    }
}

// Query i is row row[i] of the store (every row[i] < rows: the host has checked).  Lanes [0, n_blob) fill the staged blobs
// (q_piece_off), the next 2 T the staged commitments and the last 2 T the staged hashes (q_sib_off, records of 32 bytes).
__global__ __launch_bounds__(256) void k_batch_store_fetch(size_t k, size_t n_blob, size_t n_sib_pieces, const uint32_t* __restrict__ row,
                                                           const uint64_t* __restrict__ q_piece_off, const uint64_t* __restrict__ piece_off,
                                                           const uint64_t* __restrict__ q_sib_off, const uint64_t* __restrict__ sib_off,
                                                           const uint4* __restrict__ range, const uint4* __restrict__ C, const uint4* __restrict__ Hh,
                                                           uint4* __restrict__ out_range, uint4* __restrict__ out_C, uint4* __restrict__ out_H) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_blob + 2 * n_sib_pieces) return;
    if (t < n_blob) {
        out_range[t] = range[batch_store_piece_src(t, 1, k, q_piece_off, row, piece_off)];
    } else if (t < n_blob + n_sib_pieces) {
        const size_t c = t - n_blob;
        out_C[c] = C[batch_store_piece_src(c, 2, k, q_sib_off, row, sib_off)];
    } else {
        const size_t h = t - n_blob - n_sib_pieces;
        out_H[h] = Hh[batch_store_piece_src(h, 2, k, q_sib_off, row, sib_off)];
    }
}

}  // namespace dapol

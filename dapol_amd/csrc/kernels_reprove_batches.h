// Re-proving batches after an edit of the tree (host_reprove_batches.inc: dapol_reprove_batches): a sub-proof of a batch whose sibling
// commitments are byte for byte those the caller's old proof was made over keeps its old bytes; every other one is proved again with
// the batch's seed and stream id and its own first slot.  Everything stays in the caller's order: a PAIR is (batch, sub-proof of the
// batch's plan), pairs are numbered batch after batch (pair_off [nb + 1]), and a batch finds its plan through its S-group's slice of
// one table of ReproveBatchesEntry (ent0 [groups + 1]).
//   k_reprove_batches_dirty    which pairs are DIRTY (no old proof, or old commitments that differ from the tree's -- compared where
//                              they were uploaded, 16 bytes a lane); the flags are class-major ([m-class][pair]), so that one
//                              inclusive scan (rocprim, host side) gives every dirty pair its row among the dirty pairs of its m;
//   k_reprove_batches_gather   the dirty pairs write their parties, their batch's seed and stream id and their slot at that row;
//   k_reprove_batches_scatter  the pieces of the dirty pairs are copied from their compact row over the old bytes, 16 bytes a lane;
//                              kept pieces are not touched.
// No LDS, no atomics.  The index arithmetic is reprove_batches_plan.inc's.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_reprove.h"
#include "reprove_batches_plan.inc"

namespace dapol {

// The call as the kernels see it (all device arrays but the counts).
struct ReproveBatchesDev {
    size_t nb, n_pairs;
    const uint64_t* pair_off;                 // [nb + 1]
    const uint64_t* sib_off;                  // [nb + 1] sibling records
    const uint64_t* piece_off;                // [nb + 1] 16-byte pieces of the blobs
    const uint32_t* group_of;                 // [nb]
    const uint32_t* ent0;                     // [groups + 1]
    const ReproveBatchesEntry* tab;           // [ent0[groups]]
};

// The last row with off[row] <= x (rows that own nothing before it are skipped); off [rows + 1], off[0] = 0 <= x < off[rows].
__device__ __forceinline__ size_t reprove_batches_row(const uint64_t* __restrict__ off, size_t rows, uint64_t x) {
    size_t lo = 0, hi = rows;
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) >> 1;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// dirty[pair], and flag[cls][pair] = 1 for a dirty pair of class cls (the flags arrive zeroed, the closing zero included).  A
// sub-group of REPROVE_LANES lanes strides over the 16-byte pieces of the pair's old and new commitments, ORs the differences and
// votes; its first lane writes.  has_old may be null (every batch has an old proof); C_old may be null when no batch has.
__global__ __launch_bounds__(256) void k_reprove_batches_dirty(ReproveBatchesDev D, const uint8_t* __restrict__ has_old, const uint4* __restrict__ C_old,
                                                               const uint4* __restrict__ C_new, uint32_t* __restrict__ dirty,
                                                               uint32_t* __restrict__ flag) {
    const size_t pair = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / REPROVE_LANES;
    const uint32_t lane = threadIdx.x % REPROVE_LANES;
    const bool live = pair < D.n_pairs;
    bool old = false;
    uint32_t diff = 0, cls = 0;
    if (live) {
        const size_t j = reprove_batches_row(D.pair_off, D.nb, pair);
        const ReproveBatchesEntry E = D.tab[D.ent0[D.group_of[j]] + (uint32_t)(pair - D.pair_off[j])];
        cls = E.cls;
        old = !has_old || has_old[j];
        if (old) {
            const size_t at = 2 * ((size_t)D.sib_off[j] + E.start);
            for (uint32_t t = lane, n = 2u * E.count; t < n; t += REPROVE_LANES) {
                const uint4 x = C_old[at + t], y = C_new[at + t];
                diff |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
            }
        }
    }
    // (every lane of the wavefront arrives here: lanes beyond the array vote 0)
    const unsigned long long vote = __ballot(diff != 0);
    if (lane || !live) return;
    const unsigned first = (threadIdx.x & 63u) & ~(unsigned)(REPROVE_LANES - 1);
    const bool d = !old || ((vote >> first) & ((1ull << REPROVE_LANES) - 1)) != 0;
    dirty[pair] = d ? 1u : 0u;
    if (d) flag[reprove_batches_flag_at(cls, D.n_pairs, pair)] = 1u;
}

// Lane (pair, jj < max_m): party jj of a dirty pair at its compact row, as k_reprove_gather lays the parties (pad parties: v = 0,
// r = 1, commitment B_blinding); party 0 also writes the row's seed, stream id and first slot.  gv / gr / gC: the gathered sibling
// records in caller order; seeds [nb][8] and stream_in [nb]: k_batches_seed's rows.
__global__ __launch_bounds__(256) void k_reprove_batches_gather(ReproveBatchesDev D, ReproveBatchesClasses K, uint32_t max_m,
                                                                const uint32_t* __restrict__ dirty, const uint32_t* __restrict__ rank,
                                                                const uint64_t* __restrict__ gv, const uint32_t* __restrict__ gr,
                                                                const uint32_t* __restrict__ gC, const uint32_t* __restrict__ Bb_comp,
                                                                const uint32_t* __restrict__ seeds, const uint64_t* __restrict__ stream_in,
                                                                uint64_t* __restrict__ vals, uint32_t* __restrict__ blind, uint32_t* __restrict__ Vc,
                                                                uint32_t* __restrict__ seed_out, uint64_t* __restrict__ stream_out,
                                                                uint64_t* __restrict__ slot_out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, pair = t / max_m;
    if (pair >= D.n_pairs || !dirty[pair]) return;
    const uint32_t jj = (uint32_t)(t - pair * max_m);
    const size_t j = reprove_batches_row(D.pair_off, D.nb, pair);
    const ReproveBatchesEntry E = D.tab[D.ent0[D.group_of[j]] + (uint32_t)(pair - D.pair_off[j])];
    if (jj >= E.m) return;
    const size_t row = (size_t)rank[reprove_batches_flag_at(E.cls, D.n_pairs, pair)] - 1;        // over the whole call
    const size_t o = (size_t)K.party_off[E.cls] + (row - K.before[E.cls]) * E.m + jj;
    uint32_t r[8] = {1, 0, 0, 0, 0, 0, 0, 0}, c[8];
    uint64_t v = 0;
    if (jj < E.count) {
        const size_t sib = (size_t)D.sib_off[j] + E.start + jj;
        v = gv[sib];
        ld8(r, gr + sib * 8);
        ld8(c, gC + sib * 8);
    } else {
        for (int i = 0; i < 8; i++) c[i] = Bb_comp[i];
    }
    vals[o] = v;
    st8(blind + o * 8, r);
    st8(Vc + o * 8, c);
    if (jj == 0) {
        uint32_t s[8];
        ld8(s, seeds + j * 8);
        st8(seed_out + row * 8, s);
        stream_out[row] = stream_in[j];
        slot_out[row] = E.slot;
    }
}

// out = the old blobs as uploaded, in the caller's layout: piece t lies in batch j and in one sub-proof of its plan; if that pair is
// DIRTY the piece is overwritten from its compact row, else it is left alone.
__global__ __launch_bounds__(256) void k_reprove_batches_scatter(ReproveBatchesDev D, ReproveBatchesClasses K, size_t n_pieces,
                                                                 const uint32_t* __restrict__ dirty, const uint32_t* __restrict__ rank,
                                                                 const uint4* __restrict__ proofs, uint4* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_pieces) return;
    const size_t j = reprove_batches_row(D.piece_off, D.nb, t);
    const uint32_t q = (uint32_t)(t - D.piece_off[j]), g = D.group_of[j];
    const ReproveBatchesEntry* tab = D.tab + D.ent0[g];
    uint32_t lo = 0, hi = D.ent0[g + 1] - D.ent0[g];             // the last sub-proof with piece0 <= q
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab[mid].piece0 <= q) lo = mid; else hi = mid;
    }
    const size_t pair = (size_t)D.pair_off[j] + lo;
    if (!dirty[pair]) return;
    const ReproveBatchesEntry E = tab[lo];
    const size_t row = (size_t)rank[reprove_batches_flag_at(E.cls, D.n_pairs, pair)] - 1 - K.before[E.cls];
    out[t] = proofs[(size_t)K.piece_off[E.cls] + row * E.pieces + (q - E.piece0)];
}

}  // namespace dapol

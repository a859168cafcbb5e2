// Many multi-leaf inclusion proofs in one call (host_batches.inc: dapol_prove_batches / dapol_verify_batches).  The batches of a call
// with the same number S of deduplicated siblings share one plan, so they are the rows of ONE [b_S][S] call of the policy prover /
// verifier -- an S-GROUP; rows keep the caller's order within their group.
//   k_batches_seed     one lane per batch: its nonce seed (k_batch_seed's chain) and its stream id, at the batch's row in group order;
//   k_batches_gather   one lane per sibling record: C, H, v, r from the gathered single-leaf paths into the S-groups' arrays;
//   k_batches_scatter  16-byte pieces between group order and the caller's offsets, a lane per piece;
//   k_batches_merge    k_batch_merge over the operations of ALL batches of one level, with a bad flag per batch;
//   k_batches_roots    each batch's root slot against the root, ANDed with its range verdict.
// No LDS, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_ctx_tree.h"

namespace dapol {

// Row `pos[j]` of the [nb][8] seed array and of the stream ids belongs to batch j = leaves [off[j], off[j + 1]) of `leaf`.  A batch of
// one leaf keeps the caller's seed (its proof is dapol_prove_entities'); a longer one chains the seed through its leaves.
__global__ __launch_bounds__(64) void k_batches_seed(size_t nb, const uint32_t* __restrict__ seed8, const uint64_t* __restrict__ off,
                                                     const uint64_t* __restrict__ leaf, const uint32_t* __restrict__ pos,
                                                     uint32_t* __restrict__ seeds, uint64_t* __restrict__ stream) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nb) return;
    const uint64_t* l = leaf + off[j];
    const size_t k = (size_t)(off[j + 1] - off[j]);
    uint32_t s[8], w[16];
    for (int i = 0; i < 8; i++) s[i] = seed8[i];
    if (k > 1)
        for (size_t i = 0; i < k; i++) {
            seed_wide(w, s, 4u, l[i], (uint64_t)i);
            for (int q = 0; q < 8; q++) s[q] = w[q];
        }
    const size_t p = pos[j];
    st8(seeds + p * 8, s);
    stream[p] = l[0];
}

// Record d of the S-groups' arrays (group after group, [b_S][S] each) = record src[d] of the gathered single-leaf paths.
__global__ __launch_bounds__(256) void k_batches_gather(size_t n, const uint32_t* __restrict__ src, PathOut in, PathOut out) {
    const size_t d = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n) return;
    const size_t s = src[d];
    uint32_t w[8];
    ld8(w, in.C + s * 8); st8(out.C + d * 8, w);
    ld8(w, in.H + s * 8); st8(out.H + d * 8, w);
    ld8(w, in.r + s * 8); st8(out.r + d * 8, w);
    out.v[d] = in.v[s];
}

// Row j owns the pieces [dst_off[j], dst_off[j + 1]) x unit of dst and reads them from src_off[j] x unit on: lane t moves piece t of
// dst.  The prover's rows are the batches in caller order (dst = the caller's layout, src = group order); the verifier's are the
// well-formed batches in group order (dst = the S-groups' arrays, src = the caller's layout).  Offsets in units of `unit` pieces.
__global__ __launch_bounds__(256) void k_batches_scatter(size_t n_pieces, size_t rows, uint32_t unit, const uint64_t* __restrict__ dst_off,
                                                         const uint64_t* __restrict__ src_off, const uint4* __restrict__ src,
                                                         uint4* __restrict__ dst) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_pieces) return;
    const uint64_t rec = t / unit;
    size_t lo = 0, hi = rows;                                 // the last row with dst_off[row] <= rec (empty rows before it are skipped)
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) >> 1;
        if (dst_off[mid] <= rec) lo = mid; else hi = mid;
    }
    dst[t] = src[src_off[lo] * unit + (t - dst_off[lo] * unit)];
}

// MerkleProof::verify_batch's merges (host_batch.inc: k_batch_merge) for one level of every batch of the call.
struct BatchesMergeOp { uint32_t left, right, dst, batch; };
template <int DX>
__global__ __launch_bounds__(64) void k_batches_merge(int dg, size_t n, const BatchesMergeOp* __restrict__ ops, uint32_t* C, uint32_t* Hh, uint8_t* bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BatchesMergeOp o = ops[i];
    uint32_t cl[8], cr[8], hl[8], hr[8], cp[8], hp[8];
    ld8(cl, C + (size_t)o.left * 8); ld8(cr, C + (size_t)o.right * 8);
    ld8(hl, Hh + (size_t)o.left * 8); ld8(hr, Hh + (size_t)o.right * 8);
    ge_p3 a, b, p;
    const bool ok = ge_decompress(a, cl) & ge_decompress(b, cr);
    if (!ok) bad[o.batch] = 1;                                // (every writer stores the same byte: no atomic)
    ge_add(p, a, b);
    ge_compress(cp, p);
    node_hash_parent_w<8, DX>(dg, hp, cl, cr, hl, hr);
    st8(C + (size_t)o.dst * 8, cp);
    st8(Hh + (size_t)o.dst * 8, hp);
}

// ok[j] = batch j is well-formed (root_slot[j] != ~0), none of its merges met a bad point, its root slot holds the root, and the
// policy's range check accepted row pos[j] of the group-ordered verdicts.  root: C [8] then H [8].
__global__ __launch_bounds__(256) void k_batches_roots(size_t nb, const uint32_t* __restrict__ root_slot, const uint32_t* __restrict__ pos,
                                                       const uint32_t* __restrict__ C, const uint32_t* __restrict__ Hh,
                                                       const uint32_t* __restrict__ root, const uint8_t* __restrict__ bad,
                                                       const uint8_t* __restrict__ range_ok, uint8_t* __restrict__ ok) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nb) return;
    const uint32_t s = root_slot[j];
    if (s == 0xffffffffu) { ok[j] = 0; return; }
    uint32_t c[8], h[8], diff = 0;
    ld8(c, C + (size_t)s * 8); ld8(h, Hh + (size_t)s * 8);
    for (int i = 0; i < 8; i++) diff |= (c[i] ^ root[i]) | (h[i] ^ root[8 + i]);
    ok[j] = (diff == 0 && !bad[j] && range_ok[pos[j]]) ? 1 : 0;
}

}  // namespace dapol

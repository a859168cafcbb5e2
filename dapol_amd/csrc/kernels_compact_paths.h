// COMPACT MERKLE PATHS on the device (host_compact_paths.inc; index arithmetic and the LINK words in compact_paths_plan.inc):
//   k_tree_path_walk_compact  the prover's side: every row walks its chain as k_tree_path_walk does and stores a sibling only at the
//                             depths at which it is a head, at depth_off[d] + ref[d][e]; no [b][H] array exists;
//   k_cpaths_level            the verifier's fast route, one launch per depth, bottom-up: a lane per distinct node (d, key) merges the
//                             node with its record.  A CANONICAL merge (the node's head row is its parent's) hands the extended point,
//                             the encoding and the hash to the parent's slot: a point this call has made is never decoded again.  A
//                             JOIN merge (its chain ends here) leaves its result for the comparison below;
//   k_cpaths_joins            every row but the first compares the result of its join with the parent's value; row 0 compares the root;
//   k_cpaths_expand           the fallback: the [b][H] arrays of dapol_compact_paths_expand for k_verify_paths as it is;
//   k_cpaths_gather           range proofs: the head of (sub-proof, subtree key) collects its m commitments from the records it walks;
//   k_cpaths_verdict          every row ANDs the verdicts of the sub-proofs met on its walk to the root.
// No LDS, no atomics: the one shared word (`bad`) only ever receives the same value.
#pragma once
#include <hip/hip_runtime.h>
#include "compact_paths_plan.inc"

namespace dapol {

// Rows walk up from their leaves (level 0 = depth H) and store the siblings they are the head of; a row's walk ends at its join.
// wviews != null: a tree with 64-byte node hashes (outH holds 16 words a record).
__global__ __launch_bounds__(64) void k_tree_path_walk_compact(size_t b, const uint32_t* __restrict__ pos, const LevelView* views, const WideView* wviews,
                                                              CPathsDev L, const uint32_t* __restrict__ link, uint32_t* __restrict__ outC,
                                                              uint32_t* __restrict__ outH) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b) return;
    uint32_t p = pos[t];
    if (p == 0xffffffffu) return;
    size_t i = t;
    for (int level = 0; level < (int)L.H; level++) {
        const LevelView lv = views[level];
        const size_t rec = (size_t)L.depth_off[L.H - level] + i;
        uint32_t c[8], h[8];
        load_other_child(c, h, nullptr, nullptr, lv, p);
        st8(outC + rec * 8, c);
        if (wviews) {
            const WideView wv = wviews[level];
            uint32_t hw[16];
            if (lv.has_pad[p]) ld16(hw, wv.padH + (size_t)p * 16);
            else ld16(hw, wv.H + ((lv.idx[p] & 1ull) ? (size_t)p - 1 : (size_t)p + 1) * 16);
            st16(outH + rec * 16, hw);
        } else st8(outH + rec * 8, h);
        const uint32_t w = link[rec];
        if (w & CPATHS_JOIN) return;
        i = w & CPATHS_INDEX;
        p = lv.parent[p];
    }
}

// The buffers of the fast route.  Nodes of depth d < H live at node_off(d) + i of nodeC / nodeH (depth 0: the one node 0); the
// extended points and head rows of the depth being merged and of its parents' in two buffers that swap every launch.
struct CPathsMerge {
    const uint32_t* link;
    const uint32_t *leafC, *leafH;          // [b][8]
    const uint32_t *recC, *recH;            // [n_records][8]
    uint32_t *nodeC, *nodeH;                // [1 + depth_off[H]][8]
    uint32_t *joinC, *joinH;                // [b][8]: what row e's join merge made
    uint32_t* join_at;                      // [b]: the node (in nodeC / nodeH) that it must equal
    uint32_t* bad;                          // one word: a decoding failed, a join or the root differs
};
__host__ __device__ __forceinline__ size_t cpaths_node_off(const CPathsDev& L, int d) { return d == 0 ? 0 : 1 + (size_t)L.depth_off[d]; }

template <int HW, int DX>
__global__ __launch_bounds__(64) void k_cpaths_level(int dg, int d, size_t n, CPathsDev L, CPathsMerge M, const int32_t* __restrict__ ext_in,
                                                    const uint32_t* __restrict__ row_in, int32_t* __restrict__ ext_out, uint32_t* __restrict__ row_out) {
    static_assert(HW == 8, "the fast route is built for the 32-byte digests");
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const size_t rec = (size_t)L.depth_off[d] + i;
    const uint32_t w = M.link[rec];
    uint32_t c[8], h[HW], sc_[8], sh[HW], hn[HW];
    ge_p3 acc, sp;
    bool good = true;
    uint32_t row;
    if (d == (int)L.H) {                                        // the leaves: the only points of a chain that are decoded
        ld8(c, M.leafC + i * 8);
        ld8(h, M.leafH + i * HW);
        good = ge_decompress(acc, c);
        row = (uint32_t)i;
    } else {
        const size_t at = cpaths_node_off(L, d) + i;
        ld8(c, M.nodeC + at * 8);
        ld8(h, M.nodeH + at * HW);
        ld_p3(acc, ext_in + i * P3_WORDS);
        row = row_in[i];
    }
    ld8(sc_, M.recC + rec * 8);
    ld8(sh, M.recH + rec * HW);
    good &= ge_decompress(sp, sc_);                             // deserialisation rejects non-canonical points (proof/node.rs:88-94)
    if (w & CPATHS_RIGHT) node_hash_parent_w<HW, DX>(dg, hn, sc_, c, sh, h);
    else node_hash_parent_w<HW, DX>(dg, hn, c, sc_, h, sh);
    ge_p3 t;
    ge_add(t, acc, sp);
    ge_compress(c, t);
    if (!good) *M.bad = 1u;
    const size_t pi = w & CPATHS_INDEX;
    if (w & CPATHS_JOIN) {
        st8(M.joinC + (size_t)row * 8, c);
        st8(M.joinH + (size_t)row * HW, hn);
        M.join_at[row] = (uint32_t)(cpaths_node_off(L, d - 1) + pi);
    } else {
        const size_t at = cpaths_node_off(L, d - 1) + pi;
        st8(M.nodeC + at * 8, c);
        st8(M.nodeH + at * HW, hn);
        if (d > 1) {                                            // (the root has no merge above it)
            st_p3(ext_out + pi * P3_WORDS, t);
            row_out[pi] = row;
        }
    }
}

// Row e >= 1: the bytes its join merge made against the canonical value of that node; row 0: node 0 against the caller's root.
__global__ __launch_bounds__(256) void k_cpaths_joins(size_t b, CPathsMerge M, const uint32_t* __restrict__ rootC, const uint32_t* __restrict__ rootH) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= b) return;
    uint32_t a[8], x[8], ah[8], xh[8];
    if (e == 0) {
        ld8(a, M.nodeC); ld8(ah, M.nodeH);
        ld8(x, rootC); ld8(xh, rootH);
    } else {
        const size_t at = M.join_at[e];
        ld8(a, M.nodeC + at * 8); ld8(ah, M.nodeH + at * 8);
        ld8(x, M.joinC + e * 8); ld8(xh, M.joinH + e * 8);
    }
    uint32_t diff = 0;
    for (int k = 0; k < 8; k++) diff |= (a[k] ^ x[k]) | (ah[k] ^ xh[k]);
    if (diff) *M.bad = 1u;
}

// The fallback's expansion on the device: row e follows its links from the leaf to the root and copies every record it meets into
// its slot of the [b][H] arrays (cpaths_slot: the call's sibling order).
__global__ __launch_bounds__(256) void k_cpaths_expand(size_t b, CPathsDev L, int leaf_first, const uint32_t* __restrict__ link, const uint32_t* __restrict__ recC,
                                                       const uint32_t* __restrict__ recH, uint32_t* __restrict__ outC, uint32_t* __restrict__ outH) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= b) return;
    size_t i = e;
    for (int d = (int)L.H; d >= 1; d--) {
        const size_t rec = (size_t)L.depth_off[d] + i, slot = e * (size_t)L.H + (size_t)cpaths_slot((int)L.H, d, leaf_first != 0);
        uint32_t c[8], h[8];
        ld8(c, recC + rec * 8); ld8(h, recH + rec * 8);
        st8(outC + slot * 8, c); st8(outH + slot * 8, h);
        i = link[rec] & CPATHS_INDEX;
    }
}

// The range proofs of one sub-proof of the plan: its distinct statements are the nodes of its key depth D (D = 0: the one statement
// without siblings), in the order of the compact proof buffer.  Lane i walks from node (D, i) towards the root and copies the `count`
// commitments of slots [start, start + count) into parties [0, count) of row i of Vc ([n][m][8]); the other parties are pads (the
// compressed blinding base).
__global__ __launch_bounds__(256) void k_cpaths_gather(size_t n, int D, int start, int count, int m, int leaf_first, CPathsDev L,
                                                       const uint32_t* __restrict__ link, const uint32_t* __restrict__ recC, const uint32_t* __restrict__ Bb_comp,
                                                       uint32_t* __restrict__ Vc) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    uint32_t c[8];
    size_t i = r;
    int left = count;
    for (int d = D; d >= 1 && left > 0; d--) {
        const size_t rec = (size_t)L.depth_off[d] + i;
        const int jj = cpaths_slot((int)L.H, d, leaf_first != 0) - start;
        if (jj >= 0 && jj < count) {
            ld8(c, recC + rec * 8);
            st8(Vc + (r * (size_t)m + (size_t)jj) * 8, c);
            left--;
        }
        i = link[rec] & CPATHS_INDEX;
    }
    for (int k = 0; k < 8; k++) c[k] = Bb_comp[k];
    for (int jj = count; jj < m; jj++) st8(Vc + (r * (size_t)m + (size_t)jj) * 8, c);
}

// ok[e] = AND of the verdicts of the statements that row e belongs to: sub-proof s has its verdicts at sub + first[s], one per node of
// depth D[s], and the row's node there is the one its walk passes.
struct CPathsRange {
    uint32_t n_sub;
    uint8_t D[VSHARED_MAX_SUB];
    uint32_t first[VSHARED_MAX_SUB];
};
__global__ __launch_bounds__(256) void k_cpaths_verdict(size_t b, CPathsDev L, CPathsRange R, const uint32_t* __restrict__ link, const uint8_t* __restrict__ sub,
                                                        uint8_t* __restrict__ ok) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= b) return;
    uint8_t good = 1;
    size_t i = e;
    for (int d = (int)L.H; d >= 0; d--) {
        for (uint32_t s = 0; s < R.n_sub; s++)
            if ((int)R.D[s] == d) good &= sub[(size_t)R.first[s] + i] ? 1 : 0;
        if (d >= 1) i = link[(size_t)L.depth_off[d] + i] & CPATHS_INDEX;
    }
    ok[e] = good;
}

}  // namespace dapol

// Context-creation kernels (generators + window tables, derived on the GPU) and the sparse-Merkle tree kernels.
#pragma once
#include <hip/hip_runtime.h>
#include "hash.h"
#include "sc.h"
#include "tables.h"

namespace dapol {

// ------------------------------------------------------------------------------------------ small helpers
__device__ __forceinline__ void ld8(uint32_t* w, const uint32_t* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    uint4 a = q[0], b = q[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
__device__ __forceinline__ void st8(uint32_t* p, const uint32_t* w) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// An extended point in memory: a record of P3_WORDS = 40 words (160 bytes, the stride every buffer uses) holding
// X | Y | Z | T as 4 x FE_NL = 36 limbs; the last four words are unused.
enum { P3_WORDS = 40 };
__device__ __forceinline__ void ld_p3(ge_p3& p, const int32_t* src) {
    const int4* q = reinterpret_cast<const int4*>(src);
    int32_t w[4 * FE_NL];
    for (int i = 0; i < FE_NL; i++) { int4 a = q[i]; w[4 * i] = a.x; w[4 * i + 1] = a.y; w[4 * i + 2] = a.z; w[4 * i + 3] = a.w; }
    for (int i = 0; i < FE_NL; i++) { p.X.v[i] = w[i]; p.Y.v[i] = w[FE_NL + i]; p.Z.v[i] = w[2 * FE_NL + i]; p.T.v[i] = w[3 * FE_NL + i]; }
}
__device__ __forceinline__ void st_p3(int32_t* dst, const ge_p3& p) {
    int32_t w[4 * FE_NL];
    for (int i = 0; i < FE_NL; i++) { w[i] = p.X.v[i]; w[FE_NL + i] = p.Y.v[i]; w[2 * FE_NL + i] = p.Z.v[i]; w[3 * FE_NL + i] = p.T.v[i]; }
    int4* q = reinterpret_cast<int4*>(dst);
    for (int i = 0; i < FE_NL; i++) q[i] = make_int4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}

// ----------------------------------------------------------------------------- context: generator chains
// bulletproofs 4.0.0 GeneratorsChain: SHAKE256("GeneratorsChain" || label), label = 'G'|'H' || u32le(party);
// successive 64-byte reads.  One lane per chain (2 * max_parties chains), 64 reads each.
__device__ __forceinline__ void absorb_label(Sponge& sp, const char* s, int n) {
    for (int i = 0; i < n; i++) sponge_absorb_byte(sp, (uint8_t)s[i]);
}
__global__ void k_ctx_chains(uint32_t* uniform /*[2P][64][16]*/, int P) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= 2 * P) return;
    int which = c / P, party = c % P;
    Sponge sp;
    sponge_init(sp, 136);
    absorb_label(sp, LBL_GENERATORS_CHAIN);
    sponge_absorb_byte(sp, which ? LBL_GENS_H : LBL_GENS_G);
    for (int i = 0; i < 4; i++) sponge_absorb_byte(sp, (uint8_t)((uint32_t)party >> (8 * i)));
    sponge_finish(sp, 0x1F);
    uint32_t* out = uniform + (size_t)c * 64 * 16;
    for (int i = 0; i < 64 * 16; i++) {
        uint32_t w = 0;
        for (int k = 0; k < 4; k++) w |= (uint32_t)sponge_squeeze_byte(sp) << (8 * k);
        out[i] = w;
    }
}
// One lane per generator: RistrettoPoint::from_uniform_bytes.
__global__ void k_ctx_points(int32_t* base_pts /*[rows][40]*/, const uint32_t* uniform, int P) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= 128 * P) return;
    uint32_t w[16];
    for (int i = 0; i < 16; i++) w[i] = uniform[(size_t)r * 16 + i];
    ge_p3 p;
    ge_from_uniform(p, w);
    st_p3(base_pts + (size_t)r * 40, p);
}
// PedersenGens::default(): B = ristretto basepoint, B_blinding = hash_from_bytes::<Sha3_512>(B.compress()).
// Lane 0 -> 2^(W w) B_blinding rows, lane 1 -> 2^(W w) B rows.
__global__ void k_ctx_pedersen(int32_t* base_pts, int P, int wbits, int nwin) {
    int t = threadIdx.x;
    if (t >= 2) return;
    ge_p3 p;
    ge_basepoint(p);
    if (t == 0) {
        uint32_t c[8], w[16];
        ge_compress(c, p);
        Sponge sp;
        sponge_init(sp, 72);
        for (int i = 0; i < 8; i++)
            for (int k = 0; k < 4; k++) sponge_absorb_byte(sp, (uint8_t)(c[i] >> (8 * k)));
        sponge_finish(sp, 0x06);
        for (int i = 0; i < 16; i++) {
            uint32_t x = 0;
            for (int k = 0; k < 4; k++) x |= (uint32_t)sponge_squeeze_byte(sp) << (8 * k);
            w[i] = x;
        }
        ge_from_uniform(p, w);
    }
    int row0 = 128 * P + (t == 0 ? 0 : nwin);
    for (int w = 0; w < nwin; w++) {
        st_p3(base_pts + (size_t)(row0 + w) * 40, p);
        for (int d = 0; d < wbits; d++) { ge_p3 q; ge_dbl(q, p, true); p = q; }
    }
}
// High-half base points: 2^(shift) * (G / H generator), one lane per generator (TableView::hi_split).
__global__ void k_ctx_hi_points(int32_t* base_pts, int n_gh, int n_rows, int shift) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_gh) return;
    ge_p3 p, q;
    ld_p3(p, base_pts + (size_t)r * 40);
    for (int d = 0; d < shift; d++) { ge_dbl(q, p, true); p = q; }
    st_p3(base_pts + (size_t)(n_rows + r) * 40, p);
}
// One lane per table entry: k * base, normalised to affine niels form.
__global__ void k_ctx_table(int32_t* table, const int32_t* base_pts, int n_rows, int wbits, int entries) {
    size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (size_t)n_rows * entries) return;
    int row = (int)(gid / entries), k = (int)(gid % entries);
    ge_niels q;
    if (k == 0) {
        ge_niels_identity(q);
    } else {
        ge_p3 base, acc, t;
        ld_p3(base, base_pts + (size_t)row * 40);
        ge_identity(acc);
        for (int b = wbits - 1; b >= 0; b--) {
            ge_dbl(t, acc, true);
            acc = t;
            if ((k >> b) & 1) { ge_add(t, acc, base); acc = t; }
        }
        fe zi, x, y;
        fe_invert(zi, acc.Z);
        fe_mul(x, acc.X, zi);
        fe_mul(y, acc.Y, zi);
        ge_to_niels(q, x, y);
    }
    int32_t* e = table + ((size_t)row * entries + (size_t)k) * TBL_ENTRY_WORDS;
    niels_store_entry(e, q);
}
__global__ void k_ctx_compress(uint32_t* comp /*[rows][8]*/, const int32_t* base_pts, int n_rows) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    ge_p3 p;
    ld_p3(p, base_pts + (size_t)r * 40);
    uint32_t c[8];
    ge_compress(c, p);
    st8(comp + (size_t)r * 8, c);
}

// --------------------------------------------------------------------------------------------------- scan
// The level sizes live on the DEVICE (cnt[k] = real nodes of level k): every kernel of the build reads its bound from there
// and is launched over the host-side upper bound, so the host never waits for a level (no per-level synchronisation).
// flag[i] = 1 if node i starts a new parent (its index >> 1 differs from its predecessor's).
__global__ void k_tree_flags(const uint32_t* n_ptr, const uint64_t* idx, uint32_t* flag) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *n_ptr) return;
    flag[i] = (i == 0 || (idx[i] >> 1) != (idx[i - 1] >> 1)) ? 1u : 0u;
}
// Inclusive scan of 256 values held one per thread; returns the inclusive value, *total = sum over the block.
__device__ __forceinline__ uint32_t block_scan256(uint32_t x, uint32_t* wave_tot /*[4] shared*/, uint32_t* total) {
    int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) wave_tot[wv] = x;
    __syncthreads();
    uint32_t add = 0, all = 0;
    for (int k = 0; k < 4; k++) { if (k < wv) add += wave_tot[k]; all += wave_tot[k]; }
    __syncthreads();
    *total = all;
    return x + add;
}
// Block-local inclusive scan of 1024 elements per 256-thread block.
__global__ __launch_bounds__(256) void k_scan_block(const uint32_t* n_ptr, const uint32_t* in, uint32_t* out, uint32_t* block_sums) {
    __shared__ uint32_t wave_tot[4];
    const size_t n = *n_ptr;
    size_t base = (size_t)blockIdx.x * 1024 + (size_t)threadIdx.x * 4;
    if ((size_t)blockIdx.x * 1024 >= n) return;                      // (whole block: the launch covers the host-side bound)
    uint32_t a[4];
    for (int k = 0; k < 4; k++) a[k] = (base + k < n) ? in[base + k] : 0u;
    a[1] += a[0]; a[2] += a[1]; a[3] += a[2];
    uint32_t tot, incl = block_scan256(a[3], wave_tot, &tot);
    uint32_t excl = incl - a[3];
    for (int k = 0; k < 4; k++)
        if (base + k < n) out[base + k] = a[k] + excl;
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}
// Exclusive scan of the block sums by ONE block of 256 threads (256 sums per trip); the grand total = size of the next level.
__global__ __launch_bounds__(256) void k_scan_sums(const uint32_t* n_ptr, uint32_t* block_sums, uint32_t* total) {
    __shared__ uint32_t wave_tot[4];
    const size_t nb = ((size_t)*n_ptr + 1023) / 1024;
    uint32_t carry = 0;
    for (size_t base = 0; base < nb; base += 256) {
        size_t i = base + threadIdx.x;
        uint32_t t = i < nb ? block_sums[i] : 0u, tot;
        uint32_t incl = block_scan256(t, wave_tot, &tot);
        if (i < nb) block_sums[i] = carry + incl - t;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}
// pos[i] = parent slot of node i; head[q] = first child of parent q.
__global__ void k_scan_finish(const uint32_t* n_ptr, const uint32_t* flag, uint32_t* pos, const uint32_t* block_offs, uint32_t* head) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *n_ptr) return;
    uint32_t p = pos[i] + block_offs[i >> 10] - 1;
    pos[i] = p;
    if (flag[i]) head[p] = (uint32_t)i;
}

// ------------------------------------------------------------------------------------------- tree levels
struct LevelView {
    size_t n;
    uint64_t* idx;
    uint32_t* C;
    uint32_t* H;
    uint64_t* v;
    uint32_t* r;
    uint32_t* padC;
    uint32_t* padH;
    uint32_t* padr;
    uint8_t* has_pad;
    uint32_t* parent;
    int32_t* ext;   // extended points of this level (only alive while the next level is being built)
};

// ----------------------------------------------------------------------------------------- node routines
// What a DAPOL node is, once: every kernel below -- the build, its small-tree phases and the in-place edits -- makes its leaves,
// padding nodes and parents with these, so that all paths leave the same bytes.  The routines that hash, and the kernels that call
// them, are templates over DX (hash.h): DG_RUNTIME = the node digest is tbl.digest / `digest`, one of the three BLAKE ones, as these
// kernels always read it; DG_SHA256 / DG_SHA3_256 = that digest, an instantiation of its own that no other context launches.
// Leaf, DapolNode::new (src/dapol/node.rs:29-45): P = v*B + r*B_blinding, c = its encoding, h = D(c).  r: eight words with bit 255
// already cleared by the caller (Scalar::from_bits); may be >= l.
__device__ __forceinline__ void leaf_point(ge_p3& P, const TableView& tbl, uint64_t v, const uint32_t* r) {
    ge_identity(P);
    tbl_fixed_mul_add_u64(P, tbl, tbl.row_B(0), v);
    tbl_fixed_mul_add(P, tbl, tbl.row_Bb(0), r);
}
template <int DX>
__device__ __forceinline__ void leaf_encode(uint32_t* c, uint32_t* h, const TableView& tbl, const ge_p3& P) {
    ge_compress(c, P);
    node_hash32_x<DX>(tbl.digest, h, c);
}
template <int DX>
__device__ __forceinline__ void leaf_node(ge_p3& P, uint32_t* c, uint32_t* h, const TableView& tbl, uint64_t v, const uint32_t* r) {
    leaf_point(P, tbl, v, r);
    leaf_encode<DX>(c, h, tbl, P);
}
// Padding node, Paddable::padding (node.rs:86-88): new(0, r) with r drawn for the node's position (seed mode) or read from the
// caller's tape.  padding_draw = the positional 64-byte draw; padding_from_wide = the node of a draw: rm / rB = its blinding reduced
// mod l (Montgomery form / words), pB = rB*B_blinding, cB, hB as for a leaf.
__device__ __forceinline__ void padding_draw(uint32_t* wide, const uint32_t* pad_seed /*8 words*/, uint64_t level, uint64_t index) {
    uint32_t seed[8];
    for (int k = 0; k < 8; k++) seed[k] = pad_seed[k];
    seed_wide(wide, seed, 1u, level, index);
}
template <int DX>
__device__ __forceinline__ void padding_from_wide(ge_p3& pB, sc& rm, uint32_t* rB, uint32_t* cB, uint32_t* hB, const TableView& tbl, const uint32_t* wide) {
    sc_from_wide(rm, wide);
    sc_from_mont(rB, rm);
    ge_identity(pB);
    tbl_fixed_mul_add(pB, tbl, tbl.row_Bb(0), rB);
    ge_compress(cB, pB);
    node_hash32_x<DX>(tbl.digest, hB, cB);
}
template <int DX>
__device__ __forceinline__ void padding_from_wide(ge_p3& pB, uint32_t* rB, uint32_t* cB, uint32_t* hB, const TableView& tbl, const uint32_t* wide) {
    sc rm;
    padding_from_wide<DX>(pB, rm, rB, cB, hB, tbl, wide);
}
template <int DX>
__device__ __forceinline__ void padding_node(ge_p3& pB, uint32_t* rB, uint32_t* cB, uint32_t* hB, const TableView& tbl, const uint32_t* pad_seed, uint64_t level,
                                             uint64_t index) {
    uint32_t wide[16];
    padding_draw(wide, pad_seed, level, index);
    padding_from_wide<DX>(pB, rB, cB, hB, tbl, wide);
}
// The padding sibling of real node i of level L is kept beside it.
__device__ __forceinline__ void store_pad_record(const LevelView& L, size_t i, const uint32_t* cB, const uint32_t* hB, const uint32_t* rB) {
    st8(L.padC + i * 8, cB);
    st8(L.padH + i * 8, hB);
    st8(L.padr + i * 8, rB);
}
// The other child of the parent of real node c: its padding record, or the real neighbour on its right (c is a left child) or left.
// rB / vB may be null where a caller has no use for the blinding / the value (a padding node's value is 0).
__device__ __forceinline__ void load_other_child(uint32_t* cB, uint32_t* hB, uint32_t* rB, uint64_t* vB, const LevelView& L, size_t c, bool left) {
    if (vB) *vB = 0;
    if (L.has_pad[c]) {
        ld8(cB, L.padC + c * 8);
        ld8(hB, L.padH + c * 8);
        if (rB) ld8(rB, L.padr + c * 8);
    } else {
        const size_t s = left ? c + 1 : c - 1;
        ld8(cB, L.C + s * 8);
        ld8(hB, L.H + s * 8);
        if (rB) ld8(rB, L.r + s * 8);
        if (vB) *vB = L.v[s];
    }
}
// For a caller that has not read c's index: it is read only where there is a real neighbour to pick.
__device__ __forceinline__ void load_other_child(uint32_t* cB, uint32_t* hB, uint32_t* rB, uint64_t* vB, const LevelView& L, size_t c) {
    load_other_child(cB, hB, rB, vB, L, c, L.has_pad[c] || (L.idx[c] & 1ull) == 0);
}
// Parent, Mergeable::merge (node.rs:64-80): r = (r_A + r_B) mod l (dalek's Scalar add reduces even unreduced inputs), P = P_A + P_B,
// h = D(C_L || C_R || H_L || H_R) with A on the left or on the right.  (v = v_A + v_B with u64 wrap is the caller's one addition.)
__device__ __forceinline__ void sc_add_words(uint32_t* rp, const uint32_t* rA, const uint32_t* rB) {
    sc ma, mb, ms;
    sc_to_mont(ma, rA);
    sc_to_mont(mb, rB);
    sc_add(ms, ma, mb);
    sc_from_mont(rp, ms);
}
template <int DX>
__device__ __forceinline__ void parent_hash(int digest, uint32_t* hp, bool a_is_left, const uint32_t* cA, const uint32_t* cB, const uint32_t* hA, const uint32_t* hB) {
    if (a_is_left) node_hash128_x<DX>(digest, hp, cA, cB, hA, hB);
    else node_hash128_x<DX>(digest, hp, cB, cA, hB, hA);
}
template <int DX>
__device__ __forceinline__ void merge_parent(ge_p3& pp, uint32_t* rp, uint32_t* cp, uint32_t* hp, int digest, bool a_is_left, const ge_p3& pA, const ge_p3& pB,
                                             const uint32_t* rA, const uint32_t* rB, const uint32_t* cA, const uint32_t* cB, const uint32_t* hA, const uint32_t* hB) {
    sc_add_words(rp, rA, rB);
    ge_add(pp, pA, pB);
    ge_compress(cp, pp);
    parent_hash<DX>(digest, hp, a_is_left, cA, cB, hA, hB);
}
// Lower bound of `want` in the sorted idx[0 .. n).
__device__ __forceinline__ size_t lower_bound_u64(const uint64_t* idx, size_t n, uint64_t want) {
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = (lo + hi) >> 1;
        if (idx[mid] < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------- commitments
// One lane per node: leaf_node of (v[i], r[i]); bit 255 of r is ignored.
template <int DX>
__global__ __launch_bounds__(256) void k_commit_hash(TableView tbl, size_t n, const uint64_t* v, uint32_t* r, uint32_t* C,
                                                     uint32_t* H, int32_t* ext) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t rw[8];
    ld8(rw, r + i * 8);
    if (rw[7] >> 31) {             // Scalar::from_bits clears bit 255; keep the stored copy consistent
        rw[7] &= 0x7fffffffu;
        r[i * 8 + 7] = rw[7];
    }
    ge_p3 acc;
    uint32_t c[8], h[8];
    leaf_node<DX>(acc, c, h, tbl, v[i], rw);
    st8(C + i * 8, c);
    st8(H + i * 8, h);
    if (ext) st_p3(ext + i * 40, acc);
}

// One lane per PARENT q (smtree build restated level-synchronously): children = the real node head[q] and either
// the adjacent real node or a padding node made on the spot (Paddable::padding, src/dapol/node.rs:86-88, with the
// positional seed-mode blinding); parent = Mergeable::merge (node.rs:64-80).
// TAPE mode (pad_tape != null; dapol_tree_build_tape): the padding node's 64-byte draw is read from the caller's tape instead of being
// derived from the seed.  Tape order = (level bottom-up, index ascending) over the padding nodes.  Parent q of this level has the
// real children head[q] (and head[q] + 1 when they are a pair), so 2 q - head[q] parents before it own a padding child -- the rank
// inside the level -- and the levels below hold sum (2 cnt[j + 1] - cnt[j]) padding nodes: no scan, no second pass.
struct PadTape {
    const uint32_t* draws;     // [n_draws][16] or null (seed mode)
    uint32_t n_draws;
    uint32_t* short_flag;      // set when the tree needs more draws than the tape holds
};
// SPLIT = 1 (the default since round 6; DAPOL_TREE_SPLIT=0 turns it off): the padding children of the level were made by k_tree_pad_level just before --
// their records are read from padC / padH / padr and their points from extpad[q] -- so that neither kernel holds a fixed-base
// product, two encodings and three hashes in one register allocation.
template <int SPLIT, int DX>
__global__ __launch_bounds__(256) void k_tree_merge(TableView tbl, LevelView cur, LevelView nxt, const uint32_t* head, int level,
                                                    const uint32_t* pad_seed /*8 words*/, const uint32_t* cnt /*[levels + 1], device*/, PadTape tape,
                                                    const int32_t* extpad) {
    size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t cur_n = cnt[level], nxt_n = cnt[level + 1];           // (cur.n / nxt.n are only host-side bounds during the build)
    if (q >= nxt_n) return;
    size_t i = head[q];
    uint64_t my_idx = cur.idx[i];
    bool pair = (i + 1 < cur_n) && (cur.idx[i + 1] == (my_idx ^ 1ull));
    uint32_t cA[8], hA[8], rA[8], cB[8], hB[8], rB[8];
    uint64_t vA = cur.v[i], vB = 0;
    ge_p3 pA, pB;
    ld8(cA, cur.C + i * 8);
    ld8(hA, cur.H + i * 8);
    ld8(rA, cur.r + i * 8);
    ld_p3(pA, cur.ext + i * 40);
    if (pair) {
        ld8(cB, cur.C + (i + 1) * 8);
        ld8(hB, cur.H + (i + 1) * 8);
        ld8(rB, cur.r + (i + 1) * 8);
        vB = cur.v[i + 1];
        ld_p3(pB, cur.ext + (i + 1) * 40);
        cur.has_pad[i] = 0;
        cur.has_pad[i + 1] = 0;
        cur.parent[i + 1] = (uint32_t)q;
    } else if (SPLIT) {
        ld8(cB, cur.padC + i * 8);
        ld8(hB, cur.padH + i * 8);
        ld8(rB, cur.padr + i * 8);
        ld_p3(pB, extpad + q * 40);
        cur.has_pad[i] = 1;
    } else {
        uint32_t wide[16];
        if (tape.draws) {
            uint64_t rank = 2 * (uint64_t)q - (uint64_t)i;
            for (int j = 0; j < level; j++) rank += 2 * (uint64_t)cnt[j + 1] - (uint64_t)cnt[j];
            if (rank < tape.n_draws) { for (int k = 0; k < 16; k++) wide[k] = tape.draws[rank * 16 + k]; }
            else { atomicOr(tape.short_flag, 1u); for (int k = 0; k < 16; k++) wide[k] = 0; }
        } else {
            padding_draw(wide, pad_seed, (uint64_t)level, my_idx ^ 1ull);
        }
        padding_from_wide<DX>(pB, rB, cB, hB, tbl, wide);
        store_pad_record(cur, i, cB, hB, rB);
        cur.has_pad[i] = 1;
    }
    cur.parent[i] = (uint32_t)q;
    uint32_t rp[8], cp[8], hp[8];
    ge_p3 pp;
    merge_parent<DX>(pp, rp, cp, hp, tbl.digest, pair || ((my_idx & 1ull) == 0), pA, pB, rA, rB, cA, cB, hA, hB);
    nxt.idx[q] = my_idx >> 1;
    nxt.v[q] = vA + vB;           // u64 wrap == release-mode Rust (node.rs:72)
    st8(nxt.r + q * 8, rp);
    st8(nxt.C + q * 8, cp);
    st8(nxt.H + q * 8, hp);
    if (nxt.ext) st_p3(nxt.ext + q * 40, pp);
}

// The padding children of one level on their own (seed mode): Paddable::padding for every parent q whose second child is not real.
template <int DX>
__global__ __launch_bounds__(256) void k_tree_pad_level(TableView tbl, LevelView cur, const uint32_t* head, int level, const uint32_t* pad_seed,
                                                        const uint32_t* cnt, int32_t* extpad) {
    size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t cur_n = cnt[level], nxt_n = cnt[level + 1];
    if (q >= nxt_n) return;
    size_t i = head[q];
    uint64_t my_idx = cur.idx[i];
    if ((i + 1 < cur_n) && (cur.idx[i + 1] == (my_idx ^ 1ull))) return;
    uint32_t rB[8], cB[8], hB[8];
    ge_p3 pB;
    padding_node<DX>(pB, rB, cB, hB, tbl, pad_seed, (uint64_t)level, my_idx ^ 1ull);
    store_pad_record(cur, i, cB, hB, rB);
    st_p3(extpad + q * 40, pB);
}

// The padding nodes of n given positions (level[i], index[i]), as records.
template <int DX>
__global__ void k_padding_nodes(TableView tbl, size_t n, const uint32_t* pad_seed, const uint8_t* level, const uint64_t* index, uint32_t* C,
                                uint32_t* H, uint32_t* r) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t rB[8], cB[8], hB[8];
    ge_p3 p;
    padding_node<DX>(p, rB, cB, hB, tbl, pad_seed, (uint64_t)level[i], index[i]);
    st8(C + i * 8, cB);
    st8(H + i * 8, hB);
    st8(r + i * 8, rB);
}

// ------------------------------------------------------------------------------------- incremental update
// smtree's `update` (src/dapol/mod.rs:210-213 -> SparseMerkleTree::update) re-merges ONE root-to-leaf path.  Replacing the
// liabilities of k leaves that already exist changes no structure: the same nodes, parents and padding siblings (those are keyed
// by position).  What changes along every path is a sum: an ancestor's value, blinding and commitment move by the sum of the
// deltas of the updated leaves below it --
//     v' = v + sum dv (u64 wrap, as Mergeable::merge),   r' = r + sum dr (mod l),   C' = C + sum dP  (group addition)
// -- and every ancestor is independent of every other, so all levels run side by side (U2); only the hash chain is sequential
// over the levels (U3, one block stepping through them).  The result equals dapol_tree_build over the new leaf set bit for bit
// (ristretto encodings are canonical; tests/test_gpu_parity.py::test_update_equals_build).
//   U0  k_tree_find_paths   per update: find the leaf and its node positions at every level (parent pointers); a missing index
//                           sends the whole batch to the rebuild before anything has been written
//   U1  k_tree_upd_leaves   per update: the leaf's new node, dP = P_new - P_old, dv, dr
//   U2  k_tree_upd_nodes    per (update, level >= 1): the first update of a run that shares the node adds the run's deltas to it
//   U3  k_tree_upd_hash     one block, level by level: re-hash the touched parents from their (updated) children
struct TreeUpdArgs {
    size_t k;                  // updates, sorted by leaf index, distinct
    int height;
    const uint64_t* idx;       // [k]
    const uint64_t* v;         // [k]
    const uint32_t* r;         // [k][8]
    uint32_t* pos;             // [k][height + 1]   node position of update j at every level
    int32_t* dP;               // [k][40]           P_new - P_old, extended
    uint64_t* dv;              // [k]
    uint32_t* dr;              // [k][8]            Montgomery form
    uint32_t* missing;         // U0's outputs (TreeFind): != 0: some leaf index is not in the tree (the caller rebuilds instead)
    uint8_t* found;            // [k] (may be null): per update, whether its leaf exists
    const uint32_t* first;     // [k] (may be null = 1): lowest level whose EXISTING node this update changes by its delta
};
// U0 (and R0 of the removal): where the edited leaves are, before anything is written to the tree.  The optional outputs are null
// where a path has no use for them.
struct TreeFind {
    size_t k;
    int height;
    const uint64_t* idx;       // [k] sorted, distinct
    uint32_t* pos;             // [k][height + 1] node position at every level (parent pointers)
    uint8_t* has_pad;          // [k][height + 1] (may be null): has_pad of that node
    uint32_t* missing;         // != 0: some index is not a leaf of the tree
    uint8_t* found;            // [k] (may be null): per index, whether its leaf exists
};
__global__ __launch_bounds__(64) void k_tree_find_paths(const LevelView* views, TreeFind F) {
    const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= F.k) return;
    const LevelView L0 = views[0];
    const uint64_t want = F.idx[j];
    const size_t lo = lower_bound_u64(L0.idx, L0.n, want);
    const bool found = lo < L0.n && L0.idx[lo] == want;
    if (F.found) F.found[j] = found ? 1 : 0;
    if (!found) { atomicOr(F.missing, 1u); return; }
    const size_t stride = (size_t)F.height + 1;
    uint32_t* pos = F.pos + j * stride;
    uint8_t* hp = F.has_pad ? F.has_pad + j * stride : nullptr;
    size_t p = lo;
    for (int t = 0; t < F.height; t++) {
        pos[t] = (uint32_t)p;
        if (hp) hp[t] = views[t].has_pad[p];
        p = views[t].parent[p];
    }
    pos[F.height] = (uint32_t)p;
    if (hp) hp[F.height] = 0;
}
template <int DX>
__global__ __launch_bounds__(64) void k_tree_upd_leaves(TableView tbl, const LevelView* views, TreeUpdArgs U) {
    const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= U.k) return;
    const LevelView L0 = views[0];
    const size_t lo = U.pos[j * (size_t)(U.height + 1)];
    uint32_t rn[8], ro[8], c[8], h[8];
    ld8(rn, U.r + j * 8);
    rn[7] &= 0x7fffffffu;                          // Scalar::from_bits
    ld8(ro, L0.r + lo * 8);
    ld8(c, L0.C + lo * 8);
    ge_p3 pn, po, npo, d;
    leaf_point(pn, tbl, U.v[j], rn);
    (void)ge_decompress(po, c);                    // the tree's own encoding: always decodes
    ge_neg(npo, po);
    ge_add(d, pn, npo);
    st_p3(U.dP + j * 40, d);
    sc mn, mo, md;
    sc_to_mont(mn, rn);
    sc_to_mont(mo, ro);
    sc_sub(md, mn, mo);
    for (int i = 0; i < 8; i++) U.dr[j * 8 + i] = md.v[i];
    U.dv[j] = U.v[j] - L0.v[lo];
    leaf_encode<DX>(c, h, tbl, pn);                    // (after the delta: the old encoding's words are free by now)
    L0.v[lo] = U.v[j];
    st8(L0.r + lo * 8, rn);
    st8(L0.C + lo * 8, c);
    st8(L0.H + lo * 8, h);
}
__global__ __launch_bounds__(64) void k_tree_upd_nodes(const LevelView* views, TreeUpdArgs U) {
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= U.k * (size_t)U.height) return;
    const size_t j = t / (size_t)U.height;
    const int k = 1 + (int)(t - j * (size_t)U.height);
    const size_t stride = (size_t)U.height + 1;
    if (U.first && k < (int)U.first[j]) return;                     // (an inserted leaf: its own new nodes below that level)
    const uint32_t p = U.pos[j * stride + k];
    if (j > 0 && U.pos[(j - 1) * stride + k] == p) return;          // an earlier update of the run owns this node
    ge_p3 sum, q, s;
    ld_p3(sum, U.dP + j * 40);
    uint64_t dv = U.dv[j];
    sc dr, t2;
    for (int i = 0; i < 8; i++) dr.v[i] = U.dr[j * 8 + i];
    for (size_t jj = j + 1; jj < U.k && U.pos[jj * stride + k] == p; jj++) {
        ld_p3(q, U.dP + jj * 40);
        ge_add(s, sum, q);
        sum = s;
        dv += U.dv[jj];
        for (int i = 0; i < 8; i++) t2.v[i] = U.dr[jj * 8 + i];
        sc_add(dr, dr, t2);
    }
    const LevelView L = views[k];
    uint32_t c[8], rr[8];
    ld8(c, L.C + (size_t)p * 8);
    ge_p3 old;
    (void)ge_decompress(old, c);
    ge_add(s, old, sum);
    ge_compress(c, s);
    st8(L.C + (size_t)p * 8, c);
    L.v[p] += dv;
    ld8(rr, L.r + (size_t)p * 8);
    sc mr;
    sc_to_mont(mr, rr);
    sc_add(mr, mr, dr);
    sc_from_mont(rr, mr);
    st8(L.r + (size_t)p * 8, rr);
}
// grid = 1 block of up to 1,024 threads; thread j = update j (k <= 1,024), stepping through the levels together.
template <int DX>
__global__ __launch_bounds__(1024) void k_tree_upd_hash(int digest, const LevelView* views, TreeUpdArgs U, int level_begin, int level_end) {
    const size_t j = threadIdx.x + (size_t)blockIdx.x * blockDim.x;
    const size_t stride = (size_t)U.height + 1;
    for (int k = level_begin; k < level_end; k++) {                // children at level k -> parent at level k + 1
        if (j < U.k) {
            const uint32_t pp = U.pos[j * stride + k + 1];
            if (j == 0 || U.pos[(j - 1) * stride + k + 1] != pp) {
                const LevelView L = views[k];
                const size_t i = U.pos[j * stride + k];
                const uint64_t my = L.idx[i];
                uint32_t cA[8], hA[8], cB[8], hB[8], hp[8];
                ld8(cA, L.C + i * 8); ld8(hA, L.H + i * 8);
                const bool left = (my & 1ull) == 0;
                load_other_child(cB, hB, nullptr, nullptr, L, i, left);
                parent_hash<DX>(digest, hp, left, cA, cB, hA, hB);
                st8(views[k + 1].H + (size_t)pp * 8, hp);
            }
        }
        if (gridDim.x == 1) __syncthreads();                       // (several blocks: one launch per level instead)
    }
}

// ------------------------------------------------------------------------------------- incremental insert
// A NEW leaf x changes the structure, but only along its own path and only below the first ancestor that exists already: the
// nodes (x >> t) for t < m are new -- each the merge of the one below with a padding sibling made for its position -- and at
// level m - 1 the new node's sibling S is a real node whose padding sibling (at the new node's position) goes away.  From level m
// upwards the ancestors exist and move by a delta, exactly as in the replacement path: dP = P_chain_top - P_old_pad, dr alike,
// dv = v.  The level arrays are compact and sorted, so a level that gains nodes is rewritten out of place (k_tree_relayout: every
// existing node moves up by the number of insertions before it, parent pointers follow the next level's moves); no commitment is
// recomputed for it.  Leaves whose new chains would share a node (two new leaves under one new subtree) are left to the rebuild.
//   I1  k_tree_ins_plan<1>  per new leaf: chain length m, insertion position at every level below m, position of the first
//                           existing ancestor; flags chains that share a node
//   I2  k_tree_relayout     per level that gains nodes: the level's arrays in their new order (existing nodes only)
//   I3  k_tree_ins_chain    a wavefront per new leaf, lane t = chain node t: padding siblings, prefix sums of their points,
//                           encodings; writes the new nodes, drops S's padding sibling, leaves the delta for the levels above
//   then U2 / U3 of the replacement path (k_tree_upd_nodes from level m, k_tree_upd_hash from the leaves).
struct TreeInsPlan {
    size_t k;
    int height;
    const uint64_t* idx;       // [k] sorted, distinct, all NEW
    uint32_t* m;               // [k] chain length (1..height)
    uint32_t* inspos;          // [k][height + 1]: t < m: lower-bound position in level t (old layout); [m]: position of the existing ancestor
    uint32_t* conflict;        // bit 1: two chains share a new node; bit 2: an index is a leaf already
};
// STOP = true (I1): the search ends at the first existing ancestor, inspos[j][t] is written for t <= m.  STOP = false (J1 of the general
// insert, below): continued to the root, inspos[j][t] is written for every t <= height.
template <bool STOP>
__global__ __launch_bounds__(64) void k_tree_ins_plan(const LevelView* views, TreeInsPlan P) {
    const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= P.k) return;
    const uint64_t x = P.idx[j];
    uint32_t* out = P.inspos + j * (size_t)(P.height + 1);
    int m = -1;
    for (int t = 0; t <= P.height; t++) {
        const LevelView L = views[t];
        const uint64_t want = t < 64 ? x >> t : 0;
        const size_t lo = lower_bound_u64(L.idx, L.n, want);
        out[t] = (uint32_t)lo;
        if (m < 0 && lo < L.n && L.idx[lo] == want) {
            m = t;
            if (STOP) break;
        }
    }
    if (m < 0) m = P.height;
    P.m[j] = (uint32_t)m;
    if (m == 0) atomicOr(P.conflict, 2u);          // the leaf exists already
    if (j > 0) {                                    // shares a new node with its left neighbour?
        const uint64_t y = P.idx[j - 1];
        for (int t = 0; t < m; t++)
            if ((t < 64 ? x >> t : 0) == (t < 64 ? y >> t : 0)) { atomicOr(P.conflict, 1u); break; }
    }
}
// Existing nodes of one level to their new positions.  ins_pos: sorted old-layout lower-bound positions of the nodes this level
// gains (n_ins of them); next_ins_pos / n_next: the same for the level above (parent pointers move with it).  The removal path
// (below) passes the level's deleted positions instead: del_pos / n_del, sorted and distinct, old layout; those nodes are dropped
// and the others move down by the number of deletions before them; next_del_pos / n_next_del: the same for the level above.
__device__ __forceinline__ uint32_t count_le(const uint32_t* a, uint32_t n, uint32_t x) {      // # of a[i] <= x, a sorted
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (a[mid] <= x) lo = mid + 1; else hi = mid; }
    return lo;
}
struct RelayoutDel {
    const uint32_t* pos; uint32_t n;               // deleted positions of this level
    const uint32_t* next_pos; uint32_t n_next;     // of the level above
};
__global__ __launch_bounds__(256) void k_tree_relayout(LevelView src, LevelView dst, size_t n_old, const uint32_t* ins_pos, uint32_t n_ins,
                                                       const uint32_t* next_ins_pos, uint32_t n_next, int is_root_level, RelayoutDel del) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_old) return;
    const uint32_t dl = del.n ? count_le(del.pos, del.n, (uint32_t)i) : 0u;
    if (dl && del.pos[dl - 1] == (uint32_t)i) return;                   // a deleted node
    const size_t d = i + count_le(ins_pos, n_ins, (uint32_t)i) - dl;
    dst.idx[d] = src.idx[i];
    dst.v[d] = src.v[i];
    uint32_t w[8];
    ld8(w, src.r + i * 8); st8(dst.r + d * 8, w);
    ld8(w, src.C + i * 8); st8(dst.C + d * 8, w);
    ld8(w, src.H + i * 8); st8(dst.H + d * 8, w);
    dst.has_pad[d] = src.has_pad[i];
    if (src.has_pad[i]) {
        ld8(w, src.padC + i * 8); st8(dst.padC + d * 8, w);
        ld8(w, src.padH + i * 8); st8(dst.padH + d * 8, w);
        ld8(w, src.padr + i * 8); st8(dst.padr + d * 8, w);
    }
    if (!is_root_level) {
        const uint32_t pq = src.parent[i];
        dst.parent[d] = pq + (n_next ? count_le(next_ins_pos, n_next, pq) : 0u) - (del.n_next ? count_le(del.next_pos, del.n_next, pq) : 0u);
    }
}
struct TreeInsArgs {
    size_t k;
    int height;
    const uint64_t* idx; const uint64_t* v; const uint32_t* r;     // the new leaves
    const uint32_t* m;                                              // [k]
    const uint32_t* newpos;                                         // [k][height + 1]: t < m: position of chain node t in the NEW layout; [m]: of the existing ancestor
    uint32_t* pos;                                                  // [k][height + 1] out: node positions at every level (new layout), for U2 / U3
    int32_t* dP; uint64_t* dv; uint32_t* dr;                        // out: the delta for levels >= m
    const uint32_t* pad_seed;                                       // [8]
};
// one wavefront per new leaf; lane t < m handles chain node t
template <int DX>
__global__ __launch_bounds__(64) void k_tree_ins_chain(TableView tbl, const LevelView* views, TreeInsArgs I) {
    const size_t j = blockIdx.x;
    const int t = threadIdx.x, m = (int)I.m[j];
    const uint64_t x = I.idx[j];
    const uint32_t* np = I.newpos + j * (size_t)(I.height + 1);
    // the leaf's own point and reduced blinding (every lane: cheaper than a broadcast of 36 + 8 words)
    uint32_t rl[8];
    ld8(rl, I.r + j * 8);
    rl[7] &= 0x7fffffffu;                          // Scalar::from_bits
    ge_p3 P0;
    leaf_point(P0, tbl, I.v[j], rl);
    sc r0;
    sc_to_mont(r0, rl);
    // lane t: the padding sibling of chain node t (needed for t < m - 1), the padding node at (t, (x >> t) ^ 1)
    const bool has_pad = t < m - 1;
    ge_p3 Pp;
    ge_identity(Pp);
    sc rp;
    sc_zero(rp);
    uint32_t rB[8] = {0}, cB[8] = {0}, hB[8] = {0};
    if (has_pad) {
        uint32_t wide[16];
        padding_draw(wide, I.pad_seed, (uint64_t)t, (x >> t) ^ 1ull);
        padding_from_wide<DX>(Pp, rp, rB, cB, hB, tbl, wide);
    }
    // inclusive prefix sums over the lanes: S_t = sum_{u <= t} pad(u) (points and blindings); chain node t = leaf + S_{t-1}
    ge_p3 S = Pp;
    sc rs = rp;
    for (int off = 1; off < 64; off <<= 1) {
        ge_p3 o, q;
        sc ro, rq;
        for (int i = 0; i < FE_NL; i++) {
            o.X.v[i] = __shfl_up(S.X.v[i], off, 64); o.Y.v[i] = __shfl_up(S.Y.v[i], off, 64);
            o.Z.v[i] = __shfl_up(S.Z.v[i], off, 64); o.T.v[i] = __shfl_up(S.T.v[i], off, 64);
        }
        for (int i = 0; i < 8; i++) ro.v[i] = (uint32_t)__shfl_up((int)rs.v[i], off, 64);
        if (t >= off) { ge_add(q, S, o); S = q; sc_add(rq, rs, ro); rs = rq; }
    }
    ge_p3 E;                                        // exclusive: S_{t-1}
    sc re;
    for (int i = 0; i < FE_NL; i++) {
        E.X.v[i] = __shfl_up(S.X.v[i], 1, 64); E.Y.v[i] = __shfl_up(S.Y.v[i], 1, 64);
        E.Z.v[i] = __shfl_up(S.Z.v[i], 1, 64); E.T.v[i] = __shfl_up(S.T.v[i], 1, 64);
    }
    for (int i = 0; i < 8; i++) re.v[i] = (uint32_t)__shfl_up((int)rs.v[i], 1, 64);
    if (t >= m) return;
    ge_p3 N;
    sc rn;
    if (t == 0) { N = P0; rn = r0; }
    else { ge_add(N, P0, E); sc_add(rn, r0, re); }
    uint32_t cN[8], hN[8], rN[8];
    ge_compress(cN, N);
    sc_from_mont(rN, rn);
    const LevelView L = views[t];
    const size_t d = np[t];
    L.idx[d] = x >> t;
    L.v[d] = I.v[j];
    st8(L.r + d * 8, t == 0 ? rl : rN);             // a leaf keeps its blinding as given (possibly >= l); parents hold the reduced sum
    st8(L.C + d * 8, cN);
    if (t == 0) { node_hash32_x<DX>(tbl.digest, hN, cN); st8(L.H + d * 8, hN); }       // (parents' hashes: k_tree_upd_hash, level by level)
    L.has_pad[d] = has_pad ? 1 : 0;
    if (has_pad) store_pad_record(L, d, cB, hB, rB);
    L.parent[d] = np[t + 1];
    uint32_t* pos = I.pos + j * (size_t)(I.height + 1);
    pos[t] = (uint32_t)d;
    if (t == m - 1) {
        // the sibling S of the chain's top node is real and adjacent in the sorted level; its padding sibling goes away
        const size_t s = ((x >> t) & 1ull) ? d - 1 : d + 1;
        uint32_t oc[8], orr[8];
        ld8(oc, L.padC + s * 8);
        ld8(orr, L.padr + s * 8);
        L.has_pad[s] = 0;
        ge_p3 po, npo, dd;
        (void)ge_decompress(po, oc);
        ge_neg(npo, po);
        ge_add(dd, N, npo);
        st_p3(I.dP + j * 40, dd);
        sc mo, md;
        sc_to_mont(mo, orr);
        sc_sub(md, rn, mo);
        for (int i = 0; i < 8; i++) I.dr[j * 8 + i] = md.v[i];
        I.dv[j] = I.v[j];
        // positions of the existing ancestors, by the (already moved) parent pointers
        size_t p = np[m];
        pos[m] = (uint32_t)p;
        for (int q = m; q < I.height; q++) { p = views[q].parent[p]; pos[q + 1] = (uint32_t)p; }
    }
}

// ------------------------------------------------------------------------------------- incremental insert, general
// dapol_tree_insert's in-place path for ANY batch of new leaves: chains may share nodes (a sibling pair, a whole new subtree), which
// the wavefront-per-chain prefix sums of I3 cannot express.  It is the removal's mirror image: the host plans the forest
// (plan_insert_general), the levels that gain nodes are rewritten by k_tree_relayout, and every FRESH node -- a new one, or an existing
// ancestor of a new leaf -- is merged from its children level by level, bottom-up.
//   J1  k_tree_ins_plan<0>    per new leaf: as I1, continued to the root: the lower bound of x >> t at EVERY level
//   J2  k_tree_relayout       per level that gains nodes (existing nodes only)
//   J3  k_tree_ins_struct     per new node: idx, parent, has_pad = 0; a chain top also clears has_pad of its real sibling S
//   J4  k_tree_ins_leaves     per new leaf: its node, its extended point
//   J5  k_tree_edit_pad<1>    per new node with a padding sibling: the padding node's record, and its extended point
//   J6  k_tree_edit_merge<1>  per level: every fresh node = the parent of its children
// A point this call has produced is never decoded again: J4 - J6 leave the extended point of every fresh node and every new padding
// node in the call's scratch (160 bytes a slot; node slots alternate between two halves by level parity), and a merge reads a child
// made by this call from there.  Only an untouched existing sibling, or an existing padding record, is decoded from its 32 bytes.
// On the private part of a new chain both children are fresh, so a merge pays one encoding and no decoding -- the removal's merge pays
// two decodings and an encoding, each an inverse square root, on what is a serial chain of single-lane launches for a small batch.
// Compiler report, gfx950: profiles/tree_node_routines.txt -- two waves a SIMD for the kernels that hold a point, which a launch of a
// few lanes does not notice and a launch of thousands shares with the build's own kernels.
// (J1 searches every level; above m the parent pointers would give the same positions for one load a level -- not done yet, see
// DESIGN.md 4.3 on the 0.1 ms this costs a small batch.)  conflict bit 1 (chains that share a node) only selects the path here.
struct TreeInsGeneral {
    size_t n_new, k;
    const uint32_t *lvl, *pos, *parent, *sib, *idx_lo, *idx_hi;    // [n_new]: the new nodes (plan_insert_general's n_*)
    const uint32_t* leaf_pos;                                       // [k]
    const uint64_t* v; const uint32_t* r;                           // [k], [k][8]: the new leaves, sorted by index
    int32_t* node_ext;                                              // [2][slots][40]: fresh nodes, half = level & 1
};
// J3
__global__ __launch_bounds__(64) void k_tree_ins_struct(const LevelView* views, TreeInsGeneral G) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= G.n_new) return;
    const LevelView L = views[G.lvl[i]];
    const size_t d = G.pos[i];
    L.idx[d] = (uint64_t)G.idx_lo[i] | ((uint64_t)G.idx_hi[i] << 32);
    L.parent[d] = G.parent[i];
    L.has_pad[d] = 0;
    if (G.sib[i] != 0xffffffffu) L.has_pad[G.sib[i]] = 0;          // a chain top: S's padding sibling (at this node's position) goes away
}
// J4
template <int DX>
__global__ __launch_bounds__(64) void k_tree_ins_leaves(TableView tbl, const LevelView* views, TreeInsGeneral G) {
    const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= G.k) return;
    const LevelView L = views[0];
    const size_t d = G.leaf_pos[j];
    uint32_t rl[8], c[8], h[8];
    ld8(rl, G.r + j * 8);
    rl[7] &= 0x7fffffffu;                          // Scalar::from_bits; the leaf keeps its blinding as given (possibly >= l)
    ge_p3 P0;
    leaf_node<DX>(P0, c, h, tbl, G.v[j], rl);
    L.v[d] = G.v[j];
    st8(L.r + d * 8, rl);
    st8(L.C + d * 8, c);
    st8(L.H + d * 8, h);
    st_p3(G.node_ext + j * 40, P0);
}
// J5 and R2 of the removal (below): real node pos[i] of level level[i] gains its padding sibling.  KEEP_EXT: the padding node's
// extended point stays in ext[i] for the merges above it.  LevelT is deduced from the plan's level list -- bytes in the removal's, words
// in the insert's -- so the two instantiations the stage lists call <0> and <1> are <false, uint8_t> and <true, uint32_t> in the code object.
template <bool KEEP_EXT, int DX, typename LevelT>
__global__ __launch_bounds__(64) void k_tree_edit_pad(TableView tbl, const LevelView* views, size_t n, const LevelT* level, const uint32_t* pos,
                                                      const uint32_t* pad_seed, int32_t* ext) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int t = (int)level[i];
    const size_t s = pos[i];
    const LevelView L = views[t];
    uint32_t rB[8], cB[8], hB[8];
    ge_p3 pB;
    padding_node<DX>(pB, rB, cB, hB, tbl, pad_seed, (uint64_t)t, L.idx[s] ^ 1ull);
    store_pad_record(L, s, cB, hB, rB);
    L.has_pad[s] = 1;
    if (KEEP_EXT) st_p3(ext + i * 40, pB);
}
// J6 and R3 of the removal, one level: a record of e per node of nxt to make again from its children in cur (new layout): the node's
// position | the position of one of its children; the other child is that child's padding record or real neighbour, as k_tree_merge
// pairs them.  SLOTS = false (removal, 2 words a record): both children's points are decoded from their encodings, which are the
// tree's own and always decode.  SLOTS = true (insert, 5 words): | the node's slot | the child's slot | the other child: a slot of
// cur's half, 0x80000000 | pad slot, or 0xffffffff = decode it; the node's point is left in its slot.
template <bool SLOTS, int DX>
__global__ __launch_bounds__(64) void k_tree_edit_merge(int digest, LevelView cur, LevelView nxt, size_t n, const uint32_t* e, const int32_t* ext_cur,
                                                        int32_t* ext_nxt, const int32_t* pad_ext) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t* rec = e + (SLOTS ? 5 : 2) * i;
    const size_t p = rec[0], c = rec[1];
    const bool left = (cur.idx[c] & 1ull) == 0;
    uint32_t cA[8], hA[8], rA[8], cB[8], hB[8], rB[8];
    const uint64_t vA = cur.v[c];
    uint64_t vB;
    ld8(cA, cur.C + c * 8); ld8(hA, cur.H + c * 8); ld8(rA, cur.r + c * 8);
    load_other_child(cB, hB, rB, &vB, cur, c, left);
    ge_p3 pA, pB, pp;
    if (SLOTS) {
        const uint32_t other = rec[4];
        ld_p3(pA, ext_cur + (size_t)rec[3] * 40);
        if (other == 0xffffffffu) (void)ge_decompress(pB, cB);
        else if (other & 0x80000000u) ld_p3(pB, pad_ext + (size_t)(other & 0x7fffffffu) * 40);
        else ld_p3(pB, ext_cur + (size_t)other * 40);
    } else {
        (void)ge_decompress(pA, cA);
        (void)ge_decompress(pB, cB);
    }
    uint32_t rp[8], cp[8], hp[8];
    merge_parent<DX>(pp, rp, cp, hp, digest, left, pA, pB, rA, rB, cA, cB, hA, hB);
    nxt.v[p] = vA + vB;                            // u64 wrap == release-mode Rust (node.rs:72)
    st8(nxt.r + p * 8, rp);
    st8(nxt.C + p * 8, cp);
    st8(nxt.H + p * 8, hp);
    if (SLOTS) st_p3(ext_nxt + (size_t)rec[2] * 40, pp);
}

// ------------------------------------------------------------------------------------- incremental remove
// Removing leaves (dapol_tree_remove) is the mirror image of the insert.  A real node dies iff all its real children die (a node
// whose has_pad is set has one real child); the dead nodes of a removed leaf form a chain from the leaf up to a CHAIN TOP whose
// parent survives.  That parent had two real children, so the top's sibling S survives: S gains has_pad and the padding node of
// the top's position (level t, idx_S ^ 1) -- the very draw k_tree_pad_level makes for it.  Padding records of dead nodes go with
// them; a survivor never loses has_pad.  Chains may share nodes (two sibling leaves, a whole subtree): the host finds the dead
// nodes and the touched survivors level by level from R0's positions, and every touched survivor is merged again from its children.
//   R0  k_tree_find_paths     per removed leaf: its node position and has_pad flag at every level (parent pointers); a missing index
//                             reports DAPOL_ERR_UNKNOWN_LEAF before anything has been written
//   R1  k_tree_relayout       per level that loses nodes: the survivors, compacted (with the deletions of RelayoutDel)
//   R2  k_tree_edit_pad<0>    per chain top: S's new padding sibling (level / pos = level and new position of S)
//   R3  k_tree_edit_merge<0>  per level, bottom-up: every touched survivor = the parent of its children, as k_tree_merge makes it
// A survivor is re-merged rather than moved by a delta: the parent of a chain top may also change through removals under S, and
// chain tops sit at different levels, so the deltas of one ancestor would have to be gathered across chains; a merge reads what
// is already there (children of the level below, the padding records of R2) and needs no bookkeeping between chains.

// ------------------------------------------------------------------------------------- mixed edit in place
// dapol_tree_apply: removals, new leaves and replacements as ONE edit.  The host plans the forest of touched nodes once
// (plan_apply, tree_edit_plan.inc): which die, which are born, which survive; then every level up to the highest that changes is
// rewritten once with both lists, and every alive touched node is made once, bottom-up.
//   A0  k_tree_apply_plan     per edited index: lower bound, existence and has_pad of its ancestor at every level (a search down to
//                             the first ancestor that exists, parent pointers from there)
//   A1  k_tree_relayout       per level below the highest that changes: survivors move by (born before) - (dead before)
//   A2  k_tree_apply_struct   per alive touched node, and per untouched sibling S of a node that died or was born: has_pad as it is
//                             afterwards; a born node also gets idx and parent
//   A3  k_tree_ins_leaves     per put, new or replacing: the leaf's node at its new position, its extended point in its slot
//   A4  k_tree_edit_pad<1>    per padding node the plan lists (the old tree did not hold that position's record)
//   A5  k_tree_apply_merge    per level: every alive touched node = the parent of an anchor child and the anchor's other child
// The insert's rule holds: a point this call has produced is never decoded again.  Either child of a merge comes from a slot (a
// touched node or put leaf), a pad slot, or is decoded (an untouched real node, an old padding record) -- so a survivor above a dead
// chain top, whose children are the untouched S and S's new padding node, pays one decoding where the removal's merge pays two.
// Compiler report, gfx950: profiles/tree_apply_kernel_resources.txt.
struct TreeApplyPlan {
    size_t k;
    int height;
    const uint64_t* idx;       // [k] sorted, distinct: the removed and the put indexes together
    uint32_t* pos;             // [k][height + 1]: old-layout lower bound of idx >> t (the node's position where it exists)
    uint8_t* flag;             // [k][height + 1]: bit 0 = the node exists, bit 1 = its has_pad
};
// A0.  Nothing of the tree is written.
__global__ __launch_bounds__(64) void k_tree_apply_plan(const LevelView* views, TreeApplyPlan P) {
    const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= P.k) return;
    const uint64_t x = P.idx[j];
    const size_t stride = (size_t)P.height + 1;
    uint32_t* pos = P.pos + j * stride;
    uint8_t* flag = P.flag + j * stride;
    bool found = false;
    size_t p = 0;
    for (int t = 0; t <= P.height; t++) {
        const LevelView L = views[t];
        if (!found) {
            const uint64_t want = t < 64 ? x >> t : 0;
            p = lower_bound_u64(L.idx, L.n, want);
            found = p < L.n && L.idx[p] == want;
        }
        pos[t] = (uint32_t)p;
        flag[t] = !found ? 0 : (t < P.height && L.has_pad[p]) ? 3 : 1;
        if (found && t < P.height) p = L.parent[p];
    }
}
struct TreeApplyStruct {
    size_t n;
    const uint32_t *lvl, *pos, *parent, *flag, *idx_lo, *idx_hi;   // [n]: plan_apply's s_*
};
// A2
__global__ __launch_bounds__(64) void k_tree_apply_struct(const LevelView* views, TreeApplyStruct G) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= G.n) return;
    const LevelView L = views[G.lvl[i]];
    const size_t d = G.pos[i];
    const uint32_t f = G.flag[i];
    if (f & 1u) {
        L.idx[d] = (uint64_t)G.idx_lo[i] | ((uint64_t)G.idx_hi[i] << 32);
        L.parent[d] = G.parent[i];
    }
    L.has_pad[d] = (uint8_t)((f >> 1) & 1u);
}
// A5, one level: five words per node of nxt to make from its children in cur (new layout): the node's position | the position of its
// anchor child | the node's slot | the anchor's slot, or 0xffffffff = decode it | the other child (the anchor's padding record or
// real neighbour, as k_tree_merge pairs them): a slot of cur's half, 0x80000000 | pad slot, or 0xffffffff = decode it.  The node's
// point is left in its slot.
template <int DX>
__global__ __launch_bounds__(64) void k_tree_apply_merge(int digest, LevelView cur, LevelView nxt, size_t n, const uint32_t* e, const int32_t* ext_cur,
                                                         int32_t* ext_nxt, const int32_t* pad_ext) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t* rec = e + 5 * i;
    const size_t p = rec[0], c = rec[1];
    const bool left = (cur.idx[c] & 1ull) == 0;
    uint32_t cA[8], hA[8], rA[8], cB[8], hB[8], rB[8];
    const uint64_t vA = cur.v[c];
    uint64_t vB;
    ld8(cA, cur.C + c * 8); ld8(hA, cur.H + c * 8); ld8(rA, cur.r + c * 8);
    load_other_child(cB, hB, rB, &vB, cur, c, left);
    ge_p3 pA, pB, pp;
    const uint32_t anchor = rec[3], other = rec[4];
    if (anchor == 0xffffffffu) (void)ge_decompress(pA, cA);
    else ld_p3(pA, ext_cur + (size_t)anchor * 40);
    if (other == 0xffffffffu) (void)ge_decompress(pB, cB);
    else if (other & 0x80000000u) ld_p3(pB, pad_ext + (size_t)(other & 0x7fffffffu) * 40);
    else ld_p3(pB, ext_cur + (size_t)other * 40);
    uint32_t rp[8], cp[8], hp[8];
    merge_parent<DX>(pp, rp, cp, hp, digest, left, pA, pB, rA, rB, cA, cB, hA, hB);
    nxt.v[p] = vA + vB;                            // u64 wrap == release-mode Rust (node.rs:72)
    st8(nxt.r + p * 8, rp);
    st8(nxt.C + p * 8, cp);
    st8(nxt.H + p * 8, hp);
    st_p3(ext_nxt + (size_t)rec[2] * 40, pp);
}

// ------------------------------------------------------------------------------------- small trees, by phases
// k_tree_merge makes a level in one pass, which is right for millions of nodes (one trip through HBM) and wrong for a tree of a
// few thousand (the reference's `build` criterion group, benches/dapol.rs:24-57; dapol_tree_update): a level is then ONE lane's
// chain -- a padding node's fixed-base product and encoding, the parent's encoding, the hashes: 0.16 ms -- times `height`.  Only
// three things really are sequential over the levels: who is whose parent (integers), the parents' POINTS (one addition per
// level) and the hash chain; the fixed-base products and the inverse square roots of all levels can run side by side.  So:
//   S  k_tree_structure_small   one block walks all levels: parent slots, pairs, index of every parent          (integers)
//   P  k_tree_padding_all       every padding node of every level: blinding, point, encoding, hash              (one launch)
//   M  k_tree_sum_level         level by level: v, r and the extended point of every parent                     (height launches)
//   C  k_tree_compress_all      the encodings of all parents of all levels                                      (one launch)
//   H  k_tree_hash_level        level by level: the parents' hashes                                             (height launches)
// The arrays they leave are exactly k_tree_merge's.
enum { TREE_SMALL_MAX = 8192, TREE_SMALL_PER = 8 };   // leaves; nodes per thread of the structure block (1024 threads)

__global__ __launch_bounds__(1024) void k_tree_structure_small(int height, const LevelView* views, uint32_t* cnt) {
    __shared__ uint32_t wave_tot[16];
    __shared__ uint64_t sidx[2][TREE_SMALL_MAX];                     // the level's node indexes and the next level's (128 KB of LDS)
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    uint32_t cur_n = cnt[0];
    {
        const uint64_t* idx0 = views[0].idx;
        for (uint32_t i = (uint32_t)t; i < cur_n; i += 1024) sidx[0][i] = idx0[i];
    }
    __syncthreads();
    for (int k = 0; k < height; k++) {
        const LevelView cur = views[k], nxt = views[k + 1];
        const uint64_t* src = sidx[k & 1];
        uint64_t* dst = sidx[(k + 1) & 1];
        const uint32_t base = (uint32_t)t * TREE_SMALL_PER;
        uint64_t v[TREE_SMALL_PER + 1];
        for (int e = 0; e <= TREE_SMALL_PER; e++) v[e] = (base + e < cur_n) ? src[base + e] : ~0ull;
        const uint64_t prev = (base > 0 && base <= cur_n) ? src[base - 1] : ~0ull;
        uint32_t f = 0, local = 0;                                   // bit e: node base + e starts a new parent
        for (int e = 0; e < TREE_SMALL_PER; e++) {
            const uint32_t i = base + e;
            const uint64_t before = e ? v[e - 1] : prev;
            if (i < cur_n && (i == 0 || (v[e] >> 1) != (before >> 1))) { f |= 1u << e; local++; }
        }
        uint32_t x = local;
        for (int off = 1; off < 64; off <<= 1) {
            uint32_t y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63) wave_tot[wv] = x;
        __syncthreads();
        uint32_t add = 0, all = 0;
        for (int w = 0; w < 16; w++) { if (w < wv) add += wave_tot[w]; all += wave_tot[w]; }
        uint32_t q = x - local + add;                                // parents started before this thread's nodes
        for (int e = 0; e < TREE_SMALL_PER; e++) {
            const uint32_t i = base + e;
            if (i >= cur_n) break;
            if ((f >> e) & 1u) {
                const bool pair = (i + 1 < cur_n) && v[e + 1] == (v[e] ^ 1ull);
                cur.parent[i] = q;
                cur.has_pad[i] = pair ? 0 : 1;
                nxt.idx[q] = v[e] >> 1;
                dst[q] = v[e] >> 1;
                q++;
            } else {                                                 // the second node of a pair: its sibling's parent
                cur.parent[i] = q - 1;
                cur.has_pad[i] = 0;
            }
        }
        cur_n = all;
        if (t == 0) cnt[k + 1] = all;
        __syncthreads();                                             // dst is the next level's src; wave_tot is reused
    }
}
// Which level a flattened node number belongs to (lvl_off[k] = nodes below level k by the host-side bounds).
__device__ __forceinline__ int tree_level_of(size_t t, const uint32_t* lvl_off, int nlev) {
    int k = 0;
    while (k + 1 < nlev && t >= lvl_off[k + 1]) k++;
    return k;
}
template <int DX>
__global__ __launch_bounds__(64) void k_tree_padding_all(TableView tbl, const LevelView* views, int height, const uint32_t* cnt, const uint32_t* lvl_off,
                                                        const uint32_t* pad_seed, int32_t* extpad) {
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= lvl_off[height]) return;                                // (the root level has no sibling)
    const int level = tree_level_of(t, lvl_off, height);
    const size_t i = t - lvl_off[level];
    const LevelView cur = views[level];
    if (i >= cnt[level] || !cur.has_pad[i]) return;
    uint32_t rB[8], cB[8], hB[8];
    ge_p3 pB;
    padding_node<DX>(pB, rB, cB, hB, tbl, pad_seed, (uint64_t)level, cur.idx[i] ^ 1ull);
    store_pad_record(cur, i, cB, hB, rB);
    st_p3(extpad + t * 40, pB);
}
__global__ __launch_bounds__(64) void k_tree_sum_level(LevelView cur, LevelView nxt, int level, const uint32_t* cnt, const int32_t* ext_cur,
                                                      const int32_t* extpad_cur, int32_t* ext_nxt) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= cnt[level]) return;
    const uint32_t q = cur.parent[i];
    if (i > 0 && cur.parent[i - 1] == q) return;                    // the second node of a pair
    const bool pair = !cur.has_pad[i];
    uint32_t rA[8], rB[8], rp[8];
    ge_p3 pA, pB, pp;
    ld8(rA, cur.r + i * 8);
    ld_p3(pA, ext_cur + i * 40);
    uint64_t vB = 0;
    if (pair) {
        ld8(rB, cur.r + (i + 1) * 8);
        ld_p3(pB, ext_cur + (i + 1) * 40);
        vB = cur.v[i + 1];
    } else {
        ld8(rB, cur.padr + i * 8);
        ld_p3(pB, extpad_cur + i * 40);
    }
    sc_add_words(rp, rA, rB);
    ge_add(pp, pA, pB);
    nxt.v[q] = cur.v[i] + vB;                                        // u64 wrap == release-mode Rust (node.rs:72)
    st8(nxt.r + (size_t)q * 8, rp);
    st_p3(ext_nxt + (size_t)q * 40, pp);
}
__global__ __launch_bounds__(64) void k_tree_compress_all(const LevelView* views, int height, const uint32_t* cnt, const uint32_t* lvl_off,
                                                         const int32_t* ext_all) {
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x + lvl_off[1];       // levels 1 .. height
    if (t >= lvl_off[height + 1]) return;
    const int level = tree_level_of(t, lvl_off, height + 1);
    const size_t q = t - lvl_off[level];
    if (q >= cnt[level]) return;
    ge_p3 p;
    uint32_t c[8];
    ld_p3(p, ext_all + t * 40);
    ge_compress(c, p);
    st8(views[level].C + q * 8, c);
}
template <int DX>
__global__ __launch_bounds__(64) void k_tree_hash_level(int digest, LevelView cur, LevelView nxt, int level, const uint32_t* cnt) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= cnt[level]) return;
    const uint32_t q = cur.parent[i];
    if (i > 0 && cur.parent[i - 1] == q) return;
    const bool pair = !cur.has_pad[i];
    uint32_t cA[8], hA[8], cB[8], hB[8], hp[8];
    ld8(cA, cur.C + i * 8);
    ld8(hA, cur.H + i * 8);
    load_other_child(cB, hB, nullptr, nullptr, cur, i, true);        // (this lane is the left node of a pair, or has a padding sibling)
    parent_hash<DX>(digest, hp, pair || (cur.idx[i] & 1ull) == 0, cA, cB, hA, hB);
    st8(nxt.H + (size_t)q * 8, hp);
}

// Validation of the leaf index array: strictly increasing and below 2^height (smtree panics otherwise).
__global__ void k_tree_check_leaves(size_t n, const uint64_t* idx, int index_bits, int levels, uint32_t* bad) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool b = (index_bits < 64 && (idx[i] >> index_bits) != 0) || (i > 0 && idx[i] <= idx[i - 1]);
    if (levels < 64 && (idx[i] >> levels) != (idx[0] >> levels)) b = true;     // all leaves in one shard subtree
    if (b) atomicOr(bad, 1u);
}

// Leaf lookup + sibling gather, one lane per (proof, level).  Output party order: root side first (or leaf first, see k_tree_path_level).
struct PathOut {
    uint32_t* C;     // [b][height][8] or null
    uint32_t* H;
    uint64_t* v;     // [b][height]
    uint32_t* r;     // [b][height][8]
};
__global__ void k_tree_find_leaves(size_t b, const uint64_t* want, size_t n, const uint64_t* idx, uint32_t* pos, uint32_t* missing) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b) return;
    uint64_t w = want[t];
    size_t lo = lower_bound_u64(idx, n, w);
    if (lo < n && idx[lo] == w) pos[t] = (uint32_t)lo;
    else { pos[t] = 0xffffffffu; atomicOr(missing, 1u); }
}
// Walks each proof's leaf up to the root: writes the sibling met at every level (one launch for the whole path; a lane's
// chain is `height` dependent gathers, the lanes of a launch cover the proofs).
__global__ __launch_bounds__(64) void k_tree_path_walk(size_t b, uint32_t* pos, const LevelView* views, int height, int n_upper, int leaf_first, PathOut out) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b) return;
    uint32_t p = pos[t];
    if (p == 0xffffffffu) return;
    for (int level = 0; level < height; level++) {
        const LevelView lv = views[level];
        // sibling order of a proof (dapol_wire_config.siblings_leaf_first): root side first (slot 0 = the root's child) or leaf first
        size_t slot = t * (size_t)(height + n_upper) + (size_t)(leaf_first ? level : n_upper + height - 1 - level);
        uint32_t c[8], h[8], r[8];
        uint64_t v;
        load_other_child(c, h, r, &v, lv, p);
        if (out.C) st8(out.C + slot * 8, c);
        if (out.H) st8(out.H + slot * 8, h);
        if (out.v) out.v[slot] = v;
        if (out.r) st8(out.r + slot * 8, r);
        p = lv.parent[p];
    }
    pos[t] = p;
}
// Siblings above a shard root are the same for every leaf of the shard: broadcast them into slots [0, n_upper).
__global__ void k_tree_path_upper(size_t b, int height, int n_upper, int leaf_first, const uint32_t* uC, const uint32_t* uH, const uint64_t* uv,
                                  const uint32_t* ur, PathOut out) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b * (size_t)n_upper) return;
    size_t e = t / n_upper;
    int u = (int)(t - e * n_upper);
    size_t slot = e * (size_t)(height + n_upper) + (size_t)(leaf_first ? height + (n_upper - 1 - u) : u);     // u = 0: the root's child
    uint32_t w[8];
    if (out.C) { ld8(w, uC + u * 8); st8(out.C + slot * 8, w); }
    if (out.H) { ld8(w, uH + u * 8); st8(out.H + slot * 8, w); }
    if (out.v) out.v[slot] = uv[u];
    if (out.r) { ld8(w, ur + u * 8); st8(out.r + slot * 8, w); }
}

// ------------------------------------------------------------------------------------- 64-byte node hashes (Blake2b)
// Dapol<blake2::Blake2b, R> on the new_blank + build path (src/tests.rs:100-106; mod.rs:196-208 has no digest check).  Everything
// of a node but its hash -- structure, values, blindings, commitments, padding nodes -- is independent of the digest, so a
// context with a 64-byte digest builds (and updates) its trees with the kernels above and then lays the hash chain over them:
// per level an array of 16-word hashes for the real nodes and one for their padding siblings (WideView), filled bottom-up, one
// launch per level.  The 8-word H arrays of such a tree are not used.
struct WideView {
    uint32_t* H;       // [n][16]  hash of real node i
    uint32_t* padH;    // [n][16]  hash of the padding sibling of real node i (where has_pad[i])
};
__device__ __forceinline__ void ld16(uint32_t* w, const uint32_t* p) { ld8(w, p); ld8(w + 8, p + 8); }
__device__ __forceinline__ void st16(uint32_t* p, const uint32_t* w) { st8(p, w); st8(p + 8, w + 8); }
// leaves: H = D(C)  (DapolNode::new, src/dapol/node.rs:34-36)
__global__ __launch_bounds__(256) void k_wide_hash_leaves(size_t n, const uint32_t* C, uint32_t* H16) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t c[8], h[16];
    ld8(c, C + i * 8);
    blake2b_hash32(h, c);
    st16(H16 + i * 16, h);
}
// level k -> k + 1: one lane per child that owns its parent (the left child of a real pair, or the real child of a padded pair):
// the padding sibling's hash D(C_pad), then Mergeable::merge's D(C_L || C_R || H_L || H_R) (node.rs:66-77).
__global__ __launch_bounds__(256) void k_wide_hash_level(LevelView cur, WideView wcur, WideView wnxt) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cur.n) return;
    const bool left = (cur.idx[i] & 1ull) == 0, padded = cur.has_pad[i] != 0;
    if (!padded && !left) return;                          // the right child of a real pair: its left neighbour does the parent
    uint32_t cA[8], cB[8], hA[16], hB[16], hp[16];
    ld8(cA, cur.C + i * 8);
    ld16(hA, wcur.H + i * 16);
    if (padded) {
        ld8(cB, cur.padC + i * 8);
        blake2b_hash32(hB, cB);
        st16(wcur.padH + i * 16, hB);
    } else {
        ld8(cB, cur.C + (i + 1) * 8);
        ld16(hB, wcur.H + (i + 1) * 16);
    }
    if (left) blake2b_hash192(hp, cA, cB, hA, hB);
    else blake2b_hash192(hp, cB, cA, hB, hA);
    st16(wnxt.H + (size_t)cur.parent[i] * 16, hp);
}
// the 64-byte hashes of the siblings along b paths (k_tree_path_walk's walk; pos = the leaves' positions, left untouched)
__global__ __launch_bounds__(64) void k_wide_path_walk(size_t b, const uint32_t* pos, const LevelView* views, const WideView* wviews, int height, int n_upper,
                                                      int leaf_first, uint32_t* outH16) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b) return;
    uint32_t p = pos[t];
    if (p == 0xffffffffu) return;
    for (int level = 0; level < height; level++) {
        const LevelView lv = views[level];
        const WideView wv = wviews[level];
        const size_t slot = t * (size_t)(height + n_upper) + (size_t)(leaf_first ? level : n_upper + height - 1 - level);
        uint32_t h[16];
        if (lv.has_pad[p]) ld16(h, wv.padH + (size_t)p * 16);
        else ld16(h, wv.H + ((lv.idx[p] & 1ull) ? (size_t)p - 1 : (size_t)p + 1) * 16);
        st16(outH16 + slot * 16, h);
        p = lv.parent[p];
    }
}

// Mergeable::merge on compressed records
template <int HW>
__device__ __forceinline__ void ldh(uint32_t* w, const uint32_t* p) { ld8(w, p); if (HW == 16) ld8(w + 8, p + 8); }
template <int HW>
__device__ __forceinline__ void sth(uint32_t* p, const uint32_t* w) { st8(p, w); if (HW == 16) st8(p + 8, w + 8); }
template <int HW, int DX>
__global__ void k_merge_records(int dg, size_t n, const uint32_t* CL, const uint32_t* HL, const uint64_t* vL, const uint32_t* rL,
                                const uint32_t* CR, const uint32_t* HR, const uint64_t* vR, const uint32_t* rR, uint32_t* C, uint32_t* H,
                                uint64_t* v, uint32_t* r, uint32_t* bad) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t cl[8], cr[8], hl[HW], hr[HW], cp[8], hp[HW];
    ld8(cl, CL + i * 8); ld8(cr, CR + i * 8); ldh<HW>(hl, HL + i * HW); ldh<HW>(hr, HR + i * HW);
    ge_p3 a, b, p;
    bool ok = ge_decompress(a, cl) & ge_decompress(b, cr);
    if (!ok) { atomicOr(bad, 1u); return; }
    ge_add(p, a, b);
    ge_compress(cp, p);
    node_hash_parent_w<HW, DX>(dg, hp, cl, cr, hl, hr);
    st8(C + i * 8, cp);
    sth<HW>(H + i * HW, hp);
    if (v) {
        uint32_t ra[8], rb[8], rp[8];
        ld8(ra, rL + i * 8); ld8(rb, rR + i * 8);
        sc_add_words(rp, ra, rb);
        st8(r + i * 8, rp);
        v[i] = vL[i] + vR[i];
    }
}

}  // namespace dapol

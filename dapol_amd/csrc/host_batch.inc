// Batched inclusion proofs: Dapol::generate_proof_batch for k > 1 leaves (src/dapol/mod.rs:172-190) and
// DapolProof::verify_batch (src/proof/mod.rs:49-54).  ONE proof covers all k leaves: the deduplicated siblings of the
// batched Merkle paths (smtree::MerkleProof::new_batch) and one R::generate_proof over exactly those siblings.
//
// Sibling order (smtree's own order is not pinned by anything in the reference repository -- DESIGN.md section 2):
// level by level from the root side (dapol_wire_config.siblings_leaf_first = 1: from the leaf level up), left to right within a
// level.  For k = 1 this is dapol_tree_paths' order.
// Included from dapol_hip.hip after the prover's and the verifier's files.

struct BatchSib { int level; uint64_t index; uint32_t src_leaf; };      // level 0 = leaves; src_leaf: a leaf below the sibling's sibling

// leaf_idx strictly increasing and < 2^height.  Pure index arithmetic.
static bool batch_plan(int height, size_t k, const uint64_t* leaf, std::vector<BatchSib>& sibs) {
    sibs.clear();
    if (height < 0 || height > 64 || k == 0) return false;
    for (size_t i = 0; i < k; i++) {
        if (height < 64 && (leaf[i] >> height)) return false;
        if (i && leaf[i] <= leaf[i - 1]) return false;
    }
    const bool leaf_first = g_wire.siblings_leaf_first != 0;
    for (int step = 0; step < height; step++) {
        const int L = leaf_first ? step : height - 1 - step;
        size_t i = 0;
        while (i < k) {
            uint64_t x = leaf[i] >> L;
            size_t j = i;
            while (j < k && (leaf[j] >> L) == x) j++;                    // [i, j): the leaves below ancestor x
            bool has_sibling;
            if (x & 1) has_sibling = i > 0 && (leaf[i - 1] >> L) == (x ^ 1);
            else has_sibling = j < k && (leaf[j] >> L) == (x ^ 1);
            if (!has_sibling) sibs.push_back({L, x ^ 1, (uint32_t)i});
            i = j;
        }
    }
    return true;
}

int32_t dapol_batch_siblings(int32_t height, size_t k, const uint64_t* leaf_idx, size_t* n_siblings, uint8_t* sib_level, uint64_t* sib_index) {
    WIRE_SCOPE();
    if (!leaf_idx || !n_siblings) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (height < 0 || height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    std::vector<BatchSib> sibs;
    if (!batch_plan(height, k, leaf_idx, sibs)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "leaf indexes must be non-empty, strictly increasing and below 2^height");
    *n_siblings = sibs.size();
    for (size_t i = 0; i < sibs.size(); i++) {
        if (sib_level) sib_level[i] = (uint8_t)sibs[i].level;
        if (sib_index) sib_index[i] = sibs[i].index;
    }
    return DAPOL_OK;
}

// One nonce seed per batch: the caller's seed chained through the leaf list, so that a batch never shares a nonce
// stream with the single-leaf proof of its first leaf (which uses the caller's seed itself).
__global__ void k_batch_seed(const uint32_t* seed8, size_t k, const uint64_t* leaf_idx, uint32_t* out8) {
    if (blockIdx.x || threadIdx.x) return;
    uint32_t s[8], w[16];
    for (int i = 0; i < 8; i++) s[i] = seed8[i];
    for (size_t i = 0; i < k; i++) {
        seed_wide(w, s, 4u, leaf_idx[i], (uint64_t)i);
        for (int j = 0; j < 8; j++) s[j] = w[j];
    }
    for (int i = 0; i < 8; i++) out8[i] = s[i];
}
// sibling i of the batch = record src[i] of the gathered single-leaf paths
__global__ void k_batch_gather(size_t n, const uint32_t* src, PathOut in, PathOut out, int hw /* words of a node hash: 8 or 16 */) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    size_t s = src[i];
    uint32_t w[8];
    ld8(w, in.C + s * 8); st8(out.C + i * 8, w);
    for (int q = 0; q < hw; q += 8) { ld8(w, in.H + s * hw + q); st8(out.H + i * hw + q, w); }
    ld8(w, in.r + s * 8); st8(out.r + i * 8, w);
    out.v[i] = in.v[s];
}

// What a batch asks of its policy: the plan over its S siblings, the words of its blob and (max_m != null) its widest sub-proof.
static int32_t batch_policy_plan(const dapol_ctx* ctx, size_t S, int policy, int agg, int n_bits, std::vector<SubProof>& plan, size_t& words, int* max_m = nullptr) {
    if (!policy_plan(policy, (int)S, agg, plan)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "aggregation_factor must be within [0, number of siblings]");
    if (dapol_range_proof_size(n_bits, 1) == 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "n_bits must be 8/16/32/64");
    words = 0;
    for (auto& s : plan) {
        if (s.m > ctx->max_parties) return fail(DAPOL_ERR_INVALID_ARGUMENT, "aggregation needs more parties than the context was created for");
        if (max_m && s.m > *max_m) *max_m = s.m;
        words += dapol_range_proof_size(n_bits, s.m) / 4;
    }
    return DAPOL_OK;
}
// The tail of both batch provers: the batch's own seed (k > 1), R::generate_proof over the S siblings in HBM, the blob back.
static int32_t batch_prove_tail(dapol_ctx* ctx, const std::vector<SubProof>& plan, size_t k, const uint64_t* d_leaf, size_t S, const uint64_t* sv, const uint32_t* sr,
                                const uint32_t* sC, int n_bits, const uint32_t* d_seed, size_t words, uint8_t* range_out) {
    DevBuf<uint32_t> bseed, dout;
    HIPCHK(bseed.alloc(8)); HIPCHK(dout.alloc(words));
    if (k > 1) {
        hipLaunchKernelGGL(k_batch_seed, dim3(1), dim3(64), 0, ctx->stream, d_seed, k, d_leaf, bseed.p);
        LAUNCH_CHECK();
        d_seed = bseed.p;
    }
    int32_t rc = prove_policy_device(ctx, plan, 1, (int)S, sv, sr, sC, n_bits, d_seed, d_leaf, dout.p, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpy(range_out, dout.p, words * 4, hipMemcpyDeviceToHost));
    return DAPOL_OK;
}

int32_t dapol_prove_batch(dapol_ctx* ctx, dapol_tree* tree, size_t k, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor,
                          int32_t n_bits, const uint8_t nonce_seed32[32], uint8_t* sib_C32, uint8_t* sib_H32, uint8_t* range_out) {
    WIRE_SCOPE();
    if (!ctx || !tree || tree->ctx != ctx || !nonce_seed32 || !leaf_idx || !range_out) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (tree->shard_bits) return fail(DAPOL_ERR_INVALID_ARGUMENT, "batched proofs need the whole tree (not a shard)");
    TREE_USABLE(tree);
    const int H = tree->height;
    std::vector<BatchSib> sibs;
    if (!batch_plan(H, k, leaf_idx, sibs)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "leaf indexes must be non-empty, strictly increasing and below 2^height");
    const size_t S = sibs.size();
    if (S > (size_t)1 << 20) return fail(DAPOL_ERR_INVALID_ARGUMENT, "batch too large");
    std::vector<SubProof> plan;
    size_t words = 0;
    if (int32_t rc = batch_policy_plan(ctx, S, policy, aggregation_factor, n_bits, plan, words)) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t tot = k * (size_t)H, hw = (size_t)ctx_hw(ctx);
    DevBuf<uint64_t> dl, pv, sv;
    DevBuf<uint32_t> dseed, pC, pH, pr, pos, sC, sH, sr, dsrc;
    HIPCHK(dl.alloc(k)); HIPCHK(dseed.alloc(8)); HIPCHK(pos.alloc(k));
    HIPCHK(pC.alloc(tot * 8 + 8)); HIPCHK(pH.alloc(tot * hw + 16)); HIPCHK(pr.alloc(tot * 8 + 8)); HIPCHK(pv.alloc(tot + 1));
    HIPCHK(sC.alloc(S * 8 + 8)); HIPCHK(sH.alloc(S * hw + 16)); HIPCHK(sr.alloc(S * 8 + 8)); HIPCHK(sv.alloc(S + 1)); HIPCHK(dsrc.alloc(S + 1));
    HIPCHK(hipMemcpyAsync(dl.p, leaf_idx, k * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dseed.p, nonce_seed32, 32, hipMemcpyHostToDevice, st));
    PathOut po{pC.p, pH.p, pv.p, pr.p};
    int32_t rc = tree_paths_device(tree, k, dl.p, po, pos.p);
    if (rc) return rc;
    std::vector<uint32_t> src(S);
    for (size_t i = 0; i < S; i++) src[i] = (uint32_t)((size_t)sibs[i].src_leaf * H + (size_t)(g_wire.siblings_leaf_first ? sibs[i].level : H - 1 - sibs[i].level));
    PathOut so{sC.p, sH.p, sv.p, sr.p};
    if (S) {
        HIPCHK(hipMemcpyAsync(dsrc.p, src.data(), S * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_batch_gather, dim3(nblk(S, 256)), dim3(256), 0, st, S, dsrc.p, po, so, (int)hw);
        LAUNCH_CHECK();
    }
    rc = batch_prove_tail(ctx, plan, k, dl.p, S, sv.p, sr.p, sC.p, n_bits, dseed.p, words, range_out);
    if (rc) return rc;
    if (sib_C32 && S) HIPCHK(hipMemcpy(sib_C32, sC.p, S * 32, hipMemcpyDeviceToHost));
    if (sib_H32 && S) HIPCHK(hipMemcpy(sib_H32, sH.p, S * hw * 4, hipMemcpyDeviceToHost));
    return DAPOL_OK;
}

// MerkleProof::verify_batch with DapolProofNode::merge: arena slots [0, k) leaves, [k, k + S) siblings, then the
// merged nodes level by level; `ops` = (left slot, right slot, destination slot).
struct MergeOp { uint32_t left, right, dst; };
// The merge schedule of one batch: walk the levels bottom-up; sibling slots are consumed in plan order within their level.  The
// leaves sit at slots leaf_slot + i, the siblings at sib_slot + i, every merged node takes next_slot++; emit(level, left, right, dst)
// level by level.  Returns the slot of the root.
template <typename Emit>
static uint32_t batch_merge_schedule(int height, size_t k, const uint64_t* leaf_idx, size_t S, const BatchSib* sibs, uint32_t leaf_slot, uint32_t sib_slot,
                                     uint32_t& next_slot, Emit emit) {
    std::vector<size_t> level_first((size_t)height + 1, 0);               // first plan entry of each level
    for (size_t i = S; i-- > 0;) level_first[sibs[i].level] = i;        // (a level's siblings are contiguous in either sibling order)
    std::vector<std::pair<uint64_t, uint32_t>> cur(k), nxt;
    for (size_t i = 0; i < k; i++) cur[i] = {leaf_idx[i], leaf_slot + (uint32_t)i};
    for (int L = 0; L < height; L++) {
        nxt.clear();
        size_t sp = level_first[L];
        for (size_t i = 0; i < cur.size();) {
            uint64_t x = cur[i].first;
            uint32_t left, right;
            if (!(x & 1) && i + 1 < cur.size() && cur[i + 1].first == x + 1) {
                left = cur[i].second; right = cur[i + 1].second;
                i += 2;
            } else {
                uint32_t sib = sib_slot + (uint32_t)sp++;
                if (x & 1) { left = sib; right = cur[i].second; }
                else { left = cur[i].second; right = sib; }
                i += 1;
            }
            emit(L, left, right, next_slot);
            nxt.push_back({x >> 1, next_slot});
            next_slot++;
        }
        cur.swap(nxt);
    }
    return cur[0].second;
}
template <int HW, int DX>
__global__ void k_batch_merge(int dg, size_t n, const MergeOp* ops, uint32_t* C, uint32_t* Hh, uint32_t* bad) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    MergeOp o = ops[i];
    uint32_t cl[8], cr[8], hl[HW], hr[HW], cp[8], hp[HW];
    ld8(cl, C + (size_t)o.left * 8); ld8(cr, C + (size_t)o.right * 8);
    ldh<HW>(hl, Hh + (size_t)o.left * HW); ldh<HW>(hr, Hh + (size_t)o.right * HW);
    ge_p3 a, b, p;
    bool ok = ge_decompress(a, cl) & ge_decompress(b, cr);
    if (!ok) atomicOr(bad, 1u);
    ge_add(p, a, b);
    ge_compress(cp, p);
    node_hash_parent_w<HW, DX>(dg, hp, cl, cr, hl, hr);
    st8(C + (size_t)o.dst * 8, cp);
    sth<HW>(Hh + (size_t)o.dst * HW, hp);
}

int32_t dapol_verify_batch(dapol_ctx* ctx, int32_t height, size_t k, const uint64_t* leaf_idx, const uint8_t* leaf_C32, const uint8_t* leaf_H32,
                           size_t n_siblings, const uint8_t* sib_C32, const uint8_t* sib_H32, const uint8_t root_C32[32],
                           const uint8_t root_H32[32], int32_t policy, int32_t aggregation_factor, int32_t n_bits,
                           const uint8_t* range_proofs, const uint8_t verify_seed32[32], uint8_t* ok) {
    WIRE_SCOPE();
    if (!ctx || !leaf_idx || !leaf_C32 || !leaf_H32 || !root_C32 || !root_H32 || !range_proofs || !ok ||
        (n_siblings && (!sib_C32 || !sib_H32)))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    VERIFY_SEED_OR_OS(verify_seed32)
    if (height < 0 || height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    *ok = 0;
    std::vector<BatchSib> sibs;
    if (!batch_plan(height, k, leaf_idx, sibs)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "leaf indexes must be non-empty, strictly increasing and below 2^height");
    const size_t S = sibs.size();
    if (S != n_siblings) return DAPOL_OK;                                 // wrong number of siblings for these leaves: proof rejected
    std::vector<SubProof> plan;
    size_t words = 0;
    int max_m = 1;
    if (int32_t rc = batch_policy_plan(ctx, S, policy, aggregation_factor, n_bits, plan, words, &max_m)) return rc;
    std::vector<MergeOp> ops;
    std::vector<size_t> level_ops((size_t)height, 0);                     // ops.size() after each level
    uint32_t next_slot = (uint32_t)(k + S);
    batch_merge_schedule(height, k, leaf_idx, S, sibs.data(), 0u, (uint32_t)k, next_slot, [&](int L, uint32_t left, uint32_t right, uint32_t dst) {
        ops.push_back({left, right, dst});
        level_ops[L] = ops.size();
    });
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t slots = next_slot, hw = (size_t)ctx_hw(ctx), hb = hw * 4;
    DevBuf<uint32_t> aC, aH, bad, droot, dseed, dR, dV;
    DevBuf<MergeOp> dops;
    DevBuf<uint8_t> dok, dsub;
    HIPCHK(aC.alloc(slots * 8)); HIPCHK(aH.alloc(slots * hw)); HIPCHK(bad.alloc(1)); HIPCHK(dops.alloc(ops.size() + 1));
    HIPCHK(dseed.alloc(8)); HIPCHK(dR.alloc(words)); HIPCHK(dV.alloc((size_t)max_m * 8)); HIPCHK(dok.alloc(1)); HIPCHK(dsub.alloc(1));
    HIPCHK(hipMemsetAsync(bad.p, 0, 4, st));
    HIPCHK(hipMemcpyAsync(aC.p, leaf_C32, k * 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(aH.p, leaf_H32, k * hb, hipMemcpyHostToDevice, st));
    if (S) {
        HIPCHK(hipMemcpyAsync(aC.p + k * 8, sib_C32, S * 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(aH.p + k * hw, sib_H32, S * hb, hipMemcpyHostToDevice, st));
    }
    if (!ops.empty()) HIPCHK(hipMemcpyAsync(dops.p, ops.data(), ops.size() * sizeof(MergeOp), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dR.p, range_proofs, words * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dseed.p, verify_seed32, 32, hipMemcpyHostToDevice, st));
    size_t done = 0;
    for (size_t lv = 0; lv < level_ops.size(); lv++) {
        size_t n = level_ops[lv] - done;
        if (hw == 16) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_batch_merge<16, DG_RUNTIME>), dim3(nblk(n, 64)), dim3(64), 0, st, ctx->tv.digest, n, dops.p + done, aC.p, aH.p, bad.p);
        else LAUNCH_DX(ctx->tv.digest, (k_batch_merge<8, DX>), dim3(nblk(n, 64)), dim3(64), 0, st, ctx->tv.digest, n, dops.p + done, aC.p, aH.p, bad.p);
        LAUNCH_CHECK();
        done = level_ops[lv];
    }
    uint8_t got[96];
    uint32_t h_bad = 0;
    const size_t root_slot = height ? slots - 1 : 0;
    HIPCHK(hipMemcpyAsync(got, aC.p + root_slot * 8, 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(got + 32, aH.p + root_slot * hw, hb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    bool merkle_ok = !h_bad && memcmp(got, root_C32, 32) == 0 && memcmp(got + 32, root_H32, hb) == 0 && (height > 0 || k == 1);
    uint8_t one = 1;
    HIPCHK(hipMemcpyAsync(dok.p, &one, 1, hipMemcpyHostToDevice, st));
    int32_t rc = verify_policy_device(ctx, plan, 1, (int)S, aC.p + k * 8, dR.p, words, n_bits, dseed.p, dok.p, dsub.p, dV.p);
    if (rc) return rc;
    uint8_t range_ok = 0;
    HIPCHK(hipMemcpy(&range_ok, dok.p, 1, hipMemcpyDeviceToHost));
    *ok = (merkle_ok && range_ok) ? 1 : 0;
    return DAPOL_OK;
}

// ------------------------------------------------------------------------------------ batched proofs on a SHARDED tree
// generate_proof_batch (src/dapol/mod.rs:172-190) when the tree is split over several GPUs: the siblings of a batch lie in
// different shards (and in the replicated top levels), so the proof is assembled from RECORDS instead of from one resident
// tree:  dapol_batch_siblings gives the positions;  every rank reads the records of the positions inside its subtree
// (dapol_tree_node_records);  the positions above the shard roots come from the exchanged subtree-root records
// (dapol_shard_top_node_records);  the ranks exchange their records (any transport: they are 104-byte rows);  then
// dapol_prove_batch_records runs R::generate_proof over the assembled siblings -- the bytes equal dapol_prove_batch's on
// the unsharded tree (tests/test_gpu_parity.py::test_batch_proof_on_a_sharded_tree).

// One lane per requested node: (level above the leaves, index within the level) -> the real node or the padding node stored
// there; found = 0 when the tree holds neither.
__global__ void k_tree_node_records(size_t n, const uint8_t* level, const uint64_t* index, const LevelView* views, int height, uint32_t* C,
                                    uint32_t* H, uint64_t* v, uint32_t* r, uint8_t* found) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    found[t] = 0;
    const int L = level[t];
    if (L > height) return;
    const LevelView& lv = views[L];
    const uint64_t want = index[t];
    auto find = [&](uint64_t x, size_t& pos) {
        size_t lo = 0, hi = lv.n;
        while (lo < hi) {
            size_t mid = (lo + hi) >> 1;
            if (lv.idx[mid] < x) lo = mid + 1; else hi = mid;
        }
        pos = lo;
        return lo < lv.n && lv.idx[lo] == x;
    };
    size_t p;
    uint32_t w[8];
    if (find(want, p)) {
        ld8(w, lv.C + p * 8); st8(C + t * 8, w);
        ld8(w, lv.H + p * 8); st8(H + t * 8, w);
        ld8(w, lv.r + p * 8); st8(r + t * 8, w);
        v[t] = lv.v[p];
        found[t] = 1;
    } else if (L < height && find(want ^ 1ull, p) && lv.has_pad[p]) {      // the padding sibling of the real node at `p`
        ld8(w, lv.padC + p * 8); st8(C + t * 8, w);
        ld8(w, lv.padH + p * 8); st8(H + t * 8, w);
        ld8(w, lv.padr + p * 8); st8(r + t * 8, w);
        v[t] = 0;
        found[t] = 1;
    }
}

int32_t dapol_tree_node_records(dapol_tree* tree, size_t n, const uint8_t* level, const uint64_t* index, uint8_t* C32, uint8_t* H32, uint64_t* v,
                                uint8_t* r32, uint8_t* found) {
    if (!tree || (n && (!level || !index || !C32 || !H32 || !v || !r32 || !found))) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    TREE_USABLE(tree);
    NEEDS_32_BYTE_DIGEST(tree->ctx, "the sharded (multi-GPU) record path");
    if (n == 0) return DAPOL_OK;
    dapol_ctx* ctx = tree->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<uint8_t> dl, df;
    DevBuf<uint64_t> di, dv;
    DevBuf<uint32_t> dC, dH, dr;
    HIPCHK(dl.alloc(n)); HIPCHK(df.alloc(n)); HIPCHK(di.alloc(n)); HIPCHK(dv.alloc(n));
    HIPCHK(dC.alloc(n * 8)); HIPCHK(dH.alloc(n * 8)); HIPCHK(dr.alloc(n * 8));
    HIPCHK(hipMemcpyAsync(dl.p, level, n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(di.p, index, n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(dC.p, 0, n * 32, st)); HIPCHK(hipMemsetAsync(dH.p, 0, n * 32, st)); HIPCHK(hipMemsetAsync(dr.p, 0, n * 32, st));
    HIPCHK(hipMemsetAsync(dv.p, 0, n * 8, st));
    hipLaunchKernelGGL(k_tree_node_records, dim3(nblk(n, 256)), dim3(256), 0, st, n, dl.p, di.p, tree->d_views.p, tree->height, dC.p, dH.p, dv.p, dr.p, df.p);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(C32, dC.p, n * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(H32, dH.p, n * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(r32, dr.p, n * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(v, dv.p, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(found, df.p, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DAPOL_OK;
}

int32_t dapol_prove_batch_records(dapol_ctx* ctx, size_t k, const uint64_t* leaf_idx, size_t n_siblings, const uint8_t* sib_C32, const uint64_t* sib_v,
                                  const uint8_t* sib_r32, int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t nonce_seed32[32],
                                  uint8_t* range_out) {
    WIRE_SCOPE();
    if (!ctx || !nonce_seed32 || !leaf_idx || !range_out || k == 0 || (n_siblings && (!sib_C32 || !sib_v || !sib_r32)))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    const size_t S = n_siblings;
    if (S > (size_t)1 << 20) return fail(DAPOL_ERR_INVALID_ARGUMENT, "batch too large");
    std::vector<SubProof> plan;
    size_t words = 0;
    if (int32_t rc = batch_policy_plan(ctx, S, policy, aggregation_factor, n_bits, plan, words)) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<uint64_t> dl, sv;
    DevBuf<uint32_t> dseed, sC, sr;
    HIPCHK(dl.alloc(k)); HIPCHK(dseed.alloc(8)); HIPCHK(sC.alloc(S * 8 + 8)); HIPCHK(sr.alloc(S * 8 + 8)); HIPCHK(sv.alloc(S + 1));
    HIPCHK(hipMemcpyAsync(dl.p, leaf_idx, k * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dseed.p, nonce_seed32, 32, hipMemcpyHostToDevice, st));
    if (S) {
        HIPCHK(hipMemcpyAsync(sC.p, sib_C32, S * 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(sr.p, sib_r32, S * 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(sv.p, sib_v, S * 8, hipMemcpyHostToDevice, st));
    }
    return batch_prove_tail(ctx, plan, k, dl.p, S, sv.p, sr.p, sC.p, n_bits, dseed.p, words, range_out);
}

// Length-checked forms of the two verifier entry points, for callers whose buffers come from UNTRUSTED bytes (a decoded wire):
// the counts the caller actually holds are passed in and compared with what (height, policy, aggregation_factor, n_bits) imply
// before anything is read.  A proof of the wrong shape is an invalid proof -- ok[] = 0, DAPOL_OK -- not an error and never an
// over-read.  include/dapol.hpp and the Python binding call these.
int32_t dapol_verify_entities_checked(dapol_ctx* ctx, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* leaf_C32, const uint8_t* leaf_H32,
                                      size_t n_path_nodes, const uint8_t* path_C32, const uint8_t* path_H32, const uint8_t root_C32[32],
                                      const uint8_t root_H32[32], int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t* range_proofs,
                                      size_t range_proofs_len, const uint8_t verify_seed32[32], uint8_t* ok) {
    if (b && !ok) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (height < 0 || height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    const size_t es = dapol_entity_proof_size(height, policy, aggregation_factor, n_bits);
    if (es == 0 || n_path_nodes != b * (size_t)height || range_proofs_len != b * es) {
        for (size_t i = 0; i < b; i++) ok[i] = 0;
        return DAPOL_OK;
    }
    return dapol_verify_entities(ctx, height, b, leaf_idx, leaf_C32, leaf_H32, path_C32, path_H32, root_C32, root_H32, policy, aggregation_factor, n_bits,
                                 range_proofs, verify_seed32, ok);
}
int32_t dapol_verify_batch_checked(dapol_ctx* ctx, int32_t height, size_t k, const uint64_t* leaf_idx, const uint8_t* leaf_C32, const uint8_t* leaf_H32,
                                   size_t n_siblings, const uint8_t* sib_C32, const uint8_t* sib_H32, const uint8_t root_C32[32], const uint8_t root_H32[32],
                                   int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t* range_proofs, size_t range_proofs_len,
                                   const uint8_t verify_seed32[32], uint8_t* ok) {
    if (!ok) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    *ok = 0;
    if (n_siblings > 0x7fffffffu) return DAPOL_OK;
    const size_t es = dapol_entity_proof_size((int32_t)n_siblings, policy, aggregation_factor, n_bits);
    if (es == 0 || range_proofs_len != es) return DAPOL_OK;
    return dapol_verify_batch(ctx, height, k, leaf_idx, leaf_C32, leaf_H32, n_siblings, sib_C32, sib_H32, root_C32, root_H32, policy, aggregation_factor,
                              n_bits, range_proofs, verify_seed32, ok);
}

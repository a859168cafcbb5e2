// Host orchestration of the on-device leaf derivation (kernels_leaf.h).

static int32_t sort_pairs_u64_u32(hipStream_t st, uint64_t* kin, uint64_t* kout, uint32_t* vin, uint32_t* vout, size_t n) {
    size_t tmp = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp, kin, kout, vin, vout, n, 0, 64, st));
    DevBuf<uint8_t> d;
    HIPCHK(d.alloc(tmp ? tmp : 1));
    HIPCHK(rocprim::radix_sort_pairs(d.p, tmp, kin, kout, vin, vout, n, 0, 64, st));
    HIPCHK(hipStreamSynchronize(st));
    return DAPOL_OK;
}

__global__ void k_iota(size_t n, uint32_t* o) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = (uint32_t)i;
}
__global__ void k_leaf_gather(size_t n, const uint32_t* ord, const uint64_t* values, const uint32_t* blind, uint64_t* v_sorted, uint32_t* r_sorted) {
    size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint32_t e = ord[p];
    v_sorted[p] = values[e];
    for (int i = 0; i < 8; i++) r_sorted[p * 8 + i] = blind[(size_t)e * 8 + i];
}

// Launches of the leaf kernels that hash: the instantiation over the streaming state of digest `kind`.
#define LAUNCH_LEAF(kind, K, ...)                                                        \
    do {                                                                                 \
        switch (kind) {                                                                  \
            case DG_SHA256: hipLaunchKernelGGL(K<Sha256Stream>, __VA_ARGS__); break;     \
            case DG_SHA3_256: hipLaunchKernelGGL(K<Sha3Stream>, __VA_ARGS__); break;     \
            default: hipLaunchKernelGGL(K<Digest>, __VA_ARGS__);                         \
        }                                                                                \
    } while (0)

// build_leaf_nodes over n liabilities that join the leaves O (none for dapol_build_leaf_nodes): a candidate that is one of O is taken
// before the batch starts (kernels_leaf.h, LeafOccupied); the sparsity rule of Dapol::new counts O's leaves too.
static int32_t leaf_derive(dapol_ctx* ctx, int32_t digest_id, const uint8_t* audit_seed, size_t audit_seed_len, int32_t height, size_t n,
                           const uint8_t* internal_ids, const uint32_t* internal_off, const uint8_t* external_ids, const uint32_t* external_off,
                           const uint64_t* values, uint64_t* leaf_idx_sorted, uint64_t* v_sorted, uint8_t* r32_sorted, uint32_t* order_sorted,
                           uint64_t* idx_by_entity, LeafOccupied O) {
    if (!ctx || !n || !internal_off || !external_off || !values || !leaf_idx_sorted || !v_sorted || !r32_sorted || !order_sorted ||
        (audit_seed_len && !audit_seed))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (digest_id != DAPOL_DIGEST_BLAKE3 && digest_id != DAPOL_DIGEST_BLAKE2S && digest_id != DAPOL_DIGEST_SHA256 && digest_id != DAPOL_DIGEST_SHA3_256)
        return fail(DAPOL_ERR_INVALID_DIGEST_SIZE, "digest must be BLAKE3, Blake2s-256, SHA-256 or SHA3-256 (32 bytes)");
    if (height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    if (height < 1) return fail(DAPOL_ERR_INVALID_ARGUMENT, "tree height must be at least 1");
    if (height < 64 && (double)(n + O.n) * 2.0 > (double)(1ull << height)) return fail(DAPOL_ERR_SPARSITY_TOO_SMALL, "2^height < 2 * number of liabilities");
    if (n > ((size_t)1 << 31) || audit_seed_len > 512) return fail(DAPOL_ERR_INVALID_ARGUMENT, "at most 2^31 liabilities; audit seed at most 512 bytes");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t ib = internal_off[n], eb = external_off[n];
    DevBuf<uint8_t> dseed, diid, deid, evicted, tab_used;
    DevBuf<uint32_t> dioff, deoff, aid, state, blind, err, ord, ord2, losers, nl, heap;
    DevBuf<uint64_t> cand, key, key2, dvals, tab_key, vs;
    DevBuf<uint32_t> rs;
    HIPCHK(dseed.alloc(audit_seed_len + 1)); HIPCHK(diid.alloc(ib + 1)); HIPCHK(deid.alloc(eb + 1));
    HIPCHK(dioff.alloc(n + 1)); HIPCHK(deoff.alloc(n + 1));
    HIPCHK(aid.alloc(n * 8)); HIPCHK(state.alloc(n * 8)); HIPCHK(blind.alloc(n * 8)); HIPCHK(err.alloc(4));
    HIPCHK(cand.alloc(n)); HIPCHK(key.alloc(n)); HIPCHK(key2.alloc(n)); HIPCHK(ord.alloc(n)); HIPCHK(ord2.alloc(n)); HIPCHK(dvals.alloc(n));
    HIPCHK(vs.alloc(n)); HIPCHK(rs.alloc(n * 8));
    if (audit_seed_len) HIPCHK(hipMemcpyAsync(dseed.p, audit_seed, audit_seed_len, hipMemcpyHostToDevice, st));
    if (ib) HIPCHK(hipMemcpyAsync(diid.p, internal_ids, ib, hipMemcpyHostToDevice, st));
    if (eb) HIPCHK(hipMemcpyAsync(deid.p, external_ids, eb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dioff.p, internal_off, (n + 1) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(deoff.p, external_off, (n + 1) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dvals.p, values, n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(err.p, 0, 16, st));
    LeafArgs A{};
    A.n = n; A.height = height; A.kind = digest_id;   // (the DAPOL_DIGEST_* ids are the DG_* kinds)
    A.seed = dseed.p; A.seed_len = (uint32_t)audit_seed_len;
    A.iid = diid.p; A.iid_off = dioff.p; A.eid = deid.p; A.eid_off = deoff.p;
    A.audit_id = aid.p; A.idx_state = state.p; A.cand = cand.p; A.blind = blind.p; A.err = err.p;
    A.max_tries = LEAF_MAX_RETRIES;
    if (const char* e = test_knob("DAPOL_LEAF_MAX_TRIES")) A.max_tries = std::min((int)LEAF_MAX_RETRIES, std::max(1, atoi(e)));   // test knob (DAPOL_TEST_HOOKS=1 beside DAPOL_ENV_KNOBS)
    LAUNCH_LEAF(A.kind, k_leaf_hash, dim3(nblk(n, 64)), dim3(64), 0, st, A); LAUNCH_CHECK();
    // duplicate internal ids
    hipLaunchKernelGGL(k_leaf_dup_keys, dim3(nblk(n, 256)), dim3(256), 0, st, n, aid.p, key.p, ord.p); LAUNCH_CHECK();
    int32_t rc = sort_pairs_u64_u32(st, key.p, key2.p, ord.p, ord2.p, n);
    if (rc) return rc;
    hipLaunchKernelGGL(k_leaf_dup_check, dim3(nblk(n, 256)), dim3(256), 0, st, A, key2.p, ord2.p); LAUNCH_CHECK();
    uint32_t herr[4];
    HIPCHK(hipMemcpyAsync(herr, err.p, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (herr[0]) return fail(DAPOL_ERR_INVALID_ARGUMENT, "a hash input is too long for the BLAKE3 chunk stack (16 GiB)");
    if (herr[1]) return fail(DAPOL_ERR_DUPLICATED_INTERNAL_ID, "liability set contains a duplicated internal ID");
    // Collisions, in the reference's order (kernels_leaf.h): claim / settle rounds over a slot table until nobody moves.
    bool resolved = false;
    if (height < 64 && !knob("DAPOL_LEAF_SERIAL")) {
        size_t tsz = 1;
        while (tsz < 4 * n + 64) tsz <<= 1;
        DevBuf<unsigned long long> tkey;
        DevBuf<uint32_t> towner, tpos, ttries, tflags;
        HIPCHK(tkey.alloc(tsz)); HIPCHK(towner.alloc(tsz)); HIPCHK(tpos.alloc(n)); HIPCHK(ttries.alloc(n)); HIPCHK(tflags.alloc(2));
        HIPCHK(hipMemsetAsync(tkey.p, 0xff, tsz * 8, st));
        HIPCHK(hipMemsetAsync(towner.p, 0xff, tsz * 4, st));
        HIPCHK(hipMemsetAsync(tflags.p, 0, 8, st));
        HIPCHK(hipMemsetAsync(err.p + 3, 0xff, 4, st));                        // (atomicMin target: the earliest entity that cannot be mapped)
        LeafTable T{tkey.p, towner.p, (uint32_t)(tsz - 1), tpos.p, ttries.p, tflags.p};
        if (O.n) hipLaunchKernelGGL(k_leaf_claim_first_onto, dim3(nblk(n, 256)), dim3(256), 0, st, A, T, O);
        else hipLaunchKernelGGL(k_leaf_claim_first, dim3(nblk(n, 256)), dim3(256), 0, st, A, T);
        LAUNCH_CHECK();
        uint32_t hflags[2] = {1, 0};
        for (int round = 0; round < 100000 && hflags[0] && !hflags[1]; round++) {
            HIPCHK(hipMemsetAsync(tflags.p, 0, 4, st));
            if (O.n) LAUNCH_LEAF(A.kind, k_leaf_settle_onto, dim3(nblk(n, 256)), dim3(256), 0, st, A, T, O);
            else LAUNCH_LEAF(A.kind, k_leaf_settle, dim3(nblk(n, 256)), dim3(256), 0, st, A, T);
            LAUNCH_CHECK();
            HIPCHK(hipMemcpyAsync(hflags, tflags.p, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        resolved = !hflags[0] && !hflags[1];
        if (resolved) {
            HIPCHK(hipMemcpyAsync(herr, err.p, 16, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (herr[2]) {
                char msg[160];
                snprintf(msg, sizeof msg, "failed to map an audit ID to a tree index within %d tries (liability %u in input order)", A.max_tries, herr[3]);
                return fail(DAPOL_ERR_FAILED_TO_MAP_INDEX, msg);
            }
        }
        if (!resolved) {                                                        // table full (cannot happen at 4 n slots in practice): start over, one lane
            LAUNCH_LEAF(A.kind, k_leaf_hash, dim3(nblk(n, 64)), dim3(64), 0, st, A); LAUNCH_CHECK();
            HIPCHK(hipMemsetAsync(err.p, 0, 16, st));
        }
    }
    hipLaunchKernelGGL(k_iota, dim3(nblk(n, 256)), dim3(256), 0, st, n, ord.p); LAUNCH_CHECK();
    rc = sort_pairs_u64_u32(st, cand.p, key2.p, ord.p, ord2.p, n);             // (indexes, input order); unique indexes once resolved
    if (rc) return rc;
    if (!resolved) {
    // the one-lane path: first candidates sorted by (index, input order) -- radix sort is stable -- then the losers in input order
    HIPCHK(losers.alloc(n)); HIPCHK(nl.alloc(1));
    HIPCHK(hipMemsetAsync(nl.p, 0, 4, st));
    if (O.n) hipLaunchKernelGGL(k_leaf_mark_onto, dim3(nblk(n, 256)), dim3(256), 0, st, n, key2.p, ord2.p, losers.p, nl.p, O);
    else hipLaunchKernelGGL(k_leaf_mark, dim3(nblk(n, 256)), dim3(256), 0, st, n, key2.p, ord2.p, losers.p, nl.p);
    LAUNCH_CHECK();
    uint32_t n_losers = 0;
    HIPCHK(hipMemcpyAsync(&n_losers, nl.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_losers) {
        size_t tsz = 1;
        while (tsz < 2 * n + 16) tsz <<= 1;
        HIPCHK(evicted.alloc(n)); HIPCHK(tab_used.alloc(tsz)); HIPCHK(tab_key.alloc(tsz));
        HIPCHK(hipMemsetAsync(evicted.p, 0, n, st));
        HIPCHK(hipMemsetAsync(tab_used.p, 0, tsz, st));
        LeafResolve R{};
        R.n = n; R.skey = key2.p; R.sord = ord2.p; R.heap = losers.p; R.heap_n = n_losers; R.evicted = evicted.p;
        R.tab_key = tab_key.p; R.tab_used = tab_used.p; R.tab_mask = (uint32_t)(tsz - 1);
        R.occ = O;
        LAUNCH_LEAF(A.kind, k_leaf_resolve, dim3(1), dim3(64), 0, st, A, R); LAUNCH_CHECK();
        HIPCHK(hipMemcpyAsync(herr, err.p, 16, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (herr[2]) {
            char msg[160];
            snprintf(msg, sizeof msg, "failed to map an audit ID to a tree index within %d tries (liability %u in input order)", A.max_tries, herr[3]);
            return fail(DAPOL_ERR_FAILED_TO_MAP_INDEX, msg);
        }
        hipLaunchKernelGGL(k_iota, dim3(nblk(n, 256)), dim3(256), 0, st, n, ord.p); LAUNCH_CHECK();
        rc = sort_pairs_u64_u32(st, cand.p, key2.p, ord.p, ord2.p, n);     // final indexes are unique now
        if (rc) return rc;
    }
    }
    hipLaunchKernelGGL(k_leaf_gather, dim3(nblk(n, 256)), dim3(256), 0, st, n, ord2.p, dvals.p, blind.p, vs.p, rs.p); LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(leaf_idx_sorted, key2.p, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(v_sorted, vs.p, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(r32_sorted, rs.p, n * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(order_sorted, ord2.p, n * 4, hipMemcpyDeviceToHost, st));
    if (idx_by_entity) HIPCHK(hipMemcpyAsync(idx_by_entity, cand.p, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DAPOL_OK;
}

int32_t dapol_build_leaf_nodes(dapol_ctx* ctx, int32_t digest_id, const uint8_t* audit_seed, size_t audit_seed_len, int32_t height, size_t n,
                               const uint8_t* internal_ids, const uint32_t* internal_off, const uint8_t* external_ids,
                               const uint32_t* external_off, const uint64_t* values, uint64_t* leaf_idx_sorted, uint64_t* v_sorted,
                               uint8_t* r32_sorted, uint32_t* order_sorted, uint64_t* idx_by_entity) {
    return leaf_derive(ctx, digest_id, audit_seed, audit_seed_len, height, n, internal_ids, internal_off, external_ids, external_off, values,
                       leaf_idx_sorted, v_sorted, r32_sorted, order_sorted, idx_by_entity, LeafOccupied{nullptr, 0});
}

// What both id-based inserts refuse about the tree before anything else: the occupied set is the tree's own level-0 index array, so
// the tree must hold ALL the leaves its liabilities compete with.
static int32_t leaf_join_begin(dapol_tree* tree) {
    TREE_USABLE(tree);
    if (tree->shard_bits)
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "a shard tree holds only its shard's leaves, not the whole set of taken indexes: derive the leaves against the whole tree");
    return DAPOL_OK;
}
int32_t dapol_tree_derive_leaves(dapol_tree* tree, int32_t digest_id, const uint8_t* audit_seed, size_t audit_seed_len, size_t k,
                                 const uint8_t* internal_ids, const uint32_t* internal_off, const uint8_t* external_ids,
                                 const uint32_t* external_off, const uint64_t* values, uint64_t* leaf_idx_sorted, uint64_t* v_sorted,
                                 uint8_t* r32_sorted, uint32_t* order_sorted, uint64_t* idx_by_entity) {
    if (!tree || (audit_seed_len && !audit_seed) ||
        (k && (!internal_off || !external_off || !values || !leaf_idx_sorted || !v_sorted || !r32_sorted || !order_sorted)))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (k == 0) return DAPOL_OK;
    int32_t rc = leaf_join_begin(tree);
    if (rc) return rc;
    return leaf_derive(tree->ctx, digest_id, audit_seed, audit_seed_len, tree->index_bits, k, internal_ids, internal_off, external_ids, external_off, values,
                       leaf_idx_sorted, v_sorted, r32_sorted, order_sorted, idx_by_entity, LeafOccupied{tree->leaf_idx, tree->levels[0].n});
}
int32_t dapol_tree_insert_liabilities(dapol_tree* tree, int32_t digest_id, const uint8_t* audit_seed, size_t audit_seed_len, size_t k,
                                      const uint8_t* internal_ids, const uint32_t* internal_off, const uint8_t* external_ids,
                                      const uint32_t* external_off, const uint64_t* values, uint64_t* idx_by_entity) {
    if (!tree || (audit_seed_len && !audit_seed) || (k && (!internal_off || !external_off || !values))) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (k == 0) return DAPOL_OK;
    int32_t rc = leaf_join_begin(tree);
    if (rc) return rc;
    dapol_tree_owned* own = nullptr;
    rc = tree_edit_begin(tree, "an insert", &own);
    if (rc) return rc;
    if (k > ((size_t)1 << 31)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "at most 2^31 liabilities; audit seed at most 512 bytes");
    // the derived batch, k x 48 bytes, comes to the host and goes into the insert as any caller's would
    std::vector<uint64_t> idx(k), v(k), by_entity(k);
    std::vector<uint8_t> r(k * 32);
    std::vector<uint32_t> order(k);
    rc = leaf_derive(tree->ctx, digest_id, audit_seed, audit_seed_len, tree->index_bits, k, internal_ids, internal_off, external_ids, external_off, values,
                     idx.data(), v.data(), r.data(), order.data(), by_entity.data(), LeafOccupied{tree->leaf_idx, tree->levels[0].n});
    if (rc) return rc;
    rc = tree_edit_end(tree, tree_insert_impl(own, k, idx.data(), v.data(), r.data()));
    if (rc == DAPOL_OK && idx_by_entity) memcpy(idx_by_entity, by_entity.data(), k * 8);
    return rc;
}

// dapol_batch_store_*: the proofs dapol_prove_batches issues for one batch list under one (context, tree, policy, aggregation factor,
// n_bits, nonce seed), kept in HBM between calls and re-proved in place after an edit of the tree (definitions: include/dapol_hip.h;
// index arithmetic: batch_store_plan.inc; kernels: kernels_batch_store.h).  The batch counterpart of host_store.inc.
// dapol_reprove_batches uploads the caller's old siblings and blobs and downloads all of the new ones on every call; here the old data is
// where the last refresh left it, a refresh hands the re-prover's device side (reprove_batches_device) the store's own buffers and plan
// tables, and only the rows a caller asks for cross the bus.  The reference has nothing like it.
// Included from dapol_hip.hip after host_reprove_batches.inc.

struct dapol_batch_store {
    dapol_ctx* ctx = nullptr;              // retained
    dapol_tree* tree = nullptr;            // counted (dapol_tree::stores): the tree outlives the store
    int policy = 0, agg = 0, n_bits = 0, leaf_first = 0;      // leaf_first: dapol_wire_config.siblings_leaf_first at creation
    DevBuf<uint32_t> seed;                 // the nonce seed, 8 words
    std::vector<uint64_t> batch_off{0}, leaf_idx;             // the list of the last successful refresh (host copy): rows = batch_off.size() - 1
    ReproveBatchesList L;                  // its counts and offsets on the host, its leaf lists and plan tables on the device
    struct Siblings { DevBuf<uint32_t> C, H; } set[2];        // [T + 1][8] commitments and hashes at L.sib_off: set[cur] holds the rows' siblings,
    int cur = 0;                           // the other one is the spare a refresh gathers into (empty until it has the right size)
    DevBuf<uint32_t> range;                // the blobs at L.range_off, [R + 4] words
    bool invalid = false;                  // a refresh failed after its first write into the store: siblings and blobs may disagree
    size_t rows() const { return batch_off.size() - 1; }
};

// What every call refuses: no store, an invalid tree, a store left inconsistent, a sibling order other than the recorded one.
static int32_t batch_store_usable(const dapol_batch_store* s) {
    if (!s) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null batch store");
    TREE_USABLE(s->tree);
    if (s->invalid)
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "the batch store was left inconsistent by a refresh that failed midway: destroy it and create it again");
    if ((g_wire.siblings_leaf_first != 0) != (s->leaf_first != 0))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "dapol_wire_config.siblings_leaf_first differs from the order the batch store was created under");
    return DAPOL_OK;
}

int32_t dapol_batch_store_create(dapol_ctx* ctx, dapol_tree* tree, int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t nonce_seed32[32],
                                 dapol_batch_store** out) {
    WIRE_SCOPE();
    // dapol_reprove_batches' refusals for these arguments, in its order (what depends on a batch is refused by the refresh that brings it)
    if (!ctx || !tree || tree->ctx != ctx || !nonce_seed32 || !out) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (tree->shard_bits) return fail(DAPOL_ERR_INVALID_ARGUMENT, "batched proofs need the whole tree (not a shard)");
    TREE_USABLE(tree);
    NEEDS_32_BYTE_DIGEST(ctx, "dapol_batch_store_create");
    HIPCHK(hipSetDevice(ctx->device));
    dapol_batch_store* s = new dapol_batch_store();
    struct Guard { dapol_batch_store* s; ~Guard() { delete s; } } guard{s};
    HIPCHK(s->seed.alloc(8));
    HIPCHK(hipMemcpy(s->seed.p, nonce_seed32, 32, hipMemcpyHostToDevice));
    s->ctx = ctx; s->tree = tree;
    s->policy = policy; s->agg = aggregation_factor; s->n_bits = n_bits;
    s->leaf_first = g_wire.siblings_leaf_first != 0 ? 1 : 0;
    s->L.H = tree->height;
    s->L.sib_off.assign(1, 0); s->L.range_off.assign(1, 0);
    ctx_retain(ctx);
    tree->stores.n++;
    guard.s = nullptr;
    *out = s;
    return DAPOL_OK;
}

int32_t dapol_batch_store_destroy(dapol_batch_store* s) {
    if (!s) return DAPOL_OK;
    dapol_ctx* ctx = s->ctx;
    (void)hipSetDevice(ctx->device);
    if (s->seed.p) (void)hipMemset(s->seed.p, 0, 32);          // the seed does not outlive the store in freed memory
    s->tree->stores.n--;
    delete s;
    (void)dapol_ctx_destroy(ctx);
    return DAPOL_OK;
}

size_t dapol_batch_store_rows(dapol_batch_store* s) {
    if (!s) { (void)fail(DAPOL_ERR_INVALID_ARGUMENT, "null batch store"); return 0; }
    return s->rows();
}

int32_t dapol_batch_store_layout(dapol_batch_store* s, uint64_t* batch_off, uint64_t* leaf_idx, uint64_t* sib_off, uint64_t* range_off) {
    WIRE_SCOPE();
    RCCHK(batch_store_usable(s));
    const size_t nb = s->rows();
    if (batch_off) memcpy(batch_off, s->batch_off.data(), (nb + 1) * 8);
    if (leaf_idx && !s->leaf_idx.empty()) memcpy(leaf_idx, s->leaf_idx.data(), s->leaf_idx.size() * 8);
    if (sib_off) memcpy(sib_off, s->L.sib_off.data(), (nb + 1) * 8);
    if (range_off) memcpy(range_off, s->L.range_off.data(), (nb + 1) * 8);
    return DAPOL_OK;
}

int32_t dapol_batch_store_refresh(dapol_batch_store* s, size_t nb_in, const uint64_t* batch_off, const uint64_t* leaf_idx, uint64_t* proved_out, uint64_t* kept_out,
                                  uint64_t* n_calls_out, uint64_t* moved_rows_out) {
    WIRE_SCOPE();
    RCCHK(batch_store_usable(s));
    if (!batch_off && nb_in) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    dapol_ctx* ctx = s->ctx;
    dapol_tree* tree = s->tree;
    const int H = tree->height;
    const size_t nb = batch_off ? nb_in : s->rows();
    const uint64_t* off = batch_off ? batch_off : s->batch_off.data();
    const uint64_t* leaf = batch_off ? leaf_idx : s->leaf_idx.data();
    // dapol_prove_batches' refusals for the list, before anything else (the stored list passed them when it came: same arguments)
    BatchesPlan P;
    if (batch_off) RCCHK(batches_plan_host(H, nb, off, leaf, s->policy, s->agg, s->n_bits, ctx->max_parties, true, P));
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    uint64_t proved = 0, calls = 0, moved = 0, pairs = 0;
    const bool in_place = !batch_off || batch_store_same_list(s->rows(), s->batch_off.data(), s->leaf_idx.data(), nb, off, leaf);
    if (nb == 0) {
        if (!in_place) {                                       // an empty list empties the store
            s->batch_off.assign(1, 0); s->leaf_idx.clear();
            s->L = ReproveBatchesList{};
            s->L.H = H; s->L.sib_off.assign(1, 0); s->L.range_off.assign(1, 0);
            s->range.release();
            for (auto& x : s->set) { x.C.release(); x.H.release(); }
            s->cur = 0;
        }
    } else if (in_place) {
        // ---- the same list: the blobs stay where they are, the old commitments are the set in use, the plan tables are on the device
        // already; the new siblings go into the spare set, only dirty pieces are written, the sets swap.  reprove_batches_device makes
        // its one write into the blobs after everything it can refuse or fail to allocate.
        const size_t T = s->L.T;
        dapol_batch_store::Siblings& spare = s->set[s->cur ^ 1];
        const bool spare_fits = spare.C.n == T * 8 + 8 && spare.H.n == T * 8 + 8;
        DevBuf<uint32_t> freshC, freshH;
        if (!spare_fits) { HIPCHK(freshC.alloc(T * 8 + 8)); HIPCHK(freshH.alloc(T * 8 + 8)); }
        bool wrote = false;
        const int32_t rc = reprove_batches_device(ctx, tree, s->L, s->n_bits, s->seed.p, nullptr, s->set[s->cur].C.p, s->range.p, spare_fits ? spare.C.p : freshC.p,
                                                  spare_fits ? spare.H.p : freshH.p, &proved, &calls, &wrote);
        if (rc) { if (wrote) s->invalid = true; return rc; }
        if (!spare_fits) { spare.C = std::move(freshC); spare.H = std::move(freshH); }
        s->cur ^= 1;
        pairs = s->L.n;
    } else {
        // ---- another list: everything is written into new buffers at the new offsets, and the store takes them over only when all of it
        // has succeeded.  Batches that continue an old row bring its blob and its commitments (to compare against) along.
        std::vector<uint32_t> src(nb);
        std::vector<uint8_t> has(nb);
        moved = batch_store_match(s->rows(), s->batch_off.data(), s->leaf_idx.data(), nb, off, leaf, src.data(), has.data());
        ReproveBatchesList NL;
        DevBuf<uint32_t> nrange, cmpC, freshC, freshH, dsrc;
        DevBuf<uint8_t> dhas;
        StreamDrain drain{st};
        RCCHK(reprove_batches_list_build(ctx, H, P, nb, off, leaf, s->n_bits, NL));
        const size_t T = NL.T, R = NL.R;
        HIPCHK(nrange.alloc(R + 4)); HIPCHK(freshC.alloc(T * 8 + 8)); HIPCHK(freshH.alloc(T * 8 + 8)); HIPCHK(dsrc.alloc(nb)); HIPCHK(dhas.alloc(nb));
        if (moved) HIPCHK(cmpC.alloc(T * 8 + 8));
        HIPCHK(hipMemcpyAsync(dsrc.p, src.data(), nb * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dhas.p, has.data(), nb, hipMemcpyHostToDevice, st));
        if (moved && R / 4 + 2 * T) {
            hipLaunchKernelGGL(k_batch_store_move, dim3(nblk(R / 4 + 2 * T, 256)), dim3(256), 0, st, nb, R / 4, 2 * T, dsrc.p, NL.piece_off.p, s->L.piece_off.p,
                               NL.d_sib_off.p, s->L.d_sib_off.p, (const uint4*)s->range.p, (const uint4*)s->set[s->cur].C.p, (uint4*)nrange.p, (uint4*)cmpC.p);
            LAUNCH_CHECK();
        }
        RCCHK(reprove_batches_device(ctx, tree, NL, s->n_bits, s->seed.p, dhas.p, cmpC.p, nrange.p, freshC.p, freshH.p, &proved, &calls, nullptr));
        pairs = NL.n;
        s->batch_off.assign(off, off + nb + 1);
        s->leaf_idx.assign(leaf, leaf + (size_t)off[nb]);
        s->L = std::move(NL);
        s->range = std::move(nrange);                          // (the old buffers are freed here, after the copy has drained)
        s->set[0].C = std::move(freshC); s->set[0].H = std::move(freshH);
        s->set[1].C.release(); s->set[1].H.release();          // of another size now: the next refresh allocates its spare
        s->cur = 0;
    }
    if (proved_out) *proved_out = proved;
    if (kept_out) *kept_out = pairs - proved;
    if (n_calls_out) *n_calls_out = calls;
    if (moved_rows_out) *moved_rows_out = moved;
    return DAPOL_OK;
}

int32_t dapol_batch_store_read(dapol_batch_store* s, size_t first, size_t count, uint8_t* sib_C32, uint8_t* sib_H32, uint8_t* range_out) {
    WIRE_SCOPE();
    RCCHK(batch_store_usable(s));
    if (first > s->rows() || count > s->rows() - first) return fail(DAPOL_ERR_INVALID_ARGUMENT, "first + count exceeds the rows of the batch store");
    if (count == 0) return DAPOL_OK;
    HIPCHK(hipSetDevice(s->ctx->device));
    const size_t s0 = (size_t)s->L.sib_off[first], S = (size_t)s->L.sib_off[first + count] - s0;
    const size_t r0 = (size_t)s->L.range_off[first], B = (size_t)s->L.range_off[first + count] - r0;
    const dapol_batch_store::Siblings& cur = s->set[s->cur];
    if (sib_C32 && S) HIPCHK(hipMemcpy(sib_C32, cur.C.p + s0 * 8, S * 32, hipMemcpyDeviceToHost));
    if (sib_H32 && S) HIPCHK(hipMemcpy(sib_H32, cur.H.p + s0 * 8, S * 32, hipMemcpyDeviceToHost));
    if (range_out && B) HIPCHK(hipMemcpy(range_out, (const uint8_t*)s->range.p + r0, B, hipMemcpyDeviceToHost));
    return DAPOL_OK;
}

int32_t dapol_batch_store_fetch(dapol_batch_store* s, size_t k, const uint64_t* row, uint8_t* sib_C32, uint8_t* sib_H32, uint8_t* range_out) {
    WIRE_SCOPE();
    RCCHK(batch_store_usable(s));
    if (k == 0) return DAPOL_OK;
    if (!row) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<uint64_t> q_sib_off(k + 1), q_piece_off(k + 1);
    if (!batch_store_fetch_offsets(k, row, s->rows(), s->L.sib_off.data(), s->L.range_off.data(), q_sib_off.data(), q_piece_off.data()))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "a row number is not below the rows of the batch store");
    std::vector<uint32_t> row32(k);
    for (size_t i = 0; i < k; i++) row32[i] = (uint32_t)row[i];
    dapol_ctx* ctx = s->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t Tq = (size_t)q_sib_off[k], Pq = (size_t)q_piece_off[k];
    // one staging buffer: the queried rows and their staging offsets, then what goes back -- commitments, hashes, blobs
    const size_t sizes[6] = {k * 4, (k + 1) * 8, (k + 1) * 8, Tq * 32, Tq * 32, Pq * 16};
    size_t offs[6], total = 0;
    for (int i = 0; i < 6; i++) { offs[i] = total; total += align_up(sizes[i], 256); }
    DevBuf<uint8_t> stage;
    StreamDrain drain{st};
    HIPCHK(stage.alloc(total));
    uint32_t* drow = (uint32_t*)(stage.p + offs[0]);
    uint64_t *dq_sib = (uint64_t*)(stage.p + offs[1]), *dq_piece = (uint64_t*)(stage.p + offs[2]);
    HIPCHK(hipMemcpyAsync(drow, row32.data(), sizes[0], hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dq_sib, q_sib_off.data(), sizes[1], hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dq_piece, q_piece_off.data(), sizes[2], hipMemcpyHostToDevice, st));
    const dapol_batch_store::Siblings& cur = s->set[s->cur];
    if (Pq + 4 * Tq) {
        hipLaunchKernelGGL(k_batch_store_fetch, dim3(nblk(Pq + 4 * Tq, 256)), dim3(256), 0, st, k, Pq, 2 * Tq, drow, dq_piece, s->L.piece_off.p, dq_sib, s->L.d_sib_off.p,
                           (const uint4*)s->range.p, (const uint4*)cur.C.p, (const uint4*)cur.H.p, (uint4*)(stage.p + offs[5]), (uint4*)(stage.p + offs[3]),
                           (uint4*)(stage.p + offs[4]));
        LAUNCH_CHECK();
    }
    HIPCHK(hipStreamSynchronize(st));
    if (sib_C32 && sizes[3]) HIPCHK(hipMemcpy(sib_C32, stage.p + offs[3], sizes[3], hipMemcpyDeviceToHost));
    if (sib_H32 && sizes[4]) HIPCHK(hipMemcpy(sib_H32, stage.p + offs[4], sizes[4], hipMemcpyDeviceToHost));
    if (range_out && sizes[5]) HIPCHK(hipMemcpy(range_out, stage.p + offs[5], sizes[5], hipMemcpyDeviceToHost));
    return DAPOL_OK;
}

// dapol_verify_batches over the store's rows with every input on the device already: the arena's leaf slots are filled from level 0 of
// the tree (k_store_leaves, by the positions k_tree_find_leaves gives), its sibling slots from the set in use, the root from the top
// level; the blobs are read where they lie.  Only the verdict bytes are copied back.
int32_t dapol_batch_store_verify(dapol_batch_store* s, const uint8_t verify_seed32[32], uint8_t* ok) {
    WIRE_SCOPE();
    RCCHK(batch_store_usable(s));
    const size_t nb = s->rows();
    if (nb == 0) return DAPOL_OK;
    if (!ok) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    VERIFY_SEED_OR_OS(verify_seed32)
    dapol_ctx* ctx = s->ctx;
    dapol_tree* tree = s->tree;
    VerifyBatchesPlan V;
    RCCHK(verify_batches_plan(ctx, tree->height, nb, s->batch_off.data(), s->leaf_idx.data(), s->L.sib_off.data(), s->policy, s->agg, s->n_bits,
                              s->L.range_off.data(), nullptr, V));
    const size_t K = V.K, T = V.Tc;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<uint32_t> aC, aH, droot, dseed, dpos, dmissing;
    DevBuf<uint8_t> dok;
    StreamDrain drain{st};
    HIPCHK(aC.alloc(V.slots * 8 + 8)); HIPCHK(aH.alloc(V.slots * 8 + 8)); HIPCHK(droot.alloc(16)); HIPCHK(dseed.alloc(8)); HIPCHK(dpos.alloc(K));
    HIPCHK(dmissing.alloc(1)); HIPCHK(dok.alloc(nb));
    HIPCHK(hipMemsetAsync(dmissing.p, 0, 4, st));
    HIPCHK(hipMemcpyAsync(dseed.p, verify_seed32, 32, hipMemcpyHostToDevice, st));
    const LevelView l0 = tree->view(0), top = tree->view(tree->height);
    hipLaunchKernelGGL(k_tree_find_leaves, dim3(nblk(K, 256)), dim3(256), 0, st, K, s->L.leaf.p, l0.n, l0.idx, dpos.p, dmissing.p);
    LAUNCH_CHECK();
    uint32_t h_missing = 0;
    HIPCHK(hipMemcpyAsync(&h_missing, dmissing.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_missing) return fail(DAPOL_ERR_UNKNOWN_LEAF, "a leaf of the batch store is no longer a leaf of the tree: refresh the store without its batches");
    hipLaunchKernelGGL(k_store_leaves, dim3(nblk(K * 4, 256)), dim3(256), 0, st, K, (size_t)2, dpos.p, (const uint4*)l0.C, (const uint4*)l0.H, (uint4*)aC.p,
                       (uint4*)aH.p);
    LAUNCH_CHECK();
    const dapol_batch_store::Siblings& cur = s->set[s->cur];
    if (T) {
        HIPCHK(hipMemcpyAsync(aC.p + K * 8, cur.C.p, T * 32, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(aH.p + K * 8, cur.H.p, T * 32, hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(droot.p, top.C, 32, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(droot.p + 8, top.H, 32, hipMemcpyDeviceToDevice, st));
    RCCHK(verify_batches_device(ctx, V, nb, s->n_bits, aC.p, aH.p, s->range.p, droot.p, dseed.p, dok.p));
    HIPCHK(hipMemcpy(ok, dok.p, nb, hipMemcpyDeviceToHost));
    return DAPOL_OK;
}

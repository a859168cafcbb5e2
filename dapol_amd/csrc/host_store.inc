// dapol_proof_store_*: the proofs dapol_prove_entities_shared issues for one (context, tree, policy, aggregation factor, n_bits, nonce
// seed), kept in HBM between calls and re-proved in place after an edit of the tree (definitions: include/dapol_hip.h; index arithmetic:
// store_plan.inc; kernels: kernels_store.h).  dapol_reprove_entities_shared uploads the caller's old paths and blobs and downloads all
// of the new ones, and that trip is most of its time; here the old data is where the last refresh left it, a refresh hands the re-prover's
// device side (entity_paths_device, reprove_policy_device) the store's own buffers, and only the rows a caller asks for cross the bus.
// The reference has nothing like it.

struct dapol_proof_store {
    dapol_ctx* ctx = nullptr;              // retained
    dapol_tree* tree = nullptr;            // counted (dapol_tree::stores): the tree outlives the store
    int policy = 0, agg = 0, n_bits = 0, leaf_first = 0;      // leaf_first: dapol_wire_config.siblings_leaf_first at creation
    EntityShape S;                         // H siblings per row, es bytes of blob per row, the policy's plan
    DevBuf<uint32_t> seed;                 // the nonce seed, 8 words
    size_t rows = 0;
    DevBuf<uint64_t> idx;                  // [rows] leaf indexes, strictly increasing
    struct Siblings { DevBuf<uint32_t> C, H; } set[2];       // [rows][H][8] commitments, [rows][H][hash words] hashes: set[cur] holds the rows'
    int cur = 0;                           // paths, the other one is the spare a refresh gathers into (empty until it has the right size)
    DevBuf<uint32_t> range;                // [rows][es / 4] blobs
    bool invalid = false;                  // a refresh failed after its first write into the store: rows and blobs may disagree
};
struct StorePoison {                       // armed before the first write of an in-place refresh, disarmed when the last one has completed
    dapol_proof_store* s;
    bool armed = false;
    ~StorePoison() { if (armed) s->invalid = true; }
};

// What every call refuses: no store, an invalid tree, a store left inconsistent, a sibling order other than the recorded one.
static int32_t store_usable(const dapol_proof_store* s) {
    if (!s) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null proof store");
    TREE_USABLE(s->tree);
    if (s->invalid)
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "the proof store was left inconsistent by a refresh that failed midway: destroy it and create it again");
    if ((g_wire.siblings_leaf_first != 0) != (s->leaf_first != 0))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "dapol_wire_config.siblings_leaf_first differs from the order the proof store was created under");
    return DAPOL_OK;
}
static void store_release_rows(dapol_proof_store* s) {
    s->idx.release(); s->range.release();
    for (auto& x : s->set) { x.C.release(); x.H.release(); }
    s->rows = 0; s->cur = 0;
}

int32_t dapol_proof_store_create(dapol_ctx* ctx, dapol_tree* tree, int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t nonce_seed32[32],
                                 dapol_proof_store** out) {
    WIRE_SCOPE();
    EntityShape S;
    int32_t rc = entity_shape(ctx, tree, nonce_seed32 && out, "null or out-of-range argument", 0, policy, aggregation_factor, n_bits, true, true, S);
    if (rc) return rc;
    TREE_USABLE(tree);
    if (!static_cast<dapol_tree_owned*>(tree)->leaves.idx.p)
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "tree does not own its leaves (workload tree): a proof store needs a tree of dapol_tree_build");
    HIPCHK(hipSetDevice(ctx->device));
    dapol_proof_store* s = new dapol_proof_store();
    struct Guard { dapol_proof_store* s; ~Guard() { delete s; } } guard{s};
    HIPCHK(s->seed.alloc(8));
    HIPCHK(hipMemcpy(s->seed.p, nonce_seed32, 32, hipMemcpyHostToDevice));
    s->ctx = ctx; s->tree = tree;
    s->policy = policy; s->agg = aggregation_factor; s->n_bits = n_bits;
    s->leaf_first = g_wire.siblings_leaf_first != 0 ? 1 : 0;
    s->S = std::move(S);
    ctx_retain(ctx);
    tree->stores.n++;
    guard.s = nullptr;
    *out = s;
    return DAPOL_OK;
}

int32_t dapol_proof_store_destroy(dapol_proof_store* s) {
    if (!s) return DAPOL_OK;
    dapol_ctx* ctx = s->ctx;
    (void)hipSetDevice(ctx->device);
    if (s->seed.p) (void)hipMemset(s->seed.p, 0, 32);          // the seed does not outlive the store in freed memory
    s->tree->stores.n--;
    delete s;
    (void)dapol_ctx_destroy(ctx);
    return DAPOL_OK;
}

size_t dapol_proof_store_rows(dapol_proof_store* s) {
    if (!s) { (void)fail(DAPOL_ERR_INVALID_ARGUMENT, "null proof store"); return 0; }
    return s->rows;
}
size_t dapol_proof_store_entity_bytes(dapol_proof_store* s) {
    if (!s) { (void)fail(DAPOL_ERR_INVALID_ARGUMENT, "null proof store"); return 0; }
    return s->S.es;
}

int32_t dapol_proof_store_refresh(dapol_proof_store* s, size_t b, const uint64_t* leaf_idx, uint64_t* proved_out, uint64_t* kept_out, uint64_t* moved_rows_out) {
    WIRE_SCOPE();
    int32_t rc = store_usable(s);
    if (rc) return rc;
    if (b && !leaf_idx) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (!strictly_increasing(b, leaf_idx)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "leaf indexes must be strictly increasing");
    dapol_ctx* ctx = s->ctx;
    dapol_tree* tree = s->tree;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool all = !leaf_idx && !b;                          // every leaf of the tree, from its own device array
    const size_t nb = all ? tree->levels[0].n : b;
    uint64_t proved = 0, kept = 0, moved = 0;
    if (nb) {
        const int H = s->S.H;
        const size_t hw = (size_t)ctx_hw(ctx), tot = nb * (size_t)H, ep = s->S.es / 16, cp = 2 * (size_t)H;
        // ---- everything that can refuse or fail to allocate, before anything of the store is written
        DevBuf<uint64_t> nidx, pv;
        DevBuf<uint32_t> pr, pos, src, flag, rank, freshC, freshH, nrange, cmpC;
        DevBuf<uint8_t> has;
        HIPCHK(nidx.alloc(nb)); HIPCHK(pv.alloc(tot)); HIPCHK(pr.alloc(tot * 8)); HIPCHK(pos.alloc(nb));
        HIPCHK(src.alloc(nb)); HIPCHK(flag.alloc(nb)); HIPCHK(rank.alloc(nb)); HIPCHK(has.alloc(nb));
        dapol_proof_store::Siblings& spare = s->set[s->cur ^ 1];
        const bool spare_fits = spare.C.n == tot * 8 && spare.H.n == tot * hw;
        if (!spare_fits) { HIPCHK(freshC.alloc(tot * 8)); HIPCHK(freshH.alloc(tot * hw)); }
        uint32_t *nC = spare_fits ? spare.C.p : freshC.p, *nH = spare_fits ? spare.H.p : freshH.p;
        HIPCHK(hipMemcpyAsync(nidx.p, all ? tree->leaf_idx : leaf_idx, nb * 8, all ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        if (s->rows) {
            hipLaunchKernelGGL(k_store_align, dim3(nblk(nb, 256)), dim3(256), 0, st, nb, nidx.p, s->rows, s->idx.p, src.p, has.p, flag.p);
            LAUNCH_CHECK();
            if ((rc = inclusive_scan_u32(st, flag.p, rank.p, nb))) return rc;
            uint32_t with_old = 0;
            HIPCHK(hipMemcpy(&with_old, rank.p + (nb - 1), 4, hipMemcpyDeviceToHost));
            moved = with_old;
        } else HIPCHK(hipMemsetAsync(has.p, 0, nb, st));
        const bool in_place = store_same_leaf_set(s->rows, nb, (size_t)moved);
        if (!in_place) {
            HIPCHK(nrange.alloc(nb * (s->S.es / 4)));
            if (moved) HIPCHK(cmpC.alloc(tot * 8));
        }
        // the paths of the tree as it is now, into the spare set (DAPOL_ERR_UNKNOWN_LEAF for an index that is no leaf)
        if ((rc = entity_paths_device(tree, nb, nidx.p, UpperDev{}, PathOut{nC, nH, pv.p, pr.p}, pos.p))) return rc;
        if (in_place) {
            // ---- the same leaves: the blobs stay where they are, the old commitments are the set in use, only dirty pieces are written.
            // reprove_policy_device allocates before its one write (k_reprove_scatter), so what it refuses (the plan's limits) or cannot
            // allocate leaves the store as it was; any other failure may have come after that write.
            StorePoison poison{s, true};
            moved = 0;
            rc = reprove_policy_device(ctx, s->S.plan, nb, H, pv.p, pr.p, nC, s->n_bits, s->seed.p, s->idx.p, nullptr, s->set[s->cur].C.p, s->range.p, &proved,
                                       &kept);
            if (rc) { poison.armed = rc != DAPOL_ERR_OUT_OF_MEMORY && rc != DAPOL_ERR_INVALID_ARGUMENT; return rc; }
            if (!spare_fits) { spare.C = std::move(freshC); spare.H = std::move(freshH); }
            s->cur ^= 1;
            poison.armed = false;
        } else {
            // ---- rows move: everything is written into new buffers, and the store takes them over only when all of it has succeeded
            if (moved) {
                hipLaunchKernelGGL(k_store_move, dim3(nblk(nb * (ep + cp), 256)), dim3(256), 0, st, nb, ep, cp, src.p, (const uint4*)s->range.p,
                                   (const uint4*)s->set[s->cur].C.p, (uint4*)nrange.p, (uint4*)cmpC.p);
                LAUNCH_CHECK();
            }
            rc = reprove_policy_device(ctx, s->S.plan, nb, H, pv.p, pr.p, nC, s->n_bits, s->seed.p, nidx.p, has.p, moved ? cmpC.p : nullptr, nrange.p, &proved, &kept);
            if (rc) return rc;
            if (!spare_fits) { spare.C = std::move(freshC); spare.H = std::move(freshH); }
            s->cur ^= 1;
            s->idx = std::move(nidx); s->range = std::move(nrange);       // (the old buffers are freed here, after the scatter has drained)
            s->rows = nb;
            dapol_proof_store::Siblings& old = s->set[s->cur ^ 1];        // of another size now: the next refresh allocates its spare
            if (old.C.n != tot * 8 || old.H.n != tot * hw) { old.C.release(); old.H.release(); }
        }
    } else store_release_rows(s);
    if (proved_out) *proved_out = proved;
    if (kept_out) *kept_out = kept;
    if (moved_rows_out) *moved_rows_out = moved;
    return DAPOL_OK;
}

int32_t dapol_proof_store_read(dapol_proof_store* s, size_t first, size_t count, uint64_t* leaf_idx_out, uint8_t* path_C32, uint8_t* path_H32, uint8_t* range_out) {
    WIRE_SCOPE();
    int32_t rc = store_usable(s);
    if (rc) return rc;
    if (first > s->rows || count > s->rows - first) return fail(DAPOL_ERR_INVALID_ARGUMENT, "first + count exceeds the rows of the proof store");
    if (count == 0) return DAPOL_OK;
    HIPCHK(hipSetDevice(s->ctx->device));
    const size_t H = (size_t)s->S.H, hw = (size_t)ctx_hw(s->ctx);
    const dapol_proof_store::Siblings& cur = s->set[s->cur];
    if (leaf_idx_out) HIPCHK(hipMemcpy(leaf_idx_out, s->idx.p + first, count * 8, hipMemcpyDeviceToHost));
    if (path_C32 && H) HIPCHK(hipMemcpy(path_C32, cur.C.p + first * H * 8, count * H * 32, hipMemcpyDeviceToHost));
    if (path_H32 && H) HIPCHK(hipMemcpy(path_H32, cur.H.p + first * H * hw, count * H * hw * 4, hipMemcpyDeviceToHost));
    if (range_out) HIPCHK(hipMemcpy(range_out, s->range.p + first * (s->S.es / 4), count * s->S.es, hipMemcpyDeviceToHost));
    return DAPOL_OK;
}

int32_t dapol_proof_store_fetch(dapol_proof_store* s, size_t k, const uint64_t* leaf_idx, uint8_t* found, uint8_t* path_C32, uint8_t* path_H32, uint8_t* range_out) {
    WIRE_SCOPE();
    int32_t rc = store_usable(s);
    if (rc) return rc;
    if (k == 0) return DAPOL_OK;
    if (!leaf_idx) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    dapol_ctx* ctx = s->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t H = (size_t)s->S.H, hw = (size_t)ctx_hw(ctx), ep = s->S.es / 16, cp = 2 * H, hp = H * hw / 4;
    // one staging buffer: the queries, their rows, then what goes back -- found bytes, commitments, hashes, blobs
    const size_t sizes[6] = {k * 8, k * 4, k, k * cp * 16, k * hp * 16, k * ep * 16};
    size_t offs[6], total = 0;
    for (int i = 0; i < 6; i++) { offs[i] = total; total += align_up(sizes[i], 256); }
    DevBuf<uint8_t> stage;
    HIPCHK(stage.alloc(total));
    uint64_t* dq = (uint64_t*)(stage.p + offs[0]);
    uint32_t* drow = (uint32_t*)(stage.p + offs[1]);
    uint8_t* dfound = stage.p + offs[2];
    HIPCHK(hipMemcpyAsync(dq, leaf_idx, k * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_store_find, dim3(nblk(k, 256)), dim3(256), 0, st, k, dq, s->rows, s->idx.p, drow, dfound);
    LAUNCH_CHECK();
    const dapol_proof_store::Siblings& cur = s->set[s->cur];
    hipLaunchKernelGGL(k_store_fetch, dim3(nblk(k * (ep + cp + hp), 256)), dim3(256), 0, st, k, ep, cp, hp, drow, (const uint4*)s->range.p, (const uint4*)cur.C.p,
                       (const uint4*)cur.H.p, (uint4*)(stage.p + offs[5]), (uint4*)(stage.p + offs[3]), (uint4*)(stage.p + offs[4]));
    LAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(st));
    if (found) HIPCHK(hipMemcpy(found, dfound, k, hipMemcpyDeviceToHost));
    if (path_C32 && sizes[3]) HIPCHK(hipMemcpy(path_C32, stage.p + offs[3], sizes[3], hipMemcpyDeviceToHost));
    if (path_H32 && sizes[4]) HIPCHK(hipMemcpy(path_H32, stage.p + offs[4], sizes[4], hipMemcpyDeviceToHost));
    if (range_out) HIPCHK(hipMemcpy(range_out, stage.p + offs[5], sizes[5], hipMemcpyDeviceToHost));
    return DAPOL_OK;
}

// dapol_verify_entities over the store's rows with every input on the device already: the leaves' own commitments and hashes from
// level 0 of the tree, the root from its top level, the Merkle re-merge by k_verify_paths and the range checks by verify_policy_device
// on the store's arrays.  Only the verdict bytes are copied back.
int32_t dapol_proof_store_verify(dapol_proof_store* s, const uint8_t verify_seed32[32], uint8_t* ok) {
    WIRE_SCOPE();
    int32_t rc = store_usable(s);
    if (rc) return rc;
    const size_t b = s->rows;
    if (b == 0) return DAPOL_OK;
    if (!ok) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    VERIFY_SEED_OR_OS(verify_seed32)
    dapol_ctx* ctx = s->ctx;
    dapol_tree* tree = s->tree;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int H = s->S.H;
    const size_t hw = (size_t)ctx_hw(ctx);
    int max_m = 1;
    for (auto& sp : s->S.plan) if (sp.m > max_m) max_m = sp.m;
    const size_t sizes[9] = {b * 32, b * hw * 4, b * 4, 256, 32, b, b, b, b * (size_t)max_m * 32};
    size_t offs[9], total = 0;
    for (int i = 0; i < 9; i++) { offs[i] = total; total += align_up(sizes[i], 256); }
    DevBuf<uint8_t> arena;
    HIPCHK(arena.alloc(total));
    uint8_t* base = arena.p;
    uint32_t *dLC = (uint32_t*)(base + offs[0]), *dLH = (uint32_t*)(base + offs[1]), *dpos = (uint32_t*)(base + offs[2]), *dmissing = (uint32_t*)(base + offs[3]);
    uint32_t *dseed = (uint32_t*)(base + offs[4]), *dV = (uint32_t*)(base + offs[8]);
    uint8_t *dok = base + offs[5], *dsub = base + offs[6], *dpath = base + offs[7];
    HIPCHK(hipMemsetAsync(dmissing, 0, 4, st));
    HIPCHK(hipMemcpyAsync(dseed, verify_seed32, 32, hipMemcpyHostToDevice, st));
    const LevelView l0 = tree->view(0), top = tree->view(tree->height);
    hipLaunchKernelGGL(k_tree_find_leaves, dim3(nblk(b, 256)), dim3(256), 0, st, b, s->idx.p, l0.n, l0.idx, dpos, dmissing);
    LAUNCH_CHECK();
    uint32_t h_missing = 0;
    HIPCHK(hipMemcpyAsync(&h_missing, dmissing, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_missing) return fail(DAPOL_ERR_UNKNOWN_LEAF, "a leaf of the proof store is no longer a leaf of the tree: refresh the store");
    const bool wide = ctx_wide(ctx);
    const uint32_t* H0 = wide ? tree->wviews[0].H : l0.H;
    const uint32_t* rootH = wide ? tree->wviews[tree->height].H : top.H;
    hipLaunchKernelGGL(k_store_leaves, dim3(nblk(b * (2 + hw / 4), 256)), dim3(256), 0, st, b, hw / 4, dpos, (const uint4*)l0.C, (const uint4*)H0, (uint4*)dLC,
                       (uint4*)dLH);
    LAUNCH_CHECK();
    const dapol_proof_store::Siblings& cur = s->set[s->cur];
    if (wide)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_verify_paths<16, DG_RUNTIME>), dim3(nblk(b, 64)), dim3(64), 0, st, ctx->tv.digest, b, H, s->idx.p, dLC, dLH, cur.C.p, cur.H.p, top.C, rootH,
                           g_wire.siblings_leaf_first, dpath);
    else
        LAUNCH_DX(ctx->tv.digest, (k_verify_paths<8, DX>), dim3(nblk(b, 64)), dim3(64), 0, st, ctx->tv.digest, b, H, s->idx.p, dLC, dLH, cur.C.p, cur.H.p, top.C, rootH,
                           g_wire.siblings_leaf_first, dpath);
    LAUNCH_CHECK();
    HIPCHK(hipMemsetAsync(dok, 1, b, st));
    if ((rc = verify_policy_device(ctx, s->S.plan, b, H, cur.C.p, s->range.p, s->S.es / 4, s->n_bits, dseed, dok, dsub, dV))) return rc;
    hipLaunchKernelGGL(k_and_bytes, dim3(nblk(b, 256)), dim3(256), 0, st, b, dok, dpath);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpy(ok, dok, b, hipMemcpyDeviceToHost));
    return DAPOL_OK;
}

// Every stored row in the compact layout of the stored leaf indexes (shared_compact_plan.inc): the key heads over the store's own
// indexes, a scan, one gather out of the blobs into a staging buffer of exactly the compact length, one copy back.
int32_t dapol_proof_store_read_compact(dapol_proof_store* s, uint8_t* compact_out, size_t compact_cap, uint64_t* compact_len_out) {
    WIRE_SCOPE();
    int32_t rc = store_usable(s);
    if (rc) return rc;
    const size_t b = s->rows;
    uint64_t len = 0;
    if (b) {
        dapol_ctx* ctx = s->ctx;
        HIPCHK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        SharedPlanDev P;
        if ((rc = shared_plan_dev_build(s->S.plan, b, s->S.H, s->n_bits, P))) return rc;
        const size_t nf = (size_t)P.n_sub * b + 1;
        DevBuf<uint32_t> flag, rank, stage;
        HIPCHK(flag.alloc(nf)); HIPCHK(rank.alloc(nf));
        hipLaunchKernelGGL(k_shared_heads, dim3(nblk(nf, 256)), dim3(256), 0, st, P, b, s->idx.p, flag.p);
        LAUNCH_CHECK();
        if ((rc = inclusive_scan_u32(st, flag.p, rank.p, nf))) return rc;
        std::vector<uint32_t> g_first(P.n_groups + 1);           // compact row at which each group starts; the last one: all of them
        for (uint32_t gi = 0; gi <= P.n_groups; gi++) {
            const size_t at = gi < P.n_groups ? (size_t)P.g[gi].s0 * b : nf - 1;
            HIPCHK(hipMemcpyAsync(&g_first[gi], rank.p + at, 4, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        for (uint32_t gi = 0; gi < P.n_groups; gi++) g_first[gi]--;
        size_t words = 0;
        for (uint32_t gi = 0; gi < P.n_groups; gi++) {
            P.g[gi].word_off = words;
            words += (size_t)(g_first[gi + 1] - g_first[gi]) * (size_t)P.g[gi].pieces * 4;
        }
        len = (uint64_t)words * 4;
        if (len > (uint64_t)compact_cap) return fail(DAPOL_ERR_INVALID_ARGUMENT, "compact_cap is below the length of the compact layout");
        if (!compact_out) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
        HIPCHK(stage.alloc(words));
        hipLaunchKernelGGL(k_store_compact, dim3(nblk(b * (size_t)P.entity_pieces, 256)), dim3(256), 0, st, P, b, flag.p, rank.p, (const uint4*)s->range.p,
                           (uint4*)stage.p);
        LAUNCH_CHECK();
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(compact_out, stage.p, (size_t)len, hipMemcpyDeviceToHost));
    }
    if (compact_len_out) *compact_len_out = len;
    return DAPOL_OK;
}

// dapol_reprove_entities_shared / dapol_reprove_plan: after an edit of the tree, only the sub-proofs whose sibling commitments moved
// are proven again (definitions: include/dapol_hip.h; index arithmetic: reprove_plan.inc; kernels: kernels_reprove.h).  A sub-proof
// {start, count, m} is a statement about `count` sibling commitments, and its nonce key is bound to them, so unchanged commitments
// mean unchanged bytes: the caller's old proof is kept.  The reference has nothing like it (its generate_all_proofs DFS proves all).

int32_t dapol_reprove_plan(int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* has_old, size_t k, const uint64_t* edited_idx, int32_t policy,
                           int32_t aggregation_factor, uint64_t* n_proved_out, uint64_t* total_proved, uint64_t* sum_m_proved, uint64_t* sum_m_shared) {
    WIRE_SCOPE();
    if ((b && !leaf_idx) || (k && !edited_idx)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (height < 0 || height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    std::vector<SubProof> plan;
    if (!policy_plan(policy, height, aggregation_factor, plan)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad policy / aggregation_factor");
    ReprovePlanOut out;
    if (!reprove_plan_host(plan, height, g_wire.siblings_leaf_first != 0, b, leaf_idx, has_old, k, edited_idx, n_proved_out, out))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "leaf and edited indexes must be strictly increasing and below 2^height");
    if (total_proved) *total_proved = out.total_proved;
    if (sum_m_proved) *sum_m_proved = out.sum_m_proved;
    if (sum_m_shared) *sum_m_shared = out.sum_m_shared;
    return DAPOL_OK;
}

// The re-proving counterpart of prove_policy_shared_device.  pv / pr / pC are the gathered [b][H] siblings of the tree as it is now,
// d_oldC the uploaded old commitments (null when no row has old data), d_has_old a byte per row (null: every row has old data), and
// d_range holds the uploaded old blobs: only the dirty pieces of it are overwritten.
static int32_t reprove_policy_device(dapol_ctx* ctx, const std::vector<SubProof>& plan, size_t b, int H, const uint64_t* pv, const uint32_t* pr,
                                     const uint32_t* pC, int n_bits, const uint32_t* d_seed, const uint64_t* d_idx, const uint8_t* d_has_old,
                                     const uint32_t* d_oldC, uint32_t* d_range, uint64_t* proved_out, uint64_t* kept_out) {
    hipStream_t st = ctx->stream;
    SharedPlanDev P;
    int32_t rc = shared_plan_dev_build(plan, b, H, n_bits, P);
    if (rc) return rc;
    const size_t n = (size_t)P.n_sub * b, nf = n + 1;
    DevBuf<uint32_t> dirty, flag, rank;
    HIPCHK(dirty.alloc(nf)); HIPCHK(flag.alloc(nf)); HIPCHK(rank.alloc(nf));
    // (nf * REPROVE_LANES lanes: the pair one past the array writes the closing zero)
    hipLaunchKernelGGL(k_reprove_heads, dim3(nblk(nf * REPROVE_LANES, 256)), dim3(256), 0, st, P, b, d_idx, d_has_old, (const uint4*)d_oldC, (const uint4*)pC,
                       dirty.p, flag.p);
    LAUNCH_CHECK();
    rc = inclusive_scan_u32(st, flag.p, rank.p, nf);
    if (rc) return rc;
    // heads before each group (the scan's element before its first pair; row 0 of a group may be kept), and all of them
    std::vector<uint32_t> base(P.n_groups + 1, 0), gm(P.n_groups), gpieces(P.n_groups);
    for (uint32_t gi = 0; gi <= P.n_groups; gi++) {
        const size_t at = gi < P.n_groups ? reprove_base_at(P.g[gi].s0, b) : nf - 1;
        if (at != (size_t)-1) HIPCHK(hipMemcpyAsync(&base[gi], rank.p + at, 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t gi = 0; gi < P.n_groups; gi++) { gm[gi] = P.g[gi].m; gpieces[gi] = P.g[gi].pieces; }
    ReproveLayout L;
    reprove_layout(P.n_groups, base.data(), gm.data(), gpieces.data(), L);
    if (L.heads) {                                           // (nothing dirty: the range prover is not entered, nothing is allocated)
        ReproveBases B{};
        for (uint32_t gi = 0; gi < P.n_groups; gi++) { B.before[gi] = base[gi]; P.g[gi].word_off = L.word_off[gi]; }
        DevBuf<uint64_t> vals, stream;
        DevBuf<uint32_t> blind, Vc, proofs;
        HIPCHK(vals.alloc(L.parties)); HIPCHK(blind.alloc(L.parties * 8)); HIPCHK(Vc.alloc(L.parties * 8)); HIPCHK(stream.alloc(L.heads));
        HIPCHK(proofs.alloc(L.words));
        const uint32_t* Bb_comp = ctx->gens_comp.p + (size_t)ctx->tv.row_Bb(0) * 8;
        for (uint32_t gi = 0; gi < P.n_groups; gi++) {
            if (!L.U[gi]) continue;
            const SharedGroup& G = P.g[gi];
            hipLaunchKernelGGL(k_reprove_gather, dim3(nblk(b * (size_t)G.k * (size_t)G.m, 256)), dim3(256), 0, st, P, gi, base[gi], b, d_idx, flag.p, rank.p, pv,
                               pr, pC, Bb_comp, vals.p + L.party_off[gi], blind.p + L.party_off[gi] * 8, Vc.p + L.party_off[gi] * 8, stream.p + base[gi]);
            LAUNCH_CHECK();
        }
        // one call of the range prover per group that has heads, one after the other as prove_policy_shared_device's
        for (uint32_t gi = 0; gi < P.n_groups; gi++) {
            if (!L.U[gi]) continue;
            const SharedGroup& G = P.g[gi];
            rc = range_prove_device(ctx, n_bits, (int)G.m, L.U[gi], vals.p + L.party_off[gi], blind.p + L.party_off[gi] * 8, Vc.p + L.party_off[gi] * 8, d_seed,
                                    stream.p + base[gi], 0, nullptr, proofs.p + G.word_off, nullptr);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(k_reprove_scatter, dim3(nblk(b * (size_t)P.entity_pieces, 256)), dim3(256), 0, st, P, B, b, dirty.p, rank.p, (const uint4*)proofs.p,
                           (uint4*)d_range);
        LAUNCH_CHECK();
        HIPCHK(hipStreamSynchronize(st));                     // (the compact buffers go at the end of this block)
    }
    // kept pairs = all pairs - dirty ones: a second scan, over the dirty flags (the ranks are no longer needed)
    uint32_t n_dirty = 0;
    rc = inclusive_scan_u32(st, dirty.p, rank.p, n);
    if (rc) return rc;
    HIPCHK(hipMemcpy(&n_dirty, rank.p + (n - 1), 4, hipMemcpyDeviceToHost));
    if (proved_out) *proved_out = L.heads;
    if (kept_out) *kept_out = (uint64_t)n - n_dirty;
    return DAPOL_OK;
}

int32_t dapol_reprove_entities_shared(dapol_ctx* ctx, dapol_tree* tree, size_t b, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor,
                                      int32_t n_bits, const uint8_t nonce_seed32[32], const uint8_t* has_old, const uint8_t* old_path_C32,
                                      const uint8_t* old_range, uint8_t* path_C32, uint8_t* path_H32, uint8_t* range_out, uint64_t* proved_out,
                                      uint64_t* kept_out) {
    WIRE_SCOPE();
    EntityShape S;
    int32_t rc = entity_shape(ctx, tree, nonce_seed32 && (!b || (leaf_idx && range_out)), "null or out-of-range argument", 0, policy, aggregation_factor, n_bits,
                              true, true, S);
    if (rc) return rc;
    if (!strictly_increasing(b, leaf_idx)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "leaf indexes must be strictly increasing");
    bool any_old = has_old == nullptr && b > 0;
    for (size_t e = 0; has_old && e < b && !any_old; e++) any_old = has_old[e] != 0;
    if (any_old && (!old_path_C32 || !old_range))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "old_path_C32 and old_range are needed while some row has old data (has_old set, or NULL)");
    uint64_t proved = 0, kept = 0;
    if (b) {
        EntityProveCall call;
        DevBuf<uint32_t> doldC;
        DevBuf<uint8_t> dhas;
        hipStream_t st = ctx->stream;
        // every input goes up before anything is written back: the outputs may alias the old arrays
        if ((rc = call.open(ctx, tree, S, b, leaf_idx, nonce_seed32, 0, nullptr, nullptr, nullptr, nullptr))) return rc;
        if (has_old) { HIPCHK(dhas.alloc(b)); HIPCHK(hipMemcpyAsync(dhas.p, has_old, b, hipMemcpyHostToDevice, st)); }
        if (any_old) {
            HIPCHK(doldC.alloc(call.tot * 8));
            if (call.tot) HIPCHK(hipMemcpyAsync(doldC.p, old_path_C32, call.tot * 32, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(call.out.p, old_range, b * S.es, hipMemcpyHostToDevice, st));      // the old blobs ARE the output buffer: kept rows never move
        }
        if ((rc = call.paths())) return rc;
        rc = reprove_policy_device(ctx, S.plan, b, S.H, call.pv.p, call.pr.p, call.pathC.p, n_bits, call.seed.p, call.idx.p, dhas.p, doldC.p, call.out.p, &proved, &kept);
        if (rc || (rc = call.download(path_C32, path_H32, range_out))) return rc;
    }
    if (proved_out) *proved_out = proved;
    if (kept_out) *kept_out = kept;
    return DAPOL_OK;
}

// dapol_verify_entities_shared: dapol_verify_entities with every run of equal sub-proofs of a call checked once (kernels in
// kernels_verify_shared.h, index arithmetic in verify_shared_plan.inc, definition in include/dapol_hip.h).  The counterpart of
// host_shared.inc: there equal subtree keys mark the rows that share a statement, here nothing is trusted but the bytes -- row e of
// sub-proof s repeats row e - 1 iff its proof bytes and the sibling commitments the proof covers are equal.

// The device buffers of one shared call: owned by verify_policy_shared_device, which drains the stream before they go.
struct VSharedBufs {
    DevBuf<uint32_t> flag, rank;         // [plan][b] + 1
    DevBuf<VsPiece> proofs, Vc;          // the compact batches, group after group
    DevBuf<uint8_t> sub;                 // a verdict per head
};
static int32_t verify_policy_shared_queue(dapol_ctx* ctx, const VSharedPlan& P, size_t b, const uint32_t* dPC, const uint32_t* dR, int n_bits,
                                          const uint32_t* dseed, uint8_t* dok, uint64_t* unique_out, VSharedBufs& B) {
    hipStream_t st = ctx->stream;
    const VsPiece *blobs = (const VsPiece*)dR, *pC = (const VsPiece*)dPC;
    DevBuf<uint32_t>&flag = B.flag, &rank = B.rank;
    DevBuf<VsPiece>&proofs = B.proofs, &Vc = B.Vc;
    DevBuf<uint8_t>& sub = B.sub;
    if (!vshared_gather_fits(P, b)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "too many sub-proofs in one call");    // (far beyond any device's memory)
    // heads and ranks, as prove_policy_shared_device: rank[s][e] = heads up to and including (s, e) in plan order
    const size_t nf = (size_t)P.n_sub * b + 1;
    HIPCHK(flag.alloc(nf)); HIPCHK(rank.alloc(nf));
    hipLaunchKernelGGL(k_vshared_heads, dim3(nblk(nf * VSHARED_LANES, 256)), dim3(256), 0, st, P, b, blobs, pC, flag.p);
    LAUNCH_CHECK();
    int32_t rc = inclusive_scan_u32(st, flag.p, rank.p, nf);
    if (rc) return rc;
    uint32_t rank_at[VSHARED_MAX_GROUPS + 1];
    for (uint32_t gi = 0; gi <= P.n_groups; gi++) {
        const size_t at = gi < P.n_groups ? (size_t)P.g[gi].s0 * b : nf - 1;
        HIPCHK(hipMemcpyAsync(&rank_at[gi], rank.p + at, 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    VSharedLayout L;
    vshared_layout(P, rank_at, L);
    const size_t U = L.first[P.n_groups];
    // compact gather: the head rows' proofs and parties, group after group
    HIPCHK(proofs.alloc(L.pieces)); HIPCHK(Vc.alloc(L.parties * 2)); HIPCHK(sub.alloc(U));
    const uint32_t* Bb_comp = ctx->gens_comp.p + (size_t)ctx->tv.row_Bb(0) * 8;
    for (uint32_t gi = 0; gi < P.n_groups; gi++) {
        const VSharedGroup& G = P.g[gi];
        const size_t lanes = b * (size_t)G.k * (size_t)vshared_gather_pieces(G);
        hipLaunchKernelGGL(k_vshared_gather, dim3(nblk(lanes, 256)), dim3(256), 0, st, P, gi, b, flag.p, rank.p, blobs, pC, Bb_comp,
                           proofs.p + L.piece_off[gi], Vc.p + L.party_off[gi] * 2);
        LAUNCH_CHECK();
    }
    // one batched check per group, one after the other: the same random linear combination with its eight-way split as everywhere in
    // the verifier, so the verdicts are the per-proof ones.  Each call returns after its kernels have drained.
    for (uint32_t gi = 0; gi < P.n_groups; gi++) {
        const VSharedGroup& G = P.g[gi];
        rc = range_verify_rlc_device(ctx, n_bits, (int)G.m, L.first[gi + 1] - L.first[gi], (const uint32_t*)(proofs.p + L.piece_off[gi]), (size_t)G.pieces * 4,
                                     (const uint32_t*)(Vc.p + L.party_off[gi] * 2), dseed, sub.p + L.first[gi]);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_vshared_verdict, dim3(nblk(b, 256)), dim3(256), 0, st, P, b, rank.p, sub.p, dok);
    LAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(st));
    if (unique_out) *unique_out = U;
    return DAPOL_OK;
}
// The range checks of b entities over the uploaded arena (dPC: [b][H][8] sibling commitments, dR: [b] blobs): ANDs of the heads'
// verdicts into dok[b]; *unique_out = heads = range proofs checked.  Returns with the stream drained, on every path: whatever was
// queued when an error came back has finished before the call's buffers are freed.
static int32_t verify_policy_shared_device(dapol_ctx* ctx, const VSharedPlan& P, size_t b, const uint32_t* dPC, const uint32_t* dR, int n_bits,
                                           const uint32_t* dseed, uint8_t* dok, uint64_t* unique_out) {
    VSharedBufs B;
    const int32_t rc = verify_policy_shared_queue(ctx, P, b, dPC, dR, n_bits, dseed, dok, unique_out, B);
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

int32_t dapol_verify_entities_shared(dapol_ctx* ctx, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* leaf_C32, const uint8_t* leaf_H32,
                                     size_t n_path_nodes, const uint8_t* path_C32, const uint8_t* path_H32, const uint8_t root_C32[32],
                                     const uint8_t root_H32[32], int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t* range_proofs,
                                     size_t range_proofs_len, const uint8_t verify_seed32[32], uint8_t* ok, uint64_t* unique_subproofs_out) {
    WIRE_SCOPE();
    if (!ctx || !root_C32 || !root_H32 || (b && (!leaf_idx || !leaf_C32 || !leaf_H32 || !path_C32 || !path_H32 || !range_proofs || !ok)))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    VERIFY_SEED_OR_OS(verify_seed32)
    if (height < 0 || height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    std::vector<SubProof> plan;
    if (!policy_plan(policy, height, aggregation_factor, plan)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad policy / aggregation_factor");
    const size_t es = dapol_entity_proof_size(height, policy, aggregation_factor, n_bits);
    if (es == 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad n_bits");
    int max_m = 1;
    for (auto& s : plan) if (s.m > max_m) max_m = s.m;
    if (b && max_m > ctx->max_parties) return fail(DAPOL_ERR_INVALID_ARGUMENT, "aggregation needs more parties than the context was created for");
    // a proof of the wrong shape is an invalid proof, never an over-read (dapol_verify_entities_checked)
    if (n_path_nodes != b * (size_t)height || range_proofs_len != b * es) {
        for (size_t i = 0; i < b; i++) ok[i] = 0;
        if (unique_subproofs_out) *unique_subproofs_out = 0;
        return DAPOL_OK;
    }
    if (b == 0) {
        if (unique_subproofs_out) *unique_subproofs_out = 0;
        return DAPOL_OK;
    }
    if (!vshared_call_fits(b, plan.size()))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "too many sub-proofs in one call (entities x (plan size + 1) must stay below 2^32)");
    // The latency regime (the lanes of verify_policy_device): nothing to gain, the existing path as it is.
    // (DAPOL_VSHARED_FORWARD_MAX, a limit override for tests/ behind both opt-ins: the small trees of the prover's tests go through
    // the kernels with 0)
    size_t forward_max = VSHARED_FORWARD_MAX;
    if (const char* e = test_knob("DAPOL_VSHARED_FORWARD_MAX")) { long long v = atoll(e); if (v >= 0) forward_max = (size_t)v; }
    if (vshared_forwards(b, plan.size(), forward_max)) {
        int32_t rc = dapol_verify_entities(ctx, height, b, leaf_idx, leaf_C32, leaf_H32, path_C32, path_H32, root_C32, root_H32, policy, aggregation_factor,
                                           n_bits, range_proofs, verify_seed32, ok);
        if (rc) return rc;
        if (unique_subproofs_out) *unique_subproofs_out = (uint64_t)b * (uint64_t)plan.size();
        return DAPOL_OK;
    }
    VSharedPlan P;
    if (vshared_plan_build(plan, height, n_bits, P)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "the plan has too many sub-proofs or runs of equal-sized sub-proofs");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    VerifyCallDev D;
    ForkGuard fg(ctx);
    int32_t rc = verify_upload_and_paths(ctx, fg, height, b, leaf_idx, leaf_C32, leaf_H32, path_C32, path_H32, root_C32, root_H32, es, range_proofs,
                                         verify_seed32, 0, D);
    if (rc) return rc;
    uint64_t unique = 0;
    rc = verify_policy_shared_device(ctx, P, b, D.dPC, D.dR, n_bits, D.dseed, D.dok, &unique);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }        // (the path kernel: on st, or behind the guard)
    if (D.side_paths) { HIPCHK(hipStreamWaitEvent(st, ctx->ev_join[2], 0)); fg.joined(2); }
    hipLaunchKernelGGL(k_and_bytes, dim3(nblk(b, 256)), dim3(256), 0, st, b, D.dok, D.dpath);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpy(ok, D.dok, b, hipMemcpyDeviceToHost));
    if (unique_subproofs_out) *unique_subproofs_out = unique;
    return DAPOL_OK;
}

// dapol_verify_entities_compact: dapol_verify_entities over the COMPACT form of shared proofs -- every distinct sub-proof uploaded
// once (kernels in kernels_verify_compact.h, index arithmetic in shared_compact_plan.inc, definition in include/dapol_hip.h).  The
// counterpart of host_verify_shared.inc: there the rows that repeat are rediscovered by comparing whole blobs, here the leaf indexes
// say which compact proof a row uses, and the sibling commitments -- the other half of the statement -- are still compared as bytes.

// The device buffers of one compact call: owned by verify_policy_compact_device, which drains the stream before they go.
struct VCompactBufs {
    DevBuf<uint32_t> kflag, hflag, kref, hrank;      // [plan][b] + 1 each
    DevBuf<VsPiece> proofs, Vc;                      // the verification batches, group after group
    DevBuf<uint8_t> sub;                             // a verdict per head
};
// sub_off: the host's layout of the uploaded compact buffer dR (scompact_layout over the same indexes as dl).
static int32_t verify_policy_compact_queue(dapol_ctx* ctx, const SCompactPlan& P, const uint64_t* sub_off, size_t b, const uint64_t* dl, const uint32_t* dPC,
                                           const uint32_t* dR, int n_bits, const uint32_t* dseed, uint8_t* dok, uint64_t* unique_out, VCompactBufs& B) {
    hipStream_t st = ctx->stream;
    const VSharedPlan& V = P.V;
    const VsPiece* pC = (const VsPiece*)dPC;
    if (!vshared_gather_fits(V, b)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "too many sub-proofs in one call");    // (far beyond any device's memory)
    // key flags and head flags in one pass, a scan each: kref names the compact proof row, hrank the verification row
    const size_t nf = (size_t)V.n_sub * b + 1;
    HIPCHK(B.kflag.alloc(nf)); HIPCHK(B.hflag.alloc(nf)); HIPCHK(B.kref.alloc(nf)); HIPCHK(B.hrank.alloc(nf));
    hipLaunchKernelGGL(k_vcompact_heads, dim3(nblk(nf * VCOMPACT_LANES, 256)), dim3(256), 0, st, P, b, dl, pC, B.kflag.p, B.hflag.p);
    LAUNCH_CHECK();
    int32_t rc = inclusive_scan_u32(st, B.kflag.p, B.kref.p, nf);
    if (rc || (rc = inclusive_scan_u32(st, B.hflag.p, B.hrank.p, nf))) return rc;
    uint32_t kref_at[VSHARED_MAX_GROUPS + 1], hrank_at[VSHARED_MAX_GROUPS + 1];
    for (uint32_t gi = 0; gi <= V.n_groups; gi++) {
        const size_t at = gi < V.n_groups ? (size_t)V.g[gi].s0 * b : nf - 1;
        HIPCHK(hipMemcpyAsync(&kref_at[gi], B.kref.p + at, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&hrank_at[gi], B.hrank.p + at, 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    // the gather reads compact rows that the device's key scan names inside slices that the host's layout places: they must agree
    for (uint32_t gi = 0; gi < V.n_groups; gi++) {
        const uint32_t s_end = V.g[gi].s0 + V.g[gi].k;
        const uint64_t rows = (sub_off[s_end] - sub_off[V.g[gi].s0]) / ((uint64_t)V.g[gi].pieces * 16);
        const uint64_t dev = (uint64_t)(gi + 1 < V.n_groups ? kref_at[gi + 1] - 1 : kref_at[V.n_groups]) - (uint64_t)(kref_at[gi] - 1);
        if (rows != dev) return fail(DAPOL_ERR_HIP, "internal error: the device counts other subtree keys than the host's layout");
    }
    VSharedLayout L;
    vshared_layout(V, hrank_at, L);
    const size_t heads = L.first[V.n_groups];
    HIPCHK(B.proofs.alloc(L.pieces)); HIPCHK(B.Vc.alloc(L.parties * 2)); HIPCHK(B.sub.alloc(heads));
    const uint32_t* Bb_comp = ctx->gens_comp.p + (size_t)ctx->tv.row_Bb(0) * 8;
    for (uint32_t gi = 0; gi < V.n_groups; gi++) {
        const VSharedGroup& G = V.g[gi];
        const size_t lanes = b * (size_t)G.k * (size_t)vshared_gather_pieces(G);
        hipLaunchKernelGGL(k_vcompact_gather, dim3(nblk(lanes, 256)), dim3(256), 0, st, P, gi, b, B.hflag.p, B.kref.p, B.hrank.p,
                           (const VsPiece*)((const uint8_t*)dR + sub_off[G.s0]), pC, Bb_comp, B.proofs.p + L.piece_off[gi], B.Vc.p + L.party_off[gi] * 2);
        LAUNCH_CHECK();
    }
    // one batched check per group, one after the other: the same random linear combination with its eight-way split as everywhere in
    // the verifier, so the verdicts are the per-proof ones.  Each call returns after its kernels have drained.
    for (uint32_t gi = 0; gi < V.n_groups; gi++) {
        const VSharedGroup& G = V.g[gi];
        rc = range_verify_rlc_device(ctx, n_bits, (int)G.m, L.first[gi + 1] - L.first[gi], (const uint32_t*)(B.proofs.p + L.piece_off[gi]), (size_t)G.pieces * 4,
                                     (const uint32_t*)(B.Vc.p + L.party_off[gi] * 2), dseed, B.sub.p + L.first[gi]);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_vcompact_verdict, dim3(nblk(b, 256)), dim3(256), 0, st, P, b, B.hrank.p, B.sub.p, dok);
    LAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(st));
    if (unique_out) *unique_out = heads;
    return DAPOL_OK;
}
// The range checks of b entities over the uploaded arena: ANDs of the heads' verdicts into dok[b]; *unique_out = heads = range proofs
// checked.  Returns with the stream drained, on every path: whatever was queued when an error came back has finished before the
// call's buffers are freed.
static int32_t verify_policy_compact_device(dapol_ctx* ctx, const SCompactPlan& P, const uint64_t* sub_off, size_t b, const uint64_t* dl, const uint32_t* dPC,
                                            const uint32_t* dR, int n_bits, const uint32_t* dseed, uint8_t* dok, uint64_t* unique_out) {
    VCompactBufs B;
    const int32_t rc = verify_policy_compact_queue(ctx, P, sub_off, b, dl, dPC, dR, n_bits, dseed, dok, unique_out, B);
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

int32_t dapol_verify_entities_compact(dapol_ctx* ctx, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* leaf_C32, const uint8_t* leaf_H32,
                                      size_t n_path_nodes, const uint8_t* path_C32, const uint8_t* path_H32, const uint8_t root_C32[32],
                                      const uint8_t root_H32[32], int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t* compact,
                                      size_t compact_len, const uint8_t verify_seed32[32], uint8_t* ok, uint64_t* unique_subproofs_out) {
    WIRE_SCOPE();
    if (!ctx || !root_C32 || !root_H32 || (b && (!leaf_idx || !leaf_C32 || !leaf_H32 || !path_C32 || !path_H32 || !compact || !ok)))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    VERIFY_SEED_OR_OS(verify_seed32)
    SCompactPlan P;
    int32_t rc = scompact_host_plan(height, b, leaf_idx, policy, aggregation_factor, n_bits, false, P);
    if (rc) return rc;
    uint32_t max_m = 1;
    for (uint32_t gi = 0; gi < P.V.n_groups; gi++) if (P.V.g[gi].m > max_m) max_m = P.V.g[gi].m;
    if (b && (int)max_m > ctx->max_parties) return fail(DAPOL_ERR_INVALID_ARGUMENT, "aggregation needs more parties than the context was created for");
    // a proof of the wrong shape is an invalid proof, never an over-read (dapol_verify_entities_checked)
    std::vector<uint64_t> sub_off(P.V.n_sub + 1);
    const uint64_t len = scompact_layout(P, b, leaf_idx, sub_off.data(), nullptr);
    if (n_path_nodes != b * (size_t)height || (uint64_t)compact_len != len) {
        for (size_t i = 0; i < b; i++) ok[i] = 0;
        if (unique_subproofs_out) *unique_subproofs_out = 0;
        return DAPOL_OK;
    }
    if (b == 0) {
        if (unique_subproofs_out) *unique_subproofs_out = 0;
        return DAPOL_OK;
    }
    // The latency regime (dapol_verify_entities_shared's): nothing to gain, the blobs are cut out on the host and take the existing path.
    size_t forward_max = VSHARED_FORWARD_MAX;
    if (const char* e = test_knob("DAPOL_VSHARED_FORWARD_MAX")) { long long v = atoll(e); if (v >= 0) forward_max = (size_t)v; }
    if (vshared_forwards(b, P.V.n_sub, forward_max)) {
        std::vector<uint8_t> blobs(b * (size_t)P.V.entity_pieces * 16);
        scompact_expand(P, b, leaf_idx, compact, 0, b, blobs.data());
        rc = dapol_verify_entities(ctx, height, b, leaf_idx, leaf_C32, leaf_H32, path_C32, path_H32, root_C32, root_H32, policy, aggregation_factor, n_bits,
                                   blobs.data(), verify_seed32, ok);
        if (rc) return rc;
        if (unique_subproofs_out) *unique_subproofs_out = (uint64_t)b * (uint64_t)P.V.n_sub;
        return DAPOL_OK;
    }
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    VerifyCallDev D;
    ForkGuard fg(ctx);
    rc = verify_upload_bytes_and_paths(ctx, fg, height, b, leaf_idx, leaf_C32, leaf_H32, path_C32, path_H32, root_C32, root_H32, (size_t)len, compact,
                                       verify_seed32, 0, D);
    if (rc) return rc;
    uint64_t unique = 0;
    rc = verify_policy_compact_device(ctx, P, sub_off.data(), b, D.dl, D.dPC, D.dR, n_bits, D.dseed, D.dok, &unique);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }        // (the path kernel: on st, or behind the guard)
    if (D.side_paths) { HIPCHK(hipStreamWaitEvent(st, ctx->ev_join[2], 0)); fg.joined(2); }
    hipLaunchKernelGGL(k_and_bytes, dim3(nblk(b, 256)), dim3(256), 0, st, b, D.dok, D.dpath);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpy(ok, D.dok, b, hipMemcpyDeviceToHost));
    if (unique_subproofs_out) *unique_subproofs_out = unique;
    return DAPOL_OK;
}

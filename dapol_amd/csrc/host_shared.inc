// dapol_prove_entities_shared / dapol_shared_plan: every distinct sub-proof statement of a call is proven once and written into the
// blob of every entity that contains it (the reference's generate_all_proofs DFS, src/dapol/mod.rs:216-314, with
// generate_proof_by_new_com / remove_proof_by_last_com, src/range/padding.rs:120-166, splitting.rs:131-178: the sub-proof over the
// upper siblings of a path is computed once for every leaf below that point).
//
// A sub-proof {start, count, m} of the plan over H siblings has the KEY DEPTH D = the largest depth below the root among its siblings
// (sibling i lies at depth i + 1 in root-first order, H - i in leaf-first order; the siblingless pad proof of aggregation 0 has D = 0),
// and an entity's SUBTREE KEY for it is S = its leaf index with the low H - D bits cleared: all siblings of the sub-proof are functions
// of S alone.  The proof's bytes are those of dapol_range_prove_batch over these parties with stream id S and slot base 0.

// shift[s] = H - D of sub-proof s under the call's sibling order (64: the key is 0 -- never used as a shift count)
static void shared_shifts(const std::vector<SubProof>& plan, int H, bool leaf_first, uint8_t* shift) {
    for (size_t s = 0; s < plan.size(); s++) {
        const int D = plan[s].count == 0 ? 0 : leaf_first ? H - plan[s].start : plan[s].start + plan[s].count;
        shift[s] = (uint8_t)(H - D);
    }
}
static inline uint64_t shared_key_host(uint64_t idx, unsigned shift) { return shift >= 64 ? 0ull : (idx >> shift) << shift; }
static bool strictly_increasing(size_t b, const uint64_t* idx) {
    for (size_t i = 1; i < b; i++) if (idx[i] <= idx[i - 1]) return false;
    return true;
}

int32_t dapol_shared_plan(int32_t height, size_t b, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor, uint64_t* n_unique_out,
                          uint64_t* total_unique, uint64_t* total_per_entity) {
    WIRE_SCOPE();
    if (b && !leaf_idx) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (height < 0 || height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    std::vector<SubProof> plan;
    if (!policy_plan(policy, height, aggregation_factor, plan)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad policy / aggregation_factor");
    if (!strictly_increasing(b, leaf_idx) || (b && height < 64 && (leaf_idx[b - 1] >> height) != 0))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "leaf indexes must be strictly increasing and below 2^height");
    std::vector<uint8_t> shift(plan.size());
    shared_shifts(plan, height, g_wire.siblings_leaf_first != 0, shift.data());
    uint64_t tot = 0;
    for (size_t s = 0; s < plan.size(); s++) {
        uint64_t u = b ? 1 : 0;
        for (size_t e = 1; e < b; e++) u += shared_key_host(leaf_idx[e], shift[s]) != shared_key_host(leaf_idx[e - 1], shift[s]);
        if (n_unique_out) n_unique_out[s] = u;
        tot += u;
    }
    if (total_unique) *total_unique = tot;
    if (total_per_entity) *total_per_entity = (uint64_t)b * (uint64_t)plan.size();
    return DAPOL_OK;
}

static int32_t inclusive_scan_u32(hipStream_t st, const uint32_t* in, uint32_t* out, size_t n) {
    size_t tmp = 0;
    HIPCHK(rocprim::inclusive_scan(nullptr, tmp, in, out, n, rocprim::plus<uint32_t>(), st));
    DevBuf<uint8_t> d;
    HIPCHK(d.alloc(tmp ? tmp : 1));
    HIPCHK(rocprim::inclusive_scan(d.p, tmp, in, out, n, rocprim::plus<uint32_t>(), st));
    HIPCHK(hipStreamSynchronize(st));                        // (the temporary storage goes at return)
    return DAPOL_OK;
}

// The plan as the kernels take it: key shifts, sibling spans, and the GROUPS (runs of equal m) with their places inside an entity's blob.
static int32_t shared_plan_dev_build(const std::vector<SubProof>& plan, size_t b, int H, int n_bits, SharedPlanDev& P) {
    if (plan.size() > SHARED_MAX_SUB || (uint64_t)b * (plan.size() + 1) >= (1ull << 32))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "too many sub-proofs in one call (entities x plan size must stay below 2^32)");
    P = SharedPlanDev{};
    P.n_sub = (uint32_t)plan.size(); P.H = (uint32_t)H;
    shared_shifts(plan, H, g_wire.siblings_leaf_first != 0, P.shift);
    uint32_t q = 0;
    for (size_t s = 0; s < plan.size(); s++) {
        P.start[s] = (uint8_t)plan[s].start; P.count[s] = (uint8_t)plan[s].count;
        const uint32_t pieces = (uint32_t)(dapol_range_proof_size(n_bits, plan[s].m) / 16);
        if (P.n_groups && P.g[P.n_groups - 1].m == (uint32_t)plan[s].m) P.g[P.n_groups - 1].k++;
        else {
            if (P.n_groups == SHARED_MAX_GROUPS) return fail(DAPOL_ERR_INVALID_ARGUMENT, "the plan has too many runs of equal-sized sub-proofs");
            SharedGroup& G = P.g[P.n_groups++];
            G.s0 = (uint32_t)s; G.k = 1; G.m = (uint32_t)plan[s].m; G.pieces = pieces; G.q0 = q;
        }
        q += pieces;
    }
    P.entity_pieces = q;
    return DAPOL_OK;
}

// What the shared call holds before its scatter: the plan as the kernels take it, the ranks, and the distinct proofs group after
// group -- which is the compact layout of shared_compact_plan.inc as it lies (words * 4 bytes).
struct SharedProved {
    SharedPlanDev P;
    DevBuf<uint32_t> flag, rank, proofs;
    size_t words = 0;
    uint64_t unique = 0;
};
// Everything of the shared call up to the scatter: heads, scan, gather, one call of the range prover per group.  pv / pr / pC are
// the gathered [b][H] siblings, d_idx the b ascending leaf indexes.  expect_heads (may be null): the head count that the host worked
// out from the indexes; another count on the device is an internal error, returned before anything is proven.
static int32_t prove_policy_shared_compact_device(dapol_ctx* ctx, const std::vector<SubProof>& plan, size_t b, int H, const uint64_t* pv, const uint32_t* pr,
                                                  const uint32_t* pC, int n_bits, const uint32_t* d_seed, const uint64_t* d_idx, const uint64_t* expect_heads,
                                                  SharedProved& R) {
    hipStream_t st = ctx->stream;
    SharedPlanDev& P = R.P;
    DevBuf<uint32_t>&flag = R.flag, &rank = R.rank, &proofs = R.proofs;
    int32_t rc = shared_plan_dev_build(plan, b, H, n_bits, P);
    if (rc) return rc;
    // heads and ranks: rank[s][e] = heads up to and including (s, e) in plan order, so rank - 1 is the compact row of the statement
    // that (s, e) belongs to -- its own if it is a head, its predecessors' otherwise; the last element (a closing zero flag) counts
    // all heads.  Row 0 of every sub-proof is a head: a group's first compact row is rank[s0][0] - 1.
    const size_t nf = (size_t)P.n_sub * b + 1;
    HIPCHK(flag.alloc(nf)); HIPCHK(rank.alloc(nf));
    hipLaunchKernelGGL(k_shared_heads, dim3(nblk(nf, 256)), dim3(256), 0, st, P, b, d_idx, flag.p);
    LAUNCH_CHECK();
    rc = inclusive_scan_u32(st, flag.p, rank.p, nf);
    if (rc) return rc;
    std::vector<uint32_t> g_first(P.n_groups + 1);           // compact row at which each group starts; the last one: all of them
    for (uint32_t gi = 0; gi <= P.n_groups; gi++) {
        const size_t at = gi < P.n_groups ? (size_t)P.g[gi].s0 * b : nf - 1;
        HIPCHK(hipMemcpyAsync(&g_first[gi], rank.p + at, 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t gi = 0; gi < P.n_groups; gi++) g_first[gi]--;
    R.unique = g_first[P.n_groups];
    if (expect_heads && *expect_heads != R.unique) return fail(DAPOL_ERR_HIP, "internal error: the device counts other heads than the host's layout");
    // compact gather: the head rows' parties, group after group
    size_t parties = 0, words = 0;
    std::vector<size_t> p_off(P.n_groups);
    for (uint32_t gi = 0; gi < P.n_groups; gi++) {
        const size_t U = g_first[gi + 1] - g_first[gi];
        p_off[gi] = parties; P.g[gi].word_off = words;
        parties += U * P.g[gi].m; words += U * (size_t)P.g[gi].pieces * 4;
    }
    R.words = words;
    DevBuf<uint64_t> vals, stream;
    DevBuf<uint32_t> blind, Vc;
    HIPCHK(vals.alloc(parties)); HIPCHK(blind.alloc(parties * 8)); HIPCHK(Vc.alloc(parties * 8)); HIPCHK(stream.alloc(g_first[P.n_groups]));
    HIPCHK(proofs.alloc(words));
    const uint32_t* Bb_comp = ctx->gens_comp.p + (size_t)ctx->tv.row_Bb(0) * 8;
    for (uint32_t gi = 0; gi < P.n_groups; gi++) {
        const SharedGroup& G = P.g[gi];
        hipLaunchKernelGGL(k_shared_gather, dim3(nblk(b * (size_t)G.k * (size_t)G.m, 256)), dim3(256), 0, st, P, gi, b, d_idx, flag.p, rank.p, pv, pr, pC,
                           Bb_comp, vals.p + p_off[gi], blind.p + p_off[gi] * 8, Vc.p + p_off[gi] * 8, stream.p + g_first[gi]);
        LAUNCH_CHECK();
    }
    // one call of the range prover per group: a stream id per row, slot base 0.  One after the other, as prove_policy_device's
    // sequential branch: each call returns after its kernels have drained, so an error return frees nothing that is still in use.
    for (uint32_t gi = 0; gi < P.n_groups; gi++) {
        const SharedGroup& G = P.g[gi];
        rc = range_prove_device(ctx, n_bits, (int)G.m, g_first[gi + 1] - g_first[gi], vals.p + p_off[gi], blind.p + p_off[gi] * 8, Vc.p + p_off[gi] * 8, d_seed,
                                stream.p + g_first[gi], 0, nullptr, proofs.p + G.word_off, nullptr);
        if (rc) return rc;
    }
    return DAPOL_OK;
}
// The shared counterpart of prove_policy_device: the compact proofs, then the scatter into the [b] blobs of d_range.
static int32_t prove_policy_shared_device(dapol_ctx* ctx, const std::vector<SubProof>& plan, size_t b, int H, const uint64_t* pv, const uint32_t* pr,
                                          const uint32_t* pC, int n_bits, const uint32_t* d_seed, const uint64_t* d_idx, uint32_t* d_range,
                                          uint64_t* unique_out) {
    hipStream_t st = ctx->stream;
    SharedProved R;
    int32_t rc = prove_policy_shared_compact_device(ctx, plan, b, H, pv, pr, pC, n_bits, d_seed, d_idx, nullptr, R);
    if (rc) return rc;
    if (unique_out) *unique_out = R.unique;
    // scatter: every (entity, sub-proof) copies its proof from its compact row
    hipLaunchKernelGGL(k_shared_scatter, dim3(nblk(b * (size_t)R.P.entity_pieces, 256)), dim3(256), 0, st, R.P, b, R.rank.p, (const uint4*)R.proofs.p, (uint4*)d_range);
    LAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(st));
    return DAPOL_OK;
}

int32_t dapol_prove_entities_shared(dapol_ctx* ctx, dapol_tree* tree, size_t b, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor,
                                    int32_t n_bits, const uint8_t nonce_seed32[32], int32_t n_upper, const uint8_t* up_C32, const uint8_t* up_H32,
                                    const uint64_t* up_v, const uint8_t* up_r32, uint8_t* path_C32, uint8_t* path_H32, uint8_t* range_out,
                                    uint64_t* unique_subproofs_out) {
    WIRE_SCOPE();
    EntityShape S;
    int32_t rc = entity_shape(ctx, tree, nonce_seed32 && (!b || (leaf_idx && range_out)), "null or out-of-range argument", n_upper, policy, aggregation_factor,
                              n_bits, true, true, S);
    if (rc) return rc;
    if (!strictly_increasing(b, leaf_idx)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "leaf indexes must be strictly increasing");
    uint64_t unique = 0;
    if (b) {
        EntityProveCall call;
        if ((rc = call.open(ctx, tree, S, b, leaf_idx, nonce_seed32, n_upper, up_C32, up_H32, up_v, up_r32)) || (rc = call.paths())) return rc;
        rc = prove_policy_shared_device(ctx, S.plan, b, S.H, call.pv.p, call.pr.p, call.pathC.p, n_bits, call.seed.p, call.idx.p, call.out.p, &unique);
        if (rc || (rc = call.download(path_C32, path_H32, range_out))) return rc;
    }
    if (unique_subproofs_out) *unique_subproofs_out = unique;
    return DAPOL_OK;
}

// ------------------------------------------------------------------------------------------------ the compact form
// dapol_shared_compact_plan / _expand / _compress: host-only (shared_compact_plan.inc).  The refusals of dapol_shared_plan plus n_bits.
static int32_t scompact_host_plan(int32_t height, size_t b, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor, int32_t n_bits,
                                  bool check_range, SCompactPlan& P) {
    if (b && !leaf_idx) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (height < 0 || height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    std::vector<SubProof> plan;
    if (!policy_plan(policy, height, aggregation_factor, plan)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad policy / aggregation_factor");
    if (dapol_range_proof_size(n_bits, 1) == 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad n_bits");
    if (!strictly_increasing(b, leaf_idx) || (check_range && b && height < 64 && (leaf_idx[b - 1] >> height) != 0))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "leaf indexes must be strictly increasing and below 2^height");
    if (scompact_plan_build(plan, height, n_bits, g_wire.siblings_leaf_first != 0, P))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "the plan has too many sub-proofs or runs of equal-sized sub-proofs");
    if (!vshared_call_fits(b, plan.size()))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "too many sub-proofs in one call (entities x (plan size + 1) must stay below 2^32)");
    return DAPOL_OK;
}
int32_t dapol_shared_compact_plan(int32_t height, size_t b, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor, int32_t n_bits,
                                  uint64_t* sub_off, uint32_t* ref, uint64_t* compact_len) {
    WIRE_SCOPE();
    SCompactPlan P;
    int32_t rc = scompact_host_plan(height, b, leaf_idx, policy, aggregation_factor, n_bits, true, P);
    if (rc) return rc;
    const uint64_t len = scompact_layout(P, b, leaf_idx, sub_off, ref);
    if (compact_len) *compact_len = len;
    return DAPOL_OK;
}
int32_t dapol_shared_expand(int32_t height, size_t b, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor, int32_t n_bits,
                            const uint8_t* compact, size_t compact_len, size_t first, size_t count, uint8_t* range_out) {
    WIRE_SCOPE();
    SCompactPlan P;
    int32_t rc = scompact_host_plan(height, b, leaf_idx, policy, aggregation_factor, n_bits, true, P);
    if (rc) return rc;
    if (first > b || count > b - first) return fail(DAPOL_ERR_INVALID_ARGUMENT, "first + count exceeds the rows");
    if (scompact_layout(P, b, leaf_idx, nullptr, nullptr) != (uint64_t)compact_len)
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "compact_len is not the length of the compact layout of these leaves");
    if (count && (!compact || !range_out)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (count) scompact_expand(P, b, leaf_idx, compact, first, count, range_out);
    return DAPOL_OK;
}
int32_t dapol_shared_compress(int32_t height, size_t b, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor, int32_t n_bits,
                              const uint8_t* range_blobs, uint8_t* compact_out, size_t compact_cap, uint64_t* compact_len_out) {
    WIRE_SCOPE();
    SCompactPlan P;
    int32_t rc = scompact_host_plan(height, b, leaf_idx, policy, aggregation_factor, n_bits, true, P);
    if (rc) return rc;
    const uint64_t len = scompact_layout(P, b, leaf_idx, nullptr, nullptr);
    if (len > (uint64_t)compact_cap) return fail(DAPOL_ERR_INVALID_ARGUMENT, "compact_cap is below the length of the compact layout");
    if (b && (!range_blobs || !compact_out)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (b) scompact_compress(P, b, leaf_idx, range_blobs, compact_out);
    if (compact_len_out) *compact_len_out = len;
    return DAPOL_OK;
}

// dapol_prove_entities_shared without its scatter: the distinct proofs leave the device as they lie.  No [b][entity bytes] buffer
// exists on the device in this call.
int32_t dapol_prove_entities_shared_compact(dapol_ctx* ctx, dapol_tree* tree, size_t b, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor,
                                            int32_t n_bits, const uint8_t nonce_seed32[32], int32_t n_upper, const uint8_t* up_C32, const uint8_t* up_H32,
                                            const uint64_t* up_v, const uint8_t* up_r32, uint8_t* path_C32, uint8_t* path_H32, uint8_t* compact_out,
                                            size_t compact_cap, uint64_t* compact_len_out, uint64_t* unique_subproofs_out) {
    WIRE_SCOPE();
    EntityShape S;
    int32_t rc = entity_shape(ctx, tree, nonce_seed32 && (!b || (leaf_idx && compact_out)), "null or out-of-range argument", n_upper, policy, aggregation_factor,
                              n_bits, true, true, S);
    if (rc) return rc;
    if (!strictly_increasing(b, leaf_idx)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "leaf indexes must be strictly increasing");
    // the layout from the indexes alone, before anything is queued (an index outside the tree is the unknown leaf of paths() below)
    SCompactPlan P;
    if ((rc = scompact_host_plan(S.H, b, leaf_idx, policy, aggregation_factor, n_bits, false, P))) return rc;
    std::vector<uint64_t> sub_off(P.V.n_sub + 1);
    const uint64_t len = scompact_layout(P, b, leaf_idx, sub_off.data(), nullptr);
    if (len > (uint64_t)compact_cap) return fail(DAPOL_ERR_INVALID_ARGUMENT, "compact_cap is below the length of the compact layout");
    uint64_t heads = 0;
    for (uint32_t s = 0; s < P.V.n_sub; s++) heads += (sub_off[s + 1] - sub_off[s]) / ((uint64_t)P.V.pieces[s] * 16);
    if (b) {
        EntityProveCall call;
        if ((rc = call.open(ctx, tree, S, b, leaf_idx, nonce_seed32, n_upper, up_C32, up_H32, up_v, up_r32, false)) || (rc = call.paths())) return rc;
        SharedProved R;
        rc = prove_policy_shared_compact_device(ctx, S.plan, b, S.H, call.pv.p, call.pr.p, call.pathC.p, n_bits, call.seed.p, call.idx.p, &heads, R);
        if (rc) return rc;
        if ((uint64_t)R.words * 4 != len) return fail(DAPOL_ERR_HIP, "internal error: the device's compact buffer has another length than the host's layout");
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if ((rc = call.download(path_C32, path_H32, nullptr))) return rc;
        HIPCHK(hipMemcpy(compact_out, R.proofs.p, (size_t)len, hipMemcpyDeviceToHost));
    }
    if (compact_len_out) *compact_len_out = len;
    if (unique_subproofs_out) *unique_subproofs_out = heads;
    return DAPOL_OK;
}

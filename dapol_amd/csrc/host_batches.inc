// Many multi-leaf inclusion proofs in one call: dapol_batches_plan (host only), dapol_prove_batches, dapol_verify_batches
// (kernels_batches.h).  Per batch the outputs and verdicts are dapol_prove_batch's and dapol_verify_batch_checked's (host_batch.inc),
// byte for byte; what changes is the shape of the work.  A batch with S deduplicated siblings is proved by the policy prover over
// H := S siblings, so the batches of a call with EQUAL S share one plan: they are the rows of one [b_S][S] call -- an S-GROUP -- and the
// grouped sub-proofs, the lanes and the sweep serve them as they serve entities.  The S-groups of a call run one after the other.
// Included from dapol_hip.hip after host_batch.inc.

static int32_t fail_batch(int32_t code, size_t j, const char* msg) {
    char buf[256];
    snprintf(buf, sizeof buf, "batch %zu: %s", j, msg);
    g_last_error = buf;
    return code;
}

// What one S asks of the policy: dapol_prove_batch's refusals after the leaf indexes, in its order (max_parties = 0: no context to ask).
struct BatchesShape { int32_t code = DAPOL_OK; const char* msg = nullptr; size_t words = 0; int max_m = 1; std::vector<SubProof> plan; };
static BatchesShape batches_shape(size_t S, int policy, int agg, int n_bits, int max_parties) {
    BatchesShape R;
    auto refuse = [&](const char* m) { R.code = DAPOL_ERR_INVALID_ARGUMENT; R.msg = m; return R; };
    if (S > (size_t)1 << 20) return refuse("batch too large");
    if (!policy_plan(policy, (int)S, agg, R.plan)) return refuse("aggregation_factor must be within [0, number of siblings]");
    if (dapol_range_proof_size(n_bits, 1) == 0) return refuse("n_bits must be 8/16/32/64");
    for (auto& s : R.plan) {
        if (max_parties && s.m > max_parties) return refuse("aggregation needs more parties than the context was created for");
        if (s.m > R.max_m) R.max_m = s.m;
        R.words += dapol_range_proof_size(n_bits, s.m) / 4;
    }
    return R;
}

// The call as the host sees it: every batch's siblings (caller order), the offsets of the outputs, and the S-groups in ascending S.
struct BatchesPlan {
    std::vector<BatchSib> sibs;                      // [sib_off[nb]]; src_leaf counts within the batch
    std::vector<uint64_t> sib_off, range_off;        // [nb + 1]: sibling records, bytes
    std::vector<uint32_t> group_of;                  // [nb]
    std::vector<size_t> group_S;                     // [n_groups], ascending
    std::vector<BatchesShape> shape;                 // [n_groups]
};
static int32_t batches_offsets_ok(size_t nb, const uint64_t* off) {
    if (off[0] != 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "batch_off[0] must be 0");
    for (size_t j = 0; j < nb; j++)
        if (off[j + 1] < off[j]) return fail(DAPOL_ERR_INVALID_ARGUMENT, "batch_off must not decrease");
    return DAPOL_OK;
}
static int32_t batches_plan_host(int height, size_t nb, const uint64_t* off, const uint64_t* leaf, int policy, int agg, int n_bits, int max_parties,
                                 bool keep_sibs, BatchesPlan& P) {
    RCCHK(batches_offsets_ok(nb, off));
    if (height > 0 && off[nb] > 0xffffffffull / (uint64_t)height)
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "too many leaves in one call (leaves x height must stay below 2^32)");
    if (off[nb] && !leaf) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    P = BatchesPlan{};
    P.sib_off.assign(nb + 1, 0); P.range_off.assign(nb + 1, 0); P.group_of.assign(nb, 0);
    std::vector<size_t> S_of(nb);
    std::vector<std::pair<size_t, BatchesShape>> seen;               // shapes by S, ascending
    std::vector<BatchSib> sibs;
    for (size_t j = 0; j < nb; j++) {
        if (!batch_plan(height, (size_t)(off[j + 1] - off[j]), leaf + off[j], sibs))
            return fail_batch(DAPOL_ERR_INVALID_ARGUMENT, j, "leaf indexes must be non-empty, strictly increasing and below 2^height");
        const size_t S = sibs.size();
        auto it = std::lower_bound(seen.begin(), seen.end(), S, [](const std::pair<size_t, BatchesShape>& a, size_t s) { return a.first < s; });
        if (it == seen.end() || it->first != S) it = seen.insert(it, {S, batches_shape(S, policy, agg, n_bits, max_parties)});
        if (it->second.code) return fail_batch(it->second.code, j, it->second.msg);
        S_of[j] = S;
        P.sib_off[j + 1] = P.sib_off[j] + S;
        P.range_off[j + 1] = P.range_off[j] + it->second.words * 4;
        if (keep_sibs) P.sibs.insert(P.sibs.end(), sibs.begin(), sibs.end());
    }
    for (auto& s : seen) { P.group_S.push_back(s.first); P.shape.push_back(std::move(s.second)); }
    for (size_t j = 0; j < nb; j++) P.group_of[j] = (uint32_t)(std::lower_bound(P.group_S.begin(), P.group_S.end(), S_of[j]) - P.group_S.begin());
    return DAPOL_OK;
}

int32_t dapol_batches_plan(int32_t height, size_t nb, const uint64_t* batch_off, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor,
                           int32_t n_bits, uint64_t* n_siblings, uint64_t* sib_off, uint64_t* range_off, uint64_t* n_groups) {
    WIRE_SCOPE();
    if (!batch_off) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (height < 0 || height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    BatchesPlan P;
    RCCHK(batches_plan_host(height, nb, batch_off, leaf_idx, policy, aggregation_factor, n_bits, 0, false, P));
    for (size_t j = 0; j <= nb; j++) {
        if (n_siblings && j < nb) n_siblings[j] = P.sib_off[j + 1] - P.sib_off[j];
        if (sib_off) sib_off[j] = P.sib_off[j];
        if (range_off) range_off[j] = P.range_off[j];
    }
    if (n_groups) *n_groups = P.group_S.size();
    return DAPOL_OK;
}

// Where the rows of the S-groups live: group g's rows are [row0[g], row0[g + 1]) of every group-ordered array, its sibling records
// start at sib0[g], its range words at word0[g]; pos[j] is batch j's row (caller order within the group).
struct BatchesGroups {
    std::vector<size_t> row0, sib0, word0;          // [n_groups + 1]
    std::vector<uint32_t> pos;                      // [nb]; ~0 for a batch that is no row (the verifier's malformed ones)
};
static BatchesGroups batches_groups(const BatchesPlan& P, size_t nb, const std::vector<uint8_t>* is_row = nullptr) {
    const size_t ng = P.group_S.size();
    BatchesGroups G;
    G.row0.assign(ng + 1, 0); G.sib0.assign(ng + 1, 0); G.word0.assign(ng + 1, 0); G.pos.assign(nb, 0xffffffffu);
    for (size_t j = 0; j < nb; j++)
        if (!is_row || (*is_row)[j]) G.row0[P.group_of[j] + 1]++;
    for (size_t g = 0; g < ng; g++) {
        const size_t rows = G.row0[g + 1];
        G.row0[g + 1] = G.row0[g] + rows;
        G.sib0[g + 1] = G.sib0[g] + rows * P.group_S[g];
        G.word0[g + 1] = G.word0[g] + rows * P.shape[g].words;
    }
    std::vector<size_t> next(G.row0.begin(), G.row0.end() - 1);
    for (size_t j = 0; j < nb; j++)
        if (!is_row || (*is_row)[j]) G.pos[j] = (uint32_t)next[P.group_of[j]]++;
    return G;
}

struct StreamDrain { hipStream_t s; ~StreamDrain() { (void)hipStreamSynchronize(s); } };      // declared after a call's buffers: nothing is freed while the stream runs

static int32_t batches_move(hipStream_t st, size_t records, size_t rows, uint32_t unit, const uint64_t* d_dst_off, const uint64_t* d_src_off, const void* src,
                            void* dst) {
    if (!records) return DAPOL_OK;
    hipLaunchKernelGGL(k_batches_scatter, dim3(nblk(records * unit, 256)), dim3(256), 0, st, records * unit, rows, unit, d_dst_off, d_src_off, (const uint4*)src,
                       (uint4*)dst);
    LAUNCH_CHECK();
    return DAPOL_OK;
}

int32_t dapol_prove_batches(dapol_ctx* ctx, dapol_tree* tree, size_t nb, const uint64_t* batch_off, const uint64_t* leaf_idx, int32_t policy,
                            int32_t aggregation_factor, int32_t n_bits, const uint8_t nonce_seed32[32], uint8_t* sib_C32, uint8_t* sib_H32, uint8_t* range_out,
                            uint64_t* n_groups_out) {
    WIRE_SCOPE();
    if (!ctx || !tree || tree->ctx != ctx || !nonce_seed32 || !batch_off) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (tree->shard_bits) return fail(DAPOL_ERR_INVALID_ARGUMENT, "batched proofs need the whole tree (not a shard)");
    TREE_USABLE(tree);
    NEEDS_32_BYTE_DIGEST(ctx, "dapol_prove_batches");
    const int H = tree->height;
    BatchesPlan P;
    RCCHK(batches_plan_host(H, nb, batch_off, leaf_idx, policy, aggregation_factor, n_bits, ctx->max_parties, true, P));
    const size_t ng = P.group_S.size(), K = (size_t)batch_off[nb], T = (size_t)P.sib_off[nb], R = (size_t)P.range_off[nb] / 4;
    if (R && !range_out) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (nb == 0) {
        if (n_groups_out) *n_groups_out = 0;
        return DAPOL_OK;
    }
    const BatchesGroups G = batches_groups(P, nb);
    // host plan of the moves: where every sibling record comes from, where every batch's rows sit in group order
    std::vector<uint32_t> src(T);
    std::vector<uint64_t> sib_src(nb), rng_dst(nb + 1), rng_src(nb);
    const bool leaf_first = g_wire.siblings_leaf_first != 0;
    for (size_t j = 0; j < nb; j++) {
        const size_t g = P.group_of[j], S = P.group_S[g], row = G.pos[j] - G.row0[g];
        sib_src[j] = G.sib0[g] + row * S;
        rng_src[j] = (G.word0[g] + row * P.shape[g].words) / 4;
        rng_dst[j + 1] = P.range_off[j + 1] / 16;
        const BatchSib* sb = P.sibs.data() + P.sib_off[j];
        for (size_t i = 0; i < S; i++)
            src[sib_src[j] + i] = (uint32_t)(((size_t)batch_off[j] + sb[i].src_leaf) * (size_t)H + (size_t)(leaf_first ? sb[i].level : H - 1 - sb[i].level));
    }
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<uint64_t> dl, doff, pv, gv, dstream, dsib_dst, dsib_src, drng_dst, drng_src;
    DevBuf<uint32_t> dseed, seeds, dpos, dleafpos, pC, pH, pr, gC, gH, gr, dsrc, grange, oC, oH, orange;
    StreamDrain drain{st};
    HIPCHK(dl.alloc(K)); HIPCHK(doff.alloc(nb + 1)); HIPCHK(dseed.alloc(8)); HIPCHK(seeds.alloc(nb * 8)); HIPCHK(dstream.alloc(nb)); HIPCHK(dpos.alloc(nb));
    HIPCHK(dleafpos.alloc(K));
    const size_t tot = K * (size_t)H;
    HIPCHK(pC.alloc(tot * 8 + 8)); HIPCHK(pH.alloc(tot * 8 + 8)); HIPCHK(pr.alloc(tot * 8 + 8)); HIPCHK(pv.alloc(tot + 1));
    HIPCHK(gC.alloc(T * 8 + 8)); HIPCHK(gH.alloc(T * 8 + 8)); HIPCHK(gr.alloc(T * 8 + 8)); HIPCHK(gv.alloc(T + 1)); HIPCHK(dsrc.alloc(T + 1));
    HIPCHK(grange.alloc(R + 4)); HIPCHK(orange.alloc(R + 4)); HIPCHK(oC.alloc(T * 8 + 8)); HIPCHK(oH.alloc(T * 8 + 8));
    HIPCHK(dsib_dst.alloc(nb + 1)); HIPCHK(dsib_src.alloc(nb)); HIPCHK(drng_dst.alloc(nb + 1)); HIPCHK(drng_src.alloc(nb));
    HIPCHK(hipMemcpyAsync(dl.p, leaf_idx, K * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(doff.p, batch_off, (nb + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dseed.p, nonce_seed32, 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dpos.p, G.pos.data(), nb * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dsib_dst.p, P.sib_off.data(), (nb + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dsib_src.p, sib_src.data(), nb * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(drng_dst.p, rng_dst.data(), (nb + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(drng_src.p, rng_src.data(), nb * 8, hipMemcpyHostToDevice, st));
    if (T) HIPCHK(hipMemcpyAsync(dsrc.p, src.data(), T * 4, hipMemcpyHostToDevice, st));
    PathOut po{pC.p, pH.p, pv.p, pr.p}, go{gC.p, gH.p, gv.p, gr.p};
    RCCHK(tree_paths_device(tree, K, dl.p, po, dleafpos.p));                  // (an unknown leaf ends the call here: nothing written)
    hipLaunchKernelGGL(k_batches_seed, dim3(nblk(nb, 64)), dim3(64), 0, st, nb, dseed.p, doff.p, dl.p, dpos.p, seeds.p, dstream.p);
    LAUNCH_CHECK();
    if (T) {
        hipLaunchKernelGGL(k_batches_gather, dim3(nblk(T, 256)), dim3(256), 0, st, T, dsrc.p, po, go);
        LAUNCH_CHECK();
    }
    for (size_t g = 0; g < ng; g++) {                                          // one policy call per S-group, its real row count
        const size_t rows = G.row0[g + 1] - G.row0[g], s0 = G.sib0[g];
        RCCHK(prove_policy_device(ctx, P.shape[g].plan, rows, (int)P.group_S[g], gv.p + s0, gr.p + s0 * 8, gC.p + s0 * 8, n_bits, seeds.p + G.row0[g] * 8,
                                  dstream.p + G.row0[g], grange.p + G.word0[g], nullptr, nullptr, 0, 8));
    }
    RCCHK(batches_move(st, R / 4, nb, 1, drng_dst.p, drng_src.p, grange.p, orange.p));
    if (sib_C32) RCCHK(batches_move(st, T, nb, 2, dsib_dst.p, dsib_src.p, gC.p, oC.p));
    if (sib_H32) RCCHK(batches_move(st, T, nb, 2, dsib_dst.p, dsib_src.p, gH.p, oH.p));
    if (R) HIPCHK(hipMemcpyAsync(range_out, orange.p, R * 4, hipMemcpyDeviceToHost, st));
    if (sib_C32 && T) HIPCHK(hipMemcpyAsync(sib_C32, oC.p, T * 32, hipMemcpyDeviceToHost, st));
    if (sib_H32 && T) HIPCHK(hipMemcpyAsync(sib_H32, oH.p, T * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_groups_out) *n_groups_out = ng;
    return DAPOL_OK;
}

// dapol_verify_batches as the host plans it (nb > 0, offsets validated): which batches are well-formed, their S-groups, the merge
// operations level by level over an arena of K leaf slots, Tc sibling slots and the merged nodes, and the moves into group order.
// range_proofs is read only where a malformed batch leaves the blobs behind it off the 16-byte grid (`staged`).
struct VerifyBatchesPlan {
    BatchesPlan P;
    BatchesGroups G;
    size_t K = 0, Tc = 0, Rc = 0, W = 0, T = 0, R = 0, slots = 0, v_words = 8;      // W, T, R: rows, sibling records, range words of the well-formed batches
    std::vector<BatchesMergeOp> ops;
    std::vector<size_t> level_end;
    std::vector<uint32_t> root_slot;
    std::vector<uint64_t> sibm_dst, sibm_src, rngm_dst, rngm_src;
    bool aligned = true;
    std::vector<uint8_t> staged;
};
static int32_t verify_batches_plan(dapol_ctx* ctx, int32_t height, size_t nb, const uint64_t* batch_off, const uint64_t* leaf_idx, const uint64_t* sib_off,
                                   int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint64_t* range_off, const uint8_t* range_proofs,
                                   VerifyBatchesPlan& V) {
    const size_t K = (size_t)batch_off[nb], Tc = (size_t)(sib_off[nb] - sib_off[0]), Rc = (size_t)(range_off[nb] - range_off[0]);
    // Batch by batch what dapol_verify_batch_checked decides before it touches the GPU: a batch whose counts are not those of its
    // leaves is an invalid proof (no row of any group); bad leaf indexes, or more parties than the context has, end the call.
    BatchesPlan& P = V.P;
    std::vector<uint8_t> well(nb, 0);
    std::vector<size_t> S_of(nb, 0);
    {
        std::vector<std::pair<size_t, BatchesShape>> seen;
        std::vector<BatchSib> sibs;
        P.sib_off.assign(nb + 1, 0); P.group_of.assign(nb, 0);
        for (size_t j = 0; j < nb; j++) {
            const uint64_t ns = sib_off[j + 1] - sib_off[j], rl = range_off[j + 1] - range_off[j];
            P.sib_off[j + 1] = P.sib_off[j];
            if (ns > 0x7fffffffu) continue;
            const size_t es = dapol_entity_proof_size((int32_t)ns, policy, aggregation_factor, n_bits);
            if (es == 0 || rl != es) continue;
            if (!batch_plan(height, (size_t)(batch_off[j + 1] - batch_off[j]), leaf_idx + batch_off[j], sibs))
                return fail_batch(DAPOL_ERR_INVALID_ARGUMENT, j, "leaf indexes must be non-empty, strictly increasing and below 2^height");
            const size_t S = sibs.size();
            if (S != ns) continue;
            auto it = std::lower_bound(seen.begin(), seen.end(), S, [](const std::pair<size_t, BatchesShape>& a, size_t s) { return a.first < s; });
            if (it == seen.end() || it->first != S) it = seen.insert(it, {S, batches_shape(S, policy, aggregation_factor, n_bits, ctx->max_parties)});
            if (it->second.code) return fail_batch(it->second.code, j, it->second.msg);
            well[j] = 1; S_of[j] = S;
            P.sib_off[j + 1] += S;
            P.sibs.insert(P.sibs.end(), sibs.begin(), sibs.end());
        }
        for (auto& s : seen) { P.group_S.push_back(s.first); P.shape.push_back(std::move(s.second)); }
        for (size_t j = 0; j < nb; j++)
            if (well[j]) P.group_of[j] = (uint32_t)(std::lower_bound(P.group_S.begin(), P.group_S.end(), S_of[j]) - P.group_S.begin());
    }
    const size_t ng = P.group_S.size();
    V.G = batches_groups(P, nb, &well);
    const BatchesGroups& G = V.G;
    const size_t W = G.row0[ng], T = G.sib0[ng], R = G.word0[ng];
    // Arena slots: the caller's leaves [0, K), the caller's siblings [K, K + Tc), then the merged nodes.  The operations of all
    // well-formed batches, level by level.
    size_t merges = 0;
    for (size_t j = 0; j < nb; j++)
        if (well[j]) merges += (size_t)(batch_off[j + 1] - batch_off[j]) * (size_t)height;      // (an upper bound: one merge per leaf and level)
    if ((uint64_t)K + Tc + merges >= 0xffffffffull) return fail(DAPOL_ERR_INVALID_ARGUMENT, "too many nodes in one call (leaves x height must stay below 2^32)");
    std::vector<std::vector<BatchesMergeOp>> level_ops((size_t)height);
    std::vector<BatchesMergeOp>& ops = V.ops;
    std::vector<size_t>& level_end = V.level_end;
    std::vector<uint32_t>& root_slot = V.root_slot;
    std::vector<uint64_t>&sibm_dst = V.sibm_dst, &sibm_src = V.sibm_src, &rngm_dst = V.rngm_dst, &rngm_src = V.rngm_src;
    bool& aligned = V.aligned;
    std::vector<uint8_t>& staged = V.staged;
    ops.clear(); level_end.clear();
    root_slot.assign(nb, 0xffffffffu);
    uint32_t next_slot = (uint32_t)(K + Tc);
    for (size_t j = 0; j < nb; j++) {
        if (!well[j]) continue;
        root_slot[j] = batch_merge_schedule(height, (size_t)(batch_off[j + 1] - batch_off[j]), leaf_idx + batch_off[j], S_of[j], P.sibs.data() + P.sib_off[j],
                                            (uint32_t)batch_off[j], (uint32_t)(K + (sib_off[j] - sib_off[0])), next_slot,
                                            [&](int L, uint32_t left, uint32_t right, uint32_t dst) { level_ops[L].push_back({left, right, dst, (uint32_t)j}); });
    }
    for (auto& lv : level_ops) { ops.insert(ops.end(), lv.begin(), lv.end()); level_end.push_back(ops.size()); }
    // The moves into group order: row r = the r-th well-formed batch in (group, caller) order.  A malformed batch may leave the blobs
    // behind it at any byte offset; the pieces are 16 bytes, so such a call stages its well-formed blobs on the host first.
    const uint8_t* rbase = range_proofs ? range_proofs + range_off[0] : nullptr;
    aligned = true;
    for (size_t j = 0; j < nb; j++)
        if (well[j] && (range_off[j] - range_off[0]) % 16) aligned = false;
    staged.clear();
    sibm_dst.assign(W + 1, 0); sibm_src.assign(W, 0); rngm_dst.assign(W + 1, 0); rngm_src.assign(W, 0);
    size_t staged_at = 0;
    if (!aligned) staged.resize(R * 4);
    for (size_t j = 0; j < nb; j++) {
        if (!well[j]) continue;
        const size_t r = G.pos[j], g = P.group_of[j], bytes = P.shape[g].words * 4;
        sibm_src[r] = K + (sib_off[j] - sib_off[0]);
        if (aligned) rngm_src[r] = (range_off[j] - range_off[0]) / 16;
        else {
            if (bytes) memcpy(staged.data() + staged_at, rbase + (range_off[j] - range_off[0]), bytes);
            rngm_src[r] = staged_at / 16;
            staged_at += bytes;
        }
    }
    for (size_t g = 0; g < ng; g++)
        for (size_t r = G.row0[g]; r < G.row0[g + 1]; r++) {
            sibm_dst[r + 1] = sibm_dst[r] + P.group_S[g];
            rngm_dst[r + 1] = rngm_dst[r] + P.shape[g].words / 4;
        }
    V.v_words = 8;                                                            // verify_policy_device's [rows][max m][8] scratch, the largest group's
    for (size_t g = 0; g < ng; g++) V.v_words = std::max(V.v_words, (G.row0[g + 1] - G.row0[g]) * (size_t)P.shape[g].max_m * 8);
    V.K = K; V.Tc = Tc; V.Rc = Rc; V.W = W; V.T = T; V.R = R; V.slots = next_slot;
    return DAPOL_OK;
}

// The device core of dapol_verify_batches over an arena that is ON THE DEVICE already: aC / aH [V.slots + 1][8] words hold the leaves'
// commitments and hashes in slots [0, K) and the siblings in [K, K + Tc), the merged nodes are written behind them; dR = the range
// bytes (the caller's, or V.staged where the plan staged them), droot = the root's C [8] then H [8], dseed [8]; d_ok [nb] receives the
// verdicts.  Everything runs on the context's stream; the caller drains it before its buffers go.
static int32_t verify_batches_device(dapol_ctx* ctx, const VerifyBatchesPlan& V, size_t nb, int32_t n_bits, uint32_t* aC, uint32_t* aH, const uint32_t* dR,
                                     const uint32_t* droot, const uint32_t* dseed, uint8_t* d_ok) {
    const BatchesPlan& P = V.P;
    const BatchesGroups& G = V.G;
    const size_t ng = P.group_S.size(), W = V.W, T = V.T, R = V.R;
    const std::vector<BatchesMergeOp>& ops = V.ops;
    const std::vector<size_t>& level_end = V.level_end;
    hipStream_t st = ctx->stream;
    DevBuf<uint32_t> gPC, gR, dV, droot_slot, dpos;
    DevBuf<BatchesMergeOp> dops;
    DevBuf<uint8_t> bad, rok, dsub;
    DevBuf<uint64_t> dsibm_dst, dsibm_src, drngm_dst, drngm_src;
    StreamDrain drain{st};
    HIPCHK(gPC.alloc(T * 8 + 8)); HIPCHK(gR.alloc(R + 8)); HIPCHK(dV.alloc(V.v_words)); HIPCHK(droot_slot.alloc(nb)); HIPCHK(dpos.alloc(nb));
    HIPCHK(dops.alloc(ops.size() + 1)); HIPCHK(bad.alloc(nb)); HIPCHK(rok.alloc(W + 1)); HIPCHK(dsub.alloc(W + 1));
    HIPCHK(dsibm_dst.alloc(W + 1)); HIPCHK(dsibm_src.alloc(W + 1)); HIPCHK(drngm_dst.alloc(W + 1)); HIPCHK(drngm_src.alloc(W + 1));
    HIPCHK(hipMemsetAsync(bad.p, 0, nb, st));
    HIPCHK(hipMemsetAsync(rok.p, 1, W + 1, st));
    if (!ops.empty()) HIPCHK(hipMemcpyAsync(dops.p, ops.data(), ops.size() * sizeof(BatchesMergeOp), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(droot_slot.p, V.root_slot.data(), nb * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dpos.p, G.pos.data(), nb * 4, hipMemcpyHostToDevice, st));
    if (W) {
        HIPCHK(hipMemcpyAsync(dsibm_dst.p, V.sibm_dst.data(), (W + 1) * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dsibm_src.p, V.sibm_src.data(), W * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(drngm_dst.p, V.rngm_dst.data(), (W + 1) * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(drngm_src.p, V.rngm_src.data(), W * 8, hipMemcpyHostToDevice, st));
    }
    size_t done = 0;
    for (size_t lv = 0; lv < level_end.size(); lv++) {                         // one launch per level over ALL batches
        const size_t n = level_end[lv] - done;
        if (!n) continue;
        LAUNCH_DX(ctx->tv.digest, (k_batches_merge<DX>), dim3(nblk(n, 64)), dim3(64), 0, st, ctx->tv.digest, n, dops.p + done, aC, aH, bad.p);
        LAUNCH_CHECK();
        done = level_end[lv];
    }
    RCCHK(batches_move(st, T, W, 2, dsibm_dst.p, dsibm_src.p, aC, gPC.p));
    RCCHK(batches_move(st, R / 4, W, 1, drngm_dst.p, drngm_src.p, dR, gR.p));
    for (size_t g = 0; g < ng; g++) {                                          // one policy check per S-group
        const size_t rows = G.row0[g + 1] - G.row0[g];
        if (!rows) continue;
        RCCHK(verify_policy_device(ctx, P.shape[g].plan, rows, (int)P.group_S[g], gPC.p + G.sib0[g] * 8, gR.p + G.word0[g], P.shape[g].words, n_bits, dseed,
                                   rok.p + G.row0[g], dsub.p + G.row0[g], dV.p));
    }
    hipLaunchKernelGGL(k_batches_roots, dim3(nblk(nb, 256)), dim3(256), 0, st, nb, droot_slot.p, dpos.p, aC, aH, droot, bad.p, rok.p, d_ok);
    LAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(st));
    return DAPOL_OK;
}

int32_t dapol_verify_batches(dapol_ctx* ctx, int32_t height, size_t nb, const uint64_t* batch_off, const uint64_t* leaf_idx, const uint8_t* leaf_C32,
                             const uint8_t* leaf_H32, const uint64_t* sib_off, const uint8_t* sib_C32, const uint8_t* sib_H32, const uint8_t root_C32[32],
                             const uint8_t root_H32[32], int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint64_t* range_off,
                             const uint8_t* range_proofs, const uint8_t verify_seed32[32], uint8_t* ok) {
    WIRE_SCOPE();
    if (!ctx || !batch_off || !sib_off || !range_off || !root_C32 || !root_H32 || (nb && !ok)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    VERIFY_SEED_OR_OS(verify_seed32)
    if (height < 0 || height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    NEEDS_32_BYTE_DIGEST(ctx, "dapol_verify_batches");
    RCCHK(batches_offsets_ok(nb, batch_off));
    for (size_t j = 0; j < nb; j++)
        if (sib_off[j + 1] < sib_off[j] || range_off[j + 1] < range_off[j]) return fail(DAPOL_ERR_INVALID_ARGUMENT, "sib_off and range_off must not decrease");
    const size_t K = (size_t)batch_off[nb], Tc = nb ? (size_t)(sib_off[nb] - sib_off[0]) : 0, Rc = nb ? (size_t)(range_off[nb] - range_off[0]) : 0;
    if ((K && (!leaf_idx || !leaf_C32 || !leaf_H32)) || (Tc && (!sib_C32 || !sib_H32)) || (Rc && !range_proofs)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    for (size_t j = 0; j < nb; j++) ok[j] = 0;
    if (nb == 0) return DAPOL_OK;
    VerifyBatchesPlan V;
    RCCHK(verify_batches_plan(ctx, height, nb, batch_off, leaf_idx, sib_off, policy, aggregation_factor, n_bits, range_off, range_proofs, V));
    // the upload / download shell: the caller's leaves, siblings, blobs, root and seed go up into the arena, only ok[nb] comes back
    const uint8_t* rbase = range_proofs ? range_proofs + range_off[0] : nullptr;
    const size_t up_bytes = V.aligned ? Rc : V.staged.size();
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<uint32_t> aC, aH, droot, dseed, dR;
    DevBuf<uint8_t> dok;
    StreamDrain drain{st};
    HIPCHK(aC.alloc(V.slots * 8 + 8)); HIPCHK(aH.alloc(V.slots * 8 + 8)); HIPCHK(droot.alloc(16)); HIPCHK(dseed.alloc(8)); HIPCHK(dR.alloc(up_bytes / 4 + 8));
    HIPCHK(dok.alloc(nb));
    if (K) {
        HIPCHK(hipMemcpyAsync(aC.p, leaf_C32, K * 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(aH.p, leaf_H32, K * 32, hipMemcpyHostToDevice, st));
    }
    if (Tc) {
        HIPCHK(hipMemcpyAsync(aC.p + K * 8, sib_C32 + sib_off[0] * 32, Tc * 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(aH.p + K * 8, sib_H32 + sib_off[0] * 32, Tc * 32, hipMemcpyHostToDevice, st));
    }
    if (up_bytes) HIPCHK(hipMemcpyAsync(dR.p, V.aligned ? rbase : V.staged.data(), up_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(droot.p, root_C32, 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(droot.p + 8, root_H32, 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dseed.p, verify_seed32, 32, hipMemcpyHostToDevice, st));
    RCCHK(verify_batches_device(ctx, V, nb, n_bits, aC.p, aH.p, dR.p, droot.p, dseed.p, dok.p));
    HIPCHK(hipMemcpyAsync(ok, dok.p, nb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DAPOL_OK;
}

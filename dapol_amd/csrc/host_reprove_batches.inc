// dapol_reprove_batches / dapol_reprove_batches_plan: after an edit of the tree, only the sub-proofs of the batches whose sibling
// commitments moved are proven again (definitions: include/dapol_hip.h; index arithmetic: reprove_batches_plan.inc; kernels:
// kernels_reprove_batches.h).  The batch counterpart of host_reprove.inc.  A sub-proof of a batch carries its own seed, stream id and
// first slot (RangeArgs::slot_of), so the dirty sub-proofs need no S-groups: all of one m are ONE call of the range prover.
// Included from dapol_hip.hip after host_batches.inc.

int32_t dapol_reprove_batches_plan(int32_t height, size_t nb, const uint64_t* batch_off, const uint64_t* leaf_idx, const uint8_t* has_old, size_t k,
                                   const uint64_t* edited_idx, int32_t policy, int32_t aggregation_factor, int32_t n_bits, uint64_t* n_proved,
                                   uint64_t* total_proved, uint64_t* sum_m_proved, uint64_t* sum_m_all) {
    WIRE_SCOPE();
    if (!batch_off || (k && !edited_idx)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (height < 0 || height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    BatchesPlan P;
    RCCHK(batches_plan_host(height, nb, batch_off, leaf_idx, policy, aggregation_factor, n_bits, 0, true, P));
    if (!reprove_batches_increasing_below(height, k, edited_idx))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "edited indexes must be strictly increasing and below 2^height");
    ReproveBatchesPlanOut out;
    for (size_t j = 0; j < nb; j++) {
        const uint64_t proved = reprove_batches_plan_batch(P.shape[P.group_of[j]].plan, P.sibs.data() + P.sib_off[j], !has_old || has_old[j], k, edited_idx, out);
        if (n_proved) n_proved[j] = proved;
    }
    if (total_proved) *total_proved = out.total_proved;
    if (sum_m_proved) *sum_m_proved = out.sum_m_proved;
    if (sum_m_all) *sum_m_all = out.sum_m_all;
    return DAPOL_OK;
}

// A batch list as the re-prover's device side reads it: the counts on the host, the plan tables on the device.  dapol_reprove_batches
// builds one per call; a batch store (host_batch_store.inc) keeps its list's between refreshes, so that a refresh of an unchanged list
// uploads nothing.
struct ReproveBatchesList {
    int H = 0;
    size_t nb = 0, K = 0, T = 0, R = 0, n = 0, nf = 1;       // batches, leaves, sibling records, blob WORDS, pairs, flags (classes x pairs + 1)
    uint32_t max_m = 1;
    ReproveBatchesClasses Kc{};                                // n, m and pieces of the classes (ascending m); the rest is per call
    std::vector<uint64_t> sib_off, range_off;                  // [nb + 1] dapol_batches_plan's (host copies)
    DevBuf<uint64_t> leaf, off, pair_off, d_sib_off, piece_off;        // [K], then [nb + 1] each
    DevBuf<uint32_t> pos, src, group_of, ent0;                 // [nb] identity (k_batches_seed's rows), [T] gather sources, [nb], [groups + 1]
    DevBuf<ReproveBatchesEntry> tab;                           // one entry per sub-proof of each distinct plan
    ReproveBatchesDev dev() const { return ReproveBatchesDev{nb, n, pair_off.p, d_sib_off.p, piece_off.p, group_of.p, ent0.p, tab.p}; }
};

// The tables of a validated list (P: batches_plan_host's, with the siblings kept) built on the host and uploaded to the
// device (the uploads have completed on return).  Refuses what the plan's limits refuse, before anything is allocated.
static int32_t reprove_batches_list_build(dapol_ctx* ctx, int H, const BatchesPlan& P, size_t nb, const uint64_t* batch_off, const uint64_t* leaf_idx, int n_bits,
                                          ReproveBatchesList& L) {
    const size_t ng = P.group_S.size(), K = (size_t)batch_off[nb], T = (size_t)P.sib_off[nb];
    // host plan: where every sibling record comes from (caller order), the pairs of every batch, one table entry per sub-proof of
    // each distinct plan, the m-classes in ascending m
    std::vector<uint32_t> class_m;
    for (size_t g = 0; g < ng; g++)
        for (auto& sp : P.shape[g].plan)
            if (std::find(class_m.begin(), class_m.end(), (uint32_t)sp.m) == class_m.end()) class_m.push_back((uint32_t)sp.m);
    std::sort(class_m.begin(), class_m.end());
    if (class_m.size() > REPROVE_BATCHES_MAX_CLASSES) return fail(DAPOL_ERR_INVALID_ARGUMENT, "batch too large");
    L.H = H; L.nb = nb; L.K = K; L.T = T; L.R = (size_t)P.range_off[nb] / 4;
    L.sib_off = P.sib_off; L.range_off = P.range_off;
    L.Kc = ReproveBatchesClasses{};
    L.Kc.n = (uint32_t)class_m.size();
    L.max_m = 1;
    for (uint32_t c = 0; c < L.Kc.n; c++) {
        L.Kc.m[c] = class_m[c]; L.Kc.pieces[c] = (uint32_t)(dapol_range_proof_size(n_bits, (int32_t)class_m[c]) / 16);
        L.max_m = std::max(L.max_m, class_m[c]);
    }
    std::vector<ReproveBatchesEntry> tab;
    std::vector<uint32_t> ent0(ng + 1, 0);
    for (size_t g = 0; g < ng; g++) {
        reprove_batches_entries(P.shape[g].plan, n_bits, class_m, tab);
        ent0[g + 1] = (uint32_t)tab.size();
    }
    std::vector<uint32_t> src(T);
    std::vector<uint64_t> pair_off(nb + 1, 0), piece_off(nb + 1, 0);
    std::vector<uint32_t> ident(nb);
    const bool leaf_first = g_wire.siblings_leaf_first != 0;
    for (size_t j = 0; j < nb; j++) {
        const size_t g = P.group_of[j], S = P.group_S[g];
        pair_off[j + 1] = pair_off[j] + P.shape[g].plan.size();
        piece_off[j + 1] = P.range_off[j + 1] / 16;
        ident[j] = (uint32_t)j;
        const BatchSib* sb = P.sibs.data() + P.sib_off[j];
        for (size_t i = 0; i < S; i++)
            src[P.sib_off[j] + i] = (uint32_t)(((size_t)batch_off[j] + sb[i].src_leaf) * (size_t)H + (size_t)(leaf_first ? sb[i].level : H - 1 - sb[i].level));
    }
    L.n = (size_t)pair_off[nb]; L.nf = (size_t)L.Kc.n * L.n + 1;
    if (L.nf > 0xffffffffull) return fail(DAPOL_ERR_INVALID_ARGUMENT, "too many sub-proofs in one call (classes x sub-proofs must stay below 2^32)");

    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    HIPCHK(L.leaf.alloc(K)); HIPCHK(L.off.alloc(nb + 1)); HIPCHK(L.pos.alloc(nb)); HIPCHK(L.src.alloc(T + 1));
    HIPCHK(L.pair_off.alloc(nb + 1)); HIPCHK(L.d_sib_off.alloc(nb + 1)); HIPCHK(L.piece_off.alloc(nb + 1)); HIPCHK(L.group_of.alloc(nb)); HIPCHK(L.ent0.alloc(ng + 1));
    HIPCHK(L.tab.alloc(tab.size() + 1));
    HIPCHK(hipMemcpyAsync(L.leaf.p, leaf_idx, K * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(L.off.p, batch_off, (nb + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(L.pos.p, ident.data(), nb * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(L.pair_off.p, pair_off.data(), (nb + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(L.d_sib_off.p, P.sib_off.data(), (nb + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(L.piece_off.p, piece_off.data(), (nb + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(L.group_of.p, P.group_of.data(), nb * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(L.ent0.p, ent0.data(), (ng + 1) * 4, hipMemcpyHostToDevice, st));
    if (!tab.empty()) HIPCHK(hipMemcpyAsync(L.tab.p, tab.data(), tab.size() * sizeof(ReproveBatchesEntry), hipMemcpyHostToDevice, st));
    if (T) HIPCHK(hipMemcpyAsync(L.src.p, src.data(), T * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));                         // the host tables above go out of scope here
    return DAPOL_OK;
}

// The device side of a re-prove over a list whose tables, old commitments and blobs are on the device already (nb > 0).  The tree's
// current siblings are gathered into new_C / new_H ([T + 1][8] words each); a pair is dirty where has_old (device, may be null: every
// batch has an old proof) is 0 or old_C (may be null when no batch has one) differs from new_C; the dirty sub-proofs of each m are one
// call of the range prover; their pieces are written over `range` ([R + 4] words), where the old blobs lie -- the ONLY write into
// caller state, made after every refusal and allocation of the call: *wrote_range (may be null) is set just before it.  An unknown
// leaf ends the call before anything is written.  Everything runs on the context's stream; on return the stream has been drained.
static int32_t reprove_batches_device(dapol_ctx* ctx, dapol_tree* tree, const ReproveBatchesList& L, int n_bits, const uint32_t* d_seed8, const uint8_t* d_has_old,
                                      const uint32_t* old_C, uint32_t* range, uint32_t* new_C, uint32_t* new_H, uint64_t* proved_out, uint64_t* calls_out,
                                      bool* wrote_range) {
    hipStream_t st = ctx->stream;
    const size_t nb = L.nb, K = L.K, T = L.T, R = L.R, n = L.n, nf = L.nf, tot = K * (size_t)L.H;
    ReproveBatchesClasses Kc = L.Kc;
    DevBuf<uint64_t> pv, gv, dstream, vals, cstream, cslot;
    DevBuf<uint32_t> seeds, dleafpos, pC, pH, pr, gr, dirty, flag, rank, blind, Vc, cseed, proofs;
    StreamDrain drain{st};
    HIPCHK(seeds.alloc(nb * 8)); HIPCHK(dstream.alloc(nb)); HIPCHK(dleafpos.alloc(K));
    HIPCHK(pC.alloc(tot * 8 + 8)); HIPCHK(pH.alloc(tot * 8 + 8)); HIPCHK(pr.alloc(tot * 8 + 8)); HIPCHK(pv.alloc(tot + 1));
    HIPCHK(gr.alloc(T * 8 + 8)); HIPCHK(gv.alloc(T + 1));
    HIPCHK(dirty.alloc(n + 1)); HIPCHK(flag.alloc(nf)); HIPCHK(rank.alloc(nf));
    PathOut po{pC.p, pH.p, pv.p, pr.p}, go{new_C, new_H, gv.p, gr.p};
    RCCHK(tree_paths_device(tree, K, L.leaf.p, po, dleafpos.p));                  // (an unknown leaf ends the call here: nothing written)
    hipLaunchKernelGGL(k_batches_seed, dim3(nblk(nb, 64)), dim3(64), 0, st, nb, d_seed8, L.off.p, L.leaf.p, L.pos.p, seeds.p, dstream.p);
    LAUNCH_CHECK();
    if (T) {
        hipLaunchKernelGGL(k_batches_gather, dim3(nblk(T, 256)), dim3(256), 0, st, T, L.src.p, po, go);
        LAUNCH_CHECK();
    }
    uint64_t calls = 0, proved = 0;
    if (n) {
        const ReproveBatchesDev D = L.dev();
        HIPCHK(hipMemsetAsync(flag.p, 0, nf * 4, st));
        hipLaunchKernelGGL(k_reprove_batches_dirty, dim3(nblk(n * REPROVE_LANES, 256)), dim3(256), 0, st, D, d_has_old, (const uint4*)old_C, (const uint4*)new_C,
                           dirty.p, flag.p);
        LAUNCH_CHECK();
        RCCHK(inclusive_scan_u32(st, flag.p, rank.p, nf));
        // the dirty pairs before each class (the scan's element before its first pair), and all of them: one read-back
        for (uint32_t c = 0; c <= Kc.n; c++) {
            const size_t at = c < Kc.n ? reprove_batches_base_at(c, n) : nf - 1;
            if (at != (size_t)-1) HIPCHK(hipMemcpyAsync(&Kc.before[c], rank.p + at, 4, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        reprove_batches_layout(Kc);
        const size_t U = Kc.before[Kc.n];
        if (U) {                                             // (nothing dirty: the range prover is not entered)
            HIPCHK(vals.alloc(Kc.parties)); HIPCHK(blind.alloc(Kc.parties * 8)); HIPCHK(Vc.alloc(Kc.parties * 8)); HIPCHK(cseed.alloc(U * 8));
            HIPCHK(cstream.alloc(U)); HIPCHK(cslot.alloc(U)); HIPCHK(proofs.alloc(Kc.proof_pieces * 4));
            const uint32_t* Bb_comp = ctx->gens_comp.p + (size_t)ctx->tv.row_Bb(0) * 8;
            hipLaunchKernelGGL(k_reprove_batches_gather, dim3(nblk(n * (size_t)L.max_m, 256)), dim3(256), 0, st, D, Kc, L.max_m, dirty.p, rank.p, gv.p, gr.p, new_C, Bb_comp,
                               seeds.p, dstream.p, vals.p, blind.p, Vc.p, cseed.p, cstream.p, cslot.p);
            LAUNCH_CHECK();
            // one call of the range prover per class that has dirty rows: a row per proof, each with its own seed, stream id and slot
            for (uint32_t c = 0; c < Kc.n; c++) {
                const size_t b0 = Kc.before[c], Uc = (size_t)Kc.before[c + 1] - b0;
                if (!Uc) continue;
                RCCHK(range_prove_device(ctx, n_bits, (int)Kc.m[c], Uc, vals.p + Kc.party_off[c], blind.p + Kc.party_off[c] * 8, Vc.p + Kc.party_off[c] * 8,
                                         cseed.p + b0 * 8, cstream.p + b0, 0, nullptr, proofs.p + Kc.piece_off[c] * 4, nullptr, 0, 1, 0, nullptr, 8, cslot.p + b0));
                calls++;
            }
            if (wrote_range) *wrote_range = true;
            hipLaunchKernelGGL(k_reprove_batches_scatter, dim3(nblk(R / 4, 256)), dim3(256), 0, st, D, Kc, R / 4, dirty.p, rank.p, (const uint4*)proofs.p,
                               (uint4*)range);
            LAUNCH_CHECK();
        }
        proved = U;
    }
    HIPCHK(hipStreamSynchronize(st));
    if (proved_out) *proved_out = proved;
    if (calls_out) *calls_out = calls;
    return DAPOL_OK;
}

int32_t dapol_reprove_batches(dapol_ctx* ctx, dapol_tree* tree, size_t nb, const uint64_t* batch_off, const uint64_t* leaf_idx, int32_t policy,
                              int32_t aggregation_factor, int32_t n_bits, const uint8_t nonce_seed32[32], const uint8_t* has_old, const uint8_t* old_sib_C32,
                              const uint8_t* old_range, uint8_t* sib_C32, uint8_t* sib_H32, uint8_t* range_out, uint64_t* proved_out, uint64_t* kept_out,
                              uint64_t* n_calls_out) {
    WIRE_SCOPE();
    // dapol_prove_batches' refusals, in its order
    if (!ctx || !tree || tree->ctx != ctx || !nonce_seed32 || !batch_off) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (tree->shard_bits) return fail(DAPOL_ERR_INVALID_ARGUMENT, "batched proofs need the whole tree (not a shard)");
    TREE_USABLE(tree);
    NEEDS_32_BYTE_DIGEST(ctx, "dapol_reprove_batches");
    const int H = tree->height;
    BatchesPlan P;
    RCCHK(batches_plan_host(H, nb, batch_off, leaf_idx, policy, aggregation_factor, n_bits, ctx->max_parties, true, P));
    const size_t T = (size_t)P.sib_off[nb], R = (size_t)P.range_off[nb] / 4;
    if (R && !range_out) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (nb == 0) {
        if (proved_out) *proved_out = 0;
        if (kept_out) *kept_out = 0;
        if (n_calls_out) *n_calls_out = 0;
        return DAPOL_OK;
    }
    bool any_old = has_old == nullptr;
    for (size_t j = 0; has_old && j < nb && !any_old; j++) any_old = has_old[j] != 0;
    if (any_old && ((T && !old_sib_C32) || (R && !old_range)))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "old_sib_C32 and old_range are needed while some batch has an old proof (has_old set, or NULL)");
    // the upload / download shell: the list's tables, the seed, the old arrays go up; reprove_batches_device works on them where they
    // lie; the blobs and the gathered siblings come down
    ReproveBatchesList L;
    DevBuf<uint32_t> dseed, gC, gH, doldC, orange;
    DevBuf<uint8_t> dhas;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    StreamDrain drain{st};
    RCCHK(reprove_batches_list_build(ctx, H, P, nb, batch_off, leaf_idx, n_bits, L));
    HIPCHK(dseed.alloc(8)); HIPCHK(gC.alloc(T * 8 + 8)); HIPCHK(gH.alloc(T * 8 + 8)); HIPCHK(orange.alloc(R + 4));
    // every input goes up before anything is written back: the outputs may alias the old arrays
    HIPCHK(hipMemcpyAsync(dseed.p, nonce_seed32, 32, hipMemcpyHostToDevice, st));
    if (has_old) { HIPCHK(dhas.alloc(nb)); HIPCHK(hipMemcpyAsync(dhas.p, has_old, nb, hipMemcpyHostToDevice, st)); }
    if (any_old) {
        HIPCHK(doldC.alloc(T * 8 + 8));
        if (T) HIPCHK(hipMemcpyAsync(doldC.p, old_sib_C32, T * 32, hipMemcpyHostToDevice, st));
        if (R) HIPCHK(hipMemcpyAsync(orange.p, old_range, R * 4, hipMemcpyHostToDevice, st));      // the old blobs ARE the output buffer: kept pieces never move
    }
    uint64_t proved = 0, calls = 0;
    RCCHK(reprove_batches_device(ctx, tree, L, n_bits, dseed.p, dhas.p, doldC.p, orange.p, gC.p, gH.p, &proved, &calls, nullptr));
    if (R) HIPCHK(hipMemcpyAsync(range_out, orange.p, R * 4, hipMemcpyDeviceToHost, st));
    if (sib_C32 && T) HIPCHK(hipMemcpyAsync(sib_C32, gC.p, T * 32, hipMemcpyDeviceToHost, st));
    if (sib_H32 && T) HIPCHK(hipMemcpyAsync(sib_H32, gH.p, T * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (proved_out) *proved_out = proved;
    if (kept_out) *kept_out = (uint64_t)L.n - proved;
    if (n_calls_out) *n_calls_out = calls;
    return DAPOL_OK;
}

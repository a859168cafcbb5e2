// COMPACT MERKLE PATHS (definition in include/dapol_hip.h; index arithmetic in compact_paths_plan.inc; kernels in
// kernels_compact_paths.h): the host-only dapol_compact_paths_plan / _expand / _compress, the prover's dapol_tree_paths_compact and the
// verifier dapol_verify_entities_compact_paths, which merges every distinct node of the call's paths once.

static int32_t cpaths_fail(int rc, int32_t height) {
    if (rc == CPATHS_BAD_HEIGHT && height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    return fail(DAPOL_ERR_INVALID_ARGUMENT, cpaths_strerror(rc));
}

int32_t dapol_compact_paths_plan(int32_t height, size_t b, const uint64_t* leaf_idx, uint64_t* depth_off, uint32_t* ref, uint64_t* n_records) {
    const int rc = cpaths_plan_checked(height, b, leaf_idx, depth_off, ref, n_records);
    return rc ? cpaths_fail(rc, height) : DAPOL_OK;
}
int32_t dapol_compact_paths_expand(int32_t hash_bytes, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* cpath_C32, const uint8_t* cpath_H,
                                   size_t n_records, size_t first, size_t count, uint8_t* path_C32_out, uint8_t* path_H_out) {
    WIRE_SCOPE();
    const int rc = cpaths_expand_checked(hash_bytes, height, b, leaf_idx, cpath_C32, cpath_H, n_records, first, count, g_wire.siblings_leaf_first != 0,
                                         path_C32_out, path_H_out);
    return rc ? cpaths_fail(rc, height) : DAPOL_OK;
}
int32_t dapol_compact_paths_compress(int32_t hash_bytes, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* path_C32, const uint8_t* path_H,
                                     uint8_t* cpath_C32_out, uint8_t* cpath_H_out, size_t cap_records, uint64_t* n_records_out) {
    WIRE_SCOPE();
    const int rc = cpaths_compress_checked(hash_bytes, height, b, leaf_idx, path_C32, path_H, g_wire.siblings_leaf_first != 0, cpath_C32_out, cpath_H_out,
                                           cap_records, n_records_out);
    return rc ? cpaths_fail(rc, height) : DAPOL_OK;
}

// The layout and the link words of checked indexes, as the kernels take them.
struct CPathsHost {
    CPathsDev L{};
    uint64_t n_records = 0;
    std::vector<uint32_t> link;
    const uint64_t* idx = nullptr;           // the caller's checked indexes
    uint64_t n_unique(int d) const { return d == 0 ? 1 : L.depth_off[d + 1] - L.depth_off[d]; }
};
static void cpaths_host_build(int H, size_t b, const uint64_t* idx, CPathsHost& P) {
    P.L.H = (uint32_t)H; P.idx = idx;
    P.n_records = cpaths_layout(H, b, idx, P.L.depth_off, nullptr);
    P.link.resize((size_t)P.n_records);
    cpaths_links(H, b, idx, P.L.depth_off, P.link.data());
}

// ------------------------------------------------------------------------------------------------ the prover's side
int32_t dapol_tree_paths_compact(dapol_tree* tree, size_t b, const uint64_t* leaf_idx, uint8_t* cpath_C32, uint8_t* cpath_H32, size_t cap_records,
                                 uint64_t* n_records_out) {
    if (!tree || (b && !leaf_idx)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    TREE_USABLE(tree);
    if (tree->shard_bits) return fail(DAPOL_ERR_INVALID_ARGUMENT, "compact paths are built for plain trees (a shard's upper siblings are one record each: prepend them)");
    const int H = tree->height;
    if (!strictly_increasing(b, leaf_idx)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "leaf indexes must be strictly increasing");
    if (b && H < 64 && (leaf_idx[b - 1] >> H) != 0) return fail(DAPOL_ERR_UNKNOWN_LEAF, "no liability at one of the requested leaves");
    if (b == 0 || H == 0) {                                          // (a tree of height 0 is its root: no siblings)
        if (n_records_out) *n_records_out = 0;
        return DAPOL_OK;
    }
    // the layout from the indexes alone, and the length check, before anything is queued
    const uint64_t n = cpaths_layout(H, b, leaf_idx, nullptr, nullptr);
    if (n > (uint64_t)cap_records) return fail(DAPOL_ERR_INVALID_ARGUMENT, cpaths_strerror(CPATHS_BAD_CAP));
    if (!cpaths_links_fit(b, n)) return fail(DAPOL_ERR_INVALID_ARGUMENT, cpaths_strerror(CPATHS_TOO_MANY));
    if (!cpath_C32 || !cpath_H32) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    CPathsHost P;
    cpaths_host_build(H, b, leaf_idx, P);
    dapol_ctx* ctx = tree->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t hw = (size_t)ctx_hw(ctx);
    DevBuf<uint64_t> dl;
    DevBuf<uint32_t> dpos, dlink, dC, dH, missing;
    HIPCHK(dl.alloc(b)); HIPCHK(dpos.alloc(b)); HIPCHK(dlink.alloc((size_t)n)); HIPCHK(dC.alloc((size_t)n * 8)); HIPCHK(dH.alloc((size_t)n * hw));
    HIPCHK(missing.alloc(1));
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};      // nothing of the call is freed while the stream still runs
    HIPCHK(hipMemcpyAsync(dl.p, leaf_idx, b * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dlink.p, P.link.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(missing.p, 0, 4, st));
    LevelView l0 = tree->view(0);
    hipLaunchKernelGGL(k_tree_find_leaves, dim3(nblk(b, 256)), dim3(256), 0, st, b, dl.p, l0.n, l0.idx, dpos.p, missing.p);
    LAUNCH_CHECK();
    uint32_t h_missing = 0;
    HIPCHK(hipMemcpyAsync(&h_missing, missing.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_missing) return fail(DAPOL_ERR_UNKNOWN_LEAF, "no liability at one of the requested leaves");
    hipLaunchKernelGGL(k_tree_path_walk_compact, dim3(nblk(b, 64)), dim3(64), 0, st, b, dpos.p, tree->d_views.p,
                       ctx_wide(ctx) ? (const WideView*)tree->d_wviews.p : (const WideView*)nullptr, P.L, dlink.p, dC.p, dH.p);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(cpath_C32, dC.p, (size_t)n * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(cpath_H32, dH.p, (size_t)n * hw * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_records_out) *n_records_out = n;
    return DAPOL_OK;
}

// ------------------------------------------------------------------------------------------------ the verifier
// Device time of the path stage of the last dapol_verify_entities_compact_paths (HIP events around its path launches) and the route it
// took: 1 = every distinct node merged once, 2 = that and the fallback (expansion + k_verify_paths), 3 = the fallback alone (measurement
// knob DAPOL_CPATHS_FALLBACK: the per-entity re-merge of the same call, which is what dapol_verify_entities_compact runs), 0 = forwarded.
static std::atomic<double> g_last_cpaths_ms{0.0};
static std::atomic<int> g_last_cpaths_route{0};
int32_t dapol_diag_compact_paths(double* path_ms, int32_t* route) {
    if (!path_ms || !route) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    *path_ms = g_last_cpaths_ms.load(std::memory_order_relaxed);
    *route = g_last_cpaths_route.load(std::memory_order_relaxed);
    return DAPOL_OK;
}

struct CPathsEvents {
    hipEvent_t a = nullptr, z = nullptr;
    ~CPathsEvents() { if (a) (void)hipEventDestroy(a); if (z) (void)hipEventDestroy(z); }
};
// Everything the call holds on the device; the caller drains the stream before this goes.
struct CPathsVerifyBufs {
    DevBuf<uint8_t> arena;
    DevBuf<uint32_t> nodeC, nodeH, joinC, joinH, join_at, row[2], bad, expC, expH, Vc;
    DevBuf<int32_t> ext[2];
    DevBuf<uint8_t> sub;
    DevBuf<uint64_t> dl;                     // the leaf indexes: only the fallback's kernels take them
};

static int32_t verify_compact_paths_queue(dapol_ctx* ctx, int H, size_t b, const CPathsHost& P, const SCompactPlan& S, const uint64_t* sub_off, const uint32_t* first,
                                          uint64_t heads, const uint8_t* leaf_C32, const uint8_t* leaf_H32, const uint8_t* cpath_C32, const uint8_t* cpath_H32,
                                          const uint8_t* root_C32, const uint8_t* root_H32, int n_bits, const uint8_t* compact, size_t compact_len,
                                          const uint8_t* verify_seed32, uint8_t* ok, uint64_t* merges_out, CPathsVerifyBufs& B) {
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)P.n_records;
    const size_t sizes[10] = {b * 32, b * 32, n * 32, n * 32, compact_len, 64, 32, n * 4, b, b};
    size_t offs[10], total = 0;
    for (int i = 0; i < 10; i++) { offs[i] = total; total += align_up(sizes[i], 256); }
    HIPCHK(B.arena.alloc(total));
    uint8_t* base = B.arena.p;
    uint32_t *dLC = (uint32_t*)(base + offs[0]), *dLH = (uint32_t*)(base + offs[1]), *dRC = (uint32_t*)(base + offs[2]), *dRH = (uint32_t*)(base + offs[3]);
    uint32_t *dR = (uint32_t*)(base + offs[4]), *droot = (uint32_t*)(base + offs[5]), *dseed = (uint32_t*)(base + offs[6]), *dlink = (uint32_t*)(base + offs[7]);
    uint8_t *dok = base + offs[8], *dpath = base + offs[9];
    const void* src[8] = {leaf_C32, leaf_H32, cpath_C32, cpath_H32, compact, nullptr, verify_seed32, P.link.data()};
    for (int i = 0; i < 8; i++)
        if (src[i] && sizes[i]) HIPCHK(hipMemcpyAsync(base + offs[i], src[i], sizes[i], hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(droot, root_C32, 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(droot + 8, root_H32, 32, hipMemcpyHostToDevice, st));

    // ---- the path stage
    CPathsEvents ev;
    HIPCHK(hipEventCreate(&ev.a)); HIPCHK(hipEventCreate(&ev.z));
    const size_t n_nodes = 1 + (size_t)P.L.depth_off[H], n_ext = H > 1 ? (size_t)P.n_unique(H - 1) : 1;
    HIPCHK(B.bad.alloc(1));
    HIPCHK(hipMemsetAsync(B.bad.p, 0, 4, st));
    const bool only_fallback = knob("DAPOL_CPATHS_FALLBACK") != nullptr;       // measurement knob (tools/bench_compact_paths.py): the baseline's path stage
    uint32_t h_bad = 1;
    int route = 3;
    uint64_t merges = 0;
    const size_t tot = b * (size_t)H;
    // every allocation that is known to be needed comes before the first event: the stage's time is its launches'
    if (!only_fallback) {
        HIPCHK(B.nodeC.alloc(n_nodes * 8)); HIPCHK(B.nodeH.alloc(n_nodes * 8)); HIPCHK(B.joinC.alloc(b * 8)); HIPCHK(B.joinH.alloc(b * 8));
        HIPCHK(B.join_at.alloc(b));
        for (int k = 0; k < 2; k++) { HIPCHK(B.ext[k].alloc(n_ext * P3_WORDS)); HIPCHK(B.row[k].alloc(n_ext)); }
    } else { HIPCHK(B.expC.alloc(tot * 8 + 8)); HIPCHK(B.expH.alloc(tot * 8 + 16)); HIPCHK(B.dl.alloc(b)); }
    HIPCHK(hipEventRecord(ev.a, st));
    if (!only_fallback) {
        CPathsMerge M{dlink, dLC, dLH, dRC, dRH, B.nodeC.p, B.nodeH.p, B.joinC.p, B.joinH.p, B.join_at.p, B.bad.p};
        // one launch per depth over that depth's nodes, bottom-up: launch d reads the points that launch d + 1 left in buffer (d & 1)
        // and leaves its parents' in the other one
        for (int d = H; d >= 1; d--) {
            const size_t nd = (size_t)P.n_unique(d);
            LAUNCH_DX(ctx->tv.digest, (k_cpaths_level<8, DX>), dim3(nblk(nd, 64)), dim3(64), 0, st, ctx->tv.digest, d, nd, P.L, M, B.ext[d & 1].p, B.row[d & 1].p,
                      B.ext[(d & 1) ^ 1].p, B.row[(d & 1) ^ 1].p);
            LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_cpaths_joins, dim3(nblk(b, 256)), dim3(256), 0, st, b, M, droot, droot + 8);
        LAUNCH_CHECK();
        HIPCHK(hipMemcpyAsync(&h_bad, B.bad.p, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        merges = P.n_records;
        route = 1;
    }
    if (h_bad) {
        // Some decoding failed, or a join or the root differs: which rows that fails is a per-entity question (a verdict below a join
        // and one above it are different things), so the per-entity re-merge answers it over the expansion, as it is.
        if (!only_fallback) { HIPCHK(B.expC.alloc(tot * 8 + 8)); HIPCHK(B.expH.alloc(tot * 8 + 16)); HIPCHK(B.dl.alloc(b)); }
        HIPCHK(hipMemcpyAsync(B.dl.p, P.idx, b * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_cpaths_expand, dim3(nblk(b, 256)), dim3(256), 0, st, b, P.L, g_wire.siblings_leaf_first, dlink, dRC, dRH, B.expC.p, B.expH.p);
        LAUNCH_CHECK();
        if (verify_paths_few(b))
            LAUNCH_DX(ctx->tv.digest, (k_verify_paths_wave<8, DX>), dim3((unsigned)b), dim3(64), 0, st, ctx->tv.digest, b, H, B.dl.p, dLC, dLH, B.expC.p, B.expH.p, droot,
                      droot + 8, g_wire.siblings_leaf_first, dpath);
        else
            LAUNCH_DX(ctx->tv.digest, (k_verify_paths<8, DX>), dim3(nblk(b, 64)), dim3(64), 0, st, ctx->tv.digest, b, H, B.dl.p, dLC, dLH, B.expC.p, B.expH.p, droot,
                      droot + 8, g_wire.siblings_leaf_first, dpath);
        LAUNCH_CHECK();
        HIPCHK(hipStreamSynchronize(st));
        merges += (uint64_t)tot;
        if (route == 1) route = 2;
    } else HIPCHK(hipMemsetAsync(dpath, 1, b, st));             // every decoding, every join and the root held: every path verifies
    HIPCHK(hipEventRecord(ev.z, st));

    // ---- the range proofs: the compact verifier's groups, each a batch that lies in the uploaded buffer as it is; the commitments of a
    // statement come from the records its head walks
    HIPCHK(hipMemsetAsync(dok, 1, b, st));
    const VSharedPlan& V = S.V;
    size_t parties = 0;
    std::vector<size_t> party_off(V.n_groups);
    for (uint32_t gi = 0; gi < V.n_groups; gi++) {
        const VSharedGroup& G = V.g[gi];
        party_off[gi] = parties;
        parties += (size_t)(first[G.s0 + G.k] - first[G.s0]) * G.m;
    }
    HIPCHK(B.Vc.alloc(parties * 8 + 8)); HIPCHK(B.sub.alloc((size_t)heads + 1));
    const uint32_t* Bb_comp = ctx->gens_comp.p + (size_t)ctx->tv.row_Bb(0) * 8;
    CPathsRange R{};
    R.n_sub = V.n_sub;
    for (uint32_t gi = 0; gi < V.n_groups; gi++) {
        const VSharedGroup& G = V.g[gi];
        for (uint32_t s = G.s0; s < G.s0 + G.k; s++) {
            const int D = H - (int)S.shift[s];
            const size_t ns = first[s + 1] - first[s];
            R.D[s] = (uint8_t)D; R.first[s] = first[s];
            hipLaunchKernelGGL(k_cpaths_gather, dim3(nblk(ns, 256)), dim3(256), 0, st, ns, D, (int)V.start[s], (int)V.count[s], (int)G.m, g_wire.siblings_leaf_first, P.L,
                               dlink, dRC, Bb_comp, B.Vc.p + (party_off[gi] + (size_t)(first[s] - first[G.s0]) * G.m) * 8);
            LAUNCH_CHECK();
        }
    }
    for (uint32_t gi = 0; gi < V.n_groups; gi++) {
        const VSharedGroup& G = V.g[gi];
        const int32_t rc = range_verify_rlc_device(ctx, n_bits, (int)G.m, first[G.s0 + G.k] - first[G.s0], (const uint32_t*)((const uint8_t*)dR + sub_off[G.s0]),
                                                   (size_t)G.pieces * 4, B.Vc.p + party_off[gi] * 8, dseed, B.sub.p + first[G.s0]);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_cpaths_verdict, dim3(nblk(b, 256)), dim3(256), 0, st, b, P.L, R, dlink, B.sub.p, dok);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_and_bytes, dim3(nblk(b, 256)), dim3(256), 0, st, b, dok, dpath);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(ok, dok, b, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.z));
    g_last_cpaths_ms.store((double)ms, std::memory_order_relaxed);
    g_last_cpaths_route.store(route, std::memory_order_relaxed);
    *merges_out = merges;
    return DAPOL_OK;
}

int32_t dapol_verify_entities_compact_paths(dapol_ctx* ctx, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* leaf_C32, const uint8_t* leaf_H32,
                                            size_t n_records, const uint8_t* cpath_C32, const uint8_t* cpath_H32, const uint8_t root_C32[32],
                                            const uint8_t root_H32[32], int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t* compact,
                                            size_t compact_len, const uint8_t verify_seed32[32], uint8_t* ok, uint64_t* unique_subproofs_out,
                                            uint64_t* path_merges_out) {
    WIRE_SCOPE();
    if (!ctx || !root_C32 || !root_H32 || (b && (!leaf_idx || !leaf_C32 || !leaf_H32 || !cpath_C32 || !cpath_H32 || !compact || !ok)))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (ctx_wide(ctx)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "the compact-path verifier is built for the 32-byte node digests");
    VERIFY_SEED_OR_OS(verify_seed32)
    SCompactPlan S;
    int32_t rc = scompact_host_plan(height, b, leaf_idx, policy, aggregation_factor, n_bits, true, S);
    if (rc) return rc;
    if (const int c = cpaths_check(height, b, leaf_idx)) return cpaths_fail(c, height);
    uint32_t max_m = 1;
    for (uint32_t gi = 0; gi < S.V.n_groups; gi++) if (S.V.g[gi].m > max_m) max_m = S.V.g[gi].m;
    if (b && (int)max_m > ctx->max_parties) return fail(DAPOL_ERR_INVALID_ARGUMENT, "aggregation needs more parties than the context was created for");
    uint64_t unique = 0, merges = 0;
    auto finish = [&]() {
        if (unique_subproofs_out) *unique_subproofs_out = unique;
        if (path_merges_out) *path_merges_out = merges;
        return DAPOL_OK;
    };
    // a buffer of the wrong shape is an invalid proof, never an over-read (dapol_verify_entities_compact)
    CPathsHost P;
    P.L.H = (uint32_t)height;
    P.n_records = cpaths_layout(height, b, leaf_idx, P.L.depth_off, nullptr);
    // the statements of sub-proof s are the nodes of its key depth: first[s] = the verification row of its first one, sub_off[s] = its
    // list in the compact proof buffer (scompact_layout's, from the counts of the path layout)
    std::vector<uint64_t> sub_off(S.V.n_sub + 1);
    std::vector<uint32_t> first(S.V.n_sub + 1);
    uint64_t len = 0, heads = 0;
    for (uint32_t s = 0; s < S.V.n_sub; s++) {
        const uint64_t u = b ? P.n_unique(height - (int)S.shift[s]) : 0;
        sub_off[s] = len; first[s] = (uint32_t)heads;
        len += u * (uint64_t)S.V.pieces[s] * 16; heads += u;
    }
    sub_off[S.V.n_sub] = len; first[S.V.n_sub] = (uint32_t)heads;
    if ((uint64_t)n_records != P.n_records || (uint64_t)compact_len != len) {
        for (size_t i = 0; i < b; i++) ok[i] = 0;
        return finish();
    }
    if (b == 0) return finish();
    // The latency regime of the compact verifier: nothing to gain, the paths are cut out on the host and take the existing call.
    size_t forward_max = VSHARED_FORWARD_MAX;
    if (const char* e = test_knob("DAPOL_VSHARED_FORWARD_MAX")) { long long v = atoll(e); if (v >= 0) forward_max = (size_t)v; }
    if (vshared_forwards(b, S.V.n_sub, forward_max)) {
        const size_t tot = b * (size_t)height;
        std::vector<uint8_t> pC(tot * 32), pH(tot * 32);
        const int c = cpaths_expand_checked(32, height, b, leaf_idx, cpath_C32, cpath_H32, n_records, 0, b, g_wire.siblings_leaf_first != 0, pC.data(), pH.data());
        if (c) return cpaths_fail(c, height);
        rc = dapol_verify_entities_compact(ctx, height, b, leaf_idx, leaf_C32, leaf_H32, tot, pC.data(), pH.data(), root_C32, root_H32, policy, aggregation_factor,
                                           n_bits, compact, compact_len, verify_seed32, ok, &unique);
        if (rc) return rc;
        merges = (uint64_t)tot;
        g_last_cpaths_ms.store(0.0, std::memory_order_relaxed);
        g_last_cpaths_route.store(0, std::memory_order_relaxed);
        return finish();
    }
    if (!cpaths_links_fit(b, P.n_records)) return fail(DAPOL_ERR_INVALID_ARGUMENT, cpaths_strerror(CPATHS_TOO_MANY));
    P.link.resize((size_t)P.n_records);
    cpaths_links(height, b, leaf_idx, P.L.depth_off, P.link.data());
    HIPCHK(hipSetDevice(ctx->device));
    CPathsVerifyBufs B;
    P.idx = leaf_idx;
    rc = verify_compact_paths_queue(ctx, height, b, P, S, sub_off.data(), first.data(), heads, leaf_C32, leaf_H32, cpath_C32, cpath_H32, root_C32, root_H32, n_bits,
                                    compact, compact_len, verify_seed32, ok, &merges, B);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; } // drained before B goes, on every return
    unique = heads;
    return finish();
}

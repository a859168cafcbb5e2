// Edits of a built tree (dapol_tree_update, dapol_tree_insert, dapol_tree_remove, dapol_tree_apply): the launchers of the in-place
// paths -- replace, insert (disjoint chains / general), remove, mixed (kernels_ctx_tree.h, "incremental update / insert / insert,
// general / remove", "mixed edit in place") -- and the rebuild they fall back to.  What the paths decide on the host is
// tree_edit_plan.inc; here are the scratch, the launches and the tree's state.  Included by dapol_hip.hip after host_tree.inc.

// Regions of the edit paths' scratch (dapol_tree_owned::upd_scratch) as offsets, taken in order; ensure() once all are taken.
struct EditScratch {
    size_t total = 0;
    size_t take(size_t bytes, size_t align = 1) { const size_t o = align_up(total, align); total = o + bytes; return o; }
    hipError_t ensure(dapol_tree_owned* own) const { return own->upd_scratch.n < total ? own->upd_scratch.alloc(total + total / 2) : hipSuccess; }
};
// idx | v | r of k edited leaves to the front of the scratch, as one copy (`stage` lives until the caller has synchronised).
static int32_t upload_edits(dapol_tree_owned* own, const HostLeaves& E, std::vector<uint8_t>& stage) {
    const size_t k = E.idx.size();
    stage.resize(k * 48);
    memcpy(stage.data(), E.idx.data(), k * 8);
    memcpy(stage.data() + k * 8, E.v.data(), k * 8);
    memcpy(stage.data() + k * 16, E.r.data(), k * 32);
    HIPCHK(hipMemcpyAsync(own->upd_scratch.p, stage.data(), stage.size(), hipMemcpyHostToDevice, own->ctx->stream));
    return DAPOL_OK;
}
// U2 / U3 of the replacement path: the deltas into every node above the edited leaves, then the hashes bottom-up -- one block walks
// all levels while the paths fit it, a launch per level otherwise.
static int32_t rehash_paths(dapol_tree_owned* own, const TreeUpdArgs& U) {
    dapol_ctx* ctx = own->ctx;
    hipStream_t st = ctx->stream;
    const size_t k = U.k;
    const int H = U.height;
    hipLaunchKernelGGL(k_tree_upd_nodes, dim3(nblk(k * (size_t)H, 64)), dim3(64), 0, st, own->d_views.p, U);
    LAUNCH_CHECK();
    if (k <= 1024) {
        LAUNCH_DX(ctx->tv.digest, (k_tree_upd_hash<DX>), dim3(1), dim3((unsigned)align_up(k, 64)), 0, st, ctx->tv.digest, own->d_views.p, U, 0, H);
        LAUNCH_CHECK();
    } else {
        for (int lv = 0; lv < H; lv++) {
            LAUNCH_DX(ctx->tv.digest, (k_tree_upd_hash<DX>), dim3(nblk(k, 256)), dim3(256), 0, st, ctx->tv.digest, own->d_views.p, U, lv, lv + 1);
            LAUNCH_CHECK();
        }
    }
    return DAPOL_OK;
}

// The incremental path of dapol_tree_update (kernels_ctx_tree.h, "incremental update"): every updated leaf already exists, so the
// tree keeps its structure and only the k root-to-leaf paths are re-merged, on the device, in three launches.  E = the edits, sorted
// and distinct.  *done = false (nothing above the leaves touched) when some index is new: the caller then inserts or rebuilds.
static int32_t tree_update_incremental(dapol_tree_owned* own, const HostLeaves& E, bool* done, std::vector<uint8_t>* found_out = nullptr) {
    *done = false;
    dapol_ctx* ctx = own->ctx;
    hipStream_t st = ctx->stream;
    const int H = own->height;
    const size_t k = E.idx.size();
    EditScratch sc;
    const size_t o_idx = sc.take(k * 8), o_v = sc.take(k * 8), o_r = sc.take(k * 32), o_dv = sc.take(k * 8), o_dr = sc.take(k * 32), o_dP = sc.take(k * 160),
                 o_pos = sc.take(k * (size_t)(H + 1) * 4), o_miss = sc.take(8, 8), o_found = sc.take(k);
    HIPCHK(sc.ensure(own));
    uint8_t* d = own->upd_scratch.p;
    std::vector<uint8_t> stage;
    RCCHK(upload_edits(own, E, stage));
    HIPCHK(hipMemsetAsync(d + o_miss, 0, 8, st));
    TreeUpdArgs U{k, H, (const uint64_t*)(d + o_idx), (const uint64_t*)(d + o_v), (const uint32_t*)(d + o_r), (uint32_t*)(d + o_pos), (int32_t*)(d + o_dP),
                  (uint64_t*)(d + o_dv), (uint32_t*)(d + o_dr), (uint32_t*)(d + o_miss), d + o_found, nullptr};
    hipLaunchKernelGGL(k_tree_find_paths, dim3(nblk(k, 64)), dim3(64), 0, st, own->d_views.p, TreeFind{k, H, U.idx, U.pos, nullptr, U.missing, U.found});
    LAUNCH_CHECK();
    uint32_t missing = 0;
    HIPCHK(hipMemcpyAsync(&missing, d + o_miss, 4, hipMemcpyDeviceToHost, st));
    if (found_out) { found_out->resize(k); HIPCHK(hipMemcpyAsync(found_out->data(), d + o_found, k, hipMemcpyDeviceToHost, st)); }
    HIPCHK(hipStreamSynchronize(st));
    if (missing) return DAPOL_OK;                            // a new index: nothing has been written; the caller inserts or rebuilds
    TreePoison poison{own, true};                            // from here on the leaves and the levels above are rewritten in place
    if (test_knob("DAPOL_TEST_FAIL_UPDATE_MIDWAY")) return fail(DAPOL_ERR_HIP, "injected failure between the leaf update and the re-merge (test knob)");
    LAUNCH_DX(ctx->tv.digest, (k_tree_upd_leaves<DX>), dim3(nblk(k, 64)), dim3(64), 0, st, ctx->tv, own->d_views.p, U);
    LAUNCH_CHECK();
    if (H >= 1) RCCHK(rehash_paths(own, U));
    HIPCHK(hipStreamSynchronize(st));
    poison.armed = false;
    *done = true;
    return DAPOL_OK;
}

// Bytes of one level's spans in a buffer of capacity `cap` records (incremental insert / remove).
static size_t level_alt_bytes(size_t cap) { return align_up(cap * 8, 256) * 2 + align_up(cap * 32, 256) * 6 + align_up(cap * 4, 256) + align_up(cap, 256); }
// Levels 0 .. which.size() - 1 of a tree in new storage, filled but not yet the tree's: relayout_levels stages, adopt_levels swaps in.
struct StagedLevels {
    std::vector<LevelBuf> levels;
    uint64_t *leaf_idx, *leaf_v;
    uint32_t* leaf_r;
    std::vector<int> which;              // the LevelAlt buffer each level went to
};
// The storage level t moves into when it is rewritten out of place: whichever of its two LevelAlt buffers it does not live in now,
// grown to hold n_new records.  S.levels[t] (and, for level 0, the leaf pointers) then point into it.
static hipError_t level_alt_next(dapol_tree_owned* own, int t, size_t n_new, StagedLevels& S) {
    auto& A = own->alt[t];
    const int dstb = A.cur == 0 ? 1 : 0;
    if (A.cap[dstb] < n_new) {
        const size_t cap = n_new + 4096 + n_new / 64;
        hipError_t e = A.buf[dstb].alloc(level_alt_bytes(cap));
        if (e != hipSuccess) return e;
        A.cap[dstb] = cap;
    }
    const size_t cap = A.cap[dstb];
    size_t o = 0;
    auto take = [&](size_t bytes) { uint8_t* p = A.buf[dstb].p + o; o += align_up(bytes, 256); return p; };
    LevelBuf& L = S.levels[t];
    uint64_t *idx = (uint64_t*)take(cap * 8), *vv = (uint64_t*)take(cap * 8);
    uint32_t* rr = (uint32_t*)take(cap * 32);
    if (t == 0) { S.leaf_idx = idx; S.leaf_v = vv; S.leaf_r = rr; }
    else { L.idx.p = idx; L.v.p = vv; L.r.p = rr; }
    L.C.p = (uint32_t*)take(cap * 32); L.H.p = (uint32_t*)take(cap * 32);
    L.padC.p = (uint32_t*)take(cap * 32); L.padH.p = (uint32_t*)take(cap * 32); L.padr.p = (uint32_t*)take(cap * 32);
    L.parent.p = (uint32_t*)take(cap * 4);
    L.has_pad.p = take(cap);
    L.n = n_new;
    S.which[t] = dstb;
    return hipSuccess;
}
// Rewrites the levels below max(gains.size(), losses.size()) into storage of their own: level t gains the nodes of gains[t] (old-layout
// lower bounds) and loses those of losses[t] (old positions) -- sorted device arrays, either list may be empty or missing -- with the
// level above's lists beside them for the parent pointers.  The tree itself is only read.
static int32_t relayout_levels(dapol_tree_owned* own, const std::vector<RelayoutDel>& gains, const std::vector<RelayoutDel>& losses, StagedLevels& S) {
    hipStream_t st = own->ctx->stream;
    const int n_levels = (int)std::max(gains.size(), losses.size());
    const RelayoutDel none{};
    auto of = [&](const std::vector<RelayoutDel>& l, int t) -> const RelayoutDel& { return (size_t)t < l.size() ? l[t] : none; };
    if (own->alt.size() != own->levels.size()) own->alt.resize(own->levels.size());
    S.levels = own->levels;
    S.leaf_idx = own->leaf_idx; S.leaf_v = own->leaf_v; S.leaf_r = own->leaf_r;
    S.which.assign((size_t)n_levels, -1);
    for (int t = 0; t < n_levels; t++) HIPCHK(level_alt_next(own, t, own->levels[t].n + of(gains, t).n - of(losses, t).n, S));
    for (int t = 0; t < n_levels; t++) {
        const LevelView src = own->view(t), dst = level_view_of(S.levels[t], t, S.leaf_idx, S.leaf_v, S.leaf_r);
        const size_t n_old = own->levels[t].n;
        const RelayoutDel& ins = of(gains, t);
        if (n_old)
            hipLaunchKernelGGL(k_tree_relayout, dim3(nblk(n_old, 256)), dim3(256), 0, st, src, dst, n_old, ins.pos, ins.n, ins.next_pos, ins.n_next, 0, of(losses, t));
        LAUNCH_CHECK();
    }
    return DAPOL_OK;
}
// The staged levels become the tree's (its TreePoison is armed by now); hv = the new views, as uploaded to d_views.
static int32_t adopt_levels(dapol_tree_owned* own, const StagedLevels& S, std::vector<LevelView>& hv) {
    for (size_t t = 0; t < S.which.size(); t++) { own->levels[t] = S.levels[t]; own->alt[t].cur = S.which[t]; }
    own->leaf_idx = S.leaf_idx; own->leaf_v = S.leaf_v; own->leaf_r = S.leaf_r;
    hv = own->views();
    HIPCHK(hipMemcpyAsync(own->d_views.p, hv.data(), hv.size() * sizeof(LevelView), hipMemcpyHostToDevice, own->ctx->stream));
    return DAPOL_OK;
}

// The tree's node counts from its level sizes: every parent has two children, and those that are not real are padding nodes.
static void recount_nodes(dapol_tree_owned* own) {
    own->n_real = 0;
    own->n_pad = 0;
    for (int t = 0; t <= own->height; t++) {
        own->n_real += own->levels[t].n;
        if (t < own->height) own->n_pad += 2 * (uint64_t)own->levels[t + 1].n - own->levels[t].n;
    }
}

// What k_tree_ins_plan returned for a batch (dapol_tree_insert plans once, whichever insert path then runs).
struct InsPlanRead {
    std::vector<uint32_t> m, pos;        // [k], [k][H + 1]
    uint32_t flag = 0;                   // bit 1: two chains share a new node; bit 2: an index is a leaf already
};
// I1 / J1: plans the k sorted indexes at d_idx into d_m | d_pos | d_flag (cleared by the caller) and reads the rows back.  all_levels:
// the search goes on to the root (J1) instead of ending at a leaf's first existing ancestor.  Nothing of the tree is written.
static int32_t run_insert_plan(dapol_tree_owned* own, size_t k, const uint64_t* d_idx, uint32_t* d_m, uint32_t* d_pos, uint32_t* d_flag, bool all_levels,
                               InsPlanRead& R) {
    hipStream_t st = own->ctx->stream;
    const size_t S1 = (size_t)own->height + 1;
    const TreeInsPlan P{k, own->height, d_idx, d_m, d_pos, d_flag};
    if (all_levels) hipLaunchKernelGGL(k_tree_ins_plan<false>, dim3(nblk(k, 64)), dim3(64), 0, st, own->d_views.p, P);
    else hipLaunchKernelGGL(k_tree_ins_plan<true>, dim3(nblk(k, 64)), dim3(64), 0, st, own->d_views.p, P);
    LAUNCH_CHECK();
    R.m.resize(k); R.pos.resize(k * S1);
    HIPCHK(hipMemcpyAsync(R.m.data(), d_m, k * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(R.pos.data(), d_pos, k * S1 * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&R.flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DAPOL_OK;
}
// The incremental path for NEW leaves (kernels_ctx_tree.h, "incremental insert"): E sorted, distinct, none of them in the tree.
// *done = false and nothing written when two new chains share a node (the caller rebuilds).  pre: the batch has been planned already
// (no chains shared, every index new); its rows hold what I1 would write.
static int32_t tree_insert_incremental(dapol_tree_owned* own, const HostLeaves& E, bool* done, const InsPlanRead* pre = nullptr) {
    *done = false;
    dapol_ctx* ctx = own->ctx;
    hipStream_t st = ctx->stream;
    const int H = own->height;
    const size_t k = E.idx.size(), S1 = (size_t)H + 1;
    if (H < 1 || own->levels[0].n + k > ((size_t)1 << 31)) return DAPOL_OK;
    EditScratch sc;
    const size_t o_idx = sc.take(k * 8), o_v = sc.take(k * 8), o_r = sc.take(k * 32), o_m = sc.take(k * 4), o_ins = sc.take(k * S1 * 4), o_new = sc.take(k * S1 * 4),
                 o_pos = sc.take(k * S1 * 4), o_dP = sc.take(k * 160, 16), o_dv = sc.take(k * 8), o_dr = sc.take(k * 32), o_lvl = sc.take(k * S1 * 4),
                 o_seed = sc.take(32), o_flag = sc.take(8);
    HIPCHK(sc.ensure(own));
    uint8_t* d = own->upd_scratch.p;
    std::vector<uint8_t> stage;
    RCCHK(upload_edits(own, E, stage));
    HIPCHK(hipMemcpyAsync(d + o_seed, own->pad_seed, 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d + o_flag, 0, 8, st));
    InsPlanRead planned;
    if (pre) HIPCHK(hipMemcpyAsync(d + o_m, pre->m.data(), k * 4, hipMemcpyHostToDevice, st));
    else {
        RCCHK(run_insert_plan(own, k, (const uint64_t*)(d + o_idx), (uint32_t*)(d + o_m), (uint32_t*)(d + o_ins), (uint32_t*)(d + o_flag), false, planned));
        if (planned.flag) return DAPOL_OK;                  // chains that share a node (or an index that exists): the rebuild handles it
        pre = &planned;
    }
    const std::vector<uint32_t>&hm = pre->m, &hins = pre->pos;
    const InsertPlan plan = plan_insert(k, H, hm.data(), hins.data());
    HIPCHK(hipMemcpyAsync(d + o_new, plan.newpos.data(), k * S1 * 4, hipMemcpyHostToDevice, st));
    if (!plan.lvl_flat.empty()) HIPCHK(hipMemcpyAsync(d + o_lvl, plan.lvl_flat.data(), plan.lvl_flat.size() * 4, hipMemcpyHostToDevice, st));
    // new storage for the levels that gain nodes, then move their existing nodes
    const uint32_t* d_lvl = (const uint32_t*)(d + o_lvl);
    std::vector<RelayoutDel> gains((size_t)plan.max_m);
    for (int t = 0; t < plan.max_m; t++) gains[t] = RelayoutDel{d_lvl + plan.lvl_off[t], plan.gained(t), d_lvl + plan.lvl_off[t + 1], plan.gained(t + 1)};
    StagedLevels staged;
    RCCHK(relayout_levels(own, gains, {}, staged));
    TreePoison poison{own, true};                            // the tree's own state changes from here on
    std::vector<LevelView> hv;
    RCCHK(adopt_levels(own, staged, hv));
    TreeInsArgs I{k, H, (const uint64_t*)(d + o_idx), (const uint64_t*)(d + o_v), (const uint32_t*)(d + o_r), (const uint32_t*)(d + o_m),
                  (const uint32_t*)(d + o_new), (uint32_t*)(d + o_pos), (int32_t*)(d + o_dP), (uint64_t*)(d + o_dv), (uint32_t*)(d + o_dr),
                  (const uint32_t*)(d + o_seed)};
    LAUNCH_DX(ctx->tv.digest, (k_tree_ins_chain<DX>), dim3((unsigned)k), dim3(64), 0, st, ctx->tv, own->d_views.p, I);
    LAUNCH_CHECK();
    TreeUpdArgs U{k, H, (const uint64_t*)(d + o_idx), (const uint64_t*)(d + o_v), (const uint32_t*)(d + o_r), (uint32_t*)(d + o_pos), (int32_t*)(d + o_dP),
                  (uint64_t*)(d + o_dv), (uint32_t*)(d + o_dr), (uint32_t*)(d + o_flag), nullptr, (const uint32_t*)(d + o_m)};
    RCCHK(rehash_paths(own, U));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t j = 0; j < k; j++) { own->n_real += hm[j]; own->n_pad += (uint64_t)hm[j] - 2; }     // m - 1 new padding nodes, one dropped
    poison.armed = false;
    *done = true;
    return DAPOL_OK;
}

// J1 of dapol_tree_insert (kernels_ctx_tree.h, "incremental insert, general"): where the new leaves E (sorted, distinct) would go at
// every level, which of them exist and whether chains share nodes.  Nothing of the tree is written.
static int32_t insert_plan_all(dapol_tree_owned* own, const HostLeaves& E, InsPlanRead& R) {
    hipStream_t st = own->ctx->stream;
    const size_t k = E.idx.size(), S1 = (size_t)own->height + 1;
    EditScratch sc;
    sc.take(k * 8);
    const size_t o_m = sc.take(k * 4), o_pos = sc.take(k * S1 * 4), o_flag = sc.take(8, 8);
    HIPCHK(sc.ensure(own));
    uint8_t* d = own->upd_scratch.p;
    HIPCHK(hipMemcpyAsync(d, E.idx.data(), k * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d + o_flag, 0, 8, st));
    return run_insert_plan(own, k, (const uint64_t*)d, (uint32_t*)(d + o_m), (uint32_t*)(d + o_pos), (uint32_t*)(d + o_flag), true, R);
}
// The general in-place path of dapol_tree_insert: E sorted, distinct, all new and in range, R = its plan rows; chains may share
// nodes.
static int32_t tree_insert_general(dapol_tree_owned* own, const HostLeaves& E, const InsPlanRead& R) {
    dapol_ctx* ctx = own->ctx;
    hipStream_t st = ctx->stream;
    const int H = own->height;
    const size_t k = E.idx.size();
    InsertGeneralPlan plan = plan_insert_general(H, k, E.idx.data(), R.m.data(), R.pos.data());
    memcpy(plan.flat.data(), own->pad_seed, 32);
    const size_t n_new = plan.n_pos.size(), n_pad = plan.pad_pos.size(), slots = plan.max_fresh;
    // leaves | the plan, one upload | extended points: fresh nodes (two halves, by level parity), new padding nodes
    EditScratch sc;
    sc.take(k * 48);
    const size_t o_flat = sc.take(plan.flat.size() * 4, 16), o_node = sc.take(2 * slots * 160, 16), o_pad = sc.take(n_pad * 160, 16);
    HIPCHK(sc.ensure(own));
    uint8_t* d = own->upd_scratch.p;
    std::vector<uint8_t> stage;
    RCCHK(upload_edits(own, E, stage));
    HIPCHK(hipMemcpyAsync(d + o_flat, plan.flat.data(), plan.flat.size() * 4, hipMemcpyHostToDevice, st));
    const uint32_t* dw = (const uint32_t*)(d + o_flat);
    std::vector<RelayoutDel> gains((size_t)plan.D);
    for (int t = 0; t < plan.D; t++)
        gains[t] = RelayoutDel{dw + plan.gain_off[t], (uint32_t)plan.gain[t].size(), dw + plan.gain_off[t + 1], (uint32_t)plan.gain[t + 1].size()};
    StagedLevels staged;
    RCCHK(relayout_levels(own, gains, {}, staged));
    TreePoison poison{own, true};                            // the tree's own state changes from here on
    std::vector<LevelView> hv;
    RCCHK(adopt_levels(own, staged, hv));
    if (test_knob("DAPOL_TEST_FAIL_INSERT_MIDWAY")) return fail(DAPOL_ERR_HIP, "injected failure between the relayout and the new nodes (test knob)");
    int32_t* node_ext = (int32_t*)(d + o_node);
    int32_t* pad_ext = (int32_t*)(d + o_pad);
    TreeInsGeneral G{n_new, k, dw + plan.lvl_off, dw + plan.pos_off, dw + plan.parent_off, dw + plan.sib_off, dw + plan.idx_lo_off, dw + plan.idx_hi_off,
                     dw + plan.leaf_off, (const uint64_t*)(d + k * 8), (const uint32_t*)(d + k * 16), node_ext};
    hipLaunchKernelGGL(k_tree_ins_struct, dim3(nblk(n_new, 64)), dim3(64), 0, st, own->d_views.p, G);
    LAUNCH_CHECK();
    LAUNCH_DX(ctx->tv.digest, (k_tree_ins_leaves<DX>), dim3(nblk(k, 64)), dim3(64), 0, st, ctx->tv, own->d_views.p, G);
    LAUNCH_CHECK();
    if (n_pad) {
        LAUNCH_DX(ctx->tv.digest, (k_tree_edit_pad<true, DX>), dim3(nblk(n_pad, 64)), dim3(64), 0, st, ctx->tv, own->d_views.p, n_pad, dw + plan.pad_lvl_off, dw + plan.pad_pos_off,
                           dw /* the pad seed */, pad_ext);
        LAUNCH_CHECK();
    }
    for (int t = 0; t < H; t++) {
        const size_t n = plan.merge[t + 1].size() / 5;
        if (!n) continue;
        LAUNCH_DX(ctx->tv.digest, (k_tree_edit_merge<true, DX>), dim3(nblk(n, 64)), dim3(64), 0, st, ctx->tv.digest, hv[t], hv[t + 1], n, dw + plan.merge_off[t + 1],
                           node_ext + (size_t)(t & 1) * slots * 40, node_ext + (size_t)((t + 1) & 1) * slots * 40, pad_ext);
        LAUNCH_CHECK();
    }
    HIPCHK(hipStreamSynchronize(st));
    recount_nodes(own);
    poison.armed = false;
    return DAPOL_OK;
}

// The in-place path of dapol_tree_remove (kernels_ctx_tree.h, "incremental remove"); si = the indexes, sorted and distinct.  An index
// that is not a leaf (DAPOL_ERR_UNKNOWN_LEAF) or a batch that holds every leaf (DAPOL_ERR_INVALID_ARGUMENT) is reported before anything
// has been written.
static int32_t tree_remove_incremental(dapol_tree_owned* own, const std::vector<uint64_t>& si) {
    dapol_ctx* ctx = own->ctx;
    hipStream_t st = ctx->stream;
    const int H = own->height;
    const size_t k = si.size(), S1 = (size_t)H + 1;
    // R0: idx | pos | has_pad | missing
    EditScratch sc;
    sc.take(k * 8);
    const size_t o_pos = sc.take(k * S1 * 4), o_hp = sc.take(k * S1), o_miss = sc.take(8, 8);
    HIPCHK(sc.ensure(own));
    uint8_t* d = own->upd_scratch.p;
    HIPCHK(hipMemcpyAsync(d, si.data(), k * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d + o_miss, 0, 8, st));
    TreeFind F{k, H, (const uint64_t*)d, (uint32_t*)(d + o_pos), d + o_hp, (uint32_t*)(d + o_miss), nullptr};
    hipLaunchKernelGGL(k_tree_find_paths, dim3(nblk(k, 64)), dim3(64), 0, st, own->d_views.p, F);
    LAUNCH_CHECK();
    uint32_t missing = 0;
    HIPCHK(hipMemcpyAsync(&missing, d + o_miss, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (missing) return fail(DAPOL_ERR_UNKNOWN_LEAF, "an index to remove is not a leaf of the tree (nothing was removed)");
    if (k >= own->levels[0].n) return fail(DAPOL_ERR_INVALID_ARGUMENT, "removing every leaf would leave an empty tree (nothing was removed)");
    std::vector<uint32_t> pos(k * S1);
    std::vector<uint8_t> hp(k * S1);
    HIPCHK(hipMemcpyAsync(pos.data(), d + o_pos, k * S1 * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hp.data(), d + o_hp, k * S1, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    RemovePlan plan = plan_remove(H, k, si.data(), pos.data(), hp.data());
    if (!plan.ok) return fail(DAPOL_ERR_INVALID_ARGUMENT, "internal: the root of a tree with leaves left died");
    // one upload: pad seed | dead lists | pad positions | merge pairs | pad levels
    memcpy(plan.flat.data(), own->pad_seed, 32);
    EditScratch up;
    up.take(plan.flat.size() * 4);
    const size_t o_lvl = up.take(plan.pad_lvl.size());
    HIPCHK(up.ensure(own));
    d = own->upd_scratch.p;
    const uint32_t* dw = (const uint32_t*)d;
    HIPCHK(hipMemcpyAsync(d, plan.flat.data(), o_lvl, hipMemcpyHostToDevice, st));
    if (!plan.pad_lvl.empty()) HIPCHK(hipMemcpyAsync(d + o_lvl, plan.pad_lvl.data(), plan.pad_lvl.size(), hipMemcpyHostToDevice, st));
    // R1: the levels that lose nodes, compacted into storage of their own (the tree's arrays are not touched yet)
    std::vector<RelayoutDel> losses((size_t)plan.D);
    for (int t = 0; t < plan.D; t++)
        losses[t] = RelayoutDel{dw + plan.dead_off[t], (uint32_t)plan.dead[t].size(), dw + plan.dead_off[t + 1], (uint32_t)plan.dead[t + 1].size()};
    StagedLevels staged;
    RCCHK(relayout_levels(own, {}, losses, staged));
    TreePoison poison{own, true};                            // the tree's own state changes from here on
    if (test_knob("DAPOL_TEST_FAIL_REMOVE_MIDWAY")) return fail(DAPOL_ERR_HIP, "injected failure between the compaction and the re-merge (test knob)");
    std::vector<LevelView> hv;
    RCCHK(adopt_levels(own, staged, hv));
    // R2: the chain tops' siblings take their padding nodes; R3: the touched survivors, bottom-up
    if (!plan.pad_pos.empty()) {
        LAUNCH_DX(ctx->tv.digest, (k_tree_edit_pad<false, DX>), dim3(nblk(plan.pad_pos.size(), 64)), dim3(64), 0, st, ctx->tv, own->d_views.p, plan.pad_pos.size(),
                           (const uint8_t*)(d + o_lvl), dw + plan.pad_off, dw /* the pad seed */, (int32_t*)nullptr);
        LAUNCH_CHECK();
    }
    for (int t = 0; t < H; t++) {
        const size_t n = plan.merge[t + 1].size() / 2;
        if (!n) continue;
        LAUNCH_DX(ctx->tv.digest, (k_tree_edit_merge<false, DX>), dim3(nblk(n, 64)), dim3(64), 0, st, ctx->tv.digest, hv[t], hv[t + 1], n, dw + plan.merge_off[t + 1],
                           (const int32_t*)nullptr, (int32_t*)nullptr, (const int32_t*)nullptr);
        LAUNCH_CHECK();
    }
    HIPCHK(hipStreamSynchronize(st));
    recount_nodes(own);
    poison.armed = false;
    return DAPOL_OK;
}

// The rebuild path of dapol_tree_update and dapol_tree_remove: the tree's leaf set comes to the host, the edits are merged into it
// (v == nullptr: removed from it; then leaf_idx is sorted and distinct), and the level-parallel build runs again over the result with
// the tree's own pad seed and shape -- one pass for the whole batch instead of k root-to-leaf walks.  An error leaves the old tree.
// must_be_new (dapol_tree_insert; leaf_idx distinct): an edit of an index that is a leaf already is refused instead of replacing it.
// drop (dapol_tree_apply; leaf_idx distinct): edit u with drop[u] != 0 removes the leaf at its index -- which must be one -- and the
// others put theirs; a result with no leaf is refused; was_leaf[u] (may be null) = whether leaf_idx[u] was a leaf before.
static int32_t tree_rebuild_edited(dapol_tree_owned* own, size_t k, const uint64_t* leaf_idx, const uint64_t* v, const uint8_t* r32, bool must_be_new = false,
                                   const uint8_t* drop = nullptr, std::vector<uint8_t>* was_leaf = nullptr) {
    hipStream_t st = own->ctx->stream;
    const size_t n0 = own->levels[0].n;
    HostLeaves old, cur;
    old.idx.resize(n0); old.v.resize(n0); old.r.resize(n0 * 32);
    HIPCHK(hipMemcpyAsync(old.idx.data(), own->leaf_idx, n0 * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(old.v.data(), own->leaf_v, n0 * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(old.r.data(), own->leaf_r, n0 * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!v) {
        for (size_t i = 0; i < k; i++)
            if (!std::binary_search(old.idx.begin(), old.idx.end(), leaf_idx[i])) return fail(DAPOL_ERR_UNKNOWN_LEAF, "an index to remove is not a leaf of the tree (nothing was removed)");
        if (k >= n0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "removing every leaf would leave an empty tree (nothing was removed)");
    }
    if (must_be_new)
        for (size_t i = 0; i < k; i++)
            if (std::binary_search(old.idx.begin(), old.idx.end(), leaf_idx[i])) return fail(DAPOL_ERR_INVALID_ARGUMENT, "an index to insert is already a leaf of the tree (nothing was inserted)");
    if (drop)
        for (size_t i = 0; i < k; i++)
            if (drop[i] && !std::binary_search(old.idx.begin(), old.idx.end(), leaf_idx[i]))
                return fail(DAPOL_ERR_UNKNOWN_LEAF, "an index to remove is not a leaf of the tree (nothing was applied)");
    merge_leaf_edits(old, k, leaf_idx, v, r32, cur, drop);
    if (drop && cur.idx.empty()) return fail(DAPOL_ERR_INVALID_ARGUMENT, "the edit would leave an empty tree (nothing was applied)");
    if (was_leaf) {
        was_leaf->resize(k);
        for (size_t i = 0; i < k; i++) (*was_leaf)[i] = std::binary_search(old.idx.begin(), old.idx.end(), leaf_idx[i]);
    }
    dapol_tree_owned fresh;
    int32_t rc = tree_build_owned(own->ctx, own->index_bits, own->shard_bits, cur.idx.size(), cur.idx.data(), cur.v.data(), cur.r.data(), own->pad_seed, nullptr, 0, &fresh);
    if (rc != DAPOL_OK) return rc;
    fresh.holds_ctx = own->holds_ctx;
    *own = std::move(fresh);
    own->last_update_path = 0;
    return DAPOL_OK;
}
// dapol_options::update_incremental_max as the in-place paths read it (0 = none in place).
static size_t incremental_max(const dapol_ctx* ctx) {
    if (const char* e = knob("DAPOL_UPDATE_INCREMENTAL_MAX")) return (size_t)atoll(e);
    const int32_t o = ctx->opt.update_incremental_max;
    return o > 0 ? (size_t)o : o < 0 ? 0 : 65536;
}

// What dapol_tree_update and dapol_tree_remove share around their work.  Begin: the tree is usable, has a seed to draw padding nodes
// from and owns its leaves (`what` = "an update" / "a removal").  End: a 64-byte digest's hash chain is laid again over the edited
// tree -- the in-place paths re-hash 32-byte chains only, and after a rebuild once more costs a pass over the nodes and keeps this free
// of cases.
static int32_t tree_edit_begin(dapol_tree* tree, const char* what, dapol_tree_owned** own) {
    TREE_USABLE(tree);
    if (tree->tape_built)
        return fail(DAPOL_ERR_INVALID_ARGUMENT, (std::string("the tree was built from a padding tape: ") + what + " may need draws the tape does not hold; build it again").c_str());
    *own = static_cast<dapol_tree_owned*>(tree);
    if (!(*own)->leaves.idx.p) return fail(DAPOL_ERR_INVALID_ARGUMENT, "tree does not own its leaves (workload tree): rebuild the workload instead");
    HIPCHK(hipSetDevice(tree->ctx->device));
    return DAPOL_OK;
}
static int32_t tree_edit_end(dapol_tree* tree, int32_t rc) {
    if (rc || !ctx_wide(tree->ctx)) return rc;
    rc = tree_hash_wide(tree);
    if (rc) tree->invalid = true;
    return rc;
}

// New leaves go in place when there are at most 4,096 of them, all below 2^index_bits and (shard trees) under the shard's prefix;
// what is out of range is left to the rebuild, which reports the error.
static int32_t leaves_in_range(dapol_tree_owned* own, const HostLeaves& fresh, bool* ok);
static int32_t insertable_in_place(dapol_tree_owned* own, const HostLeaves& fresh, bool* ok) {
    *ok = false;
    if (fresh.idx.empty() || fresh.idx.size() > 4096 || own->height < 1 || knob("DAPOL_NO_INCREMENTAL_INSERT")) return DAPOL_OK;
    return leaves_in_range(own, fresh, ok);
}
static int32_t leaves_in_range(dapol_tree_owned* own, const HostLeaves& fresh, bool* ok) {
    *ok = false;
    for (uint64_t x : fresh.idx) if (own->index_bits < 64 && (x >> own->index_bits)) return DAPOL_OK;
    if (own->shard_bits) {
        uint64_t first = 0;
        HIPCHK(hipMemcpy(&first, own->leaf_idx, 8, hipMemcpyDeviceToHost));
        const int sh = own->index_bits - own->shard_bits;
        for (uint64_t x : fresh.idx) if ((x >> sh) != (first >> sh)) return DAPOL_OK;
    }
    *ok = true;
    return DAPOL_OK;
}
// Dapol::update (src/dapol/mod.rs:211-213) for k leaves, applied in input order: a leaf is inserted, or replaces the one already at
// its index.  Padding nodes are keyed by position, so the updated tree is exactly what dapol_tree_build gives for the resulting leaf
// set, whichever path makes it.  Up to DAPOL_UPDATE_INCREMENTAL_MAX edits (default 65,536, and at most an eighth of the leaves) are
// applied in place: replacements keep the structure (what smtree's update does to ONE leaf: re-merge its root-to-leaf path); new
// leaves whose chains are disjoint are inserted first (the level arrays that gain nodes are rewritten in order, nothing is recomputed
// for the nodes that merely move).  Anything else -- a big batch, new chains that share a node -- takes the rebuild.
static int32_t tree_update_impl(dapol_tree_owned* own, size_t k, const uint64_t* leaf_idx, const uint64_t* v, const uint8_t* r32) {
    const size_t n0 = own->levels[0].n;
    if (k <= incremental_max(own->ctx) && k <= n0 / 8 + 1 && n0 > 0) {
        HostLeaves E, fresh, existing;
        for (uint32_t u : sorted_last_wins(k, leaf_idx)) E.push(leaf_idx[u], v[u], r32 + (size_t)u * 32);
        bool done = false, insertable = false;
        std::vector<uint8_t> found;
        int32_t rc = tree_update_incremental(own, E, &done, &found);
        if (rc != DAPOL_OK) return rc;
        if (done) { own->last_update_path = 1; return DAPOL_OK; }
        // Some indexes are new: nothing has been written yet.
        for (size_t b = 0; b < E.idx.size(); b++) (found[b] ? existing : fresh).push(E.idx[b], E.v[b], E.r.data() + b * 32);
        rc = insertable_in_place(own, fresh, &insertable);
        if (rc == DAPOL_OK && insertable) rc = tree_insert_incremental(own, fresh, &done);
        if (rc != DAPOL_OK) return rc;
        if (done) {
            own->last_update_path = 2;
            if (existing.idx.empty()) return DAPOL_OK;
            rc = tree_update_incremental(own, existing, &done);
            // the inserts are in: whatever stops the replacements now -- also an error BEFORE their first write, which would leave a
            // consistent but half-updated tree -- is a failed in-place update; the tree is refused from here on
            if (rc != DAPOL_OK) { own->invalid = true; return rc; }
            if (done) { own->last_update_path = 3; return DAPOL_OK; }
            own->invalid = true;                     // the new leaves are in, the replacements are not
            return fail(DAPOL_ERR_INVALID_ARGUMENT, "internal: a leaf found before the insert was not found after it");
        }
    }
    return tree_rebuild_edited(own, k, leaf_idx, v, r32);
}
int32_t dapol_tree_update(dapol_tree* tree, size_t k, const uint64_t* leaf_idx, const uint64_t* v, const uint8_t* r32) {
    if (!tree || (k && (!leaf_idx || !v || !r32))) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (k == 0) return DAPOL_OK;
    dapol_tree_owned* own = nullptr;
    int32_t rc = tree_edit_begin(tree, "an update", &own);
    return rc ? rc : tree_edit_end(tree, tree_update_impl(own, k, leaf_idx, v, r32));
}
// What the last dapol_tree_update / dapol_tree_insert / dapol_tree_remove on this tree did: 0 = rebuilt the tree, 1 = replaced existing
// leaves in place, 2 = inserted new leaves in place (disjoint chains), 3 = both, 4 = removed leaves in place, 5 = inserted new leaves in
// place by the general path (dapol_tree_insert only), 6 = applied in place by dapol_tree_apply.  (Diagnostics: the result is the same
// tree whichever path ran.)
int32_t dapol_tree_last_update_path(dapol_tree* tree, int32_t* path) {
    if (!tree || !path) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    *path = static_cast<dapol_tree_owned*>(tree)->last_update_path;
    return DAPOL_OK;
}

// In place up to update_incremental_max removals (and at most an eighth of the leaves), as dapol_tree_update; otherwise the
// surviving leaves are built again, which is bit for bit the same tree.
static int32_t tree_remove_impl(dapol_tree_owned* own, size_t k, const uint64_t* leaf_idx) {
    std::vector<uint64_t> si(leaf_idx, leaf_idx + k);
    std::sort(si.begin(), si.end());
    si.erase(std::unique(si.begin(), si.end()), si.end());
    if (own->height >= 1 && si.size() <= incremental_max(own->ctx) && si.size() <= own->levels[0].n / 8 + 1) {
        int32_t rc = tree_remove_incremental(own, si);
        if (rc != DAPOL_OK) return rc;
        own->last_update_path = 4;
        return DAPOL_OK;
    }
    return tree_rebuild_edited(own, si.size(), si.data(), nullptr, nullptr);
}
int32_t dapol_tree_remove(dapol_tree* tree, size_t k, const uint64_t* leaf_idx) {
    if (!tree || (k && !leaf_idx)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (k == 0) return DAPOL_OK;
    dapol_tree_owned* own = nullptr;
    int32_t rc = tree_edit_begin(tree, "a removal", &own);
    return rc ? rc : tree_edit_end(tree, tree_remove_impl(own, k, leaf_idx));
}

// The general in-place insert is taken up to this many leaves (besides update_incremental_max and an eighth of the tree, the removal's
// gate).  Measured at 2^20 leaves, height 32 (profiles/tree_insert_2e20_h32.json, medians of 7): 16,384 random new leaves 14.5 ms against
// 80 ms for the forced rebuild; 65,536, the largest batch the default gate admits, 77 ms against 124 ms (spread of the rebuild 0.31,
// 39 ms) -- still ahead by more than that spread, so the cap stays where update_incremental_max is.  Where a later measurement finds
// path 5 no longer ahead of the rebuild by more than the rebuild's spread, this comes down to the largest measured k that is.
static const size_t INSERT_GENERAL_MAX = 65536;
// dapol_tree_insert: k NEW leaves, in any order, all or nothing.  The batch is planned once on the device (J1); an index that is a leaf
// already, or that occurs twice, is refused before anything is written.  Up to 4,096 leaves whose chains share no node take the
// disjoint-chain insert of dapol_tree_update (path 2: a wavefront per chain); any other batch inside the gate takes the general path
// (path 5); what is outside it -- or out of range, which the build reports -- is rebuilt (path 0).
static int32_t tree_insert_impl(dapol_tree_owned* own, size_t k, const uint64_t* leaf_idx, const uint64_t* v, const uint8_t* r32) {
    std::vector<size_t> ord(k);
    for (size_t i = 0; i < k; i++) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return leaf_idx[a] < leaf_idx[b]; });
    HostLeaves E;
    for (size_t b = 0; b < k; b++) {
        if (b && leaf_idx[ord[b]] == leaf_idx[ord[b - 1]]) return fail(DAPOL_ERR_INVALID_ARGUMENT, "an index occurs twice in the batch to insert (nothing was inserted)");
        E.push(leaf_idx[ord[b]], v[ord[b]], r32 + (size_t)ord[b] * 32);
    }
    const size_t n0 = own->levels[0].n;
    bool in_range = false;
    if (own->height >= 1 && k <= incremental_max(own->ctx) && k <= INSERT_GENERAL_MAX && k <= n0 / 8 + 1 && n0 + k <= ((size_t)1 << 31)) {
        int32_t rc = leaves_in_range(own, E, &in_range);
        if (rc != DAPOL_OK) return rc;
    }
    if (in_range) {
        InsPlanRead R;
        int32_t rc = insert_plan_all(own, E, R);
        if (rc != DAPOL_OK) return rc;
        if (R.flag & 2u) return fail(DAPOL_ERR_INVALID_ARGUMENT, "an index to insert is already a leaf of the tree (nothing was inserted)");
        bool done = false;
        if (k <= 4096 && !(R.flag & 1u)) {
            rc = tree_insert_incremental(own, E, &done, &R);
            if (rc != DAPOL_OK) return rc;
            if (done) { own->last_update_path = 2; return DAPOL_OK; }
        }
        rc = tree_insert_general(own, E, R);
        if (rc != DAPOL_OK) return rc;
        own->last_update_path = 5;
        return DAPOL_OK;
    }
    return tree_rebuild_edited(own, k, leaf_idx, v, r32, true);
}
int32_t dapol_tree_insert(dapol_tree* tree, size_t k, const uint64_t* leaf_idx, const uint64_t* v, const uint8_t* r32) {
    if (!tree || (k && (!leaf_idx || !v || !r32))) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (k == 0) return DAPOL_OK;
    dapol_tree_owned* own = nullptr;
    int32_t rc = tree_edit_begin(tree, "an insert", &own);
    return rc ? rc : tree_edit_end(tree, tree_insert_impl(own, k, leaf_idx, v, r32));
}

// The in-place path of dapol_tree_apply (kernels_ctx_tree.h, "mixed edit in place"): ux = the removed and the put indexes together,
// sorted and distinct, all in range; is_put[j] says which is which; E = the puts, sorted.  Everything the call can refuse -- a removal
// that is not a leaf, a result with no leaf -- is decided from A0's read-back, before the first write.  was_new[b] = whether put b
// (in E's order) is a new leaf.
static int32_t tree_apply_incremental(dapol_tree_owned* own, const std::vector<uint64_t>& ux, const std::vector<uint8_t>& is_put, const HostLeaves& E,
                                      std::vector<uint8_t>& was_new) {
    dapol_ctx* ctx = own->ctx;
    hipStream_t st = ctx->stream;
    const int H = own->height;
    const size_t k = ux.size(), n_put = E.idx.size(), S1 = (size_t)H + 1;
    // A0: idx | pos | flag
    EditScratch sc;
    sc.take(k * 8);
    const size_t o_pos = sc.take(k * S1 * 4), o_fl = sc.take(k * S1);
    HIPCHK(sc.ensure(own));
    uint8_t* d = own->upd_scratch.p;
    HIPCHK(hipMemcpyAsync(d, ux.data(), k * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_tree_apply_plan, dim3(nblk(k, 64)), dim3(64), 0, st, own->d_views.p, TreeApplyPlan{k, H, (const uint64_t*)d, (uint32_t*)(d + o_pos), d + o_fl});
    LAUNCH_CHECK();
    std::vector<uint32_t> lb(k * S1);
    std::vector<uint8_t> fl(k * S1);
    HIPCHK(hipMemcpyAsync(lb.data(), d + o_pos, k * S1 * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(fl.data(), d + o_fl, k * S1, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    size_t n_gone = 0, n_come = 0;
    for (size_t j = 0; j < k; j++) {
        const bool leaf = fl[j * S1] & 1;
        if (!is_put[j] && !leaf) return fail(DAPOL_ERR_UNKNOWN_LEAF, "an index to remove is not a leaf of the tree (nothing was applied)");
        n_gone += !is_put[j];
        n_come += is_put[j] && !leaf;
    }
    const size_t n0 = own->levels[0].n;
    if (n0 - n_gone + n_come == 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "the edit would leave an empty tree (nothing was applied)");
    ApplyPlan plan = plan_apply(H, k, ux.data(), is_put.data(), lb.data(), fl.data());
    if (!plan.ok) return fail(DAPOL_ERR_INVALID_ARGUMENT, "internal: the root of a tree with leaves left died");
    was_new = plan.put_new;
    memcpy(plan.flat.data(), own->pad_seed, 32);
    const size_t n_struct = plan.s_pos.size(), n_pad = plan.pad_pos.size(), slots = plan.max_slots;
    // the puts | the plan, one upload | extended points: touched nodes (two halves, by level parity), new padding nodes
    EditScratch up;
    up.take(n_put * 48);
    const size_t o_flat = up.take(plan.flat.size() * 4, 16), o_node = up.take(2 * slots * 160, 16), o_pad = up.take(n_pad * 160, 16);
    HIPCHK(up.ensure(own));
    d = own->upd_scratch.p;
    std::vector<uint8_t> stage;
    if (n_put) RCCHK(upload_edits(own, E, stage));
    HIPCHK(hipMemcpyAsync(d + o_flat, plan.flat.data(), plan.flat.size() * 4, hipMemcpyHostToDevice, st));
    const uint32_t* dw = (const uint32_t*)(d + o_flat);
    // A1: every level below the highest that changes, once, with what it gains and what it loses
    std::vector<RelayoutDel> gains((size_t)plan.D), losses((size_t)plan.D);
    for (int t = 0; t < plan.D; t++) {
        gains[t] = RelayoutDel{dw + plan.born_off[t], (uint32_t)plan.born[t].size(), dw + plan.born_off[t + 1], (uint32_t)plan.born[t + 1].size()};
        losses[t] = RelayoutDel{dw + plan.dead_off[t], (uint32_t)plan.dead[t].size(), dw + plan.dead_off[t + 1], (uint32_t)plan.dead[t + 1].size()};
    }
    StagedLevels staged;
    RCCHK(relayout_levels(own, gains, losses, staged));
    TreePoison poison{own, true};                            // the tree's own state changes from here on
    std::vector<LevelView> hv;
    RCCHK(adopt_levels(own, staged, hv));
    if (test_knob("DAPOL_TEST_FAIL_APPLY_MIDWAY")) return fail(DAPOL_ERR_HIP, "injected failure between the relayout and the touched nodes (test knob)");
    int32_t* node_ext = (int32_t*)(d + o_node);
    int32_t* pad_ext = (int32_t*)(d + o_pad);
    if (n_struct) {
        const TreeApplyStruct G{n_struct, dw + plan.lvl_off, dw + plan.pos_off, dw + plan.parent_off, dw + plan.flag_off, dw + plan.idx_lo_off, dw + plan.idx_hi_off};
        hipLaunchKernelGGL(k_tree_apply_struct, dim3(nblk(n_struct, 64)), dim3(64), 0, st, own->d_views.p, G);
        LAUNCH_CHECK();
    }
    if (n_put) {                                             // A3 is the insert's J4: only the leaf's position, liability and slot are read
        const TreeInsGeneral G{0, n_put, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, dw + plan.put_off, (const uint64_t*)(d + n_put * 8),
                               (const uint32_t*)(d + n_put * 16), node_ext};
        LAUNCH_DX(ctx->tv.digest, (k_tree_ins_leaves<DX>), dim3(nblk(n_put, 64)), dim3(64), 0, st, ctx->tv, own->d_views.p, G);
        LAUNCH_CHECK();
    }
    if (n_pad) {
        LAUNCH_DX(ctx->tv.digest, (k_tree_edit_pad<true, DX>), dim3(nblk(n_pad, 64)), dim3(64), 0, st, ctx->tv, own->d_views.p, n_pad, dw + plan.pad_lvl_off, dw + plan.pad_pos_off,
                           dw /* the pad seed */, pad_ext);
        LAUNCH_CHECK();
    }
    for (int t = 0; t < H; t++) {
        const size_t n = plan.merge[t + 1].size() / 5;
        if (!n) continue;
        LAUNCH_DX(ctx->tv.digest, (k_tree_apply_merge<DX>), dim3(nblk(n, 64)), dim3(64), 0, st, ctx->tv.digest, hv[t], hv[t + 1], n, dw + plan.merge_off[t + 1],
                           node_ext + (size_t)(t & 1) * slots * 40, node_ext + (size_t)((t + 1) & 1) * slots * 40, pad_ext);
        LAUNCH_CHECK();
    }
    HIPCHK(hipStreamSynchronize(st));
    recount_nodes(own);
    poison.armed = false;
    return DAPOL_OK;
}

// The in-place path of dapol_tree_apply is taken up to this many edits (removals and puts together; besides update_incremental_max
// and an eighth of the tree): the general insert's cap, whose stages this path shares.  Measured at 2^20 leaves, height 32
// (profiles/tree_apply_2e20_h32.json, medians of 7): 3 x 4,096 edits 13.6 ms against 81.5 ms for the forced rebuild; 3 x 21,845 = 65,535,
// the largest batch the gate admits, 82.9 ms against 92.3 ms (max - min of the rebuild 8.8 ms) -- still ahead by more than that, by a
// thin margin, so the cap stays.  Where a later measurement finds path 6 no longer ahead of the forced rebuild by more than the
// rebuild's max - min at the cap, this comes down to the largest measured batch that is.
static const size_t APPLY_IN_PLACE_MAX = INSERT_GENERAL_MAX;
// dapol_tree_apply: the leaf set becomes (old - removed) + puts, all or nothing.  What the host can refuse alone -- an index twice
// among the puts, an index both removed and put -- is refused first; the rest is decided from one planning launch (in place) or from
// the leaf set on the host (rebuild), with the same rules and codes in the same order: a removal that is not a leaf, then a result
// with no leaf or a put out of range (the two exclude each other).
static int32_t tree_apply_impl(dapol_tree_owned* own, size_t n_remove, const uint64_t* remove_idx, size_t n_put, const uint64_t* put_idx, const uint64_t* put_v,
                               const uint8_t* put_r32, uint8_t* put_was_new) {
    std::vector<uint64_t> rm(remove_idx, remove_idx + n_remove);
    std::sort(rm.begin(), rm.end());
    rm.erase(std::unique(rm.begin(), rm.end()), rm.end());
    std::vector<uint32_t> ord(n_put);
    for (size_t i = 0; i < n_put; i++) ord[i] = (uint32_t)i;
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return put_idx[a] < put_idx[b]; });
    HostLeaves E;
    for (size_t b = 0; b < n_put; b++) {
        const uint64_t x = put_idx[ord[b]];
        if (b && x == put_idx[ord[b - 1]]) return fail(DAPOL_ERR_INVALID_ARGUMENT, "an index occurs twice among the puts (nothing was applied)");
        if (std::binary_search(rm.begin(), rm.end(), x))
            return fail(DAPOL_ERR_INVALID_ARGUMENT, "an index is both removed and put: a replacement is a put alone (nothing was applied)");
        E.push(x, put_v[ord[b]], put_r32 + (size_t)ord[b] * 32);
    }
    // the union, sorted: rm and E.idx are sorted and disjoint
    const size_t k = rm.size() + n_put;
    HostLeaves U;
    std::vector<uint8_t> is_put;
    U.idx.reserve(k); is_put.reserve(k);
    for (size_t a = 0, b = 0; a < rm.size() || b < n_put;) {
        const bool put = a >= rm.size() || (b < n_put && E.idx[b] < rm[a]);
        U.idx.push_back(put ? E.idx[b++] : rm[a++]);
        is_put.push_back(put);
    }
    const size_t n0 = own->levels[0].n;
    bool in_range = false;
    if (own->height >= 1 && k <= incremental_max(own->ctx) && k <= APPLY_IN_PLACE_MAX && k <= n0 / 8 + 1 && n0 + n_put <= ((size_t)1 << 31))
        RCCHK(leaves_in_range(own, U, &in_range));
    std::vector<uint8_t> was_new;                            // per put, in E's order
    if (in_range) {
        RCCHK(tree_apply_incremental(own, U.idx, is_put, E, was_new));
        own->last_update_path = 6;
    } else {
        // one merged leaf set, built once: the union in order, the puts with their liabilities
        std::vector<uint64_t> v(k, 0);
        std::vector<uint8_t> r(k * 32, 0), drop(k), was_leaf;
        for (size_t j = 0, b = 0; j < k; j++) {
            drop[j] = !is_put[j];
            if (is_put[j]) { v[j] = E.v[b]; memcpy(r.data() + j * 32, E.r.data() + b * 32, 32); b++; }
        }
        RCCHK(tree_rebuild_edited(own, k, U.idx.data(), v.data(), r.data(), false, drop.data(), &was_leaf));
        for (size_t j = 0; j < k; j++) if (is_put[j]) was_new.push_back(!was_leaf[j]);
    }
    if (put_was_new) for (size_t b = 0; b < n_put; b++) put_was_new[ord[b]] = was_new[b];
    return DAPOL_OK;
}
int32_t dapol_tree_apply(dapol_tree* tree, size_t n_remove, const uint64_t* remove_idx, size_t n_put, const uint64_t* put_idx, const uint64_t* put_v,
                         const uint8_t* put_r32, uint8_t* put_was_new) {
    if (!tree || (n_remove && !remove_idx) || (n_put && (!put_idx || !put_v || !put_r32))) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (n_remove == 0 && n_put == 0) return DAPOL_OK;
    dapol_tree_owned* own = nullptr;
    int32_t rc = tree_edit_begin(tree, "an apply", &own);
    return rc ? rc : tree_edit_end(tree, tree_apply_impl(own, n_remove, remove_idx, n_put, put_idx, put_v, put_r32, put_was_new));
}

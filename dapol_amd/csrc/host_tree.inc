// The sparse Merkle sum tree on the host side: its storage, the level-parallel build (phased for small trees, level-wise otherwise),
// the 64-byte hash chain, the three build entry points, the queries and the path gather.  The edit paths (update, insert, remove)
// are in host_tree_edit.inc.  Included by dapol_hip.hip, before everything that proves from a tree.
#include "tree_edit_plan.inc"

template <typename T>
struct Span { T* p = nullptr; };             // a view into the tree's arena (same `.p` spelling as DevBuf)
struct LevelBuf {
    size_t n = 0;                            // real nodes of the level (the host-side bound while the build is in flight)
    Span<uint64_t> idx, v;
    Span<uint32_t> C, H, r, padC, padH, padr, parent;
    Span<uint8_t> has_pad;
};
// The kernels' view of level t: level 0 reads idx / v / r from the leaf arrays (which may be the caller's), the others from L.
static LevelView level_view_of(const LevelBuf& L, int t, uint64_t* leaf_idx, uint64_t* leaf_v, uint32_t* leaf_r) {
    LevelView lv;
    lv.n = L.n;
    lv.idx = t == 0 ? leaf_idx : L.idx.p; lv.v = t == 0 ? leaf_v : L.v.p; lv.r = t == 0 ? leaf_r : L.r.p;
    lv.C = L.C.p; lv.H = L.H.p; lv.padC = L.padC.p; lv.padH = L.padH.p; lv.padr = L.padr.p; lv.has_pad = L.has_pad.p; lv.parent = L.parent.p; lv.ext = nullptr;
    return lv;
}

// Proof stores (host_store.inc) that live on a tree.  The count belongs to the HANDLE: a rebuild move-assigns a fresh tree over this one
// (host_tree_edit.inc), and assignment leaves the count where it is.
struct StoreCount {
    int n = 0;
    StoreCount() = default;
    StoreCount(const StoreCount&) {}
    StoreCount& operator=(const StoreCount&) { return *this; }
};
struct dapol_tree {
    dapol_ctx* ctx = nullptr;
    int height = 0;
    std::vector<LevelBuf> levels;      // 0 = leaves .. height = root
    DevBuf<uint8_t> arena;             // every level's arrays: ONE allocation per build
    // level 0 may borrow caller-resident device arrays (workload path)
    uint64_t *leaf_idx = nullptr, *leaf_v = nullptr;
    uint32_t* leaf_r = nullptr;
    uint64_t n_pad = 0, n_real = 0;
    int index_bits = 0, shard_bits = 0;          // what the tree was built with (dapol_tree_update rebuilds with the same)
    uint8_t pad_seed[32] = {0};
    bool invalid = false;              // an in-place update failed after its first write: root and leaves may disagree; every call refuses the tree
    bool tape_built = false;           // dapol_tree_build_tape: the padding draws came from a caller's tape (no seed to make further ones from)
    DevBuf<LevelView> d_views;         // view(0..height) on the device, for kernels that walk several levels
    // 64-byte node hashes (a Blake2b context): the hash chain laid over the built tree (tree_hash_wide), per level H16[n] | padH16[n]
    DevBuf<uint32_t> wide;
    std::vector<WideView> wviews;      // host copy: pointers into `wide`
    DevBuf<WideView> d_wviews;
    StoreCount stores;                 // live dapol_proof_store objects on this tree: dapol_tree_destroy refuses while there is one
    LevelView view(int k, int32_t* ext = nullptr) { LevelView lv = level_view_of(levels[k], k, leaf_idx, leaf_v, leaf_r); lv.ext = ext; return lv; }
    std::vector<LevelView> views() { std::vector<LevelView> hv; for (int k = 0; k <= height; k++) hv.push_back(view(k)); return hv; }
};
struct dapol_tree_owned : dapol_tree {
    struct { DevBuf<uint64_t> idx, v; DevBuf<uint32_t> r; } leaves;     // empty when level 0 borrows the caller's device arrays (workload trees)
    DevBuf<uint8_t> upd_scratch; // the in-place edit paths' scratch (kept: an update must not pay for an allocation)
    // A level that gains or loses nodes (incremental insert / remove) is rewritten out of place into one of two buffers of its own
    // (ping-pong; the arena region it came from is simply left behind).  cur = which of the two holds the level now (-1: still in the arena).
    struct LevelAlt { DevBuf<uint8_t> buf[2]; size_t cap[2] = {0, 0}; int cur = -1; };
    std::vector<LevelAlt> alt;
    int last_update_path = 0;    // what the last dapol_tree_update / _insert / _remove / _apply did (dapol_tree_last_update_path)
    bool holds_ctx = false;      // API-created trees keep their context alive (workload trees live inside a workload that does)
};

// dapol_tree_update re-merges in place; an error between its first write and its last (a HIP failure) leaves a tree whose upper
// levels no longer match its leaves.  Such a tree is marked and every entry point refuses it, loudly, instead of proving from it.
#define TREE_USABLE(t)                                                                                                                                   \
    do {                                                                                                                                                 \
        if ((t) && (t)->invalid)                                                                                                                         \
            return fail(DAPOL_ERR_INVALID_ARGUMENT, "the tree was left inconsistent by an in-place update that failed midway: destroy it and build it again"); \
    } while (0)
struct TreePoison {                    // armed before the first write of an in-place update, disarmed when the last one has completed
    dapol_tree* t;
    bool armed = false;
    ~TreePoison() { if (armed) t->invalid = true; }
};

// The hash chain of a 64-byte digest over a tree whose structure, commitments and padding nodes are in place (after a build or an
// update): level 0 = D(C), then one launch per level (kernels_ctx_tree.h, "64-byte node hashes").  The whole chain is redone after
// every update -- a pass over the tree's nodes, milliseconds at the reference test's sizes; only the 32-byte digests have the
// incremental re-hash.
static int32_t tree_hash_wide(dapol_tree* t) {
    dapol_ctx* ctx = t->ctx;
    if (!ctx_wide(ctx)) return DAPOL_OK;
    hipStream_t st = ctx->stream;
    const int H = t->height;
    size_t words = 0;
    std::vector<size_t> off((size_t)H + 1);
    for (int k = 0; k <= H; k++) { off[k] = words; words += 2 * t->levels[k].n * 16; }
    if (t->wide.n < words) HIPCHK(t->wide.alloc(words + words / 8));
    t->wviews.resize((size_t)H + 1);
    for (int k = 0; k <= H; k++) t->wviews[k] = WideView{t->wide.p + off[k], t->wide.p + off[k] + t->levels[k].n * 16};
    if (t->d_wviews.n != t->wviews.size()) HIPCHK(t->d_wviews.alloc(t->wviews.size()));
    HIPCHK(hipMemcpyAsync(t->d_wviews.p, t->wviews.data(), t->wviews.size() * sizeof(WideView), hipMemcpyHostToDevice, st));
    const size_t n0 = t->levels[0].n;
    hipLaunchKernelGGL(k_wide_hash_leaves, dim3(nblk(n0, 256)), dim3(256), 0, st, n0, t->levels[0].C.p, t->wviews[0].H);
    LAUNCH_CHECK();
    for (int k = 0; k < H; k++) {
        LevelView cur = t->view(k);
        hipLaunchKernelGGL(k_wide_hash_level, dim3(nblk(cur.n, 256)), dim3(256), 0, st, cur, t->wviews[k], t->wviews[k + 1]);
        LAUNCH_CHECK();
    }
    HIPCHK(hipStreamSynchronize(st));              // (wviews is copied from a host vector that may be resized by the next call)
    return DAPOL_OK;
}

// ------------------------------------------------------------------------------------------------- build
// One arena for all levels, each sized by its bound; level 0 borrows idx / v / r.  The has_pad flags sit together at the end, zeroed.
static int32_t carve_arena(dapol_tree* t, const std::vector<size_t>& bound, hipStream_t st) {
    const int height = t->height;
    size_t need = 0, pad_total = 0;
    auto take = [&](size_t bytes) { size_t o = need; need += align_up(bytes, 256); return o; };
    std::vector<size_t> off((size_t)(height + 1) * 10);
    for (int k = 0; k <= height; k++) {
        const size_t c = bound[k];
        size_t* o = &off[(size_t)k * 10];
        o[0] = k ? take(c * 8) : 0; o[1] = k ? take(c * 8) : 0; o[2] = k ? take(c * 32) : 0;      // idx, v, r (level 0 borrows the caller's)
        o[3] = take(c * 32); o[4] = take(c * 32); o[5] = take(c * 32); o[6] = take(c * 32); o[7] = take(c * 32); o[8] = take(c * 4);
        pad_total += align_up(c, 256);
    }
    const size_t pad_at = need;
    need += pad_total;
    if (t->arena.n < need) HIPCHK(t->arena.alloc(need));      // (a workload hands the arena of its previous build on: no hipFree / hipMalloc per step)
    HIPCHK(hipMemsetAsync(t->arena.p + pad_at, 0, pad_total, st));
    size_t pad_off = pad_at;
    for (int k = 0; k <= height; k++) {
        LevelBuf& L = t->levels[k];
        const size_t* o = &off[(size_t)k * 10];
        uint8_t* a = t->arena.p;
        L.n = bound[k];
        if (k) { L.idx.p = (uint64_t*)(a + o[0]); L.v.p = (uint64_t*)(a + o[1]); L.r.p = (uint32_t*)(a + o[2]); }
        L.C.p = (uint32_t*)(a + o[3]); L.H.p = (uint32_t*)(a + o[4]); L.padC.p = (uint32_t*)(a + o[5]); L.padH.p = (uint32_t*)(a + o[6]);
        L.padr.p = (uint32_t*)(a + o[7]); L.parent.p = (uint32_t*)(a + o[8]);
        L.has_pad.p = a + pad_off;
        pad_off += align_up(bound[k], 256);
    }
    return DAPOL_OK;
}

// Small trees, by phases (kernels_ctx_tree.h, "small trees"): structure, all padding nodes, point sums level by level, all
// encodings, hashes level by level.  The extended points of every level are kept until the encodings are done.
static int32_t build_phased(dapol_ctx* ctx, dapol_tree* t, size_t n, const std::vector<size_t>& bound, const uint32_t* seed, uint32_t* cnt) {
    hipStream_t st = ctx->stream;
    const int height = t->height;
    std::vector<uint32_t> h_off((size_t)height + 2);
    size_t tot = 0;
    for (int k = 0; k <= height; k++) { h_off[k] = (uint32_t)tot; tot += bound[k]; }
    h_off[(size_t)height + 1] = (uint32_t)tot;
    const std::vector<LevelView> hv = t->views();
    // temporaries from the context's scratch (a fresh hipMalloc of a few MB costs more than the whole build)
    const size_t b_ext = align_up(tot * 160, 256), b_pad = align_up((size_t)h_off[height] * 160, 256), b_off = align_up(h_off.size() * 4, 256);
    HIPCHK(ctx->scratch.ensure(b_ext + b_pad + b_off));
    int32_t* const ext_all = (int32_t*)ctx->scratch.p;
    int32_t* const extpad_all = (int32_t*)((uint8_t*)ctx->scratch.p + b_ext);
    uint32_t* const d_off = (uint32_t*)((uint8_t*)ctx->scratch.p + b_ext + b_pad);
    if (t->d_views.n != hv.size()) HIPCHK(t->d_views.alloc(hv.size()));
    HIPCHK(hipMemcpyAsync(t->d_views.p, hv.data(), hv.size() * sizeof(LevelView), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_off, h_off.data(), h_off.size() * 4, hipMemcpyHostToDevice, st));
    // the leaves' commitments do not depend on the structure: they run on a side stream beside S and P
    ForkGuard fg(ctx);
    HIPCHK(hipEventRecord(ctx->ev_fork, st));
    HIPCHK(hipStreamWaitEvent(ctx->side[0], ctx->ev_fork, 0));
    fg.forked(0);
    LAUNCH_DX(ctx->tv.digest, (k_commit_hash<DX>), dim3(nblk(n, 64)), dim3(64), 0, ctx->side[0], ctx->tv, n, t->leaf_v, t->leaf_r, t->levels[0].C.p, t->levels[0].H.p, ext_all);
    LAUNCH_CHECK();
    HIPCHK(hipEventRecord(ctx->ev_join[0], ctx->side[0]));
    FAULT_AFTER_FORK("tree");
    hipLaunchKernelGGL(k_tree_structure_small, dim3(1), dim3(1024), 0, st, height, t->d_views.p, cnt);
    LAUNCH_CHECK();
    LAUNCH_DX(ctx->tv.digest, (k_tree_padding_all<DX>), dim3(nblk(h_off[height], 64)), dim3(64), 0, st, ctx->tv, t->d_views.p, height, cnt, d_off, seed, extpad_all);
    LAUNCH_CHECK();
    HIPCHK(hipStreamWaitEvent(st, ctx->ev_join[0], 0));
    fg.joined(0);
    for (int k = 0; k < height; k++) {
        hipLaunchKernelGGL(k_tree_sum_level, dim3(nblk(bound[k], 64)), dim3(64), 0, st, hv[k], hv[k + 1], k, cnt, ext_all + (size_t)h_off[k] * 40,
                           extpad_all + (size_t)h_off[k] * 40, ext_all + (size_t)h_off[k + 1] * 40);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_tree_compress_all, dim3(nblk(tot - h_off[1], 64)), dim3(64), 0, st, t->d_views.p, height, cnt, d_off, ext_all);
    LAUNCH_CHECK();
    for (int k = 0; k < height; k++) {
        LAUNCH_DX(ctx->tv.digest, (k_tree_hash_level<DX>), dim3(nblk(bound[k], 64)), dim3(64), 0, st, ctx->tv.digest, hv[k], hv[k + 1], k, cnt);
        LAUNCH_CHECK();
    }
    return DAPOL_OK;
}

// Level by level: flags, scan, merge.  The padding children of a level are made in a launch of their own (k_tree_pad_level) and the
// merge reads them back (k_tree_merge<1>): fused, the kernel needed 262 VGPRs + 6 AGPRs and 624 bytes of scratch per lane -- one
// wavefront per SIMD --; apart, 178 and 226 VGPRs, two wavefronts each: 2^20 leaves x height 32 in 36.0 ms instead of 43.8, same root
// (profiles/r6_tree_split_ab.txt).  Tape mode keeps the fused kernel (it reads the tape by rank); DAPOL_TREE_SPLIT=0 restores it.
static int32_t build_levelwise(dapol_ctx* ctx, dapol_tree* t, size_t n, const std::vector<size_t>& bound, const uint32_t* seed, uint32_t* cnt,
                               const PadTape& ptape) {
    hipStream_t st = ctx->stream;
    const int height = t->height;
    const bool split_pad = !ptape.draws && !(knob("DAPOL_TREE_SPLIT") && atoi(knob("DAPOL_TREE_SPLIT")) == 0);
    // temporaries out of the context's scratch (as the phased path): seven hipMalloc / hipFree pairs per build otherwise, and a
    // hipFree waits for the device
    struct { uint32_t *flag, *pos, *head, *bsums; int32_t *ext_a, *ext_b, *ext_pad; } tmp;
    {
        size_t need = 0;
        auto take = [&](size_t bytes) { size_t o = need; need += align_up(bytes, 256); return o; };
        const size_t o_flag = take(n * 4), o_pos = take(n * 4), o_head = take(n * 4), o_bs = take((nblk(n, 1024) + 1) * 4), o_a = take(n * 160), o_b = take(n * 160),
                     o_p = take(split_pad ? n * 160 : 16);
        HIPCHK(ctx->scratch.ensure(need));
        uint8_t* b = (uint8_t*)ctx->scratch.p;
        tmp.flag = (uint32_t*)(b + o_flag); tmp.pos = (uint32_t*)(b + o_pos); tmp.head = (uint32_t*)(b + o_head); tmp.bsums = (uint32_t*)(b + o_bs);
        tmp.ext_a = (int32_t*)(b + o_a); tmp.ext_b = (int32_t*)(b + o_b); tmp.ext_pad = (int32_t*)(b + o_p);
    }
    LAUNCH_DX(ctx->tv.digest, (k_commit_hash<DX>), dim3(nblk(n, 256)), dim3(256), 0, st, ctx->tv, n, t->leaf_v, t->leaf_r, t->levels[0].C.p, t->levels[0].H.p, tmp.ext_a);
    LAUNCH_CHECK();
    int32_t* ext_cur = tmp.ext_a;
    int32_t* ext_nxt = tmp.ext_b;
    for (int k = 0; k < height; k++) {                    // launches only: nothing here waits for the device
        LevelView cur = t->view(k, ext_cur);
        hipLaunchKernelGGL(k_tree_flags, dim3(nblk(bound[k], 256)), dim3(256), 0, st, cnt + k, cur.idx, tmp.flag);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(k_scan_block, dim3(nblk(bound[k], 1024)), dim3(256), 0, st, cnt + k, tmp.flag, tmp.pos, tmp.bsums);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(256), 0, st, cnt + k, tmp.bsums, cnt + k + 1);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(k_scan_finish, dim3(nblk(bound[k], 256)), dim3(256), 0, st, cnt + k, tmp.flag, tmp.pos, tmp.bsums, tmp.head);
        LAUNCH_CHECK();
        LevelView nxt = t->view(k + 1, k + 1 < height ? ext_nxt : nullptr);
        if (split_pad) {
            LAUNCH_DX(ctx->tv.digest, (k_tree_pad_level<DX>), dim3(nblk(bound[k + 1], 256)), dim3(256), 0, st, ctx->tv, cur, tmp.head, k, seed, cnt, tmp.ext_pad);
            LAUNCH_CHECK();
            LAUNCH_DX(ctx->tv.digest, (k_tree_merge<1, DX>), dim3(nblk(bound[k + 1], 256)), dim3(256), 0, st, ctx->tv, cur, nxt, tmp.head, k, seed, cnt, ptape, tmp.ext_pad);
        } else
            LAUNCH_DX(ctx->tv.digest, (k_tree_merge<0, DX>), dim3(nblk(bound[k + 1], 256)), dim3(256), 0, st, ctx->tv, cur, nxt, tmp.head, k, seed, cnt, ptape, (const int32_t*)nullptr);
        LAUNCH_CHECK();
        std::swap(ext_cur, ext_nxt);
    }
    return DAPOL_OK;
}

// Builds the tree from device-resident leaf arrays (d_idx sorted; d_r is masked in place), the 64-byte hash chain included.  The tree
// borrows the arrays: they must outlive it.
static int32_t tree_build_device(dapol_ctx* ctx, int index_bits, int shard_bits, size_t n, uint64_t* d_idx, uint64_t* d_v, uint32_t* d_r,
                                 const uint8_t pad_seed32[32], dapol_tree* t, const uint32_t* d_tape = nullptr, size_t tape_draws = 0) {
    hipStream_t st = ctx->stream;
    t->tape_built = d_tape != nullptr;
    const int height = index_bits - shard_bits;       // levels built on this GPU
    t->ctx = ctx;
    t->height = height;
    t->leaf_idx = d_idx; t->leaf_v = d_v; t->leaf_r = d_r;
    t->index_bits = index_bits; t->shard_bits = shard_bits;
    memcpy(t->pad_seed, pad_seed32, 32);
    t->levels.assign((size_t)height + 1, LevelBuf{});
    t->n_pad = t->n_real = 0;
    DevBuf<uint32_t> bad, seed, cnt;
    HIPCHK(bad.alloc(1)); HIPCHK(seed.alloc(8)); HIPCHK(cnt.alloc((size_t)height + 2));
    HIPCHK(hipMemsetAsync(bad.p, 0, 4, st));
    HIPCHK(hipMemcpyAsync(seed.p, pad_seed32, 32, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_tree_check_leaves, dim3(nblk(n, 256)), dim3(256), 0, st, n, d_idx, index_bits, height, bad.p);
    LAUNCH_CHECK();
    uint32_t h_bad = 0;
    HIPCHK(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));          // the one early wait: malformed input must not reach the level kernels
    if (h_bad) return fail(DAPOL_ERR_INVALID_ARGUMENT, "leaf indexes must be strictly increasing, below 2^height, and (shard build) share their top shard_bits bits");
    // Upper bound of every level's size, known on the host: a level has at most as many nodes as the one below and at most
    // 2^(levels above it) positions.  The actual sizes are computed on the device (cnt) and read back once, at the end.
    std::vector<size_t> bound((size_t)height + 1);
    bound[0] = n;
    for (int k = 0; k < height; k++) {
        const int bits_above = height - (k + 1);
        bound[k + 1] = bound[k];
        if (bits_above < 40 && ((size_t)1 << bits_above) < bound[k + 1]) bound[k + 1] = (size_t)1 << bits_above;
    }
    RCCHK(carve_arena(t, bound, st));
    const uint32_t n32 = (uint32_t)n;
    HIPCHK(hipMemcpyAsync(cnt.p, &n32, 4, hipMemcpyHostToDevice, st));
    const bool phased = n <= (size_t)TREE_SMALL_MAX && height >= 1 && !knob("DAPOL_TREE_LEVELWISE") && !d_tape;     // (tape mode: the level-wise kernel reads the tape)
    DevBuf<uint32_t> tape_short;
    HIPCHK(tape_short.alloc(1));
    HIPCHK(hipMemsetAsync(tape_short.p, 0, 4, st));
    const PadTape ptape{d_tape, (uint32_t)std::min<size_t>(tape_draws, 0xffffffffu), tape_short.p};
    int32_t rc = phased ? build_phased(ctx, t, n, bound, seed.p, cnt.p) : build_levelwise(ctx, t, n, bound, seed.p, cnt.p, ptape);
    if (rc) return rc;
    std::vector<uint32_t> h_cnt((size_t)height + 1);
    uint32_t h_short = 0;
    HIPCHK(hipMemcpyAsync(h_cnt.data(), cnt.p, ((size_t)height + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&h_short, tape_short.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_short) return fail(DAPOL_ERR_INVALID_ARGUMENT, "the padding tape is shorter than the tree's padding nodes (dapol_tree_padding_positions gives the count)");
    for (int k = 0; k <= height; k++) {
        t->levels[k].n = h_cnt[k];
        t->n_real += h_cnt[k];
        if (k < height) t->n_pad += 2 * (uint64_t)h_cnt[k + 1] - h_cnt[k];
    }
    const std::vector<LevelView> hv = t->views();
    if (t->d_views.n != hv.size()) HIPCHK(t->d_views.alloc(hv.size()));
    HIPCHK(hipMemcpy(t->d_views.p, hv.data(), hv.size() * sizeof(LevelView), hipMemcpyHostToDevice));
    return tree_hash_wide(t);
}

// Builds `t` over host leaves that it then owns (the three build entry points, and the rebuild of an edit).
static int32_t tree_build_owned(dapol_ctx* ctx, int index_bits, int shard_bits, size_t n, const uint64_t* leaf_idx, const uint64_t* v, const uint8_t* r32,
                                const uint8_t pad_seed32[32], const uint32_t* d_tape, size_t tape_draws, dapol_tree_owned* t) {
    if (n > ((size_t)1 << 31)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "at most 2^31 leaves per GPU (32-bit node positions); memory is the practical bound");
    HIPCHK(t->leaves.idx.alloc(n)); HIPCHK(t->leaves.v.alloc(n)); HIPCHK(t->leaves.r.alloc(n * 8));
    HIPCHK(hipMemcpyAsync(t->leaves.idx.p, leaf_idx, n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(t->leaves.v.p, v, n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(t->leaves.r.p, r32, n * 32, hipMemcpyHostToDevice, ctx->stream));
    return tree_build_device(ctx, index_bits, shard_bits, n, t->leaves.idx.p, t->leaves.v.p, t->leaves.r.p, pad_seed32, t, d_tape, tape_draws);
}
// A new tree of the C ABI: it owns its leaves and keeps its context alive.
static int32_t tree_create_owned(dapol_ctx* ctx, int index_bits, int shard_bits, size_t n, const uint64_t* leaf_idx, const uint64_t* v, const uint8_t* r32,
                                 const uint8_t pad_seed32[32], const uint32_t* d_tape, size_t tape_draws, dapol_tree** out) {
    dapol_tree_owned* t = new dapol_tree_owned();
    struct Guard { dapol_tree* t; ~Guard() { if (t) dapol_tree_destroy(t); } } guard{t};
    int32_t rc = tree_build_owned(ctx, index_bits, shard_bits, n, leaf_idx, v, r32, pad_seed32, d_tape, tape_draws, t);
    if (rc != DAPOL_OK) return rc;
    guard.t = nullptr;
    t->holds_ctx = true;
    ctx_retain(ctx);
    *out = t;
    return DAPOL_OK;
}

int32_t dapol_tree_build(dapol_ctx* ctx, int32_t height, size_t n, const uint64_t* leaf_idx, const uint64_t* v, const uint8_t* r32,
                         const uint8_t pad_seed32[32], int32_t enforce_sparsity, dapol_tree** out) {
    if (!ctx || !out || !pad_seed32 || (n && (!leaf_idx || !v || !r32))) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (height < 0 || height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    if (enforce_sparsity && ctx_wide(ctx))           // Dapol::new (src/dapol/mod.rs:101-103); new_blank + build (enforce_sparsity = 0) has no such check
        return fail(DAPOL_ERR_INVALID_DIGEST_SIZE, "digest size must be 32 bytes (DapolError::InvalidDigestSize)");
    if (enforce_sparsity && height < 64 && ((double)n * 2.0 > (double)(1ull << height) ))
        return fail(DAPOL_ERR_SPARSITY_TOO_SMALL, "2^height < 2 * number of liabilities");
    if (n == 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "empty leaf set");
    HIPCHK(hipSetDevice(ctx->device));
    return tree_create_owned(ctx, height, 0, n, leaf_idx, v, r32, pad_seed32, nullptr, 0, out);
}

// Padding nodes of the tree over the given (sorted, distinct) leaves, in TAPE order (tree_edit_plan.inc: padding_positions).
int32_t dapol_tree_padding_positions(int32_t height, size_t n, const uint64_t* leaf_idx, size_t* count, uint8_t* level, uint64_t* index) {
    if (!count || (n && !leaf_idx)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (height < 0 || height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    for (size_t i = 0; i < n; i++)
        if ((height < 64 && (leaf_idx[i] >> height)) || (i && leaf_idx[i] <= leaf_idx[i - 1]))
            return fail(DAPOL_ERR_INVALID_ARGUMENT, "leaf indexes must be strictly increasing and below 2^height");
    *count = padding_positions(height, n, leaf_idx, level, index);
    return DAPOL_OK;
}
// dapol_tree_build in TAPE mode: the padding nodes' blindings (Paddable::padding -> Scalar::random, src/dapol/node.rs:86-88) are read
// from `tape` -- tape_draws draws of 64 bytes, each reduced mod l, one per padding node in dapol_tree_padding_positions' order --
// instead of being derived from a seed.  With the draws a seed would give, the tree equals the seed-mode tree bit for bit.  A tree
// built from a tape has no seed to draw further padding nodes from: dapol_tree_update refuses it (build it again with a longer tape).
int32_t dapol_tree_build_tape(dapol_ctx* ctx, int32_t height, size_t n, const uint64_t* leaf_idx, const uint64_t* v, const uint8_t* r32,
                              const uint8_t* tape, size_t tape_draws, dapol_tree** out) {
    if (!ctx || !out || (n && (!leaf_idx || !v || !r32)) || (tape_draws && !tape)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (height < 0 || height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    if (n == 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "empty leaf set");
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf<uint32_t> dtape;
    HIPCHK(dtape.alloc(tape_draws * 16 + 16));
    if (tape_draws) HIPCHK(hipMemcpyAsync(dtape.p, tape, tape_draws * 64, hipMemcpyHostToDevice, ctx->stream));
    const uint8_t no_seed[32] = {0};
    return tree_create_owned(ctx, height, 0, n, leaf_idx, v, r32, no_seed, dtape.p, tape_draws, out);
}

int32_t dapol_tree_build_shard(dapol_ctx* ctx, int32_t total_height, int32_t shard_bits, size_t n, const uint64_t* leaf_idx,
                               const uint64_t* v, const uint8_t* r32, const uint8_t pad_seed32[32], dapol_tree** out) {
    if (!ctx || !out || !pad_seed32 || !n || !leaf_idx || !v || !r32) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (shard_bits) NEEDS_32_BYTE_DIGEST(ctx, "the sharded (multi-GPU) path");
    if (total_height < 0 || total_height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    if (shard_bits < 0 || shard_bits > total_height || shard_bits > 16) return fail(DAPOL_ERR_INVALID_ARGUMENT, "shard_bits out of range");
    HIPCHK(hipSetDevice(ctx->device));
    return tree_create_owned(ctx, total_height, shard_bits, n, leaf_idx, v, r32, pad_seed32, nullptr, 0, out);
}

int32_t dapol_tree_destroy(dapol_tree* tree) {
    if (!tree) return DAPOL_OK;
    if (tree->stores.n > 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "the tree still has a proof store: destroy the store first (nothing was destroyed)");
    dapol_tree_owned* own = static_cast<dapol_tree_owned*>(tree);
    dapol_ctx* ctx = own->holds_ctx ? tree->ctx : nullptr;
    if (tree->ctx) (void)hipSetDevice(tree->ctx->device);
    delete own;
    if (ctx) (void)dapol_ctx_destroy(ctx);
    return DAPOL_OK;
}

// ----------------------------------------------------------------------------------------------- queries
int32_t dapol_tree_root(dapol_tree* tree, uint8_t C32[32], uint8_t H32[32], uint64_t* v, uint8_t r32[32]) {
    if (!tree) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null tree");
    TREE_USABLE(tree);
    HIPCHK(hipSetDevice(tree->ctx->device));
    LevelView lv = tree->view(tree->height);
    if (C32) HIPCHK(hipMemcpy(C32, lv.C, 32, hipMemcpyDeviceToHost));
    if (H32) HIPCHK(hipMemcpy(H32, ctx_wide(tree->ctx) ? tree->wviews[tree->height].H : lv.H, ctx_hash_bytes(tree->ctx), hipMemcpyDeviceToHost));
    if (v) HIPCHK(hipMemcpy(v, lv.v, 8, hipMemcpyDeviceToHost));
    if (r32) HIPCHK(hipMemcpy(r32, lv.r, 32, hipMemcpyDeviceToHost));
    return DAPOL_OK;
}
int32_t dapol_tree_node_count(dapol_tree* tree, uint64_t* real_nodes, uint64_t* padding_nodes) {
    if (!tree) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null tree");
    TREE_USABLE(tree);
    if (real_nodes) *real_nodes = tree->n_real;
    if (padding_nodes) *padding_nodes = tree->n_pad;
    return DAPOL_OK;
}
static int32_t level_pad_flags(dapol_tree* tree, int level, std::vector<uint8_t>& hp) {
    LevelView lv = tree->view(level);
    hp.resize(lv.n);
    if (level == tree->height) { std::fill(hp.begin(), hp.end(), 0); return DAPOL_OK; }
    HIPCHK(hipMemcpy(hp.data(), lv.has_pad, lv.n, hipMemcpyDeviceToHost));
    return DAPOL_OK;
}
int32_t dapol_tree_level_size(dapol_tree* tree, int32_t level, uint64_t* n_real, uint64_t* n_pad) {
    if (!tree || level < 0 || level > tree->height) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad level");
    TREE_USABLE(tree);
    HIPCHK(hipSetDevice(tree->ctx->device));
    std::vector<uint8_t> hp;
    int32_t rc = level_pad_flags(tree, level, hp);
    if (rc) return rc;
    uint64_t np = 0;
    for (uint8_t f : hp) np += f;
    if (n_real) *n_real = hp.size();
    if (n_pad) *n_pad = np;
    return DAPOL_OK;
}
int32_t dapol_tree_level_nodes(dapol_tree* tree, int32_t level, uint64_t* idx, uint64_t* v, uint8_t* r32, uint8_t* C32, uint8_t* H32,
                               uint8_t* is_pad) {
    if (!tree || level < 0 || level > tree->height || !idx || !v || !r32 || !C32 || !H32 || !is_pad)
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad argument");
    TREE_USABLE(tree);
    HIPCHK(hipSetDevice(tree->ctx->device));
    LevelView lv = tree->view(level);
    size_t n = lv.n;
    std::vector<uint8_t> hp;
    int32_t rc = level_pad_flags(tree, level, hp);
    if (rc) return rc;
    HIPCHK(hipMemcpy(idx, lv.idx, n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(v, lv.v, n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(r32, lv.r, n * 32, hipMemcpyDeviceToHost));
    const bool wide = ctx_wide(tree->ctx);
    const size_t hb = ctx_hash_bytes(tree->ctx);
    HIPCHK(hipMemcpy(C32, lv.C, n * 32, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(H32, wide ? tree->wviews[level].H : lv.H, n * hb, hipMemcpyDeviceToHost));
    memset(is_pad, 0, n);
    std::vector<uint8_t> pc(n * 32), ph(n * hb), pr(n * 32);
    if (level < tree->height) {
        HIPCHK(hipMemcpy(pc.data(), lv.padC, n * 32, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ph.data(), wide ? tree->wviews[level].padH : lv.padH, n * hb, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(pr.data(), lv.padr, n * 32, hipMemcpyDeviceToHost));
    }
    size_t o = n;
    for (size_t i = 0; i < n; i++) {
        if (!hp[i]) continue;
        idx[o] = idx[i] ^ 1ull;
        v[o] = 0;
        memcpy(r32 + o * 32, pr.data() + i * 32, 32);
        memcpy(C32 + o * 32, pc.data() + i * 32, 32);
        memcpy(H32 + o * hb, ph.data() + i * hb, hb);
        is_pad[o] = 1;
        o++;
    }
    return DAPOL_OK;
}
// Gathers the siblings of b leaves into device buffers (any of which may be null).
static int32_t tree_paths_device(dapol_tree* tree, size_t b, const uint64_t* d_leaf_idx, PathOut out, uint32_t* d_pos, int n_upper = 0) {
    TREE_USABLE(tree);
    hipStream_t st = tree->ctx->stream;
    DevBuf<uint32_t> missing;
    HIPCHK(missing.alloc(1));
    HIPCHK(hipMemsetAsync(missing.p, 0, 4, st));
    LevelView l0 = tree->view(0);
    hipLaunchKernelGGL(k_tree_find_leaves, dim3(nblk(b, 256)), dim3(256), 0, st, b, d_leaf_idx, l0.n, l0.idx, d_pos, missing.p);
    LAUNCH_CHECK();
    uint32_t h_missing = 0;
    HIPCHK(hipMemcpyAsync(&h_missing, missing.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_missing) return fail(DAPOL_ERR_UNKNOWN_LEAF, "no liability at one of the requested leaves");
    if (ctx_wide(tree->ctx) && out.H) {            // 64-byte hashes: out.H is [b][height + n_upper][16], filled from the wide chain
        if (tree->height) {
            hipLaunchKernelGGL(k_wide_path_walk, dim3(nblk(b, 64)), dim3(64), 0, st, b, d_pos, tree->d_views.p, tree->d_wviews.p, tree->height, n_upper,
                               g_wire.siblings_leaf_first, out.H);
            LAUNCH_CHECK();
        }
        out.H = nullptr;
    }
    if (tree->height) {
        hipLaunchKernelGGL(k_tree_path_walk, dim3(nblk(b, 64)), dim3(64), 0, st, b, d_pos, tree->d_views.p, tree->height, n_upper, g_wire.siblings_leaf_first, out);
        LAUNCH_CHECK();
    }
    return DAPOL_OK;
}
int32_t dapol_tree_paths(dapol_tree* tree, size_t b, const uint64_t* leaf_idx, uint8_t* sib_C32, uint8_t* sib_H32, uint64_t* sib_v,
                         uint8_t* sib_r32) {
    WIRE_SCOPE();
    if (!tree || (b && !leaf_idx)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (b == 0) return DAPOL_OK;
    HIPCHK(hipSetDevice(tree->ctx->device));
    hipStream_t st = tree->ctx->stream;
    size_t h = (size_t)tree->height, tot = b * h;
    DevBuf<uint64_t> dl, dv;
    DevBuf<uint32_t> dC, dH, dr, dpos;
    HIPCHK(dl.alloc(b)); HIPCHK(dpos.alloc(b));
    HIPCHK(dC.alloc(tot * 8)); HIPCHK(dH.alloc(tot * (size_t)ctx_hw(tree->ctx))); HIPCHK(dr.alloc(tot * 8)); HIPCHK(dv.alloc(tot));
    HIPCHK(hipMemcpyAsync(dl.p, leaf_idx, b * 8, hipMemcpyHostToDevice, st));
    PathOut po{dC.p, dH.p, dv.p, dr.p};
    int32_t rc = tree_paths_device(tree, b, dl.p, po, dpos.p);
    if (rc) return rc;
    if (sib_C32) HIPCHK(hipMemcpyAsync(sib_C32, dC.p, tot * 32, hipMemcpyDeviceToHost, st));
    if (sib_H32) HIPCHK(hipMemcpyAsync(sib_H32, dH.p, tot * ctx_hash_bytes(tree->ctx), hipMemcpyDeviceToHost, st));
    if (sib_v) HIPCHK(hipMemcpyAsync(sib_v, dv.p, tot * 8, hipMemcpyDeviceToHost, st));
    if (sib_r32) HIPCHK(hipMemcpyAsync(sib_r32, dr.p, tot * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DAPOL_OK;
}

// ------------------------------------------------------------------------------ records outside a tree
int32_t dapol_padding_nodes(dapol_ctx* ctx, const uint8_t pad_seed32[32], size_t n, const uint8_t* level, const uint64_t* index, uint8_t* C32,
                            uint8_t* H32, uint8_t* r32) {
    if (!ctx || !pad_seed32 || (n && (!level || !index || !C32 || !H32 || !r32))) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return DAPOL_OK;
    for (size_t i = 0; i < n; i++)
        if (level[i] > 64) return fail(DAPOL_ERR_INVALID_ARGUMENT, "level must not exceed 64");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<uint32_t> seed, dC, dH, dr;
    DevBuf<uint8_t> dl;
    DevBuf<uint64_t> di;
    HIPCHK(seed.alloc(8)); HIPCHK(dC.alloc(n * 8)); HIPCHK(dH.alloc(n * 8)); HIPCHK(dr.alloc(n * 8)); HIPCHK(dl.alloc(n)); HIPCHK(di.alloc(n));
    HIPCHK(hipMemcpyAsync(seed.p, pad_seed32, 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dl.p, level, n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(di.p, index, n * 8, hipMemcpyHostToDevice, st));
    LAUNCH_DX(ctx->tv.digest, (k_padding_nodes<DX>), dim3(nblk(n, 64)), dim3(64), 0, st, ctx->tv, n, seed.p, dl.p, di.p, dC.p, dH.p, dr.p);
    LAUNCH_CHECK();
    DevBuf<uint32_t> dHw;
    if (ctx_wide(ctx)) {
        HIPCHK(dHw.alloc(n * 16));
        hipLaunchKernelGGL(k_wide_hash_leaves, dim3(nblk(n, 256)), dim3(256), 0, st, n, dC.p, dHw.p);
        LAUNCH_CHECK();
    }
    HIPCHK(hipMemcpyAsync(C32, dC.p, n * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(H32, ctx_wide(ctx) ? dHw.p : dH.p, n * ctx_hash_bytes(ctx), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(r32, dr.p, n * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DAPOL_OK;
}
int32_t dapol_merge_batch(dapol_ctx* ctx, size_t n, const uint8_t* CL32, const uint8_t* HL32, const uint64_t* vL, const uint8_t* rL32,
                          const uint8_t* CR32, const uint8_t* HR32, const uint64_t* vR, const uint8_t* rR32, uint8_t* C32, uint8_t* H32,
                          uint64_t* v, uint8_t* r32) {
    if (!ctx || (n && (!CL32 || !HL32 || !CR32 || !HR32 || !C32 || !H32))) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    bool with_secrets = vL || rL32 || vR || rR32 || v || r32;
    if (with_secrets && !(vL && rL32 && vR && rR32 && v && r32)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "v/r pointers must be all set or all null");
    if (n == 0) return DAPOL_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<uint32_t> d[8], bad;
    DevBuf<uint64_t> dv[3];
    const size_t hw = (size_t)ctx_hw(ctx), hb = hw * 4;            // H arrays: ctx_hash_bytes per node
    for (auto& x : d) HIPCHK(x.alloc(n * hw));
    HIPCHK(bad.alloc(1));
    HIPCHK(hipMemsetAsync(bad.p, 0, 4, st));
    HIPCHK(hipMemcpyAsync(d[0].p, CL32, n * 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d[1].p, HL32, n * hb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d[2].p, CR32, n * 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d[3].p, HR32, n * hb, hipMemcpyHostToDevice, st));
    if (with_secrets) {
        for (auto& x : dv) HIPCHK(x.alloc(n));
        HIPCHK(hipMemcpyAsync(d[4].p, rL32, n * 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d[5].p, rR32, n * 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dv[0].p, vL, n * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dv[1].p, vR, n * 8, hipMemcpyHostToDevice, st));
    }
    DevBuf<uint32_t> oC, oH;
    HIPCHK(oC.alloc(n * 8)); HIPCHK(oH.alloc(n * hw));
    if (hw == 16)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_merge_records<16, DG_RUNTIME>), dim3(nblk(n, 64)), dim3(64), 0, st, ctx->tv.digest, n, d[0].p, d[1].p,
                           with_secrets ? dv[0].p : nullptr, d[4].p, d[2].p, d[3].p, with_secrets ? dv[1].p : nullptr, d[5].p, oC.p, oH.p,
                           with_secrets ? dv[2].p : nullptr, d[6].p, bad.p);
    else
        LAUNCH_DX(ctx->tv.digest, (k_merge_records<8, DX>), dim3(nblk(n, 64)), dim3(64), 0, st, ctx->tv.digest, n, d[0].p, d[1].p,
                  with_secrets ? dv[0].p : nullptr, d[4].p, d[2].p, d[3].p, with_secrets ? dv[1].p : nullptr, d[5].p, oC.p, oH.p,
                  with_secrets ? dv[2].p : nullptr, d[6].p, bad.p);
    LAUNCH_CHECK();
    uint32_t h_bad = 0;
    HIPCHK(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(C32, oC.p, n * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(H32, oH.p, n * hb, hipMemcpyDeviceToHost, st));
    if (with_secrets) {
        HIPCHK(hipMemcpyAsync(v, dv[2].p, n * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(r32, d[6].p, n * 32, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (h_bad) return fail(DAPOL_ERR_VALUE_DECODING, "Not the canonical encoding of a point.");
    return DAPOL_OK;
}

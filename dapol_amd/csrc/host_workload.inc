// The device-resident bench workload (dapol_workload): leaves uploaded once, then tree builds and per-entity proofs without host
// traffic, timed with HIP events -- what bench.py drives.  Included from dapol_hip.hip after host_entity.inc.
// ------------------------------------------------------------------------------------------------ workload
struct dapol_workload {
    dapol_ctx* ctx = nullptr;
    int total_height = 0, shard_bits = 0;
    size_t n = 0;
    DevBuf<uint64_t> idx, v;
    DevBuf<uint32_t> r;
    DevBuf<uint32_t> proofs, pathC, pathH;     // outputs of the last prove
    size_t proofs_first = 0, proofs_count = 0, proof_words = 0;
    DevBuf<unsigned long long> csum;
    DevBuf<uint32_t> seed;
    dapol_tree_owned* tree = nullptr;          // last build (borrows idx / v / r)
    bool holds_ctx = false;
    ~dapol_workload() { delete tree; }
};

__global__ void k_checksum(size_t n_words, const uint32_t* w, unsigned long long* acc) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long s = 0;
    for (; i < n_words; i += (size_t)gridDim.x * blockDim.x) s += (unsigned long long)w[i] * (unsigned long long)(2 * (i & 0xffff) + 1);
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off);
    if ((threadIdx.x & 63) == 0) atomicAdd(acc, s);
}

int32_t dapol_workload_create_shard(dapol_ctx* ctx, int32_t total_height, int32_t shard_bits, size_t n, const uint64_t* leaf_idx,
                                    const uint64_t* v, const uint8_t* r32, dapol_workload** out) {
    if (!ctx || !out || !n || !leaf_idx || !v || !r32) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    NEEDS_32_BYTE_DIGEST(ctx, "the device-resident workload (bench) path");
    if (total_height < 1 || total_height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must be in [1, 64]");
    if (shard_bits < 0 || shard_bits >= total_height || shard_bits > 16) return fail(DAPOL_ERR_INVALID_ARGUMENT, "shard_bits out of range");
    HIPCHK(hipSetDevice(ctx->device));
    dapol_workload* w = new dapol_workload();
    struct Guard { dapol_workload* w; ~Guard() { delete w; } } guard{w};
    w->ctx = ctx; w->total_height = total_height; w->shard_bits = shard_bits; w->n = n;
    HIPCHK(w->idx.alloc(n)); HIPCHK(w->v.alloc(n)); HIPCHK(w->r.alloc(n * 8)); HIPCHK(w->csum.alloc(1)); HIPCHK(w->seed.alloc(8));
    HIPCHK(hipMemcpy(w->idx.p, leaf_idx, n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(w->v.p, v, n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(w->r.p, r32, n * 32, hipMemcpyHostToDevice));
    guard.w = nullptr;
    w->holds_ctx = true;
    ctx_retain(ctx);
    *out = w;
    return DAPOL_OK;
}
int32_t dapol_workload_create(dapol_ctx* ctx, int32_t height, size_t n, const uint64_t* leaf_idx, const uint64_t* v, const uint8_t* r32,
                              dapol_workload** out) {
    return dapol_workload_create_shard(ctx, height, 0, n, leaf_idx, v, r32, out);
}
int32_t dapol_workload_destroy(dapol_workload* w) {
    if (!w) return DAPOL_OK;
    dapol_ctx* ctx = w->holds_ctx ? w->ctx : nullptr;
    if (w->ctx) (void)hipSetDevice(w->ctx->device);
    delete w;
    if (ctx) (void)dapol_ctx_destroy(ctx);
    return DAPOL_OK;
}

int32_t dapol_workload_tree(dapol_workload* w, dapol_tree** out) {
    if (!w || !out) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (!w->tree) return fail(DAPOL_ERR_INVALID_ARGUMENT, "dapol_workload_build has not run");
    *out = w->tree;
    return DAPOL_OK;
}

int32_t dapol_workload_build(dapol_workload* w, const uint8_t pad_seed32[32], uint8_t root_C[32], uint8_t root_H[32], uint64_t* root_v,
                             uint8_t root_r[32], dapol_workload_stats* stats) {
    if (!w || !pad_seed32) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    dapol_ctx* ctx = w->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    EventPair ev;
    HIPCHK(ev.init());
    {   // The new tree takes over the arena of the previous build (same leaves => same bounds => same size): a step neither frees
        // nor allocates the 3 GB, and the first timed step of a run no longer pays a cold hipMalloc (340 ms against a 45 ms build).
        dapol_tree_owned* old = w->tree;
        w->tree = new dapol_tree_owned();
        if (old) w->tree->arena = std::move(old->arena);
        delete old;
    }
    HIPCHK(hipEventRecord(ev.a, st));
    int32_t rc = tree_build_device(ctx, w->total_height, w->shard_bits, w->n, w->idx.p, w->v.p, w->r.p, pad_seed32, w->tree);
    if (rc) { delete w->tree; w->tree = nullptr; return rc; }
    HIPCHK(hipEventRecord(ev.b, st));
    LevelView root = w->tree->view(w->tree->height, nullptr);
    if (root_C) HIPCHK(hipMemcpyAsync(root_C, root.C, 32, hipMemcpyDeviceToHost, st));
    if (root_H) HIPCHK(hipMemcpyAsync(root_H, root.H, 32, hipMemcpyDeviceToHost, st));
    if (root_v) HIPCHK(hipMemcpyAsync(root_v, root.v, 8, hipMemcpyDeviceToHost, st));
    if (root_r) HIPCHK(hipMemcpyAsync(root_r, root.r, 32, hipMemcpyDeviceToHost, st));
    if (stats) {
        HIPCHK(hipMemcpyAsync(stats->root_C, root.C, 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(stats->root_H, root.H, 32, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (stats) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
        stats->tree_ms = ms;
    }
    return DAPOL_OK;
}

int32_t dapol_workload_prove(dapol_workload* w, const uint8_t nonce_seed32[32], int32_t n_bits, size_t first_entity, size_t n_entities,
                             int32_t n_upper, const uint8_t* up_C32, const uint8_t* up_H32, const uint64_t* up_v, const uint8_t* up_r32,
                             dapol_workload_stats* stats) {
    return dapol_workload_prove_policy(w, nonce_seed32, n_bits, first_entity, n_entities, DAPOL_POLICY_PADDING, w ? w->total_height : 0, n_upper, up_C32, up_H32,
                                       up_v, up_r32, stats);
}

int32_t dapol_workload_prove_policy(dapol_workload* w, const uint8_t nonce_seed32[32], int32_t n_bits, size_t first_entity, size_t n_entities,
                                    int32_t policy, int32_t aggregation_factor, int32_t n_upper, const uint8_t* up_C32, const uint8_t* up_H32,
                                    const uint64_t* up_v, const uint8_t* up_r32, dapol_workload_stats* stats) {
    WIRE_SCOPE();
    if (!w || !nonce_seed32 || !stats) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (!w->tree) return fail(DAPOL_ERR_INVALID_ARGUMENT, "dapol_workload_build has not run");
    if (n_upper != w->shard_bits) return fail(DAPOL_ERR_INVALID_ARGUMENT, "n_upper must equal the workload's shard_bits");
    if (first_entity > w->n || n_entities > w->n - first_entity) return fail(DAPOL_ERR_INVALID_ARGUMENT, "entity range out of bounds");
    dapol_ctx* ctx = w->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int Htot = w->total_height;
    size_t es = dapol_entity_proof_size(Htot, policy, aggregation_factor, n_bits);
    if (es == 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad policy / aggregation factor / n_bits");
    EventPair ev;
    HIPCHK(ev.init());
    const size_t tot = n_entities * (size_t)Htot;
    if (w->proofs.n < n_entities * es / 4) HIPCHK(w->proofs.alloc(n_entities * es / 4));
    if (w->pathC.n < tot * 8) { HIPCHK(w->pathC.alloc(tot * 8)); HIPCHK(w->pathH.alloc(tot * 8)); }
    HIPCHK(hipMemcpyAsync(w->seed.p, nonce_seed32, 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(w->csum.p, 0, 8, st));
    UpperDev up;
    int32_t rc = up.upload(st, n_upper, up_C32, up_H32, up_v, up_r32);
    if (rc) return rc;
    MsmTiming tm;
    tm.enabled = true;
    HIPCHK(hipEventRecord(ev.a, st));
    if (n_entities) {
        rc = prove_entities_device(ctx, w->tree, n_entities, w->idx.p + first_entity, policy, aggregation_factor, n_bits, w->seed.p, up,
                                   w->pathC.p, w->pathH.p, w->proofs.p, &tm);
        if (rc) return rc;
    }
    HIPCHK(hipEventRecord(ev.b, st));
    if (n_entities) {
        hipLaunchKernelGGL(k_checksum, dim3(1024), dim3(256), 0, st, n_entities * es / 4, w->proofs.p, w->csum.p); LAUNCH_CHECK();
    }
    unsigned long long cs = 0;
    HIPCHK(hipMemcpyAsync(&cs, w->csum.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
    stats->prove_ms = ms;
    stats->msm_ms = tm.total_ms(0); stats->msm_launches = tm.launches(0);
    stats->mat_ms = tm.total_ms(1); stats->mat_launches = tm.launches(1);
    stats->msm_all_ms = tm.total_ms(-1);
    stats->msm_span_ms = tm.span_ms(0);
    stats->msm_kernels = tm.kernels[0]; stats->mat_kernels = tm.kernels[1];
    stats->proofs = n_entities; stats->proof_bytes = n_entities * es; stats->checksum = cs;
    w->proofs_first = first_entity; w->proofs_count = n_entities; w->proof_words = es / 4;
    return DAPOL_OK;
}

int32_t dapol_workload_run(dapol_workload* w, const uint8_t pad_seed32[32], const uint8_t nonce_seed32[32], int32_t n_bits,
                           size_t first_entity, size_t n_entities, dapol_workload_stats* stats) {
    if (!w || !stats) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (w->shard_bits != 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "sharded workloads use dapol_workload_build + dapol_workload_prove");
    memset(stats, 0, sizeof *stats);
    int32_t rc = dapol_workload_build(w, pad_seed32, nullptr, nullptr, nullptr, nullptr, stats);
    if (rc) return rc;
    return dapol_workload_prove(w, nonce_seed32, n_bits, first_entity, n_entities, 0, nullptr, nullptr, nullptr, nullptr, stats);
}

int32_t dapol_workload_paths(dapol_workload* w, size_t b, const uint64_t* leaf_idx, int32_t n_upper, const uint64_t* up_v,
                             const uint8_t* up_r32, const uint8_t* up_C32, const uint8_t* up_H32, uint64_t* sib_v, uint8_t* sib_r32,
                             uint8_t* sib_C32, uint8_t* sib_H32) {
    WIRE_SCOPE();
    if (!w || !w->tree || (b && !leaf_idx)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument / no build yet");
    if (n_upper != w->shard_bits) return fail(DAPOL_ERR_INVALID_ARGUMENT, "n_upper must equal the workload's shard_bits");
    if (b == 0) return DAPOL_OK;
    hipStream_t st = w->ctx->stream;
    EntityShape S;                                           // (paths only: no range proofs, es = 0)
    S.H = w->total_height;
    const size_t u = (size_t)n_upper, tot = b * (size_t)S.H;
    const std::vector<uint8_t> zeros(u * 32, 0);             // an absent upper array counts as zeros
    const std::vector<uint64_t> zv(u, 0);
    EntityProveCall call;
    int32_t rc = call.open(w->ctx, w->tree, S, b, leaf_idx, nullptr, n_upper, up_C32 ? up_C32 : zeros.data(), up_H32 ? up_H32 : zeros.data(), up_v ? up_v : zv.data(),
                           up_r32 ? up_r32 : zeros.data());
    if (rc || (rc = call.paths())) return rc;
    if (sib_v) HIPCHK(hipMemcpyAsync(sib_v, call.pv.p, tot * 8, hipMemcpyDeviceToHost, st));
    if (sib_r32) HIPCHK(hipMemcpyAsync(sib_r32, call.pr.p, tot * 32, hipMemcpyDeviceToHost, st));
    if (sib_C32) HIPCHK(hipMemcpyAsync(sib_C32, call.pathC.p, tot * 32, hipMemcpyDeviceToHost, st));
    if (sib_H32) HIPCHK(hipMemcpyAsync(sib_H32, call.pathH.p, tot * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DAPOL_OK;
}

int32_t dapol_workload_proofs(dapol_workload* w, size_t first, size_t count, uint8_t* out) {
    if (!w || (count && !out)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (first < w->proofs_first || first - w->proofs_first > w->proofs_count || count > w->proofs_count - (first - w->proofs_first))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "proof range not part of the last run");
    HIPCHK(hipSetDevice(w->ctx->device));
    HIPCHK(hipMemcpy(out, w->proofs.p + (first - w->proofs_first) * w->proof_words, count * w->proof_words * 4, hipMemcpyDeviceToHost));
    return DAPOL_OK;
}

// Per-entity inclusion proofs (Dapol::generate_proof for b single leaves): the call frame of every per-entity proving entry point --
// _upper / _tape here, _shared (host_shared.inc), the re-prover (host_reprove.inc) -- and the core of the workload's proving step.
struct UpperDev {             // device arrays of the n siblings above a shard root, root side first (n may be 0), uploaded from the host's
    int n = 0;
    DevBuf<uint32_t> C, H, r;
    DevBuf<uint64_t> v;
    int32_t upload(hipStream_t st, int n_, const uint8_t* C32, const uint8_t* H32, const uint64_t* v64, const uint8_t* r32) {
        if (n_ <= 0) return DAPOL_OK;
        if (!C32 || !H32 || !v64 || !r32) return fail(DAPOL_ERR_INVALID_ARGUMENT, "upper sibling arrays missing");
        HIPCHK(C.alloc((size_t)n_ * 8)); HIPCHK(H.alloc((size_t)n_ * 8)); HIPCHK(r.alloc((size_t)n_ * 8)); HIPCHK(v.alloc((size_t)n_));
        HIPCHK(hipMemcpyAsync(C.p, C32, (size_t)n_ * 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(H.p, H32, (size_t)n_ * 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(r.p, r32, (size_t)n_ * 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(v.p, v64, (size_t)n_ * 8, hipMemcpyHostToDevice, st));
        n = n_;
        return DAPOL_OK;
    }
};

// The siblings of b leaves (indexes in HBM), [b][tree height + up.n] per array of po: the tree's own, then the ones above a shard root.
static int32_t entity_paths_device(dapol_tree* tree, size_t b, const uint64_t* d_leaf_idx, const UpperDev& up, PathOut po, uint32_t* d_pos) {
    int32_t rc = tree_paths_device(tree, b, d_leaf_idx, po, d_pos, up.n);
    if (rc) return rc;
    if (up.n) {
        hipLaunchKernelGGL(k_tree_path_upper, dim3(nblk(b * (size_t)up.n, 256)), dim3(256), 0, tree->ctx->stream, b, tree->height, up.n,
                           g_wire.siblings_leaf_first, up.C.p, up.H.p, up.v.p, up.r.p, po);
        LAUNCH_CHECK();
    }
    return DAPOL_OK;
}

// The shape of a per-entity proving call: H siblings per path, es bytes of range proofs per entity, the policy's plan.
struct EntityShape { int H = 0; size_t es = 0; std::vector<SubProof> plan; };
static int32_t entity_parties_ok(const dapol_ctx* ctx, const EntityShape& S) {
    for (auto& s : S.plan)
        if (s.m > ctx->max_parties) return fail(DAPOL_ERR_INVALID_ARGUMENT, "aggregation needs more parties than the context was created for");
    return DAPOL_OK;
}
// The refusals the four entry points share, in their shared order: context / tree / pointers (ptrs_ok: the entry point's own null
// checks; one refusal, worded bad_args) and the range of n_upper, the digest restriction of shards, H > 64, the proof size, max_parties.
// The entry points grew apart, and callers may rely on any of it, so each difference is an argument here or a line of the entry point:
//                              _upper                _tape                 _shared               reprove
//   bad_args                   "null or out-of-range argument" (_tape: "null argument")
//   n_upper                    [0, 16]               none (0)              [0, 16]               none (0)
//   H > 64 (check_h64)         not checked           not checked           refused (code 1)      refused (code 1)
//   max_parties (parties_now)  after b == 0 and the uploads (entity_parties_ok)    here, before b == 0
//   of its own, before b == 0  --                    a shard is refused    indexes increasing    indexes increasing, old arrays given
//   b == 0 leaves              nothing               nothing               *unique = 0           *proved = *kept = 0
// (_upper and _tape: a call of no entities never sees the max_parties refusal, and missing upper sibling arrays are refused before it.)
static int32_t entity_shape(const dapol_ctx* ctx, const dapol_tree* tree, bool ptrs_ok, const char* bad_args, int n_upper, int policy, int agg, int n_bits,
                            bool check_h64, bool parties_now, EntityShape& S) {
    if (!ctx || !tree || tree->ctx != ctx || !ptrs_ok || n_upper < 0 || n_upper > 16) return fail(DAPOL_ERR_INVALID_ARGUMENT, bad_args);
    if (n_upper) NEEDS_32_BYTE_DIGEST(ctx, "the sharded (multi-GPU) path");
    S.H = tree->height + n_upper;
    if (check_h64 && S.H > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    S.es = dapol_entity_proof_size(S.H, policy, agg, n_bits);
    if (S.es == 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad policy / aggregation_factor / n_bits");
    policy_plan(policy, S.H, agg, S.plan);
    return parties_now ? entity_parties_ok(ctx, S) : DAPOL_OK;
}

// The device side of a per-entity proving call (the prover's counterpart of VerifyCallDev, host_verify.inc): open() uploads, paths()
// gathers the siblings, the entry point proves into out, download() copies back.  with_out = false: the call has no [b][es] buffer
// (the compact shared call, host_shared.inc, whose range output is the distinct proofs alone) and download() copies the paths only.
struct EntityProveCall {
    dapol_ctx* ctx = nullptr;
    dapol_tree* tree = nullptr;
    size_t b = 0, tot = 0, es = 0;
    DevBuf<uint64_t> idx, pv;                        // leaf indexes [b]; sibling values [b][H]
    DevBuf<uint32_t> seed, pathC, pathH, pr, pos, out;    // nonce seed (null in tape mode); siblings [b][H]; range proofs [b][es / 4]
    UpperDev up;
    int32_t open(dapol_ctx* ctx_, dapol_tree* tree_, const EntityShape& S, size_t b_, const uint64_t* leaf_idx, const uint8_t* seed32_or_null, int n_upper,
                 const uint8_t* up_C32, const uint8_t* up_H32, const uint64_t* up_v, const uint8_t* up_r32, bool with_out = true) {
        ctx = ctx_; tree = tree_; b = b_; tot = b * (size_t)S.H; es = S.es;
        HIPCHK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        HIPCHK(idx.alloc(b)); HIPCHK(seed.alloc(seed32_or_null ? 8 : 0)); HIPCHK(pathC.alloc(tot * 8)); HIPCHK(pathH.alloc(tot * (size_t)ctx_hw(ctx)));
        HIPCHK(out.alloc(with_out ? b * es / 4 : 0)); HIPCHK(pv.alloc(tot)); HIPCHK(pr.alloc(tot * 8)); HIPCHK(pos.alloc(b));
        HIPCHK(hipMemcpyAsync(idx.p, leaf_idx, b * 8, hipMemcpyHostToDevice, st));
        if (seed32_or_null) HIPCHK(hipMemcpyAsync(seed.p, seed32_or_null, 32, hipMemcpyHostToDevice, st));
        return up.upload(st, n_upper, up_C32, up_H32, up_v, up_r32);
    }
    int32_t paths() { return entity_paths_device(tree, b, idx.p, up, PathOut{pathC.p, pathH.p, pv.p, pr.p}, pos.p); }
    int32_t download(uint8_t* path_C32, uint8_t* path_H32, uint8_t* range_out) {
        if (path_C32) HIPCHK(hipMemcpy(path_C32, pathC.p, tot * 32, hipMemcpyDeviceToHost));
        if (path_H32) HIPCHK(hipMemcpy(path_H32, pathH.p, tot * ctx_hash_bytes(ctx), hipMemcpyDeviceToHost));
        if (out.p) HIPCHK(hipMemcpy(range_out, out.p, b * es, hipMemcpyDeviceToHost));
        return DAPOL_OK;
    }
};

// Device-side core of Dapol::generate_proof for b single leaves whose indexes are in HBM already (the workload's path).
// d_range: [b][entity_words]; d_pathC/H may be null.
static int32_t prove_entities_device(dapol_ctx* ctx, dapol_tree* tree, size_t b, const uint64_t* d_leaf_idx, int policy, int agg,
                                     int n_bits, const uint32_t* d_seed, const UpperDev& up, uint32_t* d_pathC, uint32_t* d_pathH,
                                     uint32_t* d_range, MsmTiming* tm) {
    const int H = tree->height + up.n;
    std::vector<SubProof> plan;
    if (!policy_plan(policy, H, agg, plan)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "aggregation_factor must be within [0, tree height]");
    if (dapol_range_proof_size(n_bits, 1) == 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "n_bits must be 8/16/32/64");
    for (auto& s : plan)
        if (s.m > ctx->max_parties) return fail(DAPOL_ERR_INVALID_ARGUMENT, "aggregation needs more parties than the context was created for");
    const size_t tot = b * (size_t)H;
    DevBuf<uint64_t> pv;
    DevBuf<uint32_t> pr, pCtmp, pos;
    HIPCHK(pv.alloc(tot)); HIPCHK(pr.alloc(tot * 8)); HIPCHK(pos.alloc(b));
    uint32_t* pathC = d_pathC;
    if (!pathC) { HIPCHK(pCtmp.alloc(tot * 8)); pathC = pCtmp.p; }
    int32_t rc = entity_paths_device(tree, b, d_leaf_idx, up, PathOut{pathC, d_pathH, pv.p, pr.p}, pos.p);
    if (rc) return rc;
    return prove_policy_device(ctx, plan, b, H, pv.p, pr.p, pathC, n_bits, d_seed, d_leaf_idx, d_range, tm);
}

// What dapol_prove_entities_upper and _tape do for b > 0 entities once the shape stands: nonces from a seed, or (tape != null) from
// tape[e][slot][64] (64 bytes reduced mod l, Scalar::random), slots = dapol_entity_tape_slots per entity.
static int32_t entity_prove_call(dapol_ctx* ctx, dapol_tree* tree, const EntityShape& S, size_t b, const uint64_t* leaf_idx, int n_bits, const uint8_t* seed32,
                                 const uint8_t* tape, size_t slots, int n_upper, const uint8_t* up_C32, const uint8_t* up_H32, const uint64_t* up_v,
                                 const uint8_t* up_r32, uint8_t* path_C32, uint8_t* path_H32, uint8_t* range_out) {
    EntityProveCall call;
    DevBuf<uint32_t> dtape;
    int32_t rc = call.open(ctx, tree, S, b, leaf_idx, seed32, n_upper, up_C32, up_H32, up_v, up_r32);
    if (rc) return rc;
    if (tape) { HIPCHK(dtape.alloc(b * slots * 16)); HIPCHK(hipMemcpyAsync(dtape.p, tape, b * slots * 64, hipMemcpyHostToDevice, ctx->stream)); }
    if ((rc = entity_parties_ok(ctx, S)) || (rc = call.paths())) return rc;
    rc = prove_policy_device(ctx, S.plan, b, S.H, call.pv.p, call.pr.p, call.pathC.p, n_bits, call.seed.p, call.idx.p, call.out.p, nullptr, dtape.p, slots);
    return rc ? rc : call.download(path_C32, path_H32, range_out);
}

int32_t dapol_prove_entities_upper(dapol_ctx* ctx, dapol_tree* tree, size_t b, const uint64_t* leaf_idx, int32_t policy,
                                   int32_t aggregation_factor, int32_t n_bits, const uint8_t nonce_seed32[32], int32_t n_upper,
                                   const uint8_t* up_C32, const uint8_t* up_H32, const uint64_t* up_v, const uint8_t* up_r32,
                                   uint8_t* path_C32, uint8_t* path_H32, uint8_t* range_out) {
    WIRE_SCOPE();
    EntityShape S;
    int32_t rc = entity_shape(ctx, tree, nonce_seed32 && (!b || (leaf_idx && range_out)), "null or out-of-range argument", n_upper, policy, aggregation_factor,
                              n_bits, false, false, S);
    if (rc || b == 0) return rc;
    return entity_prove_call(ctx, tree, S, b, leaf_idx, n_bits, nonce_seed32, nullptr, 0, n_upper, up_C32, up_H32, up_v, up_r32, path_C32, path_H32, range_out);
}
// Wide draws one entity's range proofs consume, in the crate's draw order: the sub-proofs of the policy one after the other (one RNG
// runs through R::generate_proof, src/range/padding.rs:104-112 / splitting.rs:110-123), each m (2 n_bits + 4) draws.
size_t dapol_entity_tape_slots(int32_t height, int32_t policy, int32_t aggregation_factor, int32_t n_bits) {
    std::vector<SubProof> plan;
    if (height < 0 || height > 80 || !policy_plan(policy, height, aggregation_factor, plan) || dapol_range_proof_size(n_bits, 1) == 0) return 0;
    size_t slots = 0;
    for (auto& s : plan) slots += (size_t)s.m * (2 * (size_t)n_bits + 4);
    return slots;
}
// dapol_prove_entities in TAPE mode: every nonce of entity e is read from the tape instead of being derived from a seed -- what a Rust
// harness replays through a custom RngCore into prove_multiple_with_rng.
int32_t dapol_prove_entities_tape(dapol_ctx* ctx, dapol_tree* tree, size_t b, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor,
                                  int32_t n_bits, const uint8_t* tape, uint8_t* path_C32, uint8_t* path_H32, uint8_t* range_out) {
    WIRE_SCOPE();
    EntityShape S;
    int32_t rc = entity_shape(ctx, tree, !b || (leaf_idx && range_out && tape), "null argument", 0, policy, aggregation_factor, n_bits, false, false, S);
    if (rc) return rc;
    const size_t slots = dapol_entity_tape_slots(S.H, policy, aggregation_factor, n_bits);
    if (slots == 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad policy / aggregation_factor / n_bits");
    if (tree->shard_bits) return fail(DAPOL_ERR_INVALID_ARGUMENT, "tape mode proves over a whole tree (not a shard)");
    if (b == 0) return DAPOL_OK;
    return entity_prove_call(ctx, tree, S, b, leaf_idx, n_bits, nullptr, tape, slots, 0, nullptr, nullptr, nullptr, nullptr, path_C32, path_H32, range_out);
}
int32_t dapol_prove_entities(dapol_ctx* ctx, dapol_tree* tree, size_t b, const uint64_t* leaf_idx, int32_t policy,
                             int32_t aggregation_factor, int32_t n_bits, const uint8_t nonce_seed32[32], uint8_t* path_C32,
                             uint8_t* path_H32, uint8_t* range_out) {
    WIRE_SCOPE();
    return dapol_prove_entities_upper(ctx, tree, b, leaf_idx, policy, aggregation_factor, n_bits, nonce_seed32, 0, nullptr, nullptr, nullptr,
                                      nullptr, path_C32, path_H32, range_out);
}

// Batched verifier host side (kernels in kernels_verify.h).  Included from dapol_hip.hip after the prover's files.
// Device-pointer core: proofs at d_proofs + e*stride_words (+ the caller's offset already applied), commitments [b][m][8],
// verdicts to d_ok[b].
// The m commitments of a many-party proof are absorbed by one wavefront per proof (k_rv_absorb_V); inclusion proofs
// (m = 32) keep the lane-per-proof replay.  DAPOL_VERIFY_WAVE_TRANSCRIPT=0 / 1 forces either path (tests).
// Seed of the verifier's batching scalars when the caller passes none: 32 bytes from the OS CSPRNG.
#include <sys/random.h>
static int32_t os_random32(uint8_t out[32]) {
    size_t got = 0;
    while (got < 32) {
        ssize_t r = getrandom(out + got, 32 - got, 0);
        if (r <= 0) break;
        got += (size_t)r;
    }
    if (got < 32) {
        FILE* f = fopen("/dev/urandom", "rb");
        if (!f) return fail(DAPOL_ERR_INVALID_ARGUMENT, "no OS randomness for the verifier seed (getrandom and /dev/urandom failed)");
        size_t n = fread(out, 1, 32, f);
        fclose(f);
        if (n != 32) return fail(DAPOL_ERR_INVALID_ARGUMENT, "no OS randomness for the verifier seed");
    }
    return DAPOL_OK;
}
#define VERIFY_SEED_OR_OS(seedptr)                                     \
    uint8_t os_seed_[32];                                              \
    if (!(seedptr)) {                                                  \
        int32_t rc_seed_ = os_random32(os_seed_);                      \
        if (rc_seed_) return rc_seed_;                                 \
        (seedptr) = os_seed_;                                          \
    }
#include "verify_plan.inc"
static_assert(sizeof(VerifyState) == 2968, "tests/cpp/verify_plan_host.cpp restates this size");
// The commitments of a batch that are still on their way from the host when the check starts (dapol_range_verify_batch): they arrive
// in K column blocks -- block k = commitments [k m / K, (k + 1) m / K) of EVERY proof -- fetch(k) issues block k's copy and records
// ev[k].  The transcript replay (k_rv_absorb_V, a 1.4 ms latency chain for 1,024 parties whatever the batch size; 2.2 ms before round 5's changes to it) runs in K phases,
// each behind its block, so the copy of the other blocks hides under it instead of preceding it.
struct VArrival {
    int K = 0;
    std::function<int32_t(int)> fetch;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
};
static VerifyShape verify_shape(const dapol_ctx* ctx, int n_bits, int m, size_t b, const VArrival* va = nullptr) {
    VerifyShape s{};
    s.n = n_bits; s.m = m; s.b = b;
    s.opt_verify_batch_min = ctx->opt.verify_batch_min;
    s.wbits = ctx->tv.wbits; s.nwin = ctx->tv.nwin_c(); s.hi_split = ctx->tv.hi_split;
    s.n_cu = ctx->n_cu;
    s.budget_bytes = scratch_budget_bytes(ctx);
    s.va_K = va ? va->K : 0;
    return s;
}
// What the two launchers' kernel arguments have in common.
static void verify_range_args(RangeArgs& A, const VerifyShape& s, int N, int lgN, int TP, size_t stride_words, const uint32_t* d_seed) {
    A.n = s.n; A.m = s.m; A.N = N; A.lgN = lgN; A.TP = TP;
    A.out_words = (int)stride_words;
    A.wbits = s.wbits; A.nwin = s.nwin;
    A.seed = d_seed;
}

// Proof by proof: s.b proofs of the shape s (verify_plan.inc: plan_range_verify decides, this queues).
// queue_only: a call of ONE chunk returns with its work queued on ctx's stream, without the host wait at the end (the groups of a
// small call's plan on lanes of their own, verify_policy_device).
static int32_t range_verify_device(dapol_ctx* ctx, const VerifyShape& s, const uint32_t* d_proofs, size_t stride_words, const uint32_t* d_V,
                                   const uint32_t* d_seed, uint8_t* d_ok, bool queue_only = false) {
    hipStream_t st = ctx->stream;
    ForkGuard fg(ctx);
    const VerifyPlan P = plan_range_verify(s);
    if (P.lgN > RV_MAX_ROUNDS) return fail(DAPOL_ERR_INVALID_ARGUMENT, "proof too large");
    const size_t b = s.b, chunk = P.chunk;
    const int m = s.m;
    VerifyArgs V{};
    RangeArgs& A = V.R;
    verify_range_args(A, s, P.N, P.lgN, P.TP, stride_words, d_seed);
    A.use_hi = P.use_hi ? 1 : 0;
    A.nsplit = P.nsplit;
    V.lb = P.lb; V.hb = P.hb; V.tab_stride = P.tab_stride;
    V.wave_transcript = P.wave_transcript ? 1 : 0;
    const int var_waves = P.var_waves;
    HIPCHK(ctx->scratch.ensure(chunk * P.per_proof + 4096));
    uint8_t* base = (uint8_t*)ctx->scratch.p;
    size_t o = 0;
    A.dig = (dig_t*)(base + o); o += align_up(chunk * (size_t)A.nwin * A.TP * sizeof(dig_t), 256);
    V.vs = (VerifyState*)(base + o); o += align_up(chunk * sizeof(VerifyState), 256);
    V.tabs = (sc*)(base + o); o += align_up(chunk * (size_t)V.tab_stride * sizeof(sc), 256);
    A.PA = (int32_t*)(base + o); o += chunk * 160;
    A.P0 = (int32_t*)(base + o); o += chunk * 160 * (size_t)A.nsplit;
    A.P1 = (int32_t*)(base + o); o += chunk * 160 * (size_t)A.nsplit;
    int32_t* sum0 = (int32_t*)(base + o); o += chunk * 160;          // small calls: the partials summed by a wavefront (k_rp_sum_splits)
    int32_t* sum1 = (int32_t*)(base + o); o += chunk * 160;
    int32_t* var_parts = (int32_t*)(base + o); o += chunk * 160 * (size_t)var_waves;
    for (size_t first = 0; first < b; first += chunk) {
        size_t cb = b - first < chunk ? b - first : chunk;
        A.B = cb;
        A.out = const_cast<uint32_t*>(d_proofs) + first * stride_words;
        A.Vc = d_V + first * (size_t)m * 8;
        V.verdict = d_ok + first;
        const unsigned g_wave = (unsigned)cb, g_lane = nblk(cb, 64), g_dig = (unsigned)(cb * (size_t)(A.TP / 64));
        if (V.wave_transcript) { hipLaunchKernelGGL(k_rv_absorb_V, dim3(g_wave), dim3(64), 0, st, V, rv_transcript_head(A.n, A.m), 0, A.m); LAUNCH_CHECK(); }
        if (P.wave_replay) hipLaunchKernelGGL(k_rv_transcript<1>, dim3(g_wave), dim3(64), 0, st, V);
        else hipLaunchKernelGGL(k_rv_transcript<0>, dim3(g_lane), dim3(64), 0, st, V);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(k_rv_weights, dim3(g_lane), dim3(64), 0, st, V, (const uint32_t*)nullptr); LAUNCH_CHECK();   // c from the proof's own digest
        hipLaunchKernelGGL(k_rv_tables, dim3((unsigned)(cb * (size_t)((V.tab_stride + 63) / 64))), dim3(64), 0, st, V); LAUNCH_CHECK();
        if (P.side_var) {                                            // the proof's own points on a side stream under the generator MSM
            HIPCHK(hipEventRecord(ctx->ev_fork, st));
            HIPCHK(hipStreamWaitEvent(ctx->side[1], ctx->ev_fork, 0));
            fg.forked(1);
            if (P.quad_var(cb)) {
                hipLaunchKernelGGL(k_rv_varpoints_quad, dim3((unsigned)(cb * (size_t)var_waves)), dim3(64), 0, ctx->side[1], V, var_parts, var_waves); LAUNCH_CHECK();
                hipLaunchKernelGGL(k_rv_sum_parts, dim3(g_wave), dim3(64), 0, ctx->side[1], cb, var_waves, var_parts, A.PA); LAUNCH_CHECK();
            } else {
                hipLaunchKernelGGL(k_rv_varpoints, dim3(g_wave), dim3(64), 0, ctx->side[1], V); LAUNCH_CHECK();
            }
            HIPCHK(hipEventRecord(ctx->ev_join[1], ctx->side[1]));
            FAULT_AFTER_FORK("verify_var");
        }
        hipLaunchKernelGGL(k_rv_scalars, dim3(g_dig), dim3(64), 0, st, V); LAUNCH_CHECK();
        if (P.quad) hipLaunchKernelGGL(k_rp_msm_quad, dim3((unsigned)(cb * (size_t)A.nsplit)), dim3(64), 0, st, A, ctx->tv, -1);
        else launch_msm(st, A, ctx->tv, -1, P.lpl);
        LAUNCH_CHECK();
        if (P.side_var) { HIPCHK(hipStreamWaitEvent(st, ctx->ev_join[1], 0)); fg.joined(1); }
        else { hipLaunchKernelGGL(k_rv_varpoints, dim3(g_wave), dim3(64), 0, st, V); LAUNCH_CHECK(); }
        if (P.tree_sum) {
            hipLaunchKernelGGL(k_rp_sum_splits, dim3((unsigned)(2 * cb)), dim3(64), 0, st, cb, A.nsplit, A.P0, A.P1, sum0, sum1); LAUNCH_CHECK();
            VerifyArgs Vs = V;
            Vs.R.nsplit = 1; Vs.R.P0 = sum0; Vs.R.P1 = sum1;
            hipLaunchKernelGGL(k_rv_finish, dim3(g_lane), dim3(64), 0, st, Vs, ctx->tv); LAUNCH_CHECK();
        } else {
            hipLaunchKernelGGL(k_rv_finish, dim3(g_lane), dim3(64), 0, st, V, ctx->tv); LAUNCH_CHECK();
        }
        if (!(queue_only && chunk >= b)) HIPCHK(hipStreamSynchronize(st));
    }
    return DAPOL_OK;
}

// Cross-proof batched verification (kernels_verify.h, "Cross-proof batching"): one random linear combination per chunk
// of proofs; a chunk whose combined check fails (or holds an undecodable point) is re-verified proof by proof, so the
// verdicts are exactly the per-proof ones.  DAPOL_VERIFY_NO_RLC=1 forces the per-proof path.
// verify_plan.inc decides (plan_range_verify_rlc per call, RlcPlan::chunk_plan per chunk size); the functions below queue.

// The chunk's buffers: the plan's offsets into the scratch (and, for the bucket method, into the per-point table region).
static void carve_rlc_chunk(RlcArgs& R, uint8_t* base, const RlcChunk& C) {
    VerifyArgs& V = R.V;
    RangeArgs& A = V.R;
    A.dig = (dig_t*)(base + C.o_dig); V.vs = (VerifyState*)(base + C.o_vs);
    A.P0 = (int32_t*)(base + C.o_p0); A.P1 = (int32_t*)(base + C.o_p1);
    R.partial = (sc*)(base + C.o_part); R.bsum = (sc*)(base + C.o_bsum);
    R.ptT = (int32_t*)(base + C.o_pt); R.dig2 = (dig_t*)(base + C.o_dig2);
    R.Q0 = (int32_t*)(base + C.o_q0); R.Q1 = (int32_t*)(base + C.o_q1);
    R.flag = (uint32_t*)(base + C.o_flag);
    V.tabs = (sc*)(base + C.o_tabs);
    R.tab29 = (uint32_t*)(base + C.o_t29); R.rzg = (sc*)(base + C.o_rzg);
    if (C.pippenger) {
        uint8_t* q = base + C.o_pt;
        R.pN = (int32_t*)(q + C.b_pN); R.pdig = (int16_t*)(q + C.b_pdig); R.psorted = (uint32_t*)(q + C.b_psorted);
        R.phist = (uint32_t*)(q + C.b_phist); R.poffs = (uint32_t*)(q + C.b_poffs); R.pcursor = (uint32_t*)(q + C.b_pcursor);
        R.pbsum = (int32_t*)(q + C.b_pbsum);
    }
}
// The batch's own points by the bucket method (R.ns2 = RVP_NW window sums in R.Q0 / R.Q1), behind their decode on sb.
static int32_t own_points_bucket(hipStream_t sb, const RlcArgs& R, size_t hsz) {
    HIPCHK(hipMemsetAsync(R.phist, 0, hsz, sb));
    const unsigned runs = nblk(R.npts, RVP_RUN);
    hipLaunchKernelGGL(k_rvp_digits, dim3(runs), dim3(RVP_BLOCK), 0, sb, R); LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rvp_scan, dim3(RVP_NW), dim3(64), 0, sb, R); LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rvp_scatter, dim3(8 * runs), dim3(RVP_BLOCK), 0, sb, R); LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rvp_buckets, dim3((unsigned)((size_t)RVP_NW * RVP_NB * RVP_S / 64)), dim3(64), 0, sb, R); LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rvp_window, dim3(RVP_NW), dim3(64), 0, sb, R); LAUNCH_CHECK();
    return DAPOL_OK;
}
// ... and by per-point tables + ONE Straus MSM over them (the prover's tail kernel).
static int32_t own_points_straus(hipStream_t st, const RlcArgs& R) {
    hipLaunchKernelGGL(k_rvb_points, dim3(nblk(2 * R.Np, 64)), dim3(64), 0, st, R); LAUNCH_CHECK();
    RangeArgs A2{};
    A2.N = (int)R.Np; A2.TP = R.TP2; A2.wbits = PT_WBITS; A2.nwin = PT_NWIN; A2.B = 1; A2.nsplit = R.ns2;
    A2.dig = R.dig2; A2.P0 = R.Q0; A2.P1 = R.Q1;
    const TableView tvp{R.ptT, 1, PT_WBITS, 0, 0};
    hipLaunchKernelGGL((k_rp_msm<MSM_TAIL, 32>), dim3((unsigned)R.ns2), dim3(64), 0, st, A2, tvp, -1); LAUNCH_CHECK();
    return DAPOL_OK;
}
// The batch digest D (BLAKE3 tree over the per-proof digests) and from it every proof's c and rho.
static int32_t batch_digest(hipStream_t st, const VerifyArgs& V, size_t cb, uint32_t* dga, uint32_t* dgb) {
    uint32_t* bufs[2] = {dga, dgb};
    const uint32_t* in = V.vs[0].dg;        // (address arithmetic only: vs is a device pointer)
    size_t stride = sizeof(VerifyState) / 4, n = cb;
    int level = 0;
    do {
        uint32_t* out = bufs[level & 1];
        hipLaunchKernelGGL(k_rv_digest_level, dim3(nblk((n + 30) / 31, 64)), dim3(64), 0, st, n, level, in, stride, out); LAUNCH_CHECK();
        in = out; stride = 8; n = (n + 30) / 31; level++;
    } while (n > 1);
    hipLaunchKernelGGL(k_rv_weights, dim3(nblk(cb, 64)), dim3(64), 0, st, V, in); LAUNCH_CHECK();
    return DAPOL_OK;
}
// The ONE generator MSM of a chunk, in the shape the plan chose.
static int32_t generator_msm(dapol_ctx* ctx, const RlcPlan& P, const RangeArgs& A, int32_t* gpart) {
    hipStream_t st = ctx->stream;
    RangeArgs A1 = A;
    A1.B = 1;
    if (P.quad_gen) hipLaunchKernelGGL(k_rp_msm_quad, dim3((unsigned)A1.nsplit), dim3(64), 0, st, A1, ctx->tv, -1);
    else if (P.gen_sweep) {
        hipLaunchKernelGGL(k_rvb_gen_sweep, dim3((unsigned)(A1.nwin * P.gen_ns)), dim3(64), 0, st, A1, ctx->tv, P.gen_ns, gpart); LAUNCH_CHECK();
        hipLaunchKernelGGL(k_rvb_gen_windows, dim3((unsigned)A1.nwin), dim3(64), 0, st, A1, P.gen_ns, gpart);
    } else launch_msm(st, A1, ctx->tv, -1, P.lpl);
    LAUNCH_CHECK();
    return DAPOL_OK;
}
// One chunk's combined check, queued on the context's stream up to its verdicts (A.B / A.out / A.Vc / V.verdict are the caller's).
// va: the commitments arrive in blocks and the replay runs in phases behind them (RlcPlan::pipelined).
static int32_t queue_rlc_chunk(dapol_ctx* ctx, ForkGuard& fg, const RlcPlan& P, const RlcChunk& C, RlcArgs& R, VArrival* va) {
    hipStream_t st = ctx->stream;
    VerifyArgs& V = R.V;
    RangeArgs& A = V.R;
    const size_t cb = C.cb;
    const int m = A.m;
    R.G = C.G; R.npts = C.npts; R.Np = C.Np; R.TP2 = C.TP2; R.ns2 = C.ns2; R.lazy = C.lazy ? 1 : 0;
    HIPCHK(ctx->scratch.ensure(C.need + 4096));
    uint8_t* base = (uint8_t*)ctx->scratch.p;
    carve_rlc_chunk(R, base, C);
    HIPCHK(hipMemsetAsync(R.flag, 0, 16, st));
    bool absorbed = false;
    HIPCHK(hipEventRecord(ctx->ev_fork, st));                 // (what the decode on the side stream has to wait for on THIS stream)
    if (va) {                                                  // the replay in phases, each behind its block of commitments
        for (int k = 0; k < va->K; k++) {
            int32_t rc = va->fetch(k);
            if (rc) return rc;
            HIPCHK(hipStreamWaitEvent(st, va->ev[k], 0));
            hipLaunchKernelGGL(k_rv_absorb_V, dim3((unsigned)cb), dim3(64), 0, st, V, rv_transcript_head(A.n, A.m), k * (m / va->K), (k + 1) * (m / va->K)); LAUNCH_CHECK();
        }
        absorbed = true;
    }
    if (C.pippenger) {
        if (!C.b_fits) return fail(DAPOL_ERR_OUT_OF_MEMORY, "bucket-method scratch does not fit the per-point table region");
        // decode on a side stream, beside the transcript replay (which occupies one wavefront per SIMD at most)
        HIPCHK(hipStreamWaitEvent(ctx->side[0], ctx->ev_fork, 0));
        if (va) HIPCHK(hipStreamWaitEvent(ctx->side[0], va->ev[va->K - 1], 0));      // (all the commitments: the last block lands last)
        fg.forked(0);
        hipLaunchKernelGGL(k_rvp_decode, dim3(nblk(R.npts, 64)), dim3(64), 0, ctx->side[0], R); LAUNCH_CHECK();
        HIPCHK(hipEventRecord(ctx->ev_join[0], ctx->side[0]));
        FAULT_AFTER_FORK("verify_decode");
    }
    if (V.wave_transcript && !absorbed) { hipLaunchKernelGGL(k_rv_absorb_V, dim3((unsigned)cb), dim3(64), 0, st, V, rv_transcript_head(A.n, A.m), 0, A.m); LAUNCH_CHECK(); }
    if (C.wave_replay) hipLaunchKernelGGL(k_rv_transcript<1>, dim3((unsigned)cb), dim3(64), 0, st, V);
    else hipLaunchKernelGGL(k_rv_transcript<0>, dim3(nblk(cb, 64)), dim3(64), 0, st, V);
    LAUNCH_CHECK();
    int32_t rc = batch_digest(st, V, cb, (uint32_t*)(base + C.o_dga), (uint32_t*)(base + C.o_dgb));
    if (rc) return rc;
    // Round 5: from here the pass has two independent halves -- the generator scalars with their one MSM (product tables, 2 x 65,536
    // sums over the proofs, VALU-bound) and the batch's own points by the bucket method (digits, counting sort, bucket and window
    // sums: memory- and latency-bound, ending in 23 lone wavefronts).  They used to queue behind each other on one stream; the
    // own points now follow their decode on the side stream and the two halves meet again at k_rvb_finish.
    const int ns2_saved = R.ns2;
    if (C.pippenger) R.ns2 = RVP_NW;
    // k_rv_tables BEFORE the fork: the own points' digits (k_rvp_digits -> rv_own_point) read its z^2 z^j entries for the commitment
    // terms.  (Round 5 launched it after the fork, unordered against the side stream: with the same proofs in every pass the
    // scratch still held the right values, which hid it -- ADVICE r5, high.)
    hipLaunchKernelGGL(k_rv_tables, dim3((unsigned)(cb * (size_t)((V.tab_stride + 63) / 64))), dim3(64), 0, st, V); LAUNCH_CHECK();
    if (C.fork) {
        HIPCHK(hipEventRecord(ctx->ev_fork, st));                    // the weights, the tables (and everything the replay left in vs) are there
        HIPCHK(hipStreamWaitEvent(ctx->side[0], ctx->ev_fork, 0));   // (side[0] already holds the decode)
        rc = own_points_bucket(ctx->side[0], R, C.b_hsz);
        if (rc) return rc;
        HIPCHK(hipEventRecord(ctx->ev_join[0], ctx->side[0]));
    }
    hipLaunchKernelGGL(k_rvb_tables2, dim3((unsigned)(cb * (size_t)((V.tab_stride - rv_tab_entries(A.lgN, m) + (R.lazy ? (1 << V.lb) : 0) + 63) / 64))),
                       dim3(64), 0, st, R);
    LAUNCH_CHECK();
    if (R.lazy) {
        hipLaunchKernelGGL(k_rvb_rzsum, dim3((unsigned)R.G), dim3(64), 0, st, R); LAUNCH_CHECK();
        hipLaunchKernelGGL(k_rvb_gh_lazy, dim3((unsigned)(P.nch * R.G)), dim3(64), 0, st, R); LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL(k_rvb_gh_partial, dim3((unsigned)(P.nch * R.G)), dim3(64), 0, st, R); LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_rvb_gh_reduce, dim3((unsigned)P.nch), dim3(64), 0, st, R); LAUNCH_CHECK();
    rc = generator_msm(ctx, P, A, (int32_t*)(base + C.o_gpart));
    if (rc) return rc;
    hipLaunchKernelGGL(k_rvb_base_scalars, dim3(nblk(cb, 64)), dim3(64), 0, st, R); LAUNCH_CHECK();
    if (C.pippenger) {
        HIPCHK(hipStreamWaitEvent(st, ctx->ev_join[0], 0));       // the decoded points -- or, forked, the window sums made from them
        fg.joined(0);
        if (!C.fork) { rc = own_points_bucket(st, R, C.b_hsz); if (rc) return rc; }
    } else {
        rc = own_points_straus(st, R);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_rvb_finish, dim3(1), dim3(64), 0, st, R, ctx->tv); LAUNCH_CHECK();
    R.ns2 = ns2_saved;
    hipLaunchKernelGGL(k_rvb_verdicts, dim3(nblk(cb, 256)), dim3(256), 0, st, V); LAUNCH_CHECK();
    return DAPOL_OK;
}
static int32_t range_verify_rlc_device(dapol_ctx* ctx, int n_bits, int m, size_t b, const uint32_t* d_proofs, size_t stride_words,
                                       const uint32_t* d_V, const uint32_t* d_seed, uint8_t* d_ok, VArrival* va = nullptr);
// Some proof of a chunk is bad: find out which.  Large chunks are narrowed down with the same batched check on eight parts (a part
// that passes vouches for its proofs; a part that fails is split again, down to the proof-by-proof check): one bad proof among
// 1,024 costs a few batched checks of shrinking size instead of 1,024 single ones.
static int32_t bisect_failed_chunk(dapol_ctx* ctx, const VerifyShape& s, size_t cb, const uint32_t* d_proofs, size_t stride_words, const uint32_t* d_V,
                                   const uint32_t* d_seed, uint8_t* d_ok) {
    g_verify_fallbacks.fetch_add(1, std::memory_order_relaxed);
    if (cb < 64) {
        VerifyShape s1 = s;
        s1.b = cb; s1.va_K = 0;
        return range_verify_device(ctx, s1, d_proofs, stride_words, d_V, d_seed, d_ok);
    }
    const size_t part = (cb + 7) / 8;
    for (size_t o = 0; o < cb; o += part) {
        const size_t n = std::min(part, cb - o);
        int32_t rc = range_verify_rlc_device(ctx, s.n, s.m, n, d_proofs + o * stride_words, stride_words, d_V + o * (size_t)s.m * 8, d_seed, d_ok + o);
        if (rc) return rc;
    }
    return DAPOL_OK;
}
static int32_t range_verify_rlc_device(dapol_ctx* ctx, int n_bits, int m, size_t b, const uint32_t* d_proofs, size_t stride_words,
                                       const uint32_t* d_V, const uint32_t* d_seed, uint8_t* d_ok, VArrival* va) {
    const VerifyShape s = verify_shape(ctx, n_bits, m, b, va);
    const RlcPlan P = plan_range_verify_rlc(s);
    if (va && !P.pipelined) {                               // no pipelining on this path: have every block land before anything reads it
        for (int k = 0; k < va->K; k++) {
            int32_t rc = va->fetch(k);
            if (rc) return rc;
            HIPCHK(hipStreamWaitEvent(ctx->stream, va->ev[k], 0));
        }
        va = nullptr;
    }
    if (!P.use_rlc) return range_verify_device(ctx, s, d_proofs, stride_words, d_V, d_seed, d_ok);
    if (P.lgN > RV_MAX_ROUNDS) return fail(DAPOL_ERR_INVALID_ARGUMENT, "proof too large");
    hipStream_t st = ctx->stream;
    ForkGuard fg(ctx);
    RlcArgs R{};
    VerifyArgs& V = R.V;
    RangeArgs& A = V.R;
    verify_range_args(A, s, P.N, P.lgN, P.TP, stride_words, d_seed);
    A.nsplit = P.nsplit; A.use_hi = P.use_hi ? 1 : 0;
    R.K = P.K;
    V.lb = P.lb; V.hb = P.hb; V.tab_stride = P.tab_stride;
    V.wave_transcript = P.wave_transcript ? 1 : 0;
    RlcChunk C{};
    for (size_t first = 0; first < b; first += P.chunk) {
        const size_t cb = b - first < P.chunk ? b - first : P.chunk;
        if (cb != C.cb) C = P.chunk_plan(cb);
        A.B = cb;
        A.out = const_cast<uint32_t*>(d_proofs) + first * stride_words;
        A.Vc = d_V + first * (size_t)m * 8;
        V.verdict = d_ok + first;
        int32_t rc = queue_rlc_chunk(ctx, fg, P, C, R, va);
        if (rc) return rc;
        uint32_t h_flag[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(h_flag, R.flag, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!h_flag[0] || h_flag[1]) {
            rc = bisect_failed_chunk(ctx, s, cb, d_proofs + first * stride_words, stride_words, d_V + first * (size_t)m * 8, d_seed, d_ok + first);
            if (rc) return rc;
        }
    }
    return DAPOL_OK;
}


int32_t dapol_range_verify_batch(dapol_ctx* ctx, int32_t n_bits, int32_t m, size_t b, const uint8_t* proofs, const uint8_t* V32,
                                 const uint8_t verify_seed32[32], uint8_t* ok) {
    if (!ctx || (b && (!proofs || !V32 || !ok))) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    VERIFY_SEED_OR_OS(verify_seed32)
    size_t ps = dapol_range_proof_size(n_bits, m);
    if (ps == 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "n_bits must be 8/16/32/64 and m a power of two");
    if (m > ctx->max_parties) return fail(DAPOL_ERR_INVALID_ARGUMENT, "m exceeds the context's max_parties (InvalidGeneratorsLength)");
    if (b == 0) return DAPOL_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // one arena for the call's device copies, kept on the context between calls while it stays below 1 GB
    struct Span32 { uint32_t* p; };
    struct Span8 { uint8_t* p; };
    const size_t o_pr = 0, o_V = align_up(b * ps, 256), o_seed = o_V + align_up(b * (size_t)m * 32, 256), o_ok = o_seed + 256, io_bytes = o_ok + align_up(b, 256);
    DevBuf<uint8_t> io_big;
    uint8_t* io = nullptr;
    // (kept up to 1 GB on a DAPOL_PROFILE_BENCH context, up to 64 MB on a DAPOL_PROFILE_HOST one -- a context that shares its GPU does not
    // sit on a gigabyte for the sake of the next call; larger calls allocate and free.  INTEGRATION.md section 4 counts it.)
    const size_t vio_keep = ctx->opt.profile == DAPOL_PROFILE_HOST ? ((size_t)64 << 20) : ((size_t)1 << 30);
    if (io_bytes <= vio_keep) { HIPCHK(ctx->vio.ensure(io_bytes)); io = (uint8_t*)ctx->vio.p; }
    else { HIPCHK(io_big.alloc(io_bytes)); io = io_big.p; }
    const Span32 dproofs{(uint32_t*)(io + o_pr)}, dV{(uint32_t*)(io + o_V)}, dseed{(uint32_t*)(io + o_seed)};
    const Span8 dok{io + o_ok};
    HIPCHK(hipMemcpyAsync(dproofs.p, proofs, b * ps, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dseed.p, verify_seed32, 32, hipMemcpyHostToDevice, st));
    // Many-party batches (tens of MB of commitments): the commitments travel in four column blocks on a side stream while the
    // transcript replay already runs on the blocks that have landed (VArrival above).  Everything else: one copy, up front.
    const bool pipe = verify_pipe_arrival(m, b);
    ForkGuard fg(ctx);
    VArrival va;
    if (pipe) {
        va.K = 4;
        for (int k = 0; k < 4; k++) va.ev[k] = ctx->ev_v[k];
        const size_t pitch = (size_t)m * 32, cw = pitch / 4;
        va.fetch = [&, pitch, cw](int k) -> int32_t {
            fg.forked(1);
            HIPCHK(hipMemcpy2DAsync((uint8_t*)dV.p + (size_t)k * cw, pitch, V32 + (size_t)k * cw, pitch, cw, b, hipMemcpyHostToDevice, ctx->side[1]));
            HIPCHK(hipEventRecord(va.ev[k], ctx->side[1]));
            return DAPOL_OK;
        };
    } else HIPCHK(hipMemcpyAsync(dV.p, V32, b * (size_t)m * 32, hipMemcpyHostToDevice, st));
    int32_t rc = range_verify_rlc_device(ctx, n_bits, m, b, dproofs.p, ps / 4, dV.p, dseed.p, dok.p, pipe ? &va : nullptr);
    if (rc) return rc;
    fg.joined(1);                                              // (the main stream waited for every block and has drained)
    HIPCHK(hipMemcpy(ok, dok.p, b, hipMemcpyDeviceToHost));
    return DAPOL_OK;
}

// R::verify (src/range/padding.rs:169-196, splitting.rs:181-210) for b proofs over H sibling commitments each
// (dPC: [b][H][8]); ANDs the verdicts into dok.  dsub: [b] bytes, dV: [b][max m][8] scratch.
// A run of equal-sized FULL sub-proofs (the individual proofs beyond aggregation_factor, with the one-party part of an odd split before
// them -- as the prover groups them, host_policy.inc) is ONE batched check of b * k proofs: their words gathered into a contiguous
// batch, commitments [b * k][m], the entity's verdict the AND over its k sub-proofs (round 6; DAPOL_NO_GROUP=1: one check per sub-proof).
static int32_t verify_policy_device(dapol_ctx* ctx, const std::vector<SubProof>& plan, size_t b, int H, const uint32_t* dPC, const uint32_t* dR,
                                    size_t entity_words, int n_bits, const uint32_t* dseed, uint8_t* dok, uint8_t* dsub, uint32_t* dV) {
    hipStream_t st = ctx->stream;
    const uint32_t* Bb_comp = ctx->gens_comp.p + (size_t)ctx->tv.row_Bb(0) * 8;
    const PolicyGroups PG = group_policy_plan(plan, policy_grouping_on());
    const std::vector<PolicyGroup>& groups = PG.groups;
    const bool on_lanes = verify_groups_on_lanes(groups.size(), b, PG.sum_proofs, PG.max_k, ctx->opt.verify_batch_min);
    const PolicyLayout L = policy_layout(PG, b, n_bits, !on_lanes);
    // What the checks need beside the caller's [b]-sized buffers: the gathered words, commitments and verdicts of every group (on lanes)
    // or of the largest one (one after the other: only runs of several sub-proofs are gathered, a lone one is read in place).
    DevBuf<uint32_t> arena;
    uint32_t *aR = nullptr, *aV = nullptr;
    uint8_t* asub = nullptr;
    if (on_lanes || PG.max_k > 1) {
        const size_t o_V = align_up(L.words * 4, 256), o_sub = o_V + align_up(L.parties * 32, 256), total = o_sub + align_up(L.proofs, 256);
        HIPCHK(arena.alloc(total / 4 + 64));
        aR = arena.p; aV = (uint32_t*)((uint8_t*)arena.p + o_V); asub = (uint8_t*)arena.p + o_sub;
    }
    // one group's commitments, [b * k][m]: an aggregated (or lone individual) proof pads its parties, a run of full ones does not
    auto gather_commitments = [&](const PolicyGroup& g, uint32_t* out) -> int32_t {
        if (g.k == 1) hipLaunchKernelGGL(k_gather_commitments, dim3(nblk(b * (size_t)g.m, 256)), dim3(256), 0, st, b, H, g.start, g.count, g.m, dPC, Bb_comp, out);
        else hipLaunchKernelGGL(k_gather_commitments_grouped, dim3(nblk(b * (size_t)g.k * (size_t)g.m, 256)), dim3(256), 0, st, b, H, g.start, g.m, g.k, dPC, out);
        LAUNCH_CHECK();
        return DAPOL_OK;
    };
    auto gather_words = [&](size_t gi) -> int32_t {
        const PolicyLayout::Group& lg = L.g[gi];
        hipLaunchKernelGGL(k_gather_words_grouped, dim3(nblk(b * (size_t)groups[gi].k * lg.proof_words, 256)), dim3(256), 0, st, b, groups[gi].k, lg.proof_words,
                           entity_words, lg.word_off, dR, aR + lg.gathered_word_off);
        LAUNCH_CHECK();
        return DAPOL_OK;
    };
    int32_t rc = DAPOL_OK;
    if (!on_lanes) {
        for (size_t gi = 0; gi < groups.size(); gi++) {
            const PolicyGroup& g = groups[gi];
            const PolicyLayout::Group& lg = L.g[gi];
            if ((rc = gather_commitments(g, g.k == 1 ? dV : aV))) return rc;
            if (g.k == 1) {                                     // (its words are read in place, an entity's blob apart)
                if ((rc = range_verify_rlc_device(ctx, n_bits, g.m, b, dR + lg.word_off, entity_words, dV, dseed, dsub))) return rc;
                hipLaunchKernelGGL(k_and_bytes, dim3(nblk(b, 256)), dim3(256), 0, st, b, dok, dsub);
            } else {
                if ((rc = gather_words(gi)) || (rc = range_verify_rlc_device(ctx, n_bits, g.m, b * (size_t)g.k, aR, lg.proof_words, aV, dseed, asub))) return rc;
                hipLaunchKernelGGL(k_and_bytes_grouped, dim3(nblk(b, 256)), dim3(256), 0, st, b, g.k, dok, asub);
            }
            LAUNCH_CHECK();
        }
        HIPCHK(hipStreamSynchronize(st));                      // (the arena dies with this scope)
        return DAPOL_OK;
    }
    // A SMALL call with several groups (as the prover, host_policy.inc): the per-proof checks of the groups side by side, each on a
    // lane of its own, queued without a host wait; the verdicts are ANDed on the context's stream behind the lanes' events.
    PolicyLanes lanes(ctx);                                    // (an early return below: it waits for the lanes before the arena goes)
    for (size_t gi = 0; gi < groups.size(); gi++)
        if ((rc = gather_commitments(groups[gi], aV + L.g[gi].party_off * 8)) || (rc = gather_words(gi))) return rc;
    if ((rc = lanes.fork(st))) return rc;
    for (size_t gi = 0; gi < groups.size(); gi++) {
        if (gi == 2) FAULT_AFTER_FORK("policy_verify_lanes");     // (group 1 is in flight on a lane of its own)
        const PolicyGroup& g = groups[gi];
        const PolicyLayout::Group& lg = L.g[gi];
        dapol_ctx* lane = nullptr;
        if ((rc = lanes.take(gi, &lane))) return rc;
        rc = range_verify_device(lane, verify_shape(lane, n_bits, g.m, b * (size_t)g.k), aR + lg.gathered_word_off, lg.proof_words, aV + lg.party_off * 8, dseed,
                                 asub + lg.verdict_off, true);
        if (rc) return rc;
        if (lane != ctx) {                                      // the context's stream takes the verdicts behind the lane (one event per lane and use)
            HIPCHK(hipEventRecord(lane->ev_v[1 + (gi / 4) % 3], lane->stream));
            HIPCHK(hipStreamWaitEvent(st, lane->ev_v[1 + (gi / 4) % 3], 0));
        }
        hipLaunchKernelGGL(k_and_bytes_grouped, dim3(nblk(b, 256)), dim3(256), 0, st, b, g.k, dok, asub + lg.verdict_off);
        LAUNCH_CHECK();
    }
    HIPCHK(hipStreamSynchronize(st));                          // (behind every lane's event: the lanes have drained too)
    lanes.close();
    return DAPOL_OK;
}

// The device side that dapol_verify_entities and dapol_verify_entities_shared (host_verify_shared.inc) have in common: one arena for the
// call's inputs and verdict bytes, its upload, the Merkle re-merge queued (on a side stream for a call of few proofs: fg is the
// caller's guard, and D.side_paths says that the caller has to join ctx->ev_join[2]) and dok set to ones.  v_parties: commitments per
// entity of the [b][m] scratch dV (0: none).
struct VerifyCallDev {
    DevBuf<uint8_t> arena;
    uint32_t *dPC = nullptr, *dR = nullptr, *dseed = nullptr, *dV = nullptr;
    uint8_t *dok = nullptr, *dsub = nullptr, *dpath = nullptr;
    uint64_t* dl = nullptr;              // the uploaded leaf indexes
    bool side_paths = false;
};
// (range_bytes: the bytes of range_proofs as a whole -- b blobs, or the compact buffer of host_verify_compact.inc)
static int32_t verify_upload_bytes_and_paths(dapol_ctx* ctx, ForkGuard& fg, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* leaf_C32,
                                             const uint8_t* leaf_H32, const uint8_t* path_C32, const uint8_t* path_H32, const uint8_t root_C32[32],
                                             const uint8_t root_H32[32], size_t range_bytes, const uint8_t* range_proofs, const uint8_t verify_seed32[32],
                                             size_t v_parties, VerifyCallDev& D) {
    hipStream_t st = ctx->stream;
    const size_t tot = b * (size_t)height;
    // One device arena for the call's inputs and verdict bytes; small calls also stage the nine host arrays into ONE upload
    // (a pageable-memory copy costs ~20 us of latency however small: 0.24 ms of a 2.2 ms single-proof check).
    const size_t hb = ctx_hash_bytes(ctx);                        // leaf_H32 / path_H32 / root_H32: hb bytes per node (32, or 64 for Blake2b)
    const size_t sizes[12] = {b * 8, b * 32, b * hb, tot * 32 + 32, tot * hb + 64, range_bytes, 32 + 64, 32, b, b, b, b * v_parties * 32};
    size_t offs[12], total = 0;
    for (int i = 0; i < 12; i++) { offs[i] = total; total += align_up(sizes[i], 256); }
    HIPCHK(D.arena.alloc(total));
    uint8_t* base = D.arena.p;
    uint64_t* dl = (uint64_t*)(base + offs[0]);
    uint32_t *dLC = (uint32_t*)(base + offs[1]), *dLH = (uint32_t*)(base + offs[2]), *dPC = (uint32_t*)(base + offs[3]), *dPH = (uint32_t*)(base + offs[4]);
    uint32_t *dR = (uint32_t*)(base + offs[5]), *droot = (uint32_t*)(base + offs[6]), *dseed = (uint32_t*)(base + offs[7]);
    uint8_t *dok = base + offs[8], *dsub = base + offs[9], *dpath = base + offs[10];
    uint32_t* dV = (uint32_t*)(base + offs[11]);
    const void* src[8] = {leaf_idx, leaf_C32, leaf_H32, path_C32, path_H32, range_proofs, nullptr, verify_seed32};
    const size_t src_bytes[8] = {b * 8, b * 32, b * hb, tot * 32, tot * hb, range_bytes, 32 + hb, 32};
    const size_t in_end = offs[8];                                  // the inputs are the arena's head
    if (in_end <= ((size_t)1 << 20)) {
        std::vector<uint8_t> stage(in_end, 0);
        for (int i = 0; i < 8; i++)
            if (src[i] && src_bytes[i]) memcpy(stage.data() + offs[i], src[i], src_bytes[i]);
        memcpy(stage.data() + offs[6], root_C32, 32);
        memcpy(stage.data() + offs[6] + 32, root_H32, hb);
        HIPCHK(hipMemcpyAsync(base, stage.data(), in_end, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));                           // (the staging vector dies with this scope)
    } else {
        for (int i = 0; i < 8; i++)
            if (src[i] && src_bytes[i]) HIPCHK(hipMemcpyAsync(base + offs[i], src[i], src_bytes[i], hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(droot, root_C32, 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(droot + 8, root_H32, hb, hipMemcpyHostToDevice, st));
    }
    // The Merkle re-merge and the range proofs are independent checks: a call of few proofs runs the path kernel on a side stream
    // under the range verification (its wavefront-per-path shape leaves the chip all but idle).
    const bool few = verify_paths_few(b), side_paths = verify_paths_side(b);
    hipStream_t sp = side_paths ? ctx->side[2] : st;
    if (side_paths) {
        HIPCHK(hipEventRecord(ctx->ev_fork, st));
        HIPCHK(hipStreamWaitEvent(sp, ctx->ev_fork, 0));
        fg.forked(2);
    }
    // few proofs: a wavefront per path (latency); many: a lane per path (3x less work per path)
    if (ctx_wide(ctx))                                           // 64-byte node hashes: the lane kernel (a wavefront's shuffled hash chain is a 32-byte affair)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_verify_paths<16, DG_RUNTIME>), dim3(nblk(b, 64)), dim3(64), 0, sp, ctx->tv.digest, b, height, dl, dLC, dLH, dPC, dPH, droot, droot + 8,
                           g_wire.siblings_leaf_first, dpath);
    else if (few)
        LAUNCH_DX(ctx->tv.digest, (k_verify_paths_wave<8, DX>), dim3((unsigned)b), dim3(64), 0, sp, ctx->tv.digest, b, height, dl, dLC, dLH, dPC, dPH, droot,
                           droot + 8, g_wire.siblings_leaf_first, dpath);
    else
        LAUNCH_DX(ctx->tv.digest, (k_verify_paths<8, DX>), dim3(nblk(b, 64)), dim3(64), 0, sp, ctx->tv.digest, b, height, dl, dLC, dLH, dPC, dPH, droot, droot + 8,
                           g_wire.siblings_leaf_first, dpath);
    LAUNCH_CHECK();
    if (side_paths) { HIPCHK(hipEventRecord(ctx->ev_join[2], sp)); FAULT_AFTER_FORK("verify_paths"); }
    HIPCHK(hipMemsetAsync(dok, 1, b, st));
    D.dPC = dPC; D.dR = dR; D.dseed = dseed; D.dV = dV;
    D.dok = dok; D.dsub = dsub; D.dpath = dpath;
    D.dl = dl;
    D.side_paths = side_paths;
    return DAPOL_OK;
}
static int32_t verify_upload_and_paths(dapol_ctx* ctx, ForkGuard& fg, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* leaf_C32,
                                       const uint8_t* leaf_H32, const uint8_t* path_C32, const uint8_t* path_H32, const uint8_t root_C32[32],
                                       const uint8_t root_H32[32], size_t es, const uint8_t* range_proofs, const uint8_t verify_seed32[32],
                                       size_t v_parties, VerifyCallDev& D) {
    return verify_upload_bytes_and_paths(ctx, fg, height, b, leaf_idx, leaf_C32, leaf_H32, path_C32, path_H32, root_C32, root_H32, b * es, range_proofs,
                                         verify_seed32, v_parties, D);
}

// DapolProof::verify (src/proof/mod.rs:41-47, :89-95) for b single-leaf proofs: Merkle re-merge, then R::verify over the
// sibling commitments (src/range/padding.rs:169-196, src/range/splitting.rs:181-210).
int32_t dapol_verify_entities(dapol_ctx* ctx, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* leaf_C32,
                              const uint8_t* leaf_H32, const uint8_t* path_C32, const uint8_t* path_H32, const uint8_t root_C32[32],
                              const uint8_t root_H32[32], int32_t policy, int32_t aggregation_factor, int32_t n_bits,
                              const uint8_t* range_proofs, const uint8_t verify_seed32[32], uint8_t* ok) {
    WIRE_SCOPE();
    if (!ctx || !root_C32 || !root_H32 || (b && (!leaf_idx || !leaf_C32 || !leaf_H32 || !path_C32 || !path_H32 || !range_proofs || !ok)))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    VERIFY_SEED_OR_OS(verify_seed32)
    if (height < 0 || height > 64) return fail(DAPOL_ERR_TREE_HEIGHT_TOO_BIG, "tree height must not exceed 64");
    std::vector<SubProof> plan;
    if (!policy_plan(policy, height, aggregation_factor, plan)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad policy / aggregation_factor");
    size_t es = dapol_entity_proof_size(height, policy, aggregation_factor, n_bits);
    if (es == 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad n_bits");
    if (b == 0) return DAPOL_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int max_m = 1;
    for (auto& s : plan) if (s.m > max_m) max_m = s.m;
    if (max_m > ctx->max_parties) return fail(DAPOL_ERR_INVALID_ARGUMENT, "aggregation needs more parties than the context was created for");
    VerifyCallDev D;
    ForkGuard fg(ctx);
    int32_t rc = verify_upload_and_paths(ctx, fg, height, b, leaf_idx, leaf_C32, leaf_H32, path_C32, path_H32, root_C32, root_H32, es, range_proofs,
                                         verify_seed32, (size_t)max_m, D);
    if (rc) return rc;
    rc = verify_policy_device(ctx, plan, b, height, D.dPC, D.dR, es / 4, n_bits, D.dseed, D.dok, D.dsub, D.dV);
    if (rc) return rc;                                            // (the guard waits for the path kernel)
    if (D.side_paths) { HIPCHK(hipStreamWaitEvent(st, ctx->ev_join[2], 0)); fg.joined(2); }
    hipLaunchKernelGGL(k_and_bytes, dim3(nblk(b, 256)), dim3(256), 0, st, b, D.dok, D.dpath);
    LAUNCH_CHECK();
    HIPCHK(hipMemcpy(ok, D.dok, b, hipMemcpyDeviceToHost));
    return DAPOL_OK;
}

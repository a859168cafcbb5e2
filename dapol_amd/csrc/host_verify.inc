// Batched verifier host side (kernels in kernels_verify.h).
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
enum { RLC_MIN_DEFAULT = 112 };       // measured (profiles/r02_midsize_ab.txt): 64 proofs 2.0 ms one by one against 2.2 ms batched, 128 proofs 2.8 against 2.7
static bool verify_wave_transcript(int m) {
    if (const char* e = knob("DAPOL_VERIFY_WAVE_TRANSCRIPT")) return atoi(e) != 0;
    return m >= 256;
}
static size_t verify_rlc_min(const dapol_ctx* ctx) {          // fewest proofs that are checked as ONE random linear combination
    size_t rlc_min = ctx->opt.verify_batch_min >= 2 ? (size_t)ctx->opt.verify_batch_min : RLC_MIN_DEFAULT;
    if (const char* e = knob("DAPOL_VERIFY_RLC_MIN")) { long v = atol(e); if (v >= 2) rlc_min = (size_t)v; }
    return rlc_min;
}
// queue_only: a call of ONE chunk returns with its work queued on ctx's stream, without the host wait at the end (the groups of a
// small call's plan on lanes of their own, verify_policy_device).
static int32_t range_verify_device(dapol_ctx* ctx, int n_bits, int m, size_t b, const uint32_t* d_proofs, size_t stride_words,
                                   const uint32_t* d_V, const uint32_t* d_seed, uint8_t* d_ok, bool queue_only = false) {
    hipStream_t st = ctx->stream;
    ForkGuard fg(ctx);
    VerifyArgs V{};
    RangeArgs& A = V.R;
    A.n = n_bits; A.m = m; A.N = n_bits * m;
    A.lgN = 0;
    while ((1 << A.lgN) < A.N) A.lgN++;
    if (A.lgN > RV_MAX_ROUNDS) return fail(DAPOL_ERR_INVALID_ARGUMENT, "proof too large");
    A.TP = 2 * A.N < 64 ? 64 : 2 * A.N;
    A.out_words = (int)stride_words;
    A.wbits = ctx->tv.wbits; A.nwin = ctx->tv.nwin_c();
    // A few proofs (someone checking their own): one proof per wavefront, the term range split finely and, with the tables'
    // high-half rows, half the window steps -- as the prover's small calls (host_range.inc).
    const bool small_call = b <= 128 && A.N >= 256 && !knob("DAPOL_NO_SPLIT");
    const bool use_hi = small_call && ctx->tv.hi_split && !knob("DAPOL_NO_SMALL_HI");
    const int lpl = small_call ? 32 : msm_lanes_per_list(A.N);
    A.use_hi = use_hi ? 1 : 0;
    // enough wavefronts to fill the chip even for a few large proofs: split each proof's term range
    {
        size_t waves = (b + (32 / lpl) - 1) / (32 / lpl);
        int niter_all = (A.N + lpl - 1) / lpl, ns = 1;
        if (small_call) { while (waves * ns < 4096 && niter_all / (ns * 2) >= (use_hi ? 2 : 4) && ns < small_split_cap(use_hi)) ns *= 2; }
        else { while (waves * ns < 4096 && niter_all / (ns * 2) >= 64 && ns < 256) ns *= 2; }
        A.nsplit = ns;
    }
    // ... and one point per four lanes (k_rp_msm_quad) when that many wavefronts are still few
    // (1.5x the work per point: it pays up to about 16 proofs, profiles/r02_midsize_ab.txt)
    const bool quad = use_hi && A.nsplit > 1 && (size_t)A.nsplit * 4 * b <= quad_max_waves(4096) && A.N % (8 * A.nsplit * 4) == 0 && !knob("DAPOL_NO_QUAD");
    if (quad) A.nsplit *= 4;
    V.lb = A.lgN / 2; V.hb = A.lgN - V.lb; V.tab_stride = rv_tab_entries(A.lgN, m);
    const int var_waves = (4 + 2 * A.lgN + m + 15) / 16;               // k_rv_varpoints_quad: wavefronts per proof
    const size_t per_proof = (size_t)A.nwin * A.TP * sizeof(dig_t) + align_up(sizeof(VerifyState), 16) + (3 + 2 * (size_t)A.nsplit + (size_t)var_waves) * 160 + 1 +
                             (size_t)V.tab_stride * sizeof(sc);
    size_t chunk = scratch_budget_bytes(ctx) / per_proof;
    if (chunk < 1) chunk = 1;
    if (chunk > b) chunk = b;
    if (chunk > 60000) chunk = 60000;
    HIPCHK(ctx->scratch.ensure(chunk * per_proof + 4096));
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
    const bool tree_sum = small_call && A.nsplit > 1;
    A.seed = d_seed;
    for (size_t first = 0; first < b; first += chunk) {
        size_t cb = b - first < chunk ? b - first : chunk;
        A.B = cb;
        A.out = const_cast<uint32_t*>(d_proofs) + first * stride_words;
        A.Vc = d_V + first * (size_t)m * 8;
        V.verdict = d_ok + first;
        const unsigned g_wave = (unsigned)cb, g_lane = nblk(cb, 64), g_dig = (unsigned)(cb * (size_t)(A.TP / 64));
        V.wave_transcript = verify_wave_transcript(m) ? 1 : 0;
        if (V.wave_transcript) { hipLaunchKernelGGL(k_rv_absorb_V, dim3(g_wave), dim3(64), 0, st, V, rv_transcript_head(A.n, A.m), 0, A.m); LAUNCH_CHECK(); }
        if (small_call && !knob("DAPOL_VERIFY_LANE_TRANSCRIPT")) hipLaunchKernelGGL(k_rv_transcript<1>, dim3(g_wave), dim3(64), 0, st, V);
        else hipLaunchKernelGGL(k_rv_transcript<0>, dim3(g_lane), dim3(64), 0, st, V);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(k_rv_weights, dim3(g_lane), dim3(64), 0, st, V, (const uint32_t*)nullptr); LAUNCH_CHECK();   // c from the proof's own digest
        // a small call's two point sums are independent and neither fills the chip: the proof's own points (k_rv_varpoints: needs the
        // challenges, the weights and the z-power table) run on a side stream under the generator MSM
        const bool side_var = small_call && !knob("DAPOL_VERIFY_ONE_STREAM");
        const bool quad_var = side_var && var_waves <= 16 && (size_t)var_waves * cb <= quad_max_waves(64) && !knob("DAPOL_NO_QUAD");      // (many-party proofs, or more than a few, keep a point per lane)
        hipLaunchKernelGGL(k_rv_tables, dim3((unsigned)(cb * (size_t)((V.tab_stride + 63) / 64))), dim3(64), 0, st, V); LAUNCH_CHECK();
        if (side_var) {
            HIPCHK(hipEventRecord(ctx->ev_fork, st));
            HIPCHK(hipStreamWaitEvent(ctx->side[1], ctx->ev_fork, 0));
            fg.forked(1);
            if (quad_var) {
                hipLaunchKernelGGL(k_rv_varpoints_quad, dim3((unsigned)(cb * (size_t)var_waves)), dim3(64), 0, ctx->side[1], V, var_parts, var_waves); LAUNCH_CHECK();
                hipLaunchKernelGGL(k_rv_sum_parts, dim3(g_wave), dim3(64), 0, ctx->side[1], cb, var_waves, var_parts, A.PA); LAUNCH_CHECK();
            } else {
                hipLaunchKernelGGL(k_rv_varpoints, dim3(g_wave), dim3(64), 0, ctx->side[1], V); LAUNCH_CHECK();
            }
            HIPCHK(hipEventRecord(ctx->ev_join[1], ctx->side[1]));
            FAULT_AFTER_FORK("verify_var");
        }
        hipLaunchKernelGGL(k_rv_scalars, dim3(g_dig), dim3(64), 0, st, V); LAUNCH_CHECK();
        if (quad) hipLaunchKernelGGL(k_rp_msm_quad, dim3((unsigned)(cb * (size_t)A.nsplit)), dim3(64), 0, st, A, ctx->tv, -1);
        else launch_msm(st, A, ctx->tv, -1, lpl);
        LAUNCH_CHECK();
        if (side_var) { HIPCHK(hipStreamWaitEvent(st, ctx->ev_join[1], 0)); fg.joined(1); }
        else { hipLaunchKernelGGL(k_rv_varpoints, dim3(g_wave), dim3(64), 0, st, V); LAUNCH_CHECK(); }
        if (tree_sum) {
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
// The commitments of a batch that are still on their way from the host when the check starts (dapol_range_verify_batch): they arrive
// in K column blocks -- block k = commitments [k m / K, (k + 1) m / K) of EVERY proof -- fetch(k) issues block k's copy and records
// ev[k].  The transcript replay (k_rv_absorb_V, a 1.4 ms latency chain for 1,024 parties whatever the batch size; 2.2 ms before round 5's changes to it) runs in K phases,
// each behind its block, so the copy of the other blocks hides under it instead of preceding it.
struct VArrival {
    int K = 0;
    std::function<int32_t(int)> fetch;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
};
static int32_t range_verify_rlc_device(dapol_ctx* ctx, int n_bits, int m, size_t b, const uint32_t* d_proofs, size_t stride_words,
                                       const uint32_t* d_V, const uint32_t* d_seed, uint8_t* d_ok, VArrival* va = nullptr) {
    auto fetch_all = [&]() -> int32_t {                      // no pipelining on this path: have every block land before anything reads it
        for (int k = 0; va && k < va->K; k++) {
            int32_t rc = va->fetch(k);
            if (rc) return rc;
            HIPCHK(hipStreamWaitEvent(ctx->stream, va->ev[k], 0));
        }
        va = nullptr;
        return DAPOL_OK;
    };
    // A handful of proofs are checked one by one: the per-proof path's small-call shapes (a wavefront or a quad of lanes per unit of
    // work) finish sooner than the batched check's longer chain of launches (DAPOL_VERIFY_RLC_MIN: fewest proofs that are batched).
    const size_t rlc_min = verify_rlc_min(ctx);
    if (b < rlc_min || knob("DAPOL_VERIFY_NO_RLC")) {
        int32_t rc = fetch_all();
        if (rc) return rc;
        return range_verify_device(ctx, n_bits, m, b, d_proofs, stride_words, d_V, d_seed, d_ok);
    }
    hipStream_t st = ctx->stream;
    ForkGuard fg(ctx);
    RlcArgs R{};
    VerifyArgs& V = R.V;
    RangeArgs& A = V.R;
    A.n = n_bits; A.m = m; A.N = n_bits * m;
    A.lgN = 0;
    while ((1 << A.lgN) < A.N) A.lgN++;
    if (A.lgN > RV_MAX_ROUNDS) return fail(DAPOL_ERR_INVALID_ARGUMENT, "proof too large");
    A.TP = 2 * A.N < 64 ? 64 : 2 * A.N;
    A.out_words = (int)stride_words;
    A.wbits = ctx->tv.wbits; A.nwin = ctx->tv.nwin_c();
    A.seed = d_seed;
    int lpl = msm_lanes_per_list(A.N);
    {   // the ONE generator MSM of a chunk: split its term range over enough wavefronts to fill the chip
        int niter_all = (A.N + lpl - 1) / lpl, ns = 1;
        while (ns < 1024 && niter_all / (ns * 2) >= 8) ns *= 2;
        A.nsplit = ns;
    }
    // It is a lone MSM whatever the batch: with the tables' high-half rows it takes the small-call shape of the prover's -- one point per
    // four lanes, a term per group (k_rp_msm_quad: 0.72 -> 0.15 ms for 64-bit, 32-party proofs); DAPOL_NO_QUAD=1 keeps the lane kernel.
    const bool quad_gen = ctx->tv.hi_split && A.N >= 256 && A.N % 8 == 0 && A.N / 8 <= 1024 && !knob("DAPOL_NO_QUAD") && !knob("DAPOL_NO_SMALL_HI");
    if (quad_gen) { A.nsplit = A.N / 8; A.use_hi = 1; lpl = 32; }
    // Large proofs without high-half rows (the 1,024-party context): the generator MSM as window sweeps without doublings
    // (k_rvb_gen_sweep / k_rvb_gen_windows, kernels_verify.h).  DAPOL_VERIFY_GEN_STRAUS=1 keeps the Straus kernel.
    const bool gen_sweep = !quad_gen && A.N >= 4096 && !knob("DAPOL_VERIFY_GEN_STRAUS");
    int gen_ns = 1;
    if (gen_sweep) {
        while ((size_t)A.nwin * (size_t)gen_ns * 2 <= (size_t)ctx->n_cu * 8 && (2 * A.N) / (gen_ns * 2 * 64) >= 8) gen_ns *= 2;   // >= 2 wavefronts per SIMD, >= 8 terms per lane
        A.nsplit = A.nwin;                                     // k_rvb_finish adds nwin window points (P0) + identities (P1)
    }
    R.K = 4 + 2 * A.lgN + m;
    V.lb = A.lgN / 2; V.hb = A.lgN - V.lb; V.tab_stride = rv_tab_entries_rlc(A.lgN, m);
    const size_t per_proof = align_up(sizeof(VerifyState), 16) + 2 * sizeof(sc) + (size_t)V.tab_stride * sizeof(sc) +
                             (size_t)(3 * (1 << V.hb) + 3 * (1 << V.lb)) * 48 +
                             (size_t)R.K * ((size_t)PT_ROW_WORDS * 4 + (size_t)PT_NWIN * sizeof(dig_t) * 2) + 64;
    const size_t fixed = (size_t)A.nwin * A.TP * sizeof(dig_t) + 64 * (size_t)A.TP * sizeof(sc) + 4 * 160 * 20000 + (1 << 20);
    size_t budget = scratch_budget_bytes(ctx);
    size_t chunk = budget > fixed ? (budget - fixed) / per_proof : 1;
    if (chunk < 2) chunk = 2;
    if (chunk > b) chunk = b;
    if (chunk > 262144) chunk = 262144;
    const int nch = A.TP >> 6;
    if (va && (chunk < b || !verify_wave_transcript(m) || va->K < 2 || m % va->K)) { int32_t rc = fetch_all(); if (rc) return rc; }
    for (size_t first = 0; first < b; first += chunk) {
        size_t cb = b - first < chunk ? b - first : chunk;
        A.B = cb;
        // groups: enough blocks to fill the chip, at most one group per proof
        R.G = (int)std::min<size_t>(cb / 2 + 1, std::max<size_t>(1, (size_t)16384 / (size_t)nch));
        if (R.G > 64) R.G = 64;
        R.npts = cb * (size_t)R.K;
        R.Np = (R.npts + 1) / 2;
        const size_t niter2 = (R.Np + 31) / 32;
        R.TP2 = (int)(64 * niter2);
        R.ns2 = (int)std::min<size_t>(16384, std::max<size_t>(1, niter2 / 2));      // two points per lane: the 252 shared doublings are the chain
        size_t need = 0;
        auto take = [&](size_t bytes) { size_t o = need; need += align_up(bytes, 256); return o; };
        const size_t o_dig = take((size_t)A.nwin * A.TP * sizeof(dig_t)), o_vs = take(cb * sizeof(VerifyState)),
                     o_p0 = take((size_t)A.nsplit * 160), o_p1 = take((size_t)A.nsplit * 160), o_part = take((size_t)R.G * A.TP * sizeof(sc)),
                     o_gpart = take(gen_sweep ? (size_t)A.nwin * gen_ns * 160 : 16),
                     o_bsum = take(cb * 2 * sizeof(sc)), o_pt = take(2 * R.Np * (size_t)PT_ROW_WORDS * 4),
                     o_dig2 = take((size_t)PT_NWIN * R.TP2 * sizeof(dig_t)), o_q0 = take((size_t)R.ns2 * 160), o_q1 = take((size_t)R.ns2 * 160),
                     o_flag = take(16), o_tabs = take(cb * (size_t)V.tab_stride * sizeof(sc)),
                     o_dga = take(((cb + 30) / 31 + 1) * 32), o_dgb = take(((cb + 30) / 31 / 31 + 2) * 32);
        // lazy generator scalars: limb copies of the product tables (needs the one-side-per-wavefront mapping, N >= 64)
        const size_t per29 = (size_t)(3 * (1 << V.hb) + 3 * (1 << V.lb)) * 12 * sizeof(uint32_t);
        R.lazy = (nch > 1 && !knob("DAPOL_VERIFY_GH_EAGER")) ? 1 : 0;
        const size_t o_t29 = take(R.lazy ? cb * per29 : 16), o_rzg = take((size_t)R.G * sizeof(sc));
        HIPCHK(ctx->scratch.ensure(need + 4096));
        uint8_t* base = (uint8_t*)ctx->scratch.p;
        A.dig = (dig_t*)(base + o_dig); V.vs = (VerifyState*)(base + o_vs);
        A.P0 = (int32_t*)(base + o_p0); A.P1 = (int32_t*)(base + o_p1);
        R.partial = (sc*)(base + o_part); R.bsum = (sc*)(base + o_bsum);
        R.ptT = (int32_t*)(base + o_pt); R.dig2 = (dig_t*)(base + o_dig2);
        R.Q0 = (int32_t*)(base + o_q0); R.Q1 = (int32_t*)(base + o_q1);
        R.flag = (uint32_t*)(base + o_flag);
        V.tabs = (sc*)(base + o_tabs);
        R.tab29 = (uint32_t*)(base + o_t29); R.rzg = (sc*)(base + o_rzg);
        A.out = const_cast<uint32_t*>(d_proofs) + first * stride_words;
        A.Vc = d_V + first * (size_t)m * 8;
        V.verdict = d_ok + first;
        HIPCHK(hipMemsetAsync(R.flag, 0, 16, st));
        // the proofs' own points: bucket method for large batches, per-point tables + Straus otherwise
        size_t pip_min = 32768;                                   // DAPOL_VERIFY_PIPPENGER_MIN=<points> moves the switch (tests), 0 disables
        if (const char* e = knob("DAPOL_VERIFY_PIPPENGER_MIN")) { long v = atol(e); pip_min = v <= 0 ? (size_t)-1 : (size_t)std::max<long>(v, 12288); }
        const bool pippenger = R.npts >= pip_min;
        size_t hsz = 0;
        V.wave_transcript = verify_wave_transcript(m) ? 1 : 0;
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
        if (pippenger) {
            // carved out of the per-point table region (1,152 bytes per point there, 260 here)
            uint8_t* q = (uint8_t*)R.ptT;
            R.pN = (int32_t*)q; q += align_up(R.npts * 128, 256);
            R.pdig = (int16_t*)q; q += align_up((size_t)RVP_NW * R.npts * 2, 256);
            R.psorted = (uint32_t*)q; q += align_up((size_t)RVP_NW * R.npts * 4, 256);
            hsz = align_up((size_t)RVP_NW * (RVP_NB + 1) * 4, 256);
            R.phist = (uint32_t*)q; q += hsz;
            R.poffs = (uint32_t*)q; q += hsz;
            R.pcursor = (uint32_t*)q; q += hsz;
            R.pbsum = (int32_t*)q; q += (size_t)RVP_NW * RVP_NB * 160;
            if ((size_t)(q - (uint8_t*)R.ptT) > 2 * R.Np * (size_t)PT_ROW_WORDS * 4)
                return fail(DAPOL_ERR_OUT_OF_MEMORY, "bucket-method scratch does not fit the per-point table region");
            // decode on a side stream, beside the transcript replay (which occupies one wavefront per SIMD at most)
            HIPCHK(hipStreamWaitEvent(ctx->side[0], ctx->ev_fork, 0));
            if (va) HIPCHK(hipStreamWaitEvent(ctx->side[0], va->ev[va->K - 1], 0));      // (all the commitments: the last block lands last)
            fg.forked(0);
            hipLaunchKernelGGL(k_rvp_decode, dim3(nblk(R.npts, 64)), dim3(64), 0, ctx->side[0], R); LAUNCH_CHECK();
            HIPCHK(hipEventRecord(ctx->ev_join[0], ctx->side[0]));
            FAULT_AFTER_FORK("verify_decode");
        }
        if (V.wave_transcript && !absorbed) { hipLaunchKernelGGL(k_rv_absorb_V, dim3((unsigned)cb), dim3(64), 0, st, V, rv_transcript_head(A.n, A.m), 0, A.m); LAUNCH_CHECK(); }
        // up to a few thousand proofs the replay is a lane's latency (1.0 ms), so a wavefront replays each proof (0.5 ms)
        if (cb <= 4096 && !knob("DAPOL_VERIFY_LANE_TRANSCRIPT")) hipLaunchKernelGGL(k_rv_transcript<1>, dim3((unsigned)cb), dim3(64), 0, st, V);
        else hipLaunchKernelGGL(k_rv_transcript<0>, dim3(nblk(cb, 64)), dim3(64), 0, st, V);
        LAUNCH_CHECK();
        {   // the batch digest D (BLAKE3 tree over the per-proof digests) and from it every proof's c and rho
            uint32_t* bufs[2] = {(uint32_t*)(base + o_dga), (uint32_t*)(base + o_dgb)};
            const uint32_t* in = V.vs[0].dg;        // (address arithmetic only: vs is a device pointer)
            size_t stride = sizeof(VerifyState) / 4, n = cb;
            int level = 0;
            do {
                uint32_t* out = bufs[level & 1];
                hipLaunchKernelGGL(k_rv_digest_level, dim3(nblk((n + 30) / 31, 64)), dim3(64), 0, st, n, level, in, stride, out); LAUNCH_CHECK();
                in = out; stride = 8; n = (n + 30) / 31; level++;
            } while (n > 1);
            hipLaunchKernelGGL(k_rv_weights, dim3(nblk(cb, 64)), dim3(64), 0, st, V, in); LAUNCH_CHECK();
        }
        // Round 5: from here the pass has two independent halves -- the generator scalars with their one MSM (product tables, 2 x 65,536
        // sums over the proofs, VALU-bound) and the batch's own points by the bucket method (digits, counting sort, bucket and window
        // sums: memory- and latency-bound, ending in 23 lone wavefronts).  They used to queue behind each other on one stream; the
        // own points now follow their decode on the side stream and the two halves meet again at k_rvb_finish.
        const int ns2_saved = R.ns2;
        const bool fork_points = pippenger && !knob("DAPOL_VERIFY_ONE_STREAM");
        auto own_points_bucket = [&](hipStream_t sb) -> int32_t {
            HIPCHK(hipMemsetAsync(R.phist, 0, hsz, sb));
            const unsigned runs = nblk(R.npts, RVP_RUN);
            hipLaunchKernelGGL(k_rvp_digits, dim3(runs), dim3(RVP_BLOCK), 0, sb, R); LAUNCH_CHECK();
            hipLaunchKernelGGL(k_rvp_scan, dim3(RVP_NW), dim3(64), 0, sb, R); LAUNCH_CHECK();
            hipLaunchKernelGGL(k_rvp_scatter, dim3(8 * runs), dim3(RVP_BLOCK), 0, sb, R); LAUNCH_CHECK();
            hipLaunchKernelGGL(k_rvp_buckets, dim3((unsigned)((size_t)RVP_NW * RVP_NB * RVP_S / 64)), dim3(64), 0, sb, R); LAUNCH_CHECK();
            hipLaunchKernelGGL(k_rvp_window, dim3(RVP_NW), dim3(64), 0, sb, R); LAUNCH_CHECK();
            return DAPOL_OK;
        };
        if (pippenger) R.ns2 = RVP_NW;
        // k_rv_tables BEFORE the fork: the own points' digits (k_rvp_digits -> rv_own_point) read its z^2 z^j entries for the commitment
        // terms.  (Round 5 launched it after the fork, unordered against the side stream: with the same proofs in every pass the
        // scratch still held the right values, which hid it -- ADVICE r5, high.)
        hipLaunchKernelGGL(k_rv_tables, dim3((unsigned)(cb * (size_t)((V.tab_stride + 63) / 64))), dim3(64), 0, st, V); LAUNCH_CHECK();
        if (fork_points) {
            HIPCHK(hipEventRecord(ctx->ev_fork, st));                    // the weights, the tables (and everything the replay left in vs) are there
            HIPCHK(hipStreamWaitEvent(ctx->side[0], ctx->ev_fork, 0));   // (side[0] already holds the decode)
            int32_t rc = own_points_bucket(ctx->side[0]);
            if (rc) return rc;
            HIPCHK(hipEventRecord(ctx->ev_join[0], ctx->side[0]));
        }
        hipLaunchKernelGGL(k_rvb_tables2, dim3((unsigned)(cb * (size_t)((V.tab_stride - rv_tab_entries(A.lgN, m) + (R.lazy ? (1 << V.lb) : 0) + 63) / 64))),
                           dim3(64), 0, st, R);
        LAUNCH_CHECK();
        if (R.lazy) {
            hipLaunchKernelGGL(k_rvb_rzsum, dim3((unsigned)R.G), dim3(64), 0, st, R); LAUNCH_CHECK();
            hipLaunchKernelGGL(k_rvb_gh_lazy, dim3((unsigned)(nch * R.G)), dim3(64), 0, st, R); LAUNCH_CHECK();
        } else {
            hipLaunchKernelGGL(k_rvb_gh_partial, dim3((unsigned)(nch * R.G)), dim3(64), 0, st, R); LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_rvb_gh_reduce, dim3((unsigned)nch), dim3(64), 0, st, R); LAUNCH_CHECK();
        {
            RangeArgs A1 = A;
            A1.B = 1;
            if (quad_gen) hipLaunchKernelGGL(k_rp_msm_quad, dim3((unsigned)A1.nsplit), dim3(64), 0, st, A1, ctx->tv, -1);
            else if (gen_sweep) {
                int32_t* gpart = (int32_t*)(base + o_gpart);
                hipLaunchKernelGGL(k_rvb_gen_sweep, dim3((unsigned)(A1.nwin * gen_ns)), dim3(64), 0, st, A1, ctx->tv, gen_ns, gpart); LAUNCH_CHECK();
                hipLaunchKernelGGL(k_rvb_gen_windows, dim3((unsigned)A1.nwin), dim3(64), 0, st, A1, gen_ns, gpart);
            } else launch_msm(st, A1, ctx->tv, -1, lpl);
            LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_rvb_base_scalars, dim3(nblk(cb, 64)), dim3(64), 0, st, R); LAUNCH_CHECK();
        if (pippenger) {
            HIPCHK(hipStreamWaitEvent(st, ctx->ev_join[0], 0));       // the decoded points -- or, forked, the window sums made from them
            fg.joined(0);
            if (!fork_points) { int32_t rc = own_points_bucket(st); if (rc) return rc; }
            hipLaunchKernelGGL(k_rvb_finish, dim3(1), dim3(64), 0, st, R, ctx->tv); LAUNCH_CHECK();
            R.ns2 = ns2_saved;
        } else {
        hipLaunchKernelGGL(k_rvb_points, dim3(nblk(2 * R.Np, 64)), dim3(64), 0, st, R); LAUNCH_CHECK();
        {
            RangeArgs A2{};
            A2.N = (int)R.Np; A2.TP = R.TP2; A2.wbits = PT_WBITS; A2.nwin = PT_NWIN; A2.B = 1; A2.nsplit = R.ns2;
            A2.dig = R.dig2; A2.P0 = R.Q0; A2.P1 = R.Q1;
            const TableView tvp{R.ptT, 1, PT_WBITS, 0, 0};
            hipLaunchKernelGGL((k_rp_msm<MSM_TAIL, 32>), dim3((unsigned)R.ns2), dim3(64), 0, st, A2, tvp, -1); LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_rvb_finish, dim3(1), dim3(64), 0, st, R, ctx->tv); LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_rvb_verdicts, dim3(nblk(cb, 256)), dim3(256), 0, st, V); LAUNCH_CHECK();
        uint32_t h_flag[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(h_flag, R.flag, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!h_flag[0] || h_flag[1]) {          // some proof of the chunk is bad: find out which
            g_verify_fallbacks.fetch_add(1, std::memory_order_relaxed);
            if (cb >= 64) {
                // narrow it down with the same batched check on eight parts (a part that passes vouches for its proofs; a part
                // that fails is split again, down to the proof-by-proof check): one bad proof among 1,024 costs a few batched
                // checks of shrinking size instead of 1,024 single ones
                const size_t part = (cb + 7) / 8;
                for (size_t o = 0; o < cb; o += part) {
                    const size_t n = std::min(part, cb - o);
                    int32_t rc = range_verify_rlc_device(ctx, n_bits, m, n, d_proofs + (first + o) * stride_words, stride_words,
                                                         d_V + (first + o) * (size_t)m * 8, d_seed, d_ok + first + o);
                    if (rc) return rc;
                }
            } else {
                int32_t rc = range_verify_device(ctx, n_bits, m, cb, d_proofs + first * stride_words, stride_words, d_V + first * (size_t)m * 8,
                                                 d_seed, d_ok + first);
                if (rc) return rc;
            }
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
    const bool pipe = verify_wave_transcript(m) && m % 4 == 0 && b * (size_t)m * 32 >= ((size_t)8 << 20) && !knob("DAPOL_VERIFY_NO_PIPELINE");
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
// them -- as the prover groups them, host_range.inc) is ONE batched check of b * k proofs: their words gathered into a contiguous
// batch, commitments [b * k][m], the entity's verdict the AND over its k sub-proofs (round 6; DAPOL_NO_GROUP=1: one check per sub-proof).
static int32_t verify_policy_device(dapol_ctx* ctx, const std::vector<SubProof>& plan, size_t b, int H, const uint32_t* dPC, const uint32_t* dR,
                                    size_t entity_words, int n_bits, const uint32_t* dseed, uint8_t* dok, uint8_t* dsub, uint32_t* dV) {
    hipStream_t st = ctx->stream;
    const uint32_t* Bb_comp = ctx->gens_comp.p + (size_t)ctx->tv.row_Bb(0) * 8;
    struct Group { int start, count, m, k; };
    std::vector<Group> groups;
    const bool group = !knob("DAPOL_NO_GROUP");
    for (auto& s : plan) {
        if (group && !groups.empty() && groups.back().m == s.m && groups.back().count == s.m && s.count == s.m &&
            groups.back().start + groups.back().k * s.m == s.start) groups.back().k++;
        else groups.push_back({s.start, s.count, s.m, 1});
    }
    size_t g_words = 0, g_parties = 0, g_proofs = 0;           // what the grouped checks need beside the caller's [b]-sized buffers
    for (auto& g : groups)
        if (g.k > 1) {
            const size_t pw = dapol_range_proof_size(n_bits, g.m) / 4;
            g_words = std::max(g_words, b * (size_t)g.k * pw);
            g_parties = std::max(g_parties, b * (size_t)g.k * (size_t)g.m);
            g_proofs = std::max(g_proofs, b * (size_t)g.k);
        }
    // A SMALL call with several groups (as the prover, host_range.inc): the per-proof checks of the groups side by side, each on a
    // lane of its own, queued without a host wait; the verdicts are ANDed on the context's stream behind the lanes' events.
    size_t sum_proofs = 0, sum_parties = 0, sum_words = 0, max_gk = 1;
    for (auto& g : groups) {
        sum_proofs += (size_t)g.k; sum_parties += (size_t)g.k * (size_t)g.m; sum_words += (size_t)g.k * (dapol_range_proof_size(n_bits, g.m) / 4);
        max_gk = std::max(max_gk, (size_t)g.k);
    }
    if (groups.size() >= 2 && groups.size() <= 16 && b * sum_proofs <= 64 && b * max_gk < verify_rlc_min(ctx) && !knob("DAPOL_NO_LANES") && !knob("DAPOL_VERIFY_NO_RLC")) {
        DevBuf<uint32_t> arena;
        const size_t o_V = align_up(b * sum_words * 4, 256), o_sub = o_V + align_up(b * sum_parties * 32, 256), total = o_sub + align_up(b * sum_proofs, 256);
        HIPCHK(arena.alloc(total / 4 + 64));
        uint32_t* const aR = arena.p;
        uint32_t* const aV = (uint32_t*)((uint8_t*)arena.p + o_V);
        uint8_t* const asub = (uint8_t*)arena.p + o_sub;
        std::vector<size_t> offR(groups.size()), offV(groups.size()), offS(groups.size());
        size_t word_off = 0, r_off = 0, v_off = 0, s_off = 0;
        for (size_t gi = 0; gi < groups.size(); gi++) {
            auto& g = groups[gi];
            const size_t pw = dapol_range_proof_size(n_bits, g.m) / 4, np = b * (size_t)g.k;
            offR[gi] = r_off; offV[gi] = v_off; offS[gi] = s_off;
            if (g.k == 1) hipLaunchKernelGGL(k_gather_commitments, dim3(nblk(b * (size_t)g.m, 256)), dim3(256), 0, st, b, H, g.start, g.count, g.m, dPC, Bb_comp, aV + v_off * 8);
            else hipLaunchKernelGGL(k_gather_commitments_grouped, dim3(nblk(np * (size_t)g.m, 256)), dim3(256), 0, st, b, H, g.start, g.m, g.k, dPC, aV + v_off * 8);
            LAUNCH_CHECK();
            hipLaunchKernelGGL(k_gather_words_grouped, dim3(nblk(np * pw, 256)), dim3(256), 0, st, b, g.k, pw, entity_words, word_off, dR, aR + r_off);
            LAUNCH_CHECK();
            word_off += pw * (size_t)g.k; r_off += np * pw; v_off += np * (size_t)g.m; s_off += np;
        }
        HIPCHK(hipEventRecord(ctx->ev_v[0], st));
        int32_t rc = DAPOL_OK;
        std::vector<dapol_ctx*> lanes(groups.size(), nullptr);
        for (size_t gi = 0; gi < groups.size() && !rc; gi++) {
            auto& g = groups[gi];
            const size_t pw = dapol_range_proof_size(n_bits, g.m) / 4;
            rc = ctx_lane(ctx, (int)(gi % 4), &lanes[gi]);
            if (rc) break;
            dapol_ctx* lane = lanes[gi];
            if (lane != ctx) HIPCHK(hipStreamWaitEvent(lane->stream, ctx->ev_v[0], 0));
            rc = range_verify_device(lane, n_bits, g.m, b * (size_t)g.k, aR + offR[gi], pw, aV + offV[gi] * 8, dseed, asub + offS[gi], true);
            if (rc) break;
            if (lane != ctx) {                                  // the context's stream takes the verdicts behind the lane (one event per lane and use)
                HIPCHK(hipEventRecord(lane->ev_v[1 + (gi / 4) % 3], lane->stream));
                HIPCHK(hipStreamWaitEvent(st, lane->ev_v[1 + (gi / 4) % 3], 0));
            }
            hipLaunchKernelGGL(k_and_bytes_grouped, dim3(nblk(b, 256)), dim3(256), 0, st, b, g.k, dok, asub + offS[gi]);
            LAUNCH_CHECK();
        }
        for (auto* l : lanes) if (l && l != ctx) (void)hipStreamSynchronize(l->stream);      // (every lane drains before the arena is freed)
        HIPCHK(hipStreamSynchronize(st));
        return rc;
    }
    DevBuf<uint32_t> garena;
    uint32_t *gR = nullptr, *gV = nullptr;
    uint8_t* gsub = nullptr;
    if (g_proofs) {
        const size_t o_V = align_up(g_words * 4, 256), o_sub = o_V + align_up(g_parties * 32, 256), total = o_sub + align_up(g_proofs, 256);
        HIPCHK(garena.alloc(total / 4 + 64));
        gR = garena.p; gV = (uint32_t*)((uint8_t*)garena.p + o_V); gsub = (uint8_t*)garena.p + o_sub;
    }
    size_t word_off = 0;
    for (auto& g : groups) {
        const size_t pw = dapol_range_proof_size(n_bits, g.m) / 4;
        if (g.k == 1) {
            hipLaunchKernelGGL(k_gather_commitments, dim3(nblk(b * (size_t)g.m, 256)), dim3(256), 0, st, b, H, g.start, g.count, g.m, dPC, Bb_comp, dV);
            LAUNCH_CHECK();
            int32_t rc = range_verify_rlc_device(ctx, n_bits, g.m, b, dR + word_off, entity_words, dV, dseed, dsub);
            if (rc) return rc;
            hipLaunchKernelGGL(k_and_bytes, dim3(nblk(b, 256)), dim3(256), 0, st, b, dok, dsub);
            LAUNCH_CHECK();
        } else {
            const size_t np = b * (size_t)g.k;
            hipLaunchKernelGGL(k_gather_commitments_grouped, dim3(nblk(np * (size_t)g.m, 256)), dim3(256), 0, st, b, H, g.start, g.m, g.k, dPC, gV);
            LAUNCH_CHECK();
            hipLaunchKernelGGL(k_gather_words_grouped, dim3(nblk(np * pw, 256)), dim3(256), 0, st, b, g.k, pw, entity_words, word_off, dR, gR);
            LAUNCH_CHECK();
            int32_t rc = range_verify_rlc_device(ctx, n_bits, g.m, np, gR, pw, gV, dseed, gsub);
            if (rc) return rc;
            hipLaunchKernelGGL(k_and_bytes_grouped, dim3(nblk(b, 256)), dim3(256), 0, st, b, g.k, dok, gsub);
            LAUNCH_CHECK();
        }
        word_off += pw * (size_t)g.k;
    }
    HIPCHK(hipStreamSynchronize(st));                          // (the grouped batch's arena dies with this scope)
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
    bool side_paths = false;
};
static int32_t verify_upload_and_paths(dapol_ctx* ctx, ForkGuard& fg, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* leaf_C32,
                                       const uint8_t* leaf_H32, const uint8_t* path_C32, const uint8_t* path_H32, const uint8_t root_C32[32],
                                       const uint8_t root_H32[32], size_t es, const uint8_t* range_proofs, const uint8_t verify_seed32[32],
                                       size_t v_parties, VerifyCallDev& D) {
    hipStream_t st = ctx->stream;
    const size_t tot = b * (size_t)height;
    // One device arena for the call's inputs and verdict bytes; small calls also stage the nine host arrays into ONE upload
    // (a pageable-memory copy costs ~20 us of latency however small: 0.24 ms of a 2.2 ms single-proof check).
    const size_t hb = ctx_hash_bytes(ctx);                        // leaf_H32 / path_H32 / root_H32: hb bytes per node (32, or 64 for Blake2b)
    const size_t sizes[12] = {b * 8, b * 32, b * hb, tot * 32 + 32, tot * hb + 64, b * es, 32 + 64, 32, b, b, b, b * v_parties * 32};
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
    const size_t src_bytes[8] = {b * 8, b * 32, b * hb, tot * 32, tot * hb, b * es, 32 + hb, 32};
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
    const bool few = b <= 16384 && !knob("DAPOL_PATHS_LANE");
    const bool side_paths = few && b <= 64 && !knob("DAPOL_VERIFY_ONE_STREAM");
    hipStream_t sp = side_paths ? ctx->side[2] : st;
    if (side_paths) {
        HIPCHK(hipEventRecord(ctx->ev_fork, st));
        HIPCHK(hipStreamWaitEvent(sp, ctx->ev_fork, 0));
        fg.forked(2);
    }
    // few proofs: a wavefront per path (latency); many: a lane per path (3x less work per path)
    if (ctx_wide(ctx))                                           // 64-byte node hashes: the lane kernel (a wavefront's shuffled hash chain is a 32-byte affair)
        hipLaunchKernelGGL(k_verify_paths<16>, dim3(nblk(b, 64)), dim3(64), 0, sp, ctx->tv.digest, b, height, dl, dLC, dLH, dPC, dPH, droot, droot + 8,
                           g_wire.siblings_leaf_first, dpath);
    else if (few)
        hipLaunchKernelGGL(k_verify_paths_wave<8>, dim3((unsigned)b), dim3(64), 0, sp, ctx->tv.digest, b, height, dl, dLC, dLH, dPC, dPH, droot,
                           droot + 8, g_wire.siblings_leaf_first, dpath);
    else
        hipLaunchKernelGGL(k_verify_paths<8>, dim3(nblk(b, 64)), dim3(64), 0, sp, ctx->tv.digest, b, height, dl, dLC, dLH, dPC, dPH, droot, droot + 8,
                           g_wire.siblings_leaf_first, dpath);
    LAUNCH_CHECK();
    if (side_paths) { HIPCHK(hipEventRecord(ctx->ev_join[2], sp)); FAULT_AFTER_FORK("verify_paths"); }
    HIPCHK(hipMemsetAsync(dok, 1, b, st));
    D.dPC = dPC; D.dR = dR; D.dseed = dseed; D.dV = dV;
    D.dok = dok; D.dsub = dsub; D.dpath = dpath;
    D.side_paths = side_paths;
    return DAPOL_OK;
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

// Host orchestration of the batched range prover: the plan of a call (prove_plan.inc) turned into launches.
// Included from dapol_hip.hip; the policy layer on top of it is host_policy.inc.

#include <cstdlib>
#include "policy_plan.inc"
#include "prove_plan.inc"

struct MsmTiming {                       // HIP-event timing of the fixed-base MSM kernels, on the stream they run on
    // Brackets come in two kinds: 0 = the plain MSMs (S commitment, never-fold rounds: k_rp_msm_gs / k_rp_msm<0, .>),
    // 1 = the materialisation of the folded generators (k_rp_mat_gs / k_rp_msm<1, .>).  kernels[k] counts the launches of the
    // dominant kernel inside the brackets of kind k (a generator-stationary MSM is a few hundred tile launches).
    std::vector<hipEvent_t> ev;
    std::vector<int> kind;                // per bracket
    size_t used = 0;
    bool enabled = false;
    size_t kernels[2] = {0, 0};
    ~MsmTiming() { for (auto e : ev) (void)hipEventDestroy(e); }
    hipError_t mark(hipStream_t st, int k = 0) {
        if (!enabled) return hipSuccess;
        if (used == ev.size()) {
            hipEvent_t e;
            hipError_t r = hipEventCreate(&e);
            if (r != hipSuccess) return r;
            ev.push_back(e);
        }
        if ((used & 1) == 0) { if (kind.size() <= used / 2) kind.push_back(k); else kind[used / 2] = k; }
        return hipEventRecord(ev[used++], st);
    }
    void count(int k, size_t n) { if (enabled) kernels[k] += n; }
    // Time during which at least one bracket of kind k (k < 0: of either kind) was open: the UNION of the bracket intervals.  Two
    // chunks are in flight on two streams, so the brackets of one stream overlap those of the other (their tile launches
    // alternate on the chip); summing bracket lengths would count that time twice.
    double total_ms(int k) {
        if (used < 2) return 0.0;
        std::vector<std::pair<float, float>> iv;
        for (size_t i = 0; i + 1 < used; i += 2) {
            if (k >= 0 && kind[i / 2] != k) continue;
            float a = 0, b = 0;
            if (hipEventElapsedTime(&a, ev[0], ev[i]) != hipSuccess || hipEventElapsedTime(&b, ev[0], ev[i + 1]) != hipSuccess) continue;
            iv.emplace_back(a, b);
        }
        std::sort(iv.begin(), iv.end());
        double t = 0, end = -1e30;
        for (auto& x : iv) {
            if (x.first > end) { t += x.second - x.first; end = x.second; }
            else if (x.second > end) { t += x.second - end; end = x.second; }
        }
        return t;
    }
    double span_ms(int k) {                       // sum of the bracket lengths of kind k (what a per-kernel profiler adds up)
        double t = 0;
        for (size_t i = 0; i + 1 < used; i += 2) {
            if (kind[i / 2] != k) continue;
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) t += ms;
        }
        return t;
    }
    size_t launches(int k) const {
        size_t n = 0;
        for (size_t i = 0; i + 1 < used; i += 2) n += kind[i / 2] == k;
        return n;
    }
};

// The Fiat-Shamir kernels' three shapes (kernels_range.h, FsShape): fs = 0 lane per proof, 1 lane pair, 2 wavefront per proof.
#define LAUNCH_FS(kernel, fs, cb, st, ...)                                                                          \
    do {                                                                                                             \
        if ((fs) == 2) hipLaunchKernelGGL(kernel<2>, dim3((unsigned)(cb)), dim3(64), 0, st, __VA_ARGS__);            \
        else if ((fs) == 1) hipLaunchKernelGGL(kernel<1>, dim3(nblk(2 * (cb), 64)), dim3(64), 0, st, __VA_ARGS__);   \
        else hipLaunchKernelGGL(kernel<0>, dim3(nblk((cb), 64)), dim3(64), 0, st, __VA_ARGS__);                      \
    } while (0)
// The fixed-base MSM with LPL lanes per list (32 / LPL proofs per wavefront).
static void launch_msm(hipStream_t st, const RangeArgs& A, const TableView& tv, int round, int lpl) {
    const unsigned B = (unsigned)A.B, S = (unsigned)(A.nsplit > 1 ? A.nsplit : 1);
    if (lpl == 8) hipLaunchKernelGGL((k_rp_msm<MSM_PLAIN, 8>), dim3((B + 3) / 4 * S), dim3(64), 0, st, A, tv, round);
    else if (lpl == 4) hipLaunchKernelGGL((k_rp_msm<MSM_PLAIN, 4>), dim3((B + 7) / 8 * S), dim3(64), 0, st, A, tv, round);
    else if (lpl == 2) hipLaunchKernelGGL((k_rp_msm<MSM_PLAIN, 2>), dim3((B + 15) / 16 * S), dim3(64), 0, st, A, tv, round);
    else if (lpl == 16) hipLaunchKernelGGL((k_rp_msm<MSM_PLAIN, 16>), dim3((B + 1) / 2 * S), dim3(64), 0, st, A, tv, round);
    else hipLaunchKernelGGL((k_rp_msm<MSM_PLAIN, 32>), dim3(B * S), dim3(64), 0, st, A, tv, round);
}
// The tail argument's MSM over the per-proof tables: 32 terms per list, LPL lanes per list.
static void launch_msm_tail(hipStream_t st, const RangeArgs& At, const TableView& tvt, int round, int lpl) {
    const unsigned B = (unsigned)At.B;
    if (lpl == 2) hipLaunchKernelGGL((k_rp_msm<MSM_TAIL, 2>), dim3((B + 15) / 16), dim3(64), 0, st, At, tvt, round);
    else if (lpl == 1) hipLaunchKernelGGL((k_rp_msm<MSM_TAIL, 1>), dim3((B + 31) / 32), dim3(64), 0, st, At, tvt, round);
    else if (lpl == 32) hipLaunchKernelGGL((k_rp_msm<MSM_TAIL, 32>), dim3(B), dim3(64), 0, st, At, tvt, round);
    else if (lpl == 8) hipLaunchKernelGGL((k_rp_msm<MSM_TAIL, 8>), dim3((B + 3) / 4), dim3(64), 0, st, At, tvt, round);
    else hipLaunchKernelGGL((k_rp_msm<MSM_TAIL, 4>), dim3((B + 7) / 8), dim3(64), 0, st, At, tvt, round);
}

// Scratch budget of the range prover / verifier: DAPOL_SCRATCH_GB if set; else 130 GB (two 73,728-proof chunks of the
// headline shape in flight) but never more than what the device has free beyond an 8 GB margin, counting the scratch
// this context already holds as available (it is re-used).
static size_t scratch_budget_bytes(const dapol_ctx* ctx = nullptr) {
    const double GiB = 1024.0 * 1024.0 * 1024.0;
    if (const char* e = knob("DAPOL_SCRATCH_GB")) {
        double gb = atof(e);
        if (gb < 0.25) gb = 0.25;
        return (size_t)(gb * GiB);
    }
    if (ctx && ctx->opt.scratch_gb > 0) return (size_t)((ctx->opt.scratch_gb < 0.25 ? 0.25 : ctx->opt.scratch_gb) * GiB);
    // BENCH: room for a chunk of two rounds of resident wavefronts (102 GB at 32 parties).  HOST: one round (51 GB).
    double want = (ctx && ctx->opt.profile == DAPOL_PROFILE_HOST ? 56.0 : 130.0) * GiB;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        double avail = (double)free_b + (ctx ? (double)ctx->scratch.bytes : 0.0) - 8.0 * GiB;
        if (avail < 0.25 * GiB) avail = 0.25 * GiB;
        if (avail < want) want = avail;
    }
    return (size_t)want;
}


// Blocks of 256 lanes of k_rp_fold (kernels_range.h): B * N lanes in vector mode; B * max(half, table entries to write) with tables.
static unsigned fold_blocks(const RangeArgs& A, size_t cb, int round) {
    if (!A.stab) return nblk(cb * (size_t)A.N, 256);
    const size_t half = (size_t)1 << (A.lgN - 1 - round), nt = (round + 1 <= STAB_ROUNDS) ? ((size_t)2 << (round + 1)) : 0;
    return nblk(cb * (half > nt ? half : nt), 256);
}

// Proves B aggregated proofs whose inputs are device resident.  d_out: [B][out_words] words.
// sub_k > 1: the B proofs are sub_k equal-sized sub-proofs of each of B / sub_k ROWS (RangeArgs::sub_k: the individual proofs of an
// entity under a policy, or equal parts of a split): d_stream / d_tape are indexed by row, sub-proof j draws from slot
// slot_base + j m (2n + 4) on and lands at d_out + row * out_stride + j * out_words.  d_vals / d_blind / d_Vc stay [B][m].
// pend != null: the call returns with its work QUEUED on ctx's stream(s) -- no host wait -- and the caller finishes it with
// pend->finish() (wait + the zero-challenge flag).  How the groups of one small call's plan run side by side on lanes of their own
// (dapol_ctx::aux; prove_policy_device).
struct PendingProve {
    dapol_ctx* ctx = nullptr;
    DevBuf<uint32_t> err;
    int pinned_slot = 0;             // which of the 16 words (several groups of one call may share a lane)
    uint32_t* h_err_p = nullptr;     // a page-locked word of the lane's context (dapol_ctx::h_pinned): the copy into it does not block the host
    bool armed = false;
    int32_t finish() {
        if (!armed) return DAPOL_OK;
        armed = false;
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (*h_err_p) return fail(DAPOL_ERR_INVALID_ARGUMENT, "prover drew a zero challenge (ProofError::MaliciousDealer)");
        return DAPOL_OK;
    }
    ~PendingProve() { if (armed) (void)hipStreamSynchronize(ctx->stream); }
};

// One chunk in flight owns one share of the context's scratch: the buffers of RangeArgs (A: everything else is the call's), the
// partial points of a split main MSM (two lists) and of a split materialisation, and the sweep's accumulators.
struct ProveLane {
    RangeArgs A;
    int32_t* split[3];
    int32_t* gsacc;
};
static ProveLane carve_lane(const ProvePlan& P, RangeArgs A, uint8_t* base) {
    ProveLane L{};
    const size_t chunk = P.chunk, N = (size_t)P.N, T = (size_t)P.tail_n;
    size_t o = 0;
    A.a = (sc*)(base + o); o += chunk * N * sizeof(sc);
    A.b = (sc*)(base + o); o += chunk * N * sizeof(sc);
    A.s1 = (sc*)(base + o); o += chunk * N * sizeof(sc);
    A.s2 = (sc*)(base + o); o += chunk * N * sizeof(sc);
    A.dig = (dig_t*)(base + o); o += align_up(chunk * P.dig_elems * sizeof(dig_t), 256);
    A.st = (ProofState*)(base + o); o += align_up(chunk * sizeof(ProofState), 256);
    A.PA = (int32_t*)(base + o); o += chunk * 160;
    A.P0 = (int32_t*)(base + o); o += chunk * 160;
    A.P1 = (int32_t*)(base + o); o += chunk * 160;
    A.tailT = (int32_t*)(base + o); o += chunk * 2 * T * TAIL_ROW_WORDS * 4;
    A.tail_a = (sc*)(base + o); o += chunk * T * sizeof(sc);
    A.tail_b = (sc*)(base + o); o += chunk * T * sizeof(sc);
    A.tail_s1 = (sc*)(base + o); o += chunk * T * sizeof(sc);
    A.tail_s2 = (sc*)(base + o); o += chunk * T * sizeof(sc);
    A.fs_part = (sc*)(base + o); o += chunk * FS_PARTS_MAX * 3 * sizeof(sc);
    A.stab = P.stab_bytes ? (sc*)(base + o) : nullptr; o += chunk * P.stab_bytes;
    L.gsacc = (int32_t*)(base + o); o += chunk * (P.acc_bytes + P.tail_rec_bytes);    // (the tail's window sums share it: ProvePlan::tail_gs)
    o = align_up(o, 256);
    // (the split buffers stay LAST: split_bytes only counts them when a split is in use)
    L.split[0] = (int32_t*)(base + o); o += chunk * (size_t)P.part_split() * 160;
    L.split[1] = (int32_t*)(base + o); o += chunk * (size_t)P.part_split() * 160;
    o = align_up(o, 256);
    L.split[2] = (int32_t*)(base + o);
    L.A = A;
    return L;
}

// The fixed-base MSM of one round of the main argument for the chunk A (round -1: the S commitment), split or not.
static void launch_main_msm(dapol_ctx* ctx, const ProvePlan& P, const ProveLane& L, const RangeArgs& A, hipStream_t st, int round, MsmTiming* tm) {
    const size_t cb = A.B;
    if (P.gs) {                                           // large calls: sweep the generators, a tile of rows per launch
        const int LW = P.gs_LW;
        const unsigned g_acc = nblk(cb * (size_t)LW, 64);
        // calls of a few thousand proofs: slices of each list side by side (lanes enough to fill the chip)
        const int ns = P.slices_for(cb), slice_rows = A.N / ns, tile = P.tile_for(cb, ns);
        const size_t side_words = (size_t)4 * FE_NL * cb * LW * ns;         // the two lists' accumulators, one after the other
        for (int side = 0; side < 2; side++)
            for (int q0 = 0; q0 < slice_rows; q0 += tile) {
                const int nq = slice_rows - q0 < tile ? slice_rows - q0 : tile;
                if (LW < A.nwin)
                    hipLaunchKernelGGL(k_rp_msm_gs_hi, dim3(g_acc, ns), dim3(64), 0, st, A, ctx->tv, round, side, q0, nq, q0 == 0 ? 1 : 0,
                                       L.gsacc + side * side_words, slice_rows, LW);
                else
                    hipLaunchKernelGGL(k_rp_msm_gs, dim3(g_acc, ns), dim3(64), 0, st, A, ctx->tv, round, side, q0, nq, q0 == 0 ? 1 : 0,
                                       L.gsacc + side * side_words, slice_rows);
            }
        if (ns > 1) hipLaunchKernelGGL(k_rp_gs_sum_slices, dim3(nblk(2 * cb * (size_t)LW, 64)), dim3(64), 0, st, A, L.gsacc, side_words, ns, LW);
        hipLaunchKernelGGL(k_rp_gs_combine, dim3(nblk(2 * cb, 64)), dim3(64), 0, st, A, L.gsacc, side_words, ns, LW);
        if (tm) tm->count(0, 2 * (size_t)((slice_rows + tile - 1) / tile));
    } else if (P.part_split() > 1) {                      // small calls: a proof's term range over several wavefronts, partials summed
        RangeArgs As = A;
        As.nsplit = P.part_split(); As.P0 = L.split[0]; As.P1 = L.split[1];
        // a few proofs: one point per four lanes (k_rp_msm_quad)
        if (P.quad_split) hipLaunchKernelGGL(k_rp_msm_quad, dim3((unsigned)(cb * (size_t)P.quad_split)), dim3(64), 0, st, As, ctx->tv, round);
        else launch_msm(st, As, ctx->tv, round, P.lpl);
        hipLaunchKernelGGL(k_rp_sum_splits, dim3((unsigned)(2 * cb)), dim3(64), 0, st, cb, As.nsplit, As.P0, As.P1, A.P0, A.P1);
    } else {
        launch_msm(st, A, ctx->tv, round, P.lpl);
        if (tm) tm->count(0, 1);
    }
}

// Materialises the 2T folded generators of the chunk A into its per-proof tail tables' input (A.tailT).
static int32_t launch_materialise(dapol_ctx* ctx, const ProvePlan& P, const ProveLane& L, const RangeArgs& A, hipStream_t st, MsmTiming* tm) {
    const size_t cb = A.B, T = (size_t)P.tail_n;
    const unsigned g_tail = (unsigned)(cb * (size_t)(P.tail_n / 32));
    if (P.gs_mat) {                                       // a class (one folded generator of every proof) per tile, MAT_GROUP classes per Horner launch
        const int LW = P.mat_LW(), cpl = P.mat_cpl(cb);
        const unsigned g_cls = nblk(cb * (size_t)LW, 64);
        const size_t slot_words = (size_t)4 * FE_NL * cb * LW;
        for (int side = 0; side < 2; side++)
            for (int c0 = 0; c0 < P.tail_n; c0 += MAT_GROUP) {
                const int nc = P.tail_n - c0 < MAT_GROUP ? P.tail_n - c0 : MAT_GROUP;
                for (int c = 0; c < nc; c += cpl) {               // cpl classes per launch (1 when one class's lanes fill the chip)
                    const int ny = nc - c < cpl ? nc - c : cpl;
                    hipLaunchKernelGGL(k_rp_mat_gs, dim3(g_cls, ny), dim3(64), 0, st, A, ctx->tv, side, c0 + c, 0, LW, L.gsacc + c * slot_words);
                    if (LW < A.nwin) hipLaunchKernelGGL(k_rp_mat_gs, dim3(g_cls, ny), dim3(64), 0, st, A, ctx->tv, side, c0 + c, 1, LW, L.gsacc + c * slot_words);
                }
                hipLaunchKernelGGL(k_rp_mat_gs_horner, dim3(nblk(cb * (size_t)nc, 64)), dim3(64), 0, st, A, side, c0, nc, LW, L.gsacc);
            }
        if (tm) tm->count(1, 2 * (size_t)((P.tail_n + cpl - 1) / cpl) * (LW < A.nwin ? 2 : 1));
    } else if (P.mat_split > 1) {
        RangeArgs Am = A;
        Am.nsplit = P.mat_split; Am.P0 = L.split[2];
        hipLaunchKernelGGL((k_rp_msm<MSM_MATERIALIZE, 32>), dim3(g_tail * (unsigned)P.mat_split), dim3(64), 0, st, Am, ctx->tv, -1); LAUNCH_CHECK();
        hipLaunchKernelGGL(k_rp_sum_mat, dim3(nblk(cb * 2 * T, 64)), dim3(64), 0, st, cb * 2 * T, P.mat_split, Am.P0, A.tailT);
    } else {
        hipLaunchKernelGGL((k_rp_msm<MSM_MATERIALIZE, 32>), dim3(g_tail), dim3(64), 0, st, A, ctx->tv, -1);
        if (tm) tm->count(1, 1);
    }
    LAUNCH_CHECK();
    return DAPOL_OK;
}

// Queues every kernel of one chunk on the stream st.  A: the lane's buffers (L.A) with the chunk's inputs, outputs and B filled in.
// Only a small call's A commitment leaves st (ProvePlan::side_A: forked to ctx->side[2] and joined again in here, under fg).
static int32_t queue_chunk(dapol_ctx* ctx, const ProvePlan& P, const ProveLane& L, RangeArgs A, hipStream_t st, ForkGuard& fg, uint32_t* d_err,
                           MsmTiming* tm) {
    const size_t cb = A.B;
    const int fs_shape = P.fs_shape, nf_rounds = P.nf_rounds();
    sc* const stab_buf = A.stab;
    if (!P.stab_main) A.stab = nullptr;
    const unsigned g_wave = (unsigned)cb, g_lane = nblk(cb, 64), g_dig = (unsigned)(cb * (size_t)(A.TP / 64));
    const unsigned g_gsdig = nblk(cb * (size_t)(2 * A.N), 64);               // generator-stationary producers: a thread per term
    hipLaunchKernelGGL(k_rp_nonce_key, dim3(g_lane), dim3(64), 0, st, A); LAUNCH_CHECK();
    if (P.gs) hipLaunchKernelGGL(k_rp_nonces_gs, dim3(g_gsdig), dim3(64), 0, st, A);
    else hipLaunchKernelGGL(k_rp_nonces, dim3(g_dig), dim3(64), 0, st, A);
    LAUNCH_CHECK();
    if (P.side_A) {
        HIPCHK(hipEventRecord(ctx->ev_fork, st));
        HIPCHK(hipStreamWaitEvent(ctx->side[2], ctx->ev_fork, 0));
        fg.forked(2);
        hipLaunchKernelGGL(k_rp_A, dim3(g_wave), dim3(64), 0, ctx->side[2], A, ctx->tv); LAUNCH_CHECK();
        HIPCHK(hipEventRecord(ctx->ev_join[2], ctx->side[2]));
        FAULT_AFTER_FORK("prove_A");
    } else if (P.a_lane(cb)) {
        hipLaunchKernelGGL(k_rp_A_lane, dim3(g_lane), dim3(64), 0, st, A, ctx->tv); LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL(k_rp_A, dim3(g_wave), dim3(64), 0, st, A, ctx->tv); LAUNCH_CHECK();
    }
    if (tm) HIPCHK(tm->mark(st));
    launch_main_msm(ctx, P, L, A, st, -1, tm); LAUNCH_CHECK();
    if (tm) HIPCHK(tm->mark(st));
    if (P.side_A) { HIPCHK(hipStreamWaitEvent(st, ctx->ev_join[2], 0)); fg.joined(2); }
    LAUNCH_FS(k_rp_finish1, fs_shape, cb, st, A, ctx->tv); LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rp_poly, dim3(g_wave * (unsigned)A.fs_parts), dim3(64), 0, st, A); LAUNCH_CHECK();
    LAUNCH_FS(k_rp_finish2, fs_shape, cb, st, A, ctx->tv); LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rp_lr, dim3(g_wave * (unsigned)A.fs_parts), dim3(64), 0, st, A); LAUNCH_CHECK();
    if (fs_shape == 2) hipLaunchKernelGGL(k_rp_finish3<2>, dim3(g_wave), dim3(64), 0, st, A);
    else hipLaunchKernelGGL(k_rp_finish3<0>, dim3(g_lane), dim3(64), 0, st, A);
    LAUNCH_CHECK();
    for (int k = 0; k < nf_rounds; k++) {
        if (P.gs) hipLaunchKernelGGL(k_rp_round_prep_gs, dim3(g_gsdig), dim3(64), 0, st, A, k);
        else hipLaunchKernelGGL(k_rp_round_prep, dim3(g_dig), dim3(64), 0, st, A, k);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(k_rp_round_ip, dim3(g_wave), dim3(64), 0, st, A, k); LAUNCH_CHECK();
        if (tm) HIPCHK(tm->mark(st));
        launch_main_msm(ctx, P, L, A, st, k, tm); LAUNCH_CHECK();
        if (tm) HIPCHK(tm->mark(st));
        LAUNCH_FS(k_rp_round_finish, fs_shape, cb, st, A, ctx->tv, k); LAUNCH_CHECK();
        hipLaunchKernelGGL(k_rp_fold, dim3(fold_blocks(A, cb, k)), dim3(256), 0, st, A, k);
        LAUNCH_CHECK();
    }
    if (nf_rounds == A.lgN) {                             // no tail: the main argument went all the way
        hipLaunchKernelGGL(k_rp_final, dim3(g_lane), dim3(64), 0, st, A, d_err); LAUNCH_CHECK();
        return DAPOL_OK;
    }
    if (P.prep_share) hipLaunchKernelGGL(k_rp_mat_prep_gs_shared, dim3(nblk(cb * (size_t)(2 * (A.N / A.tail_n)), 64)), dim3(64), 0, st, A);
    else if (P.gs_mat) hipLaunchKernelGGL(k_rp_mat_prep_gs, dim3(g_gsdig), dim3(64), 0, st, A);
    else hipLaunchKernelGGL(k_rp_mat_prep, dim3(g_dig), dim3(64), 0, st, A);
    LAUNCH_CHECK();
    if (tm) HIPCHK(tm->mark(st, 1));
    { int32_t rc = launch_materialise(ctx, P, L, A, st, tm); if (rc) return rc; }
    if (tm) HIPCHK(tm->mark(st, 1));
    const unsigned g_tail = (unsigned)(cb * (size_t)(P.tail_n / 32));
    {
        RangeArgs Ai = A;
        Ai.stab = P.stab_tail ? stab_buf : nullptr;           // (k_rp_tail_table also resets the tables for the tail argument)
        if (P.tail_rpl == 4) hipLaunchKernelGGL(k_rp_tail_table4, dim3(nblk(cb * (size_t)(2 * P.tail_n / 4), 64)), dim3(64), 0, st, Ai);
        else hipLaunchKernelGGL(k_rp_tail_table, dim3(g_tail), dim3(64), 0, st, Ai);
        LAUNCH_CHECK();
    }
    // The remaining rounds: the same never-fold kernels on the length-T argument over the proof's own table.
    RangeArgs At = A;
    At.N = P.tail_n; At.lgN = P.tail_lgn; At.TP = 2 * P.tail_n; At.wbits = TAIL_WBITS; At.nwin = TAIL_NWIN; At.nsplit = 0;
    At.a = A.tail_a; At.b = A.tail_b; At.s1 = A.tail_s1; At.s2 = A.tail_s2;
    At.stab = P.stab_tail ? stab_buf : nullptr;
    At.out_round0 = nf_rounds;
    const TableView tvt{A.tailT, 1, TAIL_WBITS, 0, 0};
    for (int k = 0; k < P.tail_lgn; k++) {
        hipLaunchKernelGGL(k_rp_round_prep, dim3(g_tail), dim3(64), 0, st, At, k); LAUNCH_CHECK();
        hipLaunchKernelGGL(k_rp_round_ip, dim3(g_wave), dim3(64), 0, st, At, k); LAUNCH_CHECK();
        if (P.tail_gs) {                                      // a lane per (proof, list, window), then Horner per list
            hipLaunchKernelGGL(k_rp_tail_gs, dim3(nblk(2 * cb, TAIL_GS_LISTS)), dim3(TAIL_GS_BLOCK), 0, st, At, tvt, k, L.gsacc); LAUNCH_CHECK();
            hipLaunchKernelGGL(k_rp_tail_combine, dim3(nblk(2 * cb, 64)), dim3(64), 0, st, At, L.gsacc);
        } else launch_msm_tail(st, At, tvt, k, P.tail_lpl);
        LAUNCH_CHECK();
        LAUNCH_FS(k_rp_round_finish, fs_shape, cb, st, At, ctx->tv, k); LAUNCH_CHECK();
        hipLaunchKernelGGL(k_rp_fold, dim3(fold_blocks(At, cb, k)), dim3(256), 0, st, At, k);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_rp_final, dim3(g_lane), dim3(64), 0, st, At, d_err); LAUNCH_CHECK();
    return DAPOL_OK;
}

static int32_t range_prove_device(dapol_ctx* ctx, int n, int m, size_t B, const uint64_t* d_vals, const uint32_t* d_blind,
                                  const uint32_t* d_Vc, const uint32_t* d_seed, const uint64_t* d_stream, uint64_t slot_base,
                                  const uint32_t* d_tape, uint32_t* d_out, MsmTiming* tm, size_t tape_stride = 0, uint32_t sub_k = 1,
                                  size_t out_stride = 0, PendingProve* pend = nullptr, uint32_t seed_stride = 0 /* words; 0: one seed */,
                                  const uint64_t* d_slot_of = nullptr /* [B] first slot of every proof (RangeArgs::slot_of); null: slot_base */) {
    ProveShape s{};
    s.n = n; s.m = m; s.B = B;
    s.tail_length = ctx->opt.tail_length; s.small_call_max = ctx->opt.small_call_max; s.generator_stationary = ctx->opt.generator_stationary;
    s.streams = ctx->opt.streams; s.gs_tile_rows = ctx->opt.gs_tile_rows; s.gs_slices = ctx->opt.gs_slices; s.chunk_proofs = ctx->opt.chunk_proofs;
    s.wbits = ctx->tv.wbits; s.nwin = ctx->tv.nwin_c(); s.hi_split = ctx->tv.hi_split;
    s.n_cu = ctx->n_cu; s.resident_waves = ctx->resident_waves();
    s.budget_bytes = scratch_budget_bytes(ctx);
    s.timed = tm != nullptr;
    ProvePlan P = plan_range_prove(s);
    // The budget is a wish, the device's free memory the fact: on an allocation failure fall back to one chunk in flight,
    // then to smaller chunks, before giving up.
    for (bool lowered = false;; lowered = true) {
        hipError_t e = ctx->scratch.ensure(P.lane_bytes() * P.nlanes);
        if (e == hipSuccess) {
            if (lowered) P.finalise(s, P.chunk, P.nlanes);    // (the lanes per list follow from the chunk that fitted)
            break;
        }
        (void)hipGetLastError();
        if (e != hipErrorOutOfMemory || (P.nlanes == 1 && P.chunk <= 64)) return fail_hip(e, "scratch allocation", __FILE__, __LINE__);
        if (P.nlanes > 1) P.nlanes--;
        else P.chunk = (P.chunk + 1) / 2;
    }
    const size_t chunk = P.chunk, slots = (size_t)m * (2 * (size_t)n + 4);
    const int nlanes = P.nlanes;
    RangeArgs A{};                                           // what every chunk of the call shares
    A.n = n; A.m = m; A.N = P.N; A.lgN = P.lgN; A.TP = P.TP;
    A.out_words = 72 + 16 * A.lgN;
    A.seed = d_seed; A.seed_stride = seed_stride; A.slot_base = slot_base; A.slot_of = d_slot_of;
    A.wbits = s.wbits; A.nwin = s.nwin;
    A.prep = (P.prep_recode ? PREP_RECODE : 0) | (P.prep_share ? PREP_SHARE : 0);
    A.tail_n = P.tail_n; A.use_hi = P.use_hi ? 1 : 0; A.fs_parts = P.fs_parts; A.mat_round = P.nf_rounds();
    A.stream_id = d_stream;                                  // (row-indexed from the call's first proof: RangeArgs::p0)
    A.tape_stride = (uint32_t)(tape_stride ? tape_stride : slots);
    A.tape = d_tape;
    A.sub_k = sub_k ? sub_k : 1; A.sub_slots = (uint32_t)slots;
    A.out = d_out; A.out_stride = out_stride ? out_stride : (size_t)A.out_words;
    ProveLane lanes[4];
    hipStream_t lane_stream[4] = {ctx->stream, ctx->side[0], ctx->side[1], ctx->side[2]};
    for (int ln = 0; ln < nlanes; ln++) lanes[ln] = carve_lane(P, A, (uint8_t*)ctx->scratch.p + P.lane_bytes() * ln);
    DevBuf<uint32_t> err_own;
    DevBuf<uint32_t>& err = pend ? pend->err : err_own;
    HIPCHK(err.alloc(1));
    HIPCHK(hipMemsetAsync(err.p, 0, 4, ctx->stream));
    ForkGuard fg(ctx);                                       // an early return below waits for the chunks in flight on the side streams
    if (nlanes > 1) {                                        // the side streams start after everything already queued on the first
        HIPCHK(hipEventRecord(ctx->ev_fork, ctx->stream));
        for (int ln = 1; ln < nlanes; ln++) { HIPCHK(hipStreamWaitEvent(lane_stream[ln], ctx->ev_fork, 0)); fg.forked(ln - 1); }
    }
    size_t chunk_no = 0;
    for (size_t first = 0; first < B; first += chunk, chunk_no++) {
        const int ln = (int)(chunk_no % (size_t)nlanes);
        if (chunk_no == 2) FAULT_AFTER_FORK("prove_lanes");     // (chunk 1 is in flight on a side stream)
        RangeArgs Ac = lanes[ln].A;                             // this chunk: the lane's buffers, its slice of the inputs
        Ac.B = B - first < chunk ? B - first : chunk;
        Ac.vals = d_vals + first * m;
        Ac.blind = d_blind + first * m * 8;
        Ac.Vc = d_Vc + first * m * 8;
        Ac.p0 = first;
        int32_t rc = queue_chunk(ctx, P, lanes[ln], Ac, lane_stream[ln], fg, err.p, tm);
        if (rc) return rc;
    }
    for (int ln = 1; ln < nlanes; ln++) {                    // join: the first stream continues after the others have drained
        HIPCHK(hipEventRecord(ctx->ev_join[ln - 1], lane_stream[ln]));
        HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_join[ln - 1], 0));
        fg.joined(ln - 1);
    }
    if (pend) {                                              // queued, not awaited: the caller finishes (PendingProve::finish)
        pend->ctx = ctx;
        pend->h_err_p = ctx->h_pinned + pend->pinned_slot;
        HIPCHK(hipMemcpyAsync(pend->h_err_p, err.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        pend->armed = true;
        return DAPOL_OK;
    }
    uint32_t h_err = 0;
    HIPCHK(hipMemcpyAsync(&h_err, err.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (h_err) return fail(DAPOL_ERR_INVALID_ARGUMENT, "prover drew a zero challenge (ProofError::MaliciousDealer)");
    return DAPOL_OK;
}

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    hipError_t init() { hipError_t e = hipEventCreate(&a); return e != hipSuccess ? e : hipEventCreate(&b); }
};

int32_t dapol_range_prove_batch(dapol_ctx* ctx, int32_t n_bits, int32_t m, size_t b, const uint64_t* v, const uint8_t* r32,
                                const uint8_t nonce_seed32[32], const uint64_t* stream_id, uint64_t slot_base, const uint8_t* tape,
                                uint8_t* proofs_out) {
    if (!ctx || (b && (!v || !r32 || !proofs_out))) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (!tape && (!nonce_seed32 || (b && !stream_id))) return fail(DAPOL_ERR_INVALID_ARGUMENT, "seed mode needs nonce_seed32 and stream_id");
    size_t ps = dapol_range_proof_size(n_bits, m);
    if (ps == 0) return fail(DAPOL_ERR_INVALID_ARGUMENT, "n_bits must be 8/16/32/64 and m a power of two");
    if (m > ctx->max_parties) return fail(DAPOL_ERR_INVALID_ARGUMENT, "m exceeds the context's max_parties (InvalidGeneratorsLength)");
    if (b == 0) return DAPOL_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t tot = b * (size_t)m, slots = (size_t)m * (2 * (size_t)n_bits + 4);
    DevBuf<uint64_t> dv, dstream;
    DevBuf<uint32_t> dr, dVc, dseed, dtape, dout;
    HIPCHK(dv.alloc(tot)); HIPCHK(dr.alloc(tot * 8)); HIPCHK(dVc.alloc(tot * 8)); HIPCHK(dseed.alloc(8));
    HIPCHK(dout.alloc(b * ps / 4));
    HIPCHK(hipMemcpyAsync(dv.p, v, tot * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dr.p, r32, tot * 32, hipMemcpyHostToDevice, st));
    if (tape) {
        HIPCHK(dtape.alloc(b * slots * 16));
        HIPCHK(hipMemcpyAsync(dtape.p, tape, b * slots * 64, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(dseed.p, 0, 32, st));
    } else {
        HIPCHK(dstream.alloc(b));
        HIPCHK(hipMemcpyAsync(dstream.p, stream_id, b * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dseed.p, nonce_seed32, 32, hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(k_rp_commit_V, dim3(nblk(tot, 256)), dim3(256), 0, st, ctx->tv, tot, dv.p, dr.p, dVc.p);
    LAUNCH_CHECK();
    EventPair ev;
    HIPCHK(ev.init());
    HIPCHK(hipEventRecord(ev.a, st));
    int32_t rc = range_prove_device(ctx, n_bits, m, b, dv.p, dr.p, dVc.p, dseed.p, dstream.p, slot_base, dtape.p, dout.p, nullptr);
    if (rc) return rc;
    HIPCHK(hipEventRecord(ev.b, st));
    HIPCHK(hipMemcpy(proofs_out, dout.p, b * ps, hipMemcpyDeviceToHost));
    { float ms = 0; if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) g_last_range_prove_ms.store((double)ms, std::memory_order_relaxed); }
    return DAPOL_OK;
}

// What one call of the batched range verifier chooses, as pure host arithmetic over (n, m, b), the options, the table geometry and the
// scratch budget: one random linear combination or proof by proof, the shape of the generator MSM, chunk sizes, the per-chunk point
// counts, bucket method or per-point tables, the transcript shapes, the forks, and the carve-up of the scratch.  No HIP call and no
// dapol_ctx: the launchers (host_verify.inc) fill a VerifyShape from their context, and tests/cpp/verify_plan_host.cpp replays recorded
// shapes against tests/golden/verify_plan.json on the CPU.  The includer provides knob(), prove_plan.inc (msm_lanes_per_list,
// small_split_cap, quad_max_waves) and the layout constants of the kernel headers (sc, dig_t, VerifyState, rv_tab_entries*, PT_*, RVP_*).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

enum { RLC_MIN_DEFAULT = 112 };       // measured (profiles/r02_midsize_ab.txt): 64 proofs 2.0 ms one by one against 2.2 ms batched, 128 proofs 2.8 against 2.7
static bool verify_wave_transcript(int m) {
    if (const char* e = knob("DAPOL_VERIFY_WAVE_TRANSCRIPT")) return atoi(e) != 0;
    return m >= 256;
}
static size_t verify_rlc_min(int opt_verify_batch_min) {      // fewest proofs that are checked as ONE random linear combination
    size_t rlc_min = opt_verify_batch_min >= 2 ? (size_t)opt_verify_batch_min : RLC_MIN_DEFAULT;
    if (const char* e = knob("DAPOL_VERIFY_RLC_MIN")) { long v = atol(e); if (v >= 2) rlc_min = (size_t)v; }
    return rlc_min;
}
static size_t plan_align(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct VerifyShape {
    int n, m;
    size_t b;
    int opt_verify_batch_min;         // dapol_options::verify_batch_min (0: the library's own choice)
    int wbits, nwin, hi_split;        // TableView: window width, windows per canonical scalar, window steps with high-half rows (0: none)
    int n_cu;
    size_t budget_bytes;              // scratch_budget_bytes(ctx)
    int va_K;                         // column blocks of an attached VArrival (0: the commitments are already on the device)
};

// What both paths start from: generators a side, log2, digit-row length, and the split of the power tables' index (lgN = hb + lb).
struct VerifyDims { int N, lgN, TP, lb, hb; };
static VerifyDims verify_dims(int n, int m) {
    VerifyDims D{};
    D.N = n * m;
    while ((1 << D.lgN) < D.N) D.lgN++;
    D.TP = 2 * D.N < 64 ? 64 : 2 * D.N;
    D.lb = D.lgN / 2; D.hb = D.lgN - D.lb;
    return D;
}

// ---------------------------------------------------------------------------- proof by proof (range_verify_device)
struct VerifyPlan {
    int N, lgN, TP, lb, hb, tab_stride;
    bool small_call, use_hi;
    int lpl, nsplit;                  // lanes per list and wavefronts per proof of the generator MSM (nsplit: after the quad factor)
    bool quad;                        // k_rp_msm_quad
    int var_waves;                    // k_rv_varpoints_quad: wavefronts per proof
    size_t per_proof, chunk;
    bool tree_sum;                    // the splits' partials summed by a wavefront (k_rp_sum_splits)
    bool wave_transcript;             // k_rv_absorb_V absorbs the commitments
    bool wave_replay;                 // k_rv_transcript<1> (a wavefront per proof) or <0> (a lane)
    bool side_var;                    // the proof's own points on a side stream under the generator MSM
    bool quad_var_ok;
    size_t quad_var_max;
    // (many-party proofs, or more than a few, keep a point per lane)
    bool quad_var(size_t cb) const { return quad_var_ok && (size_t)var_waves * cb <= quad_var_max; }
};

static VerifyPlan plan_range_verify(const VerifyShape& s) {
    VerifyPlan P{};
    const VerifyDims D = verify_dims(s.n, s.m);
    P.N = D.N; P.lgN = D.lgN; P.TP = D.TP; P.lb = D.lb; P.hb = D.hb;
    const size_t b = s.b;
    const bool no_quad = knob("DAPOL_NO_QUAD") != nullptr;
    // A few proofs (someone checking their own): one proof per wavefront, the term range split finely and, with the tables'
    // high-half rows, half the window steps -- as the prover's small calls (host_range.inc).
    P.small_call = b <= 128 && P.N >= 256 && !knob("DAPOL_NO_SPLIT");
    P.use_hi = P.small_call && s.hi_split && !knob("DAPOL_NO_SMALL_HI");
    P.lpl = P.small_call ? 32 : msm_lanes_per_list(P.N);
    // enough wavefronts to fill the chip even for a few large proofs: split each proof's term range
    {
        size_t waves = (b + (32 / P.lpl) - 1) / (32 / P.lpl);
        int niter_all = (P.N + P.lpl - 1) / P.lpl, ns = 1;
        if (P.small_call) { const int cap = small_split_cap(P.use_hi); while (waves * ns < 4096 && niter_all / (ns * 2) >= (P.use_hi ? 2 : 4) && ns < cap) ns *= 2; }
        else { while (waves * ns < 4096 && niter_all / (ns * 2) >= 64 && ns < 256) ns *= 2; }
        P.nsplit = ns;
    }
    // ... and one point per four lanes (k_rp_msm_quad) when that many wavefronts are still few
    // (1.5x the work per point: it pays up to about 16 proofs, profiles/r02_midsize_ab.txt)
    P.quad = P.use_hi && P.nsplit > 1 && (size_t)P.nsplit * 4 * b <= quad_max_waves(4096) && P.N % (8 * P.nsplit * 4) == 0 && !no_quad;
    if (P.quad) P.nsplit *= 4;
    P.tab_stride = rv_tab_entries(P.lgN, s.m);
    P.var_waves = (4 + 2 * P.lgN + s.m + 15) / 16;
    P.per_proof = (size_t)s.nwin * P.TP * sizeof(dig_t) + plan_align(sizeof(VerifyState), 16) + (3 + 2 * (size_t)P.nsplit + (size_t)P.var_waves) * 160 + 1 +
                  (size_t)P.tab_stride * sizeof(sc);
    P.chunk = s.budget_bytes / P.per_proof;
    if (P.chunk < 1) P.chunk = 1;
    if (P.chunk > b) P.chunk = b;
    if (P.chunk > 60000) P.chunk = 60000;
    P.tree_sum = P.small_call && P.nsplit > 1;
    P.wave_transcript = verify_wave_transcript(s.m);
    P.wave_replay = P.small_call && !knob("DAPOL_VERIFY_LANE_TRANSCRIPT");
    // a small call's two point sums are independent and neither fills the chip: the proof's own points (k_rv_varpoints: needs the
    // challenges, the weights and the z-power table) run on a side stream under the generator MSM
    P.side_var = P.small_call && !knob("DAPOL_VERIFY_ONE_STREAM");
    P.quad_var_ok = P.side_var && P.var_waves <= 16 && !no_quad;
    P.quad_var_max = quad_max_waves(64);
    return P;
}

// ---------------------------------------------------------------------------- one random linear combination per chunk (range_verify_rlc_device)
struct RlcChunk {
    size_t cb;
    int G;                            // proof groups of the generator-scalar accumulation
    size_t npts, Np;                  // cb * K own points, as two lists of Np
    int TP2, ns2;                     // digit-row length and wavefront splits of the Straus point MSM
    bool pippenger;                   // the own points by the bucket method (else per-point tables + Straus)
    bool lazy;                        // lazy generator scalars (k_rvb_gh_lazy)
    bool wave_replay;                 // k_rv_transcript<1> or <0>
    bool fork;                        // the bucket method follows its decode on the side stream
    // the carve-up of the scratch (byte offsets) and its size
    size_t o_dig, o_vs, o_p0, o_p1, o_part, o_gpart, o_bsum, o_pt, o_dig2, o_q0, o_q1, o_flag, o_tabs, o_dga, o_dgb, o_t29, o_rzg, need;
    // the bucket method's buffers, carved out of the per-point table region at o_pt (1,152 bytes per point there, 260 here)
    size_t b_pN, b_pdig, b_psorted, b_phist, b_poffs, b_pcursor, b_pbsum, b_hsz, b_end, b_region;
    bool b_fits;
};

struct RlcPlan {
    bool use_rlc;                     // false: the call goes proof by proof (range_verify_device)
    size_t rlc_min;
    bool pipelined;                   // the transcript replay runs in phases behind the arriving commitment blocks
    int N, lgN, TP, lb, hb, tab_stride, nwin;
    bool quad_gen, gen_sweep;         // the ONE generator MSM: k_rp_msm_quad / window sweeps / Straus (neither)
    int gen_ns, nsplit, lpl;
    bool use_hi;
    int K;                            // own points per proof
    size_t per_proof, fixed, chunk;
    int nch;
    size_t pip_min;
    bool fork_points, wave_transcript, lazy, wave_replay_ok;
    RlcChunk chunk_plan(size_t cb) const;
};

static RlcPlan plan_range_verify_rlc(const VerifyShape& s) {
    RlcPlan P{};
    // A handful of proofs are checked one by one: the per-proof path's small-call shapes (a wavefront or a quad of lanes per unit of
    // work) finish sooner than the batched check's longer chain of launches (DAPOL_VERIFY_RLC_MIN: fewest proofs that are batched).
    P.rlc_min = verify_rlc_min(s.opt_verify_batch_min);
    P.use_rlc = !(s.b < P.rlc_min || knob("DAPOL_VERIFY_NO_RLC"));
    if (!P.use_rlc) return P;
    const VerifyDims D = verify_dims(s.n, s.m);
    P.N = D.N; P.lgN = D.lgN; P.TP = D.TP; P.lb = D.lb; P.hb = D.hb; P.nwin = s.nwin;
    P.lpl = msm_lanes_per_list(P.N);
    {   // the ONE generator MSM of a chunk: split its term range over enough wavefronts to fill the chip
        int niter_all = (P.N + P.lpl - 1) / P.lpl, ns = 1;
        while (ns < 1024 && niter_all / (ns * 2) >= 8) ns *= 2;
        P.nsplit = ns;
    }
    const bool no_quad = knob("DAPOL_NO_QUAD") != nullptr;
    // It is a lone MSM whatever the batch: with the tables' high-half rows it takes the small-call shape of the prover's -- one point per
    // four lanes, a term per group (k_rp_msm_quad: 0.72 -> 0.15 ms for 64-bit, 32-party proofs); DAPOL_NO_QUAD=1 keeps the lane kernel.
    P.quad_gen = s.hi_split && P.N >= 256 && P.N % 8 == 0 && P.N / 8 <= 1024 && !no_quad && !knob("DAPOL_NO_SMALL_HI");
    if (P.quad_gen) { P.nsplit = P.N / 8; P.use_hi = true; P.lpl = 32; }
    // Large proofs without high-half rows (the 1,024-party context): the generator MSM as window sweeps without doublings
    // (k_rvb_gen_sweep / k_rvb_gen_windows, kernels_verify.h).  DAPOL_VERIFY_GEN_STRAUS=1 keeps the Straus kernel.
    P.gen_sweep = !P.quad_gen && P.N >= 4096 && !knob("DAPOL_VERIFY_GEN_STRAUS");
    P.gen_ns = 1;
    if (P.gen_sweep) {
        while ((size_t)s.nwin * (size_t)P.gen_ns * 2 <= (size_t)s.n_cu * 8 && (2 * P.N) / (P.gen_ns * 2 * 64) >= 8) P.gen_ns *= 2;   // >= 2 wavefronts per SIMD, >= 8 terms per lane
        P.nsplit = s.nwin;                                     // k_rvb_finish adds nwin window points (P0) + identities (P1)
    }
    P.K = 4 + 2 * P.lgN + s.m;
    P.tab_stride = rv_tab_entries_rlc(P.lgN, s.m);
    P.per_proof = plan_align(sizeof(VerifyState), 16) + 2 * sizeof(sc) + (size_t)P.tab_stride * sizeof(sc) +
                  (size_t)(3 * (1 << P.hb) + 3 * (1 << P.lb)) * 48 +
                  (size_t)P.K * ((size_t)PT_ROW_WORDS * 4 + (size_t)PT_NWIN * sizeof(dig_t) * 2) + 64;
    P.fixed = (size_t)s.nwin * P.TP * sizeof(dig_t) + 64 * (size_t)P.TP * sizeof(sc) + 4 * 160 * 20000 + (1 << 20);
    P.chunk = s.budget_bytes > P.fixed ? (s.budget_bytes - P.fixed) / P.per_proof : 1;
    if (P.chunk < 2) P.chunk = 2;
    if (P.chunk > s.b) P.chunk = s.b;
    if (P.chunk > 262144) P.chunk = 262144;
    P.nch = P.TP >> 6;
    P.wave_transcript = verify_wave_transcript(s.m);
    // (no pipelining otherwise: every block lands before anything reads it)
    P.pipelined = s.va_K && !(P.chunk < s.b || !P.wave_transcript || s.va_K < 2 || s.m % s.va_K);
    // the proofs' own points: bucket method for large batches, per-point tables + Straus otherwise
    P.pip_min = 32768;                                         // DAPOL_VERIFY_PIPPENGER_MIN=<points> moves the switch (tests), 0 disables
    if (const char* e = knob("DAPOL_VERIFY_PIPPENGER_MIN")) { long v = atol(e); P.pip_min = v <= 0 ? (size_t)-1 : (size_t)std::max<long>(v, 12288); }
    P.fork_points = !knob("DAPOL_VERIFY_ONE_STREAM");
    // lazy generator scalars: limb copies of the product tables (needs the one-side-per-wavefront mapping, N >= 64)
    P.lazy = P.nch > 1 && !knob("DAPOL_VERIFY_GH_EAGER");
    P.wave_replay_ok = !knob("DAPOL_VERIFY_LANE_TRANSCRIPT");
    return P;
}

RlcChunk RlcPlan::chunk_plan(size_t cb) const {
    RlcChunk C{};
    C.cb = cb;
    // groups: enough blocks to fill the chip, at most one group per proof
    C.G = (int)std::min<size_t>(cb / 2 + 1, std::max<size_t>(1, (size_t)16384 / (size_t)nch));
    if (C.G > 64) C.G = 64;
    C.npts = cb * (size_t)K;
    C.Np = (C.npts + 1) / 2;
    const size_t niter2 = (C.Np + 31) / 32;
    C.TP2 = (int)(64 * niter2);
    C.ns2 = (int)std::min<size_t>(16384, std::max<size_t>(1, niter2 / 2));      // two points per lane: the 252 shared doublings are the chain
    C.pippenger = C.npts >= pip_min;
    C.lazy = lazy;
    // up to a few thousand proofs the replay is a lane's latency (1.0 ms), so a wavefront replays each proof (0.5 ms)
    C.wave_replay = cb <= 4096 && wave_replay_ok;
    C.fork = C.pippenger && fork_points;
    auto take = [&](size_t bytes) { size_t o = C.need; C.need += plan_align(bytes, 256); return o; };
    C.o_dig = take((size_t)nwin * TP * sizeof(dig_t)); C.o_vs = take(cb * sizeof(VerifyState));
    C.o_p0 = take((size_t)nsplit * 160); C.o_p1 = take((size_t)nsplit * 160); C.o_part = take((size_t)C.G * TP * sizeof(sc));
    C.o_gpart = take(gen_sweep ? (size_t)nwin * gen_ns * 160 : 16);
    C.o_bsum = take(cb * 2 * sizeof(sc)); C.o_pt = take(2 * C.Np * (size_t)PT_ROW_WORDS * 4);
    C.o_dig2 = take((size_t)PT_NWIN * C.TP2 * sizeof(dig_t)); C.o_q0 = take((size_t)C.ns2 * 160); C.o_q1 = take((size_t)C.ns2 * 160);
    C.o_flag = take(16); C.o_tabs = take(cb * (size_t)tab_stride * sizeof(sc));
    C.o_dga = take(((cb + 30) / 31 + 1) * 32); C.o_dgb = take(((cb + 30) / 31 / 31 + 2) * 32);
    const size_t per29 = (size_t)(3 * (1 << hb) + 3 * (1 << lb)) * 12 * sizeof(uint32_t);
    C.o_t29 = take(lazy ? cb * per29 : 16); C.o_rzg = take((size_t)C.G * sizeof(sc));
    if (C.pippenger) {
        size_t q = 0;
        C.b_pN = q; q += plan_align(C.npts * 128, 256);
        C.b_pdig = q; q += plan_align((size_t)RVP_NW * C.npts * 2, 256);
        C.b_psorted = q; q += plan_align((size_t)RVP_NW * C.npts * 4, 256);
        C.b_hsz = plan_align((size_t)RVP_NW * (RVP_NB + 1) * 4, 256);
        C.b_phist = q; q += C.b_hsz;
        C.b_poffs = q; q += C.b_hsz;
        C.b_pcursor = q; q += C.b_hsz;
        C.b_pbsum = q; q += (size_t)RVP_NW * RVP_NB * 160;
        C.b_end = q;
        C.b_region = 2 * C.Np * (size_t)PT_ROW_WORDS * 4;
        C.b_fits = C.b_end <= C.b_region;
    }
    return C;
}

// dapol_range_verify_batch: many-party batches (tens of MB of commitments) send their commitments in four column blocks.
static bool verify_pipe_arrival(int m, size_t b) {
    return verify_wave_transcript(m) && m % 4 == 0 && b * (size_t)m * 32 >= ((size_t)8 << 20) && !knob("DAPOL_VERIFY_NO_PIPELINE");
}
// verify_policy_device: a SMALL call with several groups runs the groups' per-proof checks side by side on lanes of their own.
static bool verify_groups_on_lanes(size_t n_groups, size_t b, size_t sum_proofs, size_t max_k, int opt_verify_batch_min) {
    return n_groups >= 2 && n_groups <= 16 && b * sum_proofs <= 64 && b * max_k < verify_rlc_min(opt_verify_batch_min) && !knob("DAPOL_NO_LANES") &&
           !knob("DAPOL_VERIFY_NO_RLC");
}
// verify_upload_and_paths: the Merkle re-merge of few proofs takes a wavefront per path (latency; many: a lane per path, 3x less work per
// path), and of a call of few proofs a side stream under the range verification.
static bool verify_paths_few(size_t b) { return b <= 16384 && !knob("DAPOL_PATHS_LANE"); }
static bool verify_paths_side(size_t b) { return verify_paths_few(b) && b <= 64 && !knob("DAPOL_VERIFY_ONE_STREAM"); }

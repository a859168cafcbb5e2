// What one call of the batched range prover chooses, as pure host arithmetic over (n, m, B), the options, the table geometry and the
// scratch budget: tail length, small-call / generator-stationary / proof-stationary regime, Fiat-Shamir shape, chunk size and chunks
// in flight, lanes per list, the order of the tail rounds, the MSM / materialisation / quad splits, slices and tile rows.  No HIP call and no dapol_ctx: the launcher
// (host_range.inc: range_prove_device) fills a ProveShape from its context, and tests/cpp/prove_plan_host.cpp replays recorded
// shapes against tests/golden/prove_plan.json on the CPU.  The includer provides knob() and the layout constants of the kernel
// headers (sc, dig_t, ProofState, FE_NL, TAIL_*, STAB_*, MAT_GROUP, GS_*).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>

enum { FS_PARTS_MAX = 8 };        // most wavefronts per proof of k_rp_poly / k_rp_lr in small calls
enum { TAIL_RPL_DEFAULT = 4 };    // the plan's own choice of ProvePlan::tail_rpl for full chunks (1 or 4)
enum { TAIL_GS_DEFAULT = 1 };     // the plan's own choice of ProvePlan::tail_gs for full chunks (0: only DAPOL_TAIL_ORDER=gs turns it on)
#ifndef DAPOL_PREP_V2_PARTS
#define DAPOL_PREP_V2_PARTS 3     // what DAPOL_PREP=v2 turns on: 1 = ProvePlan::prep_recode, 2 = prep_share (a build of one part alone: how each was measured)
#endif

struct ProveShape {
    int n, m;
    size_t B;
    // the dapol_options fields the prover reads (zeros = the library's own choices)
    int tail_length, small_call_max, generator_stationary, streams, gs_tile_rows, gs_slices;
    long long chunk_proofs;
    int wbits, nwin, hi_split;        // TableView: window width, windows per canonical scalar, window steps with high-half rows (0: none)
    int n_cu;
    size_t resident_waves;            // dapol_ctx::resident_waves()
    size_t budget_bytes;              // scratch_budget_bytes(ctx)
    bool timed;                       // the call carries an MsmTiming (its brackets sit on the chunk's own stream: no side stream for A)
};

struct ProvePlan {
    int N, lgN, TP;                   // generators a side, log2, digit-row length (RangeArgs)
    int nwin, hi_split;
    int tail_n, tail_lgn;
    bool small_call, use_hi;
    int fs_shape, fs_parts;
    bool gs, gs_mat;
    int gs_LW, acc_slots;
    bool stab_main, stab_tail;
    int msm_split, mat_split, quad_split;
    size_t dig_elems, stab_bytes, acc_bytes, per_proof, split_bytes;
    size_t chunk;
    int nlanes;
    bool big_batch;
    int lpl, tail_lpl;                // set by finalise()
    bool side_A;
    // The tail rounds a lane per (proof, list, window) instead of proof-stationary (kernels_range_gs.h: k_rp_tail_gs); set by finalise().
    // Its window sums live in the chunk's sweep accumulators, which are idle during the tail: tail_rec_bytes per proof on top of
    // acc_bytes only where the order is FORCED onto a call whose accumulators are absent or smaller (tail_order).
    bool tail_gs;
    int tail_order;                   // DAPOL_TAIL_ORDER: -1 = ps, +1 = gs (forced for any call with a tail), 0 = the plan's choice
    size_t tail_rec_bytes;
    // Rows of the proof's tail table a lane of k_rp_tail_table builds: 1, or 4 with one field inversion between them
    // (k_rp_tail_table4); set by finalise().  tail_rpl_forced: DAPOL_TAIL_ROWS_PER_LANE = 1 / 4 (0: the plan's choice).
    int tail_rpl, tail_rpl_forced;
    // DAPOL_PREP = v1 / v2 (default v2): the digit producers of a swept call as they were, or prep_recode: the unrolled recode of the
    // compiled window geometries (write_digits_gs); prep_share: the materialisation's scalars once per (side, k)
    // (k_rp_mat_prep_gs_shared) -- swept materialisation in table mode only.  Neither moves a byte of the scratch layout.
    bool prep_recode, prep_share;
    // what the per-chunk choices below start from
    int gs_tile, gs_slices_forced, mat_cpl_forced;
    bool gs_tile_set, a_lane_ok;
    const char* lpl_env;              // DAPOL_LPL, read once by plan_range_prove (finalise needs it again)

    int part_split() const { return quad_split ? quad_split : msm_split; }
    int nf_rounds() const { return lgN - tail_lgn; }          // never-fold rounds of the main argument
    size_t lane_bytes() const { return (chunk * per_proof + 8192 + split_bytes + 4095) / 4096 * 4096; }

    // A sweep's lanes are (proof, window).  A chunk that has the chip to itself (calls of up to one chunk; the ragged last chunk of a
    // call) sweeps each list in SLICES side by side (k_rp_msm_gs, gridDim.y): a few thousand proofs alone would leave every SIMD a
    // lone wavefront walking its additions one table-lookup latency at a time, and up to ~50,000 the launches are so few wavefront
    // rounds long that the partly filled last round shows (7,680 wavefronts = 1.9 rounds at 32,768 proofs); few lanes also look a
    // table row up only a few times, so there is no tile worth keeping in the Infinity Cache.  One prove call of 4,096 / 8,192 /
    // 16,384 / 32,768 / 49,152 proofs: 107.9 / 184.8 / 336.4 / 632.2 / 940.4 ms unsliced, 90.8 / 174.2 / 324.5 / 616.0 / 918.7 ms in 16 / 16 / 8 / 8 / 4
    // slices; 65,536: no difference (profiles/archive/r05r_gs_slices_forced_sweep.txt, r05s_gs_slices_sweep.txt).  Full chunks stay whole: their tile lives in the Infinity Cache and the other chunk
    // in flight fills the rounds.  dapol_options::gs_slices / DAPOL_GS_SLICES overrides (1, 2, 4, 8, 16).
    int slices_for(size_t cb) const {
        // (a forced count never exceeds the accumulator slots the scratch was sized for: short lists have 2 x min(N / 32, 16) of them)
        if (gs_slices_forced) return gs_slices_forced <= acc_slots / 2 ? gs_slices_forced : acc_slots / 2;
        int ns = cb <= 4096 ? 16 : (cb < 40000 ? 8 : (cb < 65536 ? 4 : 1));
        if (N < 1024) {                                     // by lanes: slices while one list's lanes do not fill the chip twice over
            const size_t lanes = cb * (size_t)gs_LW;
            ns = lanes >= 2 * (size_t)GS_FULL_LANES ? 1 : (lanes >= (size_t)GS_FULL_LANES ? 2 : (lanes >= (size_t)GS_FULL_LANES / 2 ? 4 : (lanes >= (size_t)GS_FULL_LANES / 8 ? 8 : 16)));
        }
        while (ns > 1 && ((N / ns) % 4 != 0 || N / ns < 32)) ns /= 2;
        return ns;
    }
    // Table rows per launch of a sweep of cb proofs in ns slices.
    int tile_for(size_t cb, int ns) const {
        // (few lanes look a row up about once per entry -- there is no tile to keep in the Infinity Cache: longer launches, fewer of them;
        // 8,192 / 12,288 / 16,384 proofs 2-3 % faster with 32 rows, full chunks 1 % slower: profiles/archive/r05o_gs_slices_sweep.txt, r03f_gs_ab_2e20.txt)
        int tile = (!gs_tile_set && cb * (size_t)nwin < 2 * (size_t)GS_FULL_LANES && N / ns >= 32) ? 32 : gs_tile;
        // (two table rows per term: half the terms per launch keep the tile the same 134 MB)
        if (gs_LW < nwin && !gs_tile_set) tile = tile / 2;
        return tile;
    }
    // Window sums per class of the generator-stationary materialisation, and classes per launch of it (1 when one class's lanes fill
    // the chip; DAPOL_GS_MAT_CPL overrides).
    int mat_LW() const { return hi_split ? hi_split : nwin; }
    int mat_cpl(size_t cb) const {
        if (mat_cpl_forced) return mat_cpl_forced;
        int cpl = 1;
        while (cpl < MAT_GROUP && cb * (size_t)mat_LW() * (size_t)cpl < GS_FULL_LANES) cpl *= 2;
        return cpl;
    }
    // short proofs in bulk: the A commitment with a lane per proof (k_rp_A_lane) instead of a wavefront (DAPOL_NO_A_LANE=1: never)
    bool a_lane(size_t cb) const { return !side_A && gs && N < 1024 && cb >= 4096 && a_lane_ok; }

    void finalise(const ProveShape& s, size_t chunk_, int nlanes_);
};

// Small calls: into how many wavefronts a proof's main MSM may be split (DAPOL_SMALL_SPLIT overrides; a power of two <= 64).
static int small_split_cap(bool use_hi) {
    if (const char* e = knob("DAPOL_SMALL_SPLIT")) { int v = atoi(e); if (v >= 1 && v <= 64 && !(v & (v - 1))) return v; }
    return use_hi ? 64 : 8;
}
// Most wavefronts a launch of the four-lanes-per-point kernels may have (DAPOL_QUAD_MAX_WAVES overrides the measured defaults).
static size_t quad_max_waves(size_t dflt) {
    if (const char* e = knob("DAPOL_QUAD_MAX_WAVES")) { long long v = atoll(e); if (v > 0) return (size_t)v; }
    return dflt;
}
// Lanes per term list for launches of `proofs` proofs: the candidate that minimises (rounds of resident wavefronts: CUs x 4 x 3) x
// (mixed adds + shared doublings per lane).  Few lanes per list amortise the doublings; many fill the chip when the call is small.
// shared_simd (the tail MSM's picker since the end of round 3): what was measured instead of that -- k wavefronts sharing a SIMD take
// about 1 + 0.23 (k - 1) times a lone wavefront's chain (a lone one leaves the issue slots between its dependent multiply-adds
// and under its table lookups empty: 16,384 proofs 2 -> 8 lanes per list = 1 -> 4 wavefronts per SIMD with a third of the chain each,
// 330.9 -> 316.7 ms per call), and one proof per wavefront pays double per addition (64 different rows per lookup instruction):
// profiles/archive/r05w_tail_lpl_sweep.txt.
static int pick_lanes_per_list(size_t proofs, int terms_per_list, int nwin, int wbits, const int* cand, int ncand, size_t resident, size_t n_simd,
                               bool shared_simd = false) {
    // A SIMD interleaves its resident wavefronts, so a round in which it holds k of them takes about k times a lone wavefront's
    // chain: cost = (chain per lane) x (wavefronts per SIMD, summed over the rounds).  (Round 1 counted rounds only, which made
    // one proof per wavefront look free for a few thousand proofs: 190 ms instead of 114 for 4,096, profiles/archive/r02_midsize_ab.txt.)
    int best = cand[0];
    double best_cost = 1e300;
    const size_t occ = n_simd ? (resident + n_simd - 1) / n_simd : 1;
    for (int i = 0; i < ncand; i++) {
        int lpl = cand[i];
        size_t waves = (proofs + (size_t)(32 / lpl) - 1) / (size_t)(32 / lpl);
        const size_t full = waves / resident, rem = waves % resident;
        const size_t krem = rem ? (rem + n_simd - 1) / (n_simd ? n_simd : 1) : 0;
        double per_simd = (double)(full * occ) + (double)krem;
        if (shared_simd) per_simd = (double)full * (1.0 + 0.23 * (double)(occ - 1)) + (krem ? 1.0 + 0.23 * (double)(krem - 1) : 0.0);
        double per_lane = (double)((terms_per_list + lpl - 1) / lpl) * nwin * (shared_simd && lpl == 32 ? 2.0 : 1.0) + (double)nwin * wbits;
        double cost = per_simd * per_lane;
        if (cost < best_cost) { best_cost = cost; best = lpl; }
    }
    return best;
}
static int tail_lanes_per_list(bool small_call, const char* e /* DAPOL_TAIL_LPL */) {
    if (e) { int v = atoi(e); if (v == 1 || v == 2 || v == 4 || v == 8 || v == 32) return v; }
    if (small_call) return 32;     // one proof per wavefront: latency, not throughput
    return 2;                 // measured 2^16 proofs, m = 32: 36.1K / 37.0K / 35.9K entities/s at 4 / 2 / 8 (profiles/archive/r01_tail_ab.txt)
}
// big_batch: the call carries at least one full chunk (whole rounds of resident wavefronts), so 16 proofs per wavefront
// (LPL = 2: 1,024 terms per lane, the 255 shared doublings amortised over 15,360 additions) still fill the chip; smaller calls
// keep 4 per wavefront (finer granularity).  Measured interleaved (profiles/archive/r02_lpl2_tail6_ab.txt): LPL 4 -> 2 +0.9 % at
// 2^18 proofs, +1.5 % at 2^20.
static int msm_lanes_per_list(int N, bool big_batch = false, const char* e = knob("DAPOL_LPL")) {
    if (e) { int v = atoi(e); if (v == 2 || v == 4 || v == 8 || v == 16 || v == 32) return v; }
    return N >= 1024 ? (big_batch ? 2 : 8) : (N >= 256 ? 16 : 32);
}

// Bytes per proof of the window sums of one tail round in the lane-per-accumulator order: two lists x TAIL_NWIN records of X | Y | Z | T.
static size_t tail_rec_need() { return (size_t)2 * TAIL_NWIN * 4 * FE_NL * 4; }

static ProvePlan plan_range_prove(const ProveShape& s) {
    ProvePlan P{};
    const size_t B = s.B;
    const int N = s.n * s.m;
    P.N = N;
    while ((1 << P.lgN) < N) P.lgN++;
    P.TP = 2 * N < 64 ? 64 : 2 * N;
    P.nwin = s.nwin; P.hi_split = s.hi_split;
    const int lgN = P.lgN;
    // Hybrid inner-product argument: never-fold rounds while the vectors are longer than T, then materialise the 2T
    // folded generators once and finish on the proof's own small tables (DESIGN.md section 4.4).
    int tail_n = 64;
    if (s.tail_length > 0) tail_n = s.tail_length;
    const char* const e_tail_n = knob("DAPOL_TAIL_N");
    if (e_tail_n) { int v = atoi(e_tail_n); if (v == 32 || v == 64 || v == 128 || v == 256) tail_n = v; }
    if (lgN < 8 || s.tail_length < 0 || knob("DAPOL_NO_TAIL")) tail_n = 0;
    // DAPOL_GS=0 / 1 forces the proof-stationary / the generator-stationary form for any call that is not a small one
    const char* const e_gs = knob("DAPOL_GS");
    const int gs_env = e_gs ? (atoi(e_gs) != 0 ? 1 : 0) : -1;
    // SHORT lists in LARGE batches (round 6): a policy's individual proofs (m = 1: 64 generators a side) and proofs of 2 ... 8 parties,
    // batched by prove_policy_device.  The proof-stationary kernel gives such a proof a wavefront per MSM whose lanes own two terms and
    // 255 shared doublings each (1/8 of the work is additions); swept generator-stationary (k_rp_msm_gs_hi) the batch does the 15
    // additions per term and a Horner combine of 126 addition-equivalents per list.  From gs_small_min proofs on (DAPOL_GS_SMALL_MIN;
    // an explicit generator_stationary option / DAPOL_GS still decides alone).
    // (individual proofs: 1,024 / 2,048 / 4,096 proofs 5.9 / 9.1 / 16.4 ms proof-stationary, 6.2 / 6.5 / 7.0 ms swept -- profiles/r6_small_parties_sweeps.txt)
    // (2 / 4 / 8 parties: 1,024 proofs 7.7 / 11.0 / 13.8 ms with the latency shapes, 7.2 / 8.8 / 12.3 ms swept; 4,096 proofs 21.1 / 29.4 / 38.4
    // against 9.9 / 16.4 / 27.3 ms -- same file)
    // (512 proofs of 4 / 8 parties: 9.7 / 11.7 ms against 8.0 / 10.5 swept; 1 and 2 parties: level or slower below the values here)
    size_t gs_small_min = N == 64 ? 2048 : (N == 128 ? 1024 : 512);
    if (const char* e = knob("DAPOL_GS_SMALL_MIN")) { long long v = atoll(e); if (v >= 64) gs_small_min = (size_t)v; }
    const bool gs_small = N >= 64 && N < 1024 && N % 4 == 0 && B >= gs_small_min && s.generator_stationary == 0 && gs_env < 0;
    // (the tail's materialisation is 2T Horner chains per proof whatever N: below 512 generators a side the remaining never-fold
    // rounds are cheaper -- N = 256: 46 K additions against 24 K + 39 K for materialisation + tail rounds)
    if (gs_small && N < 512 && !e_tail_n) tail_n = 0;
    // (512 generators a side, 2^16 proofs: 373 ms with T = 64, 321 with T = 32, 400 without a tail -- same file)
    if (gs_small && N == 512 && tail_n == 64 && s.tail_length == 0 && !e_tail_n) tail_n = 32;
    // Small calls (a user's proof on demand) are latency-bound: one proof per wavefront and the term range of every proof
    // split over many wavefronts (partials summed by k_rp_sum_splits), so that a single proof keeps 64 SIMDs busy instead
    // of a quarter of one.  Measured (tools/bench_latency.py): one 64-bit m = 32 proof in 104 ms before.
    // With the tables' high-half rows (TableView::hi_split) a small call also halves the window steps of the main MSM -- the 238
    // shared doublings are most of a lone wavefront's chain -- and splits down to one term per lane (64 ways); up to 32
    // proofs then skip the tail argument (whose per-proof tables have no high-half rows: 0.66 ms per round against 0.3 ms),
    // the materialisation is split the same way otherwise (k_rp_sum_mat), and the lane-per-proof Fiat-Shamir kernels put a
    // proof's two point computations on two lanes (PAIR).  One height-32 padding proof: 18.6 -> 8.7 ms
    // (profiles/archive/r02x_latency_sweep.txt).
    // (the latency shapes win up to where the generator-stationary sweep takes over: 5,000 / 6,144 / 7,168 proofs 16 / 21 / 30 % faster than
    // the proof-stationary throughput shapes, 8,000 proofs level with the sweep -- profiles/archive/r04h_small_max_probe.txt, r02_midsize_ab.txt)
    size_t small_max = s.small_call_max > 0 ? (size_t)s.small_call_max : 8191;
    const char* const e_small_max = knob("DAPOL_SMALL_MAX");
    if (e_small_max) { long long v = atoll(e_small_max); if (v >= 1) small_max = (size_t)v; }
    // ... except where the sweep in slices (ProvePlan::slices_for) is faster: calls of gs_min proofs or more over at least 1,024 generators a side
    // (1,280 / 3,072 / 4,096 / 6,144 proofs 14 / 15 / 14 / 6 % faster than the latency shapes, level at 1,024, slower at 512: profiles/archive/r05q_gs_slices16_sweep.txt, r05r_gs_slices_forced_sweep.txt).  An explicit
    // small_call_max / DAPOL_SMALL_MAX is taken at its word.
    size_t gs_min = 1024;
    if (const char* e = knob("DAPOL_GS_MIN")) { long long v = atoll(e); if (v >= 1) gs_min = (size_t)v; }
    const bool gs_shape = N >= 1024 && N % 4 == 0 && s.generator_stationary >= 0 && gs_env != 0;
    if (gs_shape && s.small_call_max <= 0 && !e_small_max && small_max >= gs_min) small_max = gs_min - 1;
    const char* const e_lpl = knob("DAPOL_LPL");
    P.lpl_env = e_lpl;
    const bool small_call = B <= small_max && N >= 256 && !e_lpl && !knob("DAPOL_NO_SPLIT") && !gs_small;
    const bool use_hi = small_call && s.hi_split && !knob("DAPOL_NO_SMALL_HI");
    P.small_call = small_call; P.use_hi = use_hi;
    // The Fiat-Shamir kernels' shape (DAPOL_FS_SHAPE=0/1/2 overrides; DAPOL_NO_PAIR=1 is shape 0)
    // (mid-size calls, which have the chip to themselves, keep the shapes that shorten a proof's serial chain: 1,024 proofs 34.5 ms with
    // a lane per proof, 32.2 with lane pairs, 31.4 with a wavefront per proof; 4,096: 91.7 / 89.5 / 92.1; 16,384: 329.6 / 327.7 / 347.4 --
    // profiles/archive/r05v_fs_shape_sweep.txt)
    P.fs_shape = !small_call ? (B <= 1536 ? 2 : (B <= 16384 ? 1 : 0)) : (B <= 256 ? 2 : 1);
    if (knob("DAPOL_NO_PAIR")) P.fs_shape = 0;
    if (const char* e = knob("DAPOL_FS_SHAPE")) { int v = atoi(e); if (v >= 0 && v <= 2) P.fs_shape = v; }
    if (use_hi && B <= 32 && !knob("DAPOL_SMALL_TAIL")) tail_n = 0;                     // (64 proofs: 14.8 ms with the tail, 15.6 without)
    while (tail_n && 4 * tail_n > N) tail_n >>= 1;               // at least two never-fold rounds before the tail
    if (tail_n && tail_n < 32) tail_n = 0;
    int tail_lgn = 0;
    while (tail_n && (1 << tail_lgn) < tail_n) tail_lgn++;
    P.tail_n = tail_n; P.tail_lgn = tail_lgn;
    const size_t T = (size_t)tail_n;
    // the digit matrix serves the main argument (nwin x 2N) and later the tail (TAIL_NWIN x 2T)
    size_t dig_elems = (size_t)s.nwin * P.TP;
    if (dig_elems < (size_t)TAIL_NWIN * 2 * T) dig_elems = (size_t)TAIL_NWIN * 2 * T;
    P.dig_elems = dig_elems;
    // What the call can use is decided BEFORE the scratch is sized (the chunk size follows from per_proof): the coefficient tables
    // only where an argument is short enough for them, the sweep's accumulators (69 KB per proof at 17-bit windows) only where
    // the generator-stationary form can run at all -- individual 64-generator proofs (m = 1, the splitting policy's tail) and the
    // latency shapes keep 17 KB per proof instead of 94 and therefore four times the chunk in the same budget.
    // Coefficient tables instead of per-round s-vector updates (kernels_range.h, RangeArgs::stab) wherever the argument needs at
    // most TG_6: the main argument when a tail follows within six rounds (or is that short itself), the tail argument up to T = 128.
    const bool no_stab = knob("DAPOL_NO_STAB") != nullptr;
    P.stab_main = !no_stab && (tail_n ? lgN - tail_lgn : lgN - 1) <= STAB_ROUNDS;
    P.stab_tail = !no_stab && tail_n && tail_lgn - 1 <= STAB_ROUNDS;
    bool gs_possible = (!small_call && N % 4 == 0 && N >= 1024 && B >= gs_min) || gs_small;
    if (s.generator_stationary) gs_possible = s.generator_stationary > 0 && !small_call && N % 4 == 0 && N >= 64;
    if (gs_env >= 0) gs_possible = gs_env != 0 && !small_call && N % 4 == 0 && N >= 64;
    // (one accumulator per list, slice, proof and window; MAT_GROUP classes of them for the materialisation.  Short lists have at
    // most N / 32 slices, and no classes without a tail)
    int acc_slots = GS_ACC_SLOTS;
    if (N < 1024) {
        acc_slots = 2 * (N / 32 < GS_MAX_SLICES ? N / 32 : GS_MAX_SLICES);
        if (tail_n && acc_slots < MAT_GROUP) acc_slots = MAT_GROUP;
    }
    P.acc_slots = acc_slots;
    P.acc_bytes = gs_possible ? (size_t)acc_slots * s.nwin * 4 * FE_NL * 4 : 0;
    P.stab_bytes = (P.stab_main || P.stab_tail) ? (size_t)2 * 2 * STAB_N * sizeof(sc) : 0;     // coefficient tables (two buffers x two sides)
    // DAPOL_TAIL_ORDER = ps / gs forces the order of the tail rounds (ProvePlan::tail_gs) for any call that has a tail.  A forced gs
    // needs 2 x TAIL_NWIN records per proof whatever the regime; the plan's own choice only ever uses accumulators that are there.
    if (const char* e = knob("DAPOL_TAIL_ORDER")) P.tail_order = (e[0] == 'g' && e[1] == 's' && !e[2]) ? 1 : ((e[0] == 'p' && e[1] == 's' && !e[2]) ? -1 : 0);
    if (const char* e = knob("DAPOL_TAIL_ROWS_PER_LANE")) { int v = atoi(e); if (v == 1 || v == 4) P.tail_rpl_forced = v; }
    P.tail_rec_bytes = (P.tail_order > 0 && tail_n && P.acc_bytes < tail_rec_need()) ? tail_rec_need() - P.acc_bytes : 0;
    P.per_proof = 4 * (size_t)N * sizeof(sc) + dig_elems * sizeof(dig_t) + (sizeof(ProofState) + 15) / 16 * 16 + 3 * 160 +
                  2 * T * TAIL_ROW_WORDS * 4 + 4 * T * sizeof(sc) + FS_PARTS_MAX * 3 * sizeof(sc) + P.stab_bytes + P.acc_bytes + P.tail_rec_bytes;
    // ONE chunk in flight by default since round 4 (dapol_options::streams / DAPOL_STREAMS = 2..4 puts more in flight, on the
    // context's side streams with their own shares of the scratch).  History: round 1 measured +4.8 % for two chunks in flight
    // (the scalar-vector kernels and the Fiat-Shamir chains of one chunk under the other's MSM, profiles/archive/r01_streams_ab.txt);
    // with the generator-stationary sweep the two only share the chip (round 3: +0.4 %, profiles/archive/r05g_timeline_gaps.txt), and round 4
    // tried to give the HBM-bound kernels CUs or priority of their own -- CU-masked halves, a masked stream for the VALU-bound
    // launches with 16 / 32 CUs left to the rest, stream priorities: every layout was slower than plain streams and the code was
    // removed (profiles/archive/r07a_stream_layout_ab.txt).  One stream with the same scratch spent on chunks of TWO rounds of resident
    // wavefronts (131,072 proofs) instead of two chunks of one round: +0.45 % at 2^20, +0.5 % at 2^18; three rounds (153 GB)
    // +0.7 %; one round on one stream (half the scratch) -1.6 % (profiles/archive/r07b_one_stream_chunks_ab.txt).
    int nlanes = s.streams > 0 ? s.streams : 1;
    if (const char* e = knob("DAPOL_STREAMS")) { int v = atoi(e); if (v >= 1 && v <= 4) nlanes = v; }
    size_t chunk = s.budget_bytes / nlanes / P.per_proof;
    if (chunk < 1) chunk = 1;
    if (chunk > B) chunk = B;
    // Launches are sized in whole "rounds" of resident wavefronts: the MSM kernels hold 3 wavefronts per SIMD
    // (256 CUs x 4 SIMDs x 3 = 3072) and every wavefront of a launch does the same work, so a launch of k * 3072
    // wavefronts wastes nothing on a partly filled last round.  61440 proofs = 5 rounds at 4 proofs per wavefront
    // (main MSM), 20 rounds at one (materialisation).  Measured at 2^20 proofs (profiles/archive/r01_chunk_ab.txt): 37.5K /
    // 37.6K / 38.7K / 38.7K entities/s at 49152 / 60000 / 61440 / 73728.  Calls of at least 73,728 proofs use chunks of
    // that size with 8 proofs per wavefront (3 rounds; half the shared doublings: +1.3 %, profiles/archive/r01_lpl4_ab.txt).
    // dapol_options::chunk_proofs / DAPOL_CHUNK and DAPOL_LPL override.
    {
        const char* const e_chunk = knob("DAPOL_CHUNK");
        const bool chunk_set = e_chunk || s.chunk_proofs > 0;
        const long long chunk_forced = e_chunk ? atoll(e_chunk) : s.chunk_proofs;
        // whole rounds of resident wavefronts: 16 proofs per wavefront for big calls -- as many rounds (<= 3) as the scratch holds:
        // ONE round of 4,096 wavefronts = 65,536 proofs on MI355X (256 CUs x 4 SIMDs x 4 resident wavefronts of k_rp_msm) -- and
        // 5 rounds at 4 proofs each otherwise
        const size_t rw = s.resident_waves;
        size_t ppw = 16;                                        // proofs per wavefront of a big call (LPL = 2; DAPOL_LPL overrides)
        if (e_lpl) { int v = atoi(e_lpl); if (v == 2 || v == 4 || v == 8) ppw = (size_t)(32 / v); }
        const size_t big_chunk = (3 * rw * ppw <= chunk) ? 3 * rw * ppw : ((2 * rw * ppw <= chunk) ? 2 * rw * ppw : rw * ppw), std_chunk = 5 * rw * 4;
        P.big_batch = !chunk_set && N >= 1024 && B >= big_chunk && chunk >= big_chunk;
        size_t cap = chunk_set ? (size_t)chunk_forced : (P.big_batch ? big_chunk : std_chunk);
        // short lists: a sweep's lanes are (proof, window < 8) -- chunks of whole rounds of resident wavefronts, up to 8 of them
        // (262,144 individual proofs: 6.5 GB of scratch)
        const size_t small_unit = rw * 64 / (size_t)(s.hi_split ? s.hi_split : s.nwin);
        if (gs_small && !chunk_set) cap = 8 * small_unit;
        if (cap < 64) cap = 64;
        if (chunk > cap) chunk = cap;
        if (gs_small && !chunk_set && chunk > small_unit) chunk -= chunk % small_unit;
    }
    while (nlanes > 1 && chunk * (size_t)(nlanes - 1) >= B) nlanes--;
    P.chunk = chunk; P.nlanes = nlanes;
    // Large calls sweep the generators instead of the proofs (kernels_range_gs.h): every wavefront of a launch reads the same
    // tile of table rows, which therefore sits in the Infinity Cache.  DAPOL_GS_TILE = rows per launch (a multiple of 4).
    // (also below one full chunk, for proofs of at least 1,024 generators per side: one prove call of 8,192 / 16,384 / 32,768 / 49,152 proofs
    // 23 / 6 / 11 / 11 % faster than proof-stationary, profiles/archive/r04e_gs_midsize_sweep.txt; in slices from gs_min proofs on, see above)
    // (what counts is the proofs per CHUNK -- the lanes of one sweep: many-party proofs get small chunks out of the scratch budget)
    bool gs = P.big_batch || (!small_call && B >= gs_min && chunk >= 1024 && N >= 1024 && N % 4 == 0) || (gs_small && chunk >= 64);
    if (s.generator_stationary) gs = s.generator_stationary > 0 && !small_call && N % 4 == 0 && N >= 64;
    if (gs_env >= 0) gs = gs_env != 0 && !small_call && N % 4 == 0 && N >= 64;
    if (!gs_possible) gs = false;                            // (no accumulators were counted into the scratch)
    P.gs = gs;
    P.gs_mat = gs && tail_n && (N / tail_n) % 4 == 0 && !knob("DAPOL_NO_GS_MAT");
    {
        const char* const e = knob("DAPOL_PREP");
        const int parts = (e && e[0] == 'v' && e[1] == '1' && !e[2]) ? 0 : DAPOL_PREP_V2_PARTS;     // (anything but v1 is no value)
        P.prep_recode = gs && (parts & 1);
        P.prep_share = P.gs_mat && P.stab_main && (parts & 2);
    }
    P.gs_tile = s.gs_tile_rows > 0 ? s.gs_tile_rows : 16;
    const char* const e_tile = knob("DAPOL_GS_TILE");
    P.gs_tile_set = s.gs_tile_rows > 0 || e_tile;
    if (e_tile) { int v = atoi(e_tile); if (v >= 4 && v % 4 == 0) P.gs_tile = v; }
    P.gs_slices_forced = (s.gs_slices > 0 && N % (4 * s.gs_slices) == 0 && N / s.gs_slices >= 4) ? s.gs_slices : 0;
    if (const char* e = knob("DAPOL_GS_SLICES")) { int v = atoi(e); if ((v == 1 || v == 2 || v == 4 || v == 8 || v == 16) && N % (4 * v) == 0 && N / v >= 4) P.gs_slices_forced = v; }
    // Short lists (fewer than 1,024 generators a side) are swept with two lookups per term where the tables have high-half rows:
    // LW = hi_split window sums per list instead of nwin (k_rp_msm_gs_hi; DAPOL_NO_GS_HI=1: the plain sweep).
    P.gs_LW = (gs && N < 1024 && s.hi_split && !knob("DAPOL_NO_GS_HI")) ? s.hi_split : s.nwin;
    if (const char* e = knob("DAPOL_GS_MAT_CPL")) { int v = atoi(e); if (v >= 1 && v <= MAT_GROUP) P.mat_cpl_forced = v; }
    P.a_lane_ok = !knob("DAPOL_NO_A_LANE");
    P.msm_split = 1; P.mat_split = 1;
    if (small_call) {
        const int cap = small_split_cap(use_hi), min_terms = use_hi ? 1 : 4;
        while (P.msm_split < cap && (size_t)P.msm_split * 2 * B <= 2048 && N / 32 / (P.msm_split * 2) >= min_terms) P.msm_split *= 2;
        if (tail_n && !knob("DAPOL_NO_SPLIT_MAT"))
            while (P.mat_split < 8 && (size_t)(P.mat_split * 2) * B * (size_t)(tail_n / 32) <= 4096 && N / tail_n / (P.mat_split * 2) >= 2) P.mat_split *= 2;
    }
    // ... and the two 2N-position scalar phases (k_rp_poly, k_rp_lr) are walked by up to 8 wavefronts per proof instead of one
    P.fs_parts = 1;
    if (small_call && B <= 64 && !knob("DAPOL_NO_FS_PARTS")) {
        const int iters = (N + 63) / 64;
        while (P.fs_parts < FS_PARTS_MAX && iters / (P.fs_parts * 2) >= 2) P.fs_parts *= 2;
    }
    // ... and with one point per four lanes when the proofs are few enough for 4x the wavefronts (DAPOL_NO_QUAD=1: lane kernel)
    // Four lanes per point is 1.5x the work per point: it pays while the launch is a lone wavefront's chain, up to about 8 proofs
    // (profiles/archive/r02_midsize_ab.txt: 8 proofs 6.5 against 6.8 ms, 16 proofs 8.9 against 6.9).
    if (use_hi && P.msm_split > 1 && (size_t)P.msm_split * 4 * B <= quad_max_waves(2048) && N % (8 * P.msm_split * 4) == 0 && !knob("DAPOL_NO_QUAD")) P.quad_split = P.msm_split * 4;
    // (sized for the chunk chosen here: a chunk halved by the launcher's out-of-memory fallback keeps this share)
    P.split_bytes = (P.part_split() > 1 ? (2 * chunk * (size_t)P.part_split() * 160 + 255) / 256 * 256 : 0) +
                    (P.mat_split > 1 ? (chunk * 2 * T * (size_t)P.mat_split * 160 + 255) / 256 * 256 : 0);
    P.finalise(s, chunk, nlanes);
    return P;
}

// The chunk size and the chunks in flight that the scratch allocation allowed (the launcher may have lowered both): the lanes per
// list follow from the FINAL chunk, and so does whether the A commitment gets a side stream.
void ProvePlan::finalise(const ProveShape& s, size_t chunk_, int nlanes_) {
    chunk = chunk_; nlanes = nlanes_;
    const char* const e_tail_lpl = knob("DAPOL_TAIL_LPL");
    lpl = msm_lanes_per_list(N, big_batch, lpl_env);
    tail_lpl = tail_lanes_per_list(small_call, e_tail_lpl);
    if (small_call) lpl = 32;
    else if (!lpl_env && N >= 1024 && !big_batch && chunk < 32768) {    // mid-size calls; large ones keep the measured defaults
        // (one proof per wavefront is not a candidate: with 64 different table rows per lookup instruction the kernel runs at half the
        // rate per addition of 32 or fewer -- 2,048 proofs 98 -> 63 ms, 4,096 proofs 190 -> 114 ms, profiles/archive/r02_midsize_ab.txt)
        const int cand[2] = {8, 16};
        lpl = pick_lanes_per_list(chunk, N, s.nwin, s.wbits, cand, 2, s.resident_waves, (size_t)s.n_cu * 4);
    }
    if (!e_tail_lpl && !small_call && tail_n && chunk < 65536) {             // (a chunk that has the chip to itself; full chunks: 2, measured)
        const int cand[4] = {2, 4, 8, 32};
        tail_lpl = pick_lanes_per_list(chunk, tail_n, TAIL_NWIN, TAIL_WBITS, cand, 4, s.resident_waves, (size_t)s.n_cu * 4, true);
    }
    // The tail rounds with a lane per (proof, list, window): swept calls of at least 1,024 generators a side whose chunk is a full one
    // (65,536 proofs or more: 6.7 M lanes, the chip 34 times over) -- the shape it was measured at: a round of a 131,072-proof chunk
    // 26.3 + 2.3 ms against 34.9 proof-stationary, the headline +1.06 / +1.48 % in two interleaved pairs against 0.15 % between the
    // parent's own runs (profiles/tail_order_ab.txt).  Smaller chunks have the chip to themselves and keep the proof-stationary
    // kernel with the lanes per list picked above (not measured in the new order).  Only where the sweep's accumulators hold a
    // round's records (15 windows of 17 bits: 69,120 B a proof against 14,688).
    tail_gs = tail_n != 0 && (tail_order > 0 || (tail_order == 0 && TAIL_GS_DEFAULT && gs && !small_call && N >= 1024 && chunk >= 65536 && acc_bytes >= tail_rec_need()));
    // Four table rows a lane (a quarter of the inversions, four times the chain of a lane): full chunks as above, where the launch is
    // tens of wavefront rounds long whichever way (the headline +0.20 / +0.51 % against one row a lane in two interleaved rounds, the
    // parent's own runs 0.26 % apart: same file); never where a proof's 2T rows do not divide by four.
    tail_rpl = tail_rpl_forced ? tail_rpl_forced : ((TAIL_RPL_DEFAULT == 4 && gs && !small_call && N >= 1024 && chunk >= 65536) ? 4 : 1);
    if (!tail_n || (2 * tail_n) % 4 != 0) tail_rpl = 1;
    // a small call's A commitment (a chain of additions on one wavefront) runs beside the S commitment's MSM
    side_A = small_call && nlanes == 1 && s.B <= 64 && !s.timed && !knob("DAPOL_NO_SIDE_A");
}

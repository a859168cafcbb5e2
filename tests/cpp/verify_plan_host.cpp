// Host-only build of the range verifier's planning (dapol_amd/csrc/verify_plan.inc): reads rows "KEY=VALUE ..." from stdin -- the
// fields of VerifyShape, and DAPOL_* names, which are set in the environment for that row only -- and prints per row what the plans
// hold, as lines of "KEY=VALUE ..." in the field names of tests/golden/verify_plan.json:
//   call pipe=..     verify_pipe_arrival: dapol_range_verify_batch attaches a VArrival (the golden's va_K is nonzero)
//   rlc ...          plan_range_verify_rlc (a call that is not batched: use_rlc, rlc_min and pipelined only)
//   rlc_chunk ...    RlcPlan::chunk_plan for the full chunk, and for the ragged last one if there is one
//   rv ...           plan_range_verify, for a call that is not batched
//   rv_chunk ...     VerifyPlan::quad_var per distinct chunk size
//   end
// Build + run: tests/test_verify_plan_cpu.py (once plain, once under -fsanitize=address,undefined)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "sc.h"              // sc

using namespace dapol;

// The layout constants the plans size their scratch with, as in tables.h / kernels_verify.h (HIP headers: not includable here;
// host_verify.inc asserts the size of VerifyState).
typedef int32_t dig_t;
struct VerifyState { unsigned char bytes[2968]; };
enum { RVP_C = 11, RVP_NW = 23, RVP_NB = 1 << (RVP_C - 1) };
enum { PT_WBITS = 4, PT_NWIN = 253 / PT_WBITS + 1, PT_ENTRIES = (1 << (PT_WBITS - 1)) + 1, PT_ROW_WORDS = PT_ENTRIES * 32 };
static int rv_tab_entries(int lgN, int m) {
    int lb = lgN / 2, hb = lgN - lb;
    return 2 * (1 << hb) + 2 * (1 << lb) + m;
}
static int rv_tab_entries_rlc(int lgN, int m) {
    int lb = lgN / 2, hb = lgN - lb;
    return rv_tab_entries(lgN, m) + 3 * (1 << hb) + 2 * (1 << lb) + 1;
}
// (what prove_plan.inc sizes with; the verifier's plans use its lane and split pickers only)
struct ProofState { unsigned char bytes[760]; };
enum { TAIL_WBITS = 5, TAIL_NWIN = 253 / TAIL_WBITS + 1, TAIL_ENTRIES = (1 << (TAIL_WBITS - 1)) + 1, TAIL_ROW_WORDS = TAIL_ENTRIES * 32 };
enum { STAB_ROUNDS = 6, STAB_N = 1 << STAB_ROUNDS };
enum { MAT_GROUP = 16 };
enum { GS_ACC_SLOTS = 32, GS_MAX_SLICES = 16, GS_FULL_LANES = 3072 * 64 };

static const char* knob(const char* name) { return getenv(name); }

#include "prove_plan.inc"
#include "verify_plan.inc"

static void print_rlc_chunk(const RlcPlan& P, size_t cb) {
    const RlcChunk C = P.chunk_plan(cb);
    printf("rlc_chunk cb=%zu G=%d npts=%zu Np=%zu TP2=%d ns2=%d pippenger=%d lazy=%d wave_replay=%d fork=%d o_dig=%zu o_vs=%zu o_p0=%zu o_p1=%zu o_part=%zu "
           "o_gpart=%zu o_bsum=%zu o_pt=%zu o_dig2=%zu o_q0=%zu o_q1=%zu o_flag=%zu o_tabs=%zu o_dga=%zu o_dgb=%zu o_t29=%zu o_rzg=%zu need=%zu",
           C.cb, C.G, C.npts, C.Np, C.TP2, C.ns2, (int)C.pippenger, (int)C.lazy, (int)C.wave_replay, (int)C.fork, C.o_dig, C.o_vs, C.o_p0, C.o_p1, C.o_part,
           C.o_gpart, C.o_bsum, C.o_pt, C.o_dig2, C.o_q0, C.o_q1, C.o_flag, C.o_tabs, C.o_dga, C.o_dgb, C.o_t29, C.o_rzg, C.need);
    if (C.pippenger)
        printf(" b_pN=%zu b_pdig=%zu b_psorted=%zu b_phist=%zu b_poffs=%zu b_pcursor=%zu b_pbsum=%zu b_hsz=%zu b_end=%zu b_region=%zu b_fits=%d", C.b_pN, C.b_pdig,
               C.b_psorted, C.b_phist, C.b_poffs, C.b_pcursor, C.b_pbsum, C.b_hsz, C.b_end, C.b_region, (int)C.b_fits);
    printf("\n");
}

int main() {
    char buf[4096];
    while (fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string tok;
        std::vector<std::string> env;
        VerifyShape s{};
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "bad token %s\n", tok.c_str()); return 2; }
            const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
            const long long x = atoll(v.c_str());
            if (k.rfind("DAPOL_", 0) == 0) { setenv(k.c_str(), v.c_str(), 1); env.push_back(k); }
            else if (k == "n") s.n = (int)x;
            else if (k == "m") s.m = (int)x;
            else if (k == "b") s.b = (size_t)x;
            else if (k == "opt_verify_batch_min") s.opt_verify_batch_min = (int)x;
            else if (k == "wbits") s.wbits = (int)x;
            else if (k == "nwin") s.nwin = (int)x;
            else if (k == "hi_split") s.hi_split = (int)x;
            else if (k == "n_cu") s.n_cu = (int)x;
            else if (k == "budget_bytes") s.budget_bytes = (size_t)x;
            else if (k == "va_K") s.va_K = (int)x;
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        printf("call pipe=%d\n", (int)verify_pipe_arrival(s.m, s.b));
        const RlcPlan R = plan_range_verify_rlc(s);
        printf("rlc use_rlc=%d rlc_min=%zu pipelined=%d", (int)R.use_rlc, R.rlc_min, (int)R.pipelined);
        if (R.use_rlc) {
            printf(" N=%d lgN=%d TP=%d quad_gen=%d gen_sweep=%d gen_ns=%d nsplit=%d lpl=%d use_hi=%d K=%d lb=%d hb=%d tab_stride=%d per_proof=%zu fixed=%zu chunk=%zu "
                   "nch=%d pip_min=%zu fork_points=%d wave_transcript=%d\n", R.N, R.lgN, R.TP, (int)R.quad_gen, (int)R.gen_sweep, R.gen_ns, R.nsplit, R.lpl, (int)R.use_hi, R.K,
                   R.lb, R.hb, R.tab_stride, R.per_proof, R.fixed, R.chunk, R.nch, R.pip_min, (int)R.fork_points, (int)R.wave_transcript);
            print_rlc_chunk(R, R.chunk);
            if (s.b % R.chunk) print_rlc_chunk(R, s.b % R.chunk);
        } else {
            const VerifyPlan P = plan_range_verify(s);
            printf("\nrv N=%d lgN=%d TP=%d small_call=%d use_hi=%d lpl=%d nsplit=%d quad=%d lb=%d hb=%d tab_stride=%d var_waves=%d per_proof=%zu chunk=%zu tree_sum=%d "
                   "wave_transcript=%d wave_replay=%d side_var=%d\n", P.N, P.lgN, P.TP, (int)P.small_call, (int)P.use_hi, P.lpl, P.nsplit, (int)P.quad, P.lb, P.hb, P.tab_stride,
                   P.var_waves, P.per_proof, P.chunk, (int)P.tree_sum, (int)P.wave_transcript, (int)P.wave_replay, (int)P.side_var);
            printf("rv_chunk cb=%zu quad_var=%d\n", P.chunk, (int)P.quad_var(P.chunk));
            if (s.b % P.chunk) printf("rv_chunk cb=%zu quad_var=%d\n", s.b % P.chunk, (int)P.quad_var(s.b % P.chunk));
        }
        for (auto& k : env) unsetenv(k.c_str());
        printf("end\n");
    }
    return 0;
}

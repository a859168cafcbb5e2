// Host-only build of the range prover's planning (dapol_amd/csrc/prove_plan.inc): reads rows "KEY=VALUE ..." from stdin -- the
// fields of ProveShape, and DAPOL_* names, which are set in the environment for that row only -- and prints the ProvePlan of each as
// "KEY=VALUE ..." in the field names of tests/golden/prove_plan.json.  Build + run: tests/test_prove_plan_cpu.py
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "sc.h"              // sc, FE_NL

using namespace dapol;

// The layout constants the plan sizes its scratch with, as in tables.h / kernels_range.h / kernels_range_gs.h (HIP headers: not
// includable here).
typedef int32_t dig_t;
struct ProofState { unsigned char bytes[760]; };
enum { TAIL_WBITS = 5, TAIL_NWIN = 253 / TAIL_WBITS + 1, TAIL_ENTRIES = (1 << (TAIL_WBITS - 1)) + 1, TAIL_ROW_WORDS = TAIL_ENTRIES * 32 };
enum { STAB_ROUNDS = 6, STAB_N = 1 << STAB_ROUNDS };
enum { MAT_GROUP = 16 };
enum { GS_ACC_SLOTS = 32, GS_MAX_SLICES = 16, GS_FULL_LANES = 3072 * 64 };

static const char* knob(const char* name) { return getenv(name); }

#include "prove_plan.inc"

static void print_chunk(const ProvePlan& P, const char* which, size_t cb) {
    int ns = 0, tile = 0, cpl = 0, a_lane = 0;
    if (cb && P.gs) { ns = P.slices_for(cb); tile = P.tile_for(cb, ns); }
    if (cb && P.gs_mat) cpl = P.mat_cpl(cb);
    if (cb) a_lane = P.a_lane(cb);
    printf(" %s_cb=%zu %s_slices=%d %s_tile=%d %s_cpl=%d %s_a_lane=%d", which, cb, which, ns, which, tile, which, cpl, which, a_lane);
}

int main() {
    char buf[4096];
    while (fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string tok;
        std::vector<std::string> env;
        ProveShape s{};
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "bad token %s\n", tok.c_str()); return 2; }
            const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
            const long long x = atoll(v.c_str());
            if (k.rfind("DAPOL_", 0) == 0) { setenv(k.c_str(), v.c_str(), 1); env.push_back(k); }
            else if (k == "n") s.n = (int)x;
            else if (k == "m") s.m = (int)x;
            else if (k == "B") s.B = (size_t)x;
            else if (k == "opt_tail_length") s.tail_length = (int)x;
            else if (k == "opt_small_call_max") s.small_call_max = (int)x;
            else if (k == "opt_generator_stationary") s.generator_stationary = (int)x;
            else if (k == "opt_streams") s.streams = (int)x;
            else if (k == "opt_chunk_proofs") s.chunk_proofs = x;
            else if (k == "opt_gs_tile_rows") s.gs_tile_rows = (int)x;
            else if (k == "opt_gs_slices") s.gs_slices = (int)x;
            else if (k == "wbits") s.wbits = (int)x;
            else if (k == "nwin") s.nwin = (int)x;
            else if (k == "hi_split") s.hi_split = (int)x;
            else if (k == "n_cu") s.n_cu = (int)x;
            else if (k == "resident_waves") s.resident_waves = (size_t)x;
            else if (k == "budget_bytes") s.budget_bytes = (size_t)x;
            else if (k == "timed") s.timed = x != 0;
            else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
        }
        const ProvePlan P = plan_range_prove(s);
        for (auto& k : env) unsetenv(k.c_str());
        printf("tail_n=%d tail_lgn=%d small_call=%d use_hi=%d fs_shape=%d fs_parts=%d gs=%d gs_mat=%d gs_LW=%d acc_slots=%d stab_main=%d stab_tail=%d "
               "msm_split=%d mat_split=%d quad_split=%d per_proof=%zu split_bytes=%zu chunk=%zu nlanes=%d big_batch=%d lpl=%d tail_lpl=%d side_A=%d "
               "dig_elems=%zu stab_bytes=%zu acc_bytes=%zu",
               P.tail_n, P.tail_lgn, (int)P.small_call, (int)P.use_hi, P.fs_shape, P.fs_parts, (int)P.gs, (int)P.gs_mat, P.gs_LW, P.acc_slots, (int)P.stab_main,
               (int)P.stab_tail, P.msm_split, P.mat_split, P.quad_split, P.per_proof, P.split_bytes, P.chunk, P.nlanes, (int)P.big_batch, P.lpl, P.tail_lpl,
               (int)P.side_A, P.dig_elems, P.stab_bytes, P.acc_bytes);
        print_chunk(P, "full", P.chunk < s.B ? P.chunk : s.B);
        print_chunk(P, "last", s.B % P.chunk);
        printf("\n");
    }
    return 0;
}

// Host-only build of the range prover's planning (dapol_amd/csrc/prove_plan.inc), as tests/cpp/tail_order_plan_host.cpp, for the
// fields that decide which digit producers a call runs (DAPOL_PREP): reads rows "KEY=VALUE ..." from stdin -- fields of ProveShape,
// and DAPOL_* names, which are set in the environment for that row only -- and prints "KEY=VALUE ..." per row.
// Build + run: tests/test_prep_scalars_cpu.py, tests/test_gpu_prep_scalars.py
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
        printf("N=%d tail_n=%d gs=%d gs_mat=%d small_call=%d stab_main=%d stab_tail=%d prep_recode=%d prep_share=%d chunk=%zu nlanes=%d nwin=%d "
               "dig_elems=%zu stab_bytes=%zu acc_bytes=%zu acc_slots=%d per_proof=%zu lane_bytes=%zu lpl=%d tail_gs=%d\n",
               P.N, P.tail_n, (int)P.gs, (int)P.gs_mat, (int)P.small_call, (int)P.stab_main, (int)P.stab_tail, (int)P.prep_recode, (int)P.prep_share, P.chunk,
               P.nlanes, P.nwin, P.dig_elems, P.stab_bytes, P.acc_bytes, P.acc_slots, P.per_proof, P.lane_bytes(), P.lpl, (int)P.tail_gs);
    }
    return 0;
}

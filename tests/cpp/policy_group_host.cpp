// Host-only build of the policy grouping (dapol_amd/csrc/policy_plan.inc: group_policy_plan, which the prover and the verifier share):
// for both policies, every height 0..64, every aggregation factor 0..height, grouping on and off, one line
//   policy height agg group | sum_proofs sum_parties max_k max_parties | start,count,m,k ...
// Build + run: tests/test_policy_group_cpu.py
#include <cstdint>
#include <cstdio>

#include "../../include/dapol_hip.h"
#include "policy_plan.inc"

int main() {
    const int policies[2] = {DAPOL_POLICY_PADDING, DAPOL_POLICY_SPLITTING};
    for (int policy : policies)
        for (int H = 0; H <= 64; H++)
            for (int agg = 0; agg <= H; agg++)
                for (int group = 0; group < 2; group++) {
                    std::vector<SubProof> plan;
                    if (!policy_plan(policy, H, agg, plan)) { fprintf(stderr, "no plan for %d %d %d\n", policy, H, agg); return 2; }
                    const PolicyGroups G = group_policy_plan(plan, group != 0);
                    printf("%d %d %d %d | %zu %zu %zu %zu |", policy, H, agg, group, G.sum_proofs, G.sum_parties, G.max_k, G.max_parties);
                    for (auto& g : G.groups) printf(" %d,%d,%d,%d", g.start, g.count, g.m, g.k);
                    printf("\n");
                }
    return 0;
}

// Host-only build of the policy grouping and layout (dapol_amd/csrc/policy_plan.inc: group_policy_plan and policy_layout, which the
// prover and the verifier share): for both policies, every height 0..64, every aggregation factor 0..height, grouping on and off, one line
//   policy height agg group | sum_proofs sum_parties max_k max_parties | start,count,m,k ...
// and for the grouped plan, b in {1, 3}, n_bits in {8, 64} and both modes (reuse = 0 compact, 1 one group after the other) one line
//   L policy height agg b n_bits reuse | entity_words entity_bytes parties words proofs | proof_words,word_off,slot_base,party_off,gathered_word_off,verdict_off ...
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
                    if (!group) continue;
                    for (size_t b : {(size_t)1, (size_t)3})
                        for (int n_bits : {8, 64})
                            for (int reuse = 0; reuse < 2; reuse++) {
                                const PolicyLayout L = policy_layout(G, b, n_bits, reuse != 0);
                                if (L.g.size() != G.groups.size()) { fprintf(stderr, "layout of %zu groups for %zu\n", L.g.size(), G.groups.size()); return 3; }
                                printf("L %d %d %d %zu %d %d | %zu %zu %zu %zu %zu |", policy, H, agg, b, n_bits, reuse, L.entity_words,
                                       dapol_entity_proof_size(H, policy, agg, n_bits), L.parties, L.words, L.proofs);
                                for (auto& g : L.g)
                                    printf(" %zu,%zu,%llu,%zu,%zu,%zu", g.proof_words, g.word_off, (unsigned long long)g.slot_base, g.party_off, g.gathered_word_off,
                                           g.verdict_off);
                                printf("\n");
                            }
                }
    return 0;
}

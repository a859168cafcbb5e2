// Sizes and plans that are pure host arithmetic: which siblings go into which aggregated proof under the two policies, and the
// byte sizes that follow.  Shared by the library (host_policy.inc, host_entity.inc, host_wire.inc, host_verify.inc) and by the host-only
// builds that run under AddressSanitizer on the CPU (tests/cpp/wire_asan.cpp, tests/cpp/policy_group_host.cpp).
#pragma once
#include <algorithm>
#include <vector>

size_t dapol_range_proof_size(int32_t n_bits, int32_t m) {
    if (!(n_bits == 8 || n_bits == 16 || n_bits == 32 || n_bits == 64) || m < 1 || (m & (m - 1))) return 0;
    int lg = 0;
    while ((1 << lg) < n_bits * m) lg++;
    return (size_t)32 * (9 + 2 * lg);
}

// ---------------------------------------------------------------------------- policies (padding / splitting)
struct SubProof { int start, count, m; };
// src/range/padding.rs:88-118 and src/range/splitting.rs:100-129: which siblings go into which aggregated proof;
// siblings [agg, height) get individual proofs.
static bool policy_plan(int policy, int n_siblings, int agg, std::vector<SubProof>& plan) {
    plan.clear();
    if (agg < 0 || agg > n_siblings) return false;          // the reference indexes out of bounds and panics
    if (n_siblings > (1 << 24)) return false;               // (far beyond any tree: keeps the power-of-two arithmetic below in range)
    auto np2 = [](int x) { int p = 1; while (p < x) p <<= 1; return p; };
    if (policy == DAPOL_POLICY_PADDING) {
        plan.push_back({0, agg, np2(agg)});                 // agg == 0 -> one proof over a single (0, 1) pad party
    } else if (policy == DAPOL_POLICY_SPLITTING) {
        int base = np2(agg), pos = 0;
        while (pos < agg) {
            if (agg & base) { plan.push_back({pos, base, base}); pos += base; }
            base >>= 1;
        }
    } else return false;
    for (int i = agg; i < n_siblings; i++) plan.push_back({i, 1, 1});
    return true;
}

// A run of the plan's equal-sized FULL sub-proofs (the individual proofs beyond aggregation_factor, with the one-party part of an odd
// split before them) is ONE group of k proofs per entity: the prover proves it in one call, the verifier checks it in one batch, and
// the two must agree on it.  group = false: every sub-proof is a group of its own (DAPOL_NO_GROUP).
struct PolicyGroup { int start, count, m, k; };
struct PolicyGroups {
    std::vector<PolicyGroup> groups;
    size_t sum_proofs = 0, sum_parties = 0;                 // sub-proofs and parties per entity, over all groups
    size_t max_k = 1, max_parties = 1;                      // most sub-proofs / most parties (k * m) of one group
};
static PolicyGroups group_policy_plan(const std::vector<SubProof>& plan, bool group) {
    PolicyGroups G;
    for (auto& s : plan) {
        if (group && !G.groups.empty() && G.groups.back().m == s.m && G.groups.back().count == s.m && s.count == s.m &&
            G.groups.back().start + G.groups.back().k * s.m == s.start) G.groups.back().k++;
        else G.groups.push_back({s.start, s.count, s.m, 1});
    }
    for (auto& g : G.groups) {
        const size_t k = (size_t)g.k, parties = k * (size_t)g.m;
        G.sum_proofs += k; G.sum_parties += parties;
        if (k > G.max_k) G.max_k = k;
        if (parties > G.max_parties) G.max_parties = parties;
    }
    return G;
}

// Where the groups of a call of b entities live (prove_policy_device, host_policy.inc; verify_policy_device, host_verify.inc).  Per group:
// its first word inside an entity's blob and first RNG slot inside an entity's draws (one RNG stream runs across an entity's sub-proofs),
// and its place in the call's GATHERED arrays -- parties / commitments [b * k][m], the verifier's proof words and verdicts [b * k].
// reuse = false (every group in flight at once, on lanes): the places are running sums and the sizes the totals.
// reuse = true (one group after the other through the same buffers): the places are 0 and the sizes those of the largest group.
struct PolicyLayout {
    struct Group {
        size_t proof_words;                                 // words of one sub-proof of the group
        size_t word_off;                                    // inside an entity's blob
        uint64_t slot_base;                                 // inside an entity's draws
        size_t party_off, gathered_word_off, verdict_off;   // inside the gathered arrays
    };
    std::vector<Group> g;
    size_t entity_words = 0;                                // one entity's blob: dapol_entity_proof_size / 4
    size_t parties = 0, words = 0, proofs = 0;              // sizes of the gathered arrays
};
static PolicyLayout policy_layout(const PolicyGroups& PG, size_t b, int n_bits, bool reuse) {
    PolicyLayout L;
    uint64_t slot = 0;
    for (auto& pg : PG.groups) {
        const size_t pw = dapol_range_proof_size(n_bits, pg.m) / 4, np = b * (size_t)pg.k;
        L.g.push_back({pw, L.entity_words, slot, reuse ? 0 : L.parties, reuse ? 0 : L.words, reuse ? 0 : L.proofs});
        L.entity_words += pw * (size_t)pg.k;
        slot += (uint64_t)pg.k * (uint64_t)pg.m * (2 * (uint64_t)n_bits + 4);
        if (reuse) { L.parties = std::max(L.parties, np * (size_t)pg.m); L.words = std::max(L.words, np * pw); L.proofs = std::max(L.proofs, np); }
        else { L.parties += np * (size_t)pg.m; L.words += np * pw; L.proofs += np; }
    }
    return L;
}

size_t dapol_entity_proof_size(int32_t height, int32_t policy, int32_t aggregation_factor, int32_t n_bits) {
    std::vector<SubProof> plan;
    if (!policy_plan(policy, height, aggregation_factor, plan)) return 0;
    size_t tot = 0;
    for (auto& s : plan) tot += dapol_range_proof_size(n_bits, s.m);
    return tot;
}

// Host-only build of the index arithmetic of dapol_reprove_plan / dapol_reprove_entities_shared (dapol_amd/csrc/reprove_plan.inc) with
// its own main, run directly under ASan + UBSan: reads one case per line from stdin and prints what the library computes for it as one
// line of JSON.  Build + run: tests/test_reprove_plan_cpu.py.  A case (numbers in decimal):
//   plan H leaf_first policy agg b idx[b] has(0 = NULL, 1 = given) [has_old[b]] k edited[k]
//        -> {"ok", "n_proved": [...], "total", "sum_m", "sum_m_shared"}       ("ok": 0 = bad plan, -1 = bad indexes)
//   layout n_groups b base[n_groups + 1] s0[n_groups] m[n_groups] pieces[n_groups]
//        -> {"U", "party_off", "word_off", "parties", "words", "heads", "base_at"}
// The index arrays go into heap buffers of exactly their size, so that a read outside them is a sanitizer error.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/dapol_hip.h"
#include "reprove_plan.inc"

template <typename V>
static void put(const char* key, const V& v, const char* end = ", ") {
    printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); i++) printf("%s%llu", i ? ", " : "", (unsigned long long)v[i]);
    printf("]%s", end);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string word;
        in >> word;
        if (word == "layout") {
            uint32_t ng = 0;
            size_t b = 0;
            in >> ng >> b;
            if (!in || ng > REPROVE_MAX_GROUPS) { fprintf(stderr, "bad layout case\n"); return 2; }
            std::vector<uint32_t> base(ng + 1), s0(ng), m(ng), pieces(ng);
            for (auto& x : base) in >> x;
            for (auto& x : s0) in >> x;
            for (auto& x : m) in >> x;
            for (auto& x : pieces) in >> x;
            if (!in) { fprintf(stderr, "short layout case\n"); return 2; }
            ReproveLayout L;
            reprove_layout(ng, base.data(), m.data(), pieces.data(), L);
            std::vector<size_t> U(L.U, L.U + ng), po(L.party_off, L.party_off + ng), wo(L.word_off, L.word_off + ng), at;
            for (uint32_t g = 0; g < ng; g++) at.push_back(reprove_base_at(s0[g], b) + 1);      // (+ 1: "none before it" prints as 0)
            printf("{");
            put("U", U); put("party_off", po); put("word_off", wo); put("base_at", at);
            printf("\"parties\": %zu, \"words\": %zu, \"heads\": %zu, \"row\": %zu}\n", L.parties, L.words, L.heads,
                   ng ? reprove_group_row(base[ng] + 1, base[ng - 1]) : (size_t)0);
            continue;
        }
        if (word != "plan") { fprintf(stderr, "unknown case\n"); return 2; }
        int H = 0, leaf_first = 0, policy = 0, agg = 0, has = 0;
        size_t b = 0, k = 0;
        in >> H >> leaf_first >> policy >> agg >> b;
        uint64_t* idx = new uint64_t[b];
        for (size_t i = 0; i < b; i++) in >> idx[i];
        in >> has;
        uint8_t* has_old = has ? new uint8_t[b] : nullptr;
        for (size_t i = 0; has && i < b; i++) { unsigned v = 0; in >> v; has_old[i] = (uint8_t)v; }
        in >> k;
        uint64_t* edited = new uint64_t[k];
        for (size_t i = 0; i < k; i++) in >> edited[i];
        if (!in) { fprintf(stderr, "short plan case\n"); return 2; }
        std::vector<SubProof> plan;
        if (H < 0 || H > 64 || !policy_plan(policy, H, agg, plan)) printf("{\"ok\": 0}\n");
        else {
            std::vector<uint64_t> n_proved(plan.size(), 0);
            ReprovePlanOut out;
            if (!reprove_plan_host(plan, H, leaf_first != 0, b, idx, has_old, k, edited, n_proved.data(), out)) printf("{\"ok\": -1}\n");
            else {
                printf("{\"ok\": 1, ");
                put("n_proved", n_proved);
                printf("\"total\": %llu, \"sum_m\": %llu, \"sum_m_shared\": %llu}\n", (unsigned long long)out.total_proved, (unsigned long long)out.sum_m_proved,
                       (unsigned long long)out.sum_m_shared);
            }
        }
        delete[] idx;
        delete[] has_old;
        delete[] edited;
    }
    return 0;
}

// Host-only build of the index arithmetic of dapol_reprove_batches_plan / dapol_reprove_batches (dapol_amd/csrc/reprove_batches_plan.inc)
// with its own main, run directly under ASan + UBSan: reads one case per line from stdin and prints what the library computes for it
// as one line of JSON.  Build + run: tests/test_reprove_batches_host_asan.py.  A case (numbers in decimal):
//   plan height policy agg nb { has_old S level[S] index[S] }[nb] k edited[k]      (agg is the same for every batch, S its own)
//        -> {"ok", "n_proved": [nb], "total", "sum_m", "sum_m_all"}       ("ok": 0 = a bad plan, -1 = bad edited indexes)
//   entries policy S agg n_bits n_classes class_m[n_classes]
//        -> {"start", "count", "m", "cls", "slot", "piece0", "pieces"}      (one element per sub-proof)
//   layout n_pairs n_classes m[n_classes] pieces[n_classes] before[n_classes + 1]
//        -> {"party_off", "piece_off", "base_at", "flag_at", "parties", "proof_pieces"}
// Every array goes into a heap buffer of exactly its size, so that a read outside it is a sanitizer error.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/dapol_hip.h"
#include "reprove_batches_plan.inc"

struct Sib { int level; uint64_t index; };

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
        if (word == "entries") {
            int policy = 0, S = 0, agg = 0, n_bits = 0;
            size_t nc = 0;
            in >> policy >> S >> agg >> n_bits >> nc;
            std::vector<uint32_t> class_m(nc);
            for (auto& x : class_m) in >> x;
            std::vector<SubProof> plan;
            if (!in || !policy_plan(policy, S, agg, plan)) { fprintf(stderr, "bad entries case\n"); return 2; }
            std::vector<ReproveBatchesEntry> tab;
            reprove_batches_entries(plan, n_bits, class_m, tab);
            std::vector<uint64_t> start, count, m, cls, slot, piece0, pieces;
            for (auto& e : tab) {
                start.push_back(e.start); count.push_back(e.count); m.push_back(e.m); cls.push_back(e.cls); slot.push_back(e.slot);
                piece0.push_back(e.piece0); pieces.push_back(e.pieces);
            }
            printf("{");
            put("start", start); put("count", count); put("m", m); put("cls", cls); put("slot", slot); put("piece0", piece0); put("pieces", pieces, "}\n");
            continue;
        }
        if (word == "layout") {
            size_t n_pairs = 0;
            ReproveBatchesClasses K{};
            in >> n_pairs >> K.n;
            if (!in || K.n > REPROVE_BATCHES_MAX_CLASSES) { fprintf(stderr, "bad layout case\n"); return 2; }
            for (uint32_t c = 0; c < K.n; c++) in >> K.m[c];
            for (uint32_t c = 0; c < K.n; c++) in >> K.pieces[c];
            for (uint32_t c = 0; c <= K.n; c++) in >> K.before[c];
            if (!in) { fprintf(stderr, "short layout case\n"); return 2; }
            reprove_batches_layout(K);
            std::vector<uint64_t> po(K.party_off, K.party_off + K.n), qo(K.piece_off, K.piece_off + K.n), at, fl;
            for (uint32_t c = 0; c < K.n; c++) {
                at.push_back(reprove_batches_base_at(c, n_pairs) + 1);      // (+ 1: "none before it" prints as 0)
                fl.push_back(reprove_batches_flag_at(c, n_pairs, n_pairs ? n_pairs - 1 : 0));
            }
            printf("{");
            put("party_off", po); put("piece_off", qo); put("base_at", at); put("flag_at", fl);
            printf("\"parties\": %llu, \"proof_pieces\": %llu}\n", (unsigned long long)K.parties, (unsigned long long)K.proof_pieces);
            continue;
        }
        if (word != "plan") { fprintf(stderr, "unknown case\n"); return 2; }
        int height = 0, policy = 0, agg = 0;
        size_t nb = 0, k = 0;
        in >> height >> policy >> agg >> nb;
        std::vector<unsigned> has_old(nb);
        std::vector<Sib*> sibs(nb, nullptr);
        std::vector<size_t> S(nb, 0);
        for (size_t j = 0; j < nb; j++) {
            in >> has_old[j] >> S[j];
            if (!in || S[j] > (1u << 20)) { fprintf(stderr, "bad plan case\n"); return 2; }
            sibs[j] = new Sib[S[j]];
            for (size_t i = 0; i < S[j]; i++) in >> sibs[j][i].level;
            for (size_t i = 0; i < S[j]; i++) in >> sibs[j][i].index;
        }
        in >> k;
        uint64_t* edited = new uint64_t[k];
        for (size_t i = 0; i < k; i++) in >> edited[i];
        if (!in) { fprintf(stderr, "short plan case\n"); return 2; }
        ReproveBatchesPlanOut out;
        std::vector<uint64_t> n_proved;
        int ok = reprove_batches_increasing_below(height, k, edited) ? 1 : -1;
        for (size_t j = 0; ok == 1 && j < nb; j++) {
            std::vector<SubProof> plan;
            if (!policy_plan(policy, (int)S[j], agg, plan)) { ok = 0; break; }
            n_proved.push_back(reprove_batches_plan_batch(plan, sibs[j], has_old[j] != 0, k, edited, out));
        }
        if (ok != 1) printf("{\"ok\": %d}\n", ok);
        else {
            printf("{\"ok\": 1, ");
            put("n_proved", n_proved);
            printf("\"total\": %llu, \"sum_m\": %llu, \"sum_m_all\": %llu}\n", (unsigned long long)out.total_proved, (unsigned long long)out.sum_m_proved,
                   (unsigned long long)out.sum_m_all);
        }
        for (auto p : sibs) delete[] p;
        delete[] edited;
    }
    return 0;
}

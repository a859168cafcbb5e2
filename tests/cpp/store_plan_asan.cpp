// Host-only build of the index arithmetic of dapol_proof_store (dapol_amd/csrc/store_plan.inc) with its own main, run directly under
// ASan + UBSan: reads one case per line from stdin and prints what the library computes for it as one line of JSON.  Build + run:
// tests/test_store_plan_cpu.py.  A case (numbers in decimal):
//   align n_old old[n_old] b new[b]
//        -> {"src": [...] (old row + 1, 0 = none), "has_old": [...], "with_old", "same", "lower": [...] (store_lower_bound of every new index)}
//   bytes rows H hash_bytes entity_bytes entity_pieces hash_words
//        -> {"idx", "path_C", "path_H", "range", "resident", "move_transient", "row_pieces"}
// The index arrays go into heap buffers of exactly their size, so that a read outside them is a sanitizer error.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "store_plan.inc"

template <typename T>
static void put(const char* key, const T* v, size_t n, const char* end = ", ") {
    printf("\"%s\": [", key);
    for (size_t i = 0; i < n; i++) printf("%s%llu", i ? ", " : "", (unsigned long long)v[i]);
    printf("]%s", end);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string word;
        in >> word;
        if (word == "bytes") {
            size_t rows = 0, hb = 0, es = 0, ep = 0;
            int H = 0, hw = 0;
            in >> rows >> H >> hb >> es >> ep >> hw;
            if (!in) { fprintf(stderr, "short bytes case\n"); return 2; }
            const StoreBytes B = store_bytes(rows, H, hb, es);
            printf("{\"idx\": %zu, \"path_C\": %zu, \"path_H\": %zu, \"range\": %zu, \"resident\": %zu, \"move_transient\": %zu, \"row_pieces\": %zu}\n", B.idx,
                   B.path_C, B.path_H, B.range, B.resident(), B.move_transient(), store_row_pieces(ep, H, hw));
            continue;
        }
        if (word != "align") { fprintf(stderr, "unknown case\n"); return 2; }
        size_t n_old = 0, b = 0;
        in >> n_old;
        uint64_t* old_idx = new uint64_t[n_old];
        for (size_t i = 0; i < n_old; i++) in >> old_idx[i];
        in >> b;
        uint64_t* new_idx = new uint64_t[b];
        for (size_t i = 0; i < b; i++) in >> new_idx[i];
        if (!in) { fprintf(stderr, "short align case\n"); return 2; }
        uint32_t* src = new uint32_t[b];
        uint8_t* has_old = new uint8_t[b];
        const size_t with_old = store_align_host(n_old, old_idx, b, new_idx, src, has_old);
        if (with_old != store_align_host(n_old, old_idx, b, new_idx, nullptr, nullptr)) { fprintf(stderr, "the count depends on the output pointers\n"); return 3; }
        std::vector<uint64_t> src1(b), lower(b);
        for (size_t e = 0; e < b; e++) {
            src1[e] = src[e] == STORE_NONE ? 0 : (uint64_t)src[e] + 1;
            lower[e] = store_lower_bound(old_idx, n_old, new_idx[e]);
        }
        printf("{");
        put("src", src1.data(), b); put("has_old", has_old, b); put("lower", lower.data(), b);
        printf("\"with_old\": %zu, \"same\": %d}\n", with_old, store_same_leaf_set(n_old, b, with_old) ? 1 : 0);
        delete[] old_idx;
        delete[] new_idx;
        delete[] src;
        delete[] has_old;
    }
    return 0;
}

// Host-only build of the index arithmetic of dapol_batch_store (dapol_amd/csrc/batch_store_plan.inc) with its own main, run directly
// under ASan + UBSan: reads one case per line from stdin and prints what the library computes for it as one line of JSON.  Build + run:
// tests/test_batch_store_plan_cpu.py.  A case (numbers in decimal; a list is its length followed by its elements):
//   match old_off[] old_leaf[] new_off[] new_leaf[]          (the offset lists have rows + 1 elements)
//        -> {"src": [...] (old row + 1, 0 = none), "has_old": [...], "with_old", "same"}
//   fetch sib_off[] range_off[] row[]
//        -> {"ok", "q_sib_off": [...], "q_piece_off": [...]}   (the offsets only when ok)
//   pieces unit dst_off[] from[] (old row + 1, 0 = none) src_off[]
//        -> {"src": [...]}  batch_store_piece_src of every piece of the destination (source piece + 1, 0 = not written)
// The arrays go into heap buffers of exactly their size, so that a read outside them is a sanitizer error.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "batch_store_plan.inc"

struct List {
    size_t n = 0;
    uint64_t* p = nullptr;
    explicit List(std::istream& in) {
        in >> n;
        p = new uint64_t[n];
        for (size_t i = 0; i < n; i++) in >> p[i];
    }
    List(const List&) = delete;
    ~List() { delete[] p; }
};

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
        if (word == "match") {
            List old_off(in), old_leaf(in), new_off(in), new_leaf(in);
            if (!in || !old_off.n || !new_off.n) { fprintf(stderr, "short match case\n"); return 2; }
            const size_t n_old = old_off.n - 1, nb = new_off.n - 1;
            uint32_t* src = new uint32_t[nb];
            uint8_t* has_old = new uint8_t[nb];
            const size_t with_old = batch_store_match(n_old, old_off.p, old_leaf.p, nb, new_off.p, new_leaf.p, src, has_old);
            if (with_old != batch_store_match(n_old, old_off.p, old_leaf.p, nb, new_off.p, new_leaf.p, nullptr, nullptr)) {
                fprintf(stderr, "the count depends on the output pointers\n");
                return 3;
            }
            std::vector<uint64_t> src1(nb);
            for (size_t j = 0; j < nb; j++) src1[j] = src[j] == BATCH_STORE_NONE ? 0 : (uint64_t)src[j] + 1;
            printf("{");
            put("src", src1.data(), nb); put("has_old", has_old, nb);
            printf("\"with_old\": %zu, \"same\": %d}\n", with_old, batch_store_same_list(n_old, old_off.p, old_leaf.p, nb, new_off.p, new_leaf.p) ? 1 : 0);
            delete[] src;
            delete[] has_old;
        } else if (word == "fetch") {
            List sib_off(in), range_off(in), row(in);
            if (!in || !sib_off.n || sib_off.n != range_off.n) { fprintf(stderr, "short fetch case\n"); return 2; }
            uint64_t *qs = new uint64_t[row.n + 1], *qp = new uint64_t[row.n + 1];
            const bool ok = batch_store_fetch_offsets(row.n, row.p, sib_off.n - 1, sib_off.p, range_off.p, qs, qp);
            printf("{");
            if (ok) { put("q_sib_off", qs, row.n + 1); put("q_piece_off", qp, row.n + 1); }
            printf("\"ok\": %d}\n", ok ? 1 : 0);
            delete[] qs;
            delete[] qp;
        } else if (word == "pieces") {
            uint32_t unit = 0;
            in >> unit;
            List dst_off(in), from1(in), src_off(in);
            if (!in || !unit || dst_off.n != from1.n + 1 || !src_off.n) { fprintf(stderr, "short pieces case\n"); return 2; }
            const size_t rows = from1.n, n = (size_t)dst_off.p[rows] * unit;
            uint32_t* from = new uint32_t[rows];
            for (size_t d = 0; d < rows; d++) from[d] = from1.p[d] ? (uint32_t)(from1.p[d] - 1) : (uint32_t)BATCH_STORE_NONE;
            std::vector<uint64_t> src(n);
            for (size_t t = 0; t < n; t++) {
                const size_t s = batch_store_piece_src(t, unit, rows, dst_off.p, from, src_off.p);
                src[t] = s == (size_t)-1 ? 0 : (uint64_t)s + 1;
            }
            printf("{");
            put("src", src.data(), n, "}\n");
            delete[] from;
        } else {
            fprintf(stderr, "unknown case\n");
            return 2;
        }
    }
    return 0;
}

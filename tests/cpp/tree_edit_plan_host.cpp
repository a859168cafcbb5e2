// Host-only build of the tree edit planning (dapol_amd/csrc/tree_edit_plan.inc): reads one case per line from stdin and prints the
// plan of each as one line of JSON.  Build + run: tests/test_tree_edit_plan_cpu.py.  Cases (numbers in decimal, S1 = H + 1):
//   remove H k si[k] pos[k * S1] has_pad[k * S1]       what k_tree_find_paths returns     -> RemovePlan
//   insert H k m[k] inspos[k * S1]                      what k_tree_ins_plan<true> returns -> InsertPlan
//   merge n0 idx[n0] v[n0] k idx[k] removing [v[k]]     a leaf set and k edits             -> merge_leaf_edits
//   slw k idx[k]                                                                           -> sorted_last_wins
//   pad H n idx[n]                                                                         -> padding_positions
// merge: the blinding of a record is derived from its value (byte j = value + j), so the test sees that v and r travel together.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tree_edit_plan.inc"

template <typename V>
static void put(const char* key, const V& v, const char* end = ", ") {
    printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); i++) printf("%s%llu", i ? ", " : "", (unsigned long long)v[i]);
    printf("]%s", end);
}
template <typename V>
static void put_lists(const char* key, const std::vector<V>& v) {
    printf("\"%s\": [", key);
    for (size_t t = 0; t < v.size(); t++) {
        printf("%s[", t ? ", " : "");
        for (size_t i = 0; i < v[t].size(); i++) printf("%s%llu", i ? ", " : "", (unsigned long long)v[t][i]);
        printf("]");
    }
    printf("], ");
}
template <typename T>
static std::vector<T> get(std::istream& in, size_t n) {
    std::vector<T> v(n);
    for (size_t i = 0; i < n; i++) { unsigned long long x = 0; in >> x; v[i] = (T)x; }
    return v;
}
static void blinding(uint64_t value, uint8_t* r32) { for (int j = 0; j < 32; j++) r32[j] = (uint8_t)(value + j); }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        int H = 0;
        size_t k = 0;
        if (what == "remove") {
            in >> H >> k;
            const size_t S1 = (size_t)H + 1;
            const auto si = get<uint64_t>(in, k);
            const auto pos = get<uint32_t>(in, k * S1);
            const auto hp = get<uint8_t>(in, k * S1);
            const RemovePlan P = plan_remove(H, k, si.data(), pos.data(), hp.data());
            printf("{\"ok\": %d, \"D\": %d, ", (int)P.ok, P.D);
            put_lists("dead", P.dead);
            put_lists("merge", P.merge);
            put("pad_pos", P.pad_pos); put("pad_lvl", P.pad_lvl); put("flat", P.flat); put("dead_off", P.dead_off); put("merge_off", P.merge_off);
            printf("\"pad_off\": %zu}\n", P.pad_off);
        } else if (what == "insert") {
            in >> H >> k;
            const auto m = get<uint32_t>(in, k);
            const auto ins = get<uint32_t>(in, k * ((size_t)H + 1));
            const InsertPlan P = plan_insert(k, H, m.data(), ins.data());
            printf("{\"max_m\": %d, ", P.max_m);
            put("newpos", P.newpos); put("lvl_flat", P.lvl_flat); put("lvl_off", P.lvl_off, "}\n");
        } else if (what == "merge") {
            size_t n0 = 0;
            int removing = 0;
            HostLeaves old, out;
            in >> n0;
            old.idx = get<uint64_t>(in, n0);
            old.v = get<uint64_t>(in, n0);
            old.r.resize(n0 * 32);
            for (size_t i = 0; i < n0; i++) blinding(old.v[i], old.r.data() + i * 32);
            in >> k;
            const auto idx = get<uint64_t>(in, k);
            in >> removing;
            const auto v = get<uint64_t>(in, removing ? 0 : k);
            std::vector<uint8_t> r(v.size() * 32);
            for (size_t i = 0; i < v.size(); i++) blinding(v[i], r.data() + i * 32);
            merge_leaf_edits(old, k, idx.data(), removing ? nullptr : v.data(), removing ? nullptr : r.data(), out);
            printf("{");
            put("idx", out.idx); put("v", out.v); put("r", out.r, "}\n");
        } else if (what == "slw") {
            in >> k;
            const auto idx = get<uint64_t>(in, k);
            printf("{");
            put("keep", sorted_last_wins(k, idx.data()), "}\n");
        } else if (what == "pad") {
            in >> H >> k;
            const auto idx = get<uint64_t>(in, k);
            const size_t count = padding_positions(H, k, idx.data(), nullptr, nullptr);
            std::vector<uint8_t> level(count);
            std::vector<uint64_t> index(count);
            const size_t again = padding_positions(H, k, idx.data(), level.data(), index.data());
            printf("{\"count\": %zu, \"again\": %zu, ", count, again);
            put("level", level); put("index", index, "}\n");
        } else { fprintf(stderr, "unknown case %s\n", what.c_str()); return 2; }
        if (!in) { fprintf(stderr, "short case: %s\n", line.c_str()); return 2; }
    }
    return 0;
}

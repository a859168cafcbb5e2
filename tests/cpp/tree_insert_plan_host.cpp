// Host-only build of the general insert's planning (dapol_amd/csrc/tree_edit_plan.inc, plan_insert_general): reads one case per line
// from stdin and prints its plan as one line of JSON.  Build + run: tests/test_tree_insert_plan_cpu.py.  A case (numbers in decimal,
// S1 = H + 1) is what k_tree_ins_plan<false> returns for a sorted batch:
//   H k x[k] m[k] pos_all[k * S1]
#include <cstdint>
#include <cstdio>
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
static void put_lists(const char* key, const std::vector<std::vector<uint32_t>>& v) {
    printf("\"%s\": [", key);
    for (size_t t = 0; t < v.size(); t++) {
        printf("%s[", t ? ", " : "");
        for (size_t i = 0; i < v[t].size(); i++) printf("%s%u", i ? ", " : "", v[t][i]);
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

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int H = 0;
        size_t k = 0;
        in >> H >> k;
        const auto x = get<uint64_t>(in, k);
        const auto m = get<uint32_t>(in, k);
        const auto pos = get<uint32_t>(in, k * ((size_t)H + 1));
        if (!in) { fprintf(stderr, "short case: %s\n", line.c_str()); return 2; }
        const InsertGeneralPlan P = plan_insert_general(H, k, x.data(), m.data(), pos.data());
        printf("{\"D\": %d, \"max_fresh\": %u, ", P.D, P.max_fresh);
        put_lists("gain", P.gain);
        put_lists("merge", P.merge);
        put("n_lvl", P.n_lvl); put("n_pos", P.n_pos); put("n_parent", P.n_parent); put("n_sib", P.n_sib); put("n_idx", P.n_idx); put("n_has_pad", P.n_has_pad);
        put("leaf_pos", P.leaf_pos); put("pad_lvl", P.pad_lvl); put("pad_pos", P.pad_pos); put("flat", P.flat); put("gain_off", P.gain_off);
        put("merge_off", P.merge_off);
        const std::vector<size_t> offs = {P.lvl_off, P.pos_off, P.parent_off, P.sib_off, P.idx_lo_off, P.idx_hi_off, P.leaf_off, P.pad_lvl_off, P.pad_pos_off};
        put("offs", offs, "}\n");
    }
    return 0;
}

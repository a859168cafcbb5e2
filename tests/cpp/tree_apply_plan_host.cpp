// Host-only build of the mixed edit's planning (dapol_amd/csrc/tree_edit_plan.inc, plan_apply): reads one case per line from stdin and
// prints its plan as one line of JSON.  Build + run: tests/test_tree_apply_plan_cpu.py.  A case (numbers in decimal, S1 = H + 1) is what
// k_tree_apply_plan returns for the sorted union of the edited indexes:
//   H k x[k] is_put[k] lb[k * S1] fl[k * S1]
// A batch of removals only is also planned by plan_remove ("remove": ...), one of new puts only by plan_insert_general ("insert": ...),
// from the same rows, for the test to compare positions where the shapes coincide.
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
static void put_lists(const char* key, const std::vector<std::vector<uint32_t>>& v, const char* end = ", ") {
    printf("\"%s\": [", key);
    for (size_t t = 0; t < v.size(); t++) {
        printf("%s[", t ? ", " : "");
        for (size_t i = 0; i < v[t].size(); i++) printf("%s%u", i ? ", " : "", v[t][i]);
        printf("]");
    }
    printf("]%s", end);
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
        const size_t S1 = (size_t)H + 1;
        const auto x = get<uint64_t>(in, k);
        const auto is_put = get<uint8_t>(in, k);
        const auto lb = get<uint32_t>(in, k * S1);
        const auto fl = get<uint8_t>(in, k * S1);
        if (!in) { fprintf(stderr, "short case: %s\n", line.c_str()); return 2; }
        const ApplyPlan P = plan_apply(H, k, x.data(), is_put.data(), lb.data(), fl.data());
        printf("{\"ok\": %d, \"D\": %d, \"max_slots\": %u, ", (int)P.ok, P.D, P.max_slots);
        put_lists("dead", P.dead); put_lists("born", P.born); put_lists("merge", P.merge);
        put("s_lvl", P.s_lvl); put("s_pos", P.s_pos); put("s_parent", P.s_parent); put("s_flag", P.s_flag); put("s_idx", P.s_idx);
        put("put_pos", P.put_pos); put("put_new", P.put_new); put("pad_lvl", P.pad_lvl); put("pad_pos", P.pad_pos);
        put("flat", P.flat); put("dead_off", P.dead_off); put("born_off", P.born_off); put("merge_off", P.merge_off);
        size_t n_put = 0, n_new = 0;
        for (size_t j = 0; j < k; j++) { n_put += is_put[j]; n_new += is_put[j] && !(fl[j * S1] & 1); }
        if (n_put == 0) {                                   // removals only: plan_remove from the same rows
            std::vector<uint8_t> hp(k * S1);
            for (size_t i = 0; i < hp.size(); i++) hp[i] = (fl[i] >> 1) & 1;
            const RemovePlan R = plan_remove(H, k, x.data(), lb.data(), hp.data());
            printf("\"remove\": {\"ok\": %d, ", (int)R.ok);
            put_lists("dead", R.dead); put_lists("merge", R.merge);
            put("pad_lvl", R.pad_lvl); put("pad_pos", R.pad_pos, "}, ");
        }
        if (n_new == k) {                                   // new puts only: plan_insert_general from the same rows
            std::vector<uint32_t> m(k);
            for (size_t j = 0; j < k; j++) { m[j] = 0; while (!(fl[j * S1 + m[j]] & 1)) m[j]++; }
            const InsertGeneralPlan G = plan_insert_general(H, k, x.data(), m.data(), lb.data());
            printf("\"insert\": {");
            put_lists("gain", G.gain); put_lists("merge", G.merge);
            put("n_lvl", G.n_lvl); put("n_pos", G.n_pos); put("n_parent", G.n_parent); put("leaf_pos", G.leaf_pos);
            put("pad_lvl", G.pad_lvl); put("pad_pos", G.pad_pos, "}, ");
        }
        const std::vector<size_t> offs = {P.lvl_off, P.pos_off, P.parent_off, P.flag_off, P.idx_lo_off, P.idx_hi_off, P.put_off, P.pad_lvl_off, P.pad_pos_off};
        put("offs", offs, "}\n");
    }
    return 0;
}

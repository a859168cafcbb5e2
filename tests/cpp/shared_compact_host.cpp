// Host-only build of the index arithmetic of the compact form of shared proofs (dapol_amd/csrc/shared_compact_plan.inc): reads one
// case per line from stdin and prints what the library computes for it as one line of JSON.  Build + run:
// tests/test_shared_compact_cpu.py, under ASan + UBSan.  A case (numbers in decimal, bytes in hex without separators, "-" for none):
//   policy H agg n_bits leaf_first b idx[b] commitments[b * H * 32] first count
// Output: the key shifts, sub_off, ref, the length; the key flags and the head flags of the verifier (the whole span at once, and as
// the OR over 16 strided lanes as k_vcompact_heads takes it); the expansion of rows [first, first + count) of a compact buffer whose
// byte i is pattern(i), and whether compress(expand(all rows)) gives that buffer back.  Every buffer lives on the heap with exactly
// its size, so that a read or write outside it is a sanitizer error.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/dapol_hip.h"
#include "shared_compact_plan.inc"

static uint8_t pattern(uint64_t i) { return (uint8_t)(i * 131 + (i >> 8) * 7 + (i >> 16) + 3); }
static bool unhex(const std::string& h, size_t bytes, uint8_t* o) {
    if (h.size() != 2 * bytes && !(bytes == 0 && h == "-")) return false;
    auto nib = [](char c) { return c >= '0' && c <= '9' ? c - '0' : (c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1); };
    for (size_t i = 0; i < bytes; i++) {
        const int hi = nib(h[2 * i]), lo = nib(h[2 * i + 1]);
        if (hi < 0 || lo < 0) return false;
        o[i] = (uint8_t)(hi * 16 + lo);
    }
    return true;
}
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
        int policy = 0, H = 0, agg = 0, n_bits = 0, leaf_first = 0;
        size_t b = 0, first = 0, count = 0;
        in >> policy >> H >> agg >> n_bits >> leaf_first >> b;
        uint64_t* idx = new uint64_t[b];
        for (size_t e = 0; e < b; e++) { unsigned long long x = 0; in >> x; idx[e] = x; }
        std::string hc;
        in >> hc >> first >> count;
        if (!in) { fprintf(stderr, "short case\n"); return 2; }
        std::vector<SubProof> plan;
        SCompactPlan P;
        if (!policy_plan(policy, H, agg, plan) || scompact_plan_build(plan, H, n_bits, leaf_first != 0, P)) { printf("{\"plan\": 0}\n"); delete[] idx; continue; }
        VsPiece* pC = new VsPiece[b * 2 * (size_t)H];
        if (!unhex(hc, b * (size_t)H * 32, (uint8_t*)pC)) { fprintf(stderr, "bad commitment bytes\n"); return 2; }
        const uint32_t n_sub = P.V.n_sub;
        std::vector<uint64_t> sub_off(n_sub + 1), shift(P.shift, P.shift + n_sub);
        uint32_t* ref = new uint32_t[(size_t)n_sub * b];
        const uint64_t len = scompact_layout(P, b, idx, sub_off.data(), ref);
        if (scompact_layout(P, b, idx, nullptr, nullptr) != len) { fprintf(stderr, "layout without outputs\n"); return 2; }
        printf("{\"plan\": 1, \"n_sub\": %u, \"len\": %llu, ", n_sub, (unsigned long long)len);
        put("shift", shift); put("sub_off", sub_off);
        put("ref", std::vector<uint32_t>(ref, ref + (size_t)n_sub * b));
        // the two predicates of the verifier; the kernel's lanes must OR to the whole span
        std::vector<uint32_t> kflag, hflag, hflag16, gref;
        for (uint32_t s = 0; s < n_sub; s++)
            for (size_t e = 0; e < b; e++) {
                const bool key = scompact_key_head(idx, e, P.shift[s]);
                uint32_t d = 0;
                if (e) for (uint32_t lane = 0; lane < 16; lane++) d |= scompact_com_diff(P.V, s, e, pC, lane, 16);
                kflag.push_back(key); hflag.push_back(scompact_is_head(P, s, e, idx, pC)); hflag16.push_back(key || d != 0);
            }
        put("kflag", kflag); put("hflag", hflag); put("hflag16", hflag16);
        // kref as the scan gives it: the row inside the group's slice is the row inside the own list plus the lists before it
        std::vector<uint32_t> kref((size_t)n_sub * b + 1, 0);
        uint32_t acc = 0;
        for (size_t i = 0; i < (size_t)n_sub * b; i++) { acc += kflag[i]; kref[i] = acc; }
        kref[(size_t)n_sub * b] = acc;
        int group_ref_ok = 1;
        for (uint32_t gi = 0; gi < P.V.n_groups && b; gi++) {
            const VSharedGroup& G = P.V.g[gi];
            for (uint32_t s = G.s0; s < G.s0 + G.k; s++)
                for (size_t e = 0; e < b; e++) {
                    const uint64_t at = sub_off[G.s0] + (uint64_t)scompact_group_ref(G, kref.data(), b, s, e) * G.pieces * 16;
                    if (at != sub_off[s] + (uint64_t)ref[(size_t)s * b + e] * G.pieces * 16) group_ref_ok = 0;
                }
        }
        printf("\"group_ref_ok\": %d, ", group_ref_ok);
        // expand / compress over exactly-sized buffers
        const size_t es = (size_t)P.V.entity_pieces * 16;
        uint8_t* compact = new uint8_t[len];
        for (uint64_t i = 0; i < len; i++) compact[i] = pattern(i);
        int window_ok = first <= b && count <= b - first;
        printf("\"window_ok\": %d, \"expand\": \"", window_ok);
        if (window_ok) {
            uint8_t* out = new uint8_t[count * es];
            scompact_expand(P, b, idx, compact, first, count, out);
            for (size_t i = 0; i < count * es; i++) printf("%02x", out[i]);
            delete[] out;
        }
        uint8_t* all = new uint8_t[b * es];
        uint8_t* back = new uint8_t[len];
        memset(back, 0, len);
        scompact_expand(P, b, idx, compact, 0, b, all);
        scompact_compress(P, b, idx, all, back);
        printf("\", \"round_trip\": %d}\n", (int)(memcmp(back, compact, len) == 0));
        delete[] all; delete[] back; delete[] compact; delete[] ref; delete[] pC; delete[] idx;
    }
    return 0;
}

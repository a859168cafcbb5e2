// Host-only build of the index arithmetic of dapol_verify_entities_shared (dapol_amd/csrc/verify_shared_plan.inc): reads one case per
// line from stdin and prints what the library computes for it as one line of JSON.  Build + run: tests/test_verify_shared_cpu.py,
// under ASan + UBSan.  A case (numbers in decimal, bytes in hex without separators):
//   policy H agg n_bits b blobs[b * entity bytes] commitments[b * H * 32] n_heads_max verdicts[n_heads_max]
// or, without rows,   limits policy H agg n_bits b   -> the call-size predicates alone (b may be anything up to 2^64 - 1).
// The rows go into heap buffers of exactly their size, so that a read outside a span is a sanitizer error.  Output: the spans
// (q0, pieces, start, count), the groups, flag[s][e] (+ the closing zero), the inclusive scan, the layout of the compact buffers, what
// every lane of the gather would copy (as a checksum-free list of (row, piece, source)) and the expansion of the given verdicts.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/dapol_hip.h"
#include "verify_shared_plan.inc"

static bool unhex(const std::string& h, size_t bytes, VsPiece* out) {
    if (h.size() != 2 * bytes && !(bytes == 0 && h == "-")) return false;
    uint8_t* o = (uint8_t*)out;
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
        if (line.rfind("limits ", 0) == 0) {
            std::string word;
            int policy = 0, H = 0, agg = 0, n_bits = 0;
            unsigned long long b = 0;
            in >> word >> policy >> H >> agg >> n_bits >> b;
            std::vector<SubProof> plan;
            VSharedPlan P;
            if (!in || !policy_plan(policy, H, agg, plan) || vshared_plan_build(plan, H, n_bits, P)) { fprintf(stderr, "bad limits case\n"); return 2; }
            printf("{\"n_sub\": %u, \"fits\": %d, \"gather_fits\": %d, \"forwards\": %d}\n", P.n_sub, (int)vshared_call_fits((size_t)b, P.n_sub),
                   (int)vshared_gather_fits(P, (size_t)b), (int)vshared_forwards((size_t)b, P.n_sub, VSHARED_FORWARD_MAX));
            continue;
        }
        int policy = 0, H = 0, agg = 0, n_bits = 0;
        size_t b = 0, n_heads_max = 0;
        std::string hb, hc;
        in >> policy >> H >> agg >> n_bits >> b >> hb >> hc >> n_heads_max;
        std::vector<uint8_t> verdicts(n_heads_max);
        for (auto& x : verdicts) { unsigned v = 0; in >> v; x = (uint8_t)v; }
        if (!in) { fprintf(stderr, "short case\n"); return 2; }
        std::vector<SubProof> plan;
        if (!policy_plan(policy, H, agg, plan)) { printf("{\"plan\": 0}\n"); continue; }
        VSharedPlan P;
        const int rc = vshared_plan_build(plan, H, n_bits, P);
        if (rc) { printf("{\"plan\": 0, \"rc\": %d}\n", rc); continue; }
        // exactly-sized heap copies of the rows (new[]: 16-byte aligned)
        VsPiece* blobs = new VsPiece[b * (size_t)P.entity_pieces];
        VsPiece* pC = new VsPiece[b * 2 * (size_t)H + (H == 0 || b == 0 ? 1 : 0)];
        if (!unhex(hb, b * (size_t)P.entity_pieces * 16, blobs) || !unhex(hc, b * (size_t)H * 32, pC)) { fprintf(stderr, "bad row bytes\n"); return 2; }
        std::vector<uint32_t> q0, pieces, start, count, span, gs0, gk, gm, gp, gq0;
        for (uint32_t s = 0; s < P.n_sub; s++) {
            q0.push_back(P.q0[s]); pieces.push_back(P.pieces[s]); start.push_back(P.start[s]); count.push_back(P.count[s]);
            span.push_back(vshared_span_pieces(P, s));
        }
        for (uint32_t g = 0; g < P.n_groups; g++) {
            gs0.push_back(P.g[g].s0); gk.push_back(P.g[g].k); gm.push_back(P.g[g].m); gp.push_back(P.g[g].pieces); gq0.push_back(P.g[g].q0);
        }
        printf("{\"plan\": 1, \"n_sub\": %u, \"entity_pieces\": %u, \"fits\": %d, \"forwards\": %d, ", P.n_sub, P.entity_pieces, (int)vshared_call_fits(b, P.n_sub),
               (int)vshared_forwards(b, P.n_sub, VSHARED_FORWARD_MAX));
        put("q0", q0); put("pieces", pieces); put("start", start); put("count", count); put("span", span);
        put("g_s0", gs0); put("g_k", gk); put("g_m", gm); put("g_pieces", gp); put("g_q0", gq0);
        // flags as k_vshared_heads defines them, the scan as rocprim's inclusive_scan
        const size_t nf = (size_t)P.n_sub * b + 1;
        std::vector<uint32_t> flag(nf, 0), rank(nf, 0);
        for (uint32_t s = 0; s < P.n_sub; s++)
            for (size_t e = 0; e < b; e++) flag[(size_t)s * b + e] = vshared_is_head(P, s, e, blobs, pC) ? 1 : 0;
        uint32_t acc = 0;
        for (size_t i = 0; i < nf; i++) { acc += flag[i]; rank[i] = acc; }
        put("flag", flag); put("rank", rank);
        if (b == 0) { printf("\"b\": 0}\n"); delete[] blobs; delete[] pC; continue; }
        std::vector<uint32_t> rank_at(P.n_groups + 1);
        for (uint32_t g = 0; g < P.n_groups; g++) rank_at[g] = rank[(size_t)P.g[g].s0 * b];
        rank_at[P.n_groups] = rank[nf - 1];
        VSharedLayout L;
        vshared_layout(P, rank_at.data(), L);
        std::vector<size_t> first(L.first, L.first + P.n_groups + 1), poff(L.piece_off, L.piece_off + P.n_groups), voff(L.party_off, L.party_off + P.n_groups);
        put("first", first); put("piece_off", poff); put("party_off", voff);
        printf("\"pieces_total\": %zu, \"parties_total\": %zu, ", L.pieces, L.parties);
        // the gather, lane by lane: (group, compact row, piece of the span, s, e) of every lane that copies
        std::vector<size_t> gather;
        for (uint32_t g = 0; g < P.n_groups; g++) {
            VsGatherLane ln;
            size_t t = 0;
            for (; vshared_gather_lane(P.g[g], b, t, ln); t++) {
                if (!flag[(size_t)ln.s * b + ln.e]) continue;
                gather.push_back(g); gather.push_back(vshared_group_row(P.g[g], rank.data(), b, ln.s, ln.e)); gather.push_back(ln.piece);
                gather.push_back(ln.s); gather.push_back(ln.e);
            }
            if (t != b * (size_t)P.g[g].k * vshared_gather_pieces(P.g[g])) { fprintf(stderr, "gather lanes\n"); return 2; }
        }
        put("gather", gather);
        std::vector<uint32_t> ok(b, 0), row;
        if (n_heads_max >= rank[nf - 1])
            for (size_t e = 0; e < b; e++) ok[e] = vshared_verdict(P, b, rank.data(), verdicts.data(), e);
        for (uint32_t s = 0; s < P.n_sub; s++)
            for (size_t e = 0; e < b; e++) row.push_back((uint32_t)vshared_row(rank.data(), b, s, e));
        put("row", row); put("ok", ok, "}\n");
        delete[] blobs;
        delete[] pC;
    }
    return 0;
}

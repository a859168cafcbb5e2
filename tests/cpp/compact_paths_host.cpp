// Host-only build of the index arithmetic of compact Merkle paths (dapol_amd/csrc/compact_paths_plan.inc): reads one case per line
// from stdin and prints what the library computes for it as one line of JSON.  Build + run: tests/test_compact_paths_cpu.py, under
// ASan + UBSan.  A case (numbers in decimal):
//   H leaf_first hash_bytes b idx[b] first count d_records d_cap
// d_records / d_cap are added to the true record count before it is passed as n_records to expand / as cap_records to compress, so a
// case can ask for a refusal.  Output: the plan (depth_off, ref, n_records, the kernels' link words); the expansion of rows
// [first, first + count) of a compact buffer whose bytes are pattern(i) (C) and pattern(i + 7777) (H); whether compress(expand(all
// rows)) gives the buffer back, also when every slot that compress must not read is poisoned; and for every refusal whether the
// outputs were left untouched.  Every buffer lives on the heap with exactly its size, so that a read or write outside it is a
// sanitizer error.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "compact_paths_plan.inc"

static uint8_t pattern(uint64_t i) { return (uint8_t)(i * 131 + (i >> 8) * 7 + (i >> 16) + 3); }
template <typename V>
static void put(const char* key, const V& v, const char* end = ", ") {
    printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); i++) printf("%s%llu", i ? ", " : "", (unsigned long long)v[i]);
    printf("]%s", end);
}
static bool all_are(const uint8_t* p, size_t n, uint8_t v) {
    for (size_t i = 0; i < n; i++) if (p[i] != v) return false;
    return true;
}
static void hex(const char* key, const uint8_t* p, size_t n) {
    printf("\"%s\": \"", key);
    for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
    printf("\", ");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int H = 0, leaf_first = 0, hash_bytes = 0;
        long long d_records = 0, d_cap = 0;
        size_t b = 0, first = 0, count = 0;
        in >> H >> leaf_first >> hash_bytes >> b;
        uint64_t* idx = new uint64_t[b];
        for (size_t e = 0; e < b; e++) { unsigned long long x = 0; in >> x; idx[e] = x; }
        in >> first >> count >> d_records >> d_cap;
        if (!in) { fprintf(stderr, "short case\n"); return 2; }
        const size_t hb = (size_t)hash_bytes;
        const bool shape_ok = H >= 1 && H <= 64;
        const size_t Hs = shape_ok ? (size_t)H : 1;

        // ---- the plan; a refusal leaves its three outputs alone
        uint64_t* depth_off = new uint64_t[Hs + 2];
        uint32_t* ref = new uint32_t[Hs * b];
        memset(depth_off, 0xA5, (Hs + 2) * 8); memset(ref, 0xA5, Hs * b * 4);
        uint64_t n = 0xA5A5A5A5A5A5A5A5ull;
        const int rc = cpaths_plan_checked(H, b, idx, depth_off, ref, &n);
        printf("{\"rc\": %d, ", rc);
        if (rc) {
            const int untouched = all_are((const uint8_t*)depth_off, (Hs + 2) * 8, 0xA5) && all_are((const uint8_t*)ref, Hs * b * 4, 0xA5) && n == 0xA5A5A5A5A5A5A5A5ull;
            // expand and compress refuse the same indexes, and write nothing
            uint8_t* o = new uint8_t[64];
            memset(o, 0xA5, 64);
            uint64_t nn = 7;
            const int rx = cpaths_expand_checked(hash_bytes, H, b, idx, o, o, 0, 0, 0, leaf_first != 0, o, o);
            const int rz = cpaths_compress_checked(hash_bytes, H, b, idx, o, o, leaf_first != 0, o, o, ~0ull, &nn);
            printf("\"untouched\": %d, \"expand_rc\": %d, \"compress_rc\": %d}\n", untouched && all_are(o, 64, 0xA5) && nn == 7, rx, rz);
            delete[] o; delete[] depth_off; delete[] ref; delete[] idx;
            continue;
        }
        uint64_t n2 = 0;
        if (cpaths_plan_checked(H, b, idx, nullptr, nullptr, &n2) || n2 != n || cpaths_plan_checked(H, b, idx, nullptr, nullptr, nullptr)) {
            fprintf(stderr, "plan without outputs\n");
            return 2;
        }
        printf("\"n_records\": %llu, ", (unsigned long long)n);
        put("depth_off", std::vector<uint64_t>(depth_off, depth_off + H + 2));
        put("ref", std::vector<uint32_t>(ref, ref + (size_t)H * b));
        uint32_t* link = new uint32_t[n];
        cpaths_links(H, b, idx, depth_off, link);
        put("link", std::vector<uint32_t>(link, link + n));
        printf("\"links_fit\": %d, ", (int)cpaths_links_fit(b, n));

        // ---- expand over exactly-sized buffers
        uint8_t* cC = new uint8_t[n * 32];
        uint8_t* cH = new uint8_t[n * hb];
        for (uint64_t i = 0; i < n * 32; i++) cC[i] = pattern(i);
        for (uint64_t i = 0; i < n * hb; i++) cH[i] = pattern(i + 7777);
        const bool window_ok = first <= b && count <= b - first;
        const size_t rows = window_ok ? count : 0;
        uint8_t* oC = new uint8_t[rows * H * 32];
        uint8_t* oH = new uint8_t[rows * H * hb];
        memset(oC, 0xA5, rows * H * 32); memset(oH, 0xA5, rows * H * hb);
        const int rx = cpaths_expand_checked(hash_bytes, H, b, idx, cC, cH, (uint64_t)((long long)n + d_records), first, count, leaf_first != 0, oC, oH);
        printf("\"expand_rc\": %d, ", rx);
        if (rx) printf("\"expand_untouched\": %d, ", (int)(all_are(oC, rows * H * 32, 0xA5) && all_are(oH, rows * H * hb, 0xA5)));
        else { hex("expand_C", oC, rows * H * 32); hex("expand_H", oH, rows * H * hb); }

        // ---- compress: the inverse, and it reads the first row of every run only
        int round_trip = -1, poisoned = -1, compress_untouched = -1, rz = -1;
        if (hash_bytes == 32 || hash_bytes == 64) {
            uint8_t* aC = new uint8_t[b * H * 32];
            uint8_t* aH = new uint8_t[b * H * hb];
            if (cpaths_expand_checked(hash_bytes, H, b, idx, cC, cH, n, 0, b, leaf_first != 0, aC, aH)) { fprintf(stderr, "expand of all rows\n"); return 2; }
            const uint64_t cap = (uint64_t)((long long)n + d_cap);
            const uint64_t held = d_cap < 0 ? cap : n;              // (a refused call gets buffers of the capacity it names)
            uint8_t* bC = new uint8_t[held * 32];
            uint8_t* bH = new uint8_t[held * hb];
            memset(bC, 0xA5, held * 32); memset(bH, 0xA5, held * hb);
            uint64_t nn = 7;
            rz = cpaths_compress_checked(hash_bytes, H, b, idx, aC, aH, leaf_first != 0, bC, bH, cap, &nn);
            if (rz) compress_untouched = all_are(bC, held * 32, 0xA5) && all_are(bH, held * hb, 0xA5) && nn == 7;
            else {
                round_trip = nn == n && !memcmp(bC, cC, n * 32) && !memcmp(bH, cH, n * hb);
                for (size_t e = 0; e < b; e++)
                    for (int d = 1; d <= H; d++)
                        if (!cpaths_is_head(H, idx, e, d)) {
                            const size_t slot = e * (size_t)H + (size_t)cpaths_slot(H, d, leaf_first != 0);
                            memset(aC + slot * 32, 0xEE, 32); memset(aH + slot * hb, 0xEE, hb);
                        }
                memset(bC, 0, n * 32); memset(bH, 0, n * hb);
                poisoned = !cpaths_compress_checked(hash_bytes, H, b, idx, aC, aH, leaf_first != 0, bC, bH, cap, nullptr) && !memcmp(bC, cC, n * 32) &&
                           !memcmp(bH, cH, n * hb);
            }
            delete[] aC; delete[] aH; delete[] bC; delete[] bH;
        } else {
            uint8_t* o = new uint8_t[64];
            memset(o, 0xA5, 64);
            rz = cpaths_compress_checked(hash_bytes, H, b, idx, o, o, leaf_first != 0, o, o, ~0ull, nullptr);
            compress_untouched = all_are(o, 64, 0xA5);
            delete[] o;
        }
        printf("\"compress_rc\": %d, \"compress_untouched\": %d, \"round_trip\": %d, \"round_trip_poisoned\": %d}\n", rz, compress_untouched, round_trip, poisoned);
        delete[] oC; delete[] oH; delete[] cC; delete[] cH; delete[] link; delete[] depth_off; delete[] ref; delete[] idx;
    }
    return 0;
}

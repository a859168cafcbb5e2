// COMPACT MERKLE PATHS as index arithmetic: every distinct sibling of a call's paths once (definition in include/dapol_hip.h, "COMPACT
// Merkle paths").  For strictly increasing leaf indexes below 2^H, key_d(e) = idx[e] >> (H - d) (key_0 = 0), row e is a HEAD at depth d
// iff e = 0 or key_d(e) != key_d(e - 1), and the compact buffer holds, for d = 1 .. H (root side first, whatever the sibling order of
// the expanded form), the siblings of the distinct keys of depth d in ascending key order: record depth_off[d] + ref[d][e] is the
// sibling of row e at depth d.  Heads are monotone in d, so all of it follows from ONE number per row: the shallowest depth at which
// the row is a head.
// Pure functions, no HIP call and no context: the host entry points and the launchers (host_compact_paths.inc), the kernels
// (kernels_compact_paths.h) and tests/cpp/compact_paths_host.cpp (ASan + UBSan, tests/test_compact_paths_cpu.py) call them.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define CPP_HD __host__ __device__ __forceinline__
#else
#define CPP_HD inline
#endif

enum { CPATHS_MAX_H = 64 };
// What the checked functions below answer (0: done; anything else: refused, nothing written).
enum { CPATHS_OK = 0, CPATHS_BAD_HEIGHT, CPATHS_BAD_INDEX, CPATHS_BAD_HASH, CPATHS_BAD_RECORDS, CPATHS_BAD_WINDOW, CPATHS_BAD_CAP, CPATHS_NULL, CPATHS_TOO_MANY };
static inline const char* cpaths_strerror(int rc) {
    switch (rc) {
        case CPATHS_BAD_HEIGHT: return "height must lie in [1, 64]";
        case CPATHS_BAD_INDEX: return "leaf indexes must be strictly increasing and below 2^height";
        case CPATHS_BAD_HASH: return "hash_bytes must be 32 or 64";
        case CPATHS_BAD_RECORDS: return "n_records is not the record count of the compact layout of these leaves";
        case CPATHS_BAD_WINDOW: return "first + count exceeds the rows";
        case CPATHS_BAD_CAP: return "cap_records is below the record count of the compact layout";
        case CPATHS_NULL: return "null argument";
        case CPATHS_TOO_MANY: return "too many rows or records in one call (both must stay below 2^30 and 2^32)";
        default: return "ok";
    }
}

// The key of a leaf index at depth d of a tree of height H (d = 0: the root's, never a shift by 64).
CPP_HD uint64_t cpaths_key(uint64_t idx, int H, int d) { return d == 0 ? 0ull : idx >> (H - d); }
// The shallowest depth at which row e is a head: 0 for row 0, else j + 1 where j is the deepest depth at which rows e and e - 1 share
// their key.  (idx[e] != idx[e - 1], both below 2^H: the result lies in [1, H].)
CPP_HD int cpaths_first_head(int H, const uint64_t* idx, size_t e) {
    if (e == 0) return 0;
    uint64_t x = idx[e] ^ idx[e - 1];
    int bits = 0;
    while (x) { bits++; x >>= 1; }
    return H - bits + 1;
}
CPP_HD bool cpaths_is_head(int H, const uint64_t* idx, size_t e, int d) { return e == 0 || cpaths_key(idx[e], H, d) != cpaths_key(idx[e - 1], H, d); }
// The slot of the sibling of depth d inside a row of the expanded [b][H] form under the call's sibling order.
CPP_HD int cpaths_slot(int H, int d, bool leaf_first) { return leaf_first ? H - d : d - 1; }

static inline int cpaths_check(int H, size_t b, const uint64_t* idx) {
    if (H < 1 || H > CPATHS_MAX_H) return CPATHS_BAD_HEIGHT;
    if (b && !idx) return CPATHS_NULL;
    for (size_t e = 1; e < b; e++) if (idx[e] <= idx[e - 1]) return CPATHS_BAD_INDEX;
    if (b && H < 64 && (idx[b - 1] >> H) != 0) return CPATHS_BAD_INDEX;
    return CPATHS_OK;
}

// The layout of checked indexes: depth_off[0 .. H + 1] (depth_off[0] = depth_off[1] = 0, depth_off[H + 1] = the record count, which
// is also returned) and ref[(d - 1) * b + e] for d = 1 .. H.  Both may be null.
static inline uint64_t cpaths_layout(int H, size_t b, const uint64_t* idx, uint64_t* depth_off, uint32_t* ref) {
    uint64_t cnt[CPATHS_MAX_H + 1] = {0};                      // cnt[d]: heads of depth d among the rows seen so far
    for (size_t e = 0; e < b; e++) {
        const int f = cpaths_first_head(H, idx, e);
        if (ref) {
            for (int d = 1; d <= H; d++) {
                if (d >= f) cnt[d]++;
                ref[(size_t)(d - 1) * b + e] = (uint32_t)(cnt[d] - 1);
            }
        } else cnt[f ? f : 1]++;                                 // (a histogram of f: the prefix sums below are the counts)
    }
    if (!ref) for (int d = 2; d <= H; d++) cnt[d] += cnt[d - 1];
    uint64_t at = 0;
    if (depth_off) depth_off[0] = 0;
    for (int d = 1; d <= H; d++) {
        if (depth_off) depth_off[d] = at;
        at += cnt[d];
    }
    if (depth_off) depth_off[H + 1] = at;
    return at;
}

// dapol_compact_paths_plan
static inline int cpaths_plan_checked(int H, size_t b, const uint64_t* idx, uint64_t* depth_off, uint32_t* ref, uint64_t* n_records) {
    const int rc = cpaths_check(H, b, idx);
    if (rc) return rc;
    if (ref && (uint64_t)b >= (1ull << 32)) return CPATHS_TOO_MANY;
    const uint64_t n = cpaths_layout(H, b, idx, depth_off, ref);
    if (n_records) *n_records = n;
    return CPATHS_OK;
}

// dapol_compact_paths_expand: rows [first, first + count) as [count][H] records under the sibling order leaf_first.
static inline int cpaths_expand_checked(int hash_bytes, int H, size_t b, const uint64_t* idx, const uint8_t* cC, const uint8_t* cH, uint64_t n_records,
                                        size_t first, size_t count, bool leaf_first, uint8_t* outC, uint8_t* outH) {
    if (hash_bytes != 32 && hash_bytes != 64) return CPATHS_BAD_HASH;
    const int rc = cpaths_check(H, b, idx);
    if (rc) return rc;
    if (first > b || count > b - first) return CPATHS_BAD_WINDOW;
    uint64_t off[CPATHS_MAX_H + 2];
    if (cpaths_layout(H, b, idx, off, nullptr) != n_records) return CPATHS_BAD_RECORDS;
    if (count && (!cC || !cH || !outC || !outH)) return CPATHS_NULL;
    const size_t hb = (size_t)hash_bytes;
    uint64_t cnt[CPATHS_MAX_H + 1] = {0};
    for (size_t e = 0; e < first + count; e++) {
        const int f = cpaths_first_head(H, idx, e);
        for (int d = f ? f : 1; d <= H; d++) cnt[d]++;
        if (e < first) continue;
        for (int d = 1; d <= H; d++) {
            const uint64_t rec = off[d] + cnt[d] - 1;
            const size_t slot = (e - first) * (size_t)H + (size_t)cpaths_slot(H, d, leaf_first);
            memcpy(outC + slot * 32, cC + rec * 32, 32);
            memcpy(outH + slot * hb, cH + rec * hb, hb);
        }
    }
    return CPATHS_OK;
}

// dapol_compact_paths_compress: the first row of every run is written, the other rows are not read.
static inline int cpaths_compress_checked(int hash_bytes, int H, size_t b, const uint64_t* idx, const uint8_t* pC, const uint8_t* pH, bool leaf_first,
                                          uint8_t* cC, uint8_t* cH, uint64_t cap_records, uint64_t* n_records) {
    if (hash_bytes != 32 && hash_bytes != 64) return CPATHS_BAD_HASH;
    const int rc = cpaths_check(H, b, idx);
    if (rc) return rc;
    uint64_t off[CPATHS_MAX_H + 2];
    const uint64_t n = cpaths_layout(H, b, idx, off, nullptr);
    if (n > cap_records) return CPATHS_BAD_CAP;
    if (b && (!pC || !pH || !cC || !cH)) return CPATHS_NULL;
    const size_t hb = (size_t)hash_bytes;
    uint64_t cnt[CPATHS_MAX_H + 1] = {0};
    for (size_t e = 0; e < b; e++) {
        const int f = cpaths_first_head(H, idx, e);
        for (int d = f ? f : 1; d <= H; d++) {
            const uint64_t rec = off[d] + cnt[d]++;
            const size_t slot = e * (size_t)H + (size_t)cpaths_slot(H, d, leaf_first);
            memcpy(cC + rec * 32, pC + slot * 32, 32);
            memcpy(cH + rec * hb, pH + slot * hb, hb);
        }
    }
    if (n_records) *n_records = n;
    return CPATHS_OK;
}

// ------------------------------------------------------------------------------------------------ what the kernels walk
// One LINK word per record = per distinct node (d, key), d = 1 .. H, at depth_off[d] + i: the index, among the nodes of depth d - 1, of
// the node that it lies under (depth 0 has the one node 0), CPATHS_RIGHT if the node is a right child (so its sibling, the record, is
// the left input of the merge), and CPATHS_JOIN if the head row of the node is NOT the head row of that parent -- the node's chain
// ends there, in a comparison with the parent's value that another chain has made.  A kernel that starts at a row's leaf (depth H,
// index = the row) and follows the links visits the records of the row's path; one that stops at the first join visits exactly the
// records that the row is the head of.
enum : uint32_t { CPATHS_JOIN = 0x80000000u, CPATHS_RIGHT = 0x40000000u, CPATHS_INDEX = 0x3fffffffu };
struct CPathsDev {
    uint32_t H;
    uint64_t depth_off[CPATHS_MAX_H + 2];
};
static inline bool cpaths_links_fit(size_t b, uint64_t n_records) { return (uint64_t)b < (1ull << 30) && n_records < (1ull << 32) - 1; }
// link: [n_records].  depth_off: cpaths_layout's over the same checked indexes.
static inline void cpaths_links(int H, size_t b, const uint64_t* idx, const uint64_t* depth_off, uint32_t* link) {
    uint64_t cnt[CPATHS_MAX_H + 1] = {0};
    cnt[0] = 1;
    for (size_t e = 0; e < b; e++) {
        const int f = cpaths_first_head(H, idx, e);
        for (int d = f ? f : 1; d <= H; d++) {
            const uint64_t i = cnt[d]++;
            // cnt[d - 1] - 1: the node of depth d - 1 that row e lies under -- its own if the row is a head there (just counted), else the last one
            uint32_t w = (uint32_t)(cnt[d - 1] - 1);
            if ((idx[e] >> (H - d)) & 1ull) w |= CPATHS_RIGHT;
            if (d - 1 < f) w |= CPATHS_JOIN;
            link[depth_off[d] + i] = w;
        }
    }
}
